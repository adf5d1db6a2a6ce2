"""Mean shifts on edges, host side (no GPU): the statements the GPU tests of test_gpu_shifts.py lean on, pinned to the
untouched oracle on the eight cases of test_gradient_cpu (_case, _more_cases), three shifted edges, one of them a hybrid edge.

(a) three ways to the shifted log-likelihood agree: densemvn.loglik of the wrapper (shift_ref.ShiftedModel), densemvn.loglik
    of the plain model on the tip data minus sum gamma_k tau s_k (edge_ref.shift_transfer), and the oracle's belief
    propagation of the wrapper on the clique tree;
(b) posterior node means of the wrapper = those of the plain model on the shifted data plus the offset; equal covariances;
(c) shift_ref.family_statement against Richardson central differences (1e-3, 5e-4) of the wrapper's dense log-likelihood;
(d) the fit: the quadratic model the driver solves (score at 0, information matrix) against dense GLS, cond(H) <= 100.
Everything at 1e-8 relative to the largest entry of the block; the measured figures are printed."""
import numpy as np
import pytest

from edge_ref import rel_block_nan, shift_transfer
from helpers import oracle_setup
from oracle import calibration as OC
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle.beliefupdates import BPPosDefException
from shift_ref import ShiftedModel, dense_statement, fit_edges, gls_fit
from test_gradient_cpu import _case, _more_cases, model_params, model_with, rel_block, richardson

TOL = 1e-8


def cases():
    for which in ("bm", "ou"):
        yield (f"{which}_random_root",) + _case(which)
    yield from _more_cases()


CASES = list(cases())
IDS = [c[0] for c in CASES]


def shifted_edges(net, model):
    """Three edges: two tree edges into internal nodes and a hybrid edge."""
    e = fit_edges(net, model)
    assert len(e) == 4 and e[3].hybrid
    return [e[0], e[2], e[3]]


def shifts_of(net, model, seed=3):
    rng = np.random.default_rng(seed)
    return {ed.number: rng.normal(size=model.dimension()) for ed in shifted_edges(net, model)}


def moved_data(net, model, shifts, tbl, taxa):
    """The tip data minus sum over the shifted edges of gamma tau s, and the offset of every node [N, p]."""
    pre = net.vec_node
    pos = {id(n): i for i, n in enumerate(pre)}
    p = model.dimension()
    off = np.zeros((len(pre), p))
    for ed in net.edges:
        if ed.number in shifts:
            off += ed.gamma * np.outer(shift_transfer(net, model, pos[id(ed.child)]), shifts[ed.number])
    moved = [list(col) for col in tbl]
    for i, n in enumerate(pre):
        if n.leaf:
            r = list(taxa).index(n.name)
            for t in range(p):
                if moved[t][r] is not None:
                    moved[t][r] = moved[t][r] - off[i, t]
    return moved, off


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_three_ways_to_the_shifted_likelihood(case):
    name, net, model, tbl, taxa = case
    shifts = shifts_of(net, model)
    wrapper = ShiftedModel(model, shifts)
    dense = OD.loglik(net, wrapper, tbl, taxa)
    moved, _ = moved_data(net, model, shifts, tbl, taxa)
    plain = OD.loglik(net, model, moved, taxa)
    # the factor handed to belief propagation = the generic factor of branch_qwv, family by family
    worst = 0.0
    for n in net.vec_node[1:]:
        pae = net.parent_edges(n)
        mine = wrapper.factor_treeedge(pae[0]) if len(pae) == 1 else wrapper.factor_hybridnode(pae)
        for a, b in zip(mine, wrapper.generic_factor(pae)):
            worst = max(worst, rel_block(np.atleast_1d(a), np.atleast_1d(b)) if np.any(b) else float(np.max(np.abs(a))))
    print(f"{name}: wrapper's factors vs the generic factors of branch_qwv {worst:.2e}")
    assert worst <= 1e-12
    cg = OCG.cliquetree(net)
    try:
        ocgb = oracle_setup(net, cg, wrapper, tbl, taxa)
    except BPPosDefException:
        # the two missing-data cases: the oracle's own assignfactors raises on this network's pattern for the PLAIN model
        # already (marginalize meets a block of rounding noise where it tests for exact zeros): no BP statement to compare
        with pytest.raises(BPPosDefException):
            oracle_setup(net, cg, model, tbl, taxa)
        assert name.startswith("missing") and abs(dense - plain) <= TOL * abs(dense)
        return
    root = OCG.default_rootcluster(cg, net)
    spt = OCG.spanningtree_clusterlist(cg, root)
    assert OC.calibrate(ocgb, [spt], verbose=False)[0]
    bp = ocgb.integratebelief(root)[1]
    e1, e2 = abs(dense - plain) / abs(dense), abs(bp - dense) / abs(dense)
    print(f"{name}: dense wrapper vs plain on moved data {e1:.2e}, BP vs dense {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    assert abs(dense - OD.loglik(net, model, tbl, taxa)) > 1e-3   # (the shifts do something)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_posterior_means_move_by_the_offset(case):
    name, net, model, tbl, taxa = case
    shifts = shifts_of(net, model)
    pm, pc = OD.posterior_node_moments(net, ShiftedModel(model, shifts), tbl, taxa)
    moved, off = moved_data(net, model, shifts, tbl, taxa)
    pm0, pc0 = OD.posterior_node_moments(net, model, moved, taxa)
    e1, e2 = rel_block(pm, pm0 + off.reshape(-1)), rel_block(pc, pc0)
    print(f"{name}: means {e1:.2e}, covariances {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_family_statement_against_finite_differences(case):
    """dR, dmu, dalpha, dtheta, dlength, dgamma (with its new term s_k' g_w) and gamma_k * dshift (against the difference in
    s_k itself), each block against Richardson differences of densemvn.loglik of the wrapper."""
    name, net, model, tbl, taxa = case
    shifts = shifts_of(net, model)
    p = model.dimension()
    st = dense_statement(net, model, shifts, tbl, taxa)
    rates, root_color, mu, alpha, theta = model_params(model)

    def ll(rates_=rates, mu_=mu, alpha_=alpha, theta_=theta, shifts_=shifts):
        return OD.loglik(net, ShiftedModel(model_with(model, rates_, mu_, alpha_, theta_), shifts_), tbl, taxa)
    h = 1e-3
    want = dict(dR=np.zeros_like(st["dR"]), dmu=np.zeros(p), dalpha=0.0, dtheta=np.zeros(p))
    for c in range(len(rates)):
        for a in range(p):
            for b in range(a, p):
                E = np.zeros((p, p)); E[a, b] += 0.5; E[b, a] += 0.5
                f = lambda s, c=c, E=E: ll(rates_=[r + (s * E if q == c else 0) for q, r in enumerate(rates)])
                want["dR"][c, a, b] = want["dR"][c, b, a] = richardson(f, h)
    for a in range(p):
        want["dmu"][a] = richardson(lambda s, a=a: ll(mu_=mu + s * np.eye(p)[a]), h)
    if alpha is not None:
        want["dalpha"] = richardson(lambda s: ll(alpha_=alpha + s), h)
        want["dtheta"] = np.array([richardson(lambda s: ll(theta_=theta + s), h)])
    worst = 0.0
    for k in ("dR", "dmu", "dalpha", "dtheta"):
        if not np.any(np.atleast_1d(want[k])) and not np.any(np.atleast_1d(st[k])):
            continue
        err = rel_block(st[k], want[k])
        worst = max(worst, err)
        print(f"{name} {k}: {err:.2e}")
        assert err <= TOL, (name, k, st[k], want[k])
    # per edge
    N, K = st["dlength"].shape
    fd = dict(dlength=np.full((N, K), np.nan), dgamma=np.full((N, K), np.nan), gshift=np.full((N, K, p), np.nan))
    got_gshift = np.full((N, K, p), np.nan)
    for i in range(1, N):
        for k, ed in enumerate(st["edges"][i]):
            for attr, key in (("length", "dlength"), ("gamma", "dgamma")):
                keep = getattr(ed, attr)

                def f(s, ed=ed, attr=attr, keep=keep):
                    setattr(ed, attr, keep * (1.0 + s))
                    try:
                        return ll()
                    finally:
                        setattr(ed, attr, keep)
                fd[key][i, k] = richardson(f, h) / keep
            if ed.number in shifts or i % 5 == 0:   # the shifted edges, and a fifth of the others (their shift is 0)
                for t in range(p):
                    def f(s, ed=ed, t=t):
                        sh = dict(shifts)
                        sh[ed.number] = np.asarray(sh.get(ed.number, np.zeros(p)), float) + s * np.eye(p)[t]
                        return ll(shifts_=sh)
                    fd["gshift"][i, k, t] = richardson(f, h)
                got_gshift[i, k] = ed.gamma * st["dshift"][i]
    for key, got in (("dlength", st["dlength"]), ("dgamma", st["dgamma"]), ("gshift", got_gshift)):
        err = rel_block_nan(got, fd[key])
        worst = max(worst, err)
        print(f"{name} {key}: {err:.2e}")
        assert err <= TOL, (name, key)
    # the new term is needed: without it dgamma of a shifted hybrid edge is off
    hyb = next(ed for ed in net.edges if ed.number in shifts and ed.hybrid)
    i = next(j for j, n in enumerate(net.vec_node) if n is hyb.child)
    k = next(q for q, e2 in enumerate(st["edges"][i]) if e2 is hyb)
    assert abs(float(shifts[hyb.number] @ st["dshift"][i])) > 1e-6 * abs(st["dgamma"][i, k])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fit_is_dense_gls(case):
    """The quadratic model fit_shifts_lg solves -- g(0) and H from n p + 1 evaluations of the score with unit steps, here on
    the dense statement -- gives the dense GLS estimate, its information matrix and its log-likelihood."""
    name, net, model, tbl, taxa = case
    edges = fit_edges(net, model)
    p = model.dimension()
    n = len(edges)
    shat_d, H_d, ll_d = gls_fit(net, model, tbl, taxa, edges)
    cond = np.linalg.cond(H_d)
    print(f"{name}: cond(H) = {cond:.2f}")
    assert cond <= 100.0
    pos = {id(nd): i for i, nd in enumerate(net.vec_node)}

    def score(values):
        sh = {ed.number: values[a] for a, ed in enumerate(edges)}
        st = dense_statement(net, model, sh, tbl, taxa)
        return np.concatenate([ed.gamma * st["dshift"][pos[id(ed.child)]] for ed in edges])
    g0 = score(np.zeros((n, p)))
    H = np.zeros((n * p, n * p))
    for j in range(n * p):
        unit = np.zeros(n * p); unit[j] = 1.0
        H[:, j] = g0 - score(unit.reshape(n, p))
    H = (H + H.T) / 2
    shat = np.linalg.solve(H, g0).reshape(n, p)
    e1, e2 = rel_block(shat, shat_d), rel_block(H, H_d)
    ll = OD.loglik(net, ShiftedModel(model, {ed.number: s for ed, s in zip(edges, shat)}), tbl, taxa)
    g1 = score(shat)
    print(f"{name}: shat {e1:.2e}, H {e2:.2e}, loglik {abs(ll - ll_d) / abs(ll_d):.2e}, score at shat / at 0 "
          f"{np.max(np.abs(g1)) / np.max(np.abs(g0)):.2e}")
    assert e1 <= TOL and e2 <= TOL and abs(ll - ll_d) <= TOL * abs(ll_d)
    assert np.max(np.abs(g1)) <= TOL * np.max(np.abs(g0))
    assert ll_d > OD.loglik(net, model, tbl, taxa)


def test_cholesky_names_the_failing_pivot():
    from pgbp_amd.optimize import _cholesky_or_name
    H = np.array([[2.0, 1.0, 2.0, 1.0], [1.0, 3.0, 1.0, 3.0], [2.0, 1.0, 2.0, 1.0], [1.0, 3.0, 1.0, 3.0]])   # two equal shifts
    with pytest.raises(ValueError, match=r"family 3, parent 1\), trait 0"):
        _cholesky_or_name(H, np.array([4, 7], np.int32), 2, 2)
    A = np.array([[4.0, 2.0], [2.0, 3.0]])
    L = _cholesky_or_name(A, np.array([0], np.int32), 1, 2)
    assert np.allclose(L @ L.T, A) and np.allclose(L, np.linalg.cholesky(A))

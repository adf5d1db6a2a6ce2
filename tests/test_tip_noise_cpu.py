"""Measurement error at the tips, host side (no GPU): the statements the GPU tests of test_gpu_tip_noise.py lean on, pinned to
the untouched oracle.

(a) the correction the device adds to a filled record (noise_ref.correction: D = -j E j', Delta J, Delta h, Delta g) against the
    difference of the GENERIC factors of the wrapper (noise_ref.NoisyTipModel) and of the plain model, tip absorbed, complete
    data; noise with diag(E) between 0.01 and 100 times diag(V): the statement itself stays inside 1e-8 there;
(b) belief propagation of the wrapper's factors on the clique tree against the dense log-likelihood, the p = 3 network with
    30 % missing values included;
(c) noise_ref.family_statement -- the sweeps under noise, dsigma_e among them -- against Richardson central differences of
    the wrapper's dense log-likelihood, with shifts set as well;
(d) the workaround, a pendant node of its own rate colour under every noisy tip of a tree under heterogeneous BM, gives the
    same log-likelihood as the wrapper;
(e) fill-then-correct against the direct factor at |E| / |V| = 1 .. 1e8: the error grows like 2^-52 (1 + |E| / |V|); the
    table is printed and the ratio at which 1e-8 is left is pinned to its decade.
Everything at 1e-8 relative to the largest entry of the block; the measured figures are printed."""
import numpy as np
import pytest

import loo_ref as LR
import noise_ref as NR
from edge_ref import rel_block_nan
from helpers import oracle_setup
from oracle import calibration as OC
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from shift_ref import ShiftedModel
from test_gradient_cpu import _case, _more_cases, model_params, model_with, rel_block, richardson
from test_shift_cpu import shifts_of

TOL = 1e-8


def cases():
    for which in ("bm", "ou"):
        yield (f"{which}_random_root",) + _case(which)
    yield from _more_cases()


CASES = list(cases())
IDS = [c[0] for c in CASES]
COMPLETE = [c for c in CASES if not c[0].startswith("missing")]


def noisy_tips(net, model, seed=7, with_se2=True):
    """Every second tip in preorder, a hybrid tip (one with several parent edges) among them when there is one: (node
    indices, scale, sigma_e, se2, E [n, p, p])."""
    pre = net.vec_node
    tips = [i for i, n in enumerate(pre) if n.leaf]
    pick = tips[::2]
    hyb = [i for i in tips if len(net.parent_edges(pre[i])) >= 2]
    if hyb and hyb[0] not in pick:
        pick = sorted(pick + [hyb[0]])
    rng = np.random.default_rng(seed)
    Vd = np.array([np.diag(NR.oracle_tip_variance(net, model, pre[i])) for i in pick])
    scale, sigma_e, se2 = NR.draw_noise_from_diag(Vd, rng, with_se2=with_se2)
    return pick, scale, sigma_e, se2, NR.tip_noise(scale, sigma_e, se2)


def wrapped(net, model, pick, E):
    pre = net.vec_node
    return NR.NoisyTipModel(model, {net.parent_edges(pre[i])[0].number: e for i, e in zip(pick, E)})


@pytest.mark.parametrize("case", COMPLETE, ids=[c[0] for c in COMPLETE])
def test_correction_against_the_generic_factors(case):
    name, net, model, tbl, taxa = case
    p = model.dimension()
    pre = net.vec_node
    pick, scale, sigma_e, se2, E = noisy_tips(net, model)
    w = wrapped(net, model, pick, E)
    worst, ratios = 0.0, []
    for i, e in zip(pick, E):
        pae = net.parent_edges(pre[i])
        if len(pae) == 1:
            plain, noisy = OM.EvolutionaryModel.factor_treeedge(model, pae[0]), w.factor_treeedge(pae[0])
        else:
            plain, noisy = OM.EvolutionaryModel.factor_hybridnode(model, pae), w.factor_hybridnode(pae)
        y = np.array([float(tbl[t][list(taxa).index(pre[i].name)]) for t in range(p)])
        h0, J0, g0 = NR.absorb_tip(plain, y, p)
        h1, J1, g1 = NR.absorb_tip(noisy, y, p)
        qwv = [model.branch_qwv(ed) for ed in pae]
        V = NR.oracle_tip_variance(net, model, pre[i])
        qs = [ed.gamma * float(np.atleast_2d(q)[0, 0]) for ed, (q, _, _) in zip(pae, qwv)]
        wsum = sum(ed.gamma * np.asarray(ww, float).reshape(p) for ed, (_, ww, _) in zip(pae, qwv))
        dh, dJ, dg = NR.correction(V, e, qs, wsum - y)
        ratios.append(float(np.max(np.diag(e) / np.diag(V))))
        worst = max(worst, rel_block(J0 + dJ, J1), rel_block(h0 + dh, h1), abs(g0 + dg - g1) / max(1.0, abs(g1)))
    print(f"{name}: {len(pick)} noisy tips, diag(E) / diag(V) up to {max(ratios):.1f}: fill + correction vs the generic "
          f"noisy factor {worst:.2e}")
    assert worst <= TOL


def bp_loglik(net, model, tbl, taxa):
    cg = OCG.cliquetree(net)
    ocgb = oracle_setup(net, cg, model, tbl, taxa)
    root = OCG.default_rootcluster(cg, net)
    assert OC.calibrate(ocgb, [OCG.spanningtree_clusterlist(cg, root)], verbose=False)[0]
    return ocgb.integratebelief(root)[1]


BP_CASES = COMPLETE + [("missing30_p3",) + LR.missing_case()]


@pytest.mark.parametrize("case", BP_CASES, ids=[c[0] for c in BP_CASES])
def test_bp_of_the_wrapper_against_the_dense_loglik(case):
    name, net, model, tbl, taxa = case
    pick, _, _, _, E = noisy_tips(net, model)
    w = wrapped(net, model, pick, E)
    dense = OD.loglik(net, w, tbl, taxa)
    bp = bp_loglik(net, w, tbl, taxa)
    err = abs(bp - dense) / max(1.0, abs(dense))
    print(f"{name}: BP of the wrapper vs dense {err:.2e} (loglik {dense:.6f}, without noise {OD.loglik(net, model, tbl, taxa):.6f})")
    assert err <= TOL
    assert abs(dense - OD.loglik(net, model, tbl, taxa)) > 1e-3   # (the noise does something)


SWEEP = [c for c in CASES if c[0] in ("bm_random_root", "ou_random_root", "hetero3_fixed_root", "missing_random_root")]


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_family_statement_against_finite_differences(case):
    """dR, dmu, dalpha, dtheta, dsigma_e, dlength, dgamma and gamma_k * dshift of the shifted edges, each block against
    Richardson differences of densemvn.loglik of the wrapper around the shifted model."""
    name, net, model, tbl, taxa = case
    p = model.dimension()
    shifts = shifts_of(net, model)
    pick, scale, sigma_e, se2, E = noisy_tips(net, model)
    pre = net.vec_node
    rates, root_color, mu, alpha, theta = model_params(model)

    def ll(rates_=rates, mu_=mu, alpha_=alpha, theta_=theta, shifts_=shifts, sig_=sigma_e):
        inner = ShiftedModel(model_with(model, rates_, mu_, alpha_, theta_), shifts_)
        return OD.loglik(net, wrapped(net, inner, pick, NR.tip_noise(scale, sig_, se2)), tbl, taxa)
    st = NR.dense_statement(net, wrapped(net, ShiftedModel(model, shifts), pick, E), model, shifts, dict(zip(pick, E)),
                            dict(zip(pick, scale)), tbl, taxa)
    h = 1e-3
    want = dict(dR=np.zeros_like(st["dR"]), dmu=np.zeros(p), dalpha=0.0, dtheta=np.zeros(p), dsigma_e=np.zeros((p, p)))
    for a in range(p):
        for b in range(a, p):
            B = np.zeros((p, p)); B[a, b] += 0.5; B[b, a] += 0.5
            for c in range(len(rates)):
                f = lambda s, c=c, B=B: ll(rates_=[r + (s * B if q == c else 0) for q, r in enumerate(rates)])
                want["dR"][c, a, b] = want["dR"][c, b, a] = richardson(f, h)
            want["dsigma_e"][a, b] = want["dsigma_e"][b, a] = richardson(lambda s, B=B: ll(sig_=sigma_e + s * B), h)
        want["dmu"][a] = richardson(lambda s, a=a: ll(mu_=mu + s * np.eye(p)[a]), h)
    if alpha is not None:
        want["dalpha"] = richardson(lambda s: ll(alpha_=alpha + s), h)
        want["dtheta"] = np.array([richardson(lambda s: ll(theta_=theta + s), h)])
    for k in ("dR", "dmu", "dalpha", "dtheta", "dsigma_e"):
        if not np.any(np.atleast_1d(want[k])) and not np.any(np.atleast_1d(st[k])):
            continue
        err = rel_block(st[k], want[k])
        print(f"{name} {k}: {err:.2e}")
        assert err <= TOL, (name, k, st[k], want[k])
    assert np.max(np.abs(st["dsigma_e"])) > 1e-6
    N, K = st["dlength"].shape
    fd = dict(dlength=np.full((N, K), np.nan), dgamma=np.full((N, K), np.nan))
    for i in range(1, N):
        for k, ed in enumerate(st["edges"][i]):
            for attr, key in (("length", "dlength"), ("gamma", "dgamma")):
                keep = getattr(ed, attr)
                fixed = {net.parent_edges(pre[q])[0].number: e for q, e in zip(pick, E)}

                def f(s, ed=ed, attr=attr, keep=keep):
                    # the noise E_f does not move with the edge: the wrapper divides by the CURRENT gamma of the edge
                    setattr(ed, attr, keep * (1.0 + s))
                    try:
                        return OD.loglik(net, NR.NoisyTipModel(ShiftedModel(model, shifts), fixed), tbl, taxa)
                    finally:
                        setattr(ed, attr, keep)
                fd[key][i, k] = richardson(f, h) / keep
    for key in ("dlength", "dgamma"):
        err = rel_block_nan(st[key], fd[key])
        print(f"{name} {key}: {err:.2e}")
        assert err <= TOL, (name, key)
    for ed_no, s0 in shifts.items():
        ed = next(e for e in net.edges if e.number == ed_no)
        i = next(q for q, n in enumerate(pre) if n is ed.child)
        got = ed.gamma * st["dshift"][i]
        wantg = np.array([richardson(lambda s, t=t: ll(shifts_={**shifts, ed_no: s0 + s * np.eye(p)[t]}), h) for t in range(p)])
        err = rel_block(got, wantg)
        print(f"{name} shift on edge {ed_no}: {err:.2e}")
        assert err <= TOL


def test_pendant_nodes_under_heterogeneous_bm_give_the_same_loglik():
    rng = np.random.default_rng(12)
    p, n = 2, 12
    tree = ON.random_network(n, 0, rng)
    tree.name_internal_nodes()
    taxa = tree.tip_names
    tbl = [list(rng.normal(size=n)) for _ in range(p)]
    model = LR.bm(p, rng, "random")
    tips = list(taxa[::2])
    scale = rng.uniform(0.05, 1.0, size=len(tips))
    A = rng.normal(size=(p, p))
    sigma_e = A @ A.T / p + 0.3 * np.eye(p)
    at = {nd.name: i for i, nd in enumerate(tree.vec_node)}
    w = wrapped(tree, model, [at[t] for t in tips], NR.tip_noise(scale, sigma_e))
    net2, model2 = NR.pendant_case(tree, model.R, sigma_e, model.rootpriormeanvector(), model.rootpriorvariance(), tips, scale)
    a, b = OD.loglik(tree, w, tbl, taxa), OD.loglik(net2, model2, tbl, taxa)
    print(f"wrapper {a:.10f}, pendant nodes {b:.10f} ({len(net2.vec_node)} nodes instead of {len(tree.vec_node)})")
    assert abs(a - b) <= TOL * abs(a)
    assert abs(bp_loglik(net2, model2, tbl, taxa) - a) <= TOL * abs(a)


def test_error_of_fill_then_correct_grows_with_the_ratio():
    eps = 2.0 ** -52
    rows = []
    for k in range(9):
        ratio = 10.0 ** k
        err = max(NR.fill_then_correct_error(ratio, seed=s)[0] for s in range(5))
        floor = max(NR.fill_then_correct_error(ratio, seed=s)[1] for s in range(5))
        rows.append((ratio, err, floor))
        print(f"|E| / |V| = {ratio:8.0e}: fill + correction {err:.2e} (direct inverse in double {floor:.2e}; "
              f"eps (1 + ratio) = {eps * (1 + ratio):.2e})")
    for ratio, err, _ in rows:
        assert err <= 64 * eps * (1 + ratio)       # the stated law, with room for p = 3 and the conditioning of V
    assert rows[2][1] <= 1e-12                     # nothing is lost up to |E| = 100 |V|, the range of the GPU tests
    left = [ratio for ratio, err, _ in rows if err <= 1e-8]
    print(f"1e-8 is left up to |E| / |V| = {max(left):.0e}")
    assert 1e6 <= max(left) <= 1e8

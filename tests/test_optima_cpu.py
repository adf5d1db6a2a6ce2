"""Painted optima under OU, host side (no GPU): the statements test_gpu_optima.py leans on, pinned to the untouched oracle.

(a) belief propagation of the wrapper (optima_ref.painted_model) on the clique tree against densemvn.loglik of the wrapper;
(b) the identity loglik_painted(y) = loglik_unpainted(y - Delta), Delta the tips' offsets of the equivalent shifts;
(c) optima_ref.dense_statement (doptima, dtheta, dalpha, dR, dmu) against Richardson differences (1e-3, 5e-4) of the dense
    log-likelihood of the painted model;
(d) the sum rule: dtheta + sum_r doptima_r is the derivative in a common move of all optima;
(e) the margins the GPU tests rely on: the smallest family variance (the pivots of the fill and of the sweeps) and the
    conditioning of the GLS design of the fit case, so that every regime is identified;
(f) the cancellation limit of "fill with theta, then add wc (theta_r - theta)" quoted in DESIGN.md, measured.
Everything at 1e-8 relative to max(1, |block|); the measured figures are printed."""
import numpy as np
import pytest

import optima_ref as OR
from helpers import oracle_setup
from oracle import calibration as OC
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from test_gradient_cpu import _case, _more_cases, model_params, model_with, richardson
from test_shift_cpu import moved_data

TOL = 1e-8


def cases():
    """The two OU cases of test_gradient_cpu: 30 tips / 6 hybrids with a proper random root, 16 tips / 4 hybrids fixed root."""
    yield ("ou_random_root",) + _case("ou")
    yield next(c for c in _more_cases() if c[0] == "ou_fixed_root")


CASES = list(cases())
IDS = [c[0] for c in CASES]
N_REG = 3                       # regimes 1 and 3 are carried by edges, regime 2 by none
VALUES = np.array([1.7, -4.0, -0.9])


def _rel(got, want):
    got, want = np.atleast_1d(np.asarray(got, float)), np.atleast_1d(np.asarray(want, float))
    return float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))


def _painted(net):
    reg = OR.paint(net, 4, N_REG, unused=2)
    assert {1, 3} <= set(reg.values()) and 2 not in reg.values() and 0 in reg.values()
    hyb = next(n for n in net.vec_node[1:] if len(net.parent_edges(n)) >= 2)
    a, b = net.parent_edges(hyb)[:2]
    assert reg[a.number] != reg[b.number]   # a hybrid family whose two parent edges carry different regimes
    return reg


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bp_of_the_wrapper_and_the_moved_data_identity(case):
    name, net, model, tbl, taxa = case
    reg = _painted(net)
    w = OR.painted_model(model, net, reg, VALUES)
    dense = OD.loglik(net, w, tbl, taxa)
    moved, _ = moved_data(net, model, w.shifts, tbl, taxa)
    plain = OD.loglik(net, model, moved, taxa)
    cg = OCG.cliquetree(net)
    ocgb = oracle_setup(net, cg, w, tbl, taxa)
    root = OCG.default_rootcluster(cg, net)
    assert OC.calibrate(ocgb, [OCG.spanningtree_clusterlist(cg, root)], verbose=False)[0]
    bp = ocgb.integratebelief(root)[1]
    e1, e2 = abs(bp - dense) / max(1.0, abs(dense)), abs(plain - dense) / max(1.0, abs(dense))
    print(f"{name}: BP of the wrapper vs dense {e1:.2e}, unpainted on y - Delta vs dense {e2:.2e}")
    assert e1 <= TOL and e2 <= TOL
    assert abs(dense - OD.loglik(net, model, tbl, taxa)) > 1e-3   # (the optima do something)


def _loglik(net, model, reg, tbl, taxa, alpha=None, theta=None, values=VALUES):
    rates, _, mu, a0, t0 = model_params(model)
    m = model_with(model, rates, mu, a0 if alpha is None else alpha, t0 if theta is None else np.array([theta]))
    return OD.loglik(net, OR.painted_model(m, net, reg, values), tbl, taxa)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_statement_against_finite_differences_and_the_sum_rule(case):
    name, net, model, tbl, taxa = case
    reg = _painted(net)
    st = OR.dense_statement(net, model, reg, VALUES, tbl, taxa)
    h = 1e-3
    want = dict(dalpha=richardson(lambda s: _loglik(net, model, reg, tbl, taxa, alpha=model.alpha + s), h),
                dtheta=richardson(lambda s: _loglik(net, model, reg, tbl, taxa, theta=model.theta + s), h),
                doptima=np.array([richardson(lambda s, r=r: _loglik(net, model, reg, tbl, taxa,
                                                                    values=VALUES + s * np.eye(N_REG)[r]), h)
                                  for r in range(N_REG)]))
    for k in ("dalpha", "dtheta", "doptima"):
        err = _rel(st[k], want[k])
        print(f"{name} {k}: {err:.2e}")
        assert err <= TOL, (k, st[k], want[k])
    assert st["doptima"][1] == 0.0 and np.all(st["doptima"][[0, 2]] != 0.0)   # the regime no edge carries
    common = richardson(lambda s: _loglik(net, model, reg, tbl, taxa, theta=model.theta + s, values=VALUES + s), h)
    got = float(st["dtheta"][0] + st["doptima"].sum())
    print(f"{name}: sum rule {abs(got - common) / max(1.0, abs(common)):.2e}")
    assert abs(got - common) <= TOL * max(1.0, abs(common))
    # the unpainted statement is not the painted one
    plain = OR.dense_statement(net, model, {}, VALUES, tbl, taxa)
    assert abs(plain["dalpha"] - st["dalpha"]) > 1e-3 and abs(plain["dtheta"][0] - st["dtheta"][0]) > 1e-3


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_margins_of_the_gpu_cases(case):
    """The smallest family variance over the network (every pivot of the fill and of the sweeps is a sum of these): far above
    the 1e-8 the comparisons are made at, relative to the stationary variance."""
    name, net, model, tbl, taxa = case
    small = min(sum(model.branch_qwv(e)[2][0, 0] * (e.gamma ** 2 if len(net.parent_edges(n)) > 1 else 1.0)
                    for e in net.parent_edges(n)) for n in net.vec_node[1:])
    print(f"{name}: smallest family variance {small:.3e} (stationary variance {model.gamma2:.3e})")
    assert small >= 1e-3 * model.gamma2


def fit_case(n_tips=96, n_sites=24, seed=41):
    """The fit case of test_gpu_optima.py: a 96-tip tree, two disjoint clades painted 1 and 2 (every edge inside them and their
    stems), the rest regime 0; per-site data simulated under per-site (alpha, stationary variance, mu, theta, theta_1,
    theta_2).  Returns (synth tree, oracle net, taxa, tip node of each taxon, {edge.number: r}, regime of each node's parent
    edge [n_nodes], data [n_sites, n_nodes], true parameters)."""
    from pgbp_amd import synth
    rng = np.random.default_rng(seed)
    tree = synth.random_tree(n_tips, rng)
    kids = [np.nonzero(tree.parent == i)[0] for i in range(tree.nnodes)]

    def below(i):
        out, stack = [], [i]
        while stack:
            j = stack.pop()
            out.append(j)
            stack.extend(int(c) for c in kids[j])
        return out
    sizes = {i: sum(bool(tree.is_leaf[j]) for j in below(i)) for i in range(1, tree.nnodes)}
    c1 = next(i for i in sorted(sizes, key=lambda i: (abs(sizes[i] - 20), i)))
    in1 = set(below(c1))
    c2 = next(i for i in sorted(sizes, key=lambda i: (abs(sizes[i] - 20), i)) if i not in in1 and c1 not in below(i))
    node_reg = np.zeros(tree.nnodes, np.int32)
    node_reg[below(c1)] = 1
    node_reg[below(c2)] = 2
    depth = np.zeros(tree.nnodes)
    for i in range(1, tree.nnodes):
        depth[i] = depth[tree.parent[i]] + tree.length[i]
    H = float(depth[tree.is_leaf].mean())
    # alpha H of 1 .. 3, the recipe of test_gpu_gradient_sites.ou_fit_case: the phylogenetic signal is strong enough for the
    # profile likelihood in alpha to have its optimum inside (0, inf)
    alpha, gam2 = rng.uniform(1.0, 3.0, n_sites) / H, rng.uniform(0.5, 2.0, n_sites)
    mu, theta = rng.normal(size=n_sites), rng.normal(size=n_sites)
    opt = theta[:, None] + rng.choice([-1.0, 1.0], size=(n_sites, 2)) * rng.uniform(1.5, 3.0, size=(n_sites, 2))
    X = np.zeros((n_sites, tree.nnodes))
    for s in range(n_sites):
        X[s, 0] = mu[s]
        for i in range(1, tree.nnodes):   # (synth's nodes are in preorder: parent < child)
            a = np.exp(-alpha[s] * tree.length[i])
            th = theta[s] if node_reg[i] == 0 else opt[s, node_reg[i] - 1]
            X[s, i] = a * X[s, tree.parent[i]] + (1 - a) * th + np.sqrt(gam2[s] * (1 - a * a)) * rng.normal()
    net = ON.read_newick(tree.newick())
    taxa = list(net.tip_names)
    tipnode = [int(t[1:]) for t in taxa]
    name2node = {n.name: n for n in net.vec_node}
    reg = {net.parent_edges(name2node[f"n{i}"])[0].number: int(node_reg[i]) for i in range(1, tree.nnodes)}
    return tree, net, taxa, tipnode, reg, node_reg, X, dict(alpha=alpha, gam2=gam2, mu=mu, theta=theta, optima=opt)


def test_every_regime_of_the_fit_case_is_identified():
    """cond of the GLS design (mu fixed at its value: a fixed root; columns theta, theta_1, theta_2) in the metric of the tips'
    covariance, at the smallest and the largest alpha of the fit case: the normal equations are solved far from singular."""
    tree, net, taxa, tipnode, reg, node_reg, X, true = fit_case()
    assert {0, 1, 2} == set(reg.values())
    assert min(int(np.sum(node_reg[tree.is_leaf] == r)) for r in (0, 1, 2)) >= 10
    for s in (int(np.argmin(true["alpha"])), int(np.argmax(true["alpha"]))):
        model = OM.UnivariateOrnsteinUhlenbeck(2 * true["alpha"][s] * true["gam2"][s], true["alpha"][s], true["theta"][s],
                                               true["mu"][s], None)
        tbl = [[float(X[s, i]) for i in tipnode]]
        bhat, Xd, S, r0 = OR.gls_optima(net, model, reg, 2, tbl, taxa, free=(1, 2, 3))
        Lc = np.linalg.cholesky(S)
        cond = np.linalg.cond(np.linalg.solve(Lc, Xd))
        print(f"site {s}: alpha {true['alpha'][s]:.3f}, cond of the whitened design {cond:.2f}, GLS optima {bhat}")
        assert cond <= 50.0
        # the GLS estimate is where the dense statement's dtheta and doptima vanish
        m2 = OM.UnivariateOrnsteinUhlenbeck(2 * true["alpha"][s] * true["gam2"][s], true["alpha"][s], bhat[0], true["mu"][s], None)
        st = OR.dense_statement(net, m2, reg, bhat[1:], tbl, taxa)
        scale = float(np.max(np.abs(Xd.T @ np.linalg.solve(S, r0))))
        assert abs(st["dtheta"][0]) <= TOL * scale and np.max(np.abs(st["doptima"])) <= TOL * scale


def test_cancellation_limit_of_fill_then_displace():
    """The device fills w0 = wc theta and the correction adds wc (theta_r - theta).  Against wc theta_r in extended precision
    the error is a few 2^-53 |wc| (|theta| + |theta_r|): harmless while theta is of the size of the optima, and growing in
    proportion to |theta| / |theta_r| when theta is parked far away.  Measured over 20 000 draws per ratio."""
    rng = np.random.default_rng(0)
    n = 20000
    wc = rng.uniform(0.05, 1.0, n)
    thr = rng.normal(size=n)
    eps = 2.0 ** -53
    for ratio in (1.0, 1e3, 1e6, 1e8):
        th = ratio * rng.normal(size=n)
        got = wc * th + wc * (thr - th)
        want = (np.longdouble(wc) * np.longdouble(thr)).astype(np.longdouble)
        err = np.abs(np.longdouble(got) - want)
        bound = 4 * eps * wc * (np.abs(th) + np.abs(thr))
        rel = float(np.max(err / (wc * np.maximum(1.0, np.abs(thr)))))
        print(f"|theta| / |theta_r| ~ {ratio:.0e}: worst error / (|wc| max(1, |theta_r|)) {rel:.2e}, "
              f"worst error / bound {float(np.max(err / bound)):.2f}")
        assert np.all(err <= bound)

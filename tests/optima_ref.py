"""Comparators for painted optima under OU (pgbp_lg_set_optima / set_optima_lg / fit_sites_lg(optima0=...)), host side,
shared by test_optima_cpu.py and test_gpu_optima.py (tests only).  None of them is the code under test.

1. `painted_model`: shift_ref.ShiftedModel around the oracle's (univariate) OU model with
   shifts[edge] = (1 - exp(-alpha t_e)) (theta_r - theta) on every painted edge; the wrapper weights the displacement of a
   hybrid edge with its gamma, so the family's offset gains sum_k gamma_k (1 - a_k) (theta_r(k) - theta) = d_opt.  The
   untouched oracle then states the painted model densely (densemvn) and as belief propagation.
2. `dense_statement`: doptima, dtheta and dalpha in numpy over the dense posterior of the wrapper, from
   shift_ref.family_statement (which holds the shifts CONSTANT) and the chain rule through the shift values.
3. `gls_optima`: for given alpha and stationary variance, the tips' means are affine in b = (mu, theta, theta_1 ..) by a
   preorder recursion; the GLS estimate of the free columns and the normal equations.

The oracle's OU is univariate, so p > 1 has no oracle statement: the GPU tests compare those layouts against a second engine
that carries the equivalent explicit shifts (`explicit_shifts`), a path tests/test_gpu_shifts.py pins on its own."""
import numpy as np

from oracle import densemvn as OD
from oracle import models as OM
from shift_ref import ShiftedModel, family_edge, family_nodes, family_statement


def paint(net, seed, n_regimes, unused=None, both_hybrid=True):
    """{edge.number: regime} for an oracle network: every edge draws from 0 .. n_regimes (regime `unused` is never drawn), and
    the two parent edges of the first hybrid node carry different regimes when both_hybrid."""
    rng = np.random.default_rng(seed)
    pool = [r for r in range(n_regimes + 1) if r != unused]
    reg = {e.number: int(rng.choice(pool)) for e in net.edges}
    hyb = [n for n in net.vec_node[1:] if len(net.parent_edges(n)) >= 2]
    if hyb and both_hybrid:
        painted = [r for r in pool if r > 0]
        a, b = net.parent_edges(hyb[0])[:2]
        reg[a.number] = painted[0]
        reg[b.number] = painted[1] if len(painted) > 1 else 0
    return reg


def painted_model(model, net, regimes, values):
    """regimes: {edge.number: r}; values [n_regimes] (p = 1).  The first comparator."""
    assert isinstance(model, OM.UnivariateOrnsteinUhlenbeck)
    values = np.asarray(values, float).reshape(-1)
    sh = {}
    for e in net.edges:
        r = regimes.get(e.number, 0)
        if r > 0:
            sh[e.number] = np.array([(1.0 - np.exp(-model.alpha * e.length)) * (values[r - 1] - model.theta)])
    return ShiftedModel(model, sh)


def device_regime(net, ocgb, fam, regimes):
    """The dense map [n_families, K] of set_optima_lg for {edge.number: r}."""
    nf = len(fam["cluster"])
    K = max(1, int(fam["max_parents"]))
    m = np.zeros((nf, K), np.int32)
    for f in range(nf):
        for k in range(int(fam["n_parents"][f])):
            m[f, k] = regimes.get(family_edge(net, ocgb, fam, f, k).number, 0)
    return m


def explicit_shifts(fam, regime, values, alpha, theta):
    """(edges [(f, k)], shift values [n, p]) that imitate the painted optima on an engine without them, in the table's own
    terms: s = (1 - exp(-alpha t)) (theta_r - theta) on every painted edge (gamma is applied by the shift itself)."""
    nf = len(fam["cluster"])
    K = max(1, int(fam["max_parents"]))
    length = np.asarray(fam["length"], float).reshape(nf, K)
    values = np.asarray(values, float)
    edges, out = [], []
    for f in range(nf):
        for k in range(int(fam["n_parents"][f])):
            r = int(regime[f, k])
            if r > 0:
                edges.append((f, k))
                out.append((1.0 - np.exp(-alpha * length[f, k])) * (values[r - 1] - np.asarray(theta, float)))
    return edges, np.array(out).reshape(len(edges), -1)


def dense_statement(net, model, regimes, values, tbl, taxa):
    """The second comparator: dR, dmu, dalpha, dtheta and doptima [n_regimes] of the painted model (p = 1) over the dense
    posterior.  family_statement differentiates with the shift VALUES held constant; the painted shifts move with alpha and
    theta: s_e = (1 - a_e)(theta_r - theta), a_e = exp(-alpha t_e), d s_e / d alpha = t_e a_e (theta_r - theta),
    d s_e / d theta = -(1 - a_e), d s_e / d theta_r = 1 - a_e, and d loglik / d s_e = gamma_e g_w(child of e)."""
    values = np.asarray(values, float).reshape(-1)
    w = painted_model(model, net, regimes, values)
    pm, pc = OD.posterior_node_moments(net, w, tbl, taxa)
    st = family_statement(net, model, w.shifts, pm, pc)
    pos = {id(n): i for i, n in enumerate(net.vec_node)}
    dopt = np.zeros(len(values))
    dal, dth = float(st["dalpha"]), float(np.ravel(st["dtheta"])[0])
    for e in net.edges:
        r = regimes.get(e.number, 0)
        if r <= 0:
            continue
        a = np.exp(-model.alpha * e.length)
        gs = e.gamma * float(st["dshift"][pos[id(e.child)]][0])
        dopt[r - 1] += (1.0 - a) * gs
        dth -= (1.0 - a) * gs
        dal += e.length * a * (values[r - 1] - model.theta) * gs
    return dict(dR=st["dR"], dmu=st["dmu"], dalpha=dal, dtheta=np.array([dth]), doptima=dopt)


def tip_design(net, alpha, regimes, n_regimes, fixed_root=True):
    """Preorder recursion: E[x_node] = D[node] @ (mu, theta, theta_1 .. theta_n).  Root: e_mu.  A node with parent edges k:
    sum_k gamma_k (a_k D[parent_k] + (1 - a_k) e_{regime(k)}).  Returns D [n_nodes, 2 + n_regimes]."""
    pre = net.vec_node
    pos = {id(n): i for i, n in enumerate(pre)}
    D = np.zeros((len(pre), 2 + n_regimes))
    D[0, 0] = 1.0
    for i in range(1, len(pre)):
        pes = net.parent_edges(pre[i])
        for e in pes:
            g = e.gamma if len(pes) > 1 else 1.0
            a = np.exp(-alpha * e.length)
            D[i] += g * a * D[pos[id(e.parent)]]
            D[i, 1 + regimes.get(e.number, 0)] += g * (1.0 - a)
    return D


def gls_optima(net, model, regimes, n_regimes, tbl, taxa, free):
    """The third comparator: at the model's alpha, stationary variance and root variance, the GLS estimate of the columns
    `free` of b = (mu, theta, theta_1 ..) with the others at the model's values (regime values: 0), fixed or proper random
    root.  Returns (bhat [len(free)], X [n_obs, len(free)], S, residual of the fixed part)."""
    pre = net.vec_node
    _, cov, _ = OD.node_moments(net, model)
    D = tip_design(net, model.alpha, regimes, n_regimes)
    obs, y = [], []
    for i, n in enumerate(pre):
        if n.leaf and tbl[0][list(taxa).index(n.name)] is not None:
            obs.append(i)
            y.append(float(tbl[0][list(taxa).index(n.name)]))
    S = cov[np.ix_(obs, obs)]
    b0 = np.zeros(2 + n_regimes)
    b0[0], b0[1] = float(model.mu[0]), model.theta
    b0[list(free)] = 0.0
    X = D[np.ix_(obs, list(free))]
    r0 = np.array(y) - D[obs] @ b0
    SiX = np.linalg.solve(S, X)
    return np.linalg.solve(X.T @ SiX, SiX.T @ r0), X, S, r0

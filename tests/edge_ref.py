"""Per-edge derivatives of the log-likelihood, host side: the numpy statement the device sweep pgbp_lg_edge_gradient is
compared with, and the finite differences of the dense oracle that pin it (test_edge_gradient_cpu.py).

Notation of test_gradient_cpu.family_gradient: per family r = x_child - sum_k qc_k x_k - w, V = sum_k vc_k R[colour_k],
j = V^-1, e = E[r], M = Cov(r) + e e', G_V = (j M j - j) / 2, g_w = j e, g_qk = E[r' j x_k].  The length t_k and the inheritance
gamma_k of parent edge k enter the family's factor only through (qc_k, vc_k, wc_k), so by Fisher's identity
    dX_k = dvc_k/dX tr(G_V R[colour_k]) + dwc_k/dX theta' g_w + dqc_k/dX g_qk,      X in {t, gamma},
and an additive displacement s of the child's conditional mean (r = ... - w - s) has the score g_w.
    BM:  qc = gamma, vc = gamma^2 t, wc = 0;  OU (a = exp(-alpha t)):  qc = gamma a, vc = gamma^2 (1 - a^2), wc = gamma (1 - a)."""
import numpy as np

from oracle import densemvn as OD
from oracle import models as OM
from test_gradient_cpu import model_params, richardson


def edge_coefs(alpha, t, g):
    """(qc, vc, wc) of a parent edge and their partial derivatives in t and in gamma: three triples."""
    if alpha is None:
        return (g, g * g * t, 0.0), (0.0, g * g, 0.0), (1.0, 2 * g * t, 0.0)
    a = np.exp(-alpha * t)
    return ((g * a, g * g * (1 - a * a), g * (1 - a)),
            (-g * alpha * a, 2 * g * g * alpha * a * a, g * alpha * a),
            (a, 2 * g * (1 - a * a), 1 - a))


def family_edge_gradient(net, model, pm, pc):
    """pm / pc: posterior mean / covariance of ALL node states in preorder (a fixed root, an observed tip value: variance 0),
    as densemvn.posterior_node_moments returns them.  Returns a dict over the nodes in preorder (row 0: the root):
    dlength, dgamma [N, K] (K = largest number of parents; NaN where there is no such edge, the whole root row included),
    dshift [N, p] (root row: the root prior's j e when the prior is proper, else NaN: no family), edges [N][k] (the Edge
    objects, in net.parent_edges order) and qc, wc [N, K] (0 where there is no edge)."""
    pre = net.vec_node
    p = model.dimension()
    rates, root_color, mu, alpha, theta = model_params(model)
    pos = {id(n): i for i, n in enumerate(pre)}
    sl = lambda i: slice(i * p, (i + 1) * p)
    N = len(pre)
    K = max([1] + [len(net.parent_edges(n)) for n in pre])
    hetero = isinstance(model, OM.HeterogeneousBrownianMotion)
    ou = alpha is not None
    dlen, dgam = np.full((N, K), np.nan), np.full((N, K), np.nan)
    dshift = np.full((N, p), np.nan)
    qcs, wcs = np.zeros((N, K)), np.zeros((N, K))
    edges = [[] for _ in range(N)]
    if root_color is not None:
        dshift[0] = np.linalg.inv(rates[root_color]) @ (pm[sl(0)] - mu)
    for i in range(1, N):
        pes = net.parent_edges(pre[i])
        edges[i] = list(pes)
        co = [edge_coefs(alpha, ed.length, ed.gamma) for ed in pes]
        col = [model._c(ed) if hetero else 0 for ed in pes]
        pis = [pos[id(ed.parent)] for ed in pes]
        V = sum(c[0][1] * rates[cc] for c, cc in zip(co, col))
        j = np.linalg.inv(V)
        w = sum(c[0][2] for c in co) * theta if ou else np.zeros(p)
        blocks = [(1.0, i)] + [(-c[0][0], pi) for c, pi in zip(co, pis)]
        e = sum(c * pm[sl(b)] for c, b in blocks) - w
        S = sum(ca * cb * pc[sl(a), sl(b)] for ca, a in blocks for cb, b in blocks)
        G = 0.5 * (j @ (S + np.outer(e, e)) @ j - j)
        gw = j @ e
        dshift[i] = gw
        thg = float(theta @ gw) if ou else 0.0
        for k, pi in enumerate(pis):
            Erx = sum(c * pc[sl(b), sl(pi)] for c, b in blocks) + np.outer(e, pm[sl(pi)])
            gq = np.trace(j @ Erx)
            trGR = np.trace(G @ rates[col[k]])
            (qc, _, wc), dt, dg = co[k]
            dlen[i, k] = dt[1] * trGR + dt[2] * thg + dt[0] * gq
            dgam[i, k] = dg[1] * trGR + dg[2] * thg + dg[0] * gq
            qcs[i, k], wcs[i, k] = qc, wc
    return dict(dlength=dlen, dgamma=dgam, dshift=dshift, edges=edges, qc=qcs, wc=wcs)


def dense_edge_gradient(net, model, tbl, taxa):
    """family_edge_gradient on the dense oracle's posterior moments (proper or fixed root)."""
    pm, pc = OD.posterior_node_moments(net, model, tbl, taxa)
    return family_edge_gradient(net, model, pm, pc)


def _perturbed(ed, name, f):
    """s -> f() with attribute `name` of edge `ed` at value (1 + s) x its own, restored afterwards."""
    def g(s):
        keep = getattr(ed, name)
        setattr(ed, name, keep * (1.0 + s))
        try:
            return f()
        finally:
            setattr(ed, name, keep)
    return g


def shift_transfer(net, model, c):
    """tau[n]: what a unit displacement of node c's conditional mean adds to the mean of node n (per trait; the edge
    coefficients qc are scalars): tau[c] = 1, tau[n] = sum_k qc_k tau[parent_k] down the preorder."""
    pre = net.vec_node
    pos = {id(n): i for i, n in enumerate(pre)}
    alpha = model_params(model)[3]
    tau = np.zeros(len(pre))
    tau[c] = 1.0
    for i in range(c + 1, len(pre)):
        tau[i] = sum(edge_coefs(alpha, ed.length, ed.gamma)[0][0] * tau[pos[id(ed.parent)]] for ed in net.parent_edges(pre[i]))
    return tau


def fd_edge_gradient(net, model, tbl, taxa, h=1e-3, steps=None):
    """The arrays of family_edge_gradient from Richardson central differences (steps h, h / 2) of densemvn.loglik.
    Length and gamma: one oracle edge at a time at (1 + s) x its value, derivative in s divided by the value (densemvn takes
    gamma as given, without renormalising: the FREE partial).  Shift of node c: the tips' data minus tau[tip] s (the step is
    absolute: the perturbed value is 0, and the log-likelihood is quadratic in s).  The root row: the derivative in the root
    prior's mean when the prior is proper, else NaN.
    steps: several values of h at once -- a list of dicts, one per h; an evaluation two of them share is made once."""
    hs = [h] if steps is None else list(steps)
    pre = net.vec_node
    p = model.dimension()
    N = len(pre)
    root_color = model_params(model)[1]
    ll = lambda: OD.loglik(net, model, tbl, taxa)
    edges = [[]] + [list(net.parent_edges(pre[i])) for i in range(1, N)]
    K = max([1] + [len(e) for e in edges])
    out = [dict(dlength=np.full((N, K), np.nan), dgamma=np.full((N, K), np.nan), dshift=np.full((N, p), np.nan), edges=edges)
           for _ in hs]

    def differences(f):
        seen = {}

        def g(s):
            if s not in seen:
                seen[s] = f(s)
            return seen[s]
        return [richardson(g, hh) for hh in hs]
    for i in range(1, N):
        for k, ed in enumerate(edges[i]):
            for o, dl, dg in zip(out, differences(_perturbed(ed, "length", ll)), differences(_perturbed(ed, "gamma", ll))):
                o["dlength"][i, k] = dl / ed.length
                o["dgamma"][i, k] = dg / ed.gamma
    rows = {n.name: list(taxa).index(n.name) for n in pre if n.leaf}
    for c in range(N):
        if c == 0 and root_color is None:
            continue
        tau = shift_transfer(net, model, c)
        tips = [(rows[pre[i].name], tau[i]) for i in range(N) if pre[i].leaf and tau[i] != 0.0]
        for t in range(p):
            def f(s, t=t):
                moved = [list(col) for col in tbl]
                for r, ta in tips:
                    if moved[t][r] is not None:
                        moved[t][r] = moved[t][r] - ta * s
                return OD.loglik(net, model, moved, taxa)
            for o, ds in zip(out, differences(f)):
                o["dshift"][c, t] = ds
    return out[0] if steps is None else out


def rel_block_nan(got, want):
    """max |got - want| relative to the largest entry of the block, over the entries that exist (not NaN in `want`); the
    NaN patterns must be the same."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), "NaN patterns differ"
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok])) / max(np.max(np.abs(want[ok])), 1e-300))

"""Comparators for the scan of every edge for a mean shift (pgbp_lg_shift_scan / shift_scan_lg / select_shifts_lg), host side,
shared by test_shift_scan_cpu.py and test_gpu_shift_scan.py (tests only).

`family_scan` is the dense statement of the sweep: per family, in the notation of shift_ref.family_statement,
r = x_child - sum_k qc_k x_k - w - d, j = V^-1, e = E[r], g_w = j e and C = Cov(r | data) from
densemvn.posterior_node_moments of the ShiftedModel wrapper;  H_f = j - j C j,  dhat = H_f^-1 g_w,  lr = g_w' H_f^-1 g_w, the
traits taken in index order by `skip_cholesky` (a pivot not above min_info * j_ii drops the trait).  It works on all p traits of
every family: a trait that a tip does not observe has a zero row and column in H_f (the likelihood does not depend on a
displacement of it) and is dropped by the same rule.

`gls_edge` is the independent statement: dense generalised least squares of ONE edge's shift on a subset of the traits, the
other shifts held, built from the pieces of shift_ref.gls_fit.  `dense_greedy` is forward selection on top of both."""
import numpy as np

from edge_ref import edge_coefs, shift_transfer
from oracle import densemvn as OD
from oracle import models as OM
from shift_ref import ShiftedModel, family_edge, family_nodes, gls_fit
from test_gradient_cpu import model_params


def skip_cholesky(H, scale, min_info):
    """Left-looking Cholesky of H in index order with the skip: index i is kept when its pivot, given the kept indices before
    it, exceeds min_info * scale[i].  Returns (kept [n] bool, L [n, n] -- rows and columns of dropped indices zero --,
    pivot / scale [n], the figure the rule looks at)."""
    n = H.shape[0]
    kept = np.zeros(n, bool)
    L = np.zeros((n, n))
    rel = np.zeros(n)
    for i in range(n):
        ks = np.flatnonzero(kept[:i])
        d = H[i, i] - L[i, ks] @ L[i, ks]
        rel[i] = d / scale[i]
        if not d > min_info * scale[i]:
            continue
        kept[i] = True
        L[i, i] = np.sqrt(d)
        for r in range(i + 1, n):
            L[r, i] = (H[r, i] - L[r, ks] @ L[i, ks]) / L[i, i]
    L[~kept, :] = 0.0
    return kept, L, rel


def restricted_solve(H, g, scale, min_info):
    """(kept, dhat -- NaN at the dropped indices --, lr, pivot / scale) of the maximum of g' d - d' H d / 2 over the kept
    indices: forward, then back."""
    kept, L, rel = skip_cholesky(H, scale, min_info)
    ks = np.flatnonzero(kept)
    d = np.full(len(g), np.nan)
    if ks.size == 0:
        return kept, d, 0.0, rel
    Lk = L[np.ix_(ks, ks)]
    y = np.linalg.solve(Lk, g[ks])
    d[ks] = np.linalg.solve(Lk.T, y)
    return kept, d, float(y @ y), rel


def family_scan(net, model, shifts, pm, pc, min_info=1e-8):
    """model: the PLAIN oracle model; shifts: {edge.number: s} in force; pm / pc: posterior moments of all node states in
    preorder under the SHIFTED model.  Rows = nodes in preorder (row 0, the root, has no edge: NaN, lr NaN, nothing
    identified).  Returns dict(jump [N, p], lr [N], identified [N, p], H [N, p, p] (NaN outside the kept traits), gw [N, p],
    relpivot [N, p], jdiag [N, p], edges [N][k] in net.parent_edges order)."""
    pre = net.vec_node
    p = model.dimension()
    rates, root_color, mu, alpha, theta = model_params(model)
    pos = {id(n): i for i, n in enumerate(pre)}
    sl = lambda i: slice(i * p, (i + 1) * p)
    N = len(pre)
    hetero = isinstance(model, OM.HeterogeneousBrownianMotion)
    ou = alpha is not None
    out = dict(jump=np.full((N, p), np.nan), lr=np.full(N, np.nan), identified=np.zeros((N, p), bool),
               H=np.full((N, p, p), np.nan), gw=np.full((N, p), np.nan), relpivot=np.full((N, p), np.nan),
               jdiag=np.full((N, p), np.nan), edges=[[] for _ in range(N)])
    for i in range(1, N):
        pes = net.parent_edges(pre[i])
        out["edges"][i] = list(pes)
        co = [edge_coefs(alpha, ed.length, ed.gamma)[0] for ed in pes]
        col = [model._c(ed) if hetero else 0 for ed in pes]
        pis = [pos[id(ed.parent)] for ed in pes]
        V = sum(c[1] * rates[cc] for c, cc in zip(co, col))
        j = np.linalg.inv(V)
        w = (sum(c[2] for c in co) * theta if ou else np.zeros(p)) + \
            sum(ed.gamma * np.asarray(shifts.get(int(ed.number), np.zeros(p)), float) for ed in pes)
        blocks = [(1.0, i)] + [(-c[0], pi) for c, pi in zip(co, pis)]
        e = sum(c * pm[sl(b)] for c, b in blocks) - w
        Cm = sum(ca * cb * pc[sl(a), sl(b)] for ca, a in blocks for cb, b in blocks)
        H = j - j @ Cm @ j
        H = (H + H.T) / 2
        gw = j @ e
        kept, d, lr, rel = restricted_solve(H, gw, np.diag(j), min_info)
        out["jump"][i], out["lr"][i], out["identified"][i], out["gw"][i], out["relpivot"][i] = d, lr, kept, gw, rel
        out["jdiag"][i] = np.diag(j)
        ks = np.flatnonzero(kept)
        out["H"][i][np.ix_(ks, ks)] = H[np.ix_(ks, ks)]
    return out


def dense_scan(net, model, shifts, tbl, taxa, min_info=1e-8):
    pm, pc = OD.posterior_node_moments(net, ShiftedModel(model, shifts), tbl, taxa)
    return family_scan(net, model, shifts, pm, pc, min_info)


def device_layout(sc, net, ocgb, fam):
    """The arrays of family_scan as shift_scan_lg returns them: rows = families of the table, edge_jump [F, K, p] = jump /
    gamma_k in the table's per-parent order (NaN where there is no edge).  A root-prior family (no parents) is all NaN."""
    nodes = family_nodes(ocgb, fam)
    K = max(1, int(fam["max_parents"]))
    p = sc["jump"].shape[1]
    out = {k: sc[k][nodes].copy() for k in ("jump", "lr", "identified", "H")}
    out["dof"] = out["identified"].sum(axis=1)
    out["edge_jump"] = np.full((len(nodes), K, p), np.nan)
    for f, i in enumerate(nodes):
        for k in range(int(fam["n_parents"][f])):
            out["edge_jump"][f, k] = sc["jump"][i] / family_edge(net, ocgb, fam, f, k).gamma
    return out


def gls_edge(net, model, tbl, taxa, edge, traits, held=None):
    """Dense GLS of an INCREMENT to the shift on `edge` (an oracle Edge) restricted to `traits` (indices), the shifts `held`
    ({edge.number: s}, `edge` itself possibly among them) staying where they are; fixed or proper random root.  The pieces of
    shift_ref.gls_fit: X = the offsets of a unit shift at the observed tip entries, S = their covariance.
    Returns (increment [len(traits)], H [len(traits)^2], loglik at the fit, loglik at `held`)."""
    held = dict(held or {})
    pre = net.vec_node
    p = model.dimension()
    traits = [int(t) for t in traits]
    base = ShiftedModel(model, held)
    m0, cov, _ = OD.node_moments(net, base)
    obs, y = [], []
    for i, n in enumerate(pre):
        if n.leaf:
            r = list(taxa).index(n.name)
            for t in range(p):
                if tbl[t][r] is not None:
                    obs.append((i, t))
                    y.append(float(tbl[t][r]))
    idx = np.array([i * p + t for i, t in obs])
    S = cov[np.ix_(idx, idx)]
    pos = {id(n): i for i, n in enumerate(pre)}
    tau = shift_transfer(net, model, pos[id(edge.child)])
    X = np.zeros((len(obs), len(traits)))
    for r, (i, t) in enumerate(obs):
        if t in traits:
            X[r, traits.index(t)] = edge.gamma * tau[i]
    SiX = np.linalg.solve(S, X)
    H = X.T @ SiX
    inc = np.linalg.solve(H, SiX.T @ (np.array(y) - m0[idx]))
    full = np.asarray(held.get(int(edge.number), np.zeros(p)), float).copy()
    full[traits] += inc
    moved = dict(held)
    moved[int(edge.number)] = full
    return inc, H, OD.loglik(net, ShiftedModel(model, moved), tbl, taxa), OD.loglik(net, base, tbl, taxa)


def candidate_edge(net, node):
    """The candidate edge of a node's family: the parent edge with the largest gamma (any parent edge of a hybrid describes
    the same displacements of the child)."""
    pes = net.parent_edges(node)
    return max(pes, key=lambda ed: ed.gamma)


def dense_greedy(net, model, tbl, taxa, max_shifts, nodes=None, min_info=1e-8):
    """Forward selection, densely: per step the gain of every candidate node -- 2 (loglik with the one-edge GLS increment on
    the traits the dense scan identifies, the chosen shifts held, minus loglik without it) --, the largest enters, all chosen
    shifts are refitted jointly by shift_ref.gls_fit.  nodes: the candidate nodes (preorder indices; default all but the root).
    Returns a list of dict(node, edge, lr, second (the second largest lr of the step), loglik, shifts)."""
    pre = net.vec_node
    nodes = list(range(1, len(pre))) if nodes is None else list(nodes)
    chosen, held, path = [], {}, []
    for _ in range(max_shifts):
        sc = dense_scan(net, model, held, tbl, taxa, min_info)
        gains = []
        for i in nodes:
            if i in [c[0] for c in chosen] or not sc["identified"][i].any():
                continue
            ed = candidate_edge(net, pre[i])
            _, _, ll1, ll0 = gls_edge(net, model, tbl, taxa, ed, np.flatnonzero(sc["identified"][i]), held)
            gains.append((2.0 * (ll1 - ll0), i, ed))
        if not gains:
            break
        gains.sort(key=lambda g: (-g[0], g[1]))
        lr, i, ed = gains[0]
        chosen.append((i, ed))
        shat, _, ll = gls_fit(net, model, tbl, taxa, [e for _, e in chosen])
        held = {int(e.number): s for (_, e), s in zip(chosen, shat)}
        path.append(dict(node=i, edge=ed, lr=lr, second=gains[1][0] if len(gains) > 1 else -np.inf, loglik=ll, shifts=shat))
    return path

"""Plain numpy restatement of pgbp_posterior_cov (include/pgbp.h) on the arrays of sample_ref.arrays_from_beliefs.

At one site the sampler of sample_ref.sample_posterior_ref is a linear map x = m + A z.  For functionals c (one row per column,
a weight per entry of the sampler's layout) posterior_cov_ref returns w = A'c by the header's adjoint recurrence (clusters in
reverse preorder: every child before its parent) and k = A w = Cov(x, c'x | data) by the forward one (preorder).  Per cluster
T = L^-T with J_RR = L L' (numpy's lower Cholesky factor) and G = J_RR^-1 J_RS; S, R and PS are the sampler's.
test_posterior_cov_cpu.py pins it to the dense oracle; test_gpu_posterior_cov.py compares the device with it."""
import numpy as np


def posterior_cov_ref(records, dims, sepset_clusters, scope_off, scope_idx, pa, ch, c):
    """records, dims, sepset_clusters, scope_off, scope_idx, pa, ch: as sample_posterior_ref; c [n_cols, size].
    Returns (w [n_cols, size], k [n_cols, size], info): info = 0, or 1 + the first cluster in preorder whose J_RR is not
    positive definite (w and k are then all NaN)."""
    nc = len(records)
    sepcl = np.asarray(sepset_clusters).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum(np.asarray(dims[:nc], dtype=np.int64))])
    c = np.atleast_2d(np.asarray(c, dtype=np.float64))
    pa, ch = [int(a) for a in pa], [int(b) for b in ch]
    root = pa[0] if pa else 0
    assert len(pa) == nc - 1 == len(sepcl), "the sweep is exact on a clique tree only"
    sep_of = {}
    for k, (a, b) in enumerate(sepcl):
        sep_of[(int(a), int(b))] = (k, 0, 1)
        sep_of[(int(b), int(a))] = (k, 1, 0)
    # the factors, in preorder
    preorder, fac = [(root, None)] + list(zip(ch, pa)), {}
    for cl, parent in preorder:
        m = int(dims[cl])
        if m == 0:
            continue
        J = np.triu(records[cl][0]) + np.triu(records[cl][0], 1).T
        if parent is None:
            S, PS = np.zeros(0, int), np.zeros(0, int)
        else:
            k, cside, pside = sep_of[(cl, parent)]
            S = np.asarray(scope_idx[scope_off[2 * k + cside]: scope_off[2 * k + cside + 1]], dtype=int)
            PS = np.asarray(scope_idx[scope_off[2 * k + pside]: scope_off[2 * k + pside + 1]], dtype=int)
        R = np.array([v for v in range(m) if v not in set(S.tolist())], dtype=int)
        T, Gm = np.zeros((0, 0)), np.zeros((0, len(S)))
        if len(R):
            try:
                Lc = np.linalg.cholesky(J[np.ix_(R, R)])
            except np.linalg.LinAlgError:
                return np.full_like(c, np.nan), np.full_like(c, np.nan), cl + 1
            T = np.linalg.solve(Lc, np.eye(len(R))).T                               # L^-T, upper triangular
            Gm = np.linalg.solve(Lc.T, np.linalg.solve(Lc, J[np.ix_(R, S)]))        # J_RR^-1 J_RS
        fac[cl] = (S, PS, R, T, Gm)
    # adjoint: xbar = c at the start; every child before its parent
    xbar, w = c.copy(), np.zeros_like(c)
    for cl, parent in reversed(preorder):
        if cl not in fac:
            continue
        S, PS, R, T, Gm = fac[cl]
        xc = xbar[:, off[cl]: off[cl + 1]]
        w[:, off[cl] + R] = xc[:, R] @ T                                            # w_R[l] = sum_{i <= l} T_il xbar_R[i]
        if len(S):
            np.add.at(xbar, (slice(None), off[parent] + PS), xc[:, S] - xc[:, R] @ Gm)
    # forward: k = A w, the sampler's sweep without its offset
    k = np.zeros_like(c)
    for cl, parent in preorder:
        if cl not in fac:
            continue
        S, PS, R, T, Gm = fac[cl]
        kc = k[:, off[cl]: off[cl + 1]]
        if len(S):
            kc[:, S] = k[:, off[parent] + PS]
        kc[:, R] = -kc[:, S] @ Gm.T + w[:, off[cl] + R] @ T.T
    return w, k, 0


def s_positions(dims, sepset_clusters, scope_off, scope_idx, pa, ch, nclusters):
    """the entries of the layout at S positions of non-root clusters: the sampler ignores z there, w is +0.0 there"""
    sepcl = np.asarray(sepset_clusters).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum(np.asarray(dims[:nclusters], dtype=np.int64))])
    out = []
    for parent, cl in zip(pa, ch):
        k = next(k for k in range(len(sepcl)) if set(int(v) for v in sepcl[k]) == {int(parent), int(cl)})
        side = 0 if int(sepcl[k][0]) == int(cl) else 1
        out += [int(off[int(cl)] + v) for v in scope_idx[scope_off[2 * k + side]: scope_off[2 * k + side + 1]]]
    return np.array(sorted(out), dtype=int)

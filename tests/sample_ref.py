"""Plain numpy restatement of pgbp_sample_posterior (include/pgbp.h) on arrays, and what the sampler tests share.

sample_posterior_ref is the semantics of the header, line by line: the parent -> child edges of the schedule tree in preorder;
S = the child's variables the sepset to its parent maps to, R = the rest in the child's order; x_S copied from the parent,
x_R = J_RR^-1 (h_R - J_RS x_S) + L^-T z_R with J_RR = L L' (numpy's lower Cholesky factor).  test_sample_cpu.py pins it to the
dense oracle (oracle/densemvn.py: posterior_node_moments, which shares no code with message passing); test_gpu_sample.py
compares the device with it."""
import numpy as np


def sample_size(dims, nclusters):
    return int(np.sum(np.asarray(dims[:nclusters], dtype=np.int64)))


def sample_posterior_ref(records, dims, sepset_clusters, scope_off, scope_idx, pa, ch, z):
    """records[c] = (J, h) of cluster c (the upper triangle of J is read); dims, sepset_clusters [n_sepsets, 2], scope_off,
    scope_idx: the description arrays of pgbp_desc; pa, ch: the preorder edge list (0-based cluster indices);
    z [n_draws, size].  Returns (x [n_draws, size], info): info = 0, or 1 + the first cluster in preorder whose J_RR is not
    positive definite (x is then all NaN)."""
    nc = len(records)
    sepcl = np.asarray(sepset_clusters).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum(np.asarray(dims[:nc], dtype=np.int64))])
    z = np.asarray(z, dtype=np.float64)
    x = np.zeros_like(z)
    pa, ch = [int(a) for a in pa], [int(c) for c in ch]
    root = pa[0] if pa else 0
    assert len(pa) == nc - 1 == len(sepcl), "the sweep is exact on a clique tree only"
    sep_of = {}
    for k, (a, b) in enumerate(sepcl):
        sep_of[(int(a), int(b))] = (k, 0, 1)
        sep_of[(int(b), int(a))] = (k, 1, 0)
    for c, parent in [(root, None)] + list(zip(ch, pa)):
        m = int(dims[c])
        if m == 0:
            continue
        J, h = records[c]
        J = np.triu(J) + np.triu(J, 1).T
        if parent is None:
            S, PS = np.zeros(0, int), np.zeros(0, int)
        else:
            k, cside, pside = sep_of[(c, parent)]
            S = np.asarray(scope_idx[scope_off[2 * k + cside]: scope_off[2 * k + cside + 1]], dtype=int)
            PS = np.asarray(scope_idx[scope_off[2 * k + pside]: scope_off[2 * k + pside + 1]], dtype=int)
        R = np.array([v for v in range(m) if v not in set(S.tolist())], dtype=int)
        xc = x[:, off[c]: off[c + 1]]
        if len(S):
            xc[:, S] = x[:, off[parent] + PS]
        if len(R) == 0:
            continue
        try:
            Lc = np.linalg.cholesky(J[np.ix_(R, R)])
        except np.linalg.LinAlgError:
            return np.full_like(z, np.nan), c + 1
        rhs = h[R][None, :] - xc[:, S] @ J[np.ix_(R, S)].T                       # [n_draws, r]
        mean = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs.T))                 # J_RR^-1 rhs
        noise = np.linalg.solve(Lc.T, z[:, off[c] + R].T)                        # L^-T z_R
        xc[:, R] = (mean + noise).T
    return x, 0


def arrays_from_beliefs(beliefs, nclusters, scopeindex):
    """(records, dims, sepset_clusters, scope_off, scope_idx) of a list of CanonicalBelief objects, clusters first (the oracle's
    or the product's: `scopeindex` is the module's own)."""
    cdict = {beliefs[j].metadata: j for j in range(nclusters)}
    dims = np.array([int(b.h.size) for b in beliefs], dtype=np.int32)
    sepcl, off, idx = [], [0], []
    for j in range(nclusters, len(beliefs)):
        l1, l2 = beliefs[j].metadata
        for c in (cdict[l1], cdict[l2]):
            sepcl.append(c)
            ind = [int(v) for v in scopeindex(beliefs[j], beliefs[c])]
            idx += ind
            off.append(off[-1] + len(ind))
    records = [(np.array(b.J, dtype=float), np.array(b.h, dtype=float)) for b in beliefs[:nclusters]]
    return records, dims, np.array(sepcl, dtype=np.int32).reshape(-1, 2), np.array(off, dtype=np.int64), np.array(idx, dtype=np.int32)


def variable_nodes(beliefs, nclusters):
    """(node, trait) of every entry of a sample: node = the 0-based preorder index (nodelabel - 1), in the order of the layout
    (clusters in index order, a cluster's in-scope variables node after node, trait after trait)."""
    out = []
    for b in beliefs[:nclusters]:
        insc = np.asarray(b.inscope, dtype=bool)
        for k, lab in enumerate(b.nodelabel):
            for t in range(insc.shape[0]):
                if insc[t, k]:
                    out.append((int(lab) - 1, t))
    return out


def law_errors(x, var_nodes, p, pm, pc):
    """x [1 + D, D] = the draws with z = [0; I_D].  Returns (error of the mean, error of the covariance), each relative to the
    largest entry of its reference: x[0] against the dense posterior mean, A'A (A = x[1:] - x[0]: the law's square root, one
    column per variable) against the dense posterior covariance on EVERY pair of entries, across clusters too."""
    flat = np.array([n * p + t for n, t in var_nodes], dtype=int)
    A = x[1:] - x[0]
    cov = A.T @ A
    want_m, want_c = pm[flat], pc[np.ix_(flat, flat)]
    em = float(np.max(np.abs(x[0] - want_m)) / max(np.max(np.abs(want_m)), 1e-300))
    ec = float(np.max(np.abs(cov - want_c)) / max(np.max(np.abs(want_c)), 1e-300))
    return em, ec


def unit_draws(D):
    """z = [0; I_D]"""
    return np.vstack([np.zeros((1, D)), np.eye(D)])

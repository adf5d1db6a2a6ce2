"""Comparator of pgbp_posterior_cov_sites (csrc/pgbp_cov_uni.hip), host side, shared by test_cov_uni_cpu.py and
test_gpu_cov_uni.py (tests only): a numpy restatement of the call's three outputs in its own index convention -- site-minor
rows w, k [n_cols, size, sites], gram [n_cols (n_cols + 1) / 2, sites] -- with the closed forms of a cluster of at most 2
variables (post_uni_ref.sample_rows' coefficients: T00 = 1 / sqrt(J_RR), G = J_RS / J_RR; r = 2: T = L^-T of J = L L'), the
adjoint's summation order (c first, then the children in index order, then their S positions in order) and the block-ordered
gram (per block of 64 entries in index order from 0.0, the blocks added in order from 0.0).

test_cov_uni_cpu.py pins it to cov_ref.posterior_cov_ref (the restatement of the general call) and to the dense posterior
covariance of the oracle (post_uni_ref.dense_posterior); neither is the code under test."""
import functools

import numpy as np

import post_uni_ref as PR

BLOCK = 64   # kFamUniBlock: entries per block of gram


def cov_rows(records, dims, sepset_clusters, scope_off, scope_idx, pa, ch, c):
    """One site: records[cl] = (J, h[, g]) of cluster cl (the upper triangle of J is read), c [n_cols, size].
    Returns (w [n_cols, size], k [n_cols, size], info) with the conventions of cov_ref.posterior_cov_ref."""
    nc = len(records)
    sepcl = np.asarray(sepset_clusters).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum(np.asarray(dims[:nc], dtype=np.int64))])
    c = np.atleast_2d(np.asarray(c, float))
    pa, ch = [int(a) for a in pa], [int(b) for b in ch]
    root = pa[0] if pa else 0
    sep_of = {}
    for q, (a, b) in enumerate(sepcl):
        sep_of[(int(a), int(b))] = (q, 0, 1)
        sep_of[(int(b), int(a))] = (q, 1, 0)
    plan = []
    for cl, parent in [(root, None)] + list(zip(ch, pa)):
        m = int(dims[cl])
        if m == 0:
            continue
        J = records[cl][0]
        S = PS = []
        if parent is not None:
            q, cs, ps = sep_of[(cl, parent)]
            S = [int(v) for v in scope_idx[scope_off[2 * q + cs]: scope_off[2 * q + cs + 1]]]
            PS = [int(v) for v in scope_idx[scope_off[2 * q + ps]: scope_off[2 * q + ps + 1]]]
        R = [v for v in range(m) if v not in S]
        T00 = T01 = T11 = G = 0.0
        ok = True
        if len(R) == 2:
            a, b, d = J[0, 0], J[0, 1], J[1, 1]
            ba = b / a if a != 0 else np.nan
            sc = d - ba * b
            ok = a > 0 and sc > 0
            if ok:
                T00, T11 = 1.0 / np.sqrt(a), 1.0 / np.sqrt(sc)
                T01 = -(ba * T11)
        elif len(R) == 1:
            Jrr = J[R[0], R[0]]
            ok = Jrr > 0
            if ok:
                T00 = 1.0 / np.sqrt(Jrr)
                if S:
                    G = J[min(R[0], S[0]), max(R[0], S[0])] / Jrr
        if not ok:
            return np.full_like(c, np.nan), np.full_like(c, np.nan), cl + 1
        plan.append((cl, parent, R, S, PS, T00, T01, T11, G))
    # adjoint: every child before its parent; what an entry gathers is kept with (child, j) and added in that order
    w = np.zeros_like(c)
    taken = {}
    for cl, parent, R, S, PS, T00, T01, T11, G in reversed(plan):
        xb = {}
        for v in R + S:
            acc = c[:, off[cl] + v].copy()
            for _, _, t in sorted(taken.get(int(off[cl]) + v, []), key=lambda x: x[:2]):
                acc = acc + t
            xb[v] = acc
        if len(R) == 2:
            w[:, off[cl] + R[0]] = T00 * xb[R[0]]
            w[:, off[cl] + R[1]] = T01 * xb[R[0]] + T11 * xb[R[1]]
        elif len(R) == 1:
            w[:, off[cl] + R[0]] = T00 * xb[R[0]]
        for j, v in enumerate(S):
            t = xb[v] - G * xb[R[0]] if R else xb[v]
            taken.setdefault(int(off[parent]) + PS[j], []).append((cl, j, t))
    # forward: the sampler's sweep without its offset, w for z
    k = np.zeros_like(c)
    for cl, parent, R, S, PS, T00, T01, T11, G in plan:
        kc = k[:, off[cl]: off[cl + 1]]
        wc = w[:, off[cl]: off[cl + 1]]
        for j, v in enumerate(S):
            kc[:, v] = k[:, off[parent] + PS[j]]
        if len(R) == 2:
            kc[:, R[0]] = T00 * wc[:, R[0]] + T01 * wc[:, R[1]]
            kc[:, R[1]] = T11 * wc[:, R[1]]
        elif len(R) == 1:
            kc[:, R[0]] = -(G * kc[:, S[0]]) + T00 * wc[:, R[0]] if S else T00 * wc[:, R[0]]
    return w, k, 0


def gram_rows(w):
    """w [n_cols, size, sites] -> gram [n_cols (n_cols + 1) / 2, sites]: pair (a <= b) at b (b + 1) / 2 + a; per block of 64 entries
    the products are added in index order from 0.0, then the blocks in order from 0.0 -- the device's order, no fused
    multiply-add"""
    w = np.asarray(w, float)
    nc, size, ns = w.shape
    out = np.zeros((nc * (nc + 1) // 2, ns))
    for b in range(nc):
        for a in range(b + 1):
            total = np.zeros(ns)
            for e0 in range(0, size, BLOCK):
                acc = np.zeros(ns)
                for e in range(e0, min(e0 + BLOCK, size)):
                    acc = acc + w[a, e] * w[b, e]
                total = total + acc
            out[b * (b + 1) // 2 + a] = total
    return out


def gram_full(tri, nc):
    """the packed rows [n_cols (n_cols + 1) / 2, sites] as [sites, n_cols, n_cols]"""
    tri = np.asarray(tri)
    G = np.empty((tri.shape[1], nc, nc))
    for b in range(nc):
        for a in range(b + 1):
            G[:, a, b] = G[:, b, a] = tri[b * (b + 1) // 2 + a]
    return G


def posterior_cov_sites_rows(records_by_site, dims, sepset_clusters, scope_off, scope_idx, pa, ch, c):
    """The call's outputs for the sites of `records_by_site` (a list over sites of the records of the clusters):
    (w [n_cols, size, sites], k [n_cols, size, sites], gram [n_cols (n_cols + 1) / 2, sites], info [sites])"""
    c = np.atleast_2d(np.asarray(c, float))
    ns = len(records_by_site)
    w, k = np.zeros(c.shape + (ns,)), np.zeros(c.shape + (ns,))
    info = np.zeros(ns, np.int32)
    for s, rec in enumerate(records_by_site):
        w[:, :, s], k[:, :, s], info[s] = cov_rows(rec, dims, sepset_clusters, scope_off, scope_idx, pa, ch, c)
    return w, k, gram_rows(w), info


# ----------------------------------------------------------------------------- the cases and the functionals both files use

# the shapes of post_uni_ref.SHAPES, and trees whose layout size falls on either side of a multiple of 64 entries (the blocks
# of gram): 63 | 66 around 64, 191 | 192 | 194 around 192 (192: the 130 families of SHAPES)
SHAPES = list(PR.SHAPES) + [("families", 44), ("families", 46), ("families", 145), ("families", 147)]
SIZES = {("families", 44): 63, ("families", 46): 66, ("families", 145): 191, ("families", 130): 192, ("families", 147): 194}


@functools.lru_cache(maxsize=None)
def functionals(size, n_cols=3, seed=2001):
    """c [n_cols, size]: column 0 random on every entry, column 1 a contrast of the first and the last entry, the others random
    and sparse; every column has weight on the entries on both sides of each 64-entry boundary that the layout has"""
    rng = np.random.default_rng(seed + size)
    c = np.zeros((n_cols, size))
    c[0] = rng.standard_normal(size)
    if n_cols > 1:
        c[1, 0], c[1, size - 1] = 1.0, -1.0
    for a in range(2, n_cols):
        on = rng.random(size) < 0.25
        c[a, on] = rng.standard_normal(int(on.sum()))
    for e in range(BLOCK, size, BLOCK):
        for a in range(n_cols):
            c[a, e - 1] += 0.5 + a
            c[a, e] -= 0.25 + a
    c.flags.writeable = False   # (shared by the tests)
    return c

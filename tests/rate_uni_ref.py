"""Cases and comparators of the evolutionary rate matrix between the sites of a univariate batch (pgbp_bm_rate_matrix_sites /
bm_rate_matrix_sites / calibrate_rate_matrix_sites_ / phylo_pca_sites), host side, shared by test_rate_uni_cpu.py and
test_gpu_rate_uni.py (tests only).  None of them runs the code under test.

(a) `u_rows`: a numpy restatement of the residual rows for ONE site -- per family that is not skipped t = sum gamma^2 length,
    r = x_child - sum gamma_k x_k - d (d: the shifts' displacement), u = E[r] / sqrt(t), +0.0 at a skipped family -- over the
    DENSE flat-prior posterior means of all node states (site_missing_ref.dense_moments, as exact_uni_ref.sweep takes them);
    `gram` = U'U over the sites of a case.
(b) `gls`: dense generalised least squares on the observed tips: Y'PY with P = C^-1 - C^-1 1 1' C^-1 / (1' C^-1 1) built from
    the tips' covariance of oracle.densemvn (site_missing_ref.bm_cov), the shifts' displacement taken off the data; and,
    written separately, R_hat = Y_c' C^-1 Y_c / (n - 1) with Y_c = Y - 1 mu_hat'.
(c) the cases: those of exact_uni_ref without a per-site mask, and this module's own: trees of 2 and 3 tips, tips without data
    at every site (a shared child_mask), shifts shared by the sites."""
import functools
import types

import numpy as np

import exact_uni_ref as XR
import fam_uni_ref as FR
import site_missing_ref as SM
from oracle import network as ON


# ----------------------------------------------------------------------------- (a) the restatement

def u_rows(case, s):
    """[n_families] of site s: e / sqrt(t), 0.0 at the skipped families"""
    fam = case.fam
    K, nf = max(1, int(fam["max_parents"])), len(fam["cluster"])
    shifts = {f * K + k: v for (f, k), v in FR.site_shifts(case, s).items()}
    cm, pm = fam.get("child_mask"), fam.get("parent_mask")
    vals = case.sites[s][1][0]
    mom = SM.dense_moments(case, s)
    u = np.zeros(nf)
    for f in range(nf):
        npar, cpos = int(fam["n_parents"][f]), int(fam["child_pos"][f])
        t = 0.0
        for k in range(npar):
            g = float(fam["gamma"][f * K + k])
            t = t + g * g * float(fam["length"][f * K + k])
        if npar == 0 or t == 0.0 or (cm is not None and not int(cm[f]) & 1):
            continue
        if cpos < 0 and pm is not None and int(pm[f * K]) == 0:
            continue
        m, _ = mom(int(fam["cluster"][f]))
        if len(m) == 0:
            continue
        c = np.zeros(len(m))
        cst = 0.0
        if cpos >= 0:
            c[cpos] = 1.0
        else:
            cst = float(vals[int(fam["data_row"][f])])
        d = 0.0
        for k in range(npar):
            g = float(fam["gamma"][f * K + k])
            c[int(fam["parent_pos"][f * K + k])] -= g
            d = d + g * shifts.get(f * K + k, 0.0)
        u[f] = (float(c @ m) + cst - d) / np.sqrt(t)
    return u


@functools.lru_cache(maxsize=None)
def U(key, n):
    """[n_families, n]: u_rows of the first n sites of case `key` (computed once per case and site count)"""
    case = get(key, n)
    return np.stack([u_rows(case, s) for s in range(n)], axis=1)


def gram(key, n):
    u = U(key, n)
    return u.T @ u


# ----------------------------------------------------------------------------- (b) dense GLS

def observed_rows(case):
    """the data rows every site observes (a shared pattern: None marks a tip without data)"""
    return np.array([r for r, v in enumerate(case.sites[0][1][0]) if v is not None], dtype=int)


@functools.lru_cache(maxsize=None)
def gls(key, n):
    """dict(gram = Y'PY, R = Y_c' C^-1 Y_c / (n_obs - 1), mu [n], n_obs, Y [n_obs, n], Yc) of the first n sites"""
    case = get(key, n)
    obs = observed_rows(case)
    Y = np.stack([np.array([float(case.sites[s][1][0][r]) for r in obs]) - XR.tip_displacement(case, s)[obs] for s in range(n)], axis=1)
    C = case.cov[np.ix_(obs, obs)]
    Ci = np.linalg.inv(C)
    one = np.ones(len(obs))
    Ci1 = Ci @ one
    P = Ci - np.outer(Ci1, Ci1) / float(one @ Ci1)
    mu = (Ci1 @ Y) / float(one @ Ci1)
    Yc = Y - mu[None, :]
    return dict(gram=Y.T @ P @ Y, R=Yc.T @ np.linalg.solve(C, Yc) / (len(obs) - 1), mu=mu, n_obs=len(obs), Y=Y, Yc=Yc)


def eigengap(A, k):
    """the smallest gap between the k + 1 largest eigenvalues of A, relative to the largest"""
    w = np.sort(np.linalg.eigvalsh(A))[::-1]
    return float(np.min(-np.diff(w[: k + 1])) / w[0])


def pca(A, Yc, k, scale=None):
    """(values [k] decreasing, loadings [n, k], scores [n_obs, k]) of the dense matrix A by numpy.linalg.eigh"""
    w, V = np.linalg.eigh(A)
    order = np.argsort(w)[::-1][:k]
    Z = Yc if scale is None else Yc / scale[None, :]
    return w[order], V[:, order], Z @ V[:, order]


def aligned(V, W):
    """V with the sign of every column set so that it agrees with the column of W"""
    return V * np.where(np.sum(V * W, axis=0) < 0, -1.0, 1.0)[None, :]


# ----------------------------------------------------------------------------- (c) the cases

@functools.lru_cache(maxsize=None)
def tiny(ntips, n=17):
    """trees of 2 and 3 tips, n sites of standard normal data"""
    nwk = {2: "(t0:0.7,t1:1.1);", 3: "((t0:0.4,t1:0.9):0.6,t2:1.3);"}[ntips]
    net = ON.read_newick(nwk)
    taxa = list(net.tip_names)
    X = np.random.default_rng(2400 + ntips).normal(size=(n, len(taxa)))
    return XR._pair(f"tree{ntips}", net, taxa, X)


@functools.lru_cache(maxsize=None)
def shared_missing(n=65):
    """the 30-tip random tree with three tips without data at every site: a shared child_mask"""
    b = XR.random30()
    gone = (2, 11, 23)
    values = [[None if r in gone else float(v) for r, v in enumerate(tbl[0])] for _, tbl in b.sites[:n]]
    free = FR._case("random30, three tips without data", b.net, b.taxa, [(XR._bm(np.inf), [v]) for v in values])
    free.root_node, free.root, free.cov, free.mask, free.n = b.root_node, None, b.cov, None, n
    from post_uni_ref import layout
    _, _, _, _, vn, off = layout(free)
    c = next(c for c in range(len(off) - 1) if any(nd == free.root_node for nd, _ in vn[off[c]: off[c + 1]]))
    free.root = (c, [nd for nd, _ in vn[off[c]: off[c + 1]]].index(free.root_node))
    assert free.fam.get("child_mask") is not None
    return free


@functools.lru_cache(maxsize=None)
def shared_shifts(n):
    """bm40 with the same shift values at every site, on the two edges of exact_uni_ref.shifted"""
    b = XR.shifted(n, False)
    c = types.SimpleNamespace(**b.__dict__)
    c.shifts = (b.shifts[0], np.tile(np.array([[1.5, -2.25]]), (len(b.shifts[1]), 1)))
    c.name = "bm40 + shared shifts"
    return c


@functools.lru_cache(maxsize=None)
def get(key, n):
    """exact_uni_ref.get, and "tree2" | "tree3" | "missing" | "shifts_shared" """
    if key in ("tree2", "tree3"):
        base = tiny(int(key[-1]))
    elif key == "missing":
        base = shared_missing()
    elif key == "shifts_shared":
        return shared_shifts(n)
    else:
        return XR.get(key, n)
    c = types.SimpleNamespace(**base.__dict__)
    c.sites, c.n = base.sites[:n], n
    return c


# CPU: (key, sites) -- trees of 2, 3, 12 (caterpillar, balanced) and 30 tips, 40 tips; a shared child_mask; shifts per site and shared
CPU_CASES = [("tree2", 9), ("tree3", 9), ("caterpillar12", 16), ("balanced12", 16), ("random30", 17), ("bm40", 17),
             ("missing", 17), ("shifts", 17), ("shifts_shared", 17)]
# GPU sites: 8 plain; 16, 17, 63, 64, 65 tile and wavefront edges (site-minor from 64); 257 a second workgroup of phase one
SITE_CASES = [("bm40", n) for n in (8, 16, 17, 63, 64, 65, 257)]
# GPU families: 2 tips (fewer terms than one MFMA step), 63 / 64 / 65 / 130 families (chunk and padding boundaries)
FAMILY_CASES = [("tree2", 17), ("families63", 64), ("families64", 64), ("families65", 64), ("families130", 64)]
OTHER_CASES = [("missing", 65), ("shifts", 64), ("shifts_shared", 17), ("tree3", 9)]
PCA_CASE, PCA_K = ("bm40", 8), 3

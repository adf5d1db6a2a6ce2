"""calibrate_exact_cliquetree_: the closed-form REML fit of a Brownian motion (src/calibration.jl:404-517) on the device --
two calibrations, the posterior moments of the clusters and one sweep over the node families (pgbp_bm_exact_stats).  No
test here calls an optimiser."""
import ctypes as C

import numpy as np
import pytest

from helpers import goldens

pytestmark = pytest.mark.gpu
G = goldens()


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _engines(P, netstr, taxa, data, p, n_sites=1, fixed=True, masked=False):
    """Improper-root engine (+ fixed-root engine) on the clique tree of a network; data [n_rows, p] or [n_sites, n_rows, p]."""
    net, names = P.read_newick(netstr)
    row = {t: r for r, t in enumerate(taxa)}
    data_row = [row.get(names[i], -1) for i in range(net.nnodes)]
    cn, ed, sn = P.cliquetree(net.node2family)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    data = np.asarray(data, float)
    pattern = data if data.ndim == 2 else data[0]
    out = []
    for fixedroot in ((False, True) if fixed else (False,)):
        kw = dict(data=pattern, data_row=data_row) if masked else {}
        st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=fixedroot, **kw)
        fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, data_row, p,
                            **(dict(data=pattern) if masked else {}))
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=n_sites)
        cgb.lg_setup(fam, data)
        out.append((st, fam, cgb))
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    st = out[0][0]
    ci = next(i for i, c in enumerate(cn) if 1 in c and st.dims[i] > 0)      # the root (label 1) is listed last in its cluster
    return out, spt, (ci, int(st.dims[ci]) - p)


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ----------------------------------------------------------------------------- 5: the reference's own values

@pytest.mark.parametrize("traits", ["uni", "bi"])
def test_exact_reml_level1_closed_form(P, traits):
    """test/test_exactBM.jl:185-226 at 1e-8 relative (the reference compares with rtol 1.5e-8)."""
    g = G["exact_reml_level1"]
    cols = [g["y"]] if traits == "uni" else [g["x"], g["y"]]
    p = len(cols)
    (free, fixed), spt, root = _engines(P, g["net"], g["taxa"], np.array(cols, float).T.copy(), p)
    R, mu, ll = P.calibrate_exact_cliquetree_(free[2], spt, root, fixed[2])
    want = g[traits]
    print(traits, "R", R.tolist(), "mu", mu.tolist(), "ll", ll)
    if traits == "uni":
        assert abs(R[0, 0] - want["sigma2"]) <= 1e-8 * want["sigma2"], (R, want)
        assert abs(mu[0] - want["mu"]) <= 1e-8 * abs(want["mu"]), (mu, want)
        assert abs(ll - want["ll"]) <= 1e-8 * abs(want["ll"]), (ll, want)
    else:
        assert np.all(np.abs(R - np.array(want["R"])) <= 1e-8 * np.abs(np.array(want["R"]))), (R, want)
        assert np.all(np.abs(mu - np.array(want["mu"])) <= 1e-8 * np.abs(np.array(want["mu"]))), (mu, want)
        assert np.isfinite(ll)
    # without the fixed-root engine the score is nan, the estimates the same bytes
    R2, mu2, ll2 = P.calibrate_exact_cliquetree_(free[2], spt, root)
    assert np.isnan(ll2) and np.array_equal(R2, R) and np.array_equal(mu2, mu)


def test_exact_reml_missing_closed_form(P):
    """test/test_exactBM.jl:228-251: x missing at two sister tips, their parent has nothing in scope (families skipped)."""
    g = G["exact_reml_missing"]
    data = np.array([[np.nan if v is None else float(v)] for v in g["x"]])
    (free, fixed), spt, root = _engines(P, g["net"], g["taxa"], data, 1, masked=True)
    R, mu, ll = P.calibrate_exact_cliquetree_(free[2], spt, root, fixed[2])
    print("missing: sigma2", R[0, 0], "mu", mu[0], "ll", ll)
    assert abs(R[0, 0] - g["sigma2"]) <= 1e-8 * g["sigma2"], (R, g["sigma2"])
    assert abs(mu[0] - g["mu"]) <= 1e-8 * abs(g["mu"]), (mu, g["mu"])
    assert abs(ll - g["ll"]) <= 1e-8 * abs(g["ll"]), (ll, g["ll"])


# ----------------------------------------------------------------------------- 6, 7, 8 on random trees

def _random_tree(ntips, seed):
    from pgbp_amd import synth as S
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)             # branch lengths in [0.1, 1]
    names = [f"n{i}" for i in range(tr.nnodes)]
    taxa = [names[i] for i in range(tr.nnodes) if tr.is_leaf[i]]
    return S, rng, tr, tr.newick(names), taxa


def _shared_path_matrix(tr):
    """V[a, b] = length of the path the tips a and b share from the root (tips in node order), from the tree arrays."""
    N = tr.nnodes
    assert np.all(np.asarray(tr.parent[1:]) < np.arange(1, N))          # parents come first
    tip_rank = -np.ones(N, int)
    tip_rank[np.asarray(tr.is_leaf, bool)] = np.arange(int(np.sum(tr.is_leaf)))
    below = [[] for _ in range(N)]
    for i in range(N - 1, 0, -1):
        if tr.is_leaf[i]:
            below[i].append(tip_rank[i])
        below[tr.parent[i]].extend(below[i])
    n = int(np.sum(tr.is_leaf))
    V = np.zeros((n, n))
    for i in range(1, N):
        ix = np.array(below[i])
        V[np.ix_(ix, ix)] += tr.length[i]
    return V


def _gls(V, Y, dtype):
    """mu_hat = (1'V^-1 1)^-1 1'V^-1 Y, R_hat = r'V^-1 r / (n - 1) through a Cholesky factor in `dtype`."""
    V = np.asarray(V, dtype)
    Y = np.asarray(Y, dtype)
    n = V.shape[0]
    Lc = np.zeros((n, n), dtype)
    for j in range(n):
        v = V[j:, j] - Lc[j:, :j] @ Lc[j, :j]
        Lc[j:, j] = v / np.sqrt(v[0])
    B = np.concatenate([np.ones((n, 1), dtype), Y], axis=1)
    Z = np.zeros_like(B)                       # L Z = [1 | Y]
    for i in range(n):
        Z[i] = (B[i] - Lc[i, :i] @ Z[:i]) / Lc[i, i]
    one, Zy = Z[:, 0], Z[:, 1:]
    mu = (one @ Zy) / (one @ one)
    Zr = Zy - np.outer(one, mu)
    return mu, (Zr.T @ Zr) / (n - 1)


def test_exact_estimator_equals_gls_on_a_tree(P):
    """For a BM on a tree the estimator is generalised least squares (test/test_exactBM.jl:228-248, commented block).
    Random tree of 2 000 tips (seed 5), p = 1 and p = 4, 1e-8 relative (norm-wise for R_hat); the float64 GLS reference
    agrees with the numpy.longdouble GLS on the same V to the figure printed and asserted below (<= 1e-10)."""
    S, rng, tr, nwk, taxa = _random_tree(2000, 5)
    V = _shared_path_matrix(tr)
    A = rng.standard_normal((4, 4))
    X = S.simulate_bm(tr, A @ A.T + np.eye(4), rng.standard_normal(4), rng)
    Y4 = X[np.asarray(tr.is_leaf, bool)]
    mu64, R64 = _gls(V, Y4, np.float64)
    mul, Rl = _gls(V, Y4, np.longdouble)
    head = max(_rel(mu64, mul.astype(float)), float(np.linalg.norm(R64 - Rl.astype(float)) / np.linalg.norm(R64)))
    print(f"float64 GLS vs longdouble GLS: {head:.2e}")
    assert head <= 1e-10
    for p in (1, 4):
        Y = Y4[:, :p].copy()
        (free,), spt, root = _engines(P, nwk, taxa, Y, p, fixed=False)
        R, mu, _ = P.calibrate_exact_cliquetree_(free[2], spt, root)
        e_mu = _rel(mu, mu64[:p])
        e_R = float(np.linalg.norm(R - R64[:p, :p]) / np.linalg.norm(R64[:p, :p]))
        print(f"p={p}: mu_hat {e_mu:.2e}, R_hat {e_R:.2e} from GLS")
        assert e_mu <= 1e-8 and e_R <= 1e-8


def _host_sweep(fam, moments, data, p):
    """The family loop of src/calibration.jl:442-499 in numpy on moments_ output (mu, Sigma per cluster)."""
    K = int(fam["max_parents"])
    num, den = np.zeros((p, p)), 0.0
    for f in range(len(fam["cluster"])):
        npar = int(fam["n_parents"][f])
        if npar == 0:
            continue
        gam = fam["gamma"][f * K: f * K + npar]
        t = 0.0
        for k in range(npar):
            t += gam[k] * gam[k] * fam["length"][f * K + k]
        if t == 0.0:
            continue
        mu, vv, _ = moments[int(fam["cluster"][f])]
        cm = int(fam["child_mask"][f]) if "child_mask" in fam else -1
        pm = [int(fam["parent_mask"][f * K + k]) if "parent_mask" in fam else -1 for k in range(npar)]
        ppos = fam["parent_pos"][f * K: f * K + npar]
        if fam["child_pos"][f] < 0 and fam["data_row"][f] >= 0:       # tip
            if pm[0] == 0 or cm == 0:
                continue
            d = mu[ppos[0]: ppos[0] + p] - data[int(fam["data_row"][f])]
            num += np.outer(d, d) / t
            den += 1 - vv[0, 0] / t
        else:
            if cm == 0 or fam["child_pos"][f] < 0:
                continue
            c = int(fam["child_pos"][f])
            d = mu[c: c + p].copy()
            dvar = vv[c, c]
            for k1 in range(npar):
                d -= gam[k1] * mu[ppos[k1]: ppos[k1] + p]
                dvar -= 2 * gam[k1] * vv[c, ppos[k1]]
                for k2 in range(npar):
                    dvar += gam[k1] * gam[k2] * vv[ppos[k1], ppos[k2]]
            num += np.outer(d, d) / t
            den += 1 - dvar / t
    return num, den


@pytest.mark.parametrize("case", ["level1_bi", "missing", "tree_p4", "tree_p16"])
def test_device_sweep_against_host_restatement(P, case):
    """num, den of pgbp_bm_exact_stats against the numpy restatement on moments_ of the same calibrated engine: 1e-12
    relative (same inputs; only the summation order differs)."""
    masked = False
    if case == "level1_bi":
        g = G["exact_reml_level1"]
        p, nwk, taxa, data = 2, g["net"], g["taxa"], np.array([g["x"], g["y"]], float).T.copy()
    elif case == "missing":
        g = G["exact_reml_missing"]
        p, nwk, taxa, masked = 1, g["net"], g["taxa"], True
        data = np.array([[np.nan if v is None else float(v)] for v in g["x"]])
    else:
        p = 4 if case == "tree_p4" else 16
        S, rng, tr, nwk, taxa = _random_tree(600, 21 + p)
        data = S.simulate_bm(tr, S.random_rate_matrix(p, rng), np.zeros(p), rng)[np.asarray(tr.is_leaf, bool)]
    (free,), spt, root = _engines(P, nwk, taxa, data, p, fixed=False, masked=masked)
    st, fam, cgb = free
    cgb.assignfactors_lg_(np.eye(p)[None], np.zeros(p), sync=True)
    assert P.calibrate_(cgb, [spt])[0]
    num, den = P.bm_exact_stats(cgb)
    dims = [int(d) for d in st.dims[: cgb.nclusters]]
    listed = [c for c in range(cgb.nclusters) if dims[c] > 0]
    mom = dict(zip(listed, cgb.moments_(listed)))
    for c in range(cgb.nclusters):
        mom.setdefault(c, (np.zeros(0), np.zeros((0, 0)), 0.0))
    hnum, hden = _host_sweep(fam, mom, np.nan_to_num(data), p)
    nfam = len(fam["cluster"])
    e_num, e_den = float(np.max(np.abs(num - hnum)) / np.max(np.abs(hnum))), abs(den - hden) / abs(hden)
    print(f"{case}: {nfam} families, num {e_num:.2e}, den {e_den:.2e}")
    assert e_num <= 1e-12 and e_den <= 1e-12, (nfam, e_num, e_den)
    num2, den2 = P.bm_exact_stats(cgb)
    assert np.array_equal(num, num2) and den == den2            # no atomics on doubles: the same bytes again


@pytest.mark.parametrize("p", [2, 1])
def test_exact_estimator_batch_of_sites(P, p):
    """64 sites with different data on one tree, all_sites=True, against the one-site run of each site's data: bit for
    bit for p = 2 (same state layout), 1e-12 relative for p = 1 (the batch calibrates in the site-minor layout).
    Relative means: R_hat and the score against their own size; mu_hat, a weighted mean of the tip values that passes
    through zero, against the largest tip value of the site -- the scale its rounding error is proportional to.  (Against
    |mu_hat| itself a site whose estimate happens to be 1.5e-4 on data of size 5 showed 7e-12 for an absolute
    difference of 1e-15; the other 63 sites at most 9e-16.)"""
    ns = 64
    S, rng, tr, nwk, taxa = _random_tree(40, 9)
    leaf = np.asarray(tr.is_leaf, bool)
    data = np.stack([S.simulate_bm(tr, S.random_rate_matrix(p, rng), rng.standard_normal(p), rng)[leaf] for _ in range(ns)])
    (free, fixed), spt, root = _engines(P, nwk, taxa, data, p, n_sites=ns)
    R, mu, ll = P.calibrate_exact_cliquetree_(free[2], spt, root, fixed[2], all_sites=True)
    assert R.shape == (ns, p, p) and mu.shape == (ns, p) and ll.shape == (ns,) and np.all(np.isfinite(ll))
    assert not np.array_equal(R[0], R[1])
    (f1, x1), spt1, root1 = _engines(P, nwk, taxa, data[0], p)
    worst = 0.0
    for s in range(ns):
        f1[2].lg_setup(f1[1], data[s])
        x1[2].lg_setup(x1[1], data[s])
        R1, mu1, ll1 = P.calibrate_exact_cliquetree_(f1[2], spt1, root1, x1[2])
        if p >= 2:
            assert np.array_equal(R[s], R1) and np.array_equal(mu[s], mu1) and ll[s] == ll1, s
        else:
            errs = (_rel(R[s], R1), float(np.max(np.abs(mu[s] - mu1)) / np.max(np.abs(data[s]))), abs(ll[s] - ll1) / abs(ll1))
            worst = max(worst, *errs)
    if p == 1:
        print(f"site-minor batch against one-site runs: {worst:.2e}")
        assert worst <= 1e-12


def test_exact_estimator_failure_paths(P):
    g = G["exact_reml_level1"]
    data = np.array([g["x"], g["y"]], float).T.copy()
    (free, fixed), spt, root = _engines(P, g["net"], g["taxa"], data, 2)
    # a fixed-root engine
    with pytest.raises(P.PgbpError, match="fixed root") as ei:
        P.calibrate_exact_cliquetree_(fixed[2], spt, root)
    assert ei.value.code == 1
    # a family table never set up
    st = free[0]
    bare = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    with pytest.raises(P.PgbpError, match="pgbp_lg_setup") as ei:
        P.calibrate_exact_cliquetree_(bare, spt, root)
    assert ei.value.code == 6
    # partial scopes: one trait missing at one tip
    part = data.copy()
    part[1, 0] = np.nan
    (pf,), spt2, _ = _engines(P, g["net"], g["taxa"], part, 2, fixed=False, masked=True)
    num, den, info = np.full(4, 7.0), np.full(1, 7.0), np.zeros(1, np.int32)
    rc = pf[2]._lib.pgbp_bm_exact_stats(pf[2]._eng, 0, 1, num.ctypes.data_as(C.POINTER(C.c_double)),
                                        den.ctypes.data_as(C.POINTER(C.c_double)), info.ctypes.data_as(C.POINTER(C.c_int32)))
    msg = pf[2]._lib.pgbp_last_error(pf[2]._eng).decode()
    assert rc == 1 and msg.startswith("some leaf must have partial data: cluster") and msg.endswith("has partial traits in scope")
    assert np.all(num == 7.0) and den[0] == 7.0                  # nothing launched, nothing written

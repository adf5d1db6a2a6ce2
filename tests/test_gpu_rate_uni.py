"""pgbp_bm_rate_matrix_sites (csrc/pgbp_rate_uni.hip) and its wrappers bm_rate_matrix_sites, calibrate_rate_matrix_sites_ and
phylo_pca_sites: the evolutionary rate matrix between the sites of a univariate batch, U'U on the matrix cores.

Comparators, never the new kernels themselves: the numpy restatement of tests/rate_uni_ref.py over the dense flat-prior
posterior and dense GLS on the tips (pinned to each other in test_rate_uni_cpu.py); pgbp_bm_exact_stats_sites on the same
beliefs for the diagonal, den, mu and info; calibrate_exact_cliquetree_ on a multivariate engine that holds the sites as
traits.  Every comparison is asserted at 1e-8 relative to max(1, |block|_max); each test prints its worst figure."""
import ctypes as C
import types

import numpy as np
import pytest

import exact_uni_ref as XR
import fam_uni_ref as FR
import rate_uni_ref as RR
from test_gpu_exact_uni import _calibrate
from test_gpu_fam_uni import _engine, _layout

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _rel(got, want):
    return FR.rel(got, want)


def _calibrated(P, key, n, R=None):
    case = RR.get(key, n)
    cgb = _engine(P, case, n)
    o = _calibrate(cgb, case.spt, R)
    return case, cgb, o


def _raw(cgb, rows, cols, root, want_mu=True, null_gram=False, timed=None):
    """the C call: (rc, [gram, den, mu, info]) with sentinel-filled outputs"""
    from pgbp_amd import _lib as L
    nr, nc = max(0, rows[1] - rows[0]), max(0, cols[1] - cols[0])
    out = [np.full((nr, nc), 7.0), np.full(nr + nc, 7.0), np.full(nr + nc, 7.0), np.full(nr + nc, 7, np.int32)]
    args = [cgb._eng, rows[0], rows[1], cols[0], cols[1], int(root[0]), int(root[1]), None if null_gram else L.f64p(out[0]),
            L.f64p(out[1]), L.f64p(out[2]) if want_mu else None, L.i32p(out[3])]
    if timed is not None:
        return cgb._lib.pgbp_bm_rate_matrix_sites_timed(*args, L.f64p(timed)), out
    return cgb._lib.pgbp_bm_rate_matrix_sites(*args), out


def _same(x, y):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


# ----------------------------------------------------------------------------- 1: against the restatement and dense GLS

EVERY = RR.SITE_CASES + RR.FAMILY_CASES + RR.OTHER_CASES


@pytest.mark.parametrize("key,n", EVERY, ids=[f"{k}-{n}" for k, n in EVERY])
def test_against_the_restatement_and_gls(P, key, n):
    """gram on every pair of sites against U'U of the restatement and against Y'PY of dense GLS; R_hat against
    Y_c' C^-1 Y_c / (n - 1); den, mu, info; gram symmetric to the byte.  Sites 8: the plain layout; 16 .. 65: tile and wavefront
    edges; 257: a second workgroup of phase one and a third tile; 2 tips: fewer families than one MFMA step; 63 .. 130
    families: padding rows and a second and third block."""
    case, cgb, _ = _calibrated(P, key, n)
    lay = _layout(cgb)
    assert bool(lay & 2) == (n >= 64)
    gram, den, mu, info = P.bm_rate_matrix_sites(cgb, root=case.root)
    assert _layout(cgb) == lay and not info[0].any() and not info[1].any()
    assert _same([den[0], mu[0], info[0]], [den[1], mu[1], info[1]])
    g = RR.gls(key, n)
    R = gram / np.sqrt(np.outer(den[0], den[1]))
    worst = dict(restatement=_rel(gram, RR.gram(key, n)), gls=_rel(gram, g["gram"]), R=_rel(R, g["R"]),
                 den=_rel(den[0], np.full(n, g["n_obs"] - 1.0)), mu=_rel(mu[0], g["mu"]))
    print(f"{key}/{n}: {len(case.fam['cluster'])} families, {n} x {n}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL
    assert np.array_equal(gram, gram.T)


# ----------------------------------------------------------------------------- 2: against the per-site call

@pytest.mark.parametrize("key,n", [("bm40", 65), ("families130", 64), ("shifts", 64), ("missing", 65), ("tree2", 17), ("bm40", 8)])
def test_against_the_per_site_call(P, key, n):
    """the diagonal of gram against num of pgbp_bm_exact_stats_sites on the same beliefs; den, mu and info against it too"""
    case, cgb, _ = _calibrated(P, key, n)
    gram, den, mu, info = P.bm_rate_matrix_sites(cgb, root=case.root)
    num, sden, smu, sinfo = P.bm_exact_stats_sites(cgb, case.root)
    worst = dict(diag=_rel(np.diagonal(gram), num), den=_rel(den[0], sden), mu=_rel(mu[0], smu))
    print(f"{key}/{n}: against pgbp_bm_exact_stats_sites: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) +
          f"; den and mu the same bytes: {np.array_equal(den[0], sden) and np.array_equal(mu[0], smu)}")
    assert max(worst.values()) <= TOL and np.array_equal(info[0], sinfo)


# ----------------------------------------------------------------------------- 3: against the multivariate engine

@pytest.mark.parametrize("p", [8, 16])
def test_against_the_multivariate_engine(P, p):
    """R_hat and mu_hat of p sites against calibrate_exact_cliquetree_ on an engine that holds the same data as p traits
    (pgbp_bm_exact_stats: none of the new code, and independent of the restatement)"""
    from pgbp_amd import synth
    from test_gpu_exact_bm import _engines
    rng = np.random.default_rng(2424 + p)
    tree = synth.random_tree(14, rng)
    nwk = tree.newick()
    net, names = P.read_newick(nwk)
    taxa = [names[i] for i in range(net.nnodes) if net.is_leaf[i]]
    X = rng.normal(size=(len(taxa), p)) @ rng.normal(size=(p, p))
    (multi,), spt, root = _engines(P, nwk, taxa, X, p, fixed=False)
    Rm, mum, _ = P.calibrate_exact_cliquetree_(multi[2], spt, root)
    (uni,), spt1, root1 = _engines(P, nwk, taxa, np.ascontiguousarray(X.T[:, :, None]), 1, n_sites=p, fixed=False)
    fit = P.calibrate_rate_matrix_sites_(uni[2], spt1, root1)
    assert not fit["info"][0].any()
    worst = dict(R=_rel(fit["R"], Rm), mu=_rel(fit["mu"][0], mum))
    print(f"{p} sites as {p} traits on a 14-tip tree: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL
    assert np.array_equal(fit["R"], fit["R"].T)
    d = np.sqrt(np.diagonal(Rm))
    assert _rel(fit["corr"], Rm / np.outer(d, d)) <= TOL


# ----------------------------------------------------------------------------- 4: symmetry and the transposed query

def test_symmetry_and_the_transposed_query(P):
    """gram of a square query is symmetric to the byte, and a query (rows, cols) is the transposed query (cols, rows).  At 257
    sites the square query copies its three tiles below the diagonal from their mirror images; the off-diagonal queries
    compute the same entries, (a, b) and (b, a) both, and must give the bytes of the copy: the product of two doubles
    commutes and both entries see the same sequence of steps -- asserted here, not assumed."""
    case, cgb, _ = _calibrated(P, "bm40", 257)
    rc, whole = _raw(cgb, (0, 257), (0, 257), case.root)
    assert rc == 0 and not whole[3].any() and np.array_equal(whole[0], whole[0].T)
    for rows, cols in (((1, 40), (37, 257)), ((130, 257), (0, 17)), ((3, 4), (0, 257))):
        rc1, a = _raw(cgb, rows, cols, case.root)
        rc2, b = _raw(cgb, cols, rows, case.root)
        nr = rows[1] - rows[0]
        assert rc1 == 0 and rc2 == 0 and np.array_equal(a[0], b[0].T)
        assert all(np.array_equal(x[:nr], y[len(y) - nr:]) and np.array_equal(x[nr:], y[:len(y) - nr]) for x, y in zip(a[1:], b[1:]))
        assert np.array_equal(a[0], whole[0][rows[0]:rows[1], cols[0]:cols[1]])


# ----------------------------------------------------------------------------- 5: equal bytes

def test_equal_bytes_calls_and_ranges(P):
    """two calls; the full matrix against its four quadrants and against off-diagonal ranges that start at sites 1, 37 and 130;
    the timed variant; without mu"""
    case, cgb, _ = _calibrated(P, "bm40", 257)
    root = case.root
    rc, whole = _raw(cgb, (0, 257), (0, 257), root)
    rc2, again = _raw(cgb, (0, 257), (0, 257), root)
    assert rc == 0 and rc2 == 0 and _same(whole, again) and np.all(np.isfinite(whole[0]))
    G, den, mu, info = whole
    for rows, cols in [((0, 130), (0, 130)), ((0, 130), (130, 257)), ((130, 257), (0, 130)), ((130, 257), (130, 257)),
                       ((1, 37), (37, 130)), ((37, 130), (130, 257)), ((130, 257), (1, 100)), ((1, 257), (37, 38))]:
        rc, part = _raw(cgb, rows, cols, root)
        assert rc == 0 and np.array_equal(part[0], G[rows[0]:rows[1], cols[0]:cols[1]]), (rows, cols)
        for got, full in zip(part[1:], (den, mu, info)):
            assert np.array_equal(got, np.concatenate([full[rows[0]:rows[1]], full[cols[0]:cols[1]]])), (rows, cols)
    ms = np.full(3, -1.0)
    rc, timed = _raw(cgb, (0, 257), (0, 257), root, timed=ms)
    assert rc == 0 and _same(whole, timed) and np.all(ms >= 0.0)
    rc, nomu = _raw(cgb, (0, 257), (0, 257), (-1, 9), want_mu=False)
    assert rc == 0 and np.array_equal(nomu[0], G) and np.array_equal(nomu[1], den) and np.all(nomu[2] == 7.0)
    print(f"equal bytes at 257 sites: two calls, four quadrants, ranges from sites 1, 37 and 130; phases {ms.round(3).tolist()} ms")


@pytest.mark.parametrize("key,n", [("families130", 64), ("bm40", 257), ("families65", 64), ("families64", 64)])
def test_equal_bytes_chunks(P, key, n):
    """pgbp_sites_sweep_scratch_limit set so that every chunk is one 64-family block, against one chunk"""
    case, cgb, _ = _calibrated(P, key, n)
    nf = len(case.fam["cluster"])
    rc, one = _raw(cgb, (0, n), (0, n), case.root)
    rc1, off = _raw(cgb, (1, n), (0, n - 3), case.root)
    cgb._lib.pgbp_sites_sweep_scratch_limit(1)
    try:
        rc2, many = _raw(cgb, (0, n), (0, n), case.root)
        rc3, off2 = _raw(cgb, (1, n), (0, n - 3), case.root)
    finally:
        cgb._lib.pgbp_sites_sweep_scratch_limit(0)
    assert rc == 0 and rc1 == 0 and rc2 == 0 and rc3 == 0
    assert _same(one, many) and _same(off, off2)
    print(f"{key}/{n}: {nf} families in {(nf + 63) // 64} chunks of one block against one chunk: the same bytes")


def test_equal_bytes_layouts(P):
    """the site-minor and the plain instance of the same beliefs"""
    case, sm, _ = _calibrated(P, "bm40", 65)
    assert _layout(sm) == 2
    rc, a = _raw(sm, (0, 65), (0, 65), case.root)
    sm.pull()
    assert rc == 0 and _layout(sm) == 0
    rc, b = _raw(sm, (0, 65), (0, 65), case.root)
    assert rc == 0 and _same(a, b) and _layout(sm) == 0


# ----------------------------------------------------------------------------- 6: untouched state

def test_untouched_state(P):
    """the pool, pgbp_layout and a following calibrate_ keep their bytes"""
    case, cgb, o = _calibrated(P, "bm40", 65)
    cgb.pull()
    after = cgb._packed_raw.copy()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0 and _layout(cgb) == 2
    rc, out = _raw(cgb, (0, 65), (0, 65), case.root)
    assert rc == 0 and _layout(cgb) == 2
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    rc, out2 = _raw(cgb, (0, 65), (0, 65), case.root)
    cgb.pull()
    assert rc == 0 and np.array_equal(after, cgb._packed_raw) and _same(out, out2)


# ----------------------------------------------------------------------------- 7: a bad site

def test_a_site_with_a_negative_rate(P):
    """a site filled with R = -1 reports info and NaN in its row, column, den and mu; every other entry keeps its bytes"""
    case, cgb, _ = _calibrated(P, "bm40", 65, R=np.ones(65))
    rc, good = _raw(cgb, (0, 65), (0, 65), case.root)
    assert rc == 0 and not good[3].any()
    R = np.ones(65)
    R[37] = -1.0
    _calibrate(cgb, case.spt, R=R)
    rc, got = _raw(cgb, (0, 65), (0, 65), case.root)
    keep = np.arange(65) != 37
    both = np.concatenate([keep, keep])
    assert rc == 0 and got[3][37] > 0 and got[3][65 + 37] > 0 and not got[3][both].any()
    assert np.isnan(got[0][37, :]).all() and np.isnan(got[0][:, 37]).all()
    assert np.isnan(got[1][[37, 102]]).all() and np.isnan(got[2][[37, 102]]).all()
    assert np.array_equal(got[0][np.ix_(keep, keep)], good[0][np.ix_(keep, keep)])
    assert all(np.array_equal(g[both], w[both]) for g, w in zip(got[1:], good[1:]))
    rc, blk = _raw(cgb, (30, 40), (0, 20), case.root)     # the bad site among the rows only
    assert rc == 0 and np.isnan(blk[0][7, :]).all() and np.array_equal(np.delete(blk[0], 7, 0), np.delete(good[0][30:40, 0:20], 7, 0))
    fit = P.calibrate_rate_matrix_sites_(cgb, case.spt, case.root)   # (the driver fills R = 1 itself: every site is fine again)
    assert not fit["info"][0].any() and np.all(np.isfinite(fit["R"]))
    print(f"site 37 with R = -1: info {got[3][37]}, NaN in its row and column; the other entries keep their bytes")


# ----------------------------------------------------------------------------- 8: refusals

def _refused(cgb, code, word, rows=None, cols=None, root=(0, 0), null_gram=False, want_mu=True):
    n = cgb.n_sites
    rows = (0, n) if rows is None else rows
    cols = (0, n) if cols is None else cols
    cgb.pull()
    before = cgb._packed_raw.copy()
    lay = _layout(cgb)
    rc, out = _raw(cgb, rows, cols, root, want_mu=want_mu, null_gram=null_gram)
    msg = cgb._lib.pgbp_last_error(cgb._eng).decode()
    assert rc == code and word in msg and "pgbp_bm_rate_matrix_sites" in msg, (rc, msg, word)
    assert all(np.all(x == 7) for x in out) and _layout(cgb) == lay
    cgb.pull()
    assert np.array_equal(before, cgb._packed_raw)
    return msg


def test_refusals(P):
    """every refusal, before any launch: sentinel-filled outputs, layout and pool untouched, a text that names the reason"""
    from pgbp_amd import _lib as L
    from test_gpu_gradient import _tree_batch
    from test_gpu_exact_uni import _fixed, _free
    case, cgb, _ = _calibrated(P, "bm40", 65)
    root = case.root
    for rows, cols in (((0, 66), None), ((-1, 4), None), (None, (0, 66)), (None, (5, 4))):
        _refused(cgb, L.ERR_INVALID, "site range", rows, cols, root)
    _refused(cgb, L.ERR_INVALID, "no output buffer", root=root, null_gram=True)
    engine, *_ = _tree_batch(P, 8, 2, 50, True)
    assert "pgbp_bm_exact_stats)" in _refused(engine(np.arange(8)), L.ERR_INVALID, "2 traits")
    _refused(_engine(P, XR.get("bm40", 7), 7), L.ERR_INVALID, "7 sites", root=root)
    _refused(cgb, L.ERR_INVALID, "root belief", root=(len(cgb._dims), 0))
    _refused(cgb, L.ERR_INVALID, "root position", root=(root[0], int(cgb._dims[root[0]])))
    # a per-site mask in force
    mcase = XR.get("bm40+mask", 65)
    masked = _free(P, mcase, 65)
    _calibrate(masked, mcase.spt)
    assert "same observed tips" in _refused(masked, L.ERR_INVALID, "pgbp_lg_set_site_missing", root=root)
    # an OU fill; tip noise in force
    cgb.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1), model="ou", alpha=0.5, theta=np.zeros(1), sync=True)
    _refused(cgb, L.ERR_INVALID, "Ornstein-Uhlenbeck", root=root)
    cgb.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1), sync=True)
    tip = int(FR.LR.tip_families(case.fam)[0])
    cgb.set_tip_noise_lg(np.array([tip], np.int32), np.zeros((1, 1)), np.ones(1), np.full((1, 1), 0.25))
    cgb.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1), sync=True)
    _refused(cgb, L.ERR_INVALID, "tip noise", root=root)
    cgb.clear_tip_noise_lg()
    _calibrate(cgb, case.spt)
    rc, out = _raw(cgb, (0, 65), (0, 65), root)
    assert rc == 0 and not out[3].any()
    # a family whose parent is the fixed root
    _refused(_fixed(P, mcase.base, 65), L.ERR_INVALID, "its parent is the fixed root", want_mu=False)
    # a tip family with two parents: N1's table with the fixed-root parents declared out of scope (as test_gpu_exact_uni does)
    hc = FR.hybrid_case("N1", "bm")
    fam = dict(hc.fam)
    nf, K = len(fam["cluster"]), max(1, int(fam["max_parents"]))
    pm = np.ones(nf * K, np.uint64)
    pm[np.asarray(fam["parent_pos"]).reshape(-1) < 0] = 0
    fam["parent_mask"], fam["child_mask"] = pm, np.ones(nf, np.uint64)
    two = types.SimpleNamespace(**hc.__dict__)
    two.fam = fam
    _refused(_engine(P, two, 8), L.ERR_INVALID, "a leaf with more than one parent", want_mu=False)


# ----------------------------------------------------------------------------- 9: the drivers

@pytest.mark.parametrize("mode", ["cov", "corr"])
def test_phylo_pca(P, mode):
    """phylo_pca_sites against numpy.linalg.eigh of the dense GLS matrix: eigenvalues, loadings up to sign, scores (the
    eigengap of the compared components is asserted in test_rate_uni_cpu.py)"""
    key, n = RR.PCA_CASE
    case = RR.get(key, n)
    cgb = _engine(P, case, n)
    g = RR.gls(key, n)
    sd = np.sqrt(np.diagonal(g["R"]))
    A = g["R"] if mode == "cov" else g["R"] / np.outer(sd, sd)
    assert RR.eigengap(A, RR.PCA_K) >= 1e-3
    w, V, Z = RR.pca(A, g["Yc"], RR.PCA_K, None if mode == "cov" else sd)
    got = P.phylo_pca_sites(cgb, case.spt, case.root, mode=mode, n_components=RR.PCA_K)
    worst = dict(values=_rel(got["values"], w), loadings=_rel(RR.aligned(got["loadings"], V), V),
                 scores=_rel(RR.aligned(got["scores"], Z), Z), matrix=_rel(got["R"], A))
    print(f"phylo_pca_sites({mode}) on {key}/{n}, {RR.PCA_K} components: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL
    assert np.array_equal(got["rows"], RR.observed_rows(case))


def test_driver_blocks(P):
    """calibrate_rate_matrix_sites_ on a block: R, corr, mu against dense GLS"""
    key, n = "missing", 65
    case = RR.get(key, n)
    cgb = _engine(P, case, n)
    g = RR.gls(key, n)
    fit = P.calibrate_rate_matrix_sites_(cgb, case.spt, case.root, rows=(1, 38), cols=(37, 65))
    sd = np.sqrt(np.diagonal(g["R"]))
    worst = dict(R=_rel(fit["R"], g["R"][1:38, 37:65]), corr=_rel(fit["corr"], (g["R"] / np.outer(sd, sd))[1:38, 37:65]),
                 mu_rows=_rel(fit["mu"][0], g["mu"][1:38]), mu_cols=_rel(fit["mu"][1], g["mu"][37:65]))
    print(f"calibrate_rate_matrix_sites_ on {key}/{n}, rows 1:38 x cols 37:65: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL and not fit["info"][0].any() and not fit["info"][1].any()

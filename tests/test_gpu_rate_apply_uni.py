"""pgbp_bm_rate_apply_sites (csrc/pgbp_rate_apply_uni.hip) and its wrappers bm_rate_apply_sites and phylo_pca_leading_sites:
the evolutionary rate matrix of a univariate batch applied to a block of vectors, U'(U V) on the matrix cores without the
sites x sites matrix, and the leading phylogenetic principal components by subspace iteration on it.

Comparators, never the new kernels themselves: gram @ V with gram of pgbp_bm_rate_matrix_sites on the same beliefs (called
after the new call); the numpy restatement of tests/rate_apply_ref.py and dense GLS on the tips (pinned to each other in
test_rate_apply_cpu.py); numpy.linalg.eigh of the dense GLS matrix and phylo_pca_sites for the driver.  Every comparison is
asserted at 1e-8 relative to max(1, |block|_max); each test prints its worst figure."""
import ctypes as C
import types

import numpy as np
import pytest

import exact_uni_ref as XR
import fam_uni_ref as FR
import rate_apply_ref as AR
import rate_uni_ref as RR
from test_gpu_exact_uni import _calibrate
from test_gpu_fam_uni import _engine, _layout

pytestmark = pytest.mark.gpu
TOL = 1e-8
VECTORS = (1, 15, 16, 17, 64)


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


def _raw(cgb, sites, V, root, want_mu=True, n_vec=None, null_v=False, null_gv=False, timed=None):
    """the C call on V [sites, k]: (rc, [gv [sites, k], den, mu, info]) with sentinel-filled outputs"""
    from pgbp_amd import _lib as L
    ns = max(0, sites[1] - sites[0])
    vt = np.ascontiguousarray(np.asarray(V, float).T)
    k = vt.shape[0] if n_vec is None else n_vec
    out = [np.full(vt.shape, 7.0), np.full(ns, 7.0), np.full(ns, 7.0), np.full(ns, 7, np.int32)]
    args = [cgb._eng, sites[0], sites[1], k, None if null_v else L.f64p(vt), int(root[0]), int(root[1]),
            None if null_gv else L.f64p(out[0]), L.f64p(out[1]), L.f64p(out[2]) if want_mu else None, L.i32p(out[3])]
    if timed is not None:
        rc = cgb._lib.pgbp_bm_rate_apply_sites_timed(*args, L.f64p(timed))
    else:
        rc = cgb._lib.pgbp_bm_rate_apply_sites(*args)
    out[0] = out[0].T.copy()
    return rc, out


def _gram(cgb, sites, root):
    """the rate matrix call on the same beliefs: (gram, den, mu, info) of the range"""
    from pgbp_amd import _lib as L
    ns = sites[1] - sites[0]
    out = [np.full((ns, ns), 7.0), np.full(2 * ns, 7.0), np.full(2 * ns, 7.0), np.full(2 * ns, 7, np.int32)]
    rc = cgb._lib.pgbp_bm_rate_matrix_sites(cgb._eng, sites[0], sites[1], sites[0], sites[1], int(root[0]), int(root[1]), L.f64p(out[0]),
                                            L.f64p(out[1]), L.f64p(out[2]), L.i32p(out[3]))
    assert rc == 0
    return out[0], out[1][:ns], out[2][:ns], out[3][:ns]


def _same(x, y):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


def _vectors(n, k, seed=0):
    return np.random.default_rng(2600 + 7 * n + k + seed).standard_normal((n, k))


# ----------------------------------------------------------------------------- 1: against gram @ V, the restatement and dense GLS

EVERY = RR.SITE_CASES + RR.FAMILY_CASES + RR.OTHER_CASES


@pytest.mark.parametrize("key,n", EVERY, ids=[f"{k}-{n}" for k, n in EVERY])
def test_against_gram_the_restatement_and_gls(P, key, n):
    """gv for 1, 15, 16, 17 and 64 vectors against gram @ V (gram of the rate matrix call, made after), against U'(U V) of the
    restatement and against (Y'PY) V of dense GLS; den, mu and info with the bytes of the rate matrix call; the identity
    returns the very bytes of gram's columns.  Sites 8: the plain layout; 16 .. 65: the padding to 16 and the layout switch;
    257: a second workgroup of phase one and a fifth of the second product; 2 tips: fewer families than one MFMA step;
    63 .. 130 families: padding rows, a second and a third workgroup of the first product."""
    case, cgb, _ = _calibrated(P, key, n)
    lay = _layout(cgb)
    assert bool(lay & 2) == (n >= 64)
    got = {}
    for k in VECTORS:
        rc, got[k] = _raw(cgb, (0, n), _vectors(n, k), case.root)
        assert rc == 0 and _layout(cgb) == lay and not got[k][3].any()
    unit = np.eye(n)[:, : min(n, 64)]
    rc, ident = _raw(cgb, (0, n), unit, case.root)
    assert rc == 0
    gram, den, mu, info = _gram(cgb, (0, n), case.root)
    worst = dict(gram=0.0, restatement=0.0, gls=0.0)
    for k in VECTORS:
        V = _vectors(n, k)
        gv = got[k][0]
        worst["gram"] = max(worst["gram"], _rel(gv, gram @ V))
        worst["restatement"] = max(worst["restatement"], _rel(gv, AR.apply(key, n, V)))
        worst["gls"] = max(worst["gls"], _rel(gv, AR.gls_apply(key, n, V)))
        assert _same(got[k][1:], [den, mu, info])
    unit_bytes = np.array_equal(ident[0], gram[:, : unit.shape[1]])
    print(f"{key}/{n}: {len(case.fam['cluster'])} families, vectors {VECTORS}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) +
          f"; a unit vector returns the bytes of the gram column: {unit_bytes}")
    assert max(worst.values()) <= TOL
    # W = U e_j is the column j of U to the byte (one product with 1.0, the rest +0.0), and the second product takes U as the A
    # operand and W as the B operand in the family steps of rate_uni_syrk: the same MFMA sequence as gram's column
    assert unit_bytes


def test_without_a_root_mu_is_not_touched(P):
    case, cgb, _ = _calibrated(P, "bm40", 65)
    V = _vectors(65, 3)
    rc, a = _raw(cgb, (0, 65), V, case.root)
    rc2, b = _raw(cgb, (0, 65), V, (-1, 9), want_mu=False)
    assert rc == 0 and rc2 == 0 and np.all(b[2] == 7.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])


# ----------------------------------------------------------------------------- 2: symmetry, a sub-range, the wrapper

def test_symmetry(P):
    """V'(G V) is symmetric for a random V"""
    case, cgb, _ = _calibrated(P, "bm40", 257)
    V = _vectors(257, 17)
    rc, out = _raw(cgb, (0, 257), V, case.root)
    S = V.T @ out[0]
    asym = float(np.max(np.abs(S - S.T)) / max(1.0, np.max(np.abs(S))))
    print(f"257 sites, 17 vectors: |V'GV - (V'GV)'| / max(1, |V'GV|) = {asym:.1e}")
    assert rc == 0 and asym <= TOL


def test_sub_range_and_wrapper(P):
    """a sub-range from site 37 of the 257-site case is the principal block of gram; the wrapper blocks 130 vectors into three
    calls and takes a single vector"""
    case, cgb, _ = _calibrated(P, "bm40", 257)
    gram, den, mu, info = _gram(cgb, (0, 257), case.root)
    worst = 0.0
    for a, b in ((37, 257), (37, 100), (1, 38)):
        V = _vectors(b - a, 5)
        rc, out = _raw(cgb, (a, b), V, case.root)
        assert rc == 0 and _same(out[1:], [den[a:b], mu[a:b], info[a:b]])
        worst = max(worst, _rel(out[0], gram[a:b, a:b] @ V))
    V = _vectors(220, 130)
    GV, d, m, i = P.bm_rate_apply_sites(cgb, V, sites=(37, 257), root=case.root)
    parts = [_raw(cgb, (37, 257), V[:, j: j + 64], case.root)[1][0] for j in (0, 64, 128)]
    assert GV.shape == V.shape and np.array_equal(GV, np.concatenate(parts, axis=1))
    assert np.array_equal(d, den[37:]) and np.array_equal(m, mu[37:]) and not i.any()
    worst = max(worst, _rel(GV, gram[37:, 37:] @ V))
    one, _, nomu, _ = P.bm_rate_apply_sites(cgb, V[:, 3], sites=range(37, 257))
    assert one.shape == (220,) and nomu is None and np.array_equal(one, GV[:, 3])
    with pytest.raises(ValueError):
        P.bm_rate_apply_sites(cgb, V, sites=(0, 257))
    print(f"sub-ranges of 257 sites against the blocks of gram: {worst:.1e}")
    assert worst <= TOL


# ----------------------------------------------------------------------------- 3: equal bytes

def test_equal_bytes_calls_and_vector_blocks(P):
    """two calls; the timed twin; 64 vectors in one call against 4 calls of 16, and a vector sent alone"""
    case, cgb, _ = _calibrated(P, "bm40", 257)
    V = _vectors(257, 64)
    rc, whole = _raw(cgb, (0, 257), V, case.root)
    rc2, again = _raw(cgb, (0, 257), V, case.root)
    assert rc == 0 and rc2 == 0 and _same(whole, again) and np.all(np.isfinite(whole[0]))
    ms = np.full(4, -1.0)
    rc, timed = _raw(cgb, (0, 257), V, case.root, timed=ms)
    assert rc == 0 and _same(whole, timed) and np.all(ms >= 0.0)
    for j in range(0, 64, 16):
        rc, part = _raw(cgb, (0, 257), V[:, j: j + 16], case.root)
        assert rc == 0 and np.array_equal(part[0], whole[0][:, j: j + 16]) and _same(part[1:], whole[1:])
    rc, alone = _raw(cgb, (0, 257), V[:, 37: 38], case.root)
    assert rc == 0 and np.array_equal(alone[0], whole[0][:, 37: 38])
    print(f"equal bytes at 257 sites: two calls, 64 vectors against 4 x 16 and against one alone; phases {ms.round(3).tolist()} ms")


@pytest.mark.parametrize("key,n", [("families130", 64), ("bm40", 257), ("families65", 64), ("families64", 64)])
def test_equal_bytes_chunks(P, key, n):
    """pgbp_sites_sweep_scratch_limit set so that every chunk is one 64-family block, against one chunk"""
    case, cgb, _ = _calibrated(P, key, n)
    nf = len(case.fam["cluster"])
    V = _vectors(n, 17)
    rc, one = _raw(cgb, (0, n), V, case.root)
    rc1, off = _raw(cgb, (1, n - 3), V[: n - 4], case.root)
    cgb._lib.pgbp_sites_sweep_scratch_limit(1)
    try:
        rc2, many = _raw(cgb, (0, n), V, case.root)
        rc3, off2 = _raw(cgb, (1, n - 3), V[: n - 4], case.root)
    finally:
        cgb._lib.pgbp_sites_sweep_scratch_limit(0)
    assert rc == 0 and rc1 == 0 and rc2 == 0 and rc3 == 0
    assert _same(one, many) and _same(off, off2)
    print(f"{key}/{n}: {nf} families in {(nf + 63) // 64} chunks of one block against one chunk: the same bytes")


def test_equal_bytes_layouts(P):
    """the site-minor and the plain instance of the same beliefs"""
    case, sm, _ = _calibrated(P, "bm40", 65)
    V = _vectors(65, 17)
    assert _layout(sm) == 2
    rc, a = _raw(sm, (0, 65), V, case.root)
    sm.pull()
    assert rc == 0 and _layout(sm) == 0
    rc, b = _raw(sm, (0, 65), V, case.root)
    assert rc == 0 and _same(a, b) and _layout(sm) == 0


def test_untouched_state(P):
    """the pool, pgbp_layout and a following calibrate_ keep their bytes"""
    case, cgb, o = _calibrated(P, "bm40", 65)
    V = _vectors(65, 17)
    cgb.pull()
    after = cgb._packed_raw.copy()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0 and _layout(cgb) == 2
    rc, out = _raw(cgb, (0, 65), V, case.root)
    assert rc == 0 and _layout(cgb) == 2
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    rc, out2 = _raw(cgb, (0, 65), V, case.root)
    cgb.pull()
    assert rc == 0 and np.array_equal(after, cgb._packed_raw) and _same(out, out2)


# ----------------------------------------------------------------------------- 4: a bad site

def test_a_site_with_a_negative_rate(P):
    """a site filled with R = -1: info names it, gv is NaN in every entry, den and mu are NaN at that site only"""
    case, cgb, _ = _calibrated(P, "bm40", 65, R=np.ones(65))
    V = _vectors(65, 17)
    rc, good = _raw(cgb, (0, 65), V, case.root)
    assert rc == 0 and not good[3].any() and np.all(np.isfinite(good[0]))
    R = np.ones(65)
    R[37] = -1.0
    _calibrate(cgb, case.spt, R=R)
    rc, got = _raw(cgb, (0, 65), V, case.root)
    keep = np.arange(65) != 37
    assert rc == 0 and got[3][37] > 0 and not got[3][keep].any()
    assert np.isnan(got[0]).all()
    assert np.isnan(got[1][37]) and np.isnan(got[2][37])
    assert all(np.array_equal(g[keep], w[keep]) for g, w in zip(got[1:], good[1:]))
    _, den, mu, info = _gram(cgb, (0, 65), case.root)
    assert _same(got[1:], [den, mu, info])
    rc, blk = _raw(cgb, (0, 37), V[:37], case.root)      # a range without the bad site is another operator, and fine
    assert rc == 0 and not blk[3].any() and np.all(np.isfinite(blk[0]))
    print(f"site 37 with R = -1: info {got[3][37]}, gv all NaN, den and mu NaN at the site only")


# ----------------------------------------------------------------------------- 5: refusals

def _refused(cgb, code, word, sites=None, root=(0, 0), want_mu=True, k=3, **kw):
    n = cgb.n_sites
    sites = (0, n) if sites is None else sites
    cgb.pull()
    before = cgb._packed_raw.copy()
    lay = _layout(cgb)
    rc, out = _raw(cgb, sites, np.ones((max(0, sites[1] - sites[0]), k)), root, want_mu=want_mu, **kw)
    msg = cgb._lib.pgbp_last_error(cgb._eng).decode()
    assert rc == code and word in msg and "pgbp_bm_rate_apply_sites" in msg, (rc, msg, word)
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
    for sites in ((0, 66), (-1, 4), (5, 4)):
        _refused(cgb, L.ERR_INVALID, "site range", sites, root)
    _refused(cgb, L.ERR_INVALID, "0 vectors", root=root, k=1, n_vec=0)
    _refused(cgb, L.ERR_INVALID, "65 vectors", root=root, k=65)
    _refused(cgb, L.ERR_INVALID, "no input vectors", root=root, null_v=True)
    _refused(cgb, L.ERR_INVALID, "no output buffer", root=root, null_gv=True)
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
    rc, out = _raw(cgb, (0, 65), np.ones((65, 3)), root)
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


# ----------------------------------------------------------------------------- 6: the driver

@pytest.mark.parametrize("ntips,n", AR.PLANTED, ids=[f"{a}tips-{b}" for a, b in AR.PLANTED])
def test_phylo_pca_leading(P, ntips, n):
    """phylo_pca_leading_sites on the planted spectra (gaps and decay asserted in test_rate_apply_cpu.py) against
    numpy.linalg.eigh of the dense GLS matrix and against phylo_pca_sites on the same engine: values within 1e-8 lambda_1,
    loadings and scores up to sign, explained; converged, in the iterations the dense restatement takes or one off"""
    from pgbp_amd.exact import leading_eigenpairs
    case = AR.planted(ntips, n)
    cgb = _engine(P, case, n)
    g = AR.planted_gls(ntips, n)
    for mode in ("cov", "corr"):
        A, sd = AR.matrix(g, mode)
        w, V, Z = RR.pca(A, g["Yc"], AR.K, sd)
        cpu = leading_eigenpairs(lambda Q: A @ Q, n, AR.K)
        got = P.phylo_pca_leading_sites(cgb, case.spt, case.root, AR.K, mode=mode)
        full = P.phylo_pca_sites(cgb, case.spt, case.root, mode=mode, n_components=AR.K)
        worst = dict(values=float(np.max(np.abs(got["values"] - w)) / w[0]), loadings=_rel(RR.aligned(got["loadings"], V), V),
                     scores=_rel(RR.aligned(got["scores"], Z), Z), explained=_rel(got["explained"], w / np.trace(A)),
                     mu=_rel(got["mu"], g["mu"]),
                     values_full=float(np.max(np.abs(got["values"] - full["values"])) / w[0]),
                     loadings_full=_rel(RR.aligned(got["loadings"], full["loadings"]), full["loadings"]),
                     scores_full=_rel(RR.aligned(got["scores"], full["scores"]), full["scores"]))
        print(f"phylo_pca_leading_sites({mode}) on planted {ntips} tips / {n} sites, {AR.K} components: " +
              ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) +
              f"; iterations {got['iterations']} (dense restatement {cpu['iterations']}), worst residual / lambda_1 {np.max(got['residuals']) / w[0]:.1e}")
        assert max(worst.values()) <= TOL
        assert got["converged"] and abs(got["iterations"] - cpu["iterations"]) <= 1
        assert np.array_equal(got["rows"], RR.observed_rows(case)) and "R" not in got
        assert set(got) == {"values", "loadings", "scores", "rows", "mu", "explained", "residuals", "iterations", "converged"}


def test_phylo_pca_leading_bad_site(P):
    """a site without a rate estimate raises LinAlgError naming it: the driver fills R = 1 itself, so the fill is replaced by
    the R = -1 construction of test_gpu_rate_uni.py (site 37 of 65)"""
    case = RR.get("bm40", 65)
    cgb = _engine(P, case, 65)
    fill = cgb.assignfactors_lg_
    R = np.ones(65)
    R[37] = -1.0
    cgb.assignfactors_lg_ = lambda *a, **k: fill(R.reshape(-1, 1, 1, 1), np.zeros((65, 1)), sync=True)
    with pytest.raises(np.linalg.LinAlgError, match="site 37 "):
        P.phylo_pca_leading_sites(cgb, case.spt, case.root, 2)
    del cgb.assignfactors_lg_
    with pytest.raises(ValueError):
        P.phylo_pca_leading_sites(cgb, case.spt, case.root, 2, mode="other")
    ok = P.phylo_pca_leading_sites(cgb, case.spt, case.root, 2)
    assert ok["converged"] and np.all(np.isfinite(ok["loadings"]))

"""pgbp_posterior_cov_sites (csrc/pgbp_cov_uni.hip) and its wrappers posterior_cov_sites_, node_cov_sites and
functional_moments_sites: exact posterior covariances of linear functionals of a fitted univariate batch, lanes = sites, with
the Gram matrix of the columns folded on the device.

Comparators, never the new kernels themselves: the general call on the SAME beliefs (posterior_cov_(all_sites=True), called
AFTER the new call so that its layout conversion cannot help it), for one site in eight the numpy restatement of
tests/cov_uni_ref.py on the oracle's calibrated clique tree, and with c = I the dense posterior covariance of all node states
(post_uni_ref.dense_posterior) -- pinned in test_cov_uni_cpu.py, which also checks the margin of the pivots these tests rely
on.  Every comparison is asserted at 1e-8 relative to max(1, |block|_inf); NaN patterns and info must be equal; gram must be
the block-ordered sum of the call's own w rows to the byte; each test prints its worst figure."""
import ctypes as C

import numpy as np
import pytest

import cov_ref as CR
import cov_uni_ref as CU
import fam_uni_ref as FR
import post_uni_ref as PR
from test_gpu_fam_uni import _engine, _layout

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _size(cgb):
    return int(cgb._lib.pgbp_sample_size(cgb._eng))


def _raw(cgb, a, b, c, want="wkg", expect=0):
    """the C call on [a, b): (w [n_cols, size, n], k, gram [pairs, n], info [n]), sentinel-filled first; an output not in `want`
    is passed as NULL and returned as None"""
    from pgbp_amd import _lib as L
    n, (nc, size) = b - a, c.shape
    w = np.full((nc, size, n), 7.0) if "w" in want else None
    k = np.full((nc, size, n), 7.0) if "k" in want else None
    g = np.full((nc * (nc + 1) // 2, n), 7.0) if "g" in want else None
    info = np.full(n, 7, np.int32)
    ptr = lambda x: None if x is None else L.f64p(x)
    rc = cgb._lib.pgbp_posterior_cov_sites(cgb._eng, 0, a, b, nc, L.f64p(np.ascontiguousarray(c)), ptr(w), ptr(k), ptr(g), L.i32p(info))
    assert rc == expect, cgb._lib.pgbp_last_error(cgb._eng)
    if expect == 0:
        assert not any(x is not None and np.any(x == 7.0) for x in (w, k, g)) and not np.any(info == 7)
    return w, k, g, info


def _same(x, y):
    return all((p is None and q is None) or p.tobytes() == q.tobytes() for p, q in zip(x, y))


def _per_site(cgb, n_cols, with_k):
    """the doubles of scratch a site takes with n_cols columns and gram resident (include/pgbp.h)"""
    size = _size(cgb)
    n_pre = int(np.count_nonzero(cgb._dims[: cgb.nclusters]))
    return n_cols * size * (2 if with_k else 1) + (-(-size // 64) + 1) * (n_cols * (n_cols + 1) // 2) + -(-n_pre // 64)


def _rel_sites(got, want):
    """worst over the sites of max |got - want| relative to max(1, |want|_inf) of the site's block; got, want [..., n_sites]"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN patterns differ"
    ok = ~np.isnan(want)
    g, w = np.where(ok, got, 0.0).reshape(-1, got.shape[-1]), np.where(ok, want, 0.0).reshape(-1, got.shape[-1])
    return float(np.max(np.abs(g - w).max(axis=0) / np.maximum(1.0, np.abs(w).max(axis=0))))


def _run(P, case, n, sites):
    """one calibration; the new call on the functionals (all outputs, then gram alone) and on c = I, then the general call"""
    cgb = _engine(P, case, n)
    cgb.impute_and_loglik_sites_lg(case.spt)
    lay = _layout(cgb)
    assert bool(lay & 2) == (n >= 64)
    D = _size(cgb)
    dims, sepcl, soff, sidx, vn, off = PR.layout(case)
    assert D == int(off[-1])
    tag = f"{case.name}/{n}, size {D}"
    c = CU.functionals(D)
    w, k, g, info = _raw(cgb, 0, n, c)
    assert not info.any() and _layout(cgb) == lay
    worst = {}
    # gram: the block-ordered sum of the call's own w rows to the byte; w w' from numpy to rounding; alone, the same bytes
    assert g.tobytes() == CU.gram_rows(w).tobytes(), tag
    worst["gram against w w'"] = _rel_sites(CU.gram_full(g, 3).transpose(1, 2, 0), np.einsum("aes,bes->abs", w, w))
    assert _same(_raw(cgb, 0, n, c, "g"), (None, None, g, info)), tag
    assert _same(_raw(cgb, 0, n, c, "wg"), (w, None, g, info)) and _same(_raw(cgb, 0, n, c, "k"), (None, k, None, info)), tag
    # structure
    spos = CR.s_positions(dims, sepcl, soff, sidx, case.spt[2], case.spt[3], case.ocgb0.nclusters)
    assert np.all(w[:, spos] == 0.0) and not np.signbit(w[:, spos]).any(), tag
    eye = np.eye(D)
    wI, kI, _, infoI = _raw(cgb, 0, n, eye, "wk")
    assert not infoI.any() and _layout(cgb) == lay
    worst["k = k', c = I"] = _rel_sites(kI, kI.transpose(1, 0, 2))
    first, shared = {}, 0
    for e, nt in enumerate(vn):
        if nt in first:
            shared += 1
            assert kI[:, e].tobytes() == kI[:, first[nt]].tobytes() and k[:, e].tobytes() == k[:, first[nt]].tobytes(), (tag, nt)
        else:
            first[nt] = e
    mom = cgb.moments_sites_()
    for cl in range(case.ocgb0.nclusters):
        m = int(dims[cl])
        if m:
            sl = slice(int(off[cl]), int(off[cl]) + m)
            worst["k in a cluster against moments_sites_"] = max(worst.get("k in a cluster against moments_sites_", 0.0),
                                                                 _rel_sites(kI[sl, sl], mom[cl][1].transpose(1, 2, 0)))
    # one site in eight: the numpy restatement and the dense oracle
    for key in ("w (numpy)", "k (numpy)", "gram (numpy)", "k, c = I, dense", "w w', c = I, dense"):
        worst[key] = 0.0
    flat = np.array([nd for nd, _ in vn], dtype=int)
    for s in sites:
        ocgb, _, _, _ = FR.oracle_site(case, s)
        rec = PR.records_of(ocgb)[: ocgb.nclusters]
        rw, rk, ri = CU.cov_rows(rec, dims, sepcl, soff, sidx, case.spt[2], case.spt[3], c)
        assert ri == 0
        worst["w (numpy)"] = max(worst["w (numpy)"], FR.rel(w[:, :, s], rw))
        worst["k (numpy)"] = max(worst["k (numpy)"], FR.rel(k[:, :, s], rk))
        worst["gram (numpy)"] = max(worst["gram (numpy)"], FR.rel(g[:, s], CU.gram_rows(rw[:, :, None])[:, 0]))
        _, pc = PR.dense_posterior(case, s)
        dense = pc[np.ix_(flat, flat)]
        worst["k, c = I, dense"] = max(worst["k, c = I, dense"], FR.rel(kI[:, :, s], dense))
        worst["w w', c = I, dense"] = max(worst["w w', c = I, dense"], FR.rel(wI[:, :, s] @ wI[:, :, s].T, dense))
    # the general call on the same beliefs, after the new one
    gw, gk, ginfo = cgb.posterior_cov_(c, all_sites=True)
    assert np.array_equal(ginfo, info)
    worst["w (general)"] = _rel_sites(w, gw.transpose(0, 2, 1))
    worst["k (general)"] = _rel_sites(k, gk.transpose(0, 2, 1))
    print(f"{tag}: {shared} shared entries carry the same bits; " + ", ".join(f"{key} {v:.2e}" for key, v in worst.items()))
    assert shared >= 1 or D < 4
    assert max(worst.values()) <= TOL, (tag, worst)
    return cgb


# ----------------------------------------------------------------------------- 1: every case at its site counts

PLAIN = [(c, n) for c, counts, _ in PR.cases() for n in counts]


@pytest.mark.parametrize("i", range(len(PLAIN)), ids=[f"{c.name}-{n}" for c, n in PLAIN])
def test_call_against_the_general_call_and_the_statements(P, i):
    """BM at 8 (plain pool, a partial wavefront), 64 (site-minor), 65 and 257 sites (one site into a second workgroup); OU with
    a fixed, random and improper root; the hybrid-tip networks N1 .. N4 under BM and OU (2-variable sepsets, 0-variable
    clusters); tips without data, per-site shifts and tip noise.  Three functionals with weight on both sides of every
    64-entry boundary, and c = I."""
    case, n = PLAIN[i]
    _run(P, case, n, FR.checked_sites(n))


@pytest.mark.parametrize("shape,n", CU.SHAPES)
def test_block_boundaries_and_level_shapes(P, shape, n):
    """63, 64, 65 and 130 families (the 64-cluster blocks of the validity pass), trees whose layout size is 63 | 66 and
    191 | 192 | 194 (the 64-entry blocks of gram), a caterpillar of 12 tips (many levels of one cluster) and a balanced tree
    (few wide levels); 64 sites"""
    case = PR.shape_case(shape, n)
    cgb = _run(P, case, 64, (0, 56))
    print(f"{shape} {n}: layout size {_size(cgb)}")
    assert CU.SIZES.get((shape, n), _size(cgb)) == _size(cgb)


# ----------------------------------------------------------------------------- 2: the raw call: determinism, read-only

def test_determinism_ranges_chunks_and_columns(P):
    """600 sites: two calls, [0, n) against two half ranges and an odd range, one workgroup of sites per chunk (the scratch limit
    lowered: without gram the columns are then cut one by one as well; with gram the limit is what the three columns of one
    workgroup take), and one column per call against all columns at once return the same bytes; the layout stays site-minor"""
    case = PR.bm_missing_case()
    n = 600
    cgb = _engine(P, case, n)
    cgb.impute_and_loglik_sites_lg(case.spt)
    assert _layout(cgb) == 2
    c = CU.functionals(_size(cgb))
    full = _raw(cgb, 0, n, c)
    assert not full[3].any()
    assert _same(full, _raw(cgb, 0, n, c))
    lo, hi = _raw(cgb, 0, 300, c), _raw(cgb, 300, n, c)
    assert _same(full, [np.concatenate([x, y], axis=-1) for x, y in zip(lo, hi)])
    assert _same([x[..., 77:401] for x in full], _raw(cgb, 77, 401, c))
    try:
        cgb._lib.pgbp_sites_sweep_scratch_limit(1)   # (one workgroup's sites at least: chunks of 256, one column at a time)
        assert _same((full[0], full[1], None, full[3]), _raw(cgb, 0, n, c, "wk"))
        assert _same((full[0], None, None, full[3]), _raw(cgb, 0, n, c, "w"))
        cgb._lib.pgbp_sites_sweep_scratch_limit(256 * _per_site(cgb, 3, True))   # (the three columns of one workgroup, no more)
        assert _same(full, _raw(cgb, 0, n, c))
        cgb._lib.pgbp_sites_sweep_scratch_limit(256 * _per_site(cgb, 3, False))
        assert _same((None, None, full[2], full[3]), _raw(cgb, 0, n, c, "g"))
    finally:
        cgb._lib.pgbp_sites_sweep_scratch_limit(0)
    for a in range(3):
        one = _raw(cgb, 0, n, c[a: a + 1])
        assert one[0].tobytes() == full[0][a: a + 1].tobytes() and one[1].tobytes() == full[1][a: a + 1].tobytes()
        assert one[2][0].tobytes() == full[2][a * (a + 1) // 2 + a].tobytes()
    assert _layout(cgb) == 2
    w, k, gram, info = cgb.posterior_cov_sites_(c)
    assert w.transpose(0, 2, 1).tobytes() == full[0].tobytes() and k.transpose(0, 2, 1).tobytes() == full[1].tobytes()
    assert gram.shape == (n, 3, 3) and gram[:, 0, 1].tobytes() == full[2][1].tobytes() and np.array_equal(gram[:, 1, 0], gram[:, 0, 1])
    assert not info.any()


def test_read_only_and_both_layouts(P):
    """64 sites: the pool's bytes and pgbp_layout are unchanged by the call; a calibrate_ after it gives the bytes of one
    without it; the site-minor and the plain instance of the same beliefs give the same bytes"""
    case = PR.bm_missing_case()
    cgb = _engine(P, case, 64)
    cgb.impute_and_loglik_sites_lg(case.spt)
    assert _layout(cgb) == 2
    c = CU.functionals(_size(cgb))
    sm = _raw(cgb, 0, 64, c)
    assert _layout(cgb) == 2
    cgb.pull()   # (the transfer moves the pool to the plain layout, an exact copy)
    after = cgb._packed_raw.copy()
    assert _layout(cgb) == 0
    assert _same(sm, _raw(cgb, 0, 64, c))
    assert _layout(cgb) == 0
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)
    o = cgb._opts()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    assert _layout(cgb) == 2
    assert _same(sm, _raw(cgb, 0, 64, c))
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)


# ----------------------------------------------------------------------------- 3: one bad lane

def test_one_bad_lane(P):
    """a site with a negative rate: info names the first failing cluster in preorder (the general call's and the sampler's), w,
    k and gram of the site are NaN; its 63 wavefront neighbours keep the bytes they have without the failure"""
    case = PR.bm_missing_case()
    cgb = _engine(P, case, 64)
    cgb.impute_and_loglik_sites_lg(case.spt)
    c = CU.functionals(_size(cgb))
    good = _raw(cgb, 0, 64, c)
    kw = dict(cgb._fam_uni_kw)
    kw["R"] = kw["R"].copy()
    kw["R"][37] = -1.0
    cgb.assignfactors_lg_(**kw)
    cgb.impute_and_loglik_sites_lg(case.spt)
    got = _raw(cgb, 0, 64, c)
    only = _raw(cgb, 0, 64, c, "g")
    _, xinfo, _ = cgb.sample_posterior_sites_(1, seed=1)
    gw, gk, ginfo = cgb.posterior_cov_(c, all_sites=True)
    keep = np.arange(64) != 37
    info = got[3]
    assert info[37] != 0 and not info[keep].any() and np.array_equal(info, ginfo) and np.array_equal(info, xinfo)
    order = [int(case.spt[2][0])] + [int(cl) for cl in case.spt[3]]
    print(f"one bad lane: info names cluster {info[37]}; preorder starts {[cl + 1 for cl in order[:3]]}")
    for x, y in zip(got[:3], good[:3]):
        assert np.isnan(x[..., 37]).all()
        assert np.ascontiguousarray(x[..., keep]).tobytes() == np.ascontiguousarray(y[..., keep]).tobytes()
    assert only[2].tobytes() == got[2].tobytes()
    assert np.isnan(gw[:, 37]).all() and np.isnan(gk[:, 37]).all()


# ----------------------------------------------------------------------------- 4: refusals

def _refused(cgb, code, word, a=0, b=None, n_cols=1, tree=0, null_c=False, null_out=False, general=False, want="wkg"):
    """the call returns `code` with `word` in the message (general: and the general call to use), the outputs, the layout and
    the pool untouched"""
    from pgbp_amd import _lib as L
    b = cgb.n_sites if b is None else b
    big = 1 << 16
    cgb.pull()
    before = cgb._packed_raw.copy()
    lay = _layout(cgb)
    f64 = [np.full(big, 7.0) for _ in range(3)]
    i32 = np.full(big, 7, np.int32)
    cc = np.ones(big)
    d = [L.f64p(x) if (not null_out and ch in want) else None for x, ch in zip(f64, "wkg")]
    rc = cgb._lib.pgbp_posterior_cov_sites(cgb._eng, tree, a, b, n_cols, None if null_c else L.f64p(cc), d[0], d[1], d[2], L.i32p(i32))
    msg = cgb._lib.pgbp_last_error(cgb._eng)
    assert rc == code and word.encode() in msg and msg.startswith(b"pgbp_posterior_cov_sites"), (rc, msg)
    assert not general or b"(use pgbp_posterior_cov)" in msg, msg
    assert all(np.all(x == 7.0) for x in f64) and np.all(i32 == 7) and _layout(cgb) == lay
    cgb.pull()
    assert np.array_equal(before, cgb._packed_raw)
    return msg


def test_refusals(P):
    from pgbp_amd import _lib as L
    from test_gpu_gradient import _tree_batch
    engine, spt, *_ = _tree_batch(P, 8, 2, 50, True)
    _refused(engine(np.arange(8)), L.ERR_INVALID, "2 traits", general=True)
    case = FR.bm_case()
    _refused(_engine(P, case, 7), L.ERR_INVALID, "7 sites", general=True)
    cgb8 = _engine(P, case, 8)
    _refused(cgb8, L.ERR_STATE, "no schedule")
    cgb8.impute_and_loglik_sites_lg(case.spt)
    _refused(cgb8, L.ERR_INVALID, "site range", 0, 9)
    _refused(cgb8, L.ERR_INVALID, "out of range", tree=1)
    _refused(cgb8, L.ERR_INVALID, "n_cols = 0", n_cols=0)
    _refused(cgb8, L.ERR_INVALID, "no input buffer c", null_c=True)
    _refused(cgb8, L.ERR_INVALID, "no output buffer", null_out=True)
    # gram with more columns than the lowered limit holds: the text says how many fit
    try:
        cgb8._lib.pgbp_sites_sweep_scratch_limit(256 * _per_site(cgb8, 2, True))
        msg = _refused(cgb8, L.ERR_INVALID, "2 columns fit", n_cols=3)
        _refused(cgb8, L.ERR_INVALID, "3 columns fit", n_cols=4, want="wg")   # (without k a column takes half)
        cgb8._lib.pgbp_sites_sweep_scratch_limit(1)
        _refused(cgb8, L.ERR_INVALID, "0 columns fit", n_cols=1, want="g")
        c = CU.functionals(_size(cgb8))
        assert _raw(cgb8, 0, 8, c, "wk")[3].tolist() == [0] * 8   # (without gram the columns are cut: nothing is refused)
    finally:
        cgb8._lib.pgbp_sites_sweep_scratch_limit(0)
    print("refused with:", msg.decode())


# ----------------------------------------------------------------------------- 5: the wrappers

def test_node_cov_sites_and_functional_moments_sites(P):
    """the 40-tip BM tree at 8 sites, labelled beliefs: node_cov_sites of two ancestors that share no cluster (and of a list with
    a node that has no variable: NaN) against the dense posterior covariance; functional_moments_sites of a clade mean and of
    a contrast against the dense mean and variance; a site with a negative rate is NaN and hides no other"""
    from helpers import product_beliefs_from_oracle
    case = FR.bm_case()
    cgb = _engine(P, case, 8)
    cgb._objs = product_beliefs_from_oracle(case.ocgb0.belief)   # (labels only: the engine's beliefs are the device's)
    cgb.impute_and_loglik_sites_lg(case.spt)
    ent = cgb._node_entries("the test")
    held = sorted(lab for lab, v in ent.items() if v[2][0] >= 0)
    bare = sorted(lab for lab, v in ent.items() if v[2][0] < 0)
    together = {lab: set() for lab in ent}
    for b in case.ocgb0.belief[: case.ocgb0.nclusters]:
        for lab in b.nodelabel:
            together[lab] |= set(b.nodelabel)
    a = held[0]
    far = [lab for lab in held if lab not in together[a]]
    assert len(far) >= 2 and len(bare) >= 1
    nodes_a, nodes_b = [a, far[0], bare[0]], [far[-1], a, bare[0]]
    cov = cgb.node_cov_sites(nodes_a, nodes_b)
    assert cov.shape == (8, 3, 3) and np.isnan(cov[:, 2, :]).all() and np.isnan(cov[:, :, 2]).all()
    clade = held[:5]
    W = {lab: np.array([1.0 / len(clade), 0.0]) for lab in clade}
    W[far[-1]] = np.array([0.0, -1.0])
    W[a] = W[a] + np.array([0.0, 1.0])
    mean, fcov = cgb.functional_moments_sites(W)
    assert mean.shape == (8, 2) and fcov.shape == (8, 2, 2)
    worst = dict(node_cov=0.0, mean=0.0, cov=0.0)
    for s in range(8):
        pm, pc = PR.dense_posterior(case, s)
        want = np.array([[pc[x - 1, y - 1] for y in nodes_b[:2]] for x in nodes_a[:2]])
        worst["node_cov"] = max(worst["node_cov"], FR.rel(cov[s, :2, :2], want))
        Wd = np.zeros((2, len(pm)))
        for lab, wv in W.items():
            Wd[:, lab - 1] += wv
        worst["mean"] = max(worst["mean"], FR.rel(mean[s], Wd @ pm))
        worst["cov"] = max(worst["cov"], FR.rel(fcov[s], Wd @ pc @ Wd.T))
    print(f"wrappers, 8 sites: nodes {a} and {far[-1]} share no cluster; " + ", ".join(f"{key} {v:.2e}" for key, v in worst.items()))
    assert max(worst.values()) <= TOL
    with pytest.raises(ValueError):
        cgb.functional_moments_sites({bare[0]: np.array([1.0])})
    with pytest.raises(ValueError):
        cgb.node_cov_sites([10 ** 6])
    # one bad site: NaN there, the others keep their bytes
    kw = dict(cgb._fam_uni_kw)
    kw["R"] = kw["R"].copy()
    kw["R"][3] = -1.0
    cgb.assignfactors_lg_(**kw)
    cgb.impute_and_loglik_sites_lg(case.spt)
    cov2 = cgb.node_cov_sites(nodes_a, nodes_b)
    mean2, fcov2 = cgb.functional_moments_sites(W)
    keep = np.arange(8) != 3
    assert np.isnan(cov2[3]).all() and np.isnan(mean2[3]).all() and np.isnan(fcov2[3]).all()
    assert cov2[keep].tobytes() == cov[keep].tobytes() and mean2[keep].tobytes() == mean[keep].tobytes() and fcov2[keep].tobytes() == fcov[keep].tobytes()

"""pgbp_moments_sites, pgbp_sample_posterior_sites, pgbp_lg_impute_sites (csrc/pgbp_post_uni.hip) and their wrappers
moments_sites_, sample_posterior_sites_, impute_sites_lg, impute_and_loglik_sites_lg: posterior moments, joint draws and
imputations of a fitted univariate batch, lanes = sites.

Comparators, never the new kernels themselves: the general calls on the SAME beliefs (moments_, sample_posterior_ with the same
z, impute_lg, all with all_sites=True, called AFTER the new calls so that their layout conversion cannot help them) and, for one
site in eight, the statements of tests/post_uni_ref.py on the oracle's calibrated clique tree (the dense posterior of all node
states, sample_ref.sample_posterior_ref, impute_ref.dense_impute -- pinned in test_post_uni_cpu.py, which also checks the
margins of the pivots and of the tips' variances these tests rely on).  Every comparison is asserted at 1e-8 relative to
max(1, |block|_inf); NaN patterns, info and predicted must be equal; each test prints its worst figure."""
import ctypes as C

import numpy as np
import pytest

import fam_uni_ref as FR
import post_uni_ref as PR
import sample_ref as SR
from test_gpu_fam_uni import _engine, _layout

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _rel_sites(got, want):
    """worst over the sites of max |got - want| relative to max(1, |want|_inf) of the site's block; got, want [n_sites, ...];
    the NaN and Inf patterns must be the same"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN patterns differ"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), "Inf patterns differ"
    if got.size == 0:
        return 0.0
    ok = ~np.isnan(want) & ~inf
    d = np.where(ok, np.abs(np.where(ok, got, 0.0) - np.where(ok, want, 0.0)), 0.0).reshape(got.shape[0], -1)
    scale = np.maximum(1.0, np.where(ok, np.abs(want), 0.0).reshape(got.shape[0], -1).max(axis=1))
    return float(np.max(d.max(axis=1) / scale))


def _new_then_general(cgb, spt, z, n_draws):
    """One calibration, the three new calls (the layout is the calibration's before and after each), then the three general
    calls on the same beliefs"""
    nb = len(cgb._dims)
    ll, imp = cgb.impute_and_loglik_sites_lg(spt)
    lay = _layout(cgb)
    assert bool(lay & 2) == (cgb.n_sites >= 64)
    mom = cgb.moments_sites_(np.arange(nb))
    assert _layout(cgb) == lay
    x, xinfo, views = cgb.sample_posterior_sites_(n_draws, z=z)
    assert _layout(cgb) == lay
    got = dict(ll=ll, imp=imp, mom=mom, x=x, xinfo=xinfo, views=views)
    rx, rinfo, _ = cgb.sample_posterior_(n_draws, z=z, all_sites=True)
    ref = dict(imp=cgb.impute_lg(all_sites=True), mom=cgb.moments_(np.arange(nb), all_sites=True), x=rx, xinfo=rinfo)
    return got, ref


def _against_general(tag, got, ref):
    worst = dict(mean=0.0, cov=0.0, norm=0.0, draws=0.0, impute=0.0)
    assert len(got["mom"]) == len(ref["mom"])
    for (mu, Sg, nm, inf), (rmu, rSg, rnm, rinf) in zip(got["mom"], ref["mom"]):
        assert np.array_equal(inf, rinf)
        worst["mean"] = max(worst["mean"], _rel_sites(mu, rmu))
        worst["cov"] = max(worst["cov"], _rel_sites(Sg, rSg))
        worst["norm"] = max(worst["norm"], _rel_sites(nm[:, None], rnm[:, None]))
    assert np.array_equal(got["xinfo"], ref["xinfo"])
    worst["draws"] = _rel_sites(got["x"].transpose(1, 0, 2), ref["x"].transpose(1, 0, 2))
    gi, ri = got["imp"], ref["imp"]
    assert sorted(gi) == sorted(ri)
    for k in ("families", "rows", "predicted", "info"):
        assert np.array_equal(gi[k], ri[k]), k
    assert gi["mean"].shape == ri["mean"].shape and gi["cov"].shape == ri["cov"].shape
    if gi["mean"].size:
        worst["impute"] = max(_rel_sites(gi["mean"], ri["mean"]), _rel_sites(gi["cov"], ri["cov"]))
    print(f"{tag}: against the general calls: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL, (tag, worst)


def _against_statements(tag, case, got, z, sites, impute):
    """the checked sites against the dense posterior (moments), sample_posterior_ref on the oracle's calibrated beliefs (draws)
    and the dense imputation"""
    worst = dict(mean=0.0, cov=0.0, draws=0.0, impute=0.0)
    dims, sepcl, soff, sidx, vn, off = PR.layout(case)
    for s in sites:
        pm, pc = PR.dense_posterior(case, s)
        for j, b in enumerate(case.ocgb0.belief):
            nodes = PR.belief_nodes(b)
            if len(nodes):
                mu, Sg, _, inf = got["mom"][j]
                assert inf[s] == 0
                worst["mean"] = max(worst["mean"], FR.rel(mu[s], pm[nodes]))
                worst["cov"] = max(worst["cov"], FR.rel(Sg[s], pc[np.ix_(nodes, nodes)]))
        ocgb, fam, data, kw = FR.oracle_site(case, s)
        rec = [(np.array(b.J, float), np.array(b.h, float)) for b in ocgb.belief[: ocgb.nclusters]]
        want, wi = SR.sample_posterior_ref(rec, dims, sepcl, soff, sidx, case.spt[2], case.spt[3], z[:, s, :])
        assert wi == 0 and got["xinfo"][s] == 0
        worst["draws"] = max(worst["draws"], FR.rel(got["x"][:, s, :], want))
        if impute:
            dn = PR.dense_impute(case, s)
            gi = got["imp"]
            assert sorted(dn) == sorted(int(r) for r in gi["rows"])
            for ti, r in enumerate(int(r) for r in gi["rows"]):
                if gi["predicted"][ti, 0]:
                    assert gi["info"][s, ti] == 0
                    worst["impute"] = max(worst["impute"], FR.rel(gi["mean"][s, ti, 0], dn[r][0]), FR.rel(gi["cov"][s, ti, 0, 0], dn[r][1]))
                else:
                    assert gi["info"][s, ti] == -1 and np.isnan(gi["mean"][s, ti, 0]) and np.isnan(gi["cov"][s, ti, 0, 0])
    print(f"{tag}: {len(list(sites))} sites against the dense and numpy statements: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL, (tag, worst)


def _joint(tag, case, got, z0):
    """z = 0 is the mean of moments_sites_ on every entry; a variable that several clusters hold has the same bits in all"""
    nc = case.ocgb0.nclusters
    mean = np.concatenate([got["mom"][j][0] for j in range(nc)], axis=1)   # [n_sites, size]: the layout of a draw
    e = _rel_sites(z0, mean)
    vn = SR.variable_nodes(case.ocgb0.belief, nc)
    first, shared = {}, 0
    for k, nt in enumerate(vn):
        if nt in first:
            shared += 1
            assert got["x"][:, :, k].tobytes() == got["x"][:, :, first[nt]].tobytes(), (tag, nt)
        else:
            first[nt] = k
    assert shared >= 1
    print(f"{tag}: z = 0 against the means of moments_sites_ {e:.2e}; {shared} shared entries carry the same bits")
    assert e <= TOL, tag


def _run(P, case, n, impute, sites, n_draws=3):
    cgb = _engine(P, case, n)
    size = int(cgb._lib.pgbp_sample_size(cgb._eng))
    z = np.random.default_rng(1901).standard_normal((1 + n_draws, n, size))
    z[0] = 0.0
    got, ref = _new_then_general(cgb, case.spt, z, 1 + n_draws)
    tag = f"{case.name}/{n}"
    assert not got["xinfo"].any() and not np.isnan(got["ll"]).any()
    assert (len(got["imp"]["families"]) > 0) == impute
    _against_general(tag, got, ref)
    _against_statements(tag, case, got, z, sites, impute)
    _joint(tag, case, got, got["x"][0])
    return cgb, got


# ----------------------------------------------------------------------------- 1: every case at its site counts

PLAIN = [(c, n, imp) for c, counts, imp in PR.cases() for n in counts]


@pytest.mark.parametrize("i", range(len(PLAIN)), ids=[f"{c.name}-{n}" for c, n, _ in PLAIN])
def test_calls_against_the_general_calls_and_the_statements(P, i):
    """BM at 8 (plain pool), 64 (site-minor), 65 (a ragged wavefront) and 257 sites (a second workgroup with one lane); OU with a
    fixed, random and improper root; two predicted tips next to a cherry whose parent lacks the trait (mask, NaN, info -1); the
    hybrid-tip networks N1 .. N4 under BM and OU (2-variable sepsets, 0-variable clusters, two-parent families); per-site
    shifts and tip noise with a noisy, shifted tip without data (the imputation predicts the observation).  Three random
    draws and z = 0."""
    case, n, impute = PLAIN[i]
    cgb, got = _run(P, case, n, impute, FR.checked_sites(n))
    if case is FR.missing_case():
        assert got["imp"]["predicted"][:, 0].tolist().count(False) == 2 and got["imp"]["predicted"].shape == (4, 1)
        d = P.imputed_data({k: (v[3] if k in ("mean", "cov", "info") else v) for k, v in got["imp"].items()}, cgb._lg["data"][3])
        assert int(np.isnan(d).sum()) == 2   # (imputed_data takes a site of the dict: the two predicted tips are filled)


@pytest.mark.parametrize("shape,n", PR.SHAPES)
def test_block_boundaries_and_level_shapes(P, shape, n):
    """63, 64, 65 and 130 families: the 64-belief blocks of the moments kernel (all beliefs listed) and the 64-cluster blocks
    of the validity pass; a caterpillar of 12 tips (many preorder levels of one cluster) and a balanced tree (few wide levels).
    64 sites; one draw and z = 0."""
    _run(P, PR.shape_case(shape, n), 64, False, (0, 56), n_draws=1)


def test_unit_columns_reproduce_the_dense_covariance(P):
    """z = [0; I_D] on N2 under OU at 8 sites: x[0] is the dense posterior mean and A = x[1:] - x[0] has A'A = the dense
    posterior covariance on every pair of entries, across clusters too (the check of test_gpu_sample.py), at every site"""
    case = FR.hybrid_case("N2", "ou")
    cgb = _engine(P, case, 8)
    cgb.impute_and_loglik_sites_lg(case.spt)
    D = int(cgb._lib.pgbp_sample_size(cgb._eng))
    z = np.repeat(SR.unit_draws(D)[:, None, :], 8, axis=1)
    x, info, _ = cgb.sample_posterior_sites_(1 + D, z=z)
    assert not info.any()
    vn = SR.variable_nodes(case.ocgb0.belief, case.ocgb0.nclusters)
    worst = 0.0
    for s in range(8):
        pm, pc = PR.dense_posterior(case, s)
        worst = max(worst, *SR.law_errors(x[:, s, :], vn, 1, pm, pc))
    print(f"unit columns, D = {D}, 8 sites: mean and A'A against the dense posterior {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("which", ["N2/ou", "bm"])
def test_node_moments_and_node_samples_by_label(P, which):
    """N2 under OU (two ancestors with a variable, the hybrid tip's parents) and the 40-tip BM tree: node_moments_sites and node_samples on the site-minor draws, through the node-to-entry map of an object with labelled
    beliefs (here the oracle's labels handed to an 8-site engine): every node that a cluster holds has the dense posterior's
    mean and variance at every site, and the z = 0 draw by node is that mean"""
    from helpers import product_beliefs_from_oracle
    case = FR.hybrid_case("N2", "ou") if which == "N2/ou" else FR.bm_case()
    cgb = _engine(P, case, 8)
    cgb._objs = product_beliefs_from_oracle(case.ocgb0.belief)   # (labels only: the engine's beliefs are the device's)
    cgb.impute_and_loglik_sites_lg(case.spt)
    nm = cgb.node_moments_sites()
    x, info, _ = cgb.sample_posterior_sites_(1, z=np.zeros((1, 8, int(cgb._lib.pgbp_sample_size(cgb._eng)))))
    assert not info.any()
    ent = cgb._node_entries("the test")
    # the nodes that have a variable in some cluster, from the oracle's scopes: exactly these must be held
    want_held = {n + 1 for n, _ in SR.variable_nodes(case.ocgb0.belief, case.ocgb0.nclusters)}
    worst, held = 0.0, set()
    for s in range(8):
        pm, pc = PR.dense_posterior(case, s)
        by_node = cgb.node_samples(x, site=s)
        assert sorted(by_node) == sorted(nm)
        for lab, (mean, var) in nm.items():
            if ent[lab][1][0] < 0:   # a tip with data, the fixed root: labelled in a cluster, no variable of it
                assert np.isnan(mean[s]) and np.isnan(var[s]) and np.isnan(by_node[lab][0, 0])
                continue
            held.add(lab)
            worst = max(worst, FR.rel(mean[s], pm[lab - 1]), FR.rel(var[s], pc[lab - 1, lab - 1]), FR.rel(by_node[lab][0, 0], pm[lab - 1]))
    print(f"node_moments_sites, {which}: {len(held)} nodes with a variable x 8 sites against the dense posterior {worst:.2e}")
    assert worst <= TOL and held == want_held and len(held) >= 2
    one = min(held)
    assert list(cgb.node_moments_sites([one])) == [one]
    with pytest.raises(ValueError):
        cgb.node_moments_sites([10 ** 6])


# ----------------------------------------------------------------------------- 2: the raw calls: determinism, read-only

def _raw(cgb, a, b, what, n_draws=2, seed=PR.SEED, z=None):
    """the C call on [a, b): every output as one list of arrays (sentinel-filled first)"""
    from pgbp_amd import _lib as L
    n = b - a
    dims = cgb._dims.astype(np.int64)
    nb, nm, nt = len(dims), int(dims.sum()), int((dims * (dims + 1) // 2).sum())
    f64 = lambda *shape: np.full(shape, 7.0)
    i32 = lambda *shape: np.full(shape, 7, np.int32)
    if what == "moments":
        lst = np.arange(nb, dtype=np.int32)
        out = [f64(nm, n), f64(nt, n), f64(nb, n), i32(nb, n)]
        rc = cgb._lib.pgbp_moments_sites(cgb._eng, nb, L.i32p(lst), a, b, L.f64p(out[0]), L.f64p(out[1]), L.f64p(out[2]), L.i32p(out[3]))
    elif what == "draws":
        size = int(cgb._lib.pgbp_sample_size(cgb._eng))
        out = [f64(n_draws, size, n), i32(n)]
        zp = None if z is None else L.f64p(np.ascontiguousarray(z[:, :, a:b]))
        rc = cgb._lib.pgbp_sample_posterior_sites(cgb._eng, 0, a, b, n_draws, zp, seed, L.f64p(out[0]), L.i32p(out[1]))
    else:
        nl = int(cgb._lib.pgbp_lg_impute_count(cgb._eng))
        assert nl >= 1
        out = [f64(nl, n), f64(nl, n), i32(nl, n)]
        rc = cgb._lib.pgbp_lg_impute_sites(cgb._eng, a, b, L.f64p(out[0]), L.f64p(out[1]), L.i32p(out[2]))
    assert rc == L.PGBP_OK, cgb._lib.pgbp_last_error(cgb._eng)
    assert not any(np.any(x == 7) for x in out), what
    return out


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


WHAT = ("moments", "draws", "impute")


def test_determinism_ranges_and_chunks(P):
    """600 sites, two tips without data: two calls, [0, n) against two half ranges and an odd range, and one workgroup of sites
    per chunk (the scratch limit lowered; the draws are then cut one by one as well) return the same bytes -- the draws from
    the device generator with a seed and from a host z --; the layout stays site-minor throughout"""
    case = PR.bm_missing_case()
    n = 600
    cgb = _engine(P, case, n)
    cgb.impute_and_loglik_sites_lg(case.spt)
    assert _layout(cgb) == 2
    size = int(cgb._lib.pgbp_sample_size(cgb._eng))
    z = np.random.default_rng(1902).standard_normal((2, size, n))
    for what, kw in [(w, {}) for w in WHAT] + [("draws", dict(z=z))]:
        full = _raw(cgb, 0, n, what, **kw)
        assert _same(full, _raw(cgb, 0, n, what, **kw)), what
        lo, hi = _raw(cgb, 0, 300, what, **kw), _raw(cgb, 300, n, what, **kw)
        assert _same(full, [np.concatenate([x, y], axis=-1) for x, y in zip(lo, hi)]), what
        assert _same([x[..., 77:401] for x in full], _raw(cgb, 77, 401, what, **kw)), what
        cgb._lib.pgbp_sites_sweep_scratch_limit(1)   # (one workgroup's sites at least: chunks of 256, one draw at a time)
        try:
            assert _same(full, _raw(cgb, 0, n, what, **kw)), what
        finally:
            cgb._lib.pgbp_sites_sweep_scratch_limit(0)
        assert _layout(cgb) == 2
    # another seed, another draw; the same seed through the wrapper, the same bytes
    a, b = _raw(cgb, 0, n, "draws"), _raw(cgb, 0, n, "draws", seed=PR.SEED + 1)
    assert not np.any(a[0] == b[0])
    x, info, _ = cgb.sample_posterior_sites_(2, seed=PR.SEED)
    assert x.transpose(0, 2, 1).tobytes() == a[0].tobytes() and not info.any()


def test_generator_against_the_restatement(P):
    """The device's normals against post_uni_ref.normals (numpy's Philox4x32-10, counter (entry, draw, absolute site, 1)), entry
    by entry, on sites [3, 11) of N2 under OU.  The call returns x, not z, and at one site x = m + A z is linear: A is measured
    with unit columns through the host-z path (checked against the dense posterior in the test above), z = A^-1 (x - m) is
    solved for per site (A is triangular up to the order of the entries: the condition of these A is below 1e2), and compared
    at test_gpu_simulate.py's 1e-12 absolute times max(1, cond(A)); the draw from the numpy normals through the host-z path
    agrees with the seeded draw at 1e-12 max(1, |A|_inf) as well."""
    case = FR.hybrid_case("N2", "ou")
    cgb = _engine(P, case, 16)
    cgb.impute_and_loglik_sites_lg(case.spt)
    D = int(cgb._lib.pgbp_sample_size(cgb._eng))
    nd, a, b = 3, 3, 11
    xs = _raw(cgb, a, b, "draws", n_draws=nd)[0]                       # [nd, D, 8], seeded
    zn = PR.normals(PR.SEED, np.arange(a, b), D, nd)                  # [nd, D, 8]
    zfull = np.zeros((nd, D, 16))
    zfull[:, :, a:b] = zn
    xz = _raw(cgb, a, b, "draws", n_draws=nd, z=zfull)[0]
    xu = _raw(cgb, a, b, "draws", n_draws=1 + D, z=np.repeat(SR.unit_draws(D)[:, :, None], 16, axis=2))[0]
    worst_z = worst_x = 0.0
    for s in range(b - a):
        A = (xu[1:, :, s] - xu[0, :, s]).T          # x = m + A z: column l is the response to z_l
        free = np.abs(A).sum(axis=0) > 0             # (z at the conditioned entries is ignored: those columns are 0)
        cond = np.linalg.cond(A[:, free])
        assert cond < 1e2, cond
        for d in range(nd):
            zs = np.linalg.lstsq(A[:, free], xs[d, :, s] - xu[0, :, s], rcond=None)[0]
            worst_z = max(worst_z, float(np.max(np.abs(zs - zn[d, free, s]))) / max(1.0, cond))
            worst_x = max(worst_x, float(np.max(np.abs(xs[d, :, s] - xz[d, :, s]))) / max(1.0, float(np.abs(A).sum(axis=1).max())))
    print(f"generator, {nd} draws x {D} entries x {b - a} sites: the normals solved from the seeded draws against the numpy "
          f"restatement {worst_z:.2e}, the seeded draws against the draws from numpy's normals {worst_x:.2e} (absolute, scaled)")
    assert worst_z <= 1e-12 and worst_x <= 1e-12


def test_read_only_and_both_layouts(P):
    """64 sites: the pool's bytes and pgbp_layout are unchanged by each call; a calibrate_ after the calls gives the bytes of one
    without them; the site-minor and the plain instance of the same beliefs give the same bytes"""
    case = PR.bm_missing_case()
    cgb = _engine(P, case, 64)
    cgb.impute_and_loglik_sites_lg(case.spt)
    assert _layout(cgb) == 2
    sm = {w: _raw(cgb, 0, 64, w) for w in WHAT}
    assert _layout(cgb) == 2
    cgb.pull()   # (the transfer moves the pool to the plain layout, an exact copy)
    after = cgb._packed_raw.copy()
    assert _layout(cgb) == 0
    for w in WHAT:
        assert _same(sm[w], _raw(cgb, 0, 64, w)), w
        assert _layout(cgb) == 0
        cgb.pull()
        assert np.array_equal(after, cgb._packed_raw), w
    o = cgb._opts()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    assert _layout(cgb) == 2
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)


# ----------------------------------------------------------------------------- 3: one bad lane

def test_one_bad_lane(P):
    """a site with a negative rate: its moments carry the general call's info and NaN, its draws are NaN with info = the first
    cluster in preorder (the general call's), its imputations NaN with info; its 63 wavefront neighbours keep the bytes they
    have without the failure"""
    case = PR.bm_missing_case()
    cgb = _engine(P, case, 64)
    size = int(cgb._lib.pgbp_sample_size(cgb._eng))
    z = np.random.default_rng(1903).standard_normal((2, 64, size))
    good, _ = _new_then_general(cgb, case.spt, z, 2)
    kw = dict(cgb._fam_uni_kw)
    kw["R"] = kw["R"].copy()
    kw["R"][37] = -1.0
    cgb.assignfactors_lg_(**kw)
    got, ref = _new_then_general(cgb, case.spt, z, 2)
    keep = np.arange(64) != 37
    bad_beliefs = 0
    for (mu, Sg, nm, inf), (rmu, rSg, rnm, rinf), (gmu, gSg, gnm, ginf) in zip(got["mom"], ref["mom"], good["mom"]):
        assert np.array_equal(inf, rinf) and not inf[keep].any()
        assert np.array_equal(np.isnan(mu), np.isnan(rmu)) and np.array_equal(np.isnan(nm), np.isnan(rnm))
        if inf[37]:
            bad_beliefs += 1
            assert np.isnan(mu[37]).all() and np.isnan(Sg[37]).all() and np.isnan(nm[37])
        for x, y in ((mu, gmu), (Sg, gSg), (nm, gnm), (inf, ginf)):
            assert np.ascontiguousarray(x[keep]).tobytes() == np.ascontiguousarray(y[keep]).tobytes()
    assert bad_beliefs >= 1
    order = [int(case.spt[2][0])] + [int(c) for c in case.spt[3]]
    assert got["xinfo"][37] != 0 and not got["xinfo"][keep].any() and np.array_equal(got["xinfo"], ref["xinfo"])
    dims, sepcl, soff, sidx, vn, off = PR.layout(case)
    failed = [c for c in order if dims[c] and any(got["mom"][c][3][37:38])]
    print(f"one bad lane: {bad_beliefs} beliefs of the site are not positive definite; the draws name cluster {got['xinfo'][37]}, "
          f"the first cluster in preorder whose belief failed is {failed[0] + 1 if failed else None}")
    assert np.isnan(got["x"][:, 37, :]).all()
    assert np.ascontiguousarray(got["x"][:, keep, :]).tobytes() == np.ascontiguousarray(good["x"][:, keep, :]).tobytes()
    gi, ri, oi = got["imp"], ref["imp"], good["imp"]
    assert np.array_equal(gi["info"], ri["info"]) and gi["info"][37].all() and not gi["info"][keep].any()
    assert np.isnan(gi["mean"][37]).all() and np.isnan(gi["cov"][37]).all()
    for k in ("mean", "cov", "info"):
        assert np.ascontiguousarray(gi[k][keep]).tobytes() == np.ascontiguousarray(oi[k][keep]).tobytes(), k
    assert np.isnan(got["ll"][37]) and not np.isnan(got["ll"][keep]).any()


# ----------------------------------------------------------------------------- 4: refusals

def _refused(cgb, code, word, a=0, b=None, what=WHAT, null=False, n_draws=1, tree=0, general=False):
    """each of the calls returns `code` with `word` in the message (general: and the general call to use), the outputs, the
    layout and the pool untouched"""
    from pgbp_amd import _lib as L
    b = cgb.n_sites if b is None else b
    big = 1 << 16
    cgb.pull()
    before = cgb._packed_raw.copy()
    lay = _layout(cgb)
    names = dict(moments="pgbp_moments", draws="pgbp_sample_posterior", impute="pgbp_lg_impute")
    for w in what:
        f64 = [np.full(big, 7.0) for _ in range(3)]
        i32 = np.full(big, 7, np.int32)
        d = [None if null else L.f64p(x) for x in f64]
        if w == "moments":
            rc = cgb._lib.pgbp_moments_sites(cgb._eng, 0, None, a, b, d[0], d[1], d[2], L.i32p(i32))
        elif w == "draws":
            rc = cgb._lib.pgbp_sample_posterior_sites(cgb._eng, tree, a, b, n_draws, None, 1, d[0], L.i32p(i32))
        else:
            rc = cgb._lib.pgbp_lg_impute_sites(cgb._eng, a, b, d[0], d[1], L.i32p(i32))
        msg = cgb._lib.pgbp_last_error(cgb._eng)
        assert rc == code and word.encode() in msg, (w, rc, msg)
        assert not general or f"(use {names[w]})".encode() in msg, (w, msg)
        assert all(np.all(x == 7.0) for x in f64) and np.all(i32 == 7) and _layout(cgb) == lay, w
    cgb.pull()
    assert np.array_equal(before, cgb._packed_raw)


def test_refusals(P):
    from pgbp_amd import _lib as L
    from pgbp_amd import synth
    from test_gpu_gradient import _tree_batch
    from test_gpu_gradient_sites import _oracle_batch
    from oracle import models as OM
    from oracle import network as ON
    import uni_net_ref as N
    engine, spt, *_ = _tree_batch(P, 8, 2, 50, True)
    _refused(engine(np.arange(8)), L.ERR_INVALID, "2 traits", general=True)
    # p = 1 on a network whose clique tree has a cluster of 3 nodes
    rng = np.random.default_rng(34)
    net = ON.random_network(10, 2, rng)
    taxa = list(net.tip_names)
    models = [OM.UnivariateBrownianMotion(1.0, 0.0, 1.0)] * 8
    tbls = [[[float(x) for x in rng.normal(size=len(taxa))]] for _ in range(8)]
    cgb3, _, _ = _oracle_batch(P, net, taxa, models, tbls)
    assert int(np.max(cgb3._dims)) >= 3
    _refused(cgb3, L.ERR_INVALID, "variables", general=True)
    case = FR.bm_case()
    _refused(_engine(P, case, 7), L.ERR_INVALID, "7 sites", general=True)
    cgb8 = _engine(P, case, 8)
    # no schedule yet: the draws alone need one
    _refused(cgb8, L.ERR_STATE, "no schedule", what=("draws",))
    cgb8.impute_and_loglik_sites_lg(case.spt)
    _refused(cgb8, L.ERR_INVALID, "site range", 0, 9)
    _refused(cgb8, L.ERR_INVALID, "site range", -1, 4)
    _refused(cgb8, L.ERR_INVALID, "site range", 5, 4)
    _refused(cgb8, L.ERR_INVALID, "no output buffer", null=True)
    _refused(cgb8, L.ERR_INVALID, "n_draws", what=("draws",), n_draws=0)
    _refused(cgb8, L.ERR_INVALID, "out of range", what=("draws",), tree=1)
    # the loopy Bethe graph of N1 (a hybrid tip: every belief of at most 2 variables), with its schedule: no clique tree
    bt = N.device_batch(P, "N1", "random", "bm", "bethe", 8)
    assert int(np.max(bt.dims)) <= 2
    bt.pcgb.set_schedule(bt.sched)
    _refused(bt.pcgb, L.ERR_INVALID, "clique tree", what=("draws",))
    # no family table; a table but no parameters
    tree = synth.random_tree(6, rng)
    prob = synth.cliquetree_of_tree(tree, 1)
    fresh = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=8)
    _refused(fresh, L.ERR_STATE, "pgbp_lg_setup")
    fresh.lg_setup(synth.lg_tree_table(tree, prob, 1), np.zeros((8, tree.nnodes, 1)))
    _refused(fresh, L.ERR_STATE, "pgbp_lg_assignfactors")
    # a belief index out of range
    out = np.full(16, 7.0)
    bad = np.array([0, 10 ** 6], np.int32)
    rc = cgb8._lib.pgbp_moments_sites(cgb8._eng, 2, L.i32p(bad), 0, 8, L.f64p(out), None, L.f64p(out), None)
    assert rc == L.ERR_INVALID and b"out of range" in cgb8._lib.pgbp_last_error(cgb8._eng) and np.all(out == 7.0)

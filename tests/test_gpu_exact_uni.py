"""pgbp_bm_exact_stats_sites (csrc/pgbp_exact_uni.hip) and its wrappers bm_exact_stats_sites and calibrate_exact_sites_: the
closed-form REML fit of a Brownian motion at every site of a univariate batch, lanes = sites, under a per-site mask of missing
tips and with shifts.

Comparators, never the new kernels themselves: without mask and shifts the general pgbp_bm_exact_stats and moments_ on the SAME
beliefs (called AFTER the new call, so that their layout conversion cannot help it); at every site the numpy restatement of
tests/exact_uni_ref.py over the dense flat-prior posterior and per-site GLS on the observed tips directly (both pinned to each
other in test_exact_uni_cpu.py); the score equations through the fixed-root engine and loglik_and_gradient_sites_lg, which run
none of the new device code.  Every comparison is asserted at 1e-8 relative to max(1, |block|_inf); each test prints its worst
figure."""
import ctypes as C

import numpy as np
import pytest

import exact_uni_ref as XR
import fam_uni_ref as FR
import site_missing_ref as SM
from test_gpu_fam_uni import _engine, _layout

pytestmark = pytest.mark.gpu
TOL = 1e-8
PLAIN = [(k, n) for k, counts in XR.PLAIN for n in counts]
EVERY = [(k, n) for k, counts in XR.PLAIN + XR.MASKED for n in counts]


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _rel(got, want):
    return FR.rel(got, want)


def _free(P, case, n):
    """the improper-root engine of the case's first n sites: shifts and the mask in force"""
    cgb = _engine(P, case if case.mask is None else case.base, n)
    if case.mask is not None:
        cgb.set_site_missing_lg(case.mask)
    return cgb


def _fixed(P, case, n):
    """the fixed-root engine on the same clique tree, under the same mask"""
    fx = _engine(P, case.fixed, n)
    if case.mask is not None:
        fx.set_site_missing_lg(case.mask)
    return fx


def _calibrate(cgb, spt, R=None):
    """factors of R = 1 (or per-site R), mu = 0, one calibration enqueued in the layout of the thread-per-site kernels"""
    if R is None:
        cgb.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1), sync=True)
    else:
        cgb.assignfactors_lg_(np.asarray(R, float).reshape(-1, 1, 1, 1), np.zeros((cgb.n_sites, 1)), sync=True)
    cgb._ensure_schedule([spt])
    o = cgb._opts()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    return o


def _raw(cgb, a, b, root, want_mu=True):
    """the C call on [a, b): (rc, [num, den, mu, info]) with sentinel-filled outputs"""
    from pgbp_amd import _lib as L
    n = b - a
    out = [np.full(n, 7.0), np.full(n, 7.0), np.full(n, 7.0), np.full(n, 7, np.int32)]
    rc = cgb._lib.pgbp_bm_exact_stats_sites(cgb._eng, a, b, int(root[0]), int(root[1]), L.f64p(out[0]), L.f64p(out[1]),
                                            L.f64p(out[2]) if want_mu else None, L.i32p(out[3]))
    return rc, out


def _same(x, y):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


# ----------------------------------------------------------------------------- 1: against the general calls

@pytest.mark.parametrize("key,n", PLAIN, ids=[f"{k}-{n}" for k, n in PLAIN])
def test_against_the_general_calls(P, key, n):
    """Without mask and shifts: num, den and mu against pgbp_bm_exact_stats and moments_ on the same beliefs, the general calls
    made afterwards.  8 sites: the plain layout; 64, 65: site-minor; 257: a second workgroup; trees of 63 / 64 / 65 / 130
    families: the block boundary of the partial sums."""
    case = XR.get(key, n)
    cgb = _free(P, case, n)
    _calibrate(cgb, case.spt)
    lay = _layout(cgb)
    assert bool(lay & 2) == (n >= 64)
    num, den, mu, info = P.bm_exact_stats_sites(cgb, case.root)
    assert _layout(cgb) == lay and not info.any()
    gnum, gden, ginfo = P.bm_exact_stats(cgb, all_sites=True)
    gmu = cgb.moments_([case.root[0]], cov=False, all_sites=True)[0][0][:, case.root[1]]
    assert not ginfo.any()
    worst = dict(num=_rel(num, gnum[:, 0, 0]), den=_rel(den, gden), mu=_rel(mu, gmu))
    print(f"{key}/{n}: {len(case.fam['cluster'])} families, against pgbp_bm_exact_stats and moments_: " +
          ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL


# ----------------------------------------------------------------------------- 2: against the restatement and GLS

@pytest.mark.parametrize("key,n", EVERY, ids=[f"{k}-{n}" for k, n in EVERY])
def test_against_the_restatement_and_gls(P, key, n):
    """At every site against the restatement over the dense posterior, and against GLS directly: R_hat = num / den, mu_hat,
    den against n_obs - 1.  Masks: about 30 % of the entries, a cherry wholly masked at site 2, a clade of at least 3 tips wholly
    masked at site 4 (its internal families stay in the sweep and add 0), site 1 masks nothing, bits at lanes 0 and 63 and at
    site 64; shifts: per-site values on two edges."""
    case = XR.get(key, n)
    cgb = _free(P, case, n)
    _calibrate(cgb, case.spt)
    num, den, mu, info = P.bm_exact_stats_sites(cgb, case.root)
    assert not info.any() and bool(_layout(cgb) & 2) == (n >= 64)
    ref, g = XR.reference(key, n), XR.gls_all(key, n)
    worst = dict(num=_rel(num, ref["num"]), den=_rel(den, ref["den"]), mu=_rel(mu, ref["mu"]),
                 gls_R=_rel(num / den, g["R"]), gls_mu=_rel(mu, g["mu"]), gls_den=_rel(den, g["n_obs"] - 1.0))
    per_site = float(np.max(np.abs(den - (g["n_obs"] - 1.0))))
    print(f"{key}/{n}: {n} sites against the restatement and GLS: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) +
          f"; |den - (n_obs - 1)| at most {per_site:.1e}, smallest den {den.min():.3f}")
    assert max(worst.values()) <= TOL and per_site <= TOL * float(np.max(g["n_obs"]))
    if case.mask is not None and n > XR.CLADE_SITE:
        s, cl = case.planted_mask["clade"]
        assert case.mask[s, cl].all() and abs(den[s] - (g["n_obs"][s] - 1.0)) <= TOL * g["n_obs"][s]


# ----------------------------------------------------------------------------- 3: the score equations

@pytest.mark.parametrize("key,n", [("bm40+mask", 65), ("random30+mask", 65), ("families65+mask", 64), ("bm40", 8)])
def test_score_equations(P, key, n):
    """The fixed-root engine filled per site at (R_hat den / (den + 1), mu_hat) -- the maximum-likelihood rescaling of the REML
    rate -- has a gradient in (log R, mu), from loglik_and_gradient_sites_lg, inside the project's own stopping rule
    max|g| <= 1e-8 max(1, |loglik|), and its loglik is gls_bm's optimum.  The judge runs none of the new device code."""
    case = XR.get(key, n)
    cgb = _free(P, case, n)
    _calibrate(cgb, case.spt)
    num, den, mu, info = P.bm_exact_stats_sites(cgb, case.root)
    assert not info.any()
    R_ml = (num / den) * den / (den + 1.0)
    fx = _fixed(P, case, n)
    fx.assignfactors_lg_(R_ml.reshape(n, 1, 1, 1), mu.reshape(n, 1), sync=True)
    ll, grad = fx.loglik_and_gradient_sites_lg(case.fixed.spt)
    assert not grad["info"].any()
    g_logR, g_mu = grad["dR"][:, 0, 0, 0] * R_ml, grad["dmu"][:, 0]
    score = float(np.max(np.maximum(np.abs(g_logR), np.abs(g_mu)) / np.maximum(1.0, np.abs(ll))))
    want = XR.gls_all(key, n)["loglik"]
    e_ll = float(np.max(np.abs(ll - want) / np.maximum(1.0, np.abs(want))))
    print(f"{key}/{n}: score at the ML rescaling of the closed form: max|g| / max(1, |loglik|) {score:.1e}; loglik against the GLS "
          f"optimum {e_ll:.1e}")
    assert score <= TOL and e_ll <= TOL


# ----------------------------------------------------------------------------- 4: equal bytes, state preserved

def test_equal_bytes_and_state(P):
    """Equal bytes for two calls, for site ranges split at 37 and 130, with one workgroup per chunk at 600 sites, and for the
    site-minor and the plain instance of the same beliefs; pgbp_layout, the pool and a following calibrate_ keep their bytes."""
    case = XR.get("bm40+mask", 600)
    cgb = _free(P, case, 600)
    o = _calibrate(cgb, case.spt)
    cgb.pull()
    after = cgb._packed_raw.copy()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0 and _layout(cgb) == 2
    rc, whole = _raw(cgb, 0, 600, case.root)
    assert rc == 0 and not whole[3].any() and np.all(np.isfinite(whole[0])) and _layout(cgb) == 2
    rc, again = _raw(cgb, 0, 600, case.root)
    assert rc == 0 and _same(whole, again)
    parts = [_raw(cgb, a, b, case.root) for a, b in ((0, 37), (37, 130), (130, 600))]
    assert all(rc == 0 for rc, _ in parts)
    assert _same(whole, [np.concatenate([p[1][i] for p in parts]) for i in range(4)])
    rc, nomu = _raw(cgb, 0, 600, case.root, want_mu=False)
    assert rc == 0 and _same(whole[:2], nomu[:2]) and np.all(nomu[2] == 7.0) and _same(whole[3:], nomu[3:])
    cgb._lib.pgbp_sites_sweep_scratch_limit(256)      # one workgroup's sites per chunk: three chunks
    try:
        rc, chunked = _raw(cgb, 0, 600, case.root)
        assert rc == 0 and _same(whole, chunked)
    finally:
        cgb._lib.pgbp_sites_sweep_scratch_limit(0)
    assert _layout(cgb) == 2
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)
    # the plain instance of the same beliefs: pull() converts the engine to the plain layout
    c64 = XR.get("bm40+mask", 64)
    sm = _free(P, c64, 64)
    _calibrate(sm, c64.spt)
    assert _layout(sm) == 2
    rc, a = _raw(sm, 0, 64, c64.root)
    sm.pull()
    assert rc == 0 and _layout(sm) == 0
    rc, b = _raw(sm, 0, 64, c64.root)
    assert rc == 0 and _same(a, b) and _layout(sm) == 0
    print("equal bytes: two calls, ranges split at 37 and 130, one workgroup per chunk at 600 sites, site-minor and plain")


# ----------------------------------------------------------------------------- 5: bad sites

def test_a_site_with_a_negative_rate(P):
    """a site filled with R = -1 reports info and NaN in num, den and mu; its 64 neighbours keep their bytes"""
    case = XR.get("bm40+mask", 65)
    cgb = _free(P, case, 65)
    _calibrate(cgb, case.spt, R=np.ones(65))
    rc, good = _raw(cgb, 0, 65, case.root)
    assert rc == 0 and not good[3].any()
    R = np.ones(65)
    R[37] = -1.0
    _calibrate(cgb, case.spt, R=R)
    rc, got = _raw(cgb, 0, 65, case.root)
    keep = np.arange(65) != 37
    assert rc == 0 and got[3][37] > 0 and not got[3][keep].any()
    assert np.isnan(got[0][37]) and np.isnan(got[1][37]) and np.isnan(got[2][37])
    assert all(np.array_equal(g[keep], w[keep]) for g, w in zip(got, good))
    fit = P.calibrate_exact_sites_(cgb, case.spt, case.root)   # (the driver fills R = 1 itself: every site is fine again)
    assert not fit["info"].any() and np.all(np.isfinite(fit["R"]))
    print(f"site 37 with R = -1: info {got[3][37]}, NaN; the other 64 sites keep their bytes")


def test_a_site_that_observes_one_tip(P):
    """through the driver: R = NaN with a finite den below 0.5 (n_obs - 1 = 0); the neighbours are the GLS estimates"""
    import types
    base = XR.get("bm40+mask", 65)
    rows, _ = SM.tip_rows(base)
    mask = base.mask.copy()
    mask[9, rows[1:]] = True
    mask[9, rows[0]] = False
    case = types.SimpleNamespace(**base.__dict__)
    case.mask = mask
    cgb = _free(P, case, 65)
    fit = P.calibrate_exact_sites_(cgb, case.spt, case.root)
    keep = np.arange(65) != 9
    g = XR.gls_all("bm40+mask", 65)
    print(f"site 9 observes one tip: den {fit['den'][9]:.3e}, R {fit['R'][9]}, mu {fit['mu'][9]:.6f} (the tip's value "
          f"{XR.site_values(base, 9)[rows[0]]:.6f}), info {fit['info'][9]}")
    assert np.isnan(fit["R"][9]) and np.isfinite(fit["den"][9]) and abs(fit["den"][9]) < 0.5 and fit["info"][9] == 0
    assert abs(fit["mu"][9] - XR.site_values(base, 9)[rows[0]]) <= TOL * max(1.0, abs(fit["mu"][9]))
    assert _rel(fit["R"][keep], g["R"][keep]) <= TOL and _rel(fit["mu"][keep], g["mu"][keep]) <= TOL


# ----------------------------------------------------------------------------- 6: refusals

def _refused(cgb, code, word, a=0, b=None, root=(0, 0), null=None, want_mu=True):
    from pgbp_amd import _lib as L
    n = cgb.n_sites
    b = n if b is None else b
    cgb.pull()
    before = cgb._packed_raw.copy()
    lay = _layout(cgb)
    out = [np.full(n, 7.0), np.full(n, 7.0), np.full(n, 7.0), np.full(n, 7, np.int32)]
    ptr = [L.f64p(out[0]), L.f64p(out[1]), L.f64p(out[2]) if want_mu else None, L.i32p(out[3])]
    if null is not None:
        ptr[null] = None
    rc = cgb._lib.pgbp_bm_exact_stats_sites(cgb._eng, a, b, int(root[0]), int(root[1]), *ptr)
    msg = cgb._lib.pgbp_last_error(cgb._eng).decode()
    assert rc == code and word in msg, (rc, msg, word)
    assert all(np.all(x == 7) for x in out) and _layout(cgb) == lay
    cgb.pull()
    assert np.array_equal(before, cgb._packed_raw)
    return msg


def test_refusals(P):
    """every refusal, before any launch: sentinel-filled outputs, layout and pool untouched"""
    from pgbp_amd import _lib as L
    from pgbp_amd import synth
    from oracle import models as OM
    from oracle import network as ON
    from test_gpu_gradient import _tree_batch
    from test_gpu_gradient_sites import _oracle_batch
    import uni_net_ref as N
    case = XR.get("bm40+mask", 65)
    root = case.root
    # those of pgbp_lg_gradient_sites, in its order: no table, no parameters, the range, the outputs, the engine
    rng = np.random.default_rng(34)
    tree = synth.random_tree(6, rng)
    prob = synth.cliquetree_of_tree(tree, 1)
    fresh = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=8)
    _refused(fresh, L.ERR_STATE, "pgbp_lg_setup")
    fresh.lg_setup(synth.lg_tree_table(tree, prob, 1), np.zeros((8, tree.nnodes, 1)))
    _refused(fresh, L.ERR_STATE, "pgbp_lg_assignfactors")
    cgb = _free(P, case, 65)
    _calibrate(cgb, case.spt)
    for a, b in ((0, 66), (-1, 4), (5, 4)):
        _refused(cgb, L.ERR_INVALID, "site range", a, b, root)
    _refused(cgb, L.ERR_INVALID, "no output buffer", root=root, null=0)
    _refused(cgb, L.ERR_INVALID, "no output buffer", root=root, null=1)
    engine, *_ = _tree_batch(P, 8, 2, 50, True)
    assert "pgbp_bm_exact_stats)" in _refused(engine(np.arange(8)), L.ERR_INVALID, "2 traits")
    net = ON.random_network(10, 2, rng)
    taxa = list(net.tip_names)
    wide, _, _ = _oracle_batch(P, net, taxa, [OM.UnivariateBrownianMotion(1.0, 0.0, 1.0)] * 8,
                               [[[float(x) for x in rng.normal(size=len(taxa))]] for _ in range(8)])
    assert int(np.max(wide._dims)) >= 3
    _refused(wide, L.ERR_INVALID, "variables")
    _refused(_free(P, XR.get("bm40", 7), 7), L.ERR_INVALID, "7 sites", root=root)
    # the call's own: the root out of range (only when mu is asked for)
    _refused(cgb, L.ERR_INVALID, "root belief", root=(len(cgb._dims), 0))
    _refused(cgb, L.ERR_INVALID, "root belief", root=(-1, 0))
    _refused(cgb, L.ERR_INVALID, "root position", root=(root[0], int(cgb._dims[root[0]])))
    rc, out = _raw(cgb, 0, 65, (-1, 9), want_mu=False)
    assert rc == 0 and not out[3].any() and np.all(out[2] == 7.0)
    # an OU fill; tip noise in force
    cgb.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1), model="ou", alpha=0.5, theta=np.zeros(1), sync=True)
    _refused(cgb, L.ERR_INVALID, "Ornstein-Uhlenbeck", root=root)
    cgb.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1), sync=True)
    tip = int(FR.LR.tip_families(case.fam)[0])
    cgb.set_tip_noise_lg(np.array([tip], np.int32), np.zeros((1, 1)), np.ones(1), np.full((1, 1), 0.25))
    cgb.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1), sync=True)
    assert "tip noise" in _refused(cgb, L.ERR_INVALID, "fit_sites_lg", root=root)
    cgb.clear_tip_noise_lg()
    _calibrate(cgb, case.spt)
    rc, out = _raw(cgb, 0, 65, root)
    assert rc == 0 and not out[3].any()
    # a family whose parent is the fixed root: the wording of the general call
    fx = _fixed(P, case, 65)
    _refused(fx, L.ERR_INVALID, "its parent is the fixed root: the sweep is defined on the engine with an improper root prior", root=(0, 0),
             want_mu=False)
    # a tip family with more than one parent: the hybrid-tip network N1 with an improper root
    net1, taxa1 = N.network("N1")
    rng1 = np.random.default_rng(35)
    hyb = FR._case("N1, improper root", net1, taxa1,
                   [(OM.UnivariateBrownianMotion(1.0, 0.0, np.inf), [[float(x) for x in rng1.normal(size=len(taxa1))]]) for _ in range(8)])
    h = _engine(P, hyb, 8)
    word = "a leaf with more than one parent" if int(np.max(h._dims)) <= 2 else "variables"
    print("N1 with an improper root is refused: " + _refused(h, L.ERR_INVALID, word, want_mu=False))
    # N1 .. N4 as the thread-per-site kernels take them (fixed root, every belief of at most 2 variables): whichever of the two
    # family checks meets its family first in table order
    for name in ("N1", "N2", "N3", "N4"):
        hc = FR.hybrid_case(name, "bm")
        msg = _refused(_engine(P, hc, 8), L.ERR_INVALID, "pgbp_bm_exact_stats_sites: family", want_mu=False)
        assert "a leaf with more than one parent" in msg or "its parent is the fixed root" in msg, msg
        print(f"{name} is refused: {msg}")
    # the hybrid tip's own check: N1's table with the fixed-root parents declared out of scope (parent_mask 0), so that the
    # first family either check meets is the tip with two parents
    import types
    hc = FR.hybrid_case("N1", "bm")
    fam = dict(hc.fam)
    nf, K = len(fam["cluster"]), max(1, int(fam["max_parents"]))
    pm = np.ones(nf * K, np.uint64)
    pm[np.asarray(fam["parent_pos"]).reshape(-1) < 0] = 0
    fam["parent_mask"], fam["child_mask"] = pm, np.ones(nf, np.uint64)
    hyb_tip = next(f for f in range(nf) if int(fam["child_pos"][f]) < 0 and int(fam["n_parents"][f]) > 1)
    two = types.SimpleNamespace(**hc.__dict__)
    two.fam = fam
    msg = _refused(_engine(P, two, 8), L.ERR_INVALID, f"family {hyb_tip} ", want_mu=False)
    assert "a leaf with more than one parent" in msg, msg


# ----------------------------------------------------------------------------- 7: end to end

def test_end_to_end(P):
    """calibrate_exact_sites_ on a masked 65-site case, the mask in force on both engines: R, mu and den against per-site GLS,
    loglik against the GLS log-likelihood at (R_hat, mu_hat); mu against moments_sites_ of the root."""
    key, n = "bm40+mask", 65
    case = XR.get(key, n)
    cgb, fx = _free(P, case, n), _fixed(P, case, n)
    fit = P.calibrate_exact_sites_(cgb, case.spt, case.root, fx)
    assert set(fit) == {"R", "mu", "loglik", "den", "info"} and not fit["info"].any() and fit["info"].dtype == np.int32
    g = XR.gls_all(key, n)
    want_ll = np.array([SM.gls_bm(case.cov, XR.site_values(case, s), XR.observed(case, s), fit["R"][s], fit["mu"][s])[0] for s in range(n)])
    mom = cgb.moments_sites_([case.root[0]], cov=False)[0][0][:, case.root[1]]
    worst = dict(R=_rel(fit["R"], g["R"]), mu=_rel(fit["mu"], g["mu"]), den=_rel(fit["den"], g["n_obs"] - 1.0),
                 loglik=float(np.max(np.abs(fit["loglik"] - want_ll) / np.maximum(1.0, np.abs(want_ll)))), mu_moments=_rel(fit["mu"], mom))
    print(f"calibrate_exact_sites_ on {key}/{n}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL
    # without the fixed-root engine the score is NaN, the estimates the same bytes
    fit2 = P.calibrate_exact_sites_(cgb, case.spt, case.root)
    assert np.isnan(fit2["loglik"]).all() and np.array_equal(fit2["R"], fit["R"]) and np.array_equal(fit2["mu"], fit["mu"])

"""Per-site clade shifts of the OU optimum: pgbp_lg_set_clade_shifts_sites, _update_, _slots, _get_, the fill correction
(csrc/pgbp_shift.hip: clade_shift_kernel), the scan that honours them and pgbp_lg_clade_shift_score_sites
(csrc/pgbp_optscan_uni.hip), and the drivers fit_clade_shifts_sites_lg and select_optimum_shifts_sites_lg.

Comparators, never the new code itself (tests/clade_shift_ref.py, pinned in test_clade_shift_cpu.py, which also measures the
margins these tests rely on): the dense log-likelihood and the restated scan of the model with the equivalent explicit shifts;
the dense GLS design with its joint solve and greedy path; and an existing engine painted through set_optima_lg with one
site's clades.  Every comparison is asserted at 1e-8 relative to max(1, |block|_inf); each test prints its worst figure."""
import functools

import numpy as np
import pytest

import clade_shift_ref as CS
import fam_uni_ref as FR
import optimum_scan_ref as OS
from test_gpu_fam_uni import _engine, _layout
from test_gpu_optimum_scan import _scan_engine

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _rel(got, want):
    return FR.rel(np.asarray(got, float), np.asarray(want, float))


def _records(cgb):
    cgb.pull()
    return cgb._packed_raw.copy()


def _fill(cgb):
    cgb.assignfactors_lg_(**cgb._fam_uni_kw)
    return _records(cgb)


# ----------------------------------------------------------------------------- 1: parity of the fill, loglik, score and scan

@pytest.mark.parametrize("key,n,m", CS.PARITY, ids=[f"{k}-{n}-{m}" for k, n, m in CS.PARITY])
def test_fill_loglik_score_and_scan_against_the_dense_statements(P, key, n, m):
    """8 (plain pool), 64, 65 and 257 sites; every tree shape; 1, 3 and 8 slots with 0, 1 and all slots used at different
    sites; nested, single-tip and disjoint clades; slots at lanes 0 and 63 and at site 64; fixed, random and improper roots;
    per-site shifts and noise (a noisy tip inside a shifted clade), painted optima, a per-site mask (a cherry wholly masked
    inside a shifted clade and as a slot of its own)."""
    c = OS.case(key)
    fam, delta = CS.draw_setting(c, n, m)
    used = fam >= 0
    assert used[:, 0].all() and not used[:, 1].any() and (n <= 64 or used[:, 64].all()) and (n < 64 or used[0, 63])
    cgb = _scan_engine(P, c, n)
    cgb.set_clade_shifts_sites_lg(fam, delta)
    assert cgb.clade_shift_slots_lg() == m
    got = cgb.clade_shifts_sites_lg()
    assert np.array_equal(got["family"], fam) and got["delta"].tobytes() == delta.tobytes()
    rec = _fill(cgb)
    ll, sc = cgb.loglik_and_clade_shift_score_sites_lg(c.spt)
    scan = cgb.optimum_scan_sites_lg(information=True)
    assert bool(_layout(cgb) & 2) == (n >= 64) and not sc["info"].any() and not scan["info"].any()
    ll_own, info_own = cgb.loglik_lg()     # (the fill and a postorder alone: loglik_lg honours the setting as well)
    assert not info_own.any() and _rel(ll_own, ll) <= TOL
    # the score is the scan's own rows at the site's families, to the byte; empty slots NaN
    rows = np.where(used, fam, 0)
    cols = np.arange(n)[None, :]
    H_scan, d_scan = scan["information"][cols, rows], scan["delta"][cols, rows]
    assert np.isnan(sc["g"][~used]).all() and np.isnan(sc["information"][~used]).all() and np.isnan(sc["kt"][~used]).all()
    assert sc["information"][used].tobytes() == H_scan[used].tobytes()
    ident = used & np.isfinite(sc["information"])
    assert (sc["g"][ident] / sc["information"][ident]).tobytes() == d_scan[ident].tobytes()
    assert np.isfinite(sc["g"][used]).all() and np.all(sc["kt"][used] >= 0) and np.all(sc["kt"][ident] > 0)   # (a tip masked at the site: 0)
    w_ll, w_sc, w_scan, w_rec = 0.0, 0.0, 0.0, 0.0
    twin = _scan_engine(P, c, n)
    for s in CS.checked_sites(c, n):
        w_ll = max(w_ll, abs(ll[s] - CS.loglik(c, s, fam, delta)) / max(1.0, abs(ll[s])))
        ref = CS.reference_scan(c, s, fam, delta)
        assert np.array_equal(~np.isnan(scan["delta"][s]), ref["identified"]), (key, s)
        w_scan = max(w_scan, _rel(scan["delta"][s], ref["delta"]), _rel(scan["lr"][s], ref["lr"]), _rel(scan["information"][s], ref["H"]))
        if used[:, s].any():
            g, H = CS.dense_score(c, s, fam, delta)
            for i, j in enumerate(np.flatnonzero(used[:, s])):
                if ref["identified"][fam[j, s]]:
                    w_sc = max(w_sc, abs(sc["g"][j, s] - g[i]) / max(1.0, abs(g[i])), abs(sc["information"][j, s] - H[i, i]) / max(1.0, abs(H[i, i])))
                else:
                    assert np.isnan(sc["information"][j, s]) and abs(sc["g"][j, s]) <= TOL
            # an existing engine painted with this site's clades: the filled records of the site
            reg, vals = CS.device_painting(c, s, fam, delta)
            twin.set_optima_lg(reg, np.tile(vals[None, :, None], (n, 1, 1)))
            w_rec = max(w_rec, _rel(rec[s], _fill(twin)[s]))
    print(f"{c.name}/{n}/{m}: loglik against the dense oracle {w_ll:.2e}; filled records against an engine painted per site {w_rec:.2e}; "
          f"score against the dense design {w_sc:.2e}; the next scan against the restatement {w_scan:.2e}")
    assert max(w_ll, w_rec, w_sc, w_scan) <= TOL
    if getattr(c, "mask", None) is not None and c.planted_mask["cherry"] is not None:
        site, f, _ = c.planted_mask["cherry"]     # the planted unidentified slot is reported; the clade around it in slot 0
        j = int(np.flatnonzero(fam[:, site] == f)[0])   # is classified as the restatement classifies it (the loop above)
        assert np.isnan(sc["information"][j, site]) and not sc["identified"][j, site] and abs(sc["g"][j, site]) <= TOL
        assert bool(sc["identified"][0, site]) == bool(CS.reference_scan(c, site, fam, delta)["identified"][fam[0, site]])


def test_shared_clades_against_a_painted_engine(P):
    """every site with the same two nested clades: records, log-likelihood and the next scan's delta / lr equal those of an
    engine painted through add_optimum_shift + set_optima_lg"""
    c = OS.case("main")
    n = 65
    h = OS.heights(c.fam)
    a = int(np.flatnonzero(h == h.max() // 2)[0])
    b = OS.children_of(c.fam)[a][0]
    rng = np.random.default_rng(7)
    fam = np.tile(np.array([[a], [b]], np.int32), (1, n))
    delta = rng.normal(size=(2, n))
    cgb = _scan_engine(P, c, n)
    cgb.set_clade_shifts_sites_lg(fam, delta)
    rec = _fill(cgb)
    ll, scan = cgb.loglik_and_optimum_scan_sites_lg(c.spt)
    twin = _scan_engine(P, c, n)
    reg0 = np.zeros((len(h), 1), np.int32)
    reg1, o1 = P.add_optimum_shift(reg0, c.fam["parent_family"], a)
    reg2, o2 = P.add_optimum_shift(reg1, c.fam["parent_family"], b)
    assert o1.tolist() == [0] and o2.tolist() == [1, 1]
    theta = cgb._fam_uni_kw["theta"][:n, 0]
    twin.set_optima_lg(reg2, np.stack([theta + delta[0], theta + delta[0] + delta[1]], axis=1)[:, :, None])
    rec2 = _fill(twin)
    ll2, scan2 = twin.loglik_and_optimum_scan_sites_lg(c.spt)
    worst = max(_rel(rec, rec2), _rel(ll, ll2), _rel(scan["delta"], scan2["delta"]), _rel(scan["lr"], scan2["lr"]))
    print(f"{c.name}: two shared nested clades against the painted engine {worst:.2e}")
    assert worst <= TOL and np.array_equal(np.isnan(scan["delta"]), np.isnan(scan2["delta"]))


# ----------------------------------------------------------------------------- 2: the joint refit and the selection

@pytest.mark.parametrize("key,n,m", [("main", 65, 3), ("improper", 64, 3), ("optima", 65, 8), ("balanced", 64, 8)])
def test_fit_against_the_dense_joint_gls(P, key, n, m):
    c = OS.case(key)
    fam, delta = CS.draw_setting(c, n, m)
    cgb = _scan_engine(P, c, n)
    cgb.set_clade_shifts_sites_lg(fam, delta)
    fit = P.fit_clade_shifts_sites_lg(cgb, c.spt)
    used = fam >= 0
    assert not fit["info"].any() and not fit["identified"][~used].any()
    after = cgb.clade_shift_score_sites_lg()
    scan = cgb.optimum_scan_sites_lg()
    assert cgb.clade_shifts_sites_lg()["delta"].tobytes() == fit["delta"].tobytes()
    w, w_g, w_d, dropped = 0.0, 0.0, 0.0, 0
    for s in CS.checked_sites(c, n):
        u = np.flatnonzero(used[:, s])
        ref = CS.dense_fit(c, s, fam, delta)
        if ref["singular"]:      # not jointly identified (a cherry's parent and both its tips): a slot is dropped, none raises
            assert not fit["identified"][u, s].all() and np.isfinite(fit["delta"][:, s]).all()
            dropped += 1
            continue
        assert fit["identified"][u, s].all(), (key, s)
        if len(u) == 0:
            w = max(w, abs(fit["loglik"][s] - ref["loglik"]) / max(1.0, abs(ref["loglik"])))
            continue
        w = max(w, _rel(fit["delta"][u, s], ref["delta"]), _rel(fit["H"][s][np.ix_(u, u)], ref["H"]), _rel(fit["se"][u, s], ref["se"]),
                abs(fit["loglik"][s] - ref["loglik"]) / max(1.0, abs(ref["loglik"])))
        w_g = max(w_g, float(np.max(np.abs(after["g"][u, s])) / max(1.0, np.max(np.abs(fit["g"][u, s])))))
        w_d = max(w_d, float(np.max(np.abs(scan["delta"][s, fam[u, s]])) / max(1.0, np.max(np.abs(ref["delta"])))))
    print(f"{c.name}/{n}/{m}: deltas, H, se, loglik against the dense joint GLS {w:.2e}; score afterwards {w_g:.2e} of max(1, |g0|); "
          f"|delta| of a scan afterwards at the slots {w_d:.2e}; {dropped} checked sites not jointly identified")
    assert max(w, w_g, w_d) <= TOL
    assert dropped == 0 or key == "balanced"


@pytest.mark.parametrize("key", ["fixed", "planted"])
def test_selection_against_the_dense_greedy_path(P, key):
    """forward selection of up to three clades at 64 sites at once against the dense greedy path of every site: the families
    equal, deltas, lr at entry and the log-likelihood path at tolerance; the planted case (two clades per site, different at
    different sites) recovers the planted families, on the reference and on the device"""
    c = CS.select_case(key)
    n = CS.SELECT_SITES
    cgb = _scan_engine(P, c, n)
    out = P.select_optimum_shifts_sites_lg(cgb, c.spt, CS.MAX_SHIFTS, CS.MIN_LR)
    assert not out["info"].any() and out["family"].shape == (CS.MAX_SHIFTS, n)
    worst = 0.0
    for s in range(n):
        ref = CS.greedy(key, s)
        k = ref["n_shifts"]
        assert out["n_shifts"][s] == k and np.array_equal(out["family"][:, s], ref["family"]), (key, s)
        worst = max(worst, _rel(out["delta"][:, s], ref["delta"]), _rel(out["lr"][:k, s], ref["lr"]),
                    _rel(out["loglik"][:k + 1, s], ref["loglik"]))
        assert np.isnan(out["lr"][k:, s]).all()
        if key == "planted":
            assert sorted(ref["family"][:2].tolist()) == sorted(c.planted[0][:, s].tolist()) == sorted(out["family"][:2, s].tolist())
    got = cgb.clade_shifts_sites_lg()
    assert np.array_equal(got["family"], out["family"]) and got["delta"].tobytes() == out["delta"].tobytes()
    print(f"{c.name}: {int(out['n_shifts'].sum())} shifts over {n} sites against the dense greedy path {worst:.2e}")
    assert worst <= TOL


# ----------------------------------------------------------------------------- 3: equal bytes, lifetime

def _score_raw(cgb, a, b, min_info=1e-8):
    from pgbp_amd import _lib as L
    m, n = cgb.clade_shift_slots_lg(), b - a
    out = [np.full((m, n), 7.0), np.full((m, n), 7.0), np.full((m, n), 7.0), np.full(n, 7, np.int32)]
    rc = cgb._lib.pgbp_lg_clade_shift_score_sites(cgb._eng, a, b, min_info, L.f64p(out[0]), L.f64p(out[1]), L.f64p(out[2]), L.i32p(out[3]))
    assert rc == L.PGBP_OK, cgb._lib.pgbp_last_error(cgb._eng)
    return out


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_equal_bytes_for_calls_ranges_chunks_and_layouts(P):
    """600 sites, 130 families, 3 slots: the fill twice; the score twice, split at 37 and 130, one workgroup per chunk, and on
    the plain instance; update after set against a full set"""
    c = OS.ou_shape("families", 130, ns=600, seed=9, draw="normal")
    n = 600
    fam, delta = CS.draw_setting(c, n, 3)
    cgb = _scan_engine(P, c, n)
    cgb.set_clade_shifts_sites_lg(fam, delta)
    rec = _fill(cgb)
    assert rec.tobytes() == _fill(cgb).tobytes()
    ll, sc = cgb.loglik_and_clade_shift_score_sites_lg(c.spt)
    assert _layout(cgb) == 2 and not sc["info"].any()
    full = _score_raw(cgb, 0, n)
    assert _same(full, _score_raw(cgb, 0, n)) and full[0].tobytes() == sc["g"].tobytes()
    parts = [_score_raw(cgb, a, b) for a, b in ((0, 37), (37, 130), (130, n))]
    assert _same(full, [np.concatenate(q, axis=-1) for q in zip(*parts)])
    cgb._lib.pgbp_sites_sweep_scratch_limit(256 * (130 * 5 + 3 * 3 + 8))
    try:
        assert _same(full, _score_raw(cgb, 0, n))
    finally:
        cgb._lib.pgbp_sites_sweep_scratch_limit(0)
    cgb.pull()   # (the transfer moves the pool to the plain layout, an exact copy)
    assert _layout(cgb) == 0 and _same(full, _score_raw(cgb, 0, n)) and _layout(cgb) == 0
    # update after set = a full set
    d2 = np.where(fam >= 0, delta * 0.5 - 1.0, 0.0)
    cgb.update_clade_shifts_sites_lg(d2)
    a = _fill(cgb)
    other = _scan_engine(P, c, n)
    other.set_clade_shifts_sites_lg(fam, d2)
    assert a.tobytes() == _fill(other).tobytes() and a.tobytes() != rec.tobytes()


def test_plain_and_site_minor_fill_give_the_same_bytes(P):
    """the first 8 sites of a batch filled in the plain layout (an 8-site engine) and in the site-minor one (64 sites).  The
    fills underneath are different kernels in the two layouts and may differ in the last bit on their own; the correction is one
    kernel: wherever the records agree to the byte without a setting they agree to the byte with it, and at 1e-8 everywhere"""
    c = OS.case("main")
    fam, delta = CS.draw_setting(c, 64, 3)
    big, small = _scan_engine(P, c, 64), _scan_engine(P, c, 8)
    a0, b0 = _fill(big)[:8], _fill(small)
    big.set_clade_shifts_sites_lg(fam, delta)
    small.set_clade_shifts_sites_lg(fam[:, :8], delta[:, :8])
    a, b = _fill(big)[:8], _fill(small)
    same = a0 == b0
    assert (_layout(small) & 2) == 0 and same.mean() >= 0.9 and (a != a0).any()
    assert np.array_equal(a[same], b[same]) and a[same].tobytes() == b[same].tobytes() and _rel(a, b) <= TOL
    ll_a, sa = big.loglik_and_clade_shift_score_sites_lg(c.spt)
    ll_b, sb = small.loglik_and_clade_shift_score_sites_lg(c.spt)
    assert bool(_layout(big) & 2) and not (_layout(small) & 2)
    assert _rel(ll_a[:8], ll_b) <= TOL and _rel(sa["g"][:, :8], sb["g"]) <= TOL
    print(f"plain against site-minor: {same.mean():.4f} of the entries agree to the byte before and after the correction")


@pytest.mark.parametrize("n", [8, 65])
def test_lifetime_of_the_setting(P, n):
    """set-then-clear and a BM fill give the bytes of an engine that never had a setting; the setting survives set_edges_lg and
    the other setters; lg_setup and a new topology clear it"""
    c = OS.case("main")
    fam, delta = CS.draw_setting(c, n, 3)
    never = _scan_engine(P, c, n)
    base = _fill(never)
    never.set_schedule([c.spt])
    ll0 = never.loglik_lg()[0]
    cgb = _scan_engine(P, c, n)
    cgb.set_schedule([c.spt])
    cgb.set_clade_shifts_sites_lg(fam, delta)
    with_setting = _fill(cgb)
    assert with_setting.tobytes() != base.tobytes()
    untouched = ~(fam >= 0).any(axis=0)
    assert untouched[1] and with_setting[untouched].tobytes() == base[untouched].tobytes()   # a site without slots: nothing stored
    # BM: no effect, byte for byte
    kw_bm = {k: v for k, v in cgb._fam_uni_kw.items() if k not in ("model", "alpha", "theta")}
    cgb.assignfactors_lg_(**kw_bm)
    never.assignfactors_lg_(**kw_bm)
    assert _records(cgb).tobytes() == _records(never).tobytes() and cgb.clade_shift_slots_lg() == 3
    # the other setters leave it in force
    cgb.set_edges_lg(np.asarray(c.fam["length"], float), np.asarray(c.fam["gamma"], float))
    cgb.clear_shifts_lg()
    cgb.clear_optima_lg()
    cgb.clear_tip_noise_lg()
    cgb.set_site_missing_lg(None)
    cgb.set_data_lg(cgb.get_data_lg())
    assert cgb.clade_shift_slots_lg() == 3 and _fill(cgb).tobytes() == with_setting.tobytes()
    # clear: the bytes of an engine that never had one
    cgb.clear_clade_shifts_sites_lg()
    assert cgb.clade_shift_slots_lg() == 0 and cgb.clade_shifts_sites_lg() is None
    assert _fill(cgb).tobytes() == base.tobytes() and cgb.loglik_lg()[0].tobytes() == ll0.tobytes()
    # a new topology and a new lg_setup clear it
    cgb.set_clade_shifts_sites_lg(fam, delta)
    assert cgb._lib.pgbp_lg_set_topology(cgb._eng, _i32(c.fam["parent_family"])) == 0
    assert cgb.clade_shift_slots_lg() == 0
    cgb.set_clade_shifts_sites_lg(fam, delta)
    data = np.array([[[float(v)] for v in tbl[0]] for _, tbl in c.sites[:n]])
    cgb.lg_setup(c.fam, data)
    assert cgb.clade_shift_slots_lg() == 0
    cgb.assignfactors_lg_(**cgb._fam_uni_kw)
    assert _records(cgb).tobytes() == base.tobytes()


def _i32(x):
    from pgbp_amd import _lib as L
    a = np.ascontiguousarray(np.asarray(x).reshape(-1), np.int32)
    _i32.keep = a
    return L.i32p(a)


def test_one_bad_lane(P):
    """a site with a negative rate reports info and NaN; its 63 neighbours keep the bytes they have without it"""
    c = OS.case("fixed")
    fam, delta = CS.draw_setting(c, 64, 3)
    fam[:, 37] = fam[:, 0]
    delta[:, 37] = 1.0
    cgb = _scan_engine(P, c, 64)
    cgb.set_clade_shifts_sites_lg(fam, delta)
    ll, good = cgb.loglik_and_clade_shift_score_sites_lg(c.spt)
    kw = dict(cgb._fam_uni_kw)
    kw["R"] = kw["R"].copy()
    kw["R"][37] = -1.0
    cgb.assignfactors_lg_(**kw)
    ll2, got = cgb.loglik_and_clade_shift_score_sites_lg(c.spt)
    keep = np.arange(64) != 37
    assert got["info"][37] != 0 and not got["info"][keep].any() and np.isnan(ll2[37])
    for k in ("g", "information", "kt"):
        assert np.isnan(got[k][:, 37]).all(), k
        assert got[k][:, keep].tobytes() == good[k][:, keep].tobytes(), k
    assert ll2[keep].tobytes() == ll[keep].tobytes()


# ----------------------------------------------------------------------------- 4: refusals

def _set_refused(cgb, code, fam, delta, *words):
    """the setter returns `code` with the words in the message; layout, pool and the setting in force untouched"""
    from pgbp_amd import _lib as L
    before = _records(cgb)
    lay, slots, old = _layout(cgb), cgb.clade_shift_slots_lg(), cgb.clade_shifts_sites_lg() if cgb.clade_shift_slots_lg() > 0 else None
    fam = np.ascontiguousarray(fam, np.int32)
    delta = np.ascontiguousarray(delta, np.float64)
    rc = cgb._lib.pgbp_lg_set_clade_shifts_sites(cgb._eng, fam.shape[0], L.i32p(fam), L.f64p(delta))
    msg = cgb._lib.pgbp_last_error(cgb._eng)
    assert rc == code and all(w.encode() in msg for w in words), (rc, msg)
    assert _layout(cgb) == lay and cgb.clade_shift_slots_lg() == slots and np.array_equal(before, _records(cgb))
    if old is not None:
        now = cgb.clade_shifts_sites_lg()
        assert np.array_equal(now["family"], old["family"]) and now["delta"].tobytes() == old["delta"].tobytes()


def test_refusals_leave_everything_untouched(P):
    from pgbp_amd import _lib as L
    from test_gpu_gradient import _tree_batch
    import uni_net_ref as N
    c = OS.case("main")
    n = 65
    one = lambda k: (np.full((1, k), 2, np.int32), np.ones((1, k)))
    # a non-thread-per-site engine (two traits; seven sites), no topology, a two-parent family
    engine, spt, *_ = _tree_batch(P, 8, 2, 50, True)
    _set_refused(engine(np.arange(8)), L.ERR_INVALID, *one(8), "2 traits")
    _set_refused(_engine(P, OS.base_of(c), 7), L.ERR_INVALID, *one(7), "7 sites")
    b = OS.base_of(c)
    dims, sepcl, so, si = N.engine_arrays(P, b.ocgb0)
    fresh = P.ClusterGraphBelief.from_arrays(dims, sepcl, so, si, None, n_sites=8)
    _set_refused(fresh, L.ERR_STATE, *one(8), "pgbp_lg_setup")
    data = np.array([[[float(v)] for v in tbl[0]] for _, tbl in b.sites[:8]])
    fresh.lg_setup({k: v for k, v in b.fam.items() if k != "parent_family"}, data)
    _set_refused(fresh, L.ERR_STATE, *one(8), "pgbp_lg_set_topology")
    a = N.device_batch(P, "N1", "fixed", "ou", "cliquetree", 65)
    first = int(np.flatnonzero(np.asarray(a.fam["n_parents"]) >= 2)[0])
    _set_refused(a.pcgb, L.ERR_INVALID, *one(65), f"family {first} has 2 parents")
    # a setting in force: every refused setter leaves it in force
    fam, delta = CS.draw_setting(c, n, 3)
    cgb = _scan_engine(P, c, n)
    cgb.set_clade_shifts_sites_lg(fam, delta)
    cgb.loglik_and_clade_shift_score_sites_lg(c.spt)
    nf = len(c.fam["cluster"])
    bad = fam.copy(); bad[2, 40] = bad[0, 40] if bad[0, 40] >= 0 else 5; bad[0, 40] = bad[2, 40]
    _set_refused(cgb, L.ERR_INVALID, bad, delta, f"family {int(bad[0, 40])} appears twice at site 40")
    bad = fam.copy(); bad[1, 9] = nf
    _set_refused(cgb, L.ERR_INVALID, bad, delta, f"family {nf} out of range", "site 9")
    bad = fam.copy(); bad[0, 3] = -2
    _set_refused(cgb, L.ERR_INVALID, bad, delta, "family -2 out of range")
    rc = OS.case("random")
    root_prior = int(np.flatnonzero(np.asarray(rc.fam["n_parents"]) == 0)[0])
    rcgb = _scan_engine(P, rc, 64)
    _set_refused(rcgb, L.ERR_INVALID, np.full((1, 64), root_prior, np.int32), np.ones((1, 64)), "root-prior", f"family {root_prior}")
    bad_d = delta.copy(); bad_d[np.flatnonzero(fam[:, 64] >= 0)[0], 64] = np.inf
    _set_refused(cgb, L.ERR_INVALID, fam, bad_d, "not finite", "site 64")
    with pytest.raises(L.PgbpError, match="not finite"):
        cgb.update_clade_shifts_sites_lg(bad_d)
    assert cgb.clade_shifts_sites_lg()["delta"].tobytes() == delta.tobytes()
    # the calls that do not honour the setting refuse under OU, with the setter named and nothing touched
    before, lay = _records(cgb), _layout(cgb)
    calls = [cgb.gradient_sites_lg, cgb.shift_scan_sites_lg, cgb.edge_gradient_sites_lg, cgb.loo_sites_lg,
             lambda: cgb.gradient_lg(all_sites=True), lambda: cgb.edge_gradient_lg(all_sites=True), lambda: cgb.shift_scan_lg(all_sites=True),
             lambda: cgb.loo_lg(all_sites=True), lambda: cgb.simulate_lg(seed=1, all_sites=True)]
    for call in calls:
        with pytest.raises(L.PgbpError, match="pgbp_lg_set_clade_shifts_sites") as err:
            call()
        assert err.value.code == L.ERR_INVALID
    assert _layout(cgb) == lay and np.array_equal(before, _records(cgb)) and cgb.clade_shift_slots_lg() == 3
    with pytest.raises(L.PgbpError):
        P.bootstrap_optimum_scan_lg(cgb, c.spt, seed=1)
    # the score call's own refusals: no setting; a scratch limit below one workgroup names the doubles that suffice
    cgb._lib.pgbp_sites_sweep_scratch_limit(1000)
    try:
        out = [np.full((3, n), 7.0) for _ in range(3)] + [np.full(n, 7, np.int32)]
        rc_ = cgb._lib.pgbp_lg_clade_shift_score_sites(cgb._eng, 0, n, 1e-8, L.f64p(out[0]), L.f64p(out[1]), L.f64p(out[2]), L.i32p(out[3]))
        msg = cgb._lib.pgbp_last_error(cgb._eng).decode()
        assert rc_ == L.ERR_INVALID and "suffices" in msg and all(np.all(x == 7) for x in out)
        need = int(msg.split("pgbp_sites_sweep_scratch_limit: ")[1].split(" ")[0])
        assert 256 * (nf * 5 + 9) <= need <= 256 * (nf * 5 + 9 + 16)
        cgb._lib.pgbp_sites_sweep_scratch_limit(need)
        assert not cgb.clade_shift_score_sites_lg()["info"].any()
    finally:
        cgb._lib.pgbp_sites_sweep_scratch_limit(0)
    cgb.clear_clade_shifts_sites_lg()
    with pytest.raises(L.PgbpError, match="set_clade_shifts_sites"):
        cgb.clade_shift_score_sites_lg()
    cgb.gradient_sites_lg()     # and with the setting gone the gradient runs again

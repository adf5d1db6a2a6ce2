"""pgbp_lg_optimum_scan_sites (csrc/pgbp_optscan_uni.hip) and its wrappers optimum_scan_sites_lg,
loglik_and_optimum_scan_sites_lg, add_optimum_shift and bootstrap_optimum_scan_lg: every edge of a univariate batch scanned
for a shift of the optimum of its clade under OU, lanes = sites.

Comparators, never the new code itself (tests/optimum_scan_ref.py, pinned in test_optimum_scan_cpu.py, which also checks the
margins of identification these tests rely on): at every site the numpy restatement of the recursion over the dense posterior
moments; at one site in eight the dense GLS statement; and, independent of both, the device's own log-likelihood with the clade
painted.  Every comparison is asserted at 1e-8 relative to max(1, |block|_inf); each test prints its worst figure."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import fam_uni_ref as FR
import optimum_scan_ref as OS
from test_gpu_fam_uni import _engine, _layout

pytestmark = pytest.mark.gpu
TOL = 1e-8
RUNS = [(key, n) for key, counts in OS.CASES for n in counts]


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


@functools.lru_cache(maxsize=None)
def _reference(key, s):
    return OS.reference_site(OS.case(key), s)


def _scan_engine(P, c, n):
    """the engine of the first n sites of a case: per-site parameters, shifts and noise (test_gpu_fam_uni._engine), then the
    case's mask and painted optima, factors assigned"""
    cgb = _engine(P, OS.base_of(c), n)
    assert cgb._fam_uni_kw.get("model") == "ou"
    if getattr(c, "mask", None) is not None:
        assert n == c.n
        cgb.set_site_missing_lg(c.mask)
    if getattr(c, "optima", None) is not None:
        cgb.set_optima_lg(OS.device_regime(c), c.optima[1][:n, :, None])
    cgb.assignfactors_lg_(**cgb._fam_uni_kw)
    return cgb


def _own_top(tag, sc, fam):
    """top_lr is the maximum of the call's own lr table over the identified families that have a parent, to the byte,
    top_family its first argmax"""
    real = np.asarray(fam["n_parents"]) >= 1
    lr = np.where(real[None, :] & ~np.isnan(sc["delta"]) & np.isfinite(sc["lr"]), sc["lr"], -np.inf)
    f = np.argmax(lr, axis=1)
    top = lr[np.arange(lr.shape[0]), f]
    assert sc["top_lr"].tobytes() == top.tobytes(), tag
    assert np.array_equal(sc["top_family"], np.where(np.isfinite(top), f, -1)), tag


# ----------------------------------------------------------------------------- 1: every case at its site counts

@pytest.mark.parametrize("key,n", RUNS, ids=[f"{k}-{n}" for k, n in RUNS])
def test_scan_against_the_restatement_and_dense_gls(P, key, n):
    """8 (plain pool), 64 (site-minor), 65 (a ragged wavefront) and 257 sites (a second workgroup with one lane); a fixed, a
    random and an improper root; a 2-tip tree; a caterpillar and a balanced tree (most and fewest height launches); a
    trifurcation; 63 / 64 / 65 / 130 families; per-site shifts and tip noise; per-site masks; two regimes already painted."""
    c = OS.case(key)
    cgb = _scan_engine(P, c, n)
    ll, sc = cgb.loglik_and_optimum_scan_sites_lg(c.spt, information=True)
    lay = _layout(cgb)
    assert bool(lay & 2) == (n >= 64) and not sc["info"].any()
    nf = len(c.fam["cluster"])
    assert sc["delta"].shape == sc["lr"].shape == sc["information"].shape == sc["se"].shape == (n, nf)
    worst = 0.0
    for s in range(n):
        ref = _reference(key, s)
        assert np.array_equal(~np.isnan(sc["delta"][s]), ref["identified"]), (key, s)
        worst = max(worst, FR.rel(sc["delta"][s], ref["delta"]), FR.rel(sc["lr"][s], ref["lr"]), FR.rel(sc["information"][s], ref["H"]),
                    FR.rel(sc["se"][s], 1.0 / np.sqrt(ref["H"])))
    print(f"{c.name}/{n}: every site against the restatement {worst:.2e}")
    assert worst <= TOL
    worst = 0.0
    for s in OS.checked_sites(c, n):
        dev = dict(delta=sc["delta"][s], lr=sc["lr"][s], H=sc["information"][s], identified=~np.isnan(sc["delta"][s]))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, OS.against_gls(dev, OS.gls(c, s)))
    print(f"{c.name}/{n}: one site in eight against dense GLS {worst:.2e}")
    assert worst <= TOL
    _own_top(f"{key}/{n}", sc, c.fam)
    if getattr(c, "mask", None) is not None and c.planted_mask["cherry"] is not None:
        # the planted unidentified edge: a cherry wholly masked at one site -- not identified there, identified next to it
        site, f, _ = c.planted_mask["cherry"]
        assert np.isnan(sc["delta"][site, f]) and sc["lr"][site, f] == 0.0 and np.isnan(sc["information"][site, f])
        assert np.isfinite(sc["delta"][[site - 1, site + 1], f]).all() and sc["top_family"][site] != f
    # tables=False: the two summaries alone, the same bytes; the layout as the calibration left it
    only = cgb.optimum_scan_sites_lg(tables=False)
    assert sorted(only) == ["info", "top_family", "top_lr"] and _layout(cgb) == lay
    assert only["top_lr"].tobytes() == sc["top_lr"].tobytes() and np.array_equal(only["top_family"], sc["top_family"])
    ll2, again = cgb.loglik_and_optimum_scan_sites_lg(c.spt, tables=False)
    assert again["top_lr"].tobytes() == sc["top_lr"].tobytes() and ll.tobytes() == ll2.tobytes()


# ----------------------------------------------------------------------------- 2: end to end, the device's own log-likelihood

@pytest.mark.parametrize("key", ["main", "everything"])
def test_painting_the_clade_gains_lr_and_the_next_scan_vanishes(P, key):
    """One edge: its clade painted with add_optimum_shift and the per-site values delta[site]; twice the change of the
    device's own log-likelihood is lr[site] at every identified site, and a second scan returns delta = 0 there.  With two
    regimes already painted the clade meets them and theta: three new regimes."""
    c = OS.case(key)
    n = 65
    cgb = _scan_engine(P, c, n)
    ll0, sc0 = cgb.loglik_and_optimum_scan_sites_lg(c.spt)
    h = OS.heights(c.fam)
    if key == "main":
        f = int(np.flatnonzero(h == h.max() // 2)[0])
    else:                     # the edge above the first painted clade (that clade's own edge where it hangs off the root)
        pa = int(np.asarray(c.fam["parent_family"]).reshape(len(h), -1)[c.painted[0], 0])
        f = pa if pa >= 0 else int(c.painted[0])
    ident = ~np.isnan(sc0["delta"][:, f])
    assert ident.sum() >= n - 2
    d_hat = np.where(ident, sc0["delta"][:, f], 0.0)
    reg0 = OS.device_regime(c)
    reg1, origin = P.add_optimum_shift(reg0, c.fam["parent_family"], f)
    theta = cgb._fam_uni_kw["theta"][:n, 0]
    old = np.concatenate([theta[:, None], c.optima[1][:n]], axis=1) if getattr(c, "optima", None) is not None else theta[:, None]
    n_old = old.shape[1] - 1
    vals = np.concatenate([old[:, 1:], old[:, origin[n_old:]] + d_hat[:, None]], axis=1)
    assert len(set(origin[n_old:].tolist())) == len(origin) - n_old >= (2 if key == "everything" and f != c.painted[0] else 1)
    cgb.set_optima_lg(reg1, vals[:, :, None])
    ll1, sc1 = cgb.loglik_and_optimum_scan_sites_lg(c.spt)
    e_lr = float(np.max(np.abs(2 * (ll1 - ll0) - sc0["lr"][:, f])[ident] / np.maximum(1.0, np.abs(ll0[ident]))))
    e_d = float(np.max(np.abs(sc1["delta"][:, f])[ident] / np.maximum(1.0, np.abs(d_hat[ident]))))
    print(f"{c.name}: family {f} (height {h[f]}), {int(ident.sum())} sites: 2 x the gain of loglik against lr {e_lr:.2e} of max(1, |ll|); "
          f"|delta| of the second scan {e_d:.2e} of max(1, |delta_hat|)")
    assert e_lr <= TOL and e_d <= TOL and np.all(sc0["lr"][ident, f] > 0)


# ----------------------------------------------------------------------------- 3: determinism, read-only

def _raw(cgb, a, b, tables=True, min_info=1e-8, timed=False):
    """the C call on [a, b): every output as one list of arrays (sentinel-filled first)"""
    from pgbp_amd import _lib as L
    n = b - a
    nf = len(cgb._lg["cluster"])
    out = [np.full((nf, n), 7.0), np.full((nf, n), 7.0), np.full((nf, n), 7.0), np.full(n, 7.0), np.full(n, 7, np.int32), np.full(n, 7, np.int32)]
    t = [L.f64p(x) if tables else None for x in out[:3]]
    if timed:
        ms, cnt = np.zeros(4), np.zeros(1, np.int32)
        rc = cgb._lib.pgbp_lg_optimum_scan_sites_timed(cgb._eng, a, b, min_info, t[0], t[1], t[2], L.f64p(out[3]), L.i32p(out[4]),
                                                       L.i32p(out[5]), L.f64p(ms), L.i32p(cnt))
        out = out + [ms, cnt]
    else:
        rc = cgb._lib.pgbp_lg_optimum_scan_sites(cgb._eng, a, b, min_info, t[0], t[1], t[2], L.f64p(out[3]), L.i32p(out[4]), L.i32p(out[5]))
    assert rc == L.PGBP_OK, cgb._lib.pgbp_last_error(cgb._eng)
    return out


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_equal_bytes_for_calls_ranges_chunks_and_layouts(P):
    """600 sites, 130 families, two regimes painted with per-site values: two calls; the ranges split at 37 and 130; one
    workgroup's sites per chunk (the scratch limit lowered to what 256 sites take); the timed twin; the site-minor and the
    plain instance -- the same bytes in every output; pool, layout and a following calibration keep their bytes."""
    c = OS.with_optima(OS.ou_shape("families", 130, ns=600, seed=9, draw="normal"), seed=9)
    n, nf = 600, 130
    cgb = _scan_engine(P, c, n)
    ll, sc = cgb.loglik_and_optimum_scan_sites_lg(c.spt, information=True)
    assert _layout(cgb) == 2 and not sc["info"].any()
    full = _raw(cgb, 0, n)
    assert _same(full, _raw(cgb, 0, n))
    assert full[0].tobytes() == np.ascontiguousarray(sc["delta"].T).tobytes() and full[3].tobytes() == sc["top_lr"].tobytes()
    parts = [_raw(cgb, a, b) for a, b in ((0, 37), (37, 130), (130, n))]
    assert _same(full, [np.concatenate(q, axis=-1) for q in zip(*parts)])
    tops = _raw(cgb, 0, n, tables=False)
    assert _same(full[3:], tops[3:]) and all(np.all(x == 7.0) for x in tops[:3])
    timed = _raw(cgb, 0, n, timed=True)
    assert _same(full, timed[:6]) and timed[7][0] == int(OS.heights(c.fam).max()) + 1 and np.all(timed[6] >= 0)
    cgb._lib.pgbp_sites_sweep_scratch_limit(270000)   # 256 sites take 256 (130 (4 + 3 + 1) + 2 * 3 + 3) = 268 544 doubles
    try:
        cut = _raw(cgb, 0, n)
        cut_timed = _raw(cgb, 0, n, timed=True)
    finally:
        cgb._lib.pgbp_sites_sweep_scratch_limit(0)
    assert _same(full, cut) and cut_timed[7][0] == 3 * (int(OS.heights(c.fam).max()) + 1)
    assert _layout(cgb) == 2
    cgb.pull()   # (the transfer moves the pool to the plain layout, an exact copy)
    after = cgb._packed_raw.copy()
    assert _layout(cgb) == 0
    assert _same(full, _raw(cgb, 0, n)) and _layout(cgb) == 0
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)
    # a calibration that no scan follows leaves the same pool
    o = cgb._opts()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    assert _layout(cgb) == 2
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)


def test_one_bad_lane(P):
    """a site with a negative rate reports info and NaN (top_family -1); its 63 neighbours keep the bytes they have without it"""
    c = OS.case("fixed")
    cgb = _scan_engine(P, c, 64)
    ll, good = cgb.loglik_and_optimum_scan_sites_lg(c.spt, information=True)
    kw = dict(cgb._fam_uni_kw)
    kw["R"] = kw["R"].copy()
    kw["R"][37] = -1.0
    cgb.assignfactors_lg_(**kw)
    ll2, got = cgb.loglik_and_optimum_scan_sites_lg(c.spt, information=True)
    keep = np.arange(64) != 37
    assert got["info"][37] != 0 and not got["info"][keep].any() and np.isnan(ll2[37])
    assert got["top_family"][37] == -1 and np.isnan(got["top_lr"][37])
    for k in ("delta", "lr", "information", "se", "top_lr", "top_family"):
        if k != "top_family":
            assert np.isnan(got[k][37]).all(), k
        assert got[k][keep].tobytes() == good[k][keep].tobytes(), k
    raw = _raw(cgb, 0, 64)   # the C call itself: that site NaN everywhere
    assert raw[5][37] != 0 and all(np.isnan(x[:, 37]).all() for x in raw[:3]) and np.isnan(raw[3][37]) and raw[4][37] == -1


# ----------------------------------------------------------------------------- 4: refusals

def _refused(cgb, code, *words, a=0, b=None, null=None, min_info=1e-8):
    """the call returns `code` with the words in the message; outputs, layout, pool and the optima in force untouched"""
    from pgbp_amd import _lib as L
    b = cgb.n_sites if b is None else b
    big = 1 << 16
    cgb.pull()
    before = cgb._packed_raw.copy()
    lay, n_opt = _layout(cgb), int(cgb._lib.pgbp_lg_optima_count(cgb._eng))
    f64 = [np.full(big, 7.0) for _ in range(5)]
    i32 = [np.full(big, 7, np.int32) for _ in range(3)]
    d = [None if null == "all" else L.f64p(x) for x in f64[:4]]
    tf = None if null == "all" else L.i32p(i32[0])
    rc = cgb._lib.pgbp_lg_optimum_scan_sites(cgb._eng, a, b, min_info, d[0], d[1], d[2], d[3], tf, L.i32p(i32[1]))
    msg = cgb._lib.pgbp_last_error(cgb._eng)
    assert rc == code and all(w.encode() in msg for w in words), (rc, msg)
    rc = cgb._lib.pgbp_lg_optimum_scan_sites_timed(cgb._eng, a, b, min_info, d[0], d[1], d[2], d[3], tf, L.i32p(i32[1]), L.f64p(f64[4]),
                                                   L.i32p(i32[2]))
    assert rc == code, (rc, cgb._lib.pgbp_last_error(cgb._eng))
    assert all(np.all(x == 7.0) for x in f64) and all(np.all(x == 7) for x in i32) and _layout(cgb) == lay
    assert int(cgb._lib.pgbp_lg_optima_count(cgb._eng)) == n_opt
    cgb.pull()
    assert np.array_equal(before, cgb._packed_raw)
    return msg.decode()


def test_refusals_leave_everything_untouched(P):
    from pgbp_amd import _lib as L
    from pgbp_amd import synth
    from test_gpu_gradient import _tree_batch
    from test_gpu_gradient_sites import _oracle_batch
    from oracle import models as OM
    from oracle import network as ON
    import uni_net_ref as N
    # what pgbp_lg_gradient_sites refuses
    engine, spt, *_ = _tree_batch(P, 8, 2, 50, True)
    _refused(engine(np.arange(8)), L.ERR_INVALID, "2 traits")
    rng = np.random.default_rng(34)
    net = ON.random_network(10, 2, rng)
    taxa = list(net.tip_names)
    models = [OM.UnivariateOrnsteinUhlenbeck(1.0, 0.7, 0.3, 0.0, 1.0)] * 8
    tbls = [[[float(x) for x in rng.normal(size=len(taxa))]] for _ in range(8)]
    cgb3, _, _ = _oracle_batch(P, net, taxa, models, tbls)
    assert int(np.max(cgb3._dims)) >= 3
    _refused(cgb3, L.ERR_INVALID, "variables")
    c = OS.case("optima")
    _refused(_engine(P, OS.base_of(c), 7), L.ERR_INVALID, "7 sites")
    cgb = _scan_engine(P, c, 65)            # two regimes in force: every refusal below leaves them in force
    cgb.loglik_and_optimum_scan_sites_lg(c.spt, tables=False)
    assert cgb.optima_count_lg() == 2
    _refused(cgb, L.ERR_INVALID, "site range", a=0, b=66)
    _refused(cgb, L.ERR_INVALID, "site range", a=-1, b=4)
    _refused(cgb, L.ERR_INVALID, "site range", a=5, b=4)
    _refused(cgb, L.ERR_INVALID, "no output buffer", null="all")
    _refused(cgb, L.ERR_INVALID, "min_info", min_info=1.0)
    _refused(cgb, L.ERR_INVALID, "min_info", min_info=-1e-3)
    _refused(cgb, L.ERR_INVALID, "min_info", min_info=float("nan"))
    # one workgroup of 256 sites does not fit the scratch: the text names the number of doubles that suffices
    nf = len(c.fam["cluster"])
    cgb._lib.pgbp_sites_sweep_scratch_limit(1000)
    try:
        msg = _refused(cgb, L.ERR_INVALID, "pgbp_sites_sweep_scratch_limit", "suffices")
        need = int(msg.split("pgbp_sites_sweep_scratch_limit: ")[1].split(" ")[0])
        assert 256 * nf * 8 <= need <= 256 * (nf * 8 + 16)
        cgb._lib.pgbp_sites_sweep_scratch_limit(need - 1)
        _refused(cgb, L.ERR_INVALID, "suffices")
        cgb._lib.pgbp_sites_sweep_scratch_limit(need)
        assert not cgb.optimum_scan_sites_lg(information=True)["info"].any()
    finally:
        cgb._lib.pgbp_sites_sweep_scratch_limit(0)
    # a Brownian-motion fill: wc = 0, the text names the jump scan
    kw = {k: v for k, v in cgb._fam_uni_kw.items() if k not in ("model", "alpha", "theta")}
    cgb.assignfactors_lg_(**kw)
    _refused(cgb, L.ERR_INVALID, "pgbp_lg_shift_scan_sites")
    # no topology; no parameters; no family table
    b = OS.base_of(c)
    dims, sepcl, so, si = N.engine_arrays(P, b.ocgb0)
    fresh = P.ClusterGraphBelief.from_arrays(dims, sepcl, so, si, None, n_sites=8)
    _refused(fresh, L.ERR_STATE, "pgbp_lg_setup")
    data = np.array([[[float(v)] for v in tbl[0]] for _, tbl in b.sites[:8]])
    fresh.lg_setup({k: v for k, v in b.fam.items() if k != "parent_family"}, data)
    _refused(fresh, L.ERR_STATE, "pgbp_lg_assignfactors")
    fresh.assignfactors_lg_(**{k: (v[:8] if isinstance(v, np.ndarray) and v.shape[:1] == (65,) else v) for k, v in cgb._fam_uni_kw.items()})
    _refused(fresh, L.ERR_STATE, "pgbp_lg_set_topology")
    # a family with two parents: the hybrid-tip networks, the family named
    for name in ("N1", "N2", "N3", "N4"):
        a = N.device_batch(P, name, "fixed", "ou", "cliquetree", 65)
        first = int(np.flatnonzero(np.asarray(a.fam["n_parents"]) >= 2)[0])
        _refused(a.pcgb, L.ERR_INVALID, f"family {first} has 2 parents")


# ----------------------------------------------------------------------------- 5: the bootstrap

def test_bootstrap_of_the_largest_lr(P):
    """bootstrap_optimum_scan_lg on 64 replicates with a fixed seed: max_lr against the restatement on the simulated data, and
    the same bytes as the steps done by hand on a second engine (simulate, fill, calibrate, scan with its tables)"""
    c = OS.case("fixed")
    B = 64
    cgb = _scan_engine(P, c, B)
    out = P.bootstrap_optimum_scan_lg(cgb, c.spt, seed=20262)
    assert sorted(out) == ["data", "data_before", "family", "info", "loglik", "max_lr", "x"] and not out["info"].any()
    assert _layout(cgb) == 2
    twin = _scan_engine(P, c, B)
    x, info = twin.simulate_lg(seed=20262, write_data=True, all_sites=True)
    ll, sc = twin.loglik_and_optimum_scan_sites_lg(c.spt)
    real = np.asarray(c.fam["n_parents"]) >= 1
    lr = np.where(real[None, :] & ~np.isnan(sc["delta"]) & np.isfinite(sc["lr"]), sc["lr"], -np.inf)
    assert out["x"].tobytes() == x.tobytes() and out["data"].tobytes() == twin.get_data_lg().tobytes()
    assert out["max_lr"].tobytes() == lr.max(axis=1).tobytes() and np.array_equal(out["family"], np.argmax(lr, axis=1))
    assert out["loglik"].tobytes() == ll.tobytes() and len(set(out["family"].tolist())) > 1
    sim = types.SimpleNamespace(**c.__dict__)
    sim.sites = [(m, [[float(v) for v in out["data"][s, :, 0]]]) for s, (m, _) in enumerate(c.sites[:B])]
    worst = max(abs(out["max_lr"][s] - OS.reference_site(sim, s)["top_lr"]) / max(1.0, out["max_lr"][s]) for s in range(B))
    print(f"bootstrap, 64 replicates: max_lr against the restatement {worst:.2e}; 95 % quantile {np.quantile(out['max_lr'], 0.95):.3f}")
    assert worst <= TOL
    # with optima in force the simulation refuses, and so does the bootstrap
    from pgbp_amd import _lib as L
    cgb.set_optima_lg(np.ones((len(c.fam["cluster"]), 1), np.int32), np.array([[0.5]]))
    cgb.assignfactors_lg_(**cgb._fam_uni_kw)
    with pytest.raises(L.PgbpError):
        P.bootstrap_optimum_scan_lg(cgb, c.spt, seed=1)

"""pgbp_lg_shift_scan_sites, pgbp_lg_edge_gradient_sites, pgbp_lg_loo_sites (csrc/pgbp_fam_uni.hip) and their wrappers
shift_scan_sites_lg, edge_gradient_sites_lg, loo_sites_lg and bootstrap_shift_scan_lg(sites=True): the lanes-are-sites family
sweeps of univariate batches.

Comparators, never the new kernels themselves: the general sweeps on the SAME beliefs (shift_scan_lg, edge_gradient_lg, loo_lg
with all_sites=True, called AFTER the new call so that their layout conversion cannot help it) and, for one site in eight, the
dense statements of tests/fam_uni_ref.py (pinned in test_fam_uni_cpu.py, which also checks the margins of identification, of
the leave-one-out floor and of the largest lr that these tests rely on).  Every comparison is asserted at 1e-8 relative to
max(1, |block|_inf); each test prints its worst figure."""
import ctypes as C

import numpy as np
import pytest

import fam_uni_ref as FR
from test_gradient_cpu import model_params

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _layout(cgb):
    return int(cgb._lib.pgbp_layout(cgb._eng))


def _engine(P, case, n):
    """An engine of the first n sites of a case on the oracle's clique tree, per-site parameters, shifts and noise in force,
    factors assigned"""
    import uni_net_ref as N
    dims, sepcl, so, si = N.engine_arrays(P, case.ocgb0)
    data = np.array([[[np.nan if v is None else float(v)] for v in tbl[0]] for _, tbl in case.sites[:n]])
    par = [model_params(m) for m, _ in case.sites[:n]]
    kw = dict(R=np.stack([np.stack([np.atleast_2d(r) for r in q[0]]) for q in par]), mu=np.stack([np.atleast_1d(q[2]) for q in par]))
    if par[0][3] is not None:
        kw.update(model="ou", alpha=np.array([float(q[3]) for q in par]), theta=np.stack([np.atleast_1d(q[4]) for q in par]))
    cgb = P.ClusterGraphBelief.from_arrays(dims, sepcl, so, si, None, n_sites=n)
    cgb.lg_setup(case.fam, data)
    if case.shifts is not None:
        cgb.set_shifts_lg(case.shifts[0], case.shifts[1][:n, :, None])
    if case.noise is not None:
        fams, E = case.noise
        cgb.set_tip_noise_lg(np.array(fams, np.int32), np.zeros((n, 1, 1)), np.ones(len(fams)), E[:n, :, None])
    cgb.assignfactors_lg_(**kw)
    cgb._fam_uni_kw = kw
    return cgb


def _rel(got, want):
    return FR.rel(got, want)


def _three(cgb, spt, min_info=1e-8):
    """the three new sweeps on one calibration (the layout is the calibration's before and after each), then the three
    general sweeps on the same beliefs"""
    ll, sc = cgb.loglik_and_shift_scan_sites_lg(spt, min_info=min_info, information=True)
    lay = _layout(cgb)
    eg = cgb.edge_gradient_sites_lg()
    assert _layout(cgb) == lay
    lo = cgb.loo_sites_lg()
    assert _layout(cgb) == lay and bool(lay & 2) == (cgb.n_sites >= 64)
    ref = dict(scan=cgb.shift_scan_lg(all_sites=True, min_info=min_info, information=True),
               edge=cgb.edge_gradient_lg(all_sites=True), loo=cgb.loo_lg(all_sites=True))
    return ll, dict(scan=sc, edge=eg, loo=lo), ref


def _against_general(tag, got, ref):
    """every site and block of the three sweeps against the general sweeps: NaN patterns, flags and info equal, values at
    TOL"""
    assert np.array_equal(got["scan"]["info"], ref["scan"]["info"]) and np.array_equal(got["edge"]["info"], ref["edge"]["info"])
    assert np.array_equal(got["loo"]["info"], ref["loo"]["info"]) and np.array_equal(got["loo"]["families"], ref["loo"]["families"])
    assert np.array_equal(got["scan"]["identified"], ref["scan"]["identified"]) and np.array_equal(got["scan"]["dof"], ref["scan"]["dof"])
    worst = 0.0
    blocks = [("scan", k) for k in ("jump", "lr", "edge_jump", "H", "se")] + [("edge", k) for k in ("dlength", "dgamma", "dshift")] + \
             [("loo", k) for k in ("mean", "cov", "lpd", "y")]
    for grp, k in blocks:
        a, b = got[grp][k], ref[grp][k]
        assert a.shape == b.shape, (grp, k, a.shape, b.shape)
        for s in range(a.shape[0]):
            worst = max(worst, _rel(a[s], b[s]))
    worst = max(worst, _rel(got["loo"]["total"], ref["loo"]["total"]))
    print(f"{tag}: worst block against the general sweeps {worst:.2e}")
    assert worst <= TOL, tag
    return worst


def _own_top(tag, sc, fam):
    """top_lr is the maximum of the call's own lr table over the eligible families, to the byte, top_family its first argmax"""
    real = np.asarray(fam["n_parents"]) >= 1
    lr = np.where(real[None, :] & sc["identified"][:, :, 0] & np.isfinite(sc["lr"]), sc["lr"], -np.inf)
    f = np.argmax(lr, axis=1)
    top = lr[np.arange(lr.shape[0]), f]
    assert np.array_equal(sc["top_lr"], top), tag
    assert np.array_equal(sc["top_family"], np.where(np.isfinite(top), f, -1)), tag


def _as_site(got, s):
    """site s of the device dicts in fam_uni_ref.sweeps' layout"""
    return dict(scan=dict(jump=got["scan"]["jump"][s, :, 0], lr=got["scan"]["lr"][s], identified=got["scan"]["identified"][s, :, 0]),
                edge=dict(dlength=got["edge"]["dlength"][s], dgamma=got["edge"]["dgamma"][s], dshift=got["edge"]["dshift"][s, :, 0]),
                loo=dict(mean=got["loo"]["mean"][s, :, 0], var=got["loo"]["cov"][s, :, 0, 0], lpd=got["loo"]["lpd"][s],
                         info=got["loo"]["info"][s]))


def _against_dense(tag, case, got, n):
    worst = {}
    rows = case.fam["data_row"][got["loo"]["families"]]
    for s in FR.checked_sites(n):
        w = FR.against_dense(_as_site(got, s), FR.dense_site(case, s), case.fam, rows)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"{tag}: one site in eight against the dense statements: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL, (tag, worst)


# ----------------------------------------------------------------------------- 1: every plain case at its site counts

PLAIN = [(c, n) for c, counts in FR.plain_cases() for n in counts]


@pytest.mark.parametrize("i", range(len(PLAIN)), ids=[f"{c.name}-{n}" for c, n in PLAIN])
def test_sweeps_against_the_general_calls_and_the_dense_statements(P, i):
    """BM at 8 (plain pool), 64 (site-minor), 65 (a ragged wavefront) and 257 sites (a second workgroup with one lane); OU
    with a fixed, random and improper root; missing tips and skipped families; the hybrid-tip networks N1 .. N4 under BM and
    OU (two-parent families, 2- and 0-variable clusters, a fixed-root parent, dgamma on both parent edges); per-site shifts
    and tip noise (the scan is then the increment, dgamma carries s_k g_w, the leave-one-out predicts the observation)."""
    case, n = PLAIN[i]
    cgb = _engine(P, case, n)
    ll, got, ref = _three(cgb, case.spt)
    tag = f"{case.name}/{n}"
    assert not got["scan"]["info"].any()
    nf, K = len(case.fam["cluster"]), max(1, int(case.fam["max_parents"]))
    assert got["scan"]["jump"].shape == (n, nf, 1) and got["edge"]["dgamma"].shape == (n, nf, K)
    _against_general(tag, got, ref)
    _own_top(tag, got["scan"], case.fam)
    _against_dense(tag, case, got, n)
    if case.identification:
        # a clade without data: not identified, lr 0, jump NaN, and never the top family
        cm, npar = np.asarray(case.fam["child_mask"]), np.asarray(case.fam["n_parents"])
        dead = np.flatnonzero((cm == 0) & (npar >= 1) & (np.asarray(case.fam["data_row"]) < 0))
        assert len(dead) >= 1
        assert not got["scan"]["identified"][:, dead].any() and np.all(got["scan"]["lr"][:, dead] == 0.0)
        assert np.isnan(got["scan"]["jump"][:, dead]).all() and not np.isin(got["scan"]["top_family"], dead).any()
    if case.top:
        lr = np.where((ref["scan"]["dof"] > 0) & np.isfinite(ref["scan"]["lr"]) & (np.asarray(case.fam["n_parents"]) >= 1)[None, :],
                      ref["scan"]["lr"], -np.inf)
        assert np.array_equal(got["scan"]["top_family"], np.argmax(lr, axis=1))
    # tables=False: the two summaries alone, the same bytes
    only = cgb.shift_scan_sites_lg(tables=False)
    assert sorted(only) == ["info", "top_family", "top_lr"]
    ll2, again = cgb.loglik_and_shift_scan_sites_lg(case.spt, tables=False)
    assert np.array_equal(again["top_lr"], got["scan"]["top_lr"]) and np.array_equal(again["top_family"], got["scan"]["top_family"])
    assert np.array_equal(ll, ll2)


# ----------------------------------------------------------------------------- 2: family-block boundaries

@pytest.mark.parametrize("n_fam,planted", FR.BLOCKS)
def test_family_block_boundaries(P, n_fam, planted):
    """A thread walks blocks of 64 families: 63, 64, 65, 130 and 398 families, the largest lr planted in the last family of
    block 0 and in the first family of block 1."""
    case = FR.block_case(n_fam, planted)
    ns = len(case.sites)   # (64; 16 for the 398 families)
    cgb = _engine(P, case, ns)
    ll, got, ref = _three(cgb, case.spt)
    tag = case.name
    _against_general(tag, got, ref)
    _own_top(tag, got["scan"], case.fam)
    assert np.all(got["scan"]["top_family"] == planted), got["scan"]["top_family"]
    lr = np.where((ref["scan"]["dof"] > 0) & np.isfinite(ref["scan"]["lr"]), ref["scan"]["lr"], -np.inf)
    assert np.array_equal(got["scan"]["top_family"], np.argmax(lr, axis=1))
    own = np.array([FR.block_total(row) for row in got["loo"]["lpd"]])
    err = float(np.max(np.abs(got["loo"]["total"] - own) / np.abs(own)))
    print(f"{tag}: total against the sum of its own lpd {err:.2e}")
    assert err <= 1e-12
    _against_dense(tag, case, got, ns)


# ----------------------------------------------------------------------------- 3: determinism, read-only

def _raw(cgb, a, b, what):
    """the C calls on [a, b): every output as one list of arrays (sentinel-filled first)"""
    from pgbp_amd import _lib as L
    n = b - a
    nf = len(cgb._lg["cluster"])
    K = cgb._lg["length"].size // nf
    nt = int(cgb._lib.pgbp_lg_loo_count(cgb._eng))
    f64 = lambda *shape: np.full(shape, 7.0)
    i32 = lambda *shape: np.full(shape, 7, np.int32)
    if what == "scan":
        out = [f64(nf, n), f64(nf, n), f64(nf, n), f64(n), i32(n), i32(n)]
        rc = cgb._lib.pgbp_lg_shift_scan_sites(cgb._eng, a, b, 1e-8, L.f64p(out[0]), L.f64p(out[1]), L.f64p(out[2]), L.f64p(out[3]),
                                               L.i32p(out[4]), L.i32p(out[5]))
    elif what == "edge":
        out = [f64(nf, K, n), f64(nf, K, n), f64(nf, n), i32(n)]
        rc = cgb._lib.pgbp_lg_edge_gradient_sites(cgb._eng, a, b, L.f64p(out[0]), L.f64p(out[1]), L.f64p(out[2]), L.i32p(out[3]))
    else:
        out = [f64(nt, n), f64(nt, n), f64(nt, n), f64(n), i32(nt, n)]
        rc = cgb._lib.pgbp_lg_loo_sites(cgb._eng, a, b, L.f64p(out[0]), L.f64p(out[1]), L.f64p(out[2]), L.f64p(out[3]), L.i32p(out[4]))
    assert rc == L.PGBP_OK, cgb._lib.pgbp_last_error(cgb._eng)
    return out


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_determinism_ranges_and_chunks(P):
    """600 sites: two calls, [0, n) against two half ranges, and one workgroup of sites per chunk (the scratch limit lowered)
    return the same bytes; the layout stays site-minor throughout"""
    case = FR.bm_case()
    n = 600
    cgb = _engine(P, case, n)
    cgb.loglik_and_shift_scan_sites_lg(case.spt, tables=False)
    assert _layout(cgb) == 2
    for what in ("scan", "edge", "loo"):
        full = _raw(cgb, 0, n, what)
        assert _same(full, _raw(cgb, 0, n, what)), what
        lo, hi = _raw(cgb, 0, 300, what), _raw(cgb, 300, n, what)
        assert _same(full, [np.concatenate([x, y], axis=-1) for x, y in zip(lo, hi)]), what
        odd = _raw(cgb, 77, 401, what)
        assert _same([x[..., 77:401] for x in full], odd), what
        cgb._lib.pgbp_sites_sweep_scratch_limit(1)   # (one workgroup's sites at least: chunks of 256)
        try:
            assert _same(full, _raw(cgb, 0, n, what)), what
        finally:
            cgb._lib.pgbp_sites_sweep_scratch_limit(0)
        assert _layout(cgb) == 2


def test_read_only_and_both_layouts(P):
    """64 sites: the pool's bytes and pgbp_layout are unchanged by each call; a calibrate_ after the calls gives the bytes of
    one without them; the site-minor and the plain instance of the same beliefs give the same bytes"""
    case = FR.bm_case()
    cgb = _engine(P, case, 64)
    cgb.loglik_and_shift_scan_sites_lg(case.spt, tables=False)
    assert _layout(cgb) == 2
    sm = {w: _raw(cgb, 0, 64, w) for w in ("scan", "edge", "loo")}
    assert _layout(cgb) == 2
    cgb.pull()   # (the transfer moves the pool to the plain layout, an exact copy)
    after = cgb._packed_raw.copy()
    assert _layout(cgb) == 0
    for w in ("scan", "edge", "loo"):
        assert _same(sm[w], _raw(cgb, 0, 64, w)), w
        assert _layout(cgb) == 0
        cgb.pull()
        assert np.array_equal(after, cgb._packed_raw), w
    # a calibration that no sweep follows leaves the same pool
    o = cgb._opts()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    assert _layout(cgb) == 2
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)


# ----------------------------------------------------------------------------- 4: one bad lane

def test_one_bad_lane(P):
    """a site with a negative rate reports info and NaN (top_family -1); its 63 neighbours keep the bytes they have without it"""
    case = FR.bm_case()
    cgb = _engine(P, case, 64)
    ll, good, _ = _three(cgb, case.spt)
    kw = dict(cgb._fam_uni_kw)
    kw["R"] = kw["R"].copy()
    kw["R"][37] = -1.0
    cgb.assignfactors_lg_(**kw)
    ll2, got, ref = _three(cgb, case.spt)
    keep = np.arange(64) != 37
    for grp in ("scan", "edge"):
        assert got[grp]["info"][37] != 0 and not got[grp]["info"][keep].any()
        assert np.array_equal(got[grp]["info"], ref[grp]["info"])
    assert np.isnan(ll2[37]) and got["scan"]["top_family"][37] == -1 and np.isnan(got["scan"]["top_lr"][37])
    for grp, keys in (("scan", ("jump", "lr", "H", "top_lr", "top_family")), ("edge", ("dlength", "dgamma", "dshift")),
                      ("loo", ("mean", "cov", "lpd", "total", "info"))):
        for k in keys:
            if grp != "loo" and k != "top_family":
                assert np.isnan(got[grp][k][37]).all(), (grp, k)
            assert got[grp][k][keep].tobytes() == good[grp][k][keep].tobytes(), (grp, k)
    assert got["loo"]["info"][37].all() and np.isnan(got["loo"]["lpd"][37]).all() and np.isnan(got["loo"]["total"][37])
    assert np.array_equal(got["loo"]["info"], ref["loo"]["info"])


def test_a_tip_the_other_data_do_not_determine(P):
    """improper root, 8 sites: at one site one tip is not determined -- info 1 and NaN, that site's total NaN -- other tips and
    sites are unaffected (against loo_lg, and the dense leave-one-out at site 0 and at that site)"""
    case = FR.undetermined_case()
    site, tip = case.undetermined
    cgb = _engine(P, case, 8)
    ll, got, ref = _three(cgb, case.spt)
    want = np.zeros((8, len(got["loo"]["families"])), np.int32)
    want[site, tip] = 1
    assert np.array_equal(got["loo"]["info"], want)
    assert np.isnan(got["loo"]["lpd"][site, tip]) and np.isnan(got["loo"]["mean"][site, tip]).all() and np.isnan(got["loo"]["cov"][site, tip]).all()
    assert np.array_equal(np.isnan(got["loo"]["total"]), np.arange(8) == site)
    _against_general("undetermined", got, ref)
    rows = case.fam["data_row"][got["loo"]["families"]]
    w0 = FR.against_dense(_as_site(got, 0), FR.dense_site(case, 0), case.fam, rows)
    dn = FR.dense_site(case, site)
    worst = 0.0
    for ti, r in enumerate(rows):
        if ti != tip:
            _, mean, cov, lpd = dn["loo"][int(r)]
            worst = max(worst, _rel(got["loo"]["mean"][site, ti, 0], mean[0]), _rel(got["loo"]["lpd"][site, ti], lpd),
                        abs(got["loo"]["cov"][site, ti, 0, 0] - cov[0, 0]) / cov[0, 0])
    print(f"undetermined: site 0 against the dense statements {max(w0.values()):.2e}, the other tips of site {site} {worst:.2e}")
    assert max(w0.values()) <= TOL and worst <= TOL


# ----------------------------------------------------------------------------- 5: refusals

def _refused(cgb, code, word, a=0, b=None, what=("scan", "edge", "loo"), null=None, min_info=1e-8):
    """each of the calls returns `code` with `word` in the message, the outputs, the layout and the pool untouched"""
    from pgbp_amd import _lib as L
    n = cgb.n_sites
    b = n if b is None else b
    big = 1 << 16
    cgb.pull()
    before = cgb._packed_raw.copy()
    lay = _layout(cgb)
    for w in what:
        f64 = [np.full(big, 7.0) for _ in range(4)]
        i32 = [np.full(big, 7, np.int32) for _ in range(2)]
        d = [None if null in ("all", k) else L.f64p(x) for k, x in zip(range(4), f64)]
        if w == "scan":
            tf = None if null == "all" else L.i32p(i32[0])
            rc = cgb._lib.pgbp_lg_shift_scan_sites(cgb._eng, a, b, min_info, d[0], d[1], d[2], d[3], tf, L.i32p(i32[1]))
        elif w == "edge":
            rc = cgb._lib.pgbp_lg_edge_gradient_sites(cgb._eng, a, b, d[0], d[1], d[2], L.i32p(i32[1]))
        else:
            rc = cgb._lib.pgbp_lg_loo_sites(cgb._eng, a, b, d[0], d[1], d[2], d[3], L.i32p(i32[1]))
        msg = cgb._lib.pgbp_last_error(cgb._eng)
        assert rc == code and word.encode() in msg, (w, rc, msg)
        assert all(np.all(x == 7.0) for x in f64) and all(np.all(x == 7) for x in i32) and _layout(cgb) == lay, w
    cgb.pull()
    assert np.array_equal(before, cgb._packed_raw)


def test_refusals(P):
    from pgbp_amd import _lib as L
    from pgbp_amd import synth
    from test_gpu_gradient import _tree_batch
    from test_gpu_gradient_sites import _oracle_batch
    from oracle import models as OM
    from oracle import network as ON
    engine, spt, *_ = _tree_batch(P, 8, 2, 50, True)
    _refused(engine(np.arange(8)), L.ERR_INVALID, "2 traits")
    # p = 1 on a network whose clique tree has a cluster of 3 nodes
    rng = np.random.default_rng(34)
    net = ON.random_network(10, 2, rng)
    taxa = list(net.tip_names)
    models = [OM.UnivariateBrownianMotion(1.0, 0.0, 1.0)] * 8
    tbls = [[[float(x) for x in rng.normal(size=len(taxa))]] for _ in range(8)]
    cgb3, _, _ = _oracle_batch(P, net, taxa, models, tbls)
    assert int(np.max(cgb3._dims)) >= 3
    _refused(cgb3, L.ERR_INVALID, "variables")
    case = FR.bm_case()
    _refused(_engine(P, case, 7), L.ERR_INVALID, "7 sites")
    cgb8 = _engine(P, case, 8)
    _refused(cgb8, L.ERR_INVALID, "site range", 0, 9)
    _refused(cgb8, L.ERR_INVALID, "site range", -1, 4)
    _refused(cgb8, L.ERR_INVALID, "site range", 5, 4)
    _refused(cgb8, L.ERR_INVALID, "no output buffer", null="all", what=("scan", "edge"))
    _refused(cgb8, L.ERR_INVALID, "lpd", null=2, what=("loo",))
    _refused(cgb8, L.ERR_INVALID, "min_info", what=("scan",), min_info=1.0)
    _refused(cgb8, L.ERR_INVALID, "min_info", what=("scan",), min_info=-1e-3)
    # the reason names the general call
    for w, name in (("scan", "pgbp_lg_shift_scan"), ("edge", "pgbp_lg_edge_gradient"), ("loo", "pgbp_lg_loo")):
        _refused(_engine(P, case, 7), L.ERR_INVALID, f"(use {name})", what=(w,))
    # no family table; a table but no parameters
    tree = synth.random_tree(6, rng)
    prob = synth.cliquetree_of_tree(tree, 1)
    fresh = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=8)
    _refused(fresh, L.ERR_STATE, "pgbp_lg_setup")
    fresh.lg_setup(synth.lg_tree_table(tree, prob, 1), np.zeros((8, tree.nnodes, 1)))
    _refused(fresh, L.ERR_STATE, "pgbp_lg_assignfactors")


# ----------------------------------------------------------------------------- 6: the bootstrap

def test_bootstrap_with_the_sites_scan(P):
    """bootstrap_shift_scan_lg(sites=True) against sites=False on a 32-tip tree with 64 replicates and a fixed seed: max_lr to
    1e-8, family and edge equal, x and data the same bytes; the scan it runs fetches no table"""
    from pgbp_amd import synth
    from test_gpu_gradient_sites import _synth_engine
    rng = np.random.default_rng(415)
    tree = synth.random_tree(32, rng)
    B = 64
    X = np.repeat(synth.simulate_bm_uni_sites(tree, np.array([1.3]), np.array([0.2]), rng), B, axis=0)
    out = {}
    for sites in (True, False):
        cgb, spt, fam = _synth_engine(P, tree, X)
        cgb.assignfactors_lg_(np.array([[[1.3]]]), np.array([0.2]))
        out[sites] = P.bootstrap_shift_scan_lg(cgb, spt, seed=20261, sites=sites)
        if sites:
            assert _layout(cgb) == 2
            ll, scan = cgb.loglik_and_shift_scan_sites_lg(spt, tables=False)
            assert sorted(scan) == ["info", "top_family", "top_lr"]
    a, b = out[True], out[False]
    assert sorted(a) == sorted(b) and not a["info"].any() and not b["info"].any()
    err = float(np.max(np.abs(a["max_lr"] - b["max_lr"]) / np.maximum(1.0, np.abs(b["max_lr"]))))
    print(f"bootstrap, 64 replicates: max_lr of the sites scan against the general scan {err:.2e}; "
          f"{len(set(a['family'].tolist()))} distinct families")
    assert err <= TOL
    assert np.array_equal(a["family"], b["family"]) and np.array_equal(a["edge"], b["edge"]) and len(set(a["family"].tolist())) > 1
    assert a["x"].tobytes() == b["x"].tobytes() and a["data"].tobytes() == b["data"].tobytes()
    assert np.max(np.abs(a["loglik"] - b["loglik"]) / np.maximum(1.0, np.abs(b["loglik"]))) <= TOL

"""The model run forwards on the device: pgbp_lg_set_topology, pgbp_lg_set_data / pgbp_lg_get_data, pgbp_lg_simulate
(csrc/pgbp_simulate.hip) and the driver bootstrap_shift_scan_lg.

Comparators (tests/simulate_ref.py, pinned in test_simulate_cpu.py), neither the code under test: densely,
oracle.densemvn.node_moments of the (wrapped) model -- the sweep is linear in z, x = m + A z, so z = 0 must give the dense
mean and the unit vectors A with A A' = the dense covariance --; family by family, simulate_ref.simulate for random z; and
the numpy restatement of the generator.  Every comparison at 1e-8 relative to the largest entry of the block (the generator:
1e-12 absolute); the measured figure of every case is printed."""
import numpy as np
import pytest

import loo_ref as LR
import scan_ref as SC
import simulate_ref as SR
import uni_net_ref as N
from helpers import lg_inputs_from_oracle
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from shift_ref import ShiftedModel, family_nodes
from test_gpu_shifts import MODELS, _bytes, _device, _tree_batch, _tree_case
from test_gpu_tip_noise import _batch

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _one_site(P, which, p, variant="plain", assign=True):
    """A one-site engine of a case of simulate_ref.DENSE_CASES on its clique tree under a variant (shifts / tip noise set)."""
    net, model, tbl, taxa = SR.oracle_case(which, p)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa, assign=assign, oracle_factors=False)
    w, shifts, noise, setter = SR.variant(net, ocgb, fam, kw, model, p, variant)
    if shifts is not None:
        pcgb.set_shifts_lg(*shifts)
    if setter is not None:
        pcgb.set_tip_noise_lg(*setter)
    return dict(net=net, model=model, tbl=tbl, taxa=taxa, ocgb=ocgb, pcgb=pcgb, fam=fam, kw=kw, spt=spt, wrapper=w, shifts=shifts,
                noise=noise)


def _rows(pcgb):
    """run() of simulate_ref.mean_and_map on a one-site engine: one call per row of z."""
    def run(Z):
        out = []
        for z in Z:
            x, info = pcgb.simulate_lg(z=z[None])
            assert info[0] == 0
            out.append(x[0])
        return np.stack(out)
    return run


def _tbl_of(data, fam, taxa, p):
    """The oracle's table (trait columns over taxa, None = missing) of one site's data rows [n_rows, p] under the table's masks."""
    tbl = [[None] * len(taxa) for _ in range(p)]
    for f, r, cm in SR.tip_rows(fam):
        for t in range(p):
            if cm is None or (cm >> t) & 1:
                tbl[t][r] = float(data[r, t])
    return tbl


# ----------------------------------------------------------------------------- 1, 2: mean and A A' against the dense moments

DENSE_GPU = [c for c in SR.DENSE_CASES if c not in (("tree", 16), ("tree", 40))]
assert all((w, p) in DENSE_GPU for w, p in MODELS if w != "bm_improper")


@pytest.mark.parametrize("variant", SR.VARIANTS)
@pytest.mark.parametrize("which,p", DENSE_GPU)
def test_mean_and_covariance_against_the_dense_moments(P, which, p, variant):
    """z = 0 gives the dense prior mean, the unit vectors give A with A A' = the dense covariance -- plain, under shifts
    (test_gpu_shifts._pick: a tip edge, an edge below the fixed root, both edges of a hybrid, ...) and under tip noise with se2
    (a noisy tip's row is its observation).  24-tip networks: heterogeneous BM (two-parent families with two colours, a
    root-prior family), the OU with a fixed and a random root, BM at p = 1 and p = 4; the hybrid-tip networks of uni_net_ref at
    p = 1 (N4: one parent of the hybrid tip is the fixed root) and N1 at p = 2; the missing-data networks (p = 3: the states
    keep all p traits whatever the masks); a 12-tip tree."""
    c = _one_site(P, which, p, variant)
    m, A = SR.mean_and_map(c["fam"], None, p, run=_rows(c["pcgb"]))
    em, ec = SR.moment_errors(m, A, c["net"], c["wrapper"], family_nodes(c["ocgb"], c["fam"]))
    print(f"{which}/p{p}/{variant}: {len(c['fam']['cluster'])} families, mean vs dense {em:.2e}, A A' vs dense {ec:.2e}")
    assert em <= TOL and ec <= TOL
    by_node = c["pcgb"].simulated_nodes(m.reshape(1, -1, p))
    nodes = family_nodes(c["ocgb"], c["fam"])
    assert sorted(by_node) == [i + 1 for i in nodes] and np.array_equal(by_node[nodes[-1] + 1], m.reshape(-1, p)[-1])


# ----------------------------------------------------------------------------- 3: entry by entry against simulate_ref

def _entries(tag, pcgb, fam, kw, p, per_site, shifts=None, noise=None, sites=None):
    """simulate_lg(z) of every site against simulate_ref.simulate; twice: equal bytes.  shifts: (edges, values [n, p] or
    [sites, n, p]).  Returns x."""
    n, nf = pcgb.n_sites, len(fam["cluster"])
    z = np.random.default_rng(101).normal(size=(n, nf, p))
    x, info = pcgb.simulate_lg(z=z, all_sites=True)
    x2, _, zo = pcgb.simulate_lg(z=z, all_sites=True, return_z=True)
    assert not info.any() and x.tobytes() == x2.tobytes() and np.array_equal(zo, z)
    worst = 0.0
    for s in (range(n) if sites is None else sites):
        sh = None if shifts is None else (shifts[0], shifts[1][s] if np.ndim(shifts[1]) == 3 else shifts[1])
        want = SR.simulate(fam, SR.site_kw(kw, s, p, per_site), z[s], p, sh, noise)
        worst = max(worst, SR.rel(x[s], want))
    print(f"{tag}: {n} sites x {nf} families x {p} traits against the family-by-family reference {worst:.2e}")
    assert worst <= TOL
    return x


@pytest.mark.parametrize("p", [2, 16, 40])
def test_entries_trees(P, p):
    """test_gpu_shifts._tree_case with its three shifts in force: p = 2 and p = 16 (four families per wavefront), p = 40 (a
    wavefront per family, the Cholesky's columns beyond one row of 16 lanes, 13 KB of LDS)."""
    tree, model, tbl, pcgb, spt, kw, edges, values, sh = _tree_case(P, p, 40 + p)
    pcgb.set_shifts_lg(edges, values)
    _entries(f"12-tip tree p={p}", pcgb, pcgb._lg, kw, p, False, (edges, values))


@pytest.mark.parametrize("root", ["random", "fixed"])
def test_entries_missing_data(P, root):
    """p = 3 with 30 % of the tip values missing: partial scope masks in the table, all three traits in every state."""
    c = _one_site(P, f"missing_{root}", 3)
    assert c["fam"].get("child_mask") is not None
    _entries(f"missing/{root}", c["pcgb"], c["fam"], c["kw"], 3, False)


@pytest.mark.parametrize("n_sites", [8, 64, 65])
def test_entries_univariate_batches(P, n_sites):
    """A 40-tip tree at p = 1, every site its own parameters: the states and normals in the [family][site] order (65 sites:
    the padded row tail), one parameter set per site.  And the hybrid-tip network N1 with per-site parameters."""
    nwk, taxa, data, Rs, mus = LR.batch_case(1, n_sites=n_sites)
    cgb, spt, fam = _tree_batch(P, 1, n_sites=n_sites)
    _entries(f"tree batch, {n_sites} sites", cgb, cgb._lg, dict(R=Rs[:, None], mu=mus), 1, True)
    for kind in ("bm", "ou"):
        b = N.device_batch(P, "N1", "fixed", kind, "cliquetree", n_sites)
        _entries(f"N1/{kind}, {n_sites} sites", b.pcgb, b.fam, b.kw, 1, True)


def test_entries_batch_per_site_parameters_and_shifts(P):
    """64 sites at p = 1 with their own parameters and their own shifts; then shared shifts on per-site parameters, and the
    p = 2 batch (plain order, per-site sets)."""
    nwk, taxa, data, Rs, mus = LR.batch_case(1)
    cgb, spt, fam = _tree_batch(P, 1)
    nf = len(fam["cluster"])
    edges = sorted({(0, 0), (nf // 3, 0), (nf - 1, 0)})
    values = np.random.default_rng(13).normal(size=(64, len(edges), 1))
    cgb.set_shifts_lg(edges, values)
    a = _entries("batch p=1, per-site shifts", cgb, cgb._lg, dict(R=Rs[:, None], mu=mus), 1, True, (edges, values))
    cgb.set_shifts_lg(edges, values[5])
    b = _entries("batch p=1, shared shifts", cgb, cgb._lg, dict(R=Rs[:, None], mu=mus), 1, True, (edges, values[5]))
    assert a.tobytes() != b.tobytes()
    nwk, taxa, data, Rs, mus = LR.batch_case(2)
    cgb, spt, fam = _tree_batch(P, 2)
    values = np.random.default_rng(14).normal(size=(64, len(edges), 2))
    cgb.set_shifts_lg(edges, values)
    _entries("batch p=2, per-site shifts", cgb, cgb._lg, dict(R=Rs[:, None], mu=mus), 2, True, (edges, values), sites=(0, 31, 63))


# ----------------------------------------------------------------------------- 4: write_data, set_data_lg, get_data_lg

def _check_written(pcgb, fam, x, before, sites=None):
    """get_data_lg equals x at the tips inside the masks; everything else keeps its bytes."""
    got = pcgb.get_data_lg()
    want = before.copy()
    p = x.shape[2]
    for f, r, cm in SR.tip_rows(fam):
        for t in range(p):
            if cm is None or (cm >> t) & 1:
                want[:, r, t] = x[:, f, t]
    if sites is not None:
        keep = np.ones(len(want), bool)
        keep[list(sites)] = False
        want[keep] = before[keep]
    assert got.tobytes() == want.tobytes()
    return got


def test_write_data_plain_layout_with_masks(P):
    """The missing-data network (p = 3, one site): the simulated tips land in the engine's data inside the masks, masked
    entries keep their bytes, loglik_lg of the new data equals densemvn.loglik of the simulated table.  set_data_lg of the same
    values on a second engine, and a fresh lg_setup with them, give the bytes of every belief after a fill."""
    c = _one_site(P, "missing_random", 3)
    pcgb, fam, p = c["pcgb"], c["fam"], 3
    pcgb._ensure_schedule([c["spt"]])
    before = pcgb.get_data_lg()
    raw = lg_inputs_from_oracle(P, c["net"], c["ocgb"], c["model"], c["tbl"], c["taxa"])[1]
    assert np.array_equal(before[0], np.where(np.isfinite(raw), raw, 0.0))
    x, info = pcgb.simulate_lg(seed=7, write_data=True)
    assert info[0] == 0 and any(cm is not None and cm != 7 for _, _, cm in SR.tip_rows(fam))
    data = _check_written(pcgb, fam, x, before)
    ll, linfo = pcgb.loglik_lg()
    dense = OD.loglik(c["net"], c["model"], _tbl_of(data[0], fam, c["taxa"], p), c["taxa"])
    old = OD.loglik(c["net"], c["model"], c["tbl"], c["taxa"])
    e = abs(ll[0] - dense) / max(1.0, abs(dense))
    print(f"write_data, plain layout with masks: loglik_lg vs dense on the simulated table {e:.2e} (the old table: {abs(ll[0] - old):.2e} away)")
    assert linfo[0] == 0 and e <= TOL and abs(ll[0] - old) > 1e-3
    pcgb.assignfactors_lg_(**c["kw"])
    filled = _bytes(pcgb)
    second = _one_site(P, "missing_random", 3)["pcgb"]
    assert _bytes(second) != filled
    with_nan = data.copy()
    for f, r, cm in SR.tip_rows(fam):
        with_nan[0, r, [t for t in range(p) if not (cm >> t) & 1]] = np.nan     # (outside the masks: ignored)
    second.set_data_lg(with_nan)
    assert np.array_equal(second.get_data_lg(), np.where(np.isfinite(with_nan), with_nan, 0.0))
    second.assignfactors_lg_(**c["kw"])
    assert _bytes(second) == filled
    fresh = _one_site(P, "missing_random", 3, assign=False)["pcgb"]
    fresh.lg_setup(fam, with_nan)
    fresh.assignfactors_lg_(**c["kw"])
    assert _bytes(fresh) == filled
    # a value that is not finite where the mask says observed is refused, the data stay
    f, r, cm = SR.tip_rows(fam)[0]
    bad = data.copy()
    bad[0, r, [t for t in range(p) if (cm >> t) & 1][0]] = np.nan
    with pytest.raises(P.PgbpError, match=f"family {f}"):
        second.set_data_lg(bad)
    assert second.get_data_lg().tobytes() == np.where(np.isfinite(with_nan), with_nan, 0.0).tobytes()


def test_write_data_packed_layout(P):
    """The p = 16 tree with every trait in scope, held in the packed (BS16) layout after a calibration, three shifts in
    force: write_data, then loglik_lg in that layout against the dense log-likelihood of the simulated table."""
    p = 16
    tree, model, tbl, pcgb, spt, kw, edges, values, sh = _tree_case(P, p, 40 + p)
    pcgb._ensure_schedule([spt])
    pcgb.set_shifts_lg(edges, values)
    pcgb.loglik_and_edge_gradient_lg(spt)
    assert pcgb._lib.pgbp_layout(pcgb._eng) == 1
    before = pcgb.get_data_lg()
    x, info = pcgb.simulate_lg(seed=11, write_data=True)
    data = _check_written(pcgb, pcgb._lg, x, before)
    ll, linfo = pcgb.loglik_lg()
    assert pcgb._lib.pgbp_layout(pcgb._eng) == 1
    dense = OD.loglik(tree, ShiftedModel(model, sh), _tbl_of(data[0], pcgb._lg, tree.tip_names, p), tree.tip_names)
    e = abs(ll[0] - dense) / abs(dense)
    print(f"write_data, packed layout (p = 16): loglik_lg vs dense on the simulated table {e:.2e}")
    assert info[0] == 0 and linfo[0] == 0 and e <= TOL


@pytest.mark.parametrize("n_sites", [64, 65])
def test_write_data_site_minor_layout(P, n_sites):
    """Univariate batches in the site-minor layout: the [row][site] copy of the data is written with the plain one.  Every
    site's loglik_lg against the dense log-likelihood of its simulated data; set_data_lg on a second engine gives the same
    log-likelihood bytes and the same belief bytes after a fill."""
    cgb, spt, fam, Rs, site = _batch(P, 1, n_sites)
    cgb._ensure_schedule([spt])
    before = cgb.get_data_lg()
    x, info = cgb.simulate_lg(seed=SR.SEED, write_data=True, all_sites=True)
    data = _check_written(cgb, fam, x, before)
    ll, linfo = cgb.loglik_lg()
    assert cgb._lib.pgbp_layout(cgb._eng) & 2, "a univariate batch of 64 sites is expected in the site-minor layout"
    worst = 0.0
    for s in range(n_sites):
        onet, model, _, taxa = site(s)
        dense = OD.loglik(onet, model, [list(data[s][:, 0])], taxa)
        worst = max(worst, abs(ll[s] - dense) / max(1.0, abs(dense)))
    print(f"write_data, site-minor layout, {n_sites} sites: loglik_lg vs dense on the simulated data, worst site {worst:.2e}")
    assert not info.any() and not linfo.any() and worst <= TOL
    other, spt2, _, _, _ = _batch(P, 1, n_sites)
    other._ensure_schedule([spt2])
    other.set_data_lg(data)
    ll2, _ = other.loglik_lg()
    assert ll2.tobytes() == ll.tobytes()
    cgb.assignfactors_lg_(Rs[:, None], site.mus)
    other.assignfactors_lg_(Rs[:, None], site.mus)
    assert _bytes(other) == _bytes(cgb)
    # one site only: the others keep their bytes
    cgb.site = 3
    x3, _ = cgb.simulate_lg(seed=99, write_data=True)
    _check_written(cgb, fam, np.repeat(x3, n_sites, axis=0), data, sites=[3])
    cgb.site = 0


# ----------------------------------------------------------------------------- 5: the generator

def _raw(cgb, a, b, seed, want_x=True):
    """pgbp_lg_simulate on the site range [a, b) with the device's generator: (x, z_out, info)."""
    from pgbp_amd import _lib as L
    nf, p = len(cgb._lg["cluster"]), cgb._lg_p
    x, z, info = np.zeros((b - a, nf, p)), np.zeros((b - a, nf, p)), np.zeros(b - a, np.int32)
    rc = cgb._lib.pgbp_lg_simulate(cgb._eng, a, b, None, seed, L.f64p(x) if want_x else None, L.f64p(z), 0, L.i32p(info))
    assert rc == 0
    return x, z, info


@pytest.mark.parametrize("p,n_sites", [(1, 65), (3, 9)])
def test_generator_matches_the_restatement_and_does_not_depend_on_the_chunks(P, p, n_sites):
    """z_out of the device's Philox4x32-10 / Box-Muller against simulate_ref.normals at 1e-12 absolute (log and sincos of the
    device are a few ulp from numpy's and |z| < 9); the same bytes for [0, S) in one call, in two half ranges and with one site
    per chunk; x is the sweep of those normals.  p = 1 in the [family][site] order, p = 3 (the last sine dropped) in the
    plain one."""
    cgb, spt, fam, Rs, site = _batch(P, p, n_sites)
    nf = len(fam["cluster"])
    x, z, info = _raw(cgb, 0, n_sites, SR.SEED)
    want = SR.normals(SR.SEED, np.arange(n_sites), nf, p)
    e = float(np.max(np.abs(z - want)))
    print(f"generator, p = {p}, {n_sites} sites x {nf} families: device vs the numpy restatement {e:.2e} (absolute)")
    assert e <= 1e-12 and not info.any()
    half = n_sites // 2
    xa, za, _ = _raw(cgb, 0, half, SR.SEED)
    xb, zb, _ = _raw(cgb, half, n_sites, SR.SEED)
    assert np.concatenate([za, zb]).tobytes() == z.tobytes() and np.concatenate([xa, xb]).tobytes() == x.tobytes()
    cgb._lib.pgbp_simulate_scratch_limits(1, 1)
    try:
        xc, zc, _ = _raw(cgb, 0, n_sites, SR.SEED)
    finally:
        cgb._lib.pgbp_simulate_scratch_limits(0, 0)
    assert zc.tobytes() == z.tobytes() and xc.tobytes() == x.tobytes()
    x2, _ = cgb.simulate_lg(z=z, all_sites=True)
    assert x2.tobytes() == x.tobytes()
    _, z7, _ = _raw(cgb, 0, n_sites, SR.SEED + 1, want_x=False)
    assert not np.array_equal(z7, z)


def test_generator_moments(P):
    """The first 2^17 normals of the seed ([site][family] order, 78 families at p = 1): mean and variance inside the band
    test_simulate_cpu.py checked for the restatement."""
    s, nf, p = SR.MOMENT_SHAPE
    cgb, spt, fam, Rs, site = _batch(P, p, s)
    assert len(fam["cluster"]) == nf
    _, z, _ = _raw(cgb, 0, s, SR.SEED, want_x=False)
    z = z.reshape(-1)[: 1 << 17]
    em, ev = SR.moment_band(z)
    print(f"2^17 device normals: |mean| {em:.2f} s.e., |var - 1| {ev:.2f} s.e.")
    assert em <= 5.0 and ev <= 5.0


# ----------------------------------------------------------------------------- 6: refusals

def _state(pcgb):
    return _bytes(pcgb) + pcgb.get_data_lg().tobytes()


def test_refusals_leave_the_engine_unchanged(P):
    from pgbp_amd import _lib as L
    # an improper root
    net, model, tbl, taxa = LR.random_case("bm_improper", 2)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    assert (np.asarray(fam["parent_family"]) == -2).any()
    s0 = _state(pcgb)
    with pytest.raises(L.PgbpError) as ex:
        pcgb.simulate_lg(seed=1, write_data=True)
    assert ex.value.code == L.ERR_INVALID and "without a proper prior" in ex.value.msg and "family 0, parent 0" in ex.value.msg
    assert _state(pcgb) == s0
    # no topology (an older table without parent_family), then no parameters
    c = _one_site(P, "hetero_random", 2)
    pcgb, fam, kw = c["pcgb"], c["fam"], c["kw"]
    x0, _ = pcgb.simulate_lg(seed=5)
    data = pcgb.get_data_lg()
    pcgb.lg_setup({k: v for k, v in fam.items() if k != "parent_family"}, data)
    pcgb.assignfactors_lg_(**kw)
    s0 = _state(pcgb)
    with pytest.raises(L.PgbpError) as ex:
        pcgb.simulate_lg(seed=5, write_data=True)
    assert ex.value.code == L.ERR_STATE and "topology" in ex.value.msg and _state(pcgb) == s0
    pcgb.lg_setup(fam, data)
    with pytest.raises(L.PgbpError) as ex:
        pcgb.simulate_lg(seed=5, write_data=True)
    assert ex.value.code == L.ERR_STATE and "parameters" in ex.value.msg
    pcgb.assignfactors_lg_(**kw)
    s0 = _state(pcgb)
    # a topology entry that is not before its child, out of range, or below -2: refused, the topology in force stays
    K = int(fam["max_parents"])
    f = int(np.flatnonzero(np.asarray(fam["n_parents"]) >= 2)[0])
    for k, v, text in ((1, f, "does not come before"), (0, len(fam["cluster"]), "out of range"), (0, -3, "out of range")):
        bad = np.array(fam["parent_family"], np.int32).copy()
        bad[f * K + k] = v
        assert pcgb._lib.pgbp_lg_set_topology(pcgb._eng, L.i32p(bad)) == L.ERR_INVALID
        msg = pcgb._lib.pgbp_last_error(pcgb._eng).decode()
        assert f"family {f}, parent {k}" in msg and text in msg, msg
    x1, _ = pcgb.simulate_lg(seed=5)
    assert x1.tobytes() == x0.tobytes() and _state(pcgb) == s0
    # the other refusals of the call
    nf, p = len(fam["cluster"]), 2
    x, info = np.zeros((1, nf, p)), np.zeros(1, np.int32)
    sim = pcgb._lib.pgbp_lg_simulate
    assert sim(pcgb._eng, 0, 2, None, 1, L.f64p(x), None, 0, L.i32p(info)) == L.ERR_INVALID      # a bad site range
    assert sim(pcgb._eng, 0, 1, None, 1, None, None, 0, L.i32p(info)) == L.ERR_INVALID           # nothing to do
    assert _state(pcgb) == s0
    with pytest.raises(ValueError, match="exactly one"):
        pcgb.simulate_lg()
    bare = P.ClusterGraphBelief.from_arrays(*N.engine_arrays(P, c["ocgb"]), None)
    assert bare._lib.pgbp_lg_set_topology(bare._eng, L.i32p(np.zeros(1, np.int32))) == L.ERR_STATE
    assert bare._lib.pgbp_lg_get_data(bare._eng, 0, 1, L.f64p(np.zeros(1))) == L.ERR_STATE


def test_a_site_whose_variance_is_indefinite(P):
    """Eight sites at p = 2 with their own R; site 3's is made indefinite: info = 1 there (the first family), its x NaN, its
    data untouched; the other sites as with a proper R at site 3."""
    n_sites, p = 8, 2
    nwk, taxa, data, Rs, mus = LR.batch_case(p, n_sites=n_sites)
    cgb, spt, fam, _, site = _batch(P, p, n_sites)
    good, ginfo = cgb.simulate_lg(seed=3, all_sites=True)
    bad_R = Rs.copy()
    bad_R[3] = np.array([[1.0, 2.0], [2.0, 1.0]])
    cgb.assignfactors_lg_(bad_R[:, None], mus)
    before = cgb.get_data_lg()
    x, info = cgb.simulate_lg(seed=3, write_data=True, all_sites=True)
    assert not ginfo.any() and info.tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert np.isnan(x[3]).all()
    keep = [s for s in range(n_sites) if s != 3]
    assert x[keep].tobytes() == good[keep].tobytes()
    after = _check_written(cgb, fam, np.where(np.isnan(x), 0.0, x), before, sites=keep)
    assert after[3].tobytes() == before[3].tobytes()


# ----------------------------------------------------------------------------- 7: the bootstrap driver

def _replicates(P, n_sites=8):
    net, model, tbl, taxa = LR.random_case("bm_random", 2)
    cg = OCG.cliquetree(net)
    ocgb, fam, data, kw = SR.oracle_table(net, model, tbl, taxa)
    cgb = P.ClusterGraphBelief.from_arrays(*N.engine_arrays(P, ocgb), None, n_sites=n_sites)
    cgb.lg_setup(fam, np.repeat(data[None], n_sites, axis=0))
    cgb.assignfactors_lg_(**kw)
    spt = OCG.spanningtree_clusterlist(cg, OCG.default_rootcluster(cg, net))
    return net, model, taxa, ocgb, fam, cgb, spt


def test_bootstrap_of_the_shift_scan(P):
    """bootstrap_shift_scan_lg with host normals on 8 replicates of a 24-tip network (p = 2): per replicate the largest lr and
    its edge against scan_ref's dense statement on that replicate's simulated data; the call equals the same steps done by hand,
    bytes for bytes; the data it returns restore the engine."""
    net, model, taxa, ocgb, fam, cgb, spt = _replicates(P)
    nf, p, B = len(fam["cluster"]), 2, 8
    z = np.random.default_rng(77).normal(size=(B, nf, p))
    cgb._ensure_schedule([spt])
    ll0, _ = cgb.loglik_lg()
    out = P.bootstrap_shift_scan_lg(cgb, spt, z=z)
    assert not out["info"].any() and out["max_lr"].shape == (B,) and len(set(out["family"].tolist())) > 1
    K = int(fam["max_parents"])
    gam = np.asarray(fam["gamma"]).reshape(nf, K)
    worst = 0.0
    for s in range(B):
        want = SC.device_layout(SC.dense_scan(net, model, {}, _tbl_of(out["data"][s], fam, taxa, p), taxa), net, ocgb, fam)
        lr = np.where((want["dof"] > 0) & np.isfinite(want["lr"]), want["lr"], -np.inf)
        f = int(np.argmax(lr))
        worst = max(worst, abs(out["max_lr"][s] - lr[f]) / lr[f])
        assert out["family"][s] == f and tuple(out["edge"][s]) == (f, int(np.argmax(gam[f, : fam["n_parents"][f]])))
    print(f"bootstrap, 8 replicates: the largest lr against the dense scan {worst:.2e}; "
          f"max lr {np.array2string(out['max_lr'], precision=2)}")
    assert worst <= TOL
    _, _, _, _, _, hand, spt2 = _replicates(P)
    x, info = hand.simulate_lg(z=z, write_data=True, all_sites=True)
    ll, scan = hand.loglik_and_shift_scan_lg(spt2, all_sites=True)
    assert x.tobytes() == out["x"].tobytes() and ll.tobytes() == out["loglik"].tobytes()
    assert hand.get_data_lg().tobytes() == out["data"].tobytes()
    assert np.nanmax(scan["lr"], axis=1).tobytes() == out["max_lr"].tobytes()
    cgb.set_data_lg(out["data_before"])
    ll1, _ = cgb.loglik_lg()
    assert ll1.tobytes() == ll0.tobytes()
    seeded = P.bootstrap_shift_scan_lg(cgb, spt, seed=SR.SEED)
    again = P.bootstrap_shift_scan_lg(cgb, spt, seed=SR.SEED)
    assert seeded["max_lr"].tobytes() == again["max_lr"].tobytes() and seeded["max_lr"].tobytes() != out["max_lr"].tobytes()


# ----------------------------------------------------------------------------- 8: borrowed engines

def test_a_patterns_handle_takes_the_calls(P):
    """An engine borrowed from a pgbp_patterns handle takes set_topology (through lg_setup), simulate_lg, set_data_lg and
    get_data_lg like any other: the same bytes as an engine of its own on the same sites."""
    from pgbp_amd.sharding import PatternGroup
    n_sites, p = 8, 1
    nwk, taxa, data, Rs, mus = LR.batch_case(p, n_sites=n_sites)
    cgb, spt, fam, _, site = _batch(P, p, n_sites)
    arrays = (cgb._dims.copy(), cgb._sepcl.reshape(-1).copy(), cgb._scope_off.copy(), cgb._scope_idx.copy())
    pats = PatternGroup([arrays + (list(range(0, n_sites, 2)),), arrays + (list(range(1, n_sites, 2)),)])
    pats.set_schedule([spt])
    cgb._ensure_schedule([spt])
    z = np.random.default_rng(31).normal(size=(n_sites, len(fam["cluster"]), p))
    x, _ = cgb.simulate_lg(z=z, write_data=True, all_sites=True)
    ll, _ = cgb.loglik_lg()
    for k in range(2):
        idx = list(range(k, n_sites, 2))
        b = pats.beliefs[k]
        b.lg_setup(fam, data[idx])
        b.assignfactors_lg_(Rs[idx][:, None], mus[idx])
        xb, info = b.simulate_lg(z=z[idx], write_data=True, all_sites=True)
        assert not info.any() and xb.tobytes() == x[idx].tobytes()
        assert b.get_data_lg().tobytes() == cgb.get_data_lg()[idx].tobytes()
        b.set_data_lg(b.get_data_lg())
    ll2, info2 = pats.loglik_lg()
    pats.close()
    e = float(np.max(np.abs(ll2 - ll) / np.maximum(1.0, np.abs(ll))))
    print(f"patterns handle: simulated data, loglik of the handle against the engine's {e:.2e}")
    assert not info2.any() and e <= TOL


# ----------------------------------------------------------------------------- 9: a set-up replaces the whole model, or nothing

def _six_tips(P, p, n_sites, other=False, topology=True):
    """loo_ref.batch_case on 6 tips under a fixed root, the second tip's last trait missing at every site (the table carries
    masks); other: another table on the same graph (other edge lengths and data).  (family table, data, assignfactors_lg_
    arguments, schedule tree, a constructor of engines on the graph).  One site: the plain layout; 9 univariate sites: the
    site-minor one, with a ragged row."""
    nwk, taxa, data, Rs, mus = LR.batch_case(p, n_sites=n_sites, ntips=6)
    data = data.copy()
    if other:
        data = 1.5 * data[::-1] + 0.25
    data[:, 1, p - 1] = np.nan
    net, names = P.read_newick(nwk)
    row = {t: r for r, t in enumerate(taxa)}
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=True)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], p, data=data[0])
    assert fam.get("child_mask") is not None and fam.get("parent_family") is not None
    if other:
        fam = dict(fam, length=np.asarray(fam["length"]) * 1.75)
    if not topology:
        fam = {k: v for k, v in fam.items() if k != "parent_family"}
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    new = lambda: P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=n_sites)
    kw = dict(R=Rs[:, None], mu=mus) if n_sites > 1 else dict(R=Rs[0][None], mu=mus[0])
    return fam, data, kw, spt, new


def _dressed(P, p, n_sites):
    """An engine with parameters, two shifts, noise on two tips and a topology."""
    fam, data, kw, spt, new = _six_tips(P, p, n_sites)
    cgb = new()
    cgb.lg_setup(fam, data)
    cgb.assignfactors_lg_(**kw)
    real = [f for f in range(len(fam["cluster"])) if fam["n_parents"][f] == 1]
    cgb.set_shifts_lg([(real[0], 0), (real[-1], 0)], np.array([[0.5] * p, [-0.25] * p]))
    tips = [f for f in LR.tip_families(fam)]
    cgb.set_tip_noise_lg(tips[:2], 0.1 * np.eye(p), se2=np.full((2, p), 0.05))
    cgb.assignfactors_lg_(**kw)
    assert cgb.shift_count_lg() == 2 and cgb.tip_noise_count_lg() == 2
    return cgb, spt, kw


def _sweep_bytes(cgb, spt):
    """The bytes of the log-likelihood and of every sweep on a calibration under the engine's current model."""
    cgb._ensure_schedule([spt])
    d = dict(loglik=cgb.loglik_lg()[0])
    if cgb.n_sites >= 8:      # (first: it reads the beliefs in the layout the calibration leaves)
        ll, g = cgb.loglik_and_gradient_sites_lg(spt)
        d.update(ll_sites=np.asarray(ll), **{"s_" + k: np.asarray(v) for k, v in g.items()})
    ll, g = cgb.loglik_and_gradient_lg(spt, all_sites=True)
    d.update(ll=np.asarray(ll), **{"g_" + k: np.asarray(v) for k, v in g.items()})
    for tag, out in (("e_", cgb.edge_gradient_lg(all_sites=True)), ("c_", cgb.shift_scan_lg(all_sites=True, information=True)),
                     ("l_", cgb.loo_lg(all_sites=True)), ("i_", cgb.impute_lg(all_sites=True))):
        d.update({tag + k: np.asarray(v) for k, v in out.items()})
    # (the second tip misses its last trait: at p = 1 it has no observed trait left and is no leave-one-out target)
    assert len(d["l_families"]) == (6 if cgb._lg_p > 1 else 5) and len(d["i_families"]) == 1 and not d["g_info"].any()
    return {k: v.tobytes() for k, v in d.items()}


@pytest.mark.parametrize("p,n_sites", [(2, 1), (1, 9)])
def test_a_second_setup_is_a_clean_slate(P, p, n_sites):
    """lg_setup with another table on an engine that has parameters, shifts, tip noise and a topology: none of them is left,
    and after assignfactors_lg_ the log-likelihood and every sweep return the bytes of a fresh engine set up the same way."""
    cgb, spt, kw = _dressed(P, p, n_sites)
    _sweep_bytes(cgb, spt)
    fam2, data2, kw2, _, new = _six_tips(P, p, n_sites, other=True, topology=False)
    cgb.lg_setup(fam2, data2)
    assert cgb.shift_count_lg() == 0 and cgb.tip_noise_count_lg() == 0
    with pytest.raises(P.PgbpError, match="no topology"):
        cgb.simulate_lg(seed=1, all_sites=True)
    for sweep in (cgb.gradient_lg, cgb.edge_gradient_lg, cgb.shift_scan_lg, cgb.loo_lg, cgb.impute_lg):
        with pytest.raises(P.PgbpError, match="no parameters yet"):
            sweep(all_sites=True)
    cgb.assignfactors_lg_(**kw2)
    got = _sweep_bytes(cgb, spt)
    fresh = new()
    fresh.lg_setup(fam2, data2)
    fresh.assignfactors_lg_(**kw2)
    want = _sweep_bytes(fresh, spt)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], k


@pytest.mark.parametrize("p,n_sites", [(2, 1), (1, 9)])
def test_a_refused_setup_leaves_the_old_model_whole(P, p, n_sites):
    """lg_setup with a table whose last family has a non-positive edge length is refused: the counts, a seeded simulation (the
    topology) and every sweep are what they were before the call."""
    cgb, spt, kw = _dressed(P, p, n_sites)
    before = _sweep_bytes(cgb, spt)
    x0, _ = cgb.simulate_lg(seed=SR.SEED, all_sites=True)
    fam2, data2, _, _, _ = _six_tips(P, p, n_sites, other=True)
    bad = np.array(fam2["length"], np.float64)
    bad[-1] = 0.0
    mirror = cgb._lg      # (the wrapper's own copy of the table: it is replaced before the engine is asked)
    with pytest.raises(P.PgbpError, match="parent edge length must be positive"):
        cgb.lg_setup(dict(fam2, length=bad), data2)
    cgb._lg = mirror
    assert cgb.shift_count_lg() == 2 and cgb.tip_noise_count_lg() == 2
    x1, info = cgb.simulate_lg(seed=SR.SEED, all_sites=True)
    assert not info.any() and x1.tobytes() == x0.tobytes()
    after = _sweep_bytes(cgb, spt)
    for k in before:
        assert after[k] == before[k], k

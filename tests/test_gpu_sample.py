"""pgbp_sample_posterior: joint posterior draws of every cluster variable from calibrated beliefs, one device call.

The device is compared with tests/sample_ref.py (the numpy restatement of the header's semantics, pinned to the dense
oracle in test_sample_cpu.py) at 1e-8 relative to the largest entry, the project's parity bound, on the beliefs read back
from the device; the law itself is checked through the device against oracle.densemvn.posterior_node_moments with
z = [0; I_D].  Every test prints its measured figure before it
asserts.  Measured on the MI355X: device against the restatement <= 8.0e-16 over every case (largest at 128 variables), the
law through the device 5.7e-16 (mean) and 1.3e-15 (covariance), packed against plain layout 0 (the same bytes)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import goldens, make_model, oracle_setup, product_beliefs_from_oracle
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from sample_ref import law_errors, sample_posterior_ref, unit_draws, variable_nodes

pytestmark = pytest.mark.gpu
G = goldens()


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


# ----------------------------------------------------------------------------- raw calls

def _f64(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _size(cgb):
    return int(cgb._lib.pgbp_sample_size(cgb._eng))


def _raw(cgb, tree, s0, s1, n_draws, z, x=None, info=None, null_z=False, null_x=False):
    """The C call itself: (status, x [n_draws, s1 - s0, size], info [s1 - s0])."""
    ns = max(s1 - s0, 1)
    if x is None:
        x = np.full((max(n_draws, 1), ns, _size(cgb)), -7.0)
    if info is None:
        info = np.full(ns, -3, dtype=np.int32)
    z = np.ascontiguousarray(z, dtype=np.float64)
    rc = cgb._lib.pgbp_sample_posterior(cgb._eng, tree, s0, s1, n_draws, None if null_z else _f64(z),
                                        None if null_x else _f64(x), info.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, x, info


def _err(cgb):
    return cgb._lib.pgbp_last_error(cgb._eng)


def _records(cgb, site):
    out = []
    for b in range(cgb.nclusters):
        m = int(cgb._dims[b])
        rec = np.zeros(m * m + m + 1)
        assert cgb._lib.pgbp_get_belief(cgb._eng, site, b, _f64(rec)) == 0
        out.append((rec[: m * m].reshape(m, m, order="F").copy(), rec[m * m: m * m + m].copy()))
    return out


def _set_record(cgb, site, b, J, h, g=0.0):
    rec = np.concatenate([np.asarray(J, float).reshape(-1, order="F"), np.asarray(h, float), [float(g)]])
    assert cgb._lib.pgbp_set_belief(cgb._eng, site, b, _f64(rec)) == 0


def _ref(cgb, sched, z, site=0):
    """the restatement on the device's own beliefs of one site; z [n_draws, size]"""
    return sample_posterior_ref(_records(cgb, site), cgb._dims, cgb._sepcl, cgb._scope_off, cgb._scope_idx,
                                sched[-2], sched[-1], z)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _draws(cgb, n, seed, sites=1):
    """n random draws of z after one of zeros"""
    z = np.random.default_rng(seed).standard_normal((n + 1, sites, _size(cgb)))
    z[0] = 0.0
    return z


def _assert_device_is_restatement(cgb, sched, name, sites=(0,), n_sites=1, tree=0):
    z = _draws(cgb, 3, 11, n_sites)
    rc, x, info = _raw(cgb, tree, 0, n_sites, 4, z)
    assert rc == 0, _err(cgb)
    assert not info.any()
    worst = 0.0
    for s in sites:
        want, winfo = _ref(cgb, sched, z[:, s], site=s)
        assert winfo == 0
        err = float(np.max(np.abs(x[:, s] - want)) / np.max(np.abs(want)))
        worst = max(worst, err)
        assert err <= 1e-8, (name, s, err)
    print(f"{name}: size {_size(cgb)}, largest cluster {int(cgb._dims[:cgb.nclusters].max())}, device vs restatement {worst:.2e}")
    return z, x


# ----------------------------------------------------------------------------- calibrated states

def _synth_tree(P, ntips, p, seed, n_sites=1, calibrate=True):
    from pgbp_amd import synth as S
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    R = S.random_rate_matrix(p, rng)
    prob = S.cliquetree_of_tree(tr, p)
    packed = np.stack([S.bm_factors_cliquetree(tr, prob, R, np.zeros(p), S.simulate_bm(tr, R, np.zeros(p), rng))
                       for _ in range(n_sites)])
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx,
                                           packed if n_sites > 1 else packed[0], n_sites=n_sites)
    if calibrate:
        assert P.calibrate_(cgb, prob.schedule, 2) == (True, True)
    return prob, cgb


def _oracle_cliquetree(P, net, model, tbl, taxa):
    """the clique tree of `net` with the oracle's scopes and factors, calibrated on the device"""
    ct = OCG.cliquetree(net)
    spt = OCG.spanningtree_clusterlist(ct, OCG.default_rootcluster(ct, net))
    ocgb = oracle_setup(net, ct, model, tbl, taxa)
    pcgb = P.ClusterGraphBelief(product_beliefs_from_oracle(ocgb.belief), ocgb.node2cluster, ocgb.node2family,
                                ocgb.node2fixed, ocgb.cluster2nodes)
    assert P.calibrate_(pcgb, [spt])[0]
    return ocgb, pcgb, spt


def _golden_cliquetree(P, key, traits, v=None):
    g = G[key]
    md = dict(g["model"])
    if v is not None:
        md["v"] = v
    net = ON.read_newick(g["net"])
    model = make_model(md)
    tbl = [g[t] for t in traits]
    return (net, model, tbl, g["taxa"]) + _oracle_cliquetree(P, net, model, tbl, g["taxa"])


def _bm(p, rng, v=None):
    A = rng.normal(size=(p, p))
    R = A @ A.T / p + np.eye(p)
    if p == 1:
        return OM.UnivariateBrownianMotion(float(R[0, 0]), 0.3, v)
    return OM.MvFullBrownianMotion(R, rng.normal(size=p), v)


# ----------------------------------------------------------------------------- device against the restatement

@pytest.mark.parametrize("p,ntips", [(1, 6), (8, 5), (24, 5), (32, 5), (40, 4), (64, 4)])
def test_sample_random_trees_all_classes(P, p, ntips):
    """Clusters of p and 2p variables at the smallest sizes that reach each class: four clusters per wavefront (2, 16),
    a wavefront (48, 64), a workgroup (80, 128)."""
    prob, cgb = _synth_tree(P, ntips, p, 300 + p)
    assert int(cgb._dims[: cgb.nclusters].max()) == 2 * p
    _assert_device_is_restatement(cgb, prob.schedule[0], f"tree p={p}")


def test_sample_ragged_cliquetree_golden(P):
    """calibration_cliquetree_level1: clusters of one to three variables, sepsets of one and two."""
    *_, pcgb, spt = _golden_cliquetree(P, "calibration_cliquetree_level1", ["y"])
    _assert_device_is_restatement(pcgb, spt, "golden level-1 clique tree")


def test_sample_missing_data_tree_dimension_zero_sepset(P):
    """calibration_tree_2traits_missing: a dimension-0 sepset makes its child an independent draw."""
    *_, pcgb, spt = _golden_cliquetree(P, "calibration_tree_2traits_missing", ["y1", "y2"])
    assert 0 in [int(d) for d in pcgb._dims[pcgb.nclusters:]]
    _assert_device_is_restatement(pcgb, spt, "golden missing-data tree")


def test_sample_level3_network_cliquetree(P):
    """The clique tree of a small level-3 network (12 tips, 2 blobs, p = 2): sepsets that hold several nodes."""
    rng = np.random.default_rng(21)
    net = ON.random_level3_network(12, 2, rng)
    taxa = net.tip_names
    tbl = [list(rng.normal(size=len(taxa))) for _ in range(2)]
    ocgb, pcgb, spt = _oracle_cliquetree(P, net, _bm(2, rng, 0.6 * np.eye(2)), tbl, taxa)
    assert max(len(b.nodelabel) for b in ocgb.belief[ocgb.nclusters:]) >= 2
    _assert_device_is_restatement(pcgb, spt, "level-3 network clique tree")


# ----------------------------------------------------------------------------- the law, through the device

def _assert_law(P, name, net, model, tbl, taxa):
    ocgb, pcgb, spt = _oracle_cliquetree(P, net, model, tbl, taxa)
    D = _size(pcgb)
    vn = variable_nodes(ocgb.belief, ocgb.nclusters)
    assert len(vn) == D
    rc, x, info = _raw(pcgb, 0, 0, 1, 1 + D, unit_draws(D)[:, None, :])
    assert rc == 0 and info[0] == 0, _err(pcgb)
    pm, pc = OD.posterior_node_moments(net, model, tbl, taxa)
    em, ec = law_errors(x[:, 0], vn, model.dimension(), pm, pc)
    print(f"{name}: D = {D}, mean {em:.2e}, covariance {ec:.2e}")
    assert em <= 1e-8 and ec <= 1e-8
    return D


def test_sample_law_tree_6_tips_2_traits(P):
    rng = np.random.default_rng(31)
    net = ON.random_network(6, 0, rng)
    tbl = [list(rng.normal(size=6)) for _ in range(2)]
    D = _assert_law(P, "6-tip tree, 2 traits, random root", net, _bm(2, rng, 0.8 * np.eye(2)), tbl, net.tip_names)
    assert 20 <= D <= 60


def test_sample_law_level1_network(P):
    g = G["canonicalform_six_messages"]
    md = dict(g["model"])
    md["v"] = 0.8
    _assert_law(P, "level-1 network, random root", ON.read_newick(g["net"]), make_model(md), [g["y"]], g["taxa"])


# ----------------------------------------------------------------------------- batching

def test_sample_batching_bit_identity(P):
    """3 sites x 5 draws: each (draw, site) the bits of a call of its own; two identical calls the same bytes; a variable
    shared by two clusters the same bits in both."""
    prob, cgb = _synth_tree(P, 7, 3, 41, n_sites=3)
    z = np.random.default_rng(5).standard_normal((5, 3, _size(cgb)))
    rc, x, info = _raw(cgb, 0, 0, 3, 5, z)
    assert rc == 0 and not info.any(), _err(cgb)
    assert not np.array_equal(x[:, 0], x[:, 1])
    rc, again, _ = _raw(cgb, 0, 0, 3, 5, z)
    assert rc == 0 and np.array_equal(_bits(x), _bits(again))
    for d in range(5):
        for s in range(3):
            rc, one, inf1 = _raw(cgb, 0, s, s + 1, 1, z[d:d + 1, s:s + 1])
            assert rc == 0 and inf1[0] == 0
            assert np.array_equal(_bits(one[0, 0]), _bits(x[d, s])), (d, s)
    # the same batch cut into chunks of 1 site and 2 draws (strided copies of z and x): the same bytes
    cgb._lib.pgbp_sample_scratch_limits(1, 2 * _size(cgb))
    try:
        rc, cut, infc = _raw(cgb, 0, 0, 3, 5, z)
    finally:
        cgb._lib.pgbp_sample_scratch_limits(0, 0)
    assert rc == 0 and not infc.any() and np.array_equal(_bits(cut), _bits(x))
    # a strict subset of the sites: only its rows of info, the same values
    rc, mid, infm = _raw(cgb, 0, 1, 2, 5, z[:, 1:2])
    assert rc == 0 and np.array_equal(_bits(mid[:, 0]), _bits(x[:, 1]))
    # shared variables: sepset k maps positions of its two clusters onto each other
    off = np.concatenate([[0], np.cumsum(cgb._dims[: cgb.nclusters].astype(np.int64))])
    n_shared = 0
    for k, (a, b) in enumerate(cgb._sepcl):
        ia = cgb._scope_idx[cgb._scope_off[2 * k]: cgb._scope_off[2 * k + 1]]
        ib = cgb._scope_idx[cgb._scope_off[2 * k + 1]: cgb._scope_off[2 * k + 2]]
        assert np.array_equal(_bits(x[:, :, off[a] + ia]), _bits(x[:, :, off[b] + ib])), k
        n_shared += len(ia)
    assert n_shared >= 9


# ----------------------------------------------------------------------------- layouts

def test_sample_packed_layout_against_plain(P):
    """A tree with p = 16 is in the packed (BS16) layout after a calibration; the same beliefs converted to the plain layout
    (pgbp_get_belief converts) give the same draws.  Both gathers read the upper triangle, element by element the same values,
    and the arithmetic is the same: asserted at 1e-12 relative to the largest entry, the bound test_gpu_gradient.py uses for
    the two layouts; the measured figure is printed."""
    prob, cgb = _synth_tree(P, 8, 16, 51)
    assert cgb._lib.pgbp_layout(cgb._eng) == 1, "the p = 16 tree is expected in the packed layout after a calibration"
    z = _draws(cgb, 3, 2)
    rc, packed, info = _raw(cgb, 0, 0, 1, 4, z)
    assert rc == 0 and info[0] == 0, _err(cgb)
    assert cgb._lib.pgbp_layout(cgb._eng) == 1                  # (the call reads the packed records as they are)
    want, _ = _ref(cgb, prob.schedule[0], z[:, 0])              # (pgbp_get_belief: the engine is in the plain layout now)
    assert cgb._lib.pgbp_layout(cgb._eng) == 0
    rc, plain, info = _raw(cgb, 0, 0, 1, 4, z)
    assert rc == 0 and info[0] == 0
    scale = float(np.max(np.abs(want)))
    e_layout = float(np.max(np.abs(packed - plain))) / scale
    e_ref = float(np.max(np.abs(packed[:, 0] - want))) / scale
    print(f"packed vs plain layout {e_layout:.2e}, packed vs restatement {e_ref:.2e}")
    assert e_layout <= 1e-12 and e_ref <= 1e-8


def test_sample_site_minor_univariate_batch(P):
    """A univariate batch (p = 1, 64 sites) lives in the site-minor layout after a calibration: the call converts to the plain
    layout first (the restatement then reads those plain records), and the engine goes on working afterwards."""
    prob, cgb = _synth_tree(P, 9, 1, 77, n_sites=64)
    # (the host mirror of a batch pulls every belief after a calibration, which leaves the engine in the plain layout: one
    # more traversal without the pull leaves it in its own)
    assert P.calibrate_(cgb, prob.schedule, 1, sync=False)[0]
    assert cgb._lib.pgbp_layout(cgb._eng) & 2, "a univariate batch is expected in the site-minor layout after a calibration"
    _assert_device_is_restatement(cgb, prob.schedule[0], "site-minor batch", sites=(0, 17, 63), n_sites=64)
    assert P.calibrate_(cgb, prob.schedule, 1)[0]


# ----------------------------------------------------------------------------- failure

def test_sample_indefinite_cluster_of_one_site(P):
    """One cluster of one site indefinite in its R block: info names it, that site is all NaN, the other sites keep their
    bits, and nothing on the device is marked: a following calibrate_ gives what it gives on a twin that never sampled."""
    twins = []
    for _ in range(2):
        prob, cgb = _synth_tree(P, 7, 3, 61, n_sites=3)
        twins.append(cgb)
    cgb, twin = twins
    z = np.random.default_rng(9).standard_normal((2, 3, _size(cgb)))
    rc, base, info = _raw(cgb, 0, 0, 3, 2, z)
    assert rc == 0 and not info.any()
    pa, ch = prob.schedule[0][-2], prob.schedule[0][-1]
    bad = next(int(c) for c in ch if int(cgb._dims[int(c)]) == 6)      # a {child, parent} cluster: R = the child's 3 traits
    k = next(k for k in range(cgb.nsepsets) if bad in cgb._sepcl[k] and int(pa[list(ch).index(bad)]) in cgb._sepcl[k])
    side = 0 if cgb._sepcl[k][0] == bad else 1
    S = set(cgb._scope_idx[cgb._scope_off[2 * k + side]: cgb._scope_off[2 * k + side + 1]].tolist())
    R = [v for v in range(6) if v not in S]
    assert len(R) == 3
    for c in (cgb, twin):
        J, h = _records(c, 1)[bad]
        J[R[1], R[1]] = -1.0                                            # the second pivot of J_RR is negative
        _set_record(c, 1, bad, J, h)
    rc, x, info = _raw(cgb, 0, 0, 3, 2, z)
    assert rc == 0, _err(cgb)
    assert info.tolist() == [0, bad + 1, 0]
    assert np.all(np.isnan(x[:, 1]))
    assert np.array_equal(_bits(x[:, [0, 2]]), _bits(base[:, [0, 2]]))
    want, winfo = _ref(cgb, prob.schedule[0], z[:, 1], site=1)
    assert winfo == bad + 1
    r1 = P.calibrate_(cgb, prob.schedule, 1)
    r2 = P.calibrate_(twin, prob.schedule, 1)
    assert r1 == r2
    cgb.pull()
    twin.pull()
    assert np.array_equal(_bits(cgb._packed_raw), _bits(twin._packed_raw))


# ----------------------------------------------------------------------------- refusals

def test_sample_refusals(P):
    prob, cgb = _synth_tree(P, 6, 2, 71, n_sites=2)
    D = _size(cgb)
    z = np.zeros((1, 2, D))
    canvas = np.full((1, 2, D), 9.0)
    for args, code, word in (((5, 0, 2, 1), 1, b"tree 5"), ((-1, 0, 2, 1), 1, b"tree -1"), ((0, 0, 2, 0), 1, b"n_draws = 0"),
                             ((0, -1, 2, 1), 1, b"site range"), ((0, 2, 1, 1), 1, b"site range"),
                             ((0, 0, 3, 1), 1, b"site range")):
        rc, _, _ = _raw(cgb, *args, z, x=canvas)
        assert rc == code and word in _err(cgb), (args, _err(cgb))
    rc, _, _ = _raw(cgb, 0, 0, 2, 1, z, x=canvas, null_z=True)
    assert rc == 1 and b"buffer z" in _err(cgb)
    rc, _, _ = _raw(cgb, 0, 0, 2, 1, z, x=canvas, null_x=True)
    assert rc == 1 and b"buffer x" in _err(cgb)
    assert np.all(canvas == 9.0)
    with pytest.raises(P.PgbpError):
        cgb.sample_posterior_(schedule_tree=3)
    # no schedule set
    _, fresh = _synth_tree(P, 6, 2, 71, calibrate=False)
    rc, _, _ = _raw(fresh, 0, 0, 1, 1, z[:, :1])
    assert rc == 6 and b"no schedule" in _err(fresh)


def test_sample_refuses_a_bethe_graph(P):
    g = G["joingraph_mateescu"]
    net, names = P.read_newick(g["net"])
    cn, ed, sn = P.bethe(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, 2)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.set_schedule(P.spanningtrees_clusterlist(len(cn), ed, cn, net.is_leaf))
    D = _size(cgb)
    rc, x, _ = _raw(cgb, 0, 0, 1, 1, np.zeros((1, 1, D)))
    assert rc == 1 and b"clique tree only" in _err(cgb) and np.all(x == -7.0)


def test_sample_refuses_muller_cliquetree_three_traits(P):
    """The clique tree of the Mueller et al. network at 3 traits has a cluster of 162 variables."""
    from helpers import network_from_newick_file
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "muller_2022.phy")
    net, names, _, _ = network_from_newick_file(P, path)
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, 3)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.set_schedule([P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))])
    big = next(b for b in range(cgb.nclusters) if int(cgb._dims[b]) > 128)
    D = _size(cgb)
    rc, x, _ = _raw(cgb, 0, 0, 1, 1, np.zeros((1, 1, D)))
    msg = _err(cgb).decode()
    assert rc == 1 and f"belief {big} has {int(cgb._dims[big])} variables, more than the 128" in msg and np.all(x == -7.0)


# ----------------------------------------------------------------------------- the host mirror

def test_sample_host_mirror(P):
    net, model, tbl, taxa, ocgb, pcgb, spt = _golden_cliquetree(P, "calibration_tree_2traits_missing", ["y1", "y2"])
    x1, info1, views = pcgb.sample_posterior_(n_draws=4, rng=7)
    x2, info2, _ = pcgb.sample_posterior_(n_draws=4, rng=7)
    D = _size(pcgb)
    assert x1.shape == (4, 1, D) and info1.tolist() == [0] and np.array_equal(_bits(x1), _bits(x2))
    assert len(views) == pcgb.nclusters and sum(v.shape[2] for v in views) == D
    z = np.random.default_rng(7).standard_normal((4, 1, D))
    x3, _, _ = pcgb.sample_posterior_(n_draws=4, z=z)
    assert np.array_equal(_bits(x1), _bits(x3))
    xm, _, _ = pcgb.sample_posterior_(z=np.zeros((1, 1, D)))
    want, _ = _ref(pcgb, spt, np.zeros((1, D)))
    assert np.max(np.abs(xm[:, 0] - want)) <= 1e-8 * np.max(np.abs(want))
    by_node = pcgb.node_samples(x1)
    seen_nan, at, first = False, 0, {}
    for b in ocgb.belief[: ocgb.nclusters]:
        for k, lab in enumerate(b.nodelabel):
            n = int(b.inscope[:, k].sum())
            if lab not in first:
                first[lab] = (at, b.inscope[:, k].copy())
            at += n
    assert set(by_node) == set(first)
    for lab, (o, insc) in first.items():
        v = by_node[lab]
        assert v.shape == (4, 2)
        assert np.array_equal(_bits(v[:, insc]), _bits(x1[:, 0, o: o + int(insc.sum())]))
        assert np.all(np.isnan(v[:, ~insc]))
        seen_nan |= bool((~insc).any())
    assert seen_nan
    with pytest.raises(ValueError):
        pcgb.sample_posterior_(n_draws=2, z=np.zeros((1, 1, D)))

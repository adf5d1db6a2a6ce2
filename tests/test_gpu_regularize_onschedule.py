"""regularizebeliefs_onschedule! (src/clustergraphbeliefs.jl:343-403) on the device (pgbp_regularize_onschedule: the
levelled walk of pgbp_plan_onschedule) against the host walk (one pgbp_propagate per message): beliefs, residuals and
flags bit for bit on the golden Bethe pipeline, join graphs, the Mueller clique tree (bp_level_big with the workspace),
fuzzed networks and the cfg5-size join graph; several sites at once, a site range, and the first failure in walk order."""
import logging
import os
import time

import numpy as np
import pytest

from helpers import goldens, make_model, oracle_setup, product_beliefs_from_oracle
from oracle import clustergraph as OCG
from oracle import network as ON

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def state(cgb):
    cgb.pull()
    return [a.copy() for a in (cgb._packed_raw, cgb._res, cgb._flg, cgb._kl, cgb._klflg)]


def assert_same(a, b):
    for name, x, y in zip(("beliefs", "residuals", "flags", "kldiv", "kl flags"), a, b):
        assert np.array_equal(x, y), name


def host_vs_device(P, make):
    """two engines from the same start: the host walk on one, the device on the other; returns both"""
    from pgbp_amd.beliefupdates import BPPosDefException
    from pgbp_amd.regularization import _regularizebeliefs_onschedule_host

    def run(f, cgb):
        try:
            f(cgb)
        except BPPosDefException as ex:
            return str(ex), ex.info
        return None

    h, d = make(), make()
    assert_same(state(h), state(d))
    failed = run(_regularizebeliefs_onschedule_host, h)
    assert run(P.regularizebeliefs_onschedule_, d) == failed
    if failed is None:   # (after a failure the state past it is not the walk's)
        assert_same(state(h), state(d))
    return h, d


def lg_problem(P, graph, ntips, nret, seed, p, n_data=1):
    """a random level-3 network, its cluster graph, scopes and device factor-fill inputs; n_data tip data sets"""
    rng = np.random.default_rng(seed)
    net = P.random_level3_network_varied(ntips, nret, rng, n_colors=2)
    if graph == "cliquetree":
        cn, ed, sn = P.cliquetree(net.node2family)
    elif graph == "bethe":
        cn, ed, sn = P.bethe(net.node2family)
    else:
        cn, ed, sn = P.joingraph(net.node2family, int(graph[-1]))
    st = P.allocate_scopes(cn, ed, sn, net, p)
    base = P.synth.random_rate_matrix(p, rng)
    base = (base + base.T) / 2
    rates = np.stack([base, 1.7 * base])
    mu = rng.standard_normal(p)
    Xs = [P.simulate_bm_network(net, rates, mu, rng) for _ in range(n_data)]
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, list(range(net.nnodes)), p,
                        n_rates=2)
    sched = P.spanningtrees_clusterlist(len(cn), ed, cn, net.is_leaf)
    return st, fam, Xs, rates, mu, sched


def filled(P, prob, data=0):
    st, fam, Xs, rates, mu, _ = prob
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(fam, Xs[data])
    cgb.assignfactors_lg_(rates, mu)
    return cgb


def packed_of(P, prob, data=0):
    cgb = filled(P, prob, data)
    cgb.pull()
    return cgb._packed_raw[0].copy()


def from_packed(P, st, packed):
    packed = np.atleast_2d(packed)
    return P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, packed,
                                            n_sites=packed.shape[0])


def test_golden_bethe_pipeline(P, caplog):
    """test/test_calibration.jl:94-105: the device regulariser, then calibrate!(auto) reaches calibration at
    iteration 5, schedule tree 1"""
    g = goldens()["calibration_bethe_level1"]
    net = ON.read_newick(g["net"])
    cg = OCG.bethe(net)
    sched = OCG.spanningtrees_clusterlist(cg, net)

    def make():
        ocgb = oracle_setup(net, cg, make_model(g["model"]), [g["y"]], g["taxa"])
        return P.ClusterGraphBelief(product_beliefs_from_oracle(ocgb.belief), ocgb.node2cluster, ocgb.node2family,
                                    ocgb.node2fixed, ocgb.cluster2nodes)

    _, d = host_vs_device(P, make)
    with caplog.at_level(logging.INFO, logger="PhyloGaussianBeliefProp"):
        assert P.calibrate_(d, sched, g["niter"], auto=True, info=True) == (True, True)
    assert "calibration reached: iteration 5, schedule tree 1" in caplog.text


def test_join_graph_of_size_3(P):
    prob = lg_problem(P, "joingraph3", 300, 80, 7, 3)
    host_vs_device(P, lambda: filled(P, prob))


def test_muller_clique_tree_3_traits(P):
    """beliefs of up to 162 variables: bp_level_big with the working matrix in the workspace"""
    path = os.path.join(ROOT, "tests", "golden", "muller_2022.phy")
    net, _ = P.read_newick(open(path).read())
    cn, ed, sn = P.cliquetree(net.node2family)
    p = 3
    st = P.allocate_scopes(cn, ed, sn, net, p)
    assert st.dims.max() > 128
    rng = np.random.default_rng(2)
    rates = np.stack([np.eye(p) + 0.3])
    X = P.simulate_bm_network(net, rates, np.zeros(p), rng)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, list(range(net.nnodes)), p,
                        n_rates=1)

    def make():
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
        cgb.lg_setup(fam, X)
        cgb.assignfactors_lg_(rates, np.zeros(p))
        return cgb

    host_vs_device(P, make)


@pytest.mark.parametrize("seed", range(10))
def test_fuzzed_networks(P, seed):
    """as tests/fuzz_gpu_vs_c_oracle_networks.py draws them"""
    rng = np.random.default_rng(1000 + seed)
    big = rng.random() < 0.12
    p = int(rng.integers(18, 23)) if big else int(rng.integers(1, 10))
    ntips = int(rng.integers(8, 40)) if big else int(rng.integers(8, 160))
    nret = max(1, ntips // int(rng.integers(3, 9)))
    graph = str(rng.choice(["cliquetree", "bethe", "joingraph3", "joingraph4"]))
    prob = lg_problem(P, graph, ntips, nret, 2000 + seed, p)
    host_vs_device(P, lambda: filled(P, prob))


def test_cfg5_join_graph(P):
    """the cfg5-size join graph (seed 5, as test_gpu_parity.py's cfg5 test): bit for bit, and calibrate!(auto) then
    converges at the same (iteration, schedule tree) as after the host walk"""
    rng = np.random.default_rng(5)
    p = 4
    net = P.random_level3_network_varied(20000, 5001, rng, n_colors=3)
    cn, ed, sn = P.joingraph(net.node2family, 3)
    st = P.allocate_scopes(cn, ed, sn, net, p)
    base = P.synth.random_rate_matrix(p, rng)
    base = (base + base.T) / 2
    rates = np.stack([base * f for f in (0.5, 1.0, 2.0)])
    mu = np.zeros(p)
    X = P.simulate_bm_network(net, rates, mu, rng)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, list(range(net.nnodes)), p,
                        n_rates=3)
    sched = P.spanningtrees_clusterlist(len(cn), ed, cn, net.is_leaf)

    def make():
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
        cgb.lg_setup(fam, X)
        cgb.assignfactors_lg_(rates, mu)
        return cgb

    from pgbp_amd.regularization import _regularizebeliefs_onschedule_host
    h, d = make(), make()
    t0 = time.perf_counter()
    _regularizebeliefs_onschedule_host(h)
    t1 = time.perf_counter()
    P.regularizebeliefs_onschedule_(d)
    t2 = time.perf_counter()
    print(f"cfg5 join graph: host walk {t1 - t0:.2f} s, device {1e3 * (t2 - t1):.1f} ms (first call: plan + upload)")
    assert_same(state(h), state(d))
    reached = []
    for cgb in (h, d):
        cgb.init_messagecalibrationflags_reset_()
        assert P.calibrate_(cgb, sched, 100, auto=True) == (True, True)
        r = cgb.last_results[0]
        reached.append((r.iter_reached, r.tree_reached))
    assert reached[0] == reached[1]


def test_several_sites(P):
    """all_sites=True on 3 sites of different data = the host walk on single-site engines of each site's data; the
    range [1, 2) leaves sites 0 and 2 bitwise untouched"""
    import ctypes as C
    from pgbp_amd import _lib as L
    from pgbp_amd.regularization import _regularizebeliefs_onschedule_host
    prob = lg_problem(P, "joingraph3", 200, 60, 11, 2, n_data=3)
    st = prob[0]
    packs = [packed_of(P, prob, s) for s in range(3)]
    assert not np.array_equal(packs[0], packs[1])
    multi = from_packed(P, st, np.stack(packs))
    P.regularizebeliefs_onschedule_(multi, all_sites=True)
    got = state(multi)
    for s in range(3):
        one = from_packed(P, st, packs[s])
        _regularizebeliefs_onschedule_host(one)
        ref = state(one)
        for x, y in zip(got, ref):
            assert np.array_equal(x[s], y[0]), s
    multi = from_packed(P, st, np.stack(packs))
    before = state(multi)
    fm, fi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    o = multi._opts()
    assert multi._lib.pgbp_regularize_onschedule(multi._eng, 1, 2, C.byref(o), L.i32p(fm), L.i32p(fi)) == 0
    assert list(fm) == [-1, -1, -1] and list(fi) == [0, 0, 0]
    after = state(multi)
    one = from_packed(P, st, packs[1])
    P.regularizebeliefs_onschedule_(one)
    ref1 = state(one)
    for x0, x1, y in zip(before, after, ref1):
        assert np.array_equal(x0[0], x1[0]) and np.array_equal(x0[2], x1[2])
        assert np.array_equal(x1[1], y[0])


def test_failure_on_one_site(P):
    """one cluster's integrated block negative definite on site 1: the first failing message and info are the host
    walk's, the exception text is identical, and sites 0 and 2 equal their own clean runs"""
    import ctypes as C
    from pgbp_amd import _lib as L
    from pgbp_amd.beliefupdates import BPPosDefException
    from pgbp_amd.regularization import _regularizebeliefs_onschedule_host
    prob = lg_problem(P, "joingraph3", 200, 60, 13, 2, n_data=3)
    st = prob[0]
    packs = [packed_of(P, prob, s) for s in range(3)]
    probe = from_packed(P, st, packs[1])
    nc = probe.nclusters
    # a cluster in the middle of the walk with a variable outside the scopes of its sepsets to later neighbours (no eps
    # lands there: every message it sends integrates that -1e6 out)
    later = {}
    for k in range(probe.nsepsets):
        a, b = (int(x) for x in probe._sepcl[k])
        side = 0 if a < b else 1
        later.setdefault(min(a, b), set()).update(
            int(x) for x in probe._scope_idx[probe._scope_off[2 * k + side]: probe._scope_off[2 * k + side + 1]])
    c = min(c for c, sc in later.items() if c > nc // 3 and len(sc) < int(st.dims[c]))
    m = int(st.dims[c])
    o0 = int(probe._poff[c])
    bad = packs[1].copy()
    bad[o0:o0 + m * m] = (-1e6 * np.eye(m)).reshape(-1)
    one = from_packed(P, st, bad)
    with pytest.raises(BPPosDefException) as ex_host:
        _regularizebeliefs_onschedule_host(one)
    one = from_packed(P, st, bad)
    with pytest.raises(BPPosDefException) as ex_dev:
        P.regularizebeliefs_onschedule_(one)
    assert str(ex_dev.value) == str(ex_host.value) and ex_dev.value.info == ex_host.value.info
    multi = from_packed(P, st, np.stack([packs[0], bad, packs[2]]))
    fm, fi = np.zeros(3, np.int32), np.zeros(3, np.int32)
    opts = multi._opts()
    assert multi._lib.pgbp_regularize_onschedule(multi._eng, 0, 3, C.byref(opts), L.i32p(fm), L.i32p(fi)) == 0
    assert fm[0] == -1 and fm[2] == -1 and fm[1] >= 0 and fi[1] == ex_host.value.info
    k, dr = divmod(int(fm[1]), 2)
    sender = int(multi._sepcl[k][0 if dr == 1 else 1])
    assert sender == c
    assert str(multi._exception_for(sender, k, int(fi[1]))) == str(ex_host.value)
    got = state(multi)
    for s in (0, 2):
        clean = from_packed(P, st, packs[s])
        P.regularizebeliefs_onschedule_(clean)
        ref = state(clean)
        for x, y in zip(got, ref):
            assert np.array_equal(x[s], y[0]), s
    multi = from_packed(P, st, np.stack([packs[0], bad, packs[2]]))
    with pytest.raises(BPPosDefException) as ex_all:
        P.regularizebeliefs_onschedule_(multi, all_sites=True)
    assert str(ex_all.value) == str(ex_host.value)

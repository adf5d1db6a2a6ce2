"""CPU tests (no GPU) of the levelled regularizebeliefs_onschedule! (src/clustergraphbeliefs.jl:376-403) that
pgbp_regularize_onschedule runs on the device: pgbp_plan_onschedule's levels, walk positions and invariants on the
golden Bethe graph, a level-3 join graph, the Mueller clique tree and random networks, and a replay of the levelled
plan with the numpy oracle's primitives -- level by level, phase A then phase B, the tasks of a level in REVERSED
order -- that equals the sequential walk bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import pgbp_amd
from pgbp_amd import _lib as L

from helpers import goldens, make_model, oracle_setup
from oracle import beliefs as OB
from oracle import beliefupdates as BU
from oracle import clustergraph as OCG
from oracle import network as ON

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))


class Graph:
    """description arrays of include/pgbp.h"""

    def __init__(self, dims, sepset_clusters, scope_off, scope_idx):
        self.dims = np.asarray(dims, np.int32)
        self.sepcl = np.asarray(sepset_clusters, np.int32).reshape(-1, 2)
        self.scope_off = np.asarray(scope_off, np.int64)
        self.scope_idx = np.asarray(scope_idx, np.int32)
        self.ns = len(self.scope_off) // 2
        self.nc = len(self.dims) - self.ns

    def scope(self, k, side):
        return self.scope_idx[self.scope_off[2 * k + side]: self.scope_off[2 * k + side + 1]].astype(int)

    def msg(self, k, sender):
        """directed message id of the message `sender` sends through sepset k (2k + dir, dir 1 = received by b)"""
        return 2 * k + (1 if self.sepcl[k][0] == sender else 0)


def graph_of_arrays(st):
    return Graph(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx)


def graph_of_oracle(ocgb):
    nc = ocgb.nclusters
    dims = [b.dimension for b in ocgb.belief]
    sepcl, off, idx = [], [0], []
    for j in range(nc, len(ocgb.belief)):
        a, b = (ocgb.cdict[l] for l in ocgb.belief[j].metadata)
        sepcl.append((a, b))
        for c in (a, b):
            ind = OB.scopeindex(ocgb.belief[j], ocgb.belief[c])
            idx.extend(int(x) for x in ind)
            off.append(off[-1] + len(ind))
    return Graph(dims, sepcl, off, idx)


def plan_onschedule(g):
    lib = pgbp_amd.load()
    desc, keep = L.make_desc(g.dims, g.sepcl, g.scope_off, g.scope_idx, 1, 0)
    pl = C.c_void_p()
    assert lib.pgbp_plan_create(C.byref(desc), C.byref(pl)) == 0, lib.pgbp_plan_last_error(pl)
    try:
        nl = C.c_int32()
        cl = np.zeros(g.nc, np.int32)
        ml = np.zeros(max(1, 2 * g.ns), np.int32)
        wp = np.zeros(max(1, 2 * g.ns), np.int32)
        assert lib.pgbp_plan_onschedule(pl, C.byref(nl), L.i32p(cl), L.i32p(ml), L.i32p(wp)) == 0
        # a second call returns the levelling built at the first one
        nl2 = C.c_int32()
        assert lib.pgbp_plan_onschedule(pl, C.byref(nl2), None, None, None) == 0 and nl2.value == nl.value
    finally:
        lib.pgbp_plan_destroy(pl)
    return nl.value, cl, ml[:2 * g.ns], wp[:2 * g.ns]


def host_walk_order(g):
    """the reference walk's sends, in order: (sender, receiver, sepset), and per cluster the sepsets it edits"""
    nb = [[] for _ in range(g.nc)]
    for k, (a, b) in enumerate(g.sepcl):
        nb[a].append((int(b), k))
        nb[b].append((int(a), k))
    sent, sends, edits = set(), [], [[] for _ in range(g.nc)]
    for ci in range(g.nc):
        tosend = []
        for (nj, k) in nb[ci]:
            if (nj, ci) not in sent:
                edits[ci].append(k)
                sent.add((nj, ci))
            if (ci, nj) not in sent:
                tosend.append((ci, nj, k))
                sent.add((ci, nj))
        sends += tosend
    return sends, edits


# --------------------------------------------------------------------- the walk on plain arrays (oracle primitives)

def random_state(g, rng):
    """cluster beliefs J = B B' + m I, h, g random; sepsets 0 (as after assignfactors!)"""
    bel = []
    for i, m in enumerate(g.dims):
        m = int(m)
        if i < g.nc:
            B = rng.standard_normal((m, m))
            bel.append([B @ B.T + m * np.eye(m), rng.standard_normal(m), np.array([rng.standard_normal()])])
        else:
            bel.append([np.zeros((m, m)), np.zeros(m), np.zeros(1)])
    return bel


def edit(g, bel, ci, k, eps):
    """regularizebeliefs_1clustersepset (src/clustergraphbeliefs.jl:264-275)"""
    side = 0 if g.sepcl[k][0] == ci else 1
    up = g.scope(k, side)
    if up.size == 0:
        return
    J = bel[ci][0]
    J[up, up] += eps
    Js = bel[g.nc + k][0]
    Js[np.diag_indices_from(Js)] += eps


def cluster_eps(bel, ci):
    J = bel[ci][0]
    return max(float(np.max(np.abs(J))) if J.size else 0.0, SQRT_EPS)


def send(g, bel, res, ci, nj, k):
    """propagate_belief!(nj, sepset, ci) with its residual (src/beliefupdates.jl:634-665)"""
    side_f = 0 if g.sepcl[k][0] == ci else 1
    keep, up = g.scope(k, side_f), g.scope(k, 1 - side_f)
    Jf, hf, gf = bel[ci]
    h, J, gg = BU.marginalize(hf, Jf, gf[0], keep, None, ci)
    sep = bel[g.nc + k]
    dh, dJ, dg = BU.divide(sep[1], sep[0], sep[2][0], h, J, gg)
    sep[1] = np.array(h, dtype=float, copy=True)
    sep[0] = np.array(J, dtype=float, copy=True)
    sep[2] = np.array([gg])
    to = bel[nj]
    BU.mult_inplace(to[1], to[0], to[2], up, dh, dJ, dg)
    res[g.msg(k, ci)] = (dh.copy(), dJ.copy())


def sequential_walk(g, bel, res):
    sends, edits = host_walk_order(g)
    by_sender = {}
    for (ci, nj, k) in sends:
        by_sender.setdefault(ci, []).append((nj, k))
    for ci in range(g.nc):
        eps = cluster_eps(bel, ci)
        for k in edits[ci]:
            edit(g, bel, ci, k, eps)
        for (nj, k) in by_sender.get(ci, []):
            send(g, bel, res, ci, nj, k)


def levelled_replay(g, bel, res, n_levels, cluster_level, msg_level, walk_pos):
    """level by level: phase A (the eps of every cluster of the level first, then its edits), then phase B with the
    level's tasks (messages into one receiver, in walk order) in reversed order"""
    sends, edits = host_walk_order(g)
    by_pos = {int(walk_pos[g.msg(k, ci)]): (ci, nj, k) for (ci, nj, k) in sends}
    for L_ in range(n_levels):
        cls = [c for c in range(g.nc) if cluster_level[c] == L_]
        eps = {c: cluster_eps(bel, c) for c in cls}
        for c in reversed(cls):
            for k in edits[c]:
                edit(g, bel, c, k, eps[c])
        tasks = {}
        for pos in sorted(by_pos):
            ci, nj, k = by_pos[pos]
            if msg_level[g.msg(k, ci)] == L_:
                tasks.setdefault(nj, []).append((ci, nj, k))
        for nj in reversed(list(tasks)):
            for (ci, _, k) in tasks[nj]:
                send(g, bel, res, ci, nj, k)


# --------------------------------------------------------------------- checks

def check_levelling(g, n_levels, cluster_level, msg_level, walk_pos):
    sends, _ = host_walk_order(g)
    # every sepset sends exactly one message, from its lower cluster to its higher one
    assert len(sends) == g.ns
    for k, (a, b) in enumerate(g.sepcl):
        lo, hi = min(a, b), max(a, b)
        assert msg_level[g.msg(k, lo)] >= 0 and walk_pos[g.msg(k, lo)] >= 0
        assert msg_level[g.msg(k, hi)] == -1 and walk_pos[g.msg(k, hi)] == -1
    # walk positions = the host walk's order
    for pos, (ci, nj, k) in enumerate(sends):
        assert walk_pos[g.msg(k, ci)] == pos
    last_into, max_in = {}, {}
    for (ci, nj, k) in sends:
        m = g.msg(k, ci)
        assert msg_level[m] >= cluster_level[ci]
        assert cluster_level[nj] > msg_level[m]
        assert msg_level[m] >= last_into.get(nj, -1)   # never decreasing along walk order into a receiver
        assert msg_level[m] == max(cluster_level[ci], last_into.get(nj, -1))   # the tightest level of the rule
        last_into[nj] = msg_level[m]
        max_in[nj] = max(max_in.get(nj, -1), int(msg_level[m]))
    for c in range(g.nc):
        assert cluster_level[c] == 1 + max_in.get(c, -1)
    assert n_levels == (int(cluster_level.max()) + 1 if g.nc else 0)


def check_replay(g, rng, oracle_check=None):
    n_levels, cl, ml, wp = plan_onschedule(g)
    check_levelling(g, n_levels, cl, ml, wp)
    start = random_state(g, rng)
    seq = [[x.copy() for x in b] for b in start]
    rep = [[x.copy() for x in b] for b in start]
    res_seq, res_rep = {}, {}
    sequential_walk(g, seq, res_seq)
    levelled_replay(g, rep, res_rep, n_levels, cl, ml, wp)
    for i in range(len(g.dims)):
        for t in range(3):
            assert np.array_equal(seq[i][t], rep[i][t]), (i, t)
    assert res_seq.keys() == res_rep.keys()
    for m in res_seq:
        assert np.array_equal(res_seq[m][0], res_rep[m][0]) and np.array_equal(res_seq[m][1], res_rep[m][1]), m
    return n_levels


def test_bethe_graph_of_calibration_bethe_level1():
    """the golden Bethe pipeline's graph (test/test_calibration.jl:94-105); the array walk on the oracle's own beliefs is
    oracle/beliefs.py:regularizebeliefs_onschedule bit for bit, and the levelled replay is the walk bit for bit"""
    G = goldens()["calibration_bethe_level1"]
    net = ON.read_newick(G["net"])
    cg = OCG.bethe(net)
    ocgb = oracle_setup(net, cg, make_model(G["model"]), [G["y"]], G["taxa"])
    g = graph_of_oracle(ocgb)
    n_levels, cl, ml, wp = plan_onschedule(g)
    check_levelling(g, n_levels, cl, ml, wp)
    assert n_levels == 2
    bel = [[b.J.copy(), b.h.copy(), b.g.copy()] for b in ocgb.belief]
    rep = [[x.copy() for x in b] for b in bel]
    res = {}
    sequential_walk(g, bel, res)
    levelled_replay(g, rep, {}, n_levels, cl, ml, wp)
    OB.regularizebeliefs_onschedule(ocgb)
    for i, b in enumerate(ocgb.belief):
        assert np.array_equal(bel[i][0], b.J) and np.array_equal(bel[i][1], b.h) and np.array_equal(bel[i][2], b.g), i
        assert np.array_equal(rep[i][0], b.J) and np.array_equal(rep[i][1], b.h) and np.array_equal(rep[i][2], b.g), i
    check_replay(g, np.random.default_rng(1))


def test_level3_join_graph():
    rng = np.random.default_rng(3)
    net = pgbp_amd.random_level3_network_varied(300, 80, rng, n_colors=2)
    cn, ed, sn = pgbp_amd.joingraph(net.node2family, 3)
    assert len(ed) > len(cn) - 1
    st = pgbp_amd.allocate_scopes(cn, ed, sn, net, 2)
    n_levels = check_replay(graph_of_arrays(st), rng)
    assert 2 <= n_levels <= 64


def test_muller_clique_tree():
    path = os.path.join(ROOT, "tests", "golden", "muller_2022.phy")
    net, _ = pgbp_amd.read_newick(open(path).read())
    cn, ed, sn = pgbp_amd.cliquetree(net.node2family)
    assert len(cn) == 664
    st = pgbp_amd.allocate_scopes(cn, ed, sn, net, 1)
    check_replay(graph_of_arrays(st), np.random.default_rng(4))


@pytest.mark.parametrize("seed", range(20))
def test_random_networks(seed):
    rng = np.random.default_rng(100 + seed)
    ntips = int(rng.integers(8, 120))
    net = (pgbp_amd.random_level3_network(ntips, int(rng.integers(1, 6)), rng, n_colors=2) if seed % 2 else
           pgbp_amd.random_level3_network_varied(ntips, max(1, ntips // int(rng.integers(3, 9))), rng, n_colors=2))
    graph = ["cliquetree", "bethe", "joingraph3", "joingraph4"][seed % 4]
    if graph == "cliquetree":
        cn, ed, sn = pgbp_amd.cliquetree(net.node2family)
    elif graph == "bethe":
        cn, ed, sn = pgbp_amd.bethe(net.node2family)
    else:
        cn, ed, sn = pgbp_amd.joingraph(net.node2family, int(graph[-1]))
    st = pgbp_amd.allocate_scopes(cn, ed, sn, net, int(rng.integers(1, 4)))
    check_replay(graph_of_arrays(st), rng)


def test_cfg5_join_graph_level_count(capsys):
    """the cfg5-size join graph (20 000 tips, 5 000 reticulations in varied level-3 blobs, clusters of at most 3 nodes,
    the seed of test_gpu_parity.py's cfg5 test): the walk of 50 000 messages in a few dozen levels"""
    rng = np.random.default_rng(5)
    net = pgbp_amd.random_level3_network_varied(20000, 5001, rng, n_colors=3)
    cn, ed, sn = pgbp_amd.joingraph(net.node2family, 3)
    st = pgbp_amd.allocate_scopes(cn, ed, sn, net, 4)
    g = graph_of_arrays(st)
    n_levels, cl, ml, wp = plan_onschedule(g)
    check_levelling(g, n_levels, cl, ml, wp)
    with capsys.disabled():
        print(f"\ncfg5 join graph: {g.nc} clusters, {g.ns} messages, {n_levels} levels")
    assert n_levels <= 64

#!/usr/bin/env python3
"""Timing of regularizebeliefs_onschedule! (src/clustergraphbeliefs.jl:343-403) on the cfg5-size join graph (20 000 tips,
5 000 reticulations in varied level-3 blobs, clusters of at most 3 nodes, p = 4, seed 5 as test_gpu_parity.py's cfg5
test): the host walk (one pgbp_propagate per message, get / set round trips per edited belief) against the device call
(pgbp_regularize_onschedule: the walk levelled by pgbp_plan_onschedule), both from the same filled engine state.
  python tools/time_regularize.py        one JSON line: host-walk seconds, device seconds (first call: levelling + upload
                                         included; then a steady call), levels, launches, bitwise equality of the two"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pgbp_amd as P  # noqa: E402
from pgbp_amd import _lib as L  # noqa: E402
from pgbp_amd.regularization import _regularizebeliefs_onschedule_host  # noqa: E402


def launches(st, n_levels, cluster_level, msg_level, walk_pos):
    """kernel launches of one device call: per level one phase-A launch (if any cluster of the level edits a sepset) and
    per round of its tasks one launch per kernel instance (csrc/pgbp_plan.cpp: plan_onschedule)"""
    dims = np.asarray(st.dims)
    sepcl = np.asarray(st.sepset_clusters).reshape(-1, 2)
    nc = len(dims) - len(sepcl)
    lo = sepcl.min(axis=1)
    edits = np.zeros(n_levels, bool)
    for k in range(len(sepcl)):
        if dims[nc + k] > 0:
            edits[cluster_level[lo[k]]] = True
    tasks = [dict() for _ in range(n_levels)]
    for m in np.argsort(np.where(walk_pos >= 0, walk_pos, 1 << 30))[: int((walk_pos >= 0).sum())]:
        k, d = divmod(int(m), 2)
        to, frm = (sepcl[k][0], sepcl[k][1]) if d == 0 else (sepcl[k][1], sepcl[k][0])
        mf, mt = int(dims[frm]), int(dims[to])
        kind = 0 if mf <= 64 and mt <= 254 else (2 if mf > 128 else 1)
        runs = tasks[msg_level[m]].setdefault(int(to), [])
        if not runs or runs[-1] != kind:
            runs.append(kind)
    n = int(edits.sum())
    for lev in tasks:
        rounds = max((len(r) for r in lev.values()), default=0)
        n += sum(len({r[i] for r in lev.values() if i < len(r)}) for i in range(rounds))
    return n


def main():
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
    lib = P.load()
    desc, keep = L.make_desc(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, 1, 0)
    pl = C.c_void_p()
    assert lib.pgbp_plan_create(C.byref(desc), C.byref(pl)) == 0
    nm = len(st.scope_off) - 1
    nl = C.c_int32()
    cl = np.zeros(len(cn), np.int32)
    ml, wp = np.zeros(nm, np.int32), np.zeros(nm, np.int32)
    t0 = time.perf_counter()
    assert lib.pgbp_plan_onschedule(pl, C.byref(nl), L.i32p(cl), L.i32p(ml), L.i32p(wp)) == 0
    t_level = time.perf_counter() - t0
    lib.pgbp_plan_destroy(pl)

    def make():
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
        cgb.lg_setup(fam, X)
        cgb.assignfactors_lg_(rates, mu)
        lib.pgbp_sync(cgb._eng)
        return cgb

    h = make()
    t0 = time.perf_counter()
    _regularizebeliefs_onschedule_host(h)
    t_host = time.perf_counter() - t0
    d = make()
    t0 = time.perf_counter()
    P.regularizebeliefs_onschedule_(d)
    t_first = time.perf_counter() - t0
    h.pull()
    d.pull()
    same = bool(np.array_equal(h._packed_raw, d._packed_raw) and np.array_equal(h._res, d._res)
                and np.array_equal(h._flg, d._flg))
    d2 = make()
    fm, fi = np.zeros(1, np.int32), np.zeros(1, np.int32)
    o = d2._opts()
    assert lib.pgbp_regularize_onschedule(d2._eng, 0, 1, C.byref(o), L.i32p(fm), L.i32p(fi)) == 0   # levelling + upload
    d2.init_beliefs_reset_fromfactors_()
    lib.pgbp_sync(d2._eng)
    t0 = time.perf_counter()
    assert lib.pgbp_regularize_onschedule(d2._eng, 0, 1, C.byref(o), L.i32p(fm), L.i32p(fi)) == 0
    t_dev = time.perf_counter() - t0
    print(json.dumps({
        "workload": "cfg5 join graph (20000 tips, 5001 reticulations, joingraph 3, p=4, seed 5)",
        "clusters": int(len(cn)), "messages": int((wp >= 0).sum()), "levels": int(nl.value),
        "launches": launches(st, nl.value, cl, ml, wp),
        "host_walk_s": round(t_host, 3), "device_first_s": round(t_first, 4), "device_s": round(t_dev, 5),
        "levelling_s": round(t_level, 4), "bitwise_equal": same}))


if __name__ == "__main__":
    main()

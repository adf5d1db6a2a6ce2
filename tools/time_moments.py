"""Times pgbp_moments against the one-belief route, and calibrate_exact_cliquetree_ against one calibrate_.

(a) pgbp_moments with and without the covariance over ALL clusters of cfg3 (50 000-tip tree, 16 traits, clique tree, seed 3)
    and of cfg2 (10 000 tips, 8 traits, Bethe graph, seed 2), against a loop of pgbp_integrate over a fixed sample of 1 000
    clusters -- reported per belief, the sample's figure is not extrapolated.
(b) calibrate_exact_cliquetree_ end to end against one calibrate_ of the same engine, on an improper-root clique tree
    (--exact-tips tips, 16 traits) and on a univariate batch (--exact-sites sites).
Wall time around synchronous calls (each returns after its own stream synchronisation), warm-up first, median of the
repetitions, minimum alongside.  Prints one JSON line; profiles/ keeps it, stamped with the hash of csrc/."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import pgbp_amd as P  # noqa: E402
from pgbp_amd import synth as S  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)), "reps": reps}


def moments_block(name, prob, packed, reps):
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, packed)
    assert P.calibrate_(cgb, prob.schedule, 1)[0]
    lib, eng, nc = cgb._lib, cgb._eng, cgb.nclusters
    out = {"workload": name, "clusters": nc, "max_dim": int(max(prob.dims[:nc]))}
    for cov in (1, 0):
        per = int(lib.pgbp_moments_size(eng, 0, None, cov))
        buf, info = np.zeros(per), np.zeros(nc, np.int32)

        def call():
            assert lib.pgbp_moments(eng, 0, None, 0, 1, cov, buf.ctypes.data_as(C.POINTER(C.c_double)),
                                    info.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        r = timed(call, reps)
        r["us_per_belief"] = 1e3 * r["median_ms"] / nc
        r["output_MB"] = per * 8 / 1e6
        out["moments_cov" if cov else "moments_nocov"] = r
    sample = np.random.default_rng(1).choice(nc, size=min(1000, nc), replace=False)
    mu, norm, inf = np.zeros(int(max(prob.dims))), np.zeros(1), np.zeros(1, np.int32)

    def loop():
        for b in sample:
            lib.pgbp_integrate(eng, int(b), mu.ctypes.data_as(C.POINTER(C.c_double)), norm.ctypes.data_as(C.POINTER(C.c_double)),
                               inf.ctypes.data_as(C.POINTER(C.c_int32)))
    r = timed(loop, max(3, reps // 4), warm=1)
    r["beliefs_in_sample"] = int(sample.size)
    r["us_per_belief"] = 1e3 * r["median_ms"] / sample.size
    out["integrate_loop_sample"] = r
    return out


def exact_block(name, ntips, p, ns, reps):
    rng = np.random.default_rng(7)
    tr = S.random_tree(ntips, rng)
    names = [f"n{i}" for i in range(tr.nnodes)]
    taxa = [names[i] for i in range(tr.nnodes) if tr.is_leaf[i]]
    net, nm = P.read_newick(tr.newick(names))
    row = {t: r for r, t in enumerate(taxa)}
    data_row = [row.get(nm[i], -1) for i in range(net.nnodes)]
    cn, ed, sn = P.cliquetree(net.node2family)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    leaf = np.asarray(tr.is_leaf, bool)
    data = np.stack([S.simulate_bm(tr, S.random_rate_matrix(p, rng), np.zeros(p), rng)[leaf] for _ in range(ns)])
    engines = []
    for fixedroot in (False, True):
        st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=fixedroot)
        fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, data_row, p)
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=ns)
        cgb.lg_setup(fam, data if ns > 1 else data[0])
        engines.append((st, cgb))
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    st, free = engines[0]
    ci = next(i for i, c in enumerate(cn) if 1 in c and st.dims[i] > 0)
    root = (ci, int(st.dims[ci]) - p)
    out = {"workload": name, "tips": ntips, "traits": p, "sites": ns, "clusters": len(cn)}
    out["exact_end_to_end"] = timed(lambda: P.calibrate_exact_cliquetree_(free, spt, root, engines[1][1], all_sites=ns > 1), reps)
    out["exact_without_score"] = timed(lambda: P.calibrate_exact_cliquetree_(free, spt, root, None, all_sites=ns > 1), reps)
    out["family_sweep_alone"] = timed(lambda: P.bm_exact_stats(free, all_sites=ns > 1), reps)
    out["one_calibrate"] = timed(lambda: P.calibrate_(free, [spt]), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--exact-tips", type=int, default=5000)
    ap.add_argument("--exact-sites", type=int, default=256)
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_moments.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    rng = np.random.default_rng(3)
    tr = S.random_tree(50000, rng)
    R = S.random_rate_matrix(16, rng)
    prob = S.cliquetree_of_tree(tr, 16)
    res["blocks"].append(moments_block("cfg3: 50000-tip tree, 16 traits, clique tree, seed 3", prob,
                                       S.bm_factors_cliquetree(tr, prob, R, np.zeros(16), S.simulate_bm(tr, R, np.zeros(16), rng)), a.reps))
    rng = np.random.default_rng(2)
    tr = S.random_tree(10000, rng)
    R = S.random_rate_matrix(8, rng)
    prob = S.bethe_of_tree(tr, 8)
    res["blocks"].append(moments_block("cfg2: 10000-tip tree, 8 traits, Bethe graph, seed 2", prob,
                                       S.bm_factors_bethe(tr, prob, R, np.zeros(8), S.simulate_bm(tr, R, np.zeros(8), rng)), a.reps))
    res["blocks"].append(exact_block("improper-root clique tree, 16 traits", a.exact_tips, 16, 1, max(5, a.reps // 2)))
    res["blocks"].append(exact_block("univariate batch on one tree", 2000, 1, a.exact_sites, max(5, a.reps // 2)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Times the scan of every edge for a mean shift (pgbp_lg_shift_scan) next to the edge sweep (pgbp_lg_edge_gradient) on the same
engine, and next to what the scan replaces: one one-edge fit_shifts_lg (p + 2 fills, calibrations and edge sweeps) per edge.

Per workload, on one GPU, wall time around synchronous calls (each returns after its own stream synchronisation), warm-up
first, median of the repetitions with the minimum alongside:
  scan_alone               shift_scan_lg on calibrated beliefs: jump, lr and identified of every family (sweep + fetch + the
                           host's edge_jump)
  scan_with_information    the same with information=True (H of every family comes back and se is formed on the host)
  edge_sweep_alone         edge_gradient_lg on the same beliefs: the yardstick
  ratio                    scan_alone / edge_sweep_alone (medians)
  one_edge_fit             fit_shifts_lg of ONE edge, once (p + 2 evaluations)
  all_edges_by_fits_s      one_edge_fit x the number of edges, in seconds: what the scan's answer costs without it (not run)
Workloads, those of tools/time_edge_gradient.py: (a) 5 000-tip tree, 16 traits, clique tree, full BM; (b) cfg3: 50 000 tips, 16
traits; (c) the cfg5-size level-3 network's clique tree, 4 traits, 3 rates.  Nothing is asserted on the times.  Prints one JSON
line per finished block and the whole result last; with --out it is also written there (profiles/r13_time_shift_scan.json),
stamped with the hash of csrc/."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import pgbp_amd as P  # noqa: E402
from time_gradient import timed, tree_engine  # noqa: E402


def measure(name, cgb, spt, assign, fam, reps, extra):
    """assign(): assignfactors_lg_ with the workload's parameters."""
    t0 = time.perf_counter()
    cgb.set_schedule([spt])
    assign()
    ll, sc = cgb.loglik_and_shift_scan_lg(spt, all_sites=True)   # (leaves calibrated beliefs for both sweeps)
    assert not sc["info"].any() and np.all(np.isfinite(ll)), name
    n_par = np.asarray(fam["n_parents"])
    p = int(cgb._lg_p)
    out = dict(workload=name, sites=int(cgb.n_sites), clusters=int(cgb.nclusters), families=int(len(n_par)),
               edges=int(n_par.sum()), families_fully_identified=int(np.sum(sc["dof"][0] == p)),
               families_partly_identified=int(np.sum((sc["dof"][0] > 0) & (sc["dof"][0] < p))), **extra)
    out["first_call_s"] = time.perf_counter() - t0
    out["scan_alone"] = timed(lambda: cgb.shift_scan_lg(all_sites=True), reps)
    out["scan_with_information"] = timed(lambda: cgb.shift_scan_lg(all_sites=True, information=True), reps)
    out["edge_sweep_alone"] = timed(lambda: cgb.edge_gradient_lg(all_sites=True), reps)
    out["ratio"] = out["scan_alone"]["median_ms"] / out["edge_sweep_alone"]["median_ms"]
    f = int(np.nanargmax(np.where(sc["dof"][0] == p, sc["lr"][0], -1.0)))
    t1 = time.perf_counter()
    fit = P.fit_shifts_lg(cgb, spt, [(f, 0)])
    ms = 1e3 * (time.perf_counter() - t1)
    K = cgb._lg["length"].size // len(n_par)
    gam = float(np.asarray(cgb._lg["gamma"]).reshape(-1, K)[f, 0])
    out["one_edge_fit"] = dict(ms=ms, evaluations=p + 2, family=f,
                               scan_vs_fit_shift=float(np.max(np.abs(sc["edge_jump"][0, f, 0] - fit["shifts"][0]))
                                                       / np.max(np.abs(fit["shifts"][0]))),
                               scan_vs_fit_gain=float(abs(sc["lr"][0, f] - 2.0 * (fit["loglik"] - ll[0])) / sc["lr"][0, f]),
                               gamma=gam)
    out["all_edges_by_fits_s"] = 1e-3 * ms * out["edges"]
    cgb.clear_shifts_lg()
    return out


def bm_tree_block(name, ntips, seed, reps):
    p = 16
    cgb, spt, R, rng, nf = tree_engine(ntips, p, 1, seed)
    mu = np.zeros(p)
    return measure(name, cgb, spt, lambda: cgb.assignfactors_lg_(R[None], mu), cgb._lg, reps, dict(tips=ntips, traits=p))


def network_block(reps):
    a = types.SimpleNamespace(seed=5, traits=4, blob_style="template", ntips=20000, blobs=20000 // 12, graph="cliquetree",
                              maxclustersize=3)
    net, (cn, ed, sn), st, fam, X, rates, mu, _ = bench.build_network_workload(a, 0)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(fam, X)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    return measure("cfg5-size level-3 network (20000 tips, 5001 reticulations), clique tree, 4 traits, 3 rates", cgb, spt,
                   lambda: cgb.assignfactors_lg_(rates, mu), cgb._lg, reps, dict(tips=20000, traits=4, max_dim=int(max(st.dims))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_shift_scan.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [lambda: bm_tree_block("5000-tip tree, 16 traits, clique tree, fixed root, seed 7", 5000, 7, a.reps),
            lambda: network_block(a.reps)]
    if not a.skip_cfg3:
        jobs.append(lambda: bm_tree_block("cfg3: 50000-tip tree, 16 traits, clique tree, fixed root, seed 3", 50000, 3, a.reps))
    for job in jobs:
        res["blocks"].append(job())
        print(json.dumps(res["blocks"][-1]), flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

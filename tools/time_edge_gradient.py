"""Times the per-edge sweep (pgbp_lg_edge_gradient) next to the parameter gradient (pgbp_lg_gradient) on the same engine: the
same solve of every family's cluster, here without the slot pool and its reduction, but with K + K + p numbers per family
coming back to the host instead of one gradient per site.

Per workload, on one GPU, wall time around synchronous calls (each returns after its own stream synchronisation), warm-up
first, median of the repetitions with the minimum alongside:
  edge_sweep_alone         edge_gradient_lg on calibrated beliefs (the family sweep and the fetch of its outputs)
  gradient_sweep_alone     gradient_lg on the same beliefs: the yardstick
  ratio                    edge_sweep_alone / gradient_sweep_alone (medians)
  set_edges                set_edges_lg with every length and inheritance (what a step in the edges costs before the next fill)
Workloads, those of tools/time_gradient.py: (a) 5 000-tip tree, 16 traits, clique tree, full BM; (b) cfg3: 50 000 tips, 16
traits; (c) the cfg5-size level-3 network's clique tree, 4 traits, 3 rates.  Nothing is asserted on the times.  Prints one JSON
line per finished block and the whole result last; with --out it is also written there (profiles/r10_time_edge_gradient.json),
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
    ll, g = cgb.loglik_and_edge_gradient_lg(spt, all_sites=True)   # (leaves calibrated beliefs for both sweeps)
    assert not g["info"].any() and np.all(np.isfinite(ll)), name
    n_par = np.asarray(fam["n_parents"])
    real = np.arange(g["dlength"].shape[2])[None, :] < n_par[:, None]
    assert np.all(np.isfinite(g["dlength"][0][real])) and np.all(np.isnan(g["dlength"][0][~real])), name
    out = dict(workload=name, sites=int(cgb.n_sites), clusters=int(cgb.nclusters), families=int(len(n_par)),
               K=int(g["dlength"].shape[2]), output_MB=sum(g[k].nbytes for k in ("dlength", "dgamma", "dshift")) / 1e6, **extra)
    out["first_call_s"] = time.perf_counter() - t0
    out["edge_sweep_alone"] = timed(lambda: cgb.edge_gradient_lg(all_sites=True), reps)
    out["gradient_sweep_alone"] = timed(lambda: cgb.gradient_lg(all_sites=True), reps)
    out["ratio"] = out["edge_sweep_alone"]["median_ms"] / out["gradient_sweep_alone"]["median_ms"]
    out["set_edges"] = timed(lambda: cgb.set_edges_lg(length=fam["length"], gamma=fam["gamma"]), reps)
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
    res = {"tool": "tools/time_edge_gradient.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
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

"""Times the leave-one-out sweep (pgbp_lg_loo) next to the calls it sits beside and against what it replaces: one engine per
tip with that tip's values masked, factor fill + postorder + root integrate (loglik_lg) each.

Per workload, on one GPU, wall time around synchronous calls (each returns after its own stream synchronisation), warm-up
first, median of the repetitions with the minimum alongside:
  loo_sweep         loo_lg on calibrated beliefs (the sweep over the tip families, the total and the fetch)
  gradient_sweep    gradient_lg on the same beliefs
  calibrate         calibrate_ (postorder + preorder of the clique tree)
  brute_force       per masked tip: build the family table and an engine without that tip's values, assignfactors_lg_,
                    loglik_lg -- timed on a sample of 20 tips, extrapolated to all tips (extrapolated_s)
Workloads: cfg3 (50 000 tips, 16 traits), a 5 000-tip tree with 16 traits, the cfg5-size level-3 network's clique tree
(4 traits, 3 rates).  Prints one JSON line per finished block; --out writes the whole result (profiles/r09_time_loo.json),
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import pgbp_amd as P  # noqa: E402
from pgbp_amd import synth as S  # noqa: E402
from time_gradient import timed  # noqa: E402


def measure(name, build, assign_args, reps, n_brute, extra):
    """build(mask_row) -> (engine with the family table set, schedule tree, number of tips); mask_row: a data row whose values
    are missing (None: complete data)."""
    cgb, spt, ntips = build(None)
    cgb.set_schedule([spt])
    cgb.assignfactors_lg_(*assign_args)
    ll, d = cgb.loo_and_loglik_lg(spt, all_sites=True)
    assert not d["info"].any() and np.all(np.isfinite(d["lpd"])), name
    out = dict(workload=name, tips=int(ntips), tip_families=int(d["lpd"].shape[1]), clusters=int(cgb.nclusters), **extra)
    out["loo_sweep"] = timed(lambda: cgb.loo_lg(all_sites=True), reps)
    out["gradient_sweep"] = timed(lambda: cgb.gradient_lg(all_sites=True), reps)

    def calibrate():
        cgb.assignfactors_lg_(*assign_args)
        P.calibrate_(cgb, [spt], 1, sync=False)
    out["calibrate"] = timed(calibrate, reps)
    rows = np.random.default_rng(0).choice(d["lpd"].shape[1], n_brute, replace=False)
    ts, worst = [], 0.0
    for ti in rows:
        row = int(cgb._lg["data_row"][d["families"][ti]])
        t0 = time.perf_counter()
        one, spt1, _ = build(row)
        one.set_schedule([spt1])
        one.assignfactors_lg_(*assign_args)
        ll1, info = one.loglik_lg()
        ts.append(time.perf_counter() - t0)
        worst = max(worst, abs((ll[0] - ll1[0]) - d["lpd"][0, ti]) / max(1.0, abs(d["lpd"][0, ti])))
        del one
    out["brute_force"] = {"median_ms_per_tip": 1e3 * float(np.median(ts)), "min_ms_per_tip": 1e3 * float(np.min(ts)),
                          "sampled_tips": int(n_brute), "extrapolated_s": float(np.median(ts)) * d["lpd"].shape[1],
                          "worst_lpd_disagreement": worst}
    out["ratio_brute_force_to_sweep"] = 1e3 * out["brute_force"]["extrapolated_s"] / out["loo_sweep"]["median_ms"]
    return out


def tree_block(name, ntips, seed, reps, n_brute):
    p = 16
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    names = [f"n{i}" for i in range(tr.nnodes)]
    taxa = [names[i] for i in range(tr.nnodes) if tr.is_leaf[i]]
    net, nm = P.read_newick(tr.newick(names))
    row = {t: r for r, t in enumerate(taxa)}
    data_row = [row.get(nm[i], -1) for i in range(net.nnodes)]
    cn, ed, sn = P.cliquetree(net.node2family)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    R = S.random_rate_matrix(p, rng)
    R = (R + R.T) / 2
    data = S.simulate_bm(tr, R, np.zeros(p), rng)[np.asarray(tr.is_leaf, bool)]
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=True)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))

    def build(mask_row):
        x = data
        if mask_row is not None:
            x = data.copy()
            x[mask_row] = np.nan
        fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, data_row, p,
                            data=None if mask_row is None else x)
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
        cgb.lg_setup(fam, x)
        return cgb, spt, len(taxa)
    return measure(name, build, (R[None], np.zeros(p)), reps, n_brute, dict(traits=p))


def network_block(reps, n_brute):
    a = types.SimpleNamespace(seed=5, traits=4, blob_style="template", ntips=20000, blobs=20000 // 12, graph="cliquetree",
                              maxclustersize=3)
    net, (cn, ed, sn), st, fam0, X, rates, mu, _ = bench.build_network_workload(a, 0)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    ntips = int(np.sum(net.is_leaf))

    def build(mask_row):
        fam, x = fam0, X
        if mask_row is not None:      # the family table again with that tip's mask empty (the fill skips the family)
            x = X.copy()
            x[mask_row] = np.nan
            fam = dict(fam0)
            nf, K = len(fam0["cluster"]), max(1, int(fam0["max_parents"]))
            full = np.uint64((1 << 4) - 1)
            cm = np.full(nf, full, np.uint64) if fam0.get("child_mask") is None else fam0["child_mask"].copy()
            cm[(fam0["child_pos"] < 0) & (fam0["data_row"] == mask_row)] = 0
            fam["child_mask"] = cm
            fam["parent_mask"] = np.full(nf * K, full, np.uint64) if fam0.get("parent_mask") is None else fam0["parent_mask"]
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
        cgb.lg_setup(fam, x)
        return cgb, spt, ntips
    return measure("cfg5-size level-3 network (20000 tips, 5001 reticulations), clique tree, 4 traits, 3 rates", build,
                   (rates, mu), reps, n_brute, dict(traits=4, max_dim=int(max(st.dims))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--brute-tips", type=int, default=20)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_loo.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [lambda: tree_block("5000-tip tree, 16 traits, clique tree, fixed root, seed 7", 5000, 7, a.reps, a.brute_tips),
            lambda: network_block(a.reps, a.brute_tips)]
    if not a.skip_cfg3:
        jobs.append(lambda: tree_block("cfg3: 50000-tip tree, 16 traits, clique tree, fixed root, seed 3", 50000, 3, a.reps,
                                       a.brute_tips))
    for job in jobs:
        res["blocks"].append(job())
        print(json.dumps(res["blocks"][-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

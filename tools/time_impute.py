"""Times the imputation sweep (pgbp_lg_impute) against what a user had to do before it: moments_ of the clusters of the tips
that miss a value (mean and covariance across the bus), then the conditioning algebra in numpy on the host, tip by tip.

Per workload, on one GPU, wall time around synchronous calls (each returns after its own stream synchronisation), warm-up
first, median of the repetitions with the minimum alongside:
  impute_sweep      impute_lg on calibrated beliefs (the sweep over the listed tip families and the fetch)
  host_route        moments_(clusters of the listed tips) + the numpy conditioning of every listed tip (--host-reps runs)
  loo_sweep         loo_lg on the same beliefs, for scale
  calibrate         assignfactors_lg_ + calibrate_ (postorder + preorder of the clique tree)
Workloads: the 5 000-tip tree with 16 traits and cfg3 (50 000 tips, 16 traits), 10 % of the entries masked at random (fixed
root: every internal node keeps its full scope, every missing entry is predicted).  The two routes are compared entry by
entry (worst_disagreement, relative to the largest entry of a block).  Prints one JSON line per finished block; --out writes
the whole result (profiles/r11_time_impute.json), stamped with the hash of csrc/."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import pgbp_amd as P  # noqa: E402
from pgbp_amd import synth as S  # noqa: E402
from time_gradient import timed  # noqa: E402


def host_route(cgb, fam, data, R, mu, listed):
    """The route without the sweep, for a BM on a tree (one parent per tip): (mean [n, p], cov [n, p, p]) of the listed
    families, NaN outside the missing traits."""
    p, K = int(fam["p"]), max(1, int(fam["max_parents"]))
    clusters = fam["cluster"][listed]
    uniq, inv = np.unique(clusters, return_inverse=True)
    mom = cgb.moments_(uniq)
    mean, cov = np.full((len(listed), p), np.nan), np.full((len(listed), p, p), np.nan)
    for i, f in enumerate(listed):
        O = int(fam["child_mask"][f])
        o = [t for t in range(p) if (O >> t) & 1]
        q = [t for t in range(p) if not (O >> t) & 1]
        z = o + q
        no = len(o)
        g, t_ = fam["gamma"][f * K], fam["length"][f * K]
        V = (g * g * t_) * R[np.ix_(z, z)]
        pos = int(fam["parent_pos"][f * K])
        if pos >= 0:
            m, Sg = mom[inv[i]][0], mom[inv[i]][1]
            idx = pos + np.asarray(z)
            eu, Cu = g * m[idx], (g * g) * Sg[np.ix_(idx, idx)]
        else:
            eu, Cu = g * mu[z], np.zeros((p, p))
        B = np.linalg.solve(V[:no, :no], V[:no, no:]).T if no else np.zeros((len(q), 0))
        T = np.hstack([-B, np.eye(len(q))])
        mean[i, q] = eu[no:] + B @ (data[fam["data_row"][f], o] - eu[:no])
        cov[np.ix_([i], q, q)] = T @ Cu @ T.T + V[no:, no:] - B @ V[:no, no:]
    return mean, cov


def tree_block(name, ntips, seed, reps, host_reps, frac=0.1):
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
    mu = np.zeros(p)
    data = S.simulate_bm(tr, R, mu, rng)[np.asarray(tr.is_leaf, bool)]
    data[rng.random(data.shape) < frac] = np.nan
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=True)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, data_row, p, data=data)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(fam, data)
    cgb.set_schedule([spt])
    cgb.assignfactors_lg_(R[None], mu)
    ll, d = cgb.impute_and_loglik_lg(spt)
    assert not d["info"].any() and np.isfinite(ll), name
    assert int(d["predicted"].sum()) == int(np.isnan(data).sum()), name
    out = dict(workload=name, tips=len(taxa), traits=p, masked_fraction=frac, listed_families=int(len(d["families"])),
               predicted_entries=int(d["predicted"].sum()), clusters=int(cgb.nclusters))
    hm, hc = host_route(cgb, fam, data, R, mu, d["families"])
    ok = d["predicted"]
    scale = lambda a: np.nanmax(np.abs(a).reshape(len(a), -1), axis=1)
    out["worst_disagreement"] = float(max(
        np.nanmax(np.abs(np.where(ok, d["mean"] - hm, 0.0)).max(axis=1) / scale(hm)),
        np.nanmax(np.nan_to_num(np.abs(d["cov"] - hc)).reshape(len(hc), -1).max(axis=1) / scale(hc))))
    out["impute_sweep"] = timed(lambda: cgb.impute_lg(), reps)
    out["host_route"] = timed(lambda: host_route(cgb, fam, data, R, mu, d["families"]), host_reps, warm=0)
    out["loo_sweep"] = timed(lambda: cgb.loo_lg(), reps)

    def calibrate():
        cgb.assignfactors_lg_(R[None], mu)
        P.calibrate_(cgb, [spt], 1, sync=False)
    out["calibrate"] = timed(calibrate, reps)
    out["ratio_host_route_to_sweep"] = out["host_route"]["median_ms"] / out["impute_sweep"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_impute.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [lambda: tree_block("5000-tip tree, 16 traits, clique tree, fixed root, seed 7, 10 % masked", 5000, 7, a.reps,
                               a.host_reps)]
    if not a.skip_cfg3:
        jobs.append(lambda: tree_block("cfg3: 50000-tip tree, 16 traits, clique tree, fixed root, seed 3, 10 % masked", 50000,
                                       3, a.reps, a.host_reps))
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

"""Times the lanes-are-sites gradient sweep (pgbp_lg_gradient_sites / gradient_sites_lg) and the per-site fit on top of it
(optimize.fit_sites_lg) on univariate OU batches with per-site parameters:
  * sites256: 256 sites on a 2 000-tip tree (the 0.4 x row of tools/time_gradient.py);
  * cfg4:     a cfg4-size batch, 8 000 sites on a 20 000-tip tree.
Per workload, median and minimum of --reps wall times around the synchronous calls:
  * sweep_sites:             gradient_sites_lg() on calibrated beliefs (no layout conversion);
  * sweep_existing:          gradient_lg(all_sites=True) on the same beliefs, and the calibrate_ step that follows it (the two
                             transpositions it causes on a site-minor engine are inside these two);
  * value_and_gradient_sites / value_and_gradient_existing: assignfactors_lg_ + loglik_and_gradient(_sites)_lg;
  * one_loglik_eval, central_gradient: assignfactors_lg_ + loglik_lg, and 2 n_theta = 8 of them;
  * fit: fit_sites_lg end to end from a neutral start, evaluations and accepted steps per site.
Blocks of the existing sweep that would not finish in --max-existing-s (estimated from one call) are run once only.
Prints one JSON line; profiles/ keeps it, stamped with the hash of csrc/."""
import argparse
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


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)), "reps": reps}


def block(name, ntips, ns, seed, reps, max_existing_s, fit):
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    depth = np.zeros(tr.nnodes)
    for i in range(1, tr.nnodes):
        depth[i] = depth[tr.parent[i]] + tr.length[i]
    H = float(depth[tr.is_leaf].mean())
    al = rng.uniform(1, 3, ns) / H
    g2 = rng.uniform(0.5, 2, ns)
    th = rng.normal(0, 2, ns)
    mu = th + rng.normal(0, 1, ns)
    X = S.simulate_ou_uni_sites(tr, 2 * al * g2, al, th, mu, rng)
    prob = S.cliquetree_of_tree(tr, 1)
    fam = S.lg_tree_table(tr, prob, 1)
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=ns)
    cgb.lg_setup(fam, np.ascontiguousarray(X[:, :, None]))
    spt = prob.schedule[0]
    cgb.set_schedule([spt])
    tipmean = X[:, tr.is_leaf].mean(axis=1)
    del X

    def assign():
        cgb.assignfactors_lg_(g2.reshape(ns, 1, 1, 1), mu[:, None], model="ou", alpha=al, theta=th[:, None])
    out = dict(workload=name, sites=ns, tips=ntips, families=len(fam["cluster"]), n_theta=4)
    assign()
    ll, g = cgb.loglik_and_gradient_sites_lg(spt)
    assert not g["info"].any() and np.all(np.isfinite(ll)), name
    out["layout_after_sweep"] = int(cgb._lib.pgbp_layout(cgb._eng))
    out["sweep_sites"] = timed(cgb.gradient_sites_lg, reps)

    def value_and_gradient_sites():
        assign()
        cgb.loglik_and_gradient_sites_lg(spt)

    def one_eval():
        assign()
        cgb.loglik_lg()
    out["value_and_gradient_sites"] = timed(value_and_gradient_sites, reps)
    out["one_loglik_eval"] = timed(one_eval, reps)
    out["central_gradient"] = {"evaluations": 8, "median_ms": 8 * out["one_loglik_eval"]["median_ms"],
                               "note": "8 x one_loglik_eval"}
    # the existing sweep on the same beliefs: one call first, to size the repetitions
    value_and_gradient_sites()
    t0 = time.perf_counter()
    ref = cgb.gradient_lg(all_sites=True)
    first = time.perf_counter() - t0
    worst = max(float(np.max(np.abs(g[k] - ref[k])) / max(1.0, float(np.max(np.abs(ref[k]))))) for k in ("dR", "dmu", "dalpha", "dtheta"))
    out["worst_block_against_existing"] = worst
    er = reps if first * (reps + 1) * 2 <= max_existing_s else 1

    def existing_and_back():
        cgb.gradient_lg(all_sites=True)
        cgb.loglik_lg()          # (the next traversal: back into the layout of the thread-per-site kernels)

    def value_and_gradient_existing():
        assign()
        cgb.loglik_and_gradient_lg(spt, all_sites=True)
    out["sweep_existing_first_call_ms"] = 1e3 * first
    out["sweep_existing_and_next_loglik"] = timed(existing_and_back, er, warm=0 if er == 1 else 1)
    out["value_and_gradient_existing"] = timed(value_and_gradient_existing, er, warm=0 if er == 1 else 1)
    out["ratio_existing_over_sites"] = out["value_and_gradient_existing"]["median_ms"] / out["value_and_gradient_sites"]["median_ms"]
    out["ratio_central_over_sites"] = out["central_gradient"]["median_ms"] / out["value_and_gradient_sites"]["median_ms"]
    if fit:
        t0 = time.perf_counter()
        f = P.fit_sites_lg(cgb, spt, "ou", np.ones(ns), tipmean, alpha0=np.full(ns, 1.0 / H), theta0=tipmean)
        out["fit"] = dict(seconds=time.perf_counter() - t0, device_evals=int(f["n_device_evals"]),
                          converged=int(f["converged"].sum()), steps_median=float(np.median(f["n_iter"])),
                          steps_max=int(f["n_iter"].max()))   # (every device evaluation covers all sites)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip", nargs="*", default=[], choices=["sites256", "cfg4"])
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--cfg4-sites", type=int, default=8000)
    ap.add_argument("--cfg4-tips", type=int, default=20000)
    ap.add_argument("--max-existing-s", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_time_gradient_sites.json"))
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_gradient_sites.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [("sites256", "256 univariate OU sites on a 2000-tip tree (per-site parameters)", 2000, 256, 9),
            ("cfg4", f"cfg4-size: {a.cfg4_sites} univariate OU sites on a {a.cfg4_tips}-tip tree (per-site parameters)",
             a.cfg4_tips, a.cfg4_sites, 4)]
    for key, name, ntips, ns, seed in jobs:
        if key in a.skip:
            res.setdefault("not_taken", []).append(name)
            continue
        res["blocks"].append(block(name, ntips, ns, seed, a.reps, a.max_existing_s, not a.no_fit))
        print(json.dumps(res["blocks"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

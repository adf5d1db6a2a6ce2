"""Times what painted optima under OU cost (pgbp_lg_set_optima, the displacement correction of csrc/pgbp_shift.hip,
pgbp_lg_gradient_sites_optima, fit_sites_lg(optima0=...)) on univariate OU batches with per-site parameters:
  * sites256: 256 sites on a 2 000-tip tree;
  * cfg4:     a cfg4-size batch, 8 000 sites on a 20 000-tip tree.
Per workload, median and minimum of --reps wall times around the synchronous calls:
  * fill_R / loglik_R:       assignfactors_lg_ and loglik_lg with R = 0, 2, 8 regimes painted on every edge at random (per-site
                             values; the setter is outside the timed call: the values do not move with alpha);
  * explicit_shifts_R:       the same model through per-site explicit shifts, the route before this change: the host recomputes
                             (1 - exp(-alpha t)) (theta_r - theta) for every (site, painted edge), set_shifts_lg uploads them,
                             then assignfactors_lg_ + loglik_lg; skipped, and said so, where the table of n_sites x n_edges
                             doubles would pass --max-shift-gb;
  * sweep_sites / sweep_sites_optima: gradient_sites_lg on calibrated beliefs without and with doptima (2 and 8 regimes);
  * fit: one fit_sites_lg with two painted clades, evaluations and wall time (--no-fit: left out).
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


def clades(tr, want):
    """node regimes with two disjoint clades of about `want` tips painted 1 and 2"""
    size = np.where(tr.is_leaf, 1, 0).astype(np.int64)
    for i in range(tr.nnodes - 1, 0, -1):
        size[tr.parent[i]] += size[i]
    anc = lambda i, j: any(k == j for k in iter_up(tr, i))
    order = sorted(range(1, tr.nnodes), key=lambda i: (abs(int(size[i]) - want), i))
    c1 = order[0]
    c2 = next(i for i in order[1:] if not anc(i, c1) and not anc(c1, i))
    reg = np.zeros(tr.nnodes, np.int32)
    for i in range(1, tr.nnodes):   # (preorder: a parent is painted before its children)
        if i == c1 or reg[tr.parent[i]] == 1:
            reg[i] = 1
        elif i == c2 or reg[tr.parent[i]] == 2:
            reg[i] = 2
    return reg


def iter_up(tr, i):
    while i >= 0:
        yield i
        i = int(tr.parent[i])


def block(name, ntips, ns, seed, reps, fit, max_shift_gb):
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    depth = np.zeros(tr.nnodes)
    for i in range(1, tr.nnodes):
        depth[i] = depth[tr.parent[i]] + tr.length[i]
    H = float(depth[tr.is_leaf].mean())
    al, g2 = rng.uniform(1, 3, ns) / H, rng.uniform(0.5, 2, ns)
    th = rng.normal(0, 2, ns)
    mu = th + rng.normal(0, 1, ns)
    X = S.simulate_ou_uni_sites(tr, 2 * al * g2, al, th, mu, rng)
    prob = S.cliquetree_of_tree(tr, 1)
    fam = S.lg_tree_table(tr, prob, 1)
    nf = len(fam["cluster"])
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=ns)
    cgb.lg_setup(fam, np.ascontiguousarray(X[:, :, None]))
    spt = prob.schedule[0]
    cgb.set_schedule([spt])
    tipmean = X[:, tr.is_leaf].mean(axis=1)
    length = np.asarray(fam["length"], float)

    def assign():
        cgb.assignfactors_lg_(g2.reshape(ns, 1, 1, 1), mu[:, None], model="ou", alpha=al, theta=th[:, None])

    def loglik():
        assign()
        cgb.loglik_lg()
    out = dict(workload=name, sites=ns, tips=ntips, families=nf)
    ref = {}
    for R in (0, 2, 8):
        if R:
            regime = rng.integers(0, R + 1, size=(nf, 1)).astype(np.int32)
            values = th[:, None, None] + rng.normal(0, 2, size=(ns, R, 1))
            cgb.set_optima_lg(regime, values)
        else:
            cgb.clear_optima_lg()
        out[f"fill_{R}"] = timed(assign, reps)
        out[f"loglik_{R}"] = timed(loglik, reps)
        assign()
        ref[R] = cgb.loglik_lg()[0].copy()
        if R:
            out[f"painted_families_{R}"] = int(np.count_nonzero(regime))
            cgb.clear_optima_lg()
            painted = np.flatnonzero(regime[:, 0] > 0)
            gb = ns * painted.size * 8 / 2 ** 30
            if gb > max_shift_gb:
                out[f"explicit_shifts_{R}"] = {"not_taken": f"{ns} x {painted.size} doubles = {gb:.2f} GiB of per-site shifts "
                                                            f"(above --max-shift-gb {max_shift_gb})"}
            else:
                def explicit():
                    sv = (1.0 - np.exp(-al[:, None] * length[painted][None, :])) * \
                        (values[:, regime[painted, 0] - 1, 0] - th[:, None])
                    cgb.set_shifts_lg(np.stack([painted, np.zeros_like(painted)], axis=1), sv[:, :, None])
                    assign()
                    cgb.loglik_lg()
                out[f"explicit_shifts_{R}"] = timed(explicit, reps)
                explicit()
                ll = cgb.loglik_lg()[0]
                out[f"explicit_vs_painted_{R}"] = float(np.max(np.abs(ll - ref[R]) / np.maximum(1.0, np.abs(ref[R]))))
                cgb.clear_shifts_lg()
            cgb.set_optima_lg(regime, values)
            assign()
            ll, g = cgb.loglik_and_gradient_sites_lg(spt)
            assert not g["info"].any() and "doptima" in g
            out[f"sweep_sites_optima_{R}"] = timed(cgb.gradient_sites_lg, reps)
        else:
            ll, g = cgb.loglik_and_gradient_sites_lg(spt)
            assert not g["info"].any() and "doptima" not in g
            out["sweep_sites"] = timed(cgb.gradient_sites_lg, reps)
    cgb.clear_optima_lg()
    if fit:
        cgb.set_optima_lg(clades(tr, max(10, ntips // 8))[1:, None], np.zeros((2, 1)))
        t0 = time.perf_counter()
        f = P.fit_sites_lg(cgb, spt, "ou", np.ones(ns), mu, alpha0=np.full(ns, 1.0 / H), theta0=tipmean, fit_mu=False,
                           optima0=np.stack([tipmean, tipmean], axis=1))
        out["fit_two_optima"] = dict(seconds=time.perf_counter() - t0, device_evals=int(f["n_device_evals"]),
                                     converged=int(f["converged"].sum()), steps_median=float(np.median(f["n_iter"])),
                                     steps_max=int(f["n_iter"].max()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip", nargs="*", default=[], choices=["sites256", "cfg4"])
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--cfg4-sites", type=int, default=8000)
    ap.add_argument("--cfg4-tips", type=int, default=20000)
    ap.add_argument("--max-shift-gb", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_time_optima.json"))
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_optima.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [("sites256", "256 univariate OU sites on a 2000-tip tree (per-site parameters)", 2000, 256, 9),
            ("cfg4", f"cfg4-size: {a.cfg4_sites} univariate OU sites on a {a.cfg4_tips}-tip tree (per-site parameters)",
             a.cfg4_tips, a.cfg4_sites, 4)]
    for key, name, ntips, ns, seed in jobs:
        if key in a.skip:
            res.setdefault("not_taken", []).append(name)
            continue
        res["blocks"].append(block(name, ntips, ns, seed, a.reps, not a.no_fit, a.max_shift_gb))
        print(json.dumps(res["blocks"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

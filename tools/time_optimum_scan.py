"""Times the optimum-shift scan of a univariate batch (pgbp_lg_optimum_scan_sites) on univariate OU batches with per-site
parameters:
  * sites256: 256 sites on a 2 000-tip tree;
  * cfg4:     a cfg4-size batch, 8 000 sites on a 20 000-tip tree.  Four state rows x 39 998 families x 256 sites are 328 MB,
              above the 256 MB default of pgbp_sites_sweep_scratch_limit: the tool raises the limit for this block
              (--cfg4-limit doubles) and restores the default afterwards.
Per workload, median and minimum of --reps wall times around the synchronous C calls, outputs allocated beforehand:
  * optimum_top / optimum_tables: the scan with tables=False (top_lr, top_family, info) and with delta and lr;
  * phases_*: milliseconds per phase from the _timed twin (validity, the height launches with their count, the fold, the
    copies), the median over the repetitions;
  * shift_scan_top / shift_scan_tables: pgbp_lg_shift_scan_sites on the same beliefs -- the neighbouring sweep, one launch for
    all families, the yardstick for the levelled launches;
  * by_hand: the route before -- for an edge, paint its clade (add_optimum_shift, set_optima_lg) and take two loglik_lg --
    timed for --hand-edges edges and EXTRAPOLATED to all of them (by_hand_all_edges_s is that extrapolation, not a
    measurement).
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
from pgbp_amd import _lib as L  # noqa: E402
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


def ok(cgb, rc):
    assert rc == L.PGBP_OK, cgb._lib.pgbp_last_error(cgb._eng)


def block(name, ntips, ns, seed, reps, limit, hand_edges):
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
    del X
    spt = prob.schedule[0]
    cgb.set_schedule([spt])
    cgb.assignfactors_lg_(g2.reshape(ns, 1, 1, 1), mu[:, None], model="ou", alpha=al, theta=th[:, None])
    lib, eng = cgb._lib, cgb._eng
    nf = len(fam["cluster"])
    out = dict(workload=name, sites=ns, tips=ntips, families=nf, scratch_limit_doubles=limit if limit else 32 << 20)
    if limit:
        lib.pgbp_sites_sweep_scratch_limit(limit)
    try:
        ll, scan = cgb.loglik_and_optimum_scan_sites_lg(spt, tables=False)
        assert not scan["info"].any() and np.all(np.isfinite(ll)) and np.all(scan["top_family"] >= 0), name
        out["layout_after_sweep"] = int(lib.pgbp_layout(eng))
        a, b = np.zeros((nf, ns)), np.zeros((nf, ns))
        top, topf, info = np.zeros(ns), np.zeros(ns, np.int32), np.zeros(ns, np.int32)
        ms, cnt = np.zeros(4), np.zeros(1, np.int32)
        phases = {"top": [], "tables": []}

        def optimum_top():
            ok(cgb, lib.pgbp_lg_optimum_scan_sites(eng, 0, ns, 1e-8, None, None, None, L.f64p(top), L.i32p(topf), L.i32p(info)))

        def optimum_tables():
            ok(cgb, lib.pgbp_lg_optimum_scan_sites(eng, 0, ns, 1e-8, L.f64p(a), L.f64p(b), None, L.f64p(top), L.i32p(topf), L.i32p(info)))

        def timed_twin(key, tables):
            def f():
                ok(cgb, lib.pgbp_lg_optimum_scan_sites_timed(eng, 0, ns, 1e-8, L.f64p(a) if tables else None, L.f64p(b) if tables else None,
                                                             None, L.f64p(top), L.i32p(topf), L.i32p(info), L.f64p(ms), L.i32p(cnt)))
                phases[key].append(ms.copy())
            return f

        def shift_top():
            ok(cgb, lib.pgbp_lg_shift_scan_sites(eng, 0, ns, 1e-8, None, None, None, L.f64p(top), L.i32p(topf), L.i32p(info)))

        def shift_tables():
            ok(cgb, lib.pgbp_lg_shift_scan_sites(eng, 0, ns, 1e-8, L.f64p(a), L.f64p(b), None, L.f64p(top), L.i32p(topf), L.i32p(info)))

        out["optimum_top"] = timed(optimum_top, reps)
        out["optimum_tables"] = timed(optimum_tables, reps)
        for key, tables in (("top", False), ("tables", True)):
            timed(timed_twin(key, tables), reps)
            med = np.median(np.array(phases[key][1:]), axis=0)
            out[f"phases_{key}"] = dict(validity_ms=float(med[0]), height_launches_ms=float(med[1]), fold_ms=float(med[2]),
                                        copies_ms=float(med[3]), height_launches=int(cnt[0]))
        out["shift_scan_top"] = timed(shift_top, reps)
        out["shift_scan_tables"] = timed(shift_tables, reps)
        out["ratio_optimum_over_shift_scan_top"] = out["optimum_top"]["median_ms"] / out["shift_scan_top"]["median_ms"]
        out["ratio_optimum_over_shift_scan_tables"] = out["optimum_tables"]["median_ms"] / out["shift_scan_tables"]["median_ms"]
        out["loglik_alone"] = timed(cgb.loglik_lg, reps)
        # the route before, for a handful of edges: paint the clade, two log-likelihoods
        n_edges = int((np.asarray(fam["n_parents"]) >= 1).sum())
        reg0 = np.zeros((nf, 1), np.int32)
        ts = []
        for f in rng.choice(np.flatnonzero(np.asarray(fam["n_parents"]) >= 1), size=hand_edges, replace=False):
            t0 = time.perf_counter()
            reg1, origin = P.add_optimum_shift(reg0, fam["parent_family"], int(f))
            cgb.set_optima_lg(reg1, (th + 0.1)[:, None, None])
            cgb.loglik_lg()
            cgb.set_optima_lg(reg1, (th - 0.1)[:, None, None])
            cgb.loglik_lg()
            ts.append(time.perf_counter() - t0)
        cgb.clear_optima_lg()
        out["by_hand"] = dict(edges_timed=hand_edges, median_ms_per_edge=1e3 * float(np.median(ts)), edges=n_edges)
        out["by_hand_all_edges_s"] = float(np.median(ts)) * n_edges
        out["by_hand_is_an_extrapolation"] = True
        out["ratio_by_hand_over_optimum_tables"] = 1e3 * out["by_hand_all_edges_s"] / out["optimum_tables"]["median_ms"]
    finally:
        if limit:
            lib.pgbp_sites_sweep_scratch_limit(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip", nargs="*", default=[], choices=["sites256", "cfg4"])
    ap.add_argument("--cfg4-sites", type=int, default=8000)
    ap.add_argument("--cfg4-tips", type=int, default=20000)
    ap.add_argument("--cfg4-limit", type=int, default=1 << 28, help="scratch limit in doubles for the cfg4 block")
    ap.add_argument("--hand-edges", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_time_optimum_scan.json"))
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_optimum_scan.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [("sites256", "256 univariate OU sites on a 2000-tip tree (per-site parameters)", 2000, 256, 9, 0),
            ("cfg4", f"cfg4-size: {a.cfg4_sites} univariate OU sites on a {a.cfg4_tips}-tip tree (per-site parameters)",
             a.cfg4_tips, a.cfg4_sites, 4, a.cfg4_limit)]
    for key, name, ntips, ns, seed, limit in jobs:
        if key in a.skip:
            res.setdefault("not_taken", []).append(name)
            continue
        res["blocks"].append(block(name, ntips, ns, seed, a.reps, limit, a.hand_edges))
        print(json.dumps(res["blocks"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

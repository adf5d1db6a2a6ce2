"""Times the lanes-are-sites family sweeps of a univariate batch (pgbp_lg_shift_scan_sites, pgbp_lg_edge_gradient_sites,
pgbp_lg_loo_sites) against the general calls they replace, on univariate OU batches with per-site parameters:
  * sites256: 256 sites on a 2 000-tip tree;
  * cfg4:     a cfg4-size batch, 8 000 sites on a 20 000-tip tree.
Per workload, median and minimum of --reps wall times around the synchronous C calls, outputs allocated beforehand (the Python
wrappers' own work -- edge_jump, the identified bits -- is in neither side):
  * scan_sites_top / scan_sites_tables: the new scan with tables=False (top_lr, top_family, info) and with jump and lr;
  * scan_general: pgbp_lg_shift_scan with jump and lr on the same beliefs;
  * edge_sites / edge_general, loo_sites / loo_general: all outputs of either call;
  * next_loglik_after_sites / next_loglik_after_general: the loglik_lg (fill, calibrate, integrate) that follows a sweep -- after
    a general sweep it pays for the way back into the site-minor layout.
A general call that would not finish in --max-general-s (estimated from one call) is run once only.
  * bootstrap: bootstrap_shift_scan_lg(sites=True) against sites=False at B = 1 024 replicates on the 2 000-tip tree (shared BM
    parameters, a fixed seed).
Prints one JSON line; profiles/ keeps it, stamped with the hash of csrc/."""
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


def sized(fn, reps, budget_s):
    """one call first; the repetitions only when they fit the budget"""
    t0 = time.perf_counter()
    fn()
    first = time.perf_counter() - t0
    r = reps if first * (reps + 1) <= budget_s else 1
    out = timed(fn, r, warm=0)
    out["first_call_ms"] = 1e3 * first
    return out


def ok(cgb, rc):
    assert rc == L.PGBP_OK, cgb._lib.pgbp_last_error(cgb._eng)


def block(name, ntips, ns, seed, reps, budget_s):
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
    K = cgb._lg["length"].size // nf
    nt = int(lib.pgbp_lg_loo_count(eng))
    out = dict(workload=name, sites=ns, tips=ntips, families=nf, tip_families=nt)
    ll, scan = cgb.loglik_and_shift_scan_sites_lg(spt, tables=False)
    assert not scan["info"].any() and np.all(np.isfinite(ll)), name
    out["layout_after_sweep"] = int(lib.pgbp_layout(eng))
    a, b, c = np.zeros((nf, ns)), np.zeros((nf, ns)), np.zeros((nf * K, ns))
    top, topf, info = np.zeros(ns), np.zeros(ns, np.int32), np.zeros(ns, np.int32)
    tinfo = np.zeros((nt, ns), np.int32)
    u64 = np.zeros((ns, nf), np.uint64)

    def scan_top():
        ok(cgb, lib.pgbp_lg_shift_scan_sites(eng, 0, ns, 1e-8, None, None, None, L.f64p(top), L.i32p(topf), L.i32p(info)))

    def scan_tables():
        ok(cgb, lib.pgbp_lg_shift_scan_sites(eng, 0, ns, 1e-8, L.f64p(a), L.f64p(b), None, L.f64p(top), L.i32p(topf), L.i32p(info)))

    def edge_sites():
        ok(cgb, lib.pgbp_lg_edge_gradient_sites(eng, 0, ns, L.f64p(c), L.f64p(c), L.f64p(a), L.i32p(info)))

    def loo_sites():
        ok(cgb, lib.pgbp_lg_loo_sites(eng, 0, ns, L.f64p(a[:nt]), L.f64p(b[:nt]), L.f64p(c[:nt]), L.f64p(top), L.i32p(tinfo)))

    def scan_general():
        ok(cgb, lib.pgbp_lg_shift_scan(eng, 0, ns, 1e-8, L.f64p(a), L.f64p(b), u64.ctypes.data_as(C.POINTER(C.c_uint64)), None, L.i32p(info)))

    def edge_general():
        ok(cgb, lib.pgbp_lg_edge_gradient(eng, 0, ns, L.f64p(c), L.f64p(c), L.f64p(a), L.i32p(info)))

    def loo_general():
        ok(cgb, lib.pgbp_lg_loo(eng, 0, ns, L.f64p(a[:nt]), L.f64p(b[:nt]), L.f64p(c[:nt]), L.f64p(top), L.i32p(tinfo)))

    def then_loglik(sweep):
        def f():
            sweep()
            cgb.loglik_lg()
        return f
    out["loglik_alone"] = timed(cgb.loglik_lg, reps)
    out["scan_sites_top"] = timed(scan_top, reps)
    out["scan_sites_tables"] = timed(scan_tables, reps)
    out["edge_sites"] = timed(edge_sites, reps)
    out["loo_sites"] = timed(loo_sites, reps)
    out["scan_top_then_loglik"] = timed(then_loglik(scan_top), reps)
    assert int(lib.pgbp_layout(eng)) == out["layout_after_sweep"]
    out["scan_general"] = sized(scan_general, reps, budget_s)
    cgb.loglik_lg()
    out["edge_general"] = sized(edge_general, reps, budget_s)
    cgb.loglik_lg()
    out["loo_general"] = sized(loo_general, reps, budget_s)
    cgb.loglik_lg()
    out["scan_general_then_loglik"] = sized(then_loglik(scan_general), reps, budget_s)
    for k in ("scan", "edge", "loo"):
        out[f"ratio_{k}_general_over_sites"] = out[f"{k}_general"]["median_ms"] / out[f"{k}_sites" if k != "scan" else "scan_sites_tables"]["median_ms"]
    out["next_loglik_after_sites_ms"] = out["scan_top_then_loglik"]["median_ms"] - out["scan_sites_top"]["median_ms"]
    out["next_loglik_after_general_ms"] = out["scan_general_then_loglik"]["median_ms"] - out["scan_general"]["median_ms"]
    return out


def bootstrap(ntips, B, seed, reps):
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    X = np.repeat(S.simulate_bm_uni_sites(tr, np.array([1.0]), np.array([0.0]), rng), B, axis=0)
    prob = S.cliquetree_of_tree(tr, 1)
    fam = S.lg_tree_table(tr, prob, 1)
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=B)
    cgb.lg_setup(fam, np.ascontiguousarray(X[:, :, None]))
    spt = prob.schedule[0]
    cgb.set_schedule([spt])
    cgb.assignfactors_lg_(np.array([[[1.0]]]), np.array([0.0]))
    out = dict(workload=f"bootstrap_shift_scan_lg, {B} replicates of a {ntips}-tip tree (BM, shared parameters)", replicates=B, tips=ntips)
    res = {}
    for sites in (True, False):
        res[sites] = P.bootstrap_shift_scan_lg(cgb, spt, seed=11, sites=sites)
        out["sites" if sites else "general"] = timed(lambda: P.bootstrap_shift_scan_lg(cgb, spt, seed=11, sites=sites), reps)
    out["families_equal"] = bool(np.array_equal(res[True]["family"], res[False]["family"]))
    out["worst_max_lr"] = float(np.max(np.abs(res[True]["max_lr"] - res[False]["max_lr"]) / np.maximum(1.0, res[False]["max_lr"])))
    out["ratio_general_over_sites"] = out["general"]["median_ms"] / out["sites"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip", nargs="*", default=[], choices=["sites256", "cfg4", "bootstrap"])
    ap.add_argument("--cfg4-sites", type=int, default=8000)
    ap.add_argument("--cfg4-tips", type=int, default=20000)
    ap.add_argument("--max-general-s", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_time_fam_uni.json"))
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_fam_uni.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [("sites256", "256 univariate OU sites on a 2000-tip tree (per-site parameters)", 2000, 256, 9),
            ("cfg4", f"cfg4-size: {a.cfg4_sites} univariate OU sites on a {a.cfg4_tips}-tip tree (per-site parameters)",
             a.cfg4_tips, a.cfg4_sites, 4)]
    for key, name, ntips, ns, seed in jobs:
        if key in a.skip:
            res.setdefault("not_taken", []).append(name)
            continue
        res["blocks"].append(block(name, ntips, ns, seed, a.reps, a.max_general_s))
        print(json.dumps(res["blocks"][-1]), file=sys.stderr, flush=True)
    if "bootstrap" in a.skip:
        res.setdefault("not_taken", []).append("bootstrap")
    else:
        res["bootstrap"] = bootstrap(2000, 1024, 12, a.reps)
        print(json.dumps(res["bootstrap"]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""Times the per-site clade shifts of the OU optimum (pgbp_lg_set_clade_shifts_sites and the calls around it) on univariate OU
batches with per-site parameters:
  * sites256: 256 sites on a 2 000-tip tree;
  * cfg4:     a cfg4-size batch, 8 000 sites on a 20 000-tip tree (the scratch limit raised for this block, as
              tools/time_optimum_scan.py does).
Per workload, median and minimum of --reps wall times around the synchronous calls:
  * fill_slots{0,1,4,8} / loglik_slots{0,1,4,8}: pgbp_lg_assignfactors (drained by a one-site fetch) and loglik_lg with that
    many slots in force, every site with its own random clades; with 0 slots nothing of the new code is launched;
  * score / scan_top: pgbp_lg_clade_shift_score_sites with 4 slots next to the scan with tables=False on the same beliefs;
  * refit: one fit_clade_shifts_sites_lg with 4 slots (m + 2 evaluations: fill, calibration, score);
  * select: select_optimum_shifts_sites_lg end to end, up to --max-shifts shifts at min_lr = --min-lr;
  * by_hand: the route before -- one painted engine evaluation per SITE (set_optima_lg with that site's clades, a fill, a
    calibration and a scan) -- timed for --hand-sites sites and EXTRAPOLATED to all sites and m + 2 evaluations
    (by_hand_refit_all_sites_s is that extrapolation, not a measurement).
--root PATH loads the package and the library of another checkout (the parent commit's), and --fill-only times the 0-slot fill
and loglik_lg alone and calls nothing the parent lacks: a job alternates the two checkouts with these, since with no setting
nothing of the new code is launched and the fill must lie inside the parent's own run-to-run spread.
Prints one JSON line; profiles/ keeps it, stamped with the hash of csrc/."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
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
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)), "max_ms": 1e3 * float(np.max(ts)), "reps": reps}


def block(name, ntips, ns, seed, reps, limit, hand_sites, max_shifts, min_lr, fill_only=False):
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
    kw = dict(R=g2.reshape(ns, 1, 1, 1), mu=mu[:, None], model="ou", alpha=al, theta=th[:, None])
    cgb.assignfactors_lg_(**kw)
    lib, eng = cgb._lib, cgb._eng
    nf = len(fam["cluster"])
    real = np.flatnonzero(np.asarray(fam["n_parents"]) >= 1)
    out = dict(workload=name, sites=ns, tips=ntips, families=nf, scratch_limit_doubles=limit if limit else 32 << 20)
    one = np.zeros(1)

    def fill():
        cgb.assignfactors_lg_(**kw)
        lib.pgbp_get_belief(eng, 0, 0, L.f64p(one))   # (drains the stream)

    def setting(m):
        f = np.stack([rng.choice(real, size=m, replace=False) for _ in range(ns)], axis=1).astype(np.int32)
        return f, rng.normal(size=(m, ns))

    if fill_only:
        out["fill_slots0"] = timed(fill, reps)
        out["loglik_slots0"] = timed(cgb.loglik_lg, reps)
        return out
    if limit:
        lib.pgbp_sites_sweep_scratch_limit(limit)
    try:
        for m in (0, 1, 4, 8):
            if m:
                cgb.set_clade_shifts_sites_lg(*setting(m))
            else:
                cgb.clear_clade_shifts_sites_lg()
            out[f"fill_slots{m}"] = timed(fill, reps)
            out[f"loglik_slots{m}"] = timed(cgb.loglik_lg, reps)
        fam4, d4 = setting(4)
        cgb.set_clade_shifts_sites_lg(fam4, d4)
        ll, sc = cgb.loglik_and_clade_shift_score_sites_lg(spt)
        assert not sc["info"].any() and np.all(np.isfinite(ll)), name
        g, Hd, kt = np.zeros((4, ns)), np.zeros((4, ns)), np.zeros((4, ns))
        top, topf, info = np.zeros(ns), np.zeros(ns, np.int32), np.zeros(ns, np.int32)

        def score():
            assert lib.pgbp_lg_clade_shift_score_sites(eng, 0, ns, 1e-8, L.f64p(g), L.f64p(Hd), L.f64p(kt), L.i32p(info)) == 0

        def scan_top():
            assert lib.pgbp_lg_optimum_scan_sites(eng, 0, ns, 1e-8, None, None, None, L.f64p(top), L.i32p(topf), L.i32p(info)) == 0

        out["score_slots4"] = timed(score, reps)
        out["scan_top_slots4"] = timed(scan_top, reps)
        out["refit_slots4"] = timed(lambda: P.fit_clade_shifts_sites_lg(cgb, spt), max(3, reps // 4))
        out["refit_evaluations"] = 4 + 2
        sel = {}

        def select():
            sel["out"] = P.select_optimum_shifts_sites_lg(cgb, spt, max_shifts, min_lr)

        out["select"] = timed(select, max(3, reps // 4))
        out["select_max_shifts"], out["select_min_lr"] = max_shifts, min_lr
        out["select_shifts_found"] = int(sel["out"]["n_shifts"].sum())
        # the route before: one painted engine evaluation per site
        cgb.clear_clade_shifts_sites_lg()
        ts = []
        for s in rng.choice(ns, size=hand_sites, replace=False):
            t0 = time.perf_counter()
            reg = np.zeros((nf, 1), np.int32)
            for v in fam4[:, s]:
                reg, origin = P.add_optimum_shift(reg, fam["parent_family"], int(v))
            cgb.set_optima_lg(reg, np.tile((th[:, None] + 0.1)[:, :1], (1, int(reg.max())))[:, :, None])
            cgb.loglik_and_optimum_scan_sites_lg(spt, tables=False)
            ts.append(time.perf_counter() - t0)
        cgb.clear_optima_lg()
        out["by_hand"] = dict(sites_timed=hand_sites, median_ms_per_site_evaluation=1e3 * float(np.median(ts)))
        out["by_hand_refit_all_sites_s"] = float(np.median(ts)) * ns * 6
        out["by_hand_is_an_extrapolation"] = True
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
    ap.add_argument("--hand-sites", type=int, default=4)
    ap.add_argument("--max-shifts", type=int, default=3)
    ap.add_argument("--min-lr", type=float, default=12.0)
    ap.add_argument("--root", default=None, help="another checkout whose package and library are loaded")
    ap.add_argument("--fill-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_time_clade_shifts.json"))
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_clade_shifts.py", "root": ROOT if a.root else ".", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [("sites256", "256 univariate OU sites on a 2000-tip tree (per-site parameters)", 2000, 256, 9, 0),
            ("cfg4", f"cfg4-size: {a.cfg4_sites} univariate OU sites on a {a.cfg4_tips}-tip tree (per-site parameters)",
             a.cfg4_tips, a.cfg4_sites, 4, a.cfg4_limit)]
    for key, name, ntips, ns, seed, limit in jobs:
        if key in a.skip:
            res.setdefault("not_taken", []).append(name)
            continue
        res["blocks"].append(block(name, ntips, ns, seed, a.reps, limit, a.hand_sites, a.max_shifts, a.min_lr, a.fill_only))
        print(json.dumps(res["blocks"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

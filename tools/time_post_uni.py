"""Times the lanes-are-sites calls on a fitted univariate batch (pgbp_moments_sites, pgbp_sample_posterior_sites,
pgbp_lg_impute_sites) against the general calls they replace, on univariate OU batches with per-site parameters:
  * sites256: 256 sites on a 2 000-tip tree;
  * cfg4:     a cfg4-size batch, 8 000 sites on a 20 000-tip tree.
One tip in sixteen carries no data (the imputation's list).  Per workload, median and minimum of --reps wall times around the
synchronous C calls, outputs allocated beforehand:
  * moments_sites / moments_general: mean, the covariance and norm of every cluster;
  * impute_sites / impute_general;
  * draws_sites_z{1,8} / draws_sites_seed{1,8} / draws_general{1,8}: 1 and 8 joint draws, from a host z and from the device
    generator, with the phases of one timed call each (the copies' share);
  * next_loglik_after_moments_sites / next_loglik_after_moments_general: the loglik_lg (fill, calibrate, integrate) timed on its
    own right after an untimed call -- after a general call it pays for the way back into the site-minor layout.
A call that would not finish its repetitions in --max-call-s (estimated from one call) is run once only; a block of draws whose
host arrays would exceed --max-host-gb is not taken (and listed).
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


def sized(fn, reps, budget_s):
    """one call first; the repetitions only when they fit the budget"""
    t0 = time.perf_counter()
    fn()
    first = time.perf_counter() - t0
    r = reps if first * (reps + 1) <= budget_s else 1
    out = timed(fn, r, warm=0)
    out["first_call_ms"] = 1e3 * first
    return out


def timed_after(first, fn, reps, budget_s):
    """fn timed right after an untimed `first`, each repetition (what the call leaves behind for the next traversal)"""
    t0 = time.perf_counter()
    first()
    r = reps if (time.perf_counter() - t0) * (reps + 1) <= budget_s else 1
    ts = []
    for _ in range(r):
        first()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)), "reps": r}


def ok(cgb, rc):
    assert rc == L.PGBP_OK, cgb._lib.pgbp_last_error(cgb._eng)


def block(name, ntips, ns, seed, reps, budget_s, max_host_gb):
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
    # one tip in sixteen without data, never two of one cherry (a clade without data is not predicted)
    tips = [f for f in range(len(fam["cluster"])) if fam["child_pos"][f] < 0 and fam["data_row"][f] >= 0]
    seen, gone = set(), []
    for f in tips[::16]:
        par = int(tr.parent[f + 1])   # (family f is node f + 1)
        if par not in seen:
            seen.add(par)
            gone.append(f)
    fam = dict(fam)
    cm = np.ones(len(fam["cluster"]), np.uint64)
    cm[gone] = 0
    fam["child_mask"] = cm
    fam["parent_mask"] = np.ones(len(fam["cluster"]) * max(1, int(fam["max_parents"])), np.uint64)
    data = np.ascontiguousarray(X[:, :, None])
    data[:, fam["data_row"][gone], 0] = np.nan
    del X
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=ns)
    cgb.lg_setup(fam, data)
    del data
    spt = prob.schedule[0]
    cgb.set_schedule([spt])
    cgb.assignfactors_lg_(g2.reshape(ns, 1, 1, 1), mu[:, None], model="ou", alpha=al, theta=th[:, None])
    lib, eng = cgb._lib, cgb._eng
    nc = cgb.nclusters
    dims = cgb._dims[:nc].astype(np.int64)
    nm, nt, size = int(dims.sum()), int((dims * (dims + 1) // 2).sum()), int(lib.pgbp_sample_size(eng))
    nl = int(lib.pgbp_lg_impute_count(eng))
    out = dict(workload=name, sites=ns, tips=ntips, clusters=nc, sample_size=size, listed_tips=nl)
    ll, imp = cgb.impute_and_loglik_sites_lg(spt)
    assert np.all(np.isfinite(ll)) and not imp["info"].any(), name
    out["layout_after_call"] = int(lib.pgbp_layout(eng))
    info = np.zeros(max(ns, nc * ns, nl * ns), np.int32)
    mean, tri, norm = np.zeros((nm, ns)), np.zeros((nt, ns)), np.zeros((nc, ns))
    per = int(lib.pgbp_moments_size(eng, 0, None, 1))
    gen = np.zeros((ns, per))
    im, iv = np.zeros((nl, ns)), np.zeros((nl, ns))

    def moments_sites():
        ok(cgb, lib.pgbp_moments_sites(eng, 0, None, 0, ns, L.f64p(mean), L.f64p(tri), L.f64p(norm), L.i32p(info)))

    def moments_general():
        ok(cgb, lib.pgbp_moments(eng, 0, None, 0, ns, 1, L.f64p(gen), L.i32p(info)))

    def impute_sites():
        ok(cgb, lib.pgbp_lg_impute_sites(eng, 0, ns, L.f64p(im), L.f64p(iv), L.i32p(info)))

    def impute_general():
        ok(cgb, lib.pgbp_lg_impute(eng, 0, ns, L.f64p(im), L.f64p(iv), L.i32p(info)))

    note = lambda what: print(f"[{name}] {what}", file=sys.stderr, flush=True)
    note("set up and calibrated")
    out["loglik_alone"] = timed(cgb.loglik_lg, reps)
    out["moments_sites"] = sized(moments_sites, reps, budget_s)
    out["impute_sites"] = sized(impute_sites, reps, budget_s)
    out["next_loglik_after_moments_sites"] = timed_after(moments_sites, cgb.loglik_lg, reps, budget_s)
    assert int(lib.pgbp_layout(eng)) == out["layout_after_call"]
    note("the new moments and imputation timed")
    out["moments_general"] = sized(moments_general, reps, budget_s)
    note("the general moments timed")
    cgb.loglik_lg()
    out["impute_general"] = sized(impute_general, reps, budget_s)
    cgb.loglik_lg()
    out["next_loglik_after_moments_general"] = timed_after(moments_general, cgb.loglik_lg, reps, budget_s)
    del mean, tri, norm, gen
    note("the general calls timed")
    for nd in (1, 8):
        gb = 8.0 * nd * size * ns / 2 ** 30
        if gb > max_host_gb:
            out.setdefault("not_taken", []).append(f"{nd} draws: {gb:.1f} GB of host array x")
            continue
        with_z = 2 * gb <= max_host_gb
        if not with_z:
            out.setdefault("not_taken", []).append(f"{nd} draws from a host z, new and general call: {2 * gb:.1f} GB of host arrays (z and x)")
        z = np.random.default_rng(seed + nd).standard_normal((nd, size, ns)) if with_z else None
        x = np.zeros((nd, size, ns))
        ms = np.zeros(4)

        def draws_z():
            ok(cgb, lib.pgbp_sample_posterior_sites(eng, 0, 0, ns, nd, L.f64p(z), 0, L.f64p(x), L.i32p(info)))

        def draws_seed():
            ok(cgb, lib.pgbp_sample_posterior_sites(eng, 0, 0, ns, nd, None, 20261, L.f64p(x), L.i32p(info)))

        def draws_general():   # (z and x read as [nd][ns][size]: the same bytes moved)
            ok(cgb, lib.pgbp_sample_posterior(eng, 0, 0, ns, nd, L.f64p(z), L.f64p(x), L.i32p(info)))
        cgb.loglik_lg()
        if with_z:
            out[f"draws_sites_z{nd}"] = sized(draws_z, reps, budget_s)
            ok(cgb, lib.pgbp_sample_posterior_sites_timed(eng, 0, 0, ns, nd, L.f64p(z), 0, L.f64p(x), L.i32p(info), L.f64p(ms)))
            out[f"draws_sites_z{nd}"]["phases_ms"] = dict(zip(("validity", "copy_z", "levels", "copy_x"), ms.tolist()))
        out[f"draws_sites_seed{nd}"] = sized(draws_seed, reps, budget_s)
        ok(cgb, lib.pgbp_sample_posterior_sites_timed(eng, 0, 0, ns, nd, None, 20261, L.f64p(x), L.i32p(info), L.f64p(ms)))
        out[f"draws_sites_seed{nd}"]["phases_ms"] = dict(zip(("validity", "copy_z", "levels", "copy_x"), ms.tolist()))
        assert int(lib.pgbp_layout(eng)) == out["layout_after_call"]
        note(f"{nd} draws: the new call timed")
        if not with_z:
            del x
            continue
        out[f"draws_general{nd}"] = sized(draws_general, reps, budget_s)
        ok(cgb, lib.pgbp_sample_posterior_timed(eng, 0, 0, ns, nd, L.f64p(z), L.f64p(x), L.i32p(info), L.f64p(ms)))
        out[f"draws_general{nd}"]["phases_ms"] = dict(zip(("factor", "copy_z", "apply", "copy_x"), ms.tolist()))
        out[f"ratio_draws{nd}_general_over_sites_z"] = out[f"draws_general{nd}"]["median_ms"] / out[f"draws_sites_z{nd}"]["median_ms"]
        del z, x
    for k in ("moments", "impute"):
        out[f"ratio_{k}_general_over_sites"] = out[f"{k}_general"]["median_ms"] / out[f"{k}_sites"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip", nargs="*", default=[], choices=["sites256", "cfg4"])
    ap.add_argument("--cfg4-sites", type=int, default=8000)
    ap.add_argument("--cfg4-tips", type=int, default=20000)
    ap.add_argument("--max-call-s", type=float, default=40.0)
    ap.add_argument("--max-host-gb", type=float, default=32.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_time_post_uni.json"))
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_post_uni.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [("sites256", "256 univariate OU sites on a 2000-tip tree (per-site parameters)", 2000, 256, 9),
            ("cfg4", f"cfg4-size: {a.cfg4_sites} univariate OU sites on a {a.cfg4_tips}-tip tree (per-site parameters)",
             a.cfg4_tips, a.cfg4_sites, 4)]
    for key, name, ntips, ns, seed in jobs:
        if key in a.skip:
            res.setdefault("not_taken", []).append(name)
            continue
        res["blocks"].append(block(name, ntips, ns, seed, a.reps, a.max_call_s, a.max_host_gb))
        print(json.dumps(res["blocks"][-1]), file=sys.stderr, flush=True)
        if a.out:   # (kept after every block: a later block may run out of time)
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

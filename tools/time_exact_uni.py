"""Times the closed-form BM fit of every site of a univariate batch (pgbp_bm_exact_stats_sites, calibrate_exact_sites_) against
the routes it replaces, on univariate BM batches with an improper root (and the fixed-root engine of the same batch):
  * sites256: 256 sites on a 2 000-tip tree;
  * cfg4:     a cfg4-size batch, 8 000 sites on a 20 000-tip tree.
Per workload, median and minimum of --reps wall times around the calls (the C calls with outputs allocated beforehand):
  * sweep_sites:            pgbp_bm_exact_stats_sites alone, with mu, on calibrated beliefs;
  * driver / driver_scored: calibrate_exact_sites_ end to end (fill, calibrate, sweep), without and with the score on the
                            fixed-root engine;
  * sweep_general:          pgbp_bm_exact_stats on the same beliefs, and next_loglik_after_general_ms: what the loglik_lg timed
                            right after it costs (it pays for the way back into the site-minor layout), next to loglik_alone;
  * fit_sites_lg:           fit_sites_lg(model="bm") on the fixed-root engine from (1, 0), once, with its evaluation count;
  * masked_*:               the sweep and the driver under a per-site mask of about 30 % of the entries, where the general call
                            refuses (its return code is recorded) and fit_sites_lg is the only other route.
Also the worst relative difference of the closed form from fit_sites_lg's optimum.  Prints one JSON line; profiles/ keeps it,
stamped with the hash of csrc/."""
import argparse
import gc
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


def specs(tr, X):
    """what the two engines of a synth tree on its clique tree are made from: ([improper-root spec, fixed-root spec], schedule
    tree, root, leaves); a spec is (scopes, family table, data)"""
    names = [f"n{i}" for i in range(tr.nnodes)]
    leaves = [i for i in range(tr.nnodes) if tr.is_leaf[i]]
    net, nm = P.read_newick(tr.newick(names))
    row = {names[i]: r for r, i in enumerate(leaves)}
    data_row = [row.get(nm[i], -1) for i in range(net.nnodes)]
    cn, ed, sn = P.cliquetree(net.node2family)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    data = np.ascontiguousarray(X[:, leaves, None])
    out = []
    for fixedroot in (False, True):
        st = P.allocate_scopes(cn, ed, sn, net, 1, fixedroot=fixedroot)
        out.append((st, P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, data_row, 1), data))
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    st = out[0][0]
    ci = next(i for i, c in enumerate(cn) if 1 in c and st.dims[i] > 0)   # the root (label 1) is listed last in its cluster
    return out, spt, (ci, int(st.dims[ci]) - 1), leaves


def engine(spec, ns, mask=None):
    st, fam, data = spec
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=ns)
    cgb.lg_setup(fam, data)
    if mask is not None:
        cgb.set_site_missing_lg(mask)
    return cgb


def closed_form(out, cgb, fx, spt, root, ns, reps, mask):
    """the improper-root engine's part: the sweep, the driver (scored when the fixed-root engine fits beside it), the general
    call; then the same under the mask.  Returns the two fits (without and with the mask)."""
    lib, eng = cgb._lib, cgb._eng
    num, den, mh, info = np.zeros(ns), np.zeros(ns), np.zeros(ns), np.zeros(ns, np.int32)

    def sweep_sites():
        rc = lib.pgbp_bm_exact_stats_sites(eng, 0, ns, root[0], root[1], L.f64p(num), L.f64p(den), L.f64p(mh), L.i32p(info))
        assert rc == L.PGBP_OK, lib.pgbp_last_error(eng)

    def sweep_general():
        rc = lib.pgbp_bm_exact_stats(eng, 0, ns, L.f64p(num), L.f64p(den), L.i32p(info))
        assert rc == L.PGBP_OK, lib.pgbp_last_error(eng)

    def general_then_loglik():
        sweep_general()
        cgb.loglik_lg()

    fit = P.calibrate_exact_sites_(cgb, spt, root, fx)
    assert not fit["info"].any() and (fx is None or np.all(np.isfinite(fit["loglik"]))), out["workload"]
    out["layout_after_driver"] = int(lib.pgbp_layout(eng))
    out["sweep_sites"] = timed(sweep_sites, reps)
    out["driver"] = timed(lambda: P.calibrate_exact_sites_(cgb, spt, root), reps)
    if fx is not None:
        out["driver_scored"] = timed(lambda: P.calibrate_exact_sites_(cgb, spt, root, fx), reps)
    out["loglik_alone"] = timed(cgb.loglik_lg, reps)
    P.calibrate_exact_sites_(cgb, spt, root)
    out["sweep_general"] = timed(sweep_general, reps)
    out["general_then_loglik"] = timed(general_then_loglik, reps)
    out["next_loglik_after_general_ms"] = out["general_then_loglik"]["median_ms"] - out["sweep_general"]["median_ms"]
    out["ratio_general_over_sites"] = out["sweep_general"]["median_ms"] / out["sweep_sites"]["median_ms"]
    for e in (cgb, fx):
        if e is not None:
            e.set_site_missing_lg(mask)
    m = P.calibrate_exact_sites_(cgb, spt, root, fx)
    assert not m["info"].any(), out["workload"]
    out["masked_entries"] = float(mask.mean())
    out["masked_den_against_n_obs_less_one"] = float(np.max(np.abs(m["den"] - ((~mask).sum(axis=1) - 1.0))))
    out["masked_sweep_sites"] = timed(sweep_sites, reps)
    out["masked_driver"] = timed(lambda: P.calibrate_exact_sites_(cgb, spt, root), reps)
    if fx is not None:
        out["masked_driver_scored"] = timed(lambda: P.calibrate_exact_sites_(cgb, spt, root, fx), reps)
    out["masked_general_rc"] = int(lib.pgbp_bm_exact_stats(eng, 0, ns, L.f64p(num), L.f64p(den), L.i32p(info)))
    return fit, m


def lbfgs(out, key, fx, spt, fit):
    """fit_sites_lg(model="bm") from (1, 0) on the fixed-root engine, once, against the closed form's ML rescaling"""
    t0 = time.perf_counter()
    lb = P.fit_sites_lg(fx, spt, "bm", 1.0, 0.0)
    out[key] = {"once_ms": 1e3 * (time.perf_counter() - t0), "n_device_evals": int(lb["n_device_evals"]),
                "converged": int(np.sum(lb["converged"]))}
    ml = fit["R"] * fit["den"] / (fit["den"] + 1.0)
    out[key]["closed_form_R_ml_rel"] = float(np.max(np.abs(ml / lb["R"] - 1.0)))
    out[key]["closed_form_mu_abs"] = float(np.max(np.abs(fit["mu"] - lb["mu"])))


def block(name, ntips, ns, seed, reps, with_fit):
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    s2, mu = rng.uniform(0.5, 2.0, ns), rng.normal(size=ns)
    X = S.simulate_bm_uni_sites(tr, s2, mu, rng)
    sp, spt, root, leaves = specs(tr, X)
    del X
    # the mask: about 30 % of the entries, at least three observed tips per site
    mask = rng.random((ns, len(leaves))) < 0.3
    mask[mask.sum(axis=1) > len(leaves) - 3] = False
    out = dict(workload=name, sites=ns, tips=ntips, families=len(sp[0][1]["cluster"]))
    cgb = engine(sp[0], ns)
    try:
        fx = engine(sp[1], ns)
    except P.PgbpError as err:   # (the two engines of a cfg4-size batch do not always fit one device side by side)
        fx = None
        out["fixed_root_engine_beside_the_first"] = f"no: {err}"
    fit, fit_masked = closed_form(out, cgb, fx, spt, root, ns, reps, mask)
    if with_fit:
        if fx is None:
            del cgb
            gc.collect()
            fx = engine(sp[1], ns)
        else:
            fx.set_site_missing_lg(None, data=sp[1][2])
        lbfgs(out, "fit_sites_lg", fx, spt, fit)
        out["ratio_fit_sites_lg_over_driver"] = out["fit_sites_lg"]["once_ms"] / out["driver"]["median_ms"]
        fx.set_site_missing_lg(mask)
        lbfgs(out, "masked_fit_sites_lg", fx, spt, fit_masked)
        out["ratio_masked_fit_sites_lg_over_driver"] = out["masked_fit_sites_lg"]["once_ms"] / out["masked_driver"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip", nargs="*", default=[], choices=["sites256", "cfg4"])
    ap.add_argument("--no-fit", action="store_true", help="leave fit_sites_lg out")
    ap.add_argument("--cfg4-sites", type=int, default=8000)
    ap.add_argument("--cfg4-tips", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_time_exact_uni.json"))
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_exact_uni.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [("sites256", "256 univariate BM sites on a 2000-tip tree (improper root)", 2000, 256, 9),
            ("cfg4", f"cfg4-size: {a.cfg4_sites} univariate BM sites on a {a.cfg4_tips}-tip tree (improper root)",
             a.cfg4_tips, a.cfg4_sites, 4)]
    for key, name, ntips, ns, seed in jobs:
        if key in a.skip:
            res.setdefault("not_taken", []).append(name)
            continue
        res["blocks"].append(block(name, ntips, ns, seed, a.reps, not a.no_fit))
        print(json.dumps(res["blocks"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

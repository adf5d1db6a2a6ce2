"""Times pgbp_posterior_cov_sites (the posterior covariance of a univariate batch with lanes = sites) against the general
pgbp_posterior_cov on the same beliefs, on univariate OU batches with per-site parameters:
  * sites256: 256 sites on a 2 000-tip tree;
  * cfg4:     a cfg4-size batch, 8 000 sites on a 20 000-tip tree.
Two functionals over the sampler's layout: a contrast (the difference of two ancestors far apart in the layout) and a clade
mean (the average of 64 ancestors).  Per workload, median and minimum of --reps wall times around the synchronous C calls,
outputs allocated beforehand:
  * gram_only:            both columns, gram alone (no table of size x sites on the host);
  * one_column_w_k:       the contrast with w and k, and the phases of one timed call;
  * general_gram_columns: the general call for the two columns with w alone (what functional_moments needs), and
    general_one_column_w_k with its phases -- where their host tables fit --max-host-gb, otherwise listed as not taken;
  * next_loglik_after_*:  the loglik_lg (fill, calibrate, integrate) timed on its own right after an untimed call -- after a
    general call it pays for the way back into the site-minor layout.
A call that would not finish its repetitions in --max-call-s (estimated from one call) is run once only.
Prints one JSON line; profiles/ keeps it, stamped with the hash of csrc/."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import pgbp_amd as P  # noqa: E402
from pgbp_amd import _lib as L  # noqa: E402
from pgbp_amd import synth as S  # noqa: E402
from time_post_uni import ok, sized, timed, timed_after  # noqa: E402


def block(name, ntips, ns, seed, reps, budget_s, max_host_gb):
    note = lambda what: print(f"[{name}] {what}", file=sys.stderr, flush=True)
    note("setting up")
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
    data = np.ascontiguousarray(X[:, :, None])
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
    off = np.concatenate([[0], np.cumsum(dims)])
    size = int(lib.pgbp_sample_size(eng))
    out = dict(workload=name, sites=ns, tips=ntips, clusters=nc, sample_size=size)

    def calibrate():   # (postorder, preorder, integrate: loglik_lg alone leaves the beliefs after the postorder)
        ll, _, cinfo = cgb._loglik_and_sites(spt, lambda: None)
        assert np.all(np.isfinite(ll)) and not cinfo.any(), name

    calibrate()
    out["layout_after_calibration"] = int(lib.pgbp_layout(eng))
    # the functionals: a contrast of two entries far apart, the mean of the first variable of 64 clusters spread over the layout
    two = [c for c in range(nc) if dims[c] == 2]
    c2 = np.zeros((2, size))
    c2[0, off[two[len(two) // 3]]], c2[0, off[two[2 * len(two) // 3]]] = 1.0, -1.0
    c2[1, off[np.array(two)[np.linspace(0, len(two) - 1, 64).astype(int)]]] = 1.0 / 64
    c1 = np.ascontiguousarray(c2[:1])
    info = np.zeros(ns, np.int32)
    gram = np.zeros((3, ns))
    ms = np.zeros(5)
    note("set up and calibrated")
    out["loglik_alone"] = timed(cgb.loglik_lg, reps)
    calibrate()

    def gram_only():
        ok(cgb, lib.pgbp_posterior_cov_sites(eng, 0, 0, ns, 2, L.f64p(c2), None, None, L.f64p(gram), L.i32p(info)))

    out["gram_only"] = sized(gram_only, reps, budget_s)
    ok(cgb, lib.pgbp_posterior_cov_sites_timed(eng, 0, 0, ns, 2, L.f64p(c2), None, None, L.f64p(gram), L.i32p(info), L.f64p(ms)))
    names = ("validity", "adjoint", "gram", "forward", "copies")
    out["gram_only"]["phases_ms"] = dict(zip(names, ms.tolist()))
    out["next_loglik_after_gram_only"] = timed_after(gram_only, cgb.loglik_lg, reps, budget_s)
    assert not info.any() and int(lib.pgbp_layout(eng)) == out["layout_after_calibration"]
    note("gram alone timed")
    calibrate()
    gb = 8.0 * size * ns / 2 ** 30
    out["table_gb_per_column"] = gb
    if 2 * gb > max_host_gb:
        out.setdefault("not_taken", []).append(f"one column with w and k, new and general call: {2 * gb:.1f} GB of host arrays")
        return out
    w, k = np.zeros((1, size, ns)), np.zeros((1, size, ns))

    def one_column():
        ok(cgb, lib.pgbp_posterior_cov_sites(eng, 0, 0, ns, 1, L.f64p(c1), L.f64p(w), L.f64p(k), None, L.i32p(info)))

    out["one_column_w_k"] = sized(one_column, reps, budget_s)
    ok(cgb, lib.pgbp_posterior_cov_sites_timed(eng, 0, 0, ns, 1, L.f64p(c1), L.f64p(w), L.f64p(k), None, L.i32p(info), L.f64p(ms)))
    out["one_column_w_k"]["phases_ms"] = dict(zip(names, ms.tolist()))
    out["next_loglik_after_one_column_w_k"] = timed_after(one_column, cgb.loglik_lg, reps, budget_s)
    assert int(lib.pgbp_layout(eng)) == out["layout_after_calibration"]
    note("one column with w and k timed")
    calibrate()

    def general_one_column():   # (w and k read as [1][ns][size]: the same bytes moved)
        ok(cgb, lib.pgbp_posterior_cov(eng, 0, 0, ns, 1, L.f64p(c1), L.f64p(w), L.f64p(k), L.i32p(info)))

    out["general_one_column_w_k"] = sized(general_one_column, reps, budget_s)
    ok(cgb, lib.pgbp_posterior_cov_timed(eng, 0, 0, ns, 1, L.f64p(c1), L.f64p(w), L.f64p(k), L.i32p(info), L.f64p(ms)))
    out["general_one_column_w_k"]["phases_ms"] = dict(zip(("factor", "copy_c", "adjoint_w", "forward", "copies"), ms.tolist()))
    calibrate()
    out["next_loglik_after_general_one_column_w_k"] = timed_after(general_one_column, cgb.loglik_lg, reps, budget_s)
    note("the general call, one column, timed")
    del k
    calibrate()
    w2 = np.concatenate([w, w])

    def general_gram_columns():
        ok(cgb, lib.pgbp_posterior_cov(eng, 0, 0, ns, 2, L.f64p(c2), L.f64p(w2), None, L.i32p(info)))

    out["general_gram_columns"] = sized(general_gram_columns, reps, budget_s)
    cgb.loglik_lg()
    note("the general call, two columns of w, timed")
    out["ratio_general_over_sites_one_column_w_k"] = out["general_one_column_w_k"]["median_ms"] / out["one_column_w_k"]["median_ms"]
    out["ratio_general_two_columns_w_over_gram_only"] = out["general_gram_columns"]["median_ms"] / out["gram_only"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip", nargs="*", default=[], choices=["sites256", "cfg4"])
    ap.add_argument("--cfg4-sites", type=int, default=8000)
    ap.add_argument("--cfg4-tips", type=int, default=20000)
    ap.add_argument("--max-call-s", type=float, default=40.0)
    ap.add_argument("--max-host-gb", type=float, default=32.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_time_cov_uni.json"))
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_cov_uni.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
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

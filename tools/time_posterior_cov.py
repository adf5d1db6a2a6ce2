"""Times pgbp_posterior_cov for the p columns of one internal node: the factor, adjoint and forward phases separately, against
pgbp_sample_posterior with as many draws on the same beliefs (the new call is about two applies).

Workloads: a 5 000-tip 16-trait tree and cfg3's clique tree (50 000 tips x 16 traits, seed 3), each calibrated first.
Per workload, median of --reps (default 12) repetitions, minimum alongside:
  * the whole call with w and k, and with w alone (no forward pass);
  * pgbp_posterior_cov_timed's phases (the stream drained after each): factor, copy of c, adjoint with w, forward, copies of w
    and k;
  * pgbp_sample_posterior and pgbp_sample_posterior_timed's phases with p draws;
  * the number of level launches of each phase (from the schedule tree: one adjoint launch per level and one for w, one forward
    launch per level);
  * what the only exact alternative would move -- D unit draws through pgbp_sample_posterior, z up and x down, D doubles each:
    computed from D, not run.
Prints one JSON line; profiles/ keeps it, stamped with the hash of csrc/."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import pgbp_amd as P  # noqa: E402
from time_sample import f64, timed, tree_engine  # noqa: E402


def levels_of(sched, nc):
    depth = np.zeros(nc, dtype=np.int64)
    for pa, ch in zip(sched[-2], sched[-1]):
        depth[int(ch)] = depth[int(pa)] + 1
    return int(depth.max()) + 1


def phases(call, n, reps):
    ms, rows = np.zeros(n), []
    for _ in range(reps):
        call(ms)
        rows.append(ms.copy())
    return [float(v) for v in np.median(np.array(rows), axis=0)]


def block(name, cgb, sched, reps):
    lib, eng, nc = cgb._lib, cgb._eng, cgb.nclusters
    size = int(lib.pgbp_sample_size(eng))
    dims = cgb._dims[:nc].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(dims)])
    p = int(dims.min())
    inner = [b for b in range(nc) if dims[b] == 2 * p]
    b = inner[len(inner) // 2]                      # a {node, parent} cluster: its first p entries are one internal node
    c = np.zeros((p, size))
    c[np.arange(p), off[b] + np.arange(p)] = 1.0
    w, k = np.zeros((p, 1, size)), np.zeros((p, 1, size))
    info = np.zeros(1, np.int32)
    ip = info.ctypes.data_as(C.POINTER(C.c_int32))
    n_levels = levels_of(sched, nc)
    out = {"workload": name, "clusters": nc, "max_dim": int(dims.max()), "sample_size": size, "columns": p, "cluster": int(b),
           "levels": n_levels, "launches": {"adjoint": n_levels + 1, "forward": n_levels}}

    def both():
        assert lib.pgbp_posterior_cov(eng, 0, 0, 1, p, f64(c), f64(w), f64(k), ip) == 0, lib.pgbp_last_error(eng)

    def w_only():
        assert lib.pgbp_posterior_cov(eng, 0, 0, 1, p, f64(c), f64(w), None, ip) == 0, lib.pgbp_last_error(eng)
    out["posterior_cov"] = timed(both, reps)
    assert info[0] == 0 and np.all(np.isfinite(k)) and np.all(np.isfinite(w))
    out["posterior_cov_w_only"] = timed(w_only, reps)

    def cov_timed(ms):
        assert lib.pgbp_posterior_cov_timed(eng, 0, 0, 1, p, f64(c), f64(w), f64(k), ip, f64(ms)) == 0
    ph = phases(cov_timed, 5, reps)
    out["posterior_cov"].update({"factor_ms": ph[0], "copy_c_ms": ph[1], "adjoint_ms": ph[2], "forward_ms": ph[3],
                                 "copy_w_k_ms": ph[4]})
    z = np.random.default_rng(p).standard_normal((p, 1, size))
    x = np.zeros_like(z)

    def sample():
        assert lib.pgbp_sample_posterior(eng, 0, 0, 1, p, f64(z), f64(x), ip) == 0, lib.pgbp_last_error(eng)
    out["sample_posterior"] = timed(sample, reps)

    def sample_timed(ms):
        assert lib.pgbp_sample_posterior_timed(eng, 0, 0, 1, p, f64(z), f64(x), ip, f64(ms)) == 0
    ph = phases(sample_timed, 4, reps)
    out["sample_posterior"].update({"draws": p, "factor_ms": ph[0], "copy_z_ms": ph[1], "apply_ms": ph[2], "copy_x_ms": ph[3]})
    out["vs_sample_posterior"] = out["posterior_cov"]["median_ms"] / out["sample_posterior"]["median_ms"]
    out["unit_draw_alternative"] = {"draws": size, "z_bytes": 8 * size * size, "x_bytes": 8 * size * size,
                                    "this_call_bytes": 8 * size * 3 * p, "taken": False}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip", nargs="*", default=[], choices=["cfg3", "tree5000"])
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_posterior_cov.py", "csrc_sha16": bench.csrc_sha16(), "reps": a.reps, "blocks": [],
           "not_measured": ["several GPUs", "column counts beyond one node"]}
    jobs = [("tree5000", "5000-tip tree, 16 traits, clique tree, seed 3", lambda: tree_engine(5000, 16, 3)),
            ("cfg3", "cfg3: 50000-tip tree, 16 traits, clique tree, seed 3", lambda: tree_engine(50000, 16, 3))]
    for key, name, make in jobs:
        if key in a.skip:
            res.setdefault("not_taken", []).append(name)
            continue
        cgb, sched = make()
        res["blocks"].append(block(name, cgb, sched, a.reps))
        del cgb
    print(json.dumps(res))


if __name__ == "__main__":
    main()

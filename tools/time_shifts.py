"""Times what mean shifts on edges cost (pgbp_lg_set_shifts, the correction kernel of csrc/pgbp_shift.hip, fit_shifts_lg).

Per workload, on one GPU, wall time around synchronous calls (each followed by a stream synchronisation), warm-up first,
median of the repetitions with the minimum alongside:
  assignfactors_{0,8,all}  assignfactors_lg_ + sync with no shift, 8 shifted edges, every edge shifted (the fill, and after it
                           the correction of the shifted clusters)
  loglik_{0,8}             loglik_lg (fill, postorder, root integration) with no shift and with 8 shifted edges
  fit_4                    fit_shifts_lg on 4 edges (n p + 2 fills, calibrations and edge sweeps), once
  one_evaluation           assignfactors_lg_ + loglik_and_edge_gradient_lg: one fill + calibrate + edge sweep, the unit of the fit
Workloads, those of tools/time_gradient.py: (a) 5 000-tip tree, 16 traits, clique tree, full BM; (b) cfg3: 50 000 tips, 16
traits.  Nothing is asserted on the times.  Prints one JSON line per finished block and the whole result last; with --out it is
also written there (profiles/r12_time_shifts.json), stamped with the hash of csrc/."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import pgbp_amd as P  # noqa: E402
from time_gradient import timed, tree_engine  # noqa: E402


def block(name, ntips, seed, reps):
    p = 16
    cgb, spt, R, rng, nf = tree_engine(ntips, p, 1, seed)
    mu = np.zeros(p)
    lib, eng = cgb._lib, cgb._eng
    cgb.set_schedule([spt])
    n_par = np.asarray(cgb._lg["n_parents"])
    real = np.flatnonzero(n_par >= 1)
    K = cgb._lg["length"].size // len(n_par)

    def assign():
        cgb.assignfactors_lg_(R[None], mu)
        lib.pgbp_sync(eng)

    def shifted(fams):
        e = np.asarray(fams, np.int64) * K
        cgb.set_shifts_lg(e, 0.1 * rng.normal(size=(len(e), p)))
    out = dict(workload=name, tips=ntips, traits=p, clusters=int(cgb.nclusters), families=int(len(n_par)))
    eight = real[np.linspace(0, len(real) - 1, 8).astype(int)]
    for tag, fams in (("0", []), ("8", eight), ("all", real)):
        if len(fams):
            shifted(fams)
        else:
            cgb.clear_shifts_lg()
        out["assignfactors_" + tag] = timed(assign, reps)
        if tag != "all":
            out["loglik_" + tag] = timed(lambda: cgb.loglik_lg(), reps)
    cgb.clear_shifts_lg()

    def one():
        cgb.assignfactors_lg_(R[None], mu)
        cgb.loglik_and_edge_gradient_lg(spt, all_sites=True)
    out["one_evaluation"] = timed(one, reps)
    four = [(int(f), 0) for f in real[np.linspace(0, len(real) - 1, 6).astype(int)[1:5]]]
    t0 = time.perf_counter()
    fit = P.fit_shifts_lg(cgb, spt, four)
    out["fit_4"] = dict(ms=1e3 * (time.perf_counter() - t0), evaluations=4 * p + 2, cond_H=float(np.linalg.cond(fit["H"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_shifts.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [lambda: block("5000-tip tree, 16 traits, clique tree, fixed root, seed 7", 5000, 7, a.reps)]
    if not a.skip_cfg3:
        jobs.append(lambda: block("cfg3: 50000-tip tree, 16 traits, clique tree, fixed root, seed 3", 50000, 3, a.reps))
    for job in jobs:
        res["blocks"].append(job())
        print(json.dumps(res["blocks"][-1]), flush=True)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

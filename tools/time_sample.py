"""Times pgbp_sample_posterior: the factor phase and the apply phase separately, 1 / 16 / 256 draws, against two baselines.

Workloads: cfg3's clique tree (50 000 tips x 16 traits, seed 3), a 5 000-tip 16-trait tree, and the cfg5-size network's
clique tree (20 000 tips, 1 667 blobs, 4 traits, seed 5) -- each calibrated (postorder and preorder) first.
Per workload and number of draws:
  * the whole call (wall time around the synchronous call, median of the repetitions, minimum alongside);
  * pgbp_sample_posterior_timed's phases (the stream drained after each): factor, copy of z, apply, copy of x, and the share
    of the two host copies in their sum;
Baselines, once per workload:
  * pgbp_moments with the covariance over all clusters of the same engine: the cost of one factorisation pass;
  * the same sweep on the host: every belief pulled from the device (pgbp_get_beliefs) and a numpy sweep in the style of
    tests/sample_ref.py, cluster by cluster (Cholesky of J_RR, two triangular solves) -- for ONE draw, the pull included; on the
    large workloads over the first --host-clusters clusters of the preorder only (reported per cluster, not extrapolated).
Draw counts whose z and x would not fit --max-gb of host memory each are skipped and listed under "not_taken".
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
from pgbp_amd import synth as S  # noqa: E402


def f64(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)), "reps": reps}


def host_sweep(cgb, sched, n_clusters_max):
    """the pull of every belief + the numpy sweep of one draw over the first clusters of the preorder"""
    lib, eng, nc = cgb._lib, cgb._eng, cgb.nclusters
    dims = cgb._dims.astype(np.int64)
    poff = cgb._poff
    xoff = np.concatenate([[0], np.cumsum(dims[:nc])])
    pa, ch = sched[-2], sched[-1]
    sep_of = {}
    for k, (a, b) in enumerate(cgb._sepcl):
        sep_of[(int(a), int(b))] = (k, 0, 1)
        sep_of[(int(b), int(a))] = (k, 1, 0)
    order = [(int(pa[0]), None)] + [(int(c), int(q)) for c, q in zip(ch, pa)]
    order = order[:n_clusters_max]
    z = np.random.default_rng(0).standard_normal(int(xoff[-1]))
    x = np.zeros_like(z)
    so, si = cgb._scope_off, cgb._scope_idx
    t0 = time.perf_counter()
    packed = np.zeros(int(poff[-1]))
    assert lib.pgbp_get_beliefs(eng, f64(packed)) == 0
    t_pull = time.perf_counter() - t0
    for c, parent in order:
        m = int(dims[c])
        if m == 0:
            continue
        rec = packed[poff[c]: poff[c + 1]]
        J = rec[: m * m].reshape(m, m, order="F")
        J = np.triu(J) + np.triu(J, 1).T
        h = rec[m * m: m * m + m]
        if parent is None:
            Sx, PS = np.zeros(0, int), np.zeros(0, int)
        else:
            k, cs, ps = sep_of[(c, parent)]
            Sx, PS = si[so[2 * k + cs]: so[2 * k + cs + 1]], si[so[2 * k + ps]: so[2 * k + ps + 1]]
        mask = np.ones(m, bool)
        mask[Sx] = False
        R = np.nonzero(mask)[0]
        xc = x[xoff[c]: xoff[c + 1]]
        xc[Sx] = x[xoff[parent] + PS] if parent is not None else 0.0
        if len(R) == 0:
            continue
        Lc = np.linalg.cholesky(J[np.ix_(R, R)])
        rhs = h[R] - J[np.ix_(R, Sx)] @ xc[Sx]
        xc[R] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs) + z[xoff[c] + R])
    t_all = time.perf_counter() - t0
    return {"pull_ms": 1e3 * t_pull, "pull_MB": packed.nbytes / 1e6, "sweep_ms": 1e3 * (t_all - t_pull),
            "clusters_swept": len(order), "us_per_cluster": 1e6 * (t_all - t_pull) / max(1, len(order)), "draws": 1}


def block(name, cgb, sched, draws_list, reps, max_gb, host_clusters):
    lib, eng, nc = cgb._lib, cgb._eng, cgb.nclusters
    size = int(lib.pgbp_sample_size(eng))
    out = {"workload": name, "clusters": nc, "max_dim": int(cgb._dims[:nc].max()), "sample_size": size,
           "MB_per_draw": size * 8 / 1e6, "draws": {}, "not_taken": []}
    per = int(lib.pgbp_moments_size(eng, 0, None, 1))
    buf, minfo = np.zeros(per), np.zeros(nc, np.int32)

    def mom():
        assert lib.pgbp_moments(eng, 0, None, 0, 1, 1, f64(buf), minfo.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    out["moments_cov"] = timed(mom, reps)
    del buf
    for nd in draws_list:
        if nd * size * 8 > max_gb * 2 ** 30:
            out["not_taken"].append(f"{nd} draws: z and x of {nd * size * 8 / 2 ** 30:.1f} GB each exceed --max-gb {max_gb}")
            continue
        z = np.random.default_rng(nd).standard_normal((nd, 1, size))
        x = np.zeros_like(z)
        info = np.zeros(1, np.int32)
        ip = info.ctypes.data_as(C.POINTER(C.c_int32))

        def call():
            assert lib.pgbp_sample_posterior(eng, 0, 0, 1, nd, f64(z), f64(x), ip) == 0, lib.pgbp_last_error(eng)
        r = timed(call, reps if nd < 256 else max(2, reps // 3))
        assert info[0] == 0 and np.all(np.isfinite(x))
        ms = np.zeros(4)
        phases = []
        for _ in range(3):
            assert lib.pgbp_sample_posterior_timed(eng, 0, 0, 1, nd, f64(z), f64(x), ip, f64(ms)) == 0
            phases.append(ms.copy())
        ph = np.median(np.array(phases), axis=0)
        r.update({"factor_ms": float(ph[0]), "copy_z_ms": float(ph[1]), "apply_ms": float(ph[2]), "copy_x_ms": float(ph[3]),
                  "host_copies_share": float((ph[1] + ph[3]) / ph.sum()),
                  "vs_moments_cov": r["median_ms"] / out["moments_cov"]["median_ms"]})
        out["draws"][str(nd)] = r
        del z, x
    out["host_numpy_sweep"] = host_sweep(cgb, sched, host_clusters)
    return out


def tree_engine(ntips, p, seed):
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    R = S.random_rate_matrix(p, rng)
    prob = S.cliquetree_of_tree(tr, p)
    packed = S.bm_factors_cliquetree(tr, prob, R, np.zeros(p), S.simulate_bm(tr, R, np.zeros(p), rng))
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, packed)
    assert P.calibrate_(cgb, prob.schedule, 1)[0]
    return cgb, prob.schedule[0]


def network_engine(ntips, blobs, p, seed):
    args = argparse.Namespace(seed=seed, traits=p, blob_style="varied", ntips=ntips, blobs=blobs, graph="cliquetree",
                              maxclustersize=3)
    net, (cn, ed, sn), st, fam, X, rates, mu, sched = bench.build_network_workload(args, 0)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(fam, X)
    cgb.assignfactors_lg_(rates, mu, sync=True)
    assert len(sched) == 1 and len(ed) == len(cn) - 1
    assert P.calibrate_(cgb, sched, 1)[0]
    return cgb, sched[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--draws", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--max-gb", type=float, default=4.0, help="largest z (and x) held on the host, GB")
    ap.add_argument("--host-clusters", type=int, default=5000, help="clusters of the preorder the numpy baseline sweeps")
    ap.add_argument("--skip", nargs="*", default=[], choices=["cfg3", "tree5000", "cfg5"])
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_sample.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [("cfg3", "cfg3: 50000-tip tree, 16 traits, clique tree, seed 3", lambda: tree_engine(50000, 16, 3)),
            ("tree5000", "5000-tip tree, 16 traits, clique tree, seed 3", lambda: tree_engine(5000, 16, 3)),
            ("cfg5", "cfg5 size: level-3 network, 20000 tips, 1667 blobs, 4 traits, clique tree, seed 5",
             lambda: network_engine(20000, 1667, 4, 5))]
    for key, name, make in jobs:
        if key in a.skip:
            res.setdefault("not_taken", []).append(name)
            continue
        cgb, sched = make()
        res["blocks"].append(block(name, cgb, sched, a.draws, a.reps, a.max_gb, a.host_clusters))
        del cgb
    print(json.dumps(res))


if __name__ == "__main__":
    main()

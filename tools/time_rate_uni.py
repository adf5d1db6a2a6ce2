"""Times the evolutionary rate matrix between the sites of a univariate batch (pgbp_bm_rate_matrix_sites) on univariate BM
batches with an improper root:
  * sites256: 256 sites on a 2 000-tip tree, the full 256 x 256 matrix;
  * cfg4:     a cfg4-size batch (8 000 sites on a 20 000-tip tree): one 2 048 x 2 048 block and, when the host and the device
              hold it, the full matrix;
  * sites16:  16 sites on the 2 000-tip tree, next to calibrate_exact_cliquetree_ on a multivariate engine of 16 traits.
Per shape, median and minimum of --reps wall times around the C call (outputs allocated beforehand), the phases of the _timed
variant (residual rows, rank-k update, copies; medians over the same number of calls), and the update's fp64 FLOP/s -- of
the entries returned (2 rows cols families4) and as executed (whole tiles; of a square query those on and above the diagonal)
-- next to the fp64 matrix peak of the MI355X's public specification.
Baselines, none of them the code under test: pgbp_bm_exact_stats_sites alone on the same beliefs (what phase one should cost);
the host route a caller had before -- the cluster means fetched with moments_sites_, the residual rows formed and multiplied
with numpy (sites256 only; its result is also compared with the call's); calibrate_exact_cliquetree_ at 16 traits.
Prints one JSON line; profiles/ keeps it, stamped with the hash of csrc/."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import pgbp_amd as P  # noqa: E402
from pgbp_amd import _lib as L  # noqa: E402
from pgbp_amd import synth as S  # noqa: E402
from time_exact_uni import engine, specs, timed  # noqa: E402

FP64_MATRIX_PEAK_TFLOPS = 78.6   # AMD Instinct MI355X, peak double-precision matrix throughput (public data sheet)


def calibrated(cgb, spt):
    """factors of R = 1, mu = 0 and one calibration, as calibrate_rate_matrix_sites_ enqueues them"""
    cgb.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1))
    cgb._loglik_and_sites(spt, lambda: None)


def host_route(cgb, fam, data):
    """U'U on the host: every cluster's posterior means fetched (moments_sites_), the residual rows formed with numpy"""
    mom = cgb.moments_sites_(cov=False)
    ns = cgb.n_sites
    nf = len(fam["cluster"])
    K = max(1, int(fam["max_parents"]))
    npar, cl = np.asarray(fam["n_parents"]), np.asarray(fam["cluster"])
    gam = np.asarray(fam["gamma"], float).reshape(nf, K)
    t = (gam ** 2 * np.asarray(fam["length"], float).reshape(nf, K) * (np.arange(K)[None, :] < npar[:, None])).sum(axis=1)
    U = np.zeros((nf, ns))
    for f in np.flatnonzero((npar > 0) & (t > 0)):
        m = mom[int(cl[f])][0]
        cp = int(fam["child_pos"][f])
        r = m[:, cp].copy() if cp >= 0 else data[:, int(fam["data_row"][f]), 0].copy()
        for k in range(int(npar[f])):
            r -= gam[f, k] * m[:, int(fam["parent_pos"][f * K + k])]
        U[f] = r / np.sqrt(t[f])
    return U.T @ U


def shape(out, cgb, root, rows, cols, reps, nf):
    lib, eng = cgb._lib, cgb._eng
    nr, nc = rows[1] - rows[0], cols[1] - cols[0]
    gram, den, mu, info = np.zeros((nr, nc)), np.zeros(nr + nc), np.zeros(nr + nc), np.zeros(nr + nc, np.int32)
    ms = np.zeros(3)
    args = (eng, rows[0], rows[1], cols[0], cols[1], root[0], root[1], L.f64p(gram), L.f64p(den), L.f64p(mu), L.i32p(info))

    def call():
        assert lib.pgbp_bm_rate_matrix_sites(*args) == L.PGBP_OK, lib.pgbp_last_error(eng)

    def call_timed():
        assert lib.pgbp_bm_rate_matrix_sites_timed(*args, L.f64p(ms)) == L.PGBP_OK, lib.pgbp_last_error(eng)
        return ms.copy()

    out["call"] = timed(call, reps)
    call_timed()
    ph = np.median(np.stack([call_timed() for _ in range(reps)]), axis=0)
    # the flops of the entries returned, and those the device executes: whole 128 x 128 tiles, and of a square query only the
    # tiles on and above the diagonal (the others are copied from their mirror images)
    k4 = (nf + 3) // 4 * 4
    ty, tx = (nr + 127) // 128, (nc + 127) // 128
    tiles = ty * (ty + 1) // 2 if tuple(rows) == tuple(cols) else ty * tx
    out["phases_ms"] = dict(residual_rows=float(ph[0]), update=float(ph[1]), copies=float(ph[2]))
    out["tiles_computed"] = tiles
    out["update_tflops_of_the_entries_returned"] = 2.0 * nr * nc * k4 / (ph[1] * 1e-3) / 1e12
    out["update_tflops_executed"] = 2.0 * tiles * 128 * 128 * k4 / (ph[1] * 1e-3) / 1e12
    out["update_executed_fraction_of_fp64_matrix_peak"] = out["update_tflops_executed"] / FP64_MATRIX_PEAK_TFLOPS
    assert not info.any()
    return gram


def block(name, ntips, ns, seed, reps, queries, host):
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    X = S.simulate_bm_uni_sites(tr, rng.uniform(0.5, 2.0, ns), rng.normal(size=ns), rng)
    sp, spt, root, leaves = specs(tr, X)
    nf = len(sp[0][1]["cluster"])
    out = dict(workload=name, sites=ns, tips=ntips, families=nf, shapes=[])
    cgb = engine(sp[0], ns)
    calibrated(cgb, spt)
    lib, eng = cgb._lib, cgb._eng
    num, den, mh, info = np.zeros(ns), np.zeros(ns), np.zeros(ns), np.zeros(ns, np.int32)

    def sweep_sites():
        assert lib.pgbp_bm_exact_stats_sites(eng, 0, ns, root[0], root[1], L.f64p(num), L.f64p(den), L.f64p(mh), L.i32p(info)) == L.PGBP_OK

    out["exact_stats_sites_alone"] = timed(sweep_sites, reps)
    gram = None
    for rows, cols in queries:
        q = dict(rows=list(rows), cols=list(cols))
        try:
            gram = shape(q, cgb, root, rows, cols, reps, nf)
        except (MemoryError, AssertionError) as err:
            q["not_taken"] = str(err)
        out["shapes"].append(q)
    if host and gram is not None:
        t0 = time.perf_counter()
        G = host_route(cgb, sp[0][1], sp[0][2])
        out["host_route_once_ms"] = 1e3 * (time.perf_counter() - t0)
        G = G[: gram.shape[0], : gram.shape[1]]   # (the last query starts at site 0)
        out["host_route_rel_difference"] = float(np.max(np.abs(G - gram)) / max(1.0, np.max(np.abs(gram))))
    return out, tr, X, leaves


def multivariate(tr, X, leaves, p, reps):
    """calibrate_exact_cliquetree_ on an engine that holds the first p sites as p traits"""
    names = [f"n{i}" for i in range(tr.nnodes)]
    net, nm = P.read_newick(tr.newick(names))
    row = {names[i]: r for r, i in enumerate(leaves)}
    data_row = [row.get(nm[i], -1) for i in range(net.nnodes)]
    cn, ed, sn = P.cliquetree(net.node2family)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=False)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, data_row, p)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=1)
    cgb.lg_setup(fam, np.ascontiguousarray(X[:p, leaves].T[None]))
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    ci = next(i for i, c in enumerate(cn) if 1 in c and st.dims[i] > 0)
    root = (ci, int(st.dims[ci]) - p)
    R = P.calibrate_exact_cliquetree_(cgb, spt, root)[0]
    return timed(lambda: P.calibrate_exact_cliquetree_(cgb, spt, root), reps), R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip", nargs="*", default=[], choices=["sites256", "cfg4", "cfg4full"])
    ap.add_argument("--cfg4-sites", type=int, default=8000)
    ap.add_argument("--cfg4-tips", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_time_rate_uni.json"))
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_rate_uni.py", "csrc_sha16": bench.csrc_sha16(), "fp64_matrix_peak_tflops": FP64_MATRIX_PEAK_TFLOPS,
           "blocks": [], "not_measured": ["several GPUs", "the Julia wrapper"]}
    if "sites256" not in a.skip:
        out, tr, X, leaves = block("256 univariate BM sites on a 2000-tip tree (improper root)", 2000, 256, 9, a.reps,
                                   [((0, 256), (0, 256)), ((0, 16), (0, 16))], True)
        ref, Rm = multivariate(tr, X, leaves, 16, a.reps)
        out["multivariate_engine_16_traits"] = ref
        sp, spt, root, _ = specs(tr, X[:16])
        cgb = engine(sp[0], 16)
        fit = P.calibrate_rate_matrix_sites_(cgb, spt, root)
        out["driver_16_sites"] = timed(lambda: P.calibrate_rate_matrix_sites_(cgb, spt, root), a.reps)
        out["driver_16_against_multivariate_rel"] = float(np.max(np.abs(fit["R"] - Rm)) / max(1.0, np.max(np.abs(Rm))))
        res["blocks"].append(out)
        print(json.dumps(out), file=sys.stderr, flush=True)
    if "cfg4" not in a.skip:
        ns = a.cfg4_sites
        q = [((0, min(2048, ns)), (0, min(2048, ns)))] + ([] if "cfg4full" in a.skip else [((0, ns), (0, ns))])
        out = block(f"cfg4-size: {ns} univariate BM sites on a {a.cfg4_tips}-tip tree (improper root)", a.cfg4_tips, ns, 4, a.reps, q, False)[0]
        res["blocks"].append(out)
        print(json.dumps(out), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

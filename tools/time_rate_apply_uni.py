"""Times the rate matrix of a univariate batch applied to a block of vectors (pgbp_bm_rate_apply_sites) and the leading
phylogenetic principal components on it (phylo_pca_leading_sites), on univariate BM batches with an improper root:
  * sites256: 256 sites on a 2 000-tip tree;
  * cfg4:     a cfg4-size batch (8 000 sites on a 20 000-tip tree).
Per shape and for 16 and 64 vectors: median and minimum of --reps wall times around the C call (outputs allocated
beforehand); the four phases of the _timed variant (residual rows, U v, U' W, copies; medians over the same number of
calls); the bytes per second each product achieves on U (it reads the chunk's U rows once: families4 x sites16 doubles) next
to the HBM3E peak of the MI355X's public specification; and the route before -- pgbp_bm_rate_matrix_sites for the whole
matrix, then gram @ V with numpy.
End to end: phylo_pca_leading_sites with 4 components against phylo_pca_sites (the whole matrix and numpy.linalg.eigh) on the
first --pca-sites sites of the cfg4 batch, and phylo_pca_leading_sites alone on all of them (phylo_pca_sites there only with
--pca-full: a dense eigendecomposition of 8 000 x 8 000 on the host); the data carry four planted Brownian factors (variance
shares 8, 4, 2, 1) on top of the independent per-site BM, so that there are leading components to find; iteration counts kept.
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
from time_rate_uni import calibrated  # noqa: E402

HBM_PEAK_TBS = 8.0   # AMD Instinct MI355X, HBM3E peak bandwidth (public data sheet)
AMPLITUDES = (8.0, 4.0, 2.0, 1.0)


def batch(ntips, ns, seed):
    """(tree, X [sites, nodes]): independent BM per site plus four planted BM factors with standard-normal loadings"""
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    X = S.simulate_bm_uni_sites(tr, rng.uniform(0.5, 2.0, ns), rng.normal(size=ns), rng)
    F = S.simulate_bm_uni_sites(tr, np.array(AMPLITUDES), np.zeros(len(AMPLITUDES)), rng)
    return tr, X + rng.standard_normal((ns, len(AMPLITUDES))) @ F


def apply_shape(cgb, root, ns, nf, k, reps):
    lib, eng = cgb._lib, cgb._eng
    v = np.random.default_rng(k).standard_normal((k, ns))
    gv, den, mu, info = np.zeros((k, ns)), np.zeros(ns), np.zeros(ns), np.zeros(ns, np.int32)
    ms = np.zeros(4)
    args = (eng, 0, ns, k, L.f64p(v), root[0], root[1], L.f64p(gv), L.f64p(den), L.f64p(mu), L.i32p(info))

    def call():
        assert lib.pgbp_bm_rate_apply_sites(*args) == L.PGBP_OK, lib.pgbp_last_error(eng)

    def call_timed():
        assert lib.pgbp_bm_rate_apply_sites_timed(*args, L.f64p(ms)) == L.PGBP_OK, lib.pgbp_last_error(eng)
        return ms.copy()

    out = dict(vectors=k, call=timed(call, reps))
    call_timed()
    ph = np.median(np.stack([call_timed() for _ in range(reps)]), axis=0)
    ubytes = 8.0 * ((nf + 3) // 4 * 4) * ((ns + 15) // 16 * 16)
    out["phases_ms"] = dict(residual_rows=float(ph[0]), u_v=float(ph[1]), ut_w=float(ph[2]), copies=float(ph[3]))
    out["u_bytes"] = ubytes
    out["u_v_tb_per_s_on_u"] = ubytes / (ph[1] * 1e-3) / 1e12
    out["ut_w_tb_per_s_on_u"] = ubytes / (ph[2] * 1e-3) / 1e12
    assert not info.any()
    return out, v, gv


def block(name, tr, X, ns, reps, before):
    sp, spt, root, _ = specs(tr, X[:ns])
    nf = len(sp[0][1]["cluster"])
    out = dict(workload=name, sites=ns, tips=int(np.sum(tr.is_leaf)), families=nf, shapes=[])
    cgb = engine(sp[0], ns)
    calibrated(cgb, spt)
    for k in (16, 64):
        q, v, gv = apply_shape(cgb, root, ns, nf, k, reps)
        if before:
            lib, eng = cgb._lib, cgb._eng
            gram, den, mu, info = np.zeros((ns, ns)), np.zeros(2 * ns), np.zeros(2 * ns), np.zeros(2 * ns, np.int32)

            def route():
                assert lib.pgbp_bm_rate_matrix_sites(eng, 0, ns, 0, ns, root[0], root[1], L.f64p(gram), L.f64p(den), L.f64p(mu),
                                                     L.i32p(info)) == L.PGBP_OK
                return gram @ v.T

            q["route_before_matrix_then_numpy"] = timed(route, max(1, reps // 4))
            q["route_before_rel_difference"] = float(np.max(np.abs(route().T - gv)) / max(1.0, np.max(np.abs(gv))))
        out["shapes"].append(q)
    return out, cgb, spt, root


def pca(cgb, spt, root, full):
    t0 = time.perf_counter()
    lead = P.phylo_pca_leading_sites(cgb, spt, root, 4)
    t1 = time.perf_counter()
    out = dict(sites=cgb.n_sites, components=4, leading_ms=1e3 * (t1 - t0), iterations=int(lead["iterations"]),
               converged=bool(lead["converged"]), explained=[float(x) for x in lead["explained"]],
               worst_residual_over_lambda_1=float(np.max(lead["residuals"]) / lead["values"][0]))
    if full:
        t0 = time.perf_counter()
        ref = P.phylo_pca_sites(cgb, spt, root, n_components=4)
        out["phylo_pca_sites_ms"] = 1e3 * (time.perf_counter() - t0)
        out["values_rel_difference"] = float(np.max(np.abs(ref["values"] - lead["values"])) / ref["values"][0])
    else:
        out["phylo_pca_sites_ms"] = "not taken: a dense eigendecomposition of this order on the host"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip", nargs="*", default=[], choices=["sites256", "cfg4", "pca"])
    ap.add_argument("--cfg4-sites", type=int, default=8000)
    ap.add_argument("--cfg4-tips", type=int, default=20000)
    ap.add_argument("--pca-sites", type=int, default=2048)
    ap.add_argument("--pca-full", action="store_true", help="phylo_pca_sites on all the cfg4 sites too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_time_rate_apply_uni.json"))
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_rate_apply_uni.py", "csrc_sha16": bench.csrc_sha16(), "hbm_peak_tb_per_s": HBM_PEAK_TBS, "blocks": [],
           "pca": [], "not_measured": ["several GPUs", "the Julia wrapper"]}
    if "sites256" not in a.skip:
        tr, X = batch(2000, 256, 9)
        out = block("256 univariate BM sites on a 2000-tip tree (improper root)", tr, X, 256, a.reps, True)[0]
        res["blocks"].append(out)
        print(json.dumps(out), file=sys.stderr, flush=True)
    if "cfg4" not in a.skip:
        ns = a.cfg4_sites
        tr, X = batch(a.cfg4_tips, ns, 4)
        out, cgb, spt, root = block(f"cfg4-size: {ns} univariate BM sites on a {a.cfg4_tips}-tip tree (improper root)", tr, X, ns, a.reps, True)
        res["blocks"].append(out)
        print(json.dumps(out), file=sys.stderr, flush=True)
        if "pca" not in a.skip:
            res["pca"].append(pca(cgb, spt, root, a.pca_full))
            print(json.dumps(res["pca"][-1]), file=sys.stderr, flush=True)
            del cgb
            m = min(ns, a.pca_sites)
            sp, spt, root, _ = specs(tr, X[:m])
            res["pca"].append(pca(engine(sp[0], m), spt, root, True))
            print(json.dumps(res["pca"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

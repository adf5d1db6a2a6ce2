"""Times what a per-site mask of missing tips costs (pgbp_lg_set_site_missing, the correction kernel of csrc/pgbp_sitemiss.hip,
the lanes-are-sites sweeps that read the mask), next to the only route there was before: a pgbp_patterns handle with one
engine per missingness pattern.

Per workload, on one GPU, wall time around synchronous calls (each followed by a stream synchronisation), warm-up first,
median of the repetitions with the minimum alongside:
  assignfactors_{0,1,30}   assignfactors_lg_ + sync with 0 %, 1 % and 30 % of the tip entries masked (0 %: no mask is set,
                           nothing is launched -- the figure to compare with the parent commit's)
  loglik_{0,1,30}          loglik_lg (fill, correction, postorder, root integration)
  gradient_sites_{0,30}    gradient_sites_lg on calibrated beliefs
  impute_sites_30          impute_sites_lg on calibrated beliefs (nothing is listed without a mask)
  set_site_missing_30      the setter itself (checks, packing, two copies, the zeroing kernel)
  patterns_32              (small workload only) loglik_lg of a pgbp_patterns handle over 32 distinct patterns of 8 sites each,
                           the same 256 sites: what such a batch cost before
Workloads: 256 sites on a 2 000-tip tree; cfg4's size (8 000 sites, 20 000 tips; --skip-cfg4 leaves it out), univariate BM,
fixed root, clique tree.  The masked log-likelihoods of three sites are compared with the dense GLS value on the observed tips
(1e-8) before anything is timed.  Nothing is asserted on the times.  Prints one JSON line per finished block and the whole
result last; with --out it is also written there (profiles/r21_time_site_missing.json), stamped with the hash of csrc/."""
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
from pgbp_amd import synth as S  # noqa: E402
from time_gradient import timed  # noqa: E402


def engine(tree, X):
    prob = S.cliquetree_of_tree(tree, 1)
    fam = S.lg_tree_table(tree, prob, 1)
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=X.shape[0])
    cgb.lg_setup(fam, np.ascontiguousarray(X[:, :, None]))
    cgb.set_schedule([prob.schedule[0]])
    return cgb, prob, fam


def gls_loglik(tree, y, obs, s2, mu):
    """dense log-likelihood of a BM with a fixed root on the observed tips (shared path lengths from the parent array)"""
    depth = {}
    anc = {}
    for i in obs:
        path, j = [], int(i)
        while j > 0:
            path.append(j)
            j = int(tree.parent[j])
        anc[int(i)] = path
    length = np.asarray(tree.length, float)
    Cm = np.array([[sum(length[k] for k in set(anc[int(a)]) & set(anc[int(b)])) for b in obs] for a in obs])
    r = y[obs] - mu
    n = len(obs)
    return -0.5 * (n * np.log(2 * np.pi * s2) + np.linalg.slogdet(Cm)[1] + float(r @ np.linalg.solve(Cm, r)) / s2)


def block(name, ntips, nsites, seed, reps, patterns):
    rng = np.random.default_rng(seed)
    tree = S.random_tree(ntips, rng)
    leaf = np.flatnonzero(np.asarray(tree.is_leaf, bool))
    s2, mu = rng.uniform(0.5, 2.0, nsites), rng.normal(size=nsites)
    X = S.simulate_bm_uni_sites(tree, s2, mu, rng)
    cgb, prob, fam = engine(tree, X)
    lib, eng = cgb._lib, cgb._eng
    R, M = s2[:, None, None, None], mu[:, None]

    def assign():
        cgb.assignfactors_lg_(R, M)
        lib.pgbp_sync(eng)

    def mask_of(frac):
        m = np.zeros(X.shape, bool)
        m[:, leaf] = rng.random((nsites, len(leaf))) < frac
        return m
    X3 = np.ascontiguousarray(X[:, :, None])

    def reset():   # (no mask, and the values back at the entries a mask had covered: the device keeps 0.0 there)
        cgb.set_site_missing_lg(None, data=X3)
    out = dict(workload=name, tips=ntips, sites=nsites, clusters=int(cgb.nclusters), families=int(len(fam["cluster"])))
    masks = {"1": mask_of(0.01), "30": mask_of(0.30)}
    if ntips <= 4000:   # the masked log-likelihood against the dense one, three sites
        cgb.set_site_missing_lg(masks["30"])
        assign()
        ll, info = cgb.loglik_lg()
        worst = 0.0
        for s in (0, nsites // 2, nsites - 1):
            obs = leaf[~masks["30"][s, leaf]][:400]
            keep = np.zeros(X.shape[1], bool)
            keep[obs] = True
            m1 = masks["30"].copy()
            m1[s, leaf] = ~keep[leaf]
            reset()
            cgb.set_site_missing_lg(m1)
            assign()
            l1, _ = cgb.loglik_lg()
            want = gls_loglik(tree, X[s], obs, s2[s], mu[s])
            worst = max(worst, abs(l1[s] - want) / max(1.0, abs(want)))
        assert not info.any() and worst <= 1e-8, worst
        out["loglik_masked_vs_dense"] = worst
    for tag in ("0", "1", "30"):
        reset()
        if tag != "0":
            out["masked_entries_" + tag] = int(masks[tag].sum())
            out["set_site_missing_" + tag] = timed(lambda: cgb.set_site_missing_lg(masks[tag]), max(3, reps // 4), warm=1)
        out["assignfactors_" + tag] = timed(assign, reps)
        out["loglik_" + tag] = timed(lambda: cgb.loglik_lg(), reps)
        if tag != "1":
            assign()
            cgb.loglik_and_gradient_sites_lg(prob.schedule[0])     # (calibrated beliefs for the sweeps alone)
            out["gradient_sites_" + tag] = timed(lambda: cgb.gradient_sites_lg(), reps)
        if tag == "30":
            out["impute_sites_30"] = timed(lambda: cgb.impute_sites_lg(), max(3, reps // 4), warm=1)
    if patterns:
        from pgbp_amd.sharding import PatternGroup
        arrays = (prob.dims, np.asarray(prob.sepset_clusters).reshape(-1), prob.scope_off, prob.scope_idx)
        parts = [list(range(k, nsites, patterns)) for k in range(patterns)]
        pats = PatternGroup([arrays + (idx,) for idx in parts])
        pats.set_schedule([prob.schedule[0]])
        for k, idx in enumerate(parts):
            b = pats.beliefs[k]
            b.lg_setup(fam, np.ascontiguousarray(X[idx][:, :, None]))
            b.assignfactors_lg_(R[idx], M[idx])
        out[f"patterns_{patterns}"] = timed(lambda: pats.loglik_lg(), max(3, reps // 4), warm=1)
        out["patterns_sites_per_engine"] = len(parts[0])
        pats.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip-cfg4", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_site_missing.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [lambda: block("256 sites, 2000-tip tree, univariate BM, clique tree, fixed root, seed 21", 2000, 256, 21, a.reps, 32)]
    if not a.skip_cfg4:
        jobs.append(lambda: block("cfg4's size: 8000 sites, 20000-tip tree, univariate BM, clique tree, fixed root, seed 4", 20000, 8000, 4,
                                  a.reps, 0))
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

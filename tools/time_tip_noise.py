"""Times what measurement error at the tips costs (pgbp_lg_set_tip_noise, the correction kernel of csrc/pgbp_noise.hip, dsigma_e
of the gradient sweep), next to what a user had to do before: a pendant node of its own rate colour under every noisy tip,
heterogeneous BM, on the same data.

Per workload, on one GPU, wall time around synchronous calls (each followed by a stream synchronisation), warm-up first,
median of the repetitions with the minimum alongside:
  assignfactors_{0,8,all}  assignfactors_lg_ + sync with no tip, 8 tips, every tip noisy (the fill, and after it the
                           correction of the noisy clusters)
  loglik_{0,8,all}         loglik_lg (fill, postorder, root integration)
  gradient_{0,all}         gradient_lg on calibrated beliefs, without noise (pgbp_lg_gradient) and with every tip noisy
                           (pgbp_lg_gradient_noise: one more block of the slot and of the reduction, dsigma_e)
  pendant_assignfactors, pendant_loglik
                           the same data on the tree with a second node under EVERY tip (twice the tips, two rate colours),
                           no noise set: the workaround for `all`
Workloads, those of tools/time_gradient.py: (a) 5 000-tip tree, 16 traits, clique tree, full BM; (b) cfg3: 50 000 tips, 16
traits.  The two log-likelihoods of `all` and of the pendant engine are compared (1e-8) before anything is timed.  Nothing is
asserted on the times.  Prints one JSON line per finished block and the whole result last; with --out it is also written
there (profiles/r14_time_tip_noise.json), stamped with the hash of csrc/."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import pgbp_amd as P  # noqa: E402
from pgbp_amd import synth as S  # noqa: E402
from time_gradient import timed  # noqa: E402


def engine(nwk, taxa, data, p, pendant_of=None):
    """A one-site fixed-root engine on the clique tree of a Newick tree; pendant_of: names of the leaves that hang on a
    pendant edge (rate colour 1).  Returns (beliefs, schedule tree, family table)."""
    net, nm = P.read_newick(nwk)
    row = {t: r for r, t in enumerate(taxa)}
    data_row = [row.get(nm[i], -1) if net.is_leaf[i] else -1 for i in range(net.nnodes)]
    cn, ed, sn = P.cliquetree(net.node2family)
    pend = set(pendant_of or ())
    pe = [[(t, g, 1 if nm[i] in pend else 0) for t, g in zip(net.length[i], net.gamma[i])] for i in range(net.nnodes)]
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=True)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, data_row, p, n_rates=2 if pend else 1)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(fam, data)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    cgb.set_schedule([spt])
    return cgb, spt, fam


def block(name, ntips, seed, reps):
    p = 16
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    names = [f"n{i}" for i in range(tr.nnodes)]
    leaf = np.asarray(tr.is_leaf, bool)
    taxa = [names[i] for i in range(tr.nnodes) if leaf[i]]
    R = S.random_rate_matrix(p, rng)
    R = (R + R.T) / 2
    sigma_e = S.random_rate_matrix(p, rng)
    sigma_e = 0.2 * (sigma_e + sigma_e.T) / 2
    data = S.simulate_bm(tr, R, np.zeros(p), rng)[leaf]
    mu = np.zeros(p)
    nwk = tr.newick(names)
    cgb, spt, fam = engine(nwk, taxa, data, p)
    lib, eng = cgb._lib, cgb._eng
    tips = np.array([f for f in range(len(fam["cluster"])) if fam["child_pos"][f] < 0 and fam["data_row"][f] >= 0], np.int32)
    scale = 1.0 / rng.integers(1, 9, size=len(tips))
    # the workaround: every tip t becomes the internal node t_x with the leaf t under it on an edge of length scale_t
    by_row = {int(fam["data_row"][f]): s for f, s in zip(tips, scale)}
    row_of = {t: r for r, t in enumerate(taxa)}

    def hang(m):   # (a leaf follows "(" or ",", an internal node's name follows ")")
        t = m.group(2)
        return f"{m.group(1)}({t}:{float(by_row[row_of[t]])!r}){t}_x:" if t in row_of else m.group(0)
    pnwk = re.sub(r"([(,])(n\d+):", hang, nwk)
    pcgb, pspt, pfam = engine(pnwk, taxa, data, p, pendant_of=taxa)
    rates2 = np.stack([R, sigma_e])

    def assign():
        cgb.assignfactors_lg_(R[None], mu)
        lib.pgbp_sync(eng)

    def passign():
        pcgb.assignfactors_lg_(rates2, mu)
        pcgb._lib.pgbp_sync(pcgb._eng)
    out = dict(workload=name, tips=ntips, traits=p, clusters=int(cgb.nclusters), families=int(len(fam["cluster"])),
               pendant_clusters=int(pcgb.nclusters), pendant_families=int(len(pfam["cluster"])))
    assign()
    passign()
    cgb.set_tip_noise_lg(tips, sigma_e, scale)
    ll, info = cgb.loglik_lg()
    pll, pinfo = pcgb.loglik_lg()
    assert not info.any() and not pinfo.any() and abs(ll[0] - pll[0]) <= 1e-8 * abs(pll[0]), (ll, pll)
    out["loglik_all_vs_pendant"] = abs(float(ll[0] - pll[0])) / abs(float(pll[0]))
    eight = np.linspace(0, len(tips) - 1, 8).astype(int)
    for tag, idx in (("0", None), ("8", eight), ("all", np.arange(len(tips)))):
        if idx is None:
            cgb.clear_tip_noise_lg()
        else:
            cgb.set_tip_noise_lg(tips[idx], sigma_e, scale[idx])
        out["assignfactors_" + tag] = timed(assign, reps)
        out["loglik_" + tag] = timed(lambda: cgb.loglik_lg(), reps)
        if tag != "8":
            assign()
            cgb.loglik_and_gradient_lg(spt, all_sites=True)     # (calibrated beliefs for the sweep alone)
            out["gradient_" + tag] = timed(lambda: cgb.gradient_lg(all_sites=True), reps)
    out["pendant_assignfactors"] = timed(passign, reps)
    out["pendant_loglik"] = timed(lambda: pcgb.loglik_lg(), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip-cfg3", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_tip_noise.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
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

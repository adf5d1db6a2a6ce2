"""Times the analytic gradient (pgbp_lg_gradient) against what it replaces: the central-difference gradient of
optimize.py:_minimise, 2 * n_theta evaluations of (assignfactors_lg_ + loglik_lg).

Per workload, on one GPU, wall time around synchronous calls (each returns after its own stream synchronisation), warm-up
first, median of the repetitions with the minimum alongside:
  sweep_alone              gradient_lg on calibrated beliefs (the family sweep, its reduction and the fetch)
  loglik_and_gradient      assignfactors_lg_ + loglik_and_gradient_lg: value and gradient of one optimiser step
  one_loglik_eval          assignfactors_lg_ + loglik_lg: one evaluation of the central-difference route
  central_gradient         the loop of 2 * n_theta such evaluations, actually run (not extrapolated)
  ratio                    central_gradient / loglik_and_gradient (medians)
Workloads: (a) 5 000-tip tree, 16 traits, clique tree, full BM (n_theta = 152); (b) cfg3: 50 000 tips, 16 traits (its slots
are 221 MB: one chunk); (c) the cfg5-size level-3 network's clique tree, 4 traits, 3 rates (n_theta = 34); (d) 256 univariate
OU sites on a 2 000-tip tree (n_theta = 4; per-site parameters).  Prints one JSON line per finished block and the whole
result last; profiles/ keeps it, stamped with the hash of csrc/."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import pgbp_amd as P  # noqa: E402
from pgbp_amd import synth as S  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)), "reps": reps}


def measure(name, cgb, spt, assign, n_theta, reps, extra):
    """assign(): assignfactors_lg_ with the workload's parameters."""
    t0 = time.perf_counter()
    cgb.set_schedule([spt])
    assign()
    ll, g = cgb.loglik_and_gradient_lg(spt, all_sites=True)
    assert not g["info"].any() and np.all(np.isfinite(ll)), name
    ll2, info = cgb.loglik_lg()
    assert np.allclose(ll, ll2, rtol=1e-9, atol=0), (ll[:3], ll2[:3])
    cgb.loglik_and_gradient_lg(spt, all_sites=True)          # (leave calibrated beliefs for the sweep alone)
    out = dict(workload=name, n_theta=n_theta, sites=int(cgb.n_sites), clusters=int(cgb.nclusters), **extra)
    out["first_call_s"] = time.perf_counter() - t0
    out["sweep_alone"] = timed(lambda: cgb.gradient_lg(all_sites=True), reps)

    def value_and_gradient():
        assign()
        cgb.loglik_and_gradient_lg(spt, all_sites=True)

    def one_eval():
        assign()
        cgb.loglik_lg()

    def central():
        for _ in range(2 * n_theta):
            one_eval()
    out["loglik_and_gradient"] = timed(value_and_gradient, reps)
    out["one_loglik_eval"] = timed(one_eval, reps)
    out["central_gradient"] = timed(central, max(3, reps // 4), warm=1)
    out["central_gradient"]["evaluations"] = 2 * n_theta
    out["ratio"] = out["central_gradient"]["median_ms"] / out["loglik_and_gradient"]["median_ms"]
    return out


def tree_engine(ntips, p, ns, seed):
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    names = [f"n{i}" for i in range(tr.nnodes)]
    taxa = [names[i] for i in range(tr.nnodes) if tr.is_leaf[i]]
    net, nm = P.read_newick(tr.newick(names))
    row = {t: r for r, t in enumerate(taxa)}
    data_row = [row.get(nm[i], -1) for i in range(net.nnodes)]
    cn, ed, sn = P.cliquetree(net.node2family)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    leaf = np.asarray(tr.is_leaf, bool)
    R = S.random_rate_matrix(p, rng)
    R = (R + R.T) / 2
    data = np.stack([S.simulate_bm(tr, R, np.zeros(p), rng)[leaf] for _ in range(ns)])
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=True)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, data_row, p)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=ns)
    cgb.lg_setup(fam, data if ns > 1 else data[0])
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    return cgb, spt, R, rng, len(fam["cluster"])


def bm_tree_block(name, ntips, seed, reps):
    p = 16
    cgb, spt, R, rng, nf = tree_engine(ntips, p, 1, seed)
    mu = np.zeros(p)
    return measure(name, cgb, spt, lambda: cgb.assignfactors_lg_(R[None], mu), p * (p + 1) // 2 + p, reps,
                   dict(tips=ntips, traits=p, families=nf, slot_MB=nf * (p * p + p + 4) * 8 / 1e6))


def network_block(reps):
    a = types.SimpleNamespace(seed=5, traits=4, blob_style="template", ntips=20000, blobs=20000 // 12, graph="cliquetree",
                              maxclustersize=3)
    net, (cn, ed, sn), st, fam, X, rates, mu, _ = bench.build_network_workload(a, 0)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(fam, X)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    p, nf = 4, len(fam["cluster"])
    return measure("cfg5-size level-3 network (20000 tips, 5001 reticulations), clique tree, 4 traits, 3 rates", cgb, spt,
                   lambda: cgb.assignfactors_lg_(rates, mu), 3 * (p * (p + 1) // 2) + p, reps,
                   dict(tips=20000, traits=p, families=nf, max_dim=int(max(st.dims)), slot_MB=nf * (p * p + p + 6) * 8 / 1e6))


def ou_block(reps, ns=256, ntips=2000):
    cgb, spt, R, rng, nf = tree_engine(ntips, 1, ns, 9)
    g2 = rng.uniform(0.5, 2, size=(ns, 1, 1, 1))
    al = rng.uniform(0.1, 1, size=ns)
    th = rng.normal(size=(ns, 1))
    mu = rng.normal(size=(ns, 1))
    return measure(f"{ns} univariate OU sites on a {ntips}-tip tree (per-site parameters)", cgb, spt,
                   lambda: cgb.assignfactors_lg_(g2, mu, model="ou", alpha=al, theta=th), 4, reps,
                   dict(tips=ntips, traits=1, families=nf, slot_MB=ns * nf * 6 * 8 / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip-cfg3", action="store_true")
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_gradient.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [lambda: bm_tree_block("5000-tip tree, 16 traits, clique tree, fixed root, seed 7", 5000, 7, a.reps),
            lambda: ou_block(a.reps), lambda: network_block(a.reps)]
    if not a.skip_cfg3:
        jobs.append(lambda: bm_tree_block("cfg3: 50000-tip tree, 16 traits, clique tree, fixed root, seed 3", 50000, 3, a.reps))
    for job in jobs:
        res["blocks"].append(job())
        print(json.dumps(res["blocks"][-1]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

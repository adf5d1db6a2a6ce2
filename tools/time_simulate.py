"""Times pgbp_lg_simulate: the whole call with the device's generator and write_data (what a bootstrap replicate costs), its
factor and apply phases separately, the host-z route, and what a user had to do before.

Workloads (sites are replicates):
  * tree5000: a 5 000-tip 16-trait tree, 64 replicates, shared parameters (the factor phase runs once);
  * cfg3:     the 50 000-tip 16-trait tree, 8 replicates, shared parameters;
  * cfg4:     a cfg4-like univariate batch -- a 20 000-tip tree, 8 000 sites, every site its own OU parameters (one factor
              record per family and site; the states in the [family][site] order).
Per workload:
  * simulate_lg(seed=..., write_data=True): wall time around the synchronous call, median and minimum of the repetitions;
  * pgbp_lg_simulate_timed's phases (the stream drained after each): factor, normals, apply, copies to the host, with x
    fetched and without (x == NULL: the states are scratch only);
  * the host-z route: the same call with z from the host (its upload inside), x fetched;
  * before: a numpy loop over the families in the style of tests/simulate_ref.py for ONE data set (per-family Cholesky; the
    univariate batch vectorised over its sites), and a new lg_setup with that data set -- what every bootstrap replicate,
    cross-validation fold or simulation study paid per data set.
Blocks whose host arrays would not fit --max-gb are skipped and listed under "not_taken".
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


def host_loop(fam, p, R, mu, z, alpha=None, theta=None):
    """One data set per site on the host, family by family: z [sites, n_families, p] -> x; R [sites or 1, n_rates, p, p].
    Trees with a fixed root (one parent per family), vectorised over the sites."""
    nf = len(fam["cluster"])
    pf, t = fam["parent_family"], fam["length"]
    x = np.zeros_like(z)
    for f in range(nf):
        if alpha is None:
            q, v, w = 1.0, t[f], 0.0
        else:
            a = np.exp(-alpha * t[f])
            q, v, w = a, 1.0 - a * a, (1.0 - a)
        Lf = np.linalg.cholesky(np.asarray(v).reshape(-1, 1, 1) * R[:, fam["color"][f]])
        par = mu if pf[f] < 0 else x[:, pf[f]]
        m = np.asarray(q).reshape(-1, 1) * par + (0.0 if theta is None else np.asarray(w).reshape(-1, 1) * theta)
        x[:, f] = m + np.einsum("sij,sj->si", Lf, z[:, f])
    return x


def block(name, cgb, fam, p, kw, reps, max_gb, host_kw):
    lib, eng, ns = cgb._lib, cgb._eng, cgb.n_sites
    nf = len(fam["cluster"])
    out = {"workload": name, "sites": ns, "families": nf, "traits": p, "MB_of_states": ns * nf * p * 8 / 1e6, "not_taken": []}
    out["seed_write_data"] = timed(lambda: cgb.simulate_lg(seed=17, write_data=True, all_sites=True), reps)
    info = np.zeros(ns, np.int32)
    x = np.zeros((ns, nf, p))
    ms = np.zeros(4)
    for key, xp in (("phases_x_fetched", L.f64p(x)), ("phases_x_scratch_only", None)):
        rows = []
        for _ in range(reps):
            assert lib.pgbp_lg_simulate_timed(eng, 0, ns, None, 17, xp, None, 1, L.i32p(info), L.f64p(ms)) == 0
            rows.append(ms.copy())
        ph = np.median(np.array(rows), axis=0)
        out[key] = {"factor_ms": float(ph[0]), "normals_ms": float(ph[1]), "apply_ms": float(ph[2]), "copies_ms": float(ph[3]),
                    "factor_share": float(ph[0] / ph.sum())}
    assert not info.any() and np.all(np.isfinite(x))
    if 2 * x.nbytes > max_gb * 2 ** 30:
        out["not_taken"].append(f"host z: z and x of {x.nbytes / 2 ** 30:.1f} GB each exceed --max-gb {max_gb}")
    else:
        z = np.random.default_rng(1).standard_normal(x.shape)
        out["host_z_write_data"] = timed(lambda: cgb.simulate_lg(z=z, write_data=True, all_sites=True), max(3, reps // 2))
        del z
    # before: the numpy loop for ONE data set (the first site's parameters), and a new set-up with it
    hs = min(ns, host_kw.pop("sites"))
    z1 = np.random.default_rng(2).standard_normal((hs, nf, p))
    t0 = time.perf_counter()
    x1 = host_loop(fam, p, z=z1, **{k: (v[:hs] if k != "mu" or np.ndim(v) == 2 else v) for k, v in host_kw.items()})
    t_loop = time.perf_counter() - t0
    data = cgb.get_data_lg()
    t0 = time.perf_counter()
    cgb.lg_setup(fam, data)
    cgb.assignfactors_lg_(**kw)
    t_setup = time.perf_counter() - t0
    out["before"] = {"numpy_loop_ms": 1e3 * t_loop, "numpy_loop_data_sets": hs, "numpy_loop_ms_per_data_set": 1e3 * t_loop / hs,
                     "lg_setup_and_fill_ms": 1e3 * t_setup, "lg_setup_data_sets": ns,
                     "lg_setup_and_fill_ms_per_data_set": 1e3 * t_setup / ns}
    out["device_ms_per_data_set"] = out["seed_write_data"]["median_ms"] / ns
    del x1
    return out


def tree_engine(ntips, p, n_sites, seed):
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    R = S.random_rate_matrix(p, rng)
    mu = np.zeros(p)
    prob = S.cliquetree_of_tree(tr, p)
    fam = S.lg_tree_table(tr, prob, p)
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=n_sites)
    cgb.set_schedule(prob.schedule)
    cgb.lg_setup(fam, np.zeros((n_sites, tr.nnodes, p)))
    kw = dict(R=R[None], mu=mu)
    cgb.assignfactors_lg_(**kw)
    return cgb, fam, kw, dict(R=R[None, None], mu=mu, sites=1)


def sites_engine(ntips, n_sites, seed):
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    sigma2, alpha = rng.uniform(0.5, 2.0, size=n_sites), rng.uniform(0.1, 1.0, size=n_sites)
    theta, mu = rng.normal(size=n_sites), rng.normal(size=n_sites)
    prob = S.cliquetree_of_tree(tr, 1)
    fam = S.lg_tree_table(tr, prob, 1)
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=n_sites)
    cgb.set_schedule(prob.schedule)
    cgb.lg_setup(fam, np.zeros((n_sites, tr.nnodes, 1)))
    kw = dict(R=(sigma2 / (2.0 * alpha)).reshape(n_sites, 1, 1, 1), mu=mu[:, None], model="ou", alpha=alpha, theta=theta[:, None])
    cgb.assignfactors_lg_(**kw)
    return cgb, fam, kw, dict(R=kw["R"], mu=kw["mu"], alpha=alpha, theta=kw["theta"], sites=256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--max-gb", type=float, default=6.0, help="largest z plus x held on the host, GB")
    ap.add_argument("--skip", nargs="*", default=[], choices=["tree5000", "cfg3", "cfg4"])
    ap.add_argument("--cfg4-sites", type=int, default=8000)
    ap.add_argument("--cfg4-tips", type=int, default=20000)
    a = ap.parse_args()
    P.load()
    res = {"tool": "tools/time_simulate.py", "csrc_sha16": bench.csrc_sha16(), "blocks": []}
    jobs = [("tree5000", "5000-tip tree, 16 traits, 64 replicates, shared parameters", lambda: tree_engine(5000, 16, 64, 3) + (16,)),
            ("cfg3", "cfg3: 50000-tip tree, 16 traits, 8 replicates, shared parameters", lambda: tree_engine(50000, 16, 8, 3) + (16,)),
            ("cfg4", f"cfg4-like: {a.cfg4_tips}-tip tree, {a.cfg4_sites} univariate OU sites with their own parameters",
             lambda: sites_engine(a.cfg4_tips, a.cfg4_sites, 4) + (1,))]
    for key, name, make in jobs:
        if key in a.skip:
            res.setdefault("not_taken", []).append(name)
            continue
        cgb, fam, kw, host_kw, p = make()
        res["blocks"].append(block(name, cgb, fam, p, kw, a.reps, a.max_gb, host_kw))
        del cgb
        print(json.dumps(res["blocks"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Comparators for the simulation sweep (pgbp_lg_simulate / simulate_lg), host side, shared by test_simulate_cpu.py and
test_gpu_simulate.py (tests only).  Neither is the code under test:

`simulate` is a plain numpy loop over the family table with np.linalg.cholesky: it pins the z -> x convention of
include/pgbp.h entry by entry.  `mean_and_map` runs it at z = 0 and at the unit vectors (the sweep is linear in z:
x = m + A z); `dense_moments` gives what m and A A' must be from oracle.densemvn.node_moments, which knows nothing of
families.  `philox4x32_10` / `normals` restate the device's generator in numpy integer arithmetic."""
import numpy as np

from oracle import densemvn as OD
from shift_ref import family_nodes


# ----------------------------------------------------------------------------- the sweep, family by family

def _table(fam):
    nf = len(np.asarray(fam["n_parents"]).reshape(-1))
    K = max(1, np.asarray(fam["length"]).size // max(nf, 1))
    g = lambda k, t: np.asarray(fam[k], t).reshape(nf, K)
    return nf, K, np.asarray(fam["n_parents"]).reshape(-1), g("parent_family", np.int64), g("length", float), g("gamma", float), \
        g("color", np.int64)


def site_kw(kw, s, p, per_site):
    """The keyword arguments of assignfactors_lg_ of one site: R [n_rates, p, p], mu [p], model, alpha, theta [p]."""
    pick = (lambda a: np.asarray(a, float)[s]) if per_site else (lambda a: np.asarray(a, float))
    out = dict(R=pick(kw["R"]).reshape(-1, p, p), mu=pick(kw["mu"]).reshape(p), model=kw.get("model", "bm"))
    if out["model"] == "ou":
        out["alpha"] = float(np.asarray(pick(kw["alpha"])).reshape(-1)[0])
        out["theta"] = pick(kw["theta"]).reshape(p)
    return out


def simulate(fam, kw, z, p, shifts=None, noise=None):
    """fam: a family table with `parent_family` (arrays of factors.lg_families, or ClusterGraphBelief._lg); kw: ONE site's
    parameters (site_kw); z [n_families, p]; shifts: None or (edges [(f, k)], values [n, p]); noise: None or (families [n],
    E [n, p, p]).  Returns x [n_families, p]: x_f = sum_k qc_k x_pf(k) + (sum_k wc_k) theta + sum_k gamma_k s_k + L_f z_f with
    V_f = sum_k vc_k R[colour_k] (+ E_f) = L_f L_f', L_f lower triangular; a parent -1 is mu; a root prior is
    mu + chol(R[colour]) z."""
    nf, K, npar, pf, length, gamma, color = _table(fam)
    R, mu = kw["R"], kw["mu"]
    ou = kw.get("model", "bm") == "ou"
    sh = {(int(f), int(k)): np.asarray(v, float).reshape(p) for (f, k), v in zip(*shifts)} if shifts is not None else {}
    nz = {int(f): np.asarray(E, float).reshape(p, p) for f, E in zip(*noise)} if noise is not None else {}
    z = np.asarray(z, float).reshape(nf, p)
    x = np.zeros((nf, p))
    for f in range(nf):
        if npar[f] == 0:
            m, V = mu.copy(), R[color[f, 0]].copy()
        else:
            m, V, w = np.zeros(p), np.zeros((p, p)), 0.0
            for k in range(npar[f]):
                t, g = length[f, k], gamma[f, k]
                if ou:
                    a = np.exp(-kw["alpha"] * t)
                    qc, vc, wc = g * a, g * g * (1.0 - a * a), g * (1.0 - a)
                else:
                    qc, vc, wc = g, g * g * t, 0.0
                if pf[f, k] == -2:
                    raise ValueError(f"family {f}, parent {k}: an improper root")
                assert pf[f, k] < f
                m = m + qc * (mu if pf[f, k] == -1 else x[pf[f, k]])
                V = V + vc * R[color[f, k]]
                w += wc
                m = m + g * sh.get((f, k), 0.0)
            if ou:
                m = m + w * kw["theta"]
        if f in nz:
            V = V + nz[f]
        x[f] = m + np.linalg.cholesky(V) @ z[f]
    return x


def mean_and_map(fam, kw, p, shifts=None, noise=None, run=None):
    """(m [n_families * p], A [n_families * p, n_families * p]) of x = m + A z.  run(z [B, n_families, p]) -> x [B, ...]: the
    code under test in place of `simulate` (the unit vectors as the rows of one batch)."""
    nf = len(np.asarray(fam["n_parents"]).reshape(-1))
    n = nf * p
    Z = np.concatenate([np.zeros((1, n)), np.eye(n)]).reshape(n + 1, nf, p)
    if run is None:
        X = np.stack([simulate(fam, kw, zz, p, shifts, noise) for zz in Z])
    else:
        X = np.asarray(run(Z))
    X = X.reshape(n + 1, n)
    return X[0].copy(), (X[1:] - X[0]).T.copy()


def dense_moments(net, model, nodes):
    """Prior mean and covariance of the states of `nodes` (preorder indices, family order) from densemvn.node_moments."""
    p = model.dimension()
    mean, cov, _ = OD.node_moments(net, model)
    idx = np.array([i * p + t for i in nodes for t in range(p)], int)
    return mean[idx], cov[np.ix_(idx, idx)]


def rel(a, b):
    """max |a - b| relative to the largest entry of b: the project's parity measure of a block."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def moment_errors(m, A, net, model, nodes):
    dm, dc = dense_moments(net, model, nodes)
    return rel(m, dm) if np.any(dm) else float(np.max(np.abs(m))), rel(A @ A.T, dc)


def tip_rows(fam):
    """[(family, data row, child_mask or None)] of the tip families with a data row."""
    cm = fam.get("child_mask") if hasattr(fam, "get") else None
    return [(f, int(fam["data_row"][f]), None if cm is None else int(cm[f])) for f in range(len(fam["n_parents"]))
            if fam["child_pos"][f] < 0 and fam["data_row"][f] >= 0 and fam["n_parents"][f] >= 1]


# ----------------------------------------------------------------------------- the generator

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011) on arrays: ctr [..., 4], key [..., 2] (integers < 2^32) -> [..., 4]."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # (< 2^64: no wrap)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1)


def uniform53(a, b):
    """((a >> 5) << 26 | b >> 6) + 0.5, times 2^-53: in (0, 1]."""
    k = ((a >> np.uint64(5)) << np.uint64(26)) | (b >> np.uint64(6))
    return (k.astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, sites, nf, p):
    """The device's normals for the absolute sites `sites`: [len(sites), nf, p].  Counter (family, trait pair, site, 0), key
    (seed & 0xffffffff, seed >> 32), u1 from outputs (0, 1), u2 from (2, 3), one Box-Muller pair per counter."""
    sites = np.asarray(sites, np.uint64).reshape(-1)
    npair = (p + 1) // 2
    S, F, Q = np.meshgrid(sites, np.arange(nf, dtype=np.uint64), np.arange(npair, dtype=np.uint64), indexing="ij")
    ctr = np.stack([F, Q, S, np.zeros_like(S)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64), ctr.shape[:-1] + (2,))
    r = philox4x32_10(ctr, key)
    u1, u2 = uniform53(r[..., 0], r[..., 1]), uniform53(r[..., 2], r[..., 3])
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 6.283185307179586 * u2
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(len(sites), nf, 2 * npair)
    return z[:, :, :p].copy()


SEED = 0x5EED0F2024C0FFEE        # the seed of the GPU generator tests
MOMENT_SHAPE = (1681, 78, 1)     # sites, families (loo_ref.batch_case: 40 tips, a fixed root), traits: the first 2^17 are taken


def moment_band(z):
    """(|mean| / its standard error, |variance - 1| / its standard error) of a sample of standard normals."""
    z = np.asarray(z, float).reshape(-1)
    n = z.size
    return abs(float(z.mean())) / np.sqrt(1.0 / n), abs(float(z.var()) - 1.0) / np.sqrt(2.0 / n)


# ----------------------------------------------------------------------------- the cases of both test files

DENSE_CASES = [("hetero_random", 2), ("ou_fixed", 1), ("ou_random", 1), ("bm_fixed", 1), ("bm_random", 4), ("N1_bm", 1),
               ("N1_ou", 1), ("N4_bm", 1), ("N1_p2", 2), ("missing_random", 3), ("missing_fixed", 3), ("tree", 2), ("tree", 16),
               ("tree", 40)]
VARIANTS = ("plain", "shifts", "noise")


def oracle_case(which, p):
    """(net, model, tbl, taxa) of a case of DENSE_CASES: the 24-tip networks of loo_ref.random_case, the hybrid-tip networks of
    uni_net_ref (site 0 of their batches; N1 at p = 2 as test_gpu_tip_noise sets it up), impute_ref.missing_case, and the
    12-tip trees of test_gpu_shifts._tree_case."""
    import impute_ref as IR
    import loo_ref as LR
    import uni_net_ref as N
    from oracle import network as ON
    if which.startswith("N") and which.endswith(("_bm", "_ou")):
        name, kind = which.split("_")
        net, taxa = N.network(name)
        model, tbl = N.sites(name, "fixed", kind)[0]
        return net, model, tbl, taxa
    if which == "N1_p2":
        net, taxa = N.network("N1")
        rng = np.random.default_rng(23)
        model = LR.bm(2, rng, "random")
        return net, model, [list(rng.normal(size=len(taxa))) for _ in range(2)], taxa
    if which.startswith("missing_"):
        return IR.missing_case(which.split("_")[1])
    if which == "tree":
        if p == 16:
            return LR.wavefront_case()
        rng = np.random.default_rng(40 + p)
        tree = ON.random_network(12, 0, rng)
        tbl = [list(rng.normal(size=12)) for _ in range(p)]
        return tree, LR.bm(p, rng, "random"), tbl, tree.tip_names
    return LR.random_case(which, p)


def oracle_table(net, model, tbl, taxa):
    """The family table of an oracle case on its clique tree without a device: (ocgb with the scopes only, fam, data, kw)."""
    import pgbp_amd as P
    from helpers import lg_inputs_from_oracle
    from oracle import beliefs as OB
    from oracle import clustergraph as OCG
    cg = OCG.cliquetree(net)
    b, (n2c, n2f, n2fix, _, c2n) = OB.allocatebeliefs(tbl, taxa, net, cg, model)
    ocgb = OB.ClusterGraphBelief(b, n2c, n2f, n2fix, c2n)
    return (ocgb,) + tuple(lg_inputs_from_oracle(P, net, ocgb, model, tbl, taxa))


def noisy_tips(fam):
    """Every second tip family with a data row, and every tip with several parent edges (a hybrid tip)."""
    tips = [f for f, _, cm in tip_rows(fam) if cm is None or cm != 0]
    return np.array(sorted(set(tips[::2]) | {f for f in tips if fam["n_parents"][f] >= 2}), np.int32)


def variant(net, ocgb, fam, kw, model, p, which):
    """The shifts / noise of a variant of a one-site case: (wrapper model for densemvn, shifts or None, noise or None,
    arguments of set_tip_noise_lg or None).  shifts: test_gpu_shifts._pick / _edges_values; noise: noise_ref.draw_noise."""
    import noise_ref as NR
    from shift_ref import ShiftedModel, family_edge
    from test_gpu_shifts import _edges_values, _pick
    if which == "shifts":
        edges, values = _edges_values(_pick(fam, both_hybrid=True), p)
        w = ShiftedModel(model, {family_edge(net, ocgb, fam, f, k).number: v for (f, k), v in zip(edges, values)})
        return w, (edges, values), None, None
    if which == "noise":
        families = noisy_tips(fam)
        scale, sigma_e, se2 = NR.draw_noise(fam, kw["R"], families, np.random.default_rng(3), model=kw.get("model", "bm"),
                                            alpha=kw.get("alpha"))
        E = NR.tip_noise(scale, sigma_e, se2)
        return NR.wrapper(net, ocgb, fam, model, families, E), None, (families, E), (families, sigma_e, scale, se2)
    return model, None, None, None

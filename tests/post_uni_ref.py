"""Comparators of the lanes-are-sites calls on a fitted univariate batch (pgbp_moments_sites, pgbp_sample_posterior_sites,
pgbp_lg_impute_sites: csrc/pgbp_post_uni.hip), host side, shared by test_post_uni_cpu.py and test_gpu_post_uni.py (tests only).

(a) a numpy restatement of the three calls at p = 1 for ONE site, in the calls' own index convention -- rows of the site-minor
    outputs: `moments_rows` (mean rows, the packed upper triangle S00, S01, S11, norm, info), `sample_rows` (the closed forms of
    a cluster's conditional: r = 1: x_R = (h_R / J_RR - (J_RS / J_RR) x_S) + z_R / sqrt(J_RR); r = 2: a + L^-T z), `impute_rows`
    (mean = E[u] + w, var = u' Sigma u + V, with shifts and tip noise), and `normals` (Philox4x32-10 with the counter
    (entry, draw, site, 1), the cosine branch of Box-Muller);
(b) the independent statements they are pinned to: the dense posterior of all node states (oracle.densemvn, or
    fam_uni_ref.flat_posterior for an improper root) through sample_ref.variable_nodes, sample_ref.sample_posterior_ref,
    impute_ref.dense_impute, simulate_ref's Philox;
(c) the cases of fam_uni_ref both files run, and the margins the GPU tests rely on."""
import functools

import numpy as np

import fam_uni_ref as FR
import impute_ref as IR
import noise_ref as NR
import sample_ref as SR
import simulate_ref as SIM
from edge_ref import edge_coefs
from oracle import beliefs as OB
from oracle import densemvn as OD
from shift_ref import ShiftedModel, family_edge

LOG2PI = FR.LOG2PI


# ----------------------------------------------------------------------------- (a) the restatements, one site

def moments_rows(records, beliefs):
    """records[b] = (J, h, g) of belief b (0, 1 or 2 variables; the upper triangle of J is read); beliefs: the list.
    Returns (mean [sum of dims], tri [sum of m (m + 1) / 2], norm [n], info [n]) -- one site's column of the rows of
    pgbp_moments_sites."""
    mean, tri, norm, info = [], [], [], []
    for b in beliefs:
        J, h, g = records[b]
        m = len(h)
        nz = bool(np.any(J != 0)) or bool(np.any(h != 0))
        if m == 0 or not nz:   # the constant belief; a belief without variables
            mean += [np.inf] * m
            tri += [np.nan] * (m * (m + 1) // 2)
            norm.append(float(g))
            info.append(0)
            continue
        a = J[0, 0]
        if m == 1:
            st = 0 if a > 0 else 1
            S, mu, logdet = [1.0 / a], [h[0] / a], np.log(a) if a > 0 else np.nan
        else:
            b01, d = J[0, 1], J[1, 1]
            ba = b01 / a if a != 0 else np.nan
            sc = d - ba * b01
            st = 0 if (a > 0 and sc > 0) else (2 if a > 0 else 1)
            S11 = 1.0 / sc
            S = [1.0 / a + ba * ba * S11, -(ba * S11), S11]
            m1 = (h[1] - ba * h[0]) / sc
            mu = [(h[0] - b01 * m1) / a, m1]
            logdet = np.log(a) + np.log(sc) if st == 0 else np.nan
        if st:
            mean += [np.nan] * m
            tri += [np.nan] * len(S)
            norm.append(np.nan)
        else:
            mean += mu
            tri += S
            norm.append(float(g) + 0.5 * ((m * LOG2PI - logdet) + float(np.dot(h, mu))))
        info.append(st)
    return np.array(mean, float), np.array(tri, float), np.array(norm, float), np.array(info, np.int32)


def sample_rows(records, dims, sepset_clusters, scope_off, scope_idx, pa, ch, z):
    """The closed forms of pgbp_sample_posterior_sites for one site: records[c] = (J, h[, g]) of cluster c, z [n_draws, size].
    Returns (x [n_draws, size], info) with the conventions of sample_ref.sample_posterior_ref."""
    nc = len(records)
    sepcl = np.asarray(sepset_clusters).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum(np.asarray(dims[:nc], dtype=np.int64))])
    z = np.asarray(z, float)
    x = np.zeros_like(z)
    pa, ch = [int(a) for a in pa], [int(c) for c in ch]
    root = pa[0] if pa else 0
    sep_of = {}
    for k, (a, b) in enumerate(sepcl):
        sep_of[(int(a), int(b))] = (k, 0, 1)
        sep_of[(int(b), int(a))] = (k, 1, 0)
    order = [(root, None)] + list(zip(ch, pa))
    # validity first: info is fixed before anything is written
    plan = []
    for c, parent in order:
        m = int(dims[c])
        if m == 0:
            continue
        J, h = records[c][0], records[c][1]
        S = PS = []
        if parent is not None:
            k, cs, ps = sep_of[(c, parent)]
            S = [int(v) for v in scope_idx[scope_off[2 * k + cs]: scope_off[2 * k + cs + 1]]]
            PS = [int(v) for v in scope_idx[scope_off[2 * k + ps]: scope_off[2 * k + ps + 1]]]
        R = [v for v in range(m) if v not in S]
        if len(R) == 2:
            a, b, d = J[0, 0], J[0, 1], J[1, 1]
            ok = a > 0 and d - (b / a) * b > 0
        elif len(R) == 1:
            ok = J[R[0], R[0]] > 0
        else:
            ok = True
        if not ok:
            return np.full_like(z, np.nan), c + 1
        plan.append((c, parent, m, J, h, R, S, PS))
    for c, parent, m, J, h, R, S, PS in plan:
        xc = x[:, off[c]: off[c + 1]]
        zc = z[:, off[c]: off[c + 1]]
        for j, v in enumerate(S):
            xc[:, v] = x[:, off[parent] + PS[j]]
        if len(R) == 2:
            a, b, d = J[0, 0], J[0, 1], J[1, 1]
            ba = b / a
            sc = d - ba * b
            a1 = (h[1] - ba * h[0]) / sc
            a0 = (h[0] - b * a1) / a
            T00, T11 = 1.0 / np.sqrt(a), 1.0 / np.sqrt(sc)
            T01 = -(ba * T11)
            xc[:, 0] = a0 + (T00 * zc[:, 0] + T01 * zc[:, 1])
            xc[:, 1] = a1 + T11 * zc[:, 1]
        elif len(R) == 1:
            r = R[0]
            Jrr = J[r, r]
            a0, T00 = h[r] / Jrr, 1.0 / np.sqrt(Jrr)
            if S:
                G = J[min(r, S[0]), max(r, S[0])] / Jrr
                xc[:, r] = (a0 - G * xc[:, S[0]]) + T00 * zc[:, r]
            else:
                xc[:, r] = a0 + T00 * zc[:, r]
    return x, 0


def impute_rows(fam, R, mu, moments, model="bm", alpha=None, theta=None, shifts=None, noise=None):
    """One site of pgbp_lg_impute_sites: fam the table at p = 1; moments(c) -> (J^-1 h, J^-1) of cluster c or None; shifts
    {f * K + k: s}; noise {f: E_f}.  Returns dict(families, rows, predicted [n], mean, var, info [n], relV [n] = V / (V + C)...)
    with V and total = u' Sigma u + V of every predicted tip (the margins)."""
    ou = model == "ou"
    K = max(1, int(fam["max_parents"]))
    R = np.asarray(R, float).reshape(-1)
    mu = float(np.ravel(mu)[0])
    th = float(np.ravel(theta)[0]) if ou else 0.0
    shifts, noise = shifts or {}, noise or {}
    fams, pred = IR.listed_families(fam)
    n = len(fams)
    mean, var, V_, tot = (np.full(n, np.nan) for _ in range(4))
    info = np.zeros(n, np.int32)
    for ti, f in enumerate(int(f) for f in fams):
        if not int(pred[ti]) & 1:
            info[ti] = -1
            continue
        npar = int(fam["n_parents"][f])
        ppos = [int(fam["parent_pos"][f * K + k]) for k in range(npar)]
        m, S = np.zeros(2), np.zeros((2, 2))
        if any(q >= 0 for q in ppos):
            mom = moments(int(fam["cluster"][f]))
            if mom is None:
                info[ti] = 1
                continue
            m, S = mom
        u = np.zeros(len(m))
        eu = V = w = 0.0
        for k in range(npar):
            (qc, vc, wc), _, _ = edge_coefs(alpha if ou else None, fam["length"][f * K + k], fam["gamma"][f * K + k])
            V = V + vc * R[int(fam["color"][f * K + k])]
            w = w + wc * th
            eu = eu + qc * (m[ppos[k]] if ppos[k] >= 0 else mu)
            if ppos[k] >= 0:
                u[ppos[k]] += qc
        w = w + sum(fam["gamma"][f * K + k] * shifts.get(f * K + k, 0.0) for k in range(npar))
        V = V + noise.get(f, 0.0)
        C = float(u @ S @ u)
        V_[ti], tot[ti] = V, V + C
        if V > 0:
            mean[ti], var[ti] = eu + w, V + C
        else:
            info[ti] = 1
    return dict(families=fams, rows=np.asarray(fam["data_row"])[fams], predicted=(pred & np.uint64(1)).astype(bool), mean=mean,
                var=var, info=info, V=V_, total=tot)


def normals(seed, sites, size, n_draws):
    """The device's normals of pgbp_sample_posterior_sites for the absolute sites `sites`: [n_draws, size, len(sites)].  Counter
    (entry, draw, site, 1), key (seed & 0xffffffff, seed >> 32), u1 from outputs (0, 1), u2 from (2, 3), the cosine branch."""
    sites = np.asarray(sites, np.uint64).reshape(-1)
    D, E, S = np.meshgrid(np.arange(n_draws, dtype=np.uint64), np.arange(size, dtype=np.uint64), sites, indexing="ij")
    ctr = np.stack([E, D, S, np.ones_like(S)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64), ctr.shape[:-1] + (2,))
    r = SIM.philox4x32_10(ctr, key)
    u1, u2 = SIM.uniform53(r[..., 0], r[..., 1]), SIM.uniform53(r[..., 2], r[..., 3])
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


# ----------------------------------------------------------------------------- (b) the independent statements

def site_model(case, s):
    """the model of site s with the case's shifts and tip noise wrapped in (as fam_uni_ref.dense does)"""
    model, _ = case.sites[s]
    sh = {family_edge(case.net, case.ocgb0, case.fam, f, k).number: np.array([v]) for (f, k), v in FR.site_shifts(case, s).items()}
    w = ShiftedModel(model, sh) if sh else model
    nz = FR.site_noise(case, s)
    if nz:
        fams = sorted(nz)
        w = NR.wrapper(case.net, case.ocgb0, case.fam, w, fams, np.array([nz[f] for f in fams]).reshape(-1, 1, 1))
    return w


def dense_posterior(case, s):
    """(mean, covariance) of all node states of site s given its data, dense: the flat prior for an improper root"""
    model, tbl = case.sites[s]
    w = site_model(case, s)
    return FR.flat_posterior(case.net, w, tbl, case.taxa) if FR.is_improper(model) else OD.posterior_node_moments(case.net, w, tbl, case.taxa)


def layout(case):
    """(dims, sepset_clusters, scope_off, scope_idx, variable nodes of the sample layout, offsets of the clusters in it)"""
    nc = case.ocgb0.nclusters
    _, dims, sepcl, soff, sidx = SR.arrays_from_beliefs(case.ocgb0.belief, nc, OB.scopeindex)
    vn = SR.variable_nodes(case.ocgb0.belief, nc)
    return dims, sepcl, soff, sidx, vn, np.concatenate([[0], np.cumsum(dims[:nc].astype(np.int64))])


def belief_nodes(b):
    """the nodes (0-based preorder indices) of the variables of belief b at p = 1, in the belief's order"""
    insc = np.asarray(b.inscope, bool)
    return np.array([int(lab) - 1 for k, lab in enumerate(b.nodelabel) if insc[0, k]], dtype=int)


def records_of(ocgb):
    return [(np.array(b.J, float), np.array(b.h, float), float(np.ravel(b.g)[0])) for b in ocgb.belief]


def dense_cluster_moments(case, s, cluster):
    """(mean, covariance) of the variables of `cluster` at site s from the dense posterior"""
    dims, _, _, _, vn, off = layout(case)
    pm, pc = dense_posterior(case, s)
    flat = np.array([n for n, _ in vn[off[cluster]: off[cluster + 1]]], dtype=int)
    return pm[flat], pc[np.ix_(flat, flat)]


def dense_impute(case, s):
    """impute_ref.dense_impute of site s under the wrapped model: {taxon row: (mean, var)} of the tips without data"""
    _, tbl = case.sites[s]
    d = IR.dense_impute(case.net, site_model(case, s), tbl, case.taxa)
    return {r: (float(v[1][0]), float(v[2][0, 0])) for r, v in d.items()}


def pivot_margin(records, dims, sepcl, soff, sidx, pa, ch):
    """the smallest pivot of every conditional J_RR of the sweep, relative to its diagonal entry"""
    low = np.inf
    sep_of = {}
    for k, (a, b) in enumerate(np.asarray(sepcl).reshape(-1, 2)):
        sep_of[(int(a), int(b))] = (k, 0)
        sep_of[(int(b), int(a))] = (k, 1)
    root = int(pa[0]) if len(pa) else 0
    for c, parent in [(root, None)] + [(int(c), int(p)) for c, p in zip(ch, pa)]:
        m = int(dims[c])
        J = records[c][0]
        S = []
        if parent is not None:
            k, side = sep_of[(c, parent)]
            S = [int(v) for v in sidx[soff[2 * k + side]: soff[2 * k + side + 1]]]
        R = [v for v in range(m) if v not in S]
        if len(R) == 2:
            low = min(low, 1.0, (J[1, 1] - J[0, 1] ** 2 / J[0, 0]) / J[1, 1])
        elif len(R) == 1:
            low = min(low, 1.0 if J[R[0], R[0]] > 0 else -1.0)
    return low


# ----------------------------------------------------------------------------- (c) the cases

@functools.lru_cache(maxsize=None)
def noisy_missing_case():
    """fam_uni_ref.bm_case(65, True) -- per-site shifts on three edges, per-site noise on every second tip -- with the data of
    one tip that is both noisy and under a shifted edge removed at every site: imputing it predicts the observation."""
    c = FR.bm_case(65, True)
    f = int(c.noise[0][0])
    assert (f, 0) in c.shifts[0]
    row = int(c.fam["data_row"][f])
    sites = [(m, [[None if r == row else v for r, v in enumerate(tbl[0])]]) for m, tbl in c.sites]
    d = FR._case("bm+shifts+noise, a noisy shifted tip without data", c.net, c.taxa, sites, shifts=c.shifts, noise=c.noise)
    for k in ("cluster", "n_parents", "child_pos", "data_row", "parent_pos"):
        assert np.array_equal(d.fam[k], c.fam[k]), k
    d.gone_family = f
    return d


@functools.lru_cache(maxsize=None)
def bm_missing_case():
    """fam_uni_ref.bm_case() (600 sites) with the data of two tips removed at every site: two listed tips, for the
    determinism of the imputation across site ranges and chunks"""
    c = FR.bm_case()
    gone = (0, 5)
    sites = [(m, [[None if r in gone else v for r, v in enumerate(tbl[0])]]) for m, tbl in c.sites]
    return FR._case("bm, two tips without data", c.net, c.taxa, sites)


def cases():
    """every case both files run: (case, the site counts the GPU file runs it at, does it list tips to impute)"""
    yield FR.bm_case(), (8, 64, 65, 257), False
    for root in ("fixed", "random", "improper"):
        yield FR.ou_case(root), (64,), False
    yield FR.missing_case(), (65,), True
    for name in ("N1", "N2", "N3", "N4"):
        for kind in ("bm", "ou"):
            yield FR.hybrid_case(name, kind), (8, 64, 65), False
    yield noisy_missing_case(), (8, 65), True


@functools.lru_cache(maxsize=None)
def shape_case(shape, n):
    """A tree of a given shape, fixed root, 64 sites: "families" -- fam_uni_ref.tree_with_families(n), the 64-belief block
    boundary of the moments and validity kernels --; "caterpillar" -- n tips, many preorder levels of one cluster --;
    "balanced" -- n tips, few wide levels."""
    from pgbp_amd import synth
    from oracle import models as OM
    from oracle import network as ON
    rng = np.random.default_rng(1900 + n)
    if shape == "families":
        tree = FR.tree_with_families(n)
        net, taxa, tipnode = FR._tree_net(tree)
    else:
        def nwk(lo, hi):
            if hi - lo == 1:
                return f"t{lo}:{rng.uniform(0.3, 1.2):.6f}"
            mid = lo + 1 if shape == "caterpillar" else (lo + hi) // 2
            return f"({nwk(lo, mid)},{nwk(mid, hi)}):{rng.uniform(0.3, 1.2):.6f}"
        net = ON.read_newick(nwk(0, n).rsplit(":", 1)[0] + ";")
        taxa = list(net.tip_names)
    ns = 64
    s2, mu = rng.uniform(0.5, 2.0, ns), rng.normal(size=ns)
    sites = []
    for s in range(ns):
        model = OM.UnivariateBrownianMotion(s2[s], mu[s])
        m0, S, _ = OD.node_moments(net, model)
        x = rng.multivariate_normal(m0, S)
        tip = {nd.name: float(x[i]) for i, nd in enumerate(net.vec_node) if nd.leaf}
        sites.append((model, [[tip[t] for t in taxa]]))
    return FR._case(f"{shape} {n}", net, taxa, sites)


SHAPES = [("families", 63), ("families", 64), ("families", 65), ("families", 130), ("caterpillar", 12), ("balanced", 12)]
SEED = 0x5EED0F2026C0FFEE   # the seed of the GPU generator tests

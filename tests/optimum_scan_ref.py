"""Comparators and cases of the optimum-shift scan (pgbp_lg_optimum_scan_sites / optimum_scan_sites_lg), host side, shared by
test_optimum_scan_cpu.py and test_gpu_optimum_scan.py (tests only).  None of them is the code under test.

(a) `recursion`: a numpy restatement of the leaves-to-root recursion over the family table and the DENSE posterior moments of
    each family's cluster (no message passing: what a calibrated clique tree holds), one site.
(b) `gls`: the dense GLS statement.  For the edge above family v, c_v is the derivative of the observed tips' means in an
    increment delta of the optimum of every edge of clade(v), from the preorder recursion dm_c = qc_c dm_parent +
    wc_c [c in clade(v)]; g = c' V^-1 (y - m), H = c' V^-1 c with V and m of the untouched oracle (oracle.densemvn), the painted
    optima, shifts and noise in the wrapper models of optima_ref / shift_ref / noise_ref.  An improper root takes the flat
    prior on the root state: V^-1 is replaced by the projection that removes the root's column.
(c) `loglik_with`: oracle.densemvn.loglik with clade(v) painted by delta on top of everything in force.
(d) the cases both test files run.  A case is one of fam_uni_ref (oracle network, per-site (model, table)) with optional
    per-site shifts and noise, a per-site mask (site_missing_ref) and painted optima (regimes {edge.number: r}, values
    [sites, n_regimes])."""
import functools
import types

import numpy as np

import fam_uni_ref as FR
import loo_ref as LR
import noise_ref as NR
import post_uni_ref as PU
import site_missing_ref as SM
from edge_ref import edge_coefs
from helpers import lg_inputs_from_oracle
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from shift_ref import ShiftedModel, family_edge, family_nodes

MIN_INFO = 1e-8


# ----------------------------------------------------------------------------- the model of a site, wrapped

def _product():
    import pgbp_amd
    return pgbp_amd


def base_of(case):
    return getattr(case, "base", case)


def site_values(case, s):
    return None if getattr(case, "optima", None) is None else np.asarray(case.optima[1][s], float)


def edge_shifts(case, s, extra=None):
    """{edge.number: displacement} of site s: the case's explicit shifts, its painted optima as (1 - a_e)(theta_r - theta),
    and `extra` {edge.number: increment of that edge's optimum}"""
    model, _ = case.sites[s]
    sh = {}
    for (f, k), v in FR.site_shifts(case, s).items():
        n = family_edge(case.net, case.ocgb0, case.fam, f, k).number
        sh[n] = sh.get(n, 0.0) + float(v)
    vals = site_values(case, s)
    for e in case.net.edges:
        d = 0.0
        if vals is not None and case.optima[0].get(e.number, 0) > 0:
            d += vals[case.optima[0][e.number] - 1] - model.theta
        if extra and e.number in extra:
            d += extra[e.number]
        if d != 0.0:
            sh[e.number] = sh.get(e.number, 0.0) + (1.0 - np.exp(-model.alpha * e.length)) * d
    return sh


def site_model(case, s, extra=None):
    model, _ = case.sites[s]
    sh = {n: np.array([v]) for n, v in edge_shifts(case, s, extra).items()}
    w = ShiftedModel(model, sh) if sh else model
    nz = FR.site_noise(case, s)
    if nz:
        fams = sorted(nz)
        w = NR.wrapper(case.net, case.ocgb0, case.fam, w, fams, np.array([nz[f] for f in fams]).reshape(-1, 1, 1))
    return w


def dense_posterior(case, s):
    model, tbl = case.sites[s]
    w = site_model(case, s)
    return FR.flat_posterior(case.net, w, tbl, case.taxa) if FR.is_improper(model) else OD.posterior_node_moments(case.net, w, tbl, case.taxa)


def dense_moments(case, s):
    """moments(c) of the clusters of the graph from the dense posterior of all node states given the observed tips"""
    _, _, _, _, vn, off = PU.layout(case)
    pm, pc = dense_posterior(case, s)

    def mom(c):
        flat = np.array([n for n, _ in vn[off[c]: off[c + 1]]], dtype=int)
        return pm[flat], pc[np.ix_(flat, flat)]
    return mom


def site_table(case, s):
    """(family table with the tips masked at site s skipped, data [n_rows, 1], assignfactors keywords of the site)"""
    b = base_of(case)
    model, tbl = b.sites[s]
    kw = lg_inputs_from_oracle(_product(), case.net, case.ocgb0, model, tbl, case.taxa)[2]
    if getattr(case, "mask", None) is not None:
        fam, data = SM.site_table(case, s)
    else:
        fam = case.fam
        data = np.array([[0.0 if v is None else float(v)] for v in tbl[0]])
    return fam, data, kw


def device_regime(case):
    """the dense map [n_families, K] of set_optima_lg of the case's painting"""
    nf, K = len(case.fam["cluster"]), max(1, int(case.fam["max_parents"]))
    m = np.zeros((nf, K), np.int32)
    if getattr(case, "optima", None) is not None:
        for f in range(nf):
            for k in range(int(case.fam["n_parents"][f])):
                m[f, k] = case.optima[0].get(family_edge(case.net, case.ocgb0, case.fam, f, k).number, 0)
    return m


# ----------------------------------------------------------------------------- (a) the recursion, restated

def children_of(fam):
    nf, K = len(fam["cluster"]), max(1, int(fam["max_parents"]))
    pf = np.asarray(fam["parent_family"]).reshape(nf, K)
    kids = [[] for _ in range(nf)]
    for f in range(nf):
        if int(fam["n_parents"][f]) >= 1 and pf[f, 0] >= 0:
            kids[int(pf[f, 0])].append(f)
    return kids


def heights(fam):
    kids = children_of(fam)
    h = np.zeros(len(kids), int)
    for f in range(len(kids) - 1, -1, -1):
        h[f] = 1 + max(h[c] for c in kids[f]) if kids[f] else 0
    return h


def recursion(fam, data, kw, moments, shifts=None, noise=None, regime=None, values=None, min_info=MIN_INFO):
    """One site.  fam: the table at p = 1 (a family with child_mask == 0 is skipped); kw: R, mu, alpha, theta of the site;
    moments(c) -> (mean, covariance) of cluster c; shifts {f * K + k: s}; noise {f: E_f}; regime [n_families, K] with values
    [n_regimes].  Returns dict(delta, lr, H, Kt, relH = H / Kt, identified, top_lr, top_family) over the families."""
    K, nf = max(1, int(fam["max_parents"])), len(fam["cluster"])
    R = np.asarray(kw["R"], float).reshape(-1)
    mu, th, alpha = float(np.ravel(kw["mu"])[0]), float(np.ravel(kw["theta"])[0]), float(kw["alpha"])
    shifts, noise = shifts or {}, noise or {}
    cm = fam.get("child_mask")
    kids = children_of(fam)
    st = np.zeros((nf, 4))
    delta, lr, H, Kt_, relH = (np.full(nf, np.nan) for _ in range(5))
    for f in range(nf - 1, -1, -1):
        npar, cpos = int(fam["n_parents"][f]), int(fam["child_pos"][f])
        assert npar <= 1, "a tree"
        if (cm is not None and not int(cm[f]) & 1) or (npar == 0 and cpos < 0):
            lr[f] = np.nan if npar == 0 else 0.0
            continue
        if npar == 0:
            continue
        ppos = int(fam["parent_pos"][f * K])
        if cpos >= 0 or ppos >= 0:
            m, S = moments(int(fam["cluster"][f]))
        else:
            m, S = np.zeros(0), np.zeros((0, 0))
        qc, vc, wc = edge_coefs(alpha, fam["length"][f * K], fam["gamma"][f * K])[0]
        V = vc * R[int(fam["color"][f * K])] + noise.get(f, 0.0)
        r = int(regime[f, 0]) if regime is not None else 0
        w = wc * (float(values[r - 1]) if r > 0 else th) + fam["gamma"][f * K] * shifts.get(f * K, 0.0)
        x_c = m[cpos] if cpos >= 0 else float(np.asarray(data, float)[fam["data_row"][f], 0])
        x_u = m[ppos] if ppos >= 0 else mu
        e = x_c - qc * x_u - w
        j = 1.0 / V
        kap = wc * j
        B, Sv, G, Kv = (sum(st[c, i] for c in kids[f]) for i in range(4))
        g, Kt = G + kap * e, Kv + wc * kap
        a, b = kap + B, -kap * qc
        Vu = S[ppos, ppos] if ppos >= 0 else 0.0
        if cpos >= 0:
            Vv = S[cpos, cpos]
            Cvu = S[cpos, ppos] if ppos >= 0 else 0.0
            var = a * a * Vv + 2 * a * b * Cvu + b * b * Vu + Sv
            rho = Cvu / Vu if ppos >= 0 else 0.0
            tau = Vv - Cvu * Cvu / Vu if ppos >= 0 else Vv
            st[f] = (a * rho + b, Sv + a * a * tau, g, Kt)
        else:
            var = b * b * Vu
            st[f] = (b, 0.0, g, Kt)
        Hf = Kt - var
        Kt_[f], relH[f] = Kt, Hf / Kt
        if Hf > min_info * Kt:
            delta[f], lr[f], H[f] = g / Hf, g * g / Hf, Hf
        else:
            lr[f] = 0.0
    ident = ~np.isnan(delta)
    top_lr, top_family = FR.top_of(lr, ident, fam["n_parents"])
    return dict(delta=delta, lr=lr, H=H, Kt=Kt_, relH=relH, identified=ident, top_lr=top_lr, top_family=top_family)


def reference_site(case, s, min_info=MIN_INFO):
    fam, data, kw = site_table(case, s)
    K = max(1, int(fam["max_parents"]))
    shifts = {f * K + k: v for (f, k), v in FR.site_shifts(case, s).items()}
    return recursion(fam, data, kw, dense_moments(case, s), shifts, FR.site_noise(case, s),
                     device_regime(case) if getattr(case, "optima", None) is not None else None, site_values(case, s), min_info)


# ----------------------------------------------------------------------------- (b) the dense GLS statement

def clade_edges(case, f):
    """the oracle edges of clade(f): the edge above family f's node and every edge below it"""
    nd = case.net.vec_node[family_nodes(case.ocgb0, case.fam)[f]]
    out, stack = [family_edge(case.net, case.ocgb0, case.fam, f, 0)], [nd]
    while stack:
        for e in case.net.child_edges(stack.pop()):
            out.append(e)
            stack.append(e.child)
    return out


def _observed(case, s):
    _, tbl = case.sites[s]
    obs, y = [], []
    for i, n in enumerate(case.net.vec_node):
        if n.leaf and tbl[0][case.taxa.index(n.name)] is not None:
            obs.append(i)
            y.append(float(tbl[0][case.taxa.index(n.name)]))
    return np.array(obs, int), np.array(y)


def gls(case, s, families=None):
    """dict(g, H, clade_observed) [n_families] (NaN / False where the family has no parent edge) of site s"""
    model, _ = case.sites[s]
    w = site_model(case, s)
    pre = case.net.vec_node
    pos = {id(n): i for i, n in enumerate(pre)}
    improper = FR.is_improper(model)
    if improper:
        m, V, A = OD.node_moments(case.net, w, np.zeros(1), np.zeros((1, 1)))
    else:
        m, V, A = OD.node_moments(case.net, w)
    obs, y = _observed(case, s)
    Vi = np.linalg.inv(V[np.ix_(obs, obs)])
    if improper:
        Ao = A[obs]
        Vi = Vi - Vi @ Ao @ np.linalg.solve(Ao.T @ Vi @ Ao, Ao.T @ Vi)
    r = y - m[obs]
    nf = len(case.fam["cluster"])
    g, H, seen = np.full(nf, np.nan), np.full(nf, np.nan), np.zeros(nf, bool)
    for f in (range(nf) if families is None else families):
        if int(case.fam["n_parents"][f]) < 1:
            continue
        inside = {e.number for e in clade_edges(case, f)}
        dm = np.zeros(len(pre))
        for i in range(1, len(pre)):
            (e,) = case.net.parent_edges(pre[i])
            a = np.exp(-model.alpha * e.length)
            dm[i] = a * dm[pos[id(e.parent)]] + ((1.0 - a) if e.number in inside else 0.0)
        c = dm[obs]
        g[f], H[f] = float(c @ Vi @ r), float(c @ Vi @ c)
        below = {pos[id(e.child)] for e in clade_edges(case, f)}
        seen[f] = any(i in below for i in obs)
    return dict(g=g, H=H, clade_observed=seen)


def loglik_with(case, s, f=None, delta=0.0):
    """oracle.densemvn.loglik of site s with clade(f) painted by an increment delta of the optimum on top of what is in force"""
    _, tbl = case.sites[s]
    extra = {e.number: float(delta) for e in clade_edges(case, f)} if f is not None else None
    return float(OD.loglik(case.net, site_model(case, s, extra), tbl, case.taxa))


def rel(got, want):
    return FR.rel(got, want)


def against_gls(ref, dn):
    """worst relative difference of g = delta H and H of a restated (or device) site `ref` against the dense statement, over
    the identified families; blocks relative to max(1, |block|)"""
    ok = ref["identified"]
    with np.errstate(divide="ignore", invalid="ignore"):
        want_lr = dn["g"] ** 2 / dn["H"]
    return max(rel((ref["delta"] * ref["H"])[ok], dn["g"][ok]), rel(ref["H"][ok], dn["H"][ok]),
               rel(ref["lr"][ok], want_lr[ok]))


# ----------------------------------------------------------------------------- (d) the cases

def _sample_sites(net, taxa, ns, root, rng, draw="model"):
    """per-site OU parameters and data drawn from the model itself (draw="normal": standard normals, where only bytes are
    compared)"""
    alpha, gam2 = rng.uniform(0.3, 1.5, ns), rng.uniform(0.5, 2.0, ns)
    theta, mu = rng.normal(size=ns), rng.normal(size=ns)
    v = {"fixed": None, "random": 0.8, "improper": np.inf}[root]
    sites = []
    for s in range(ns):
        model = OM.UnivariateOrnsteinUhlenbeck(2 * alpha[s] * gam2[s], alpha[s], theta[s], mu[s], v)
        if draw == "normal":
            sites.append((model, [[float(x) for x in rng.normal(size=len(taxa))]]))
            continue
        prior = OM.UnivariateOrnsteinUhlenbeck(2 * alpha[s] * gam2[s], alpha[s], theta[s], mu[s], 0.8 if root == "improper" else v)
        m0, S, _ = OD.node_moments(net, prior)
        x = rng.multivariate_normal(m0, S)
        tip = {nd.name: float(x[i]) for i, nd in enumerate(net.vec_node) if nd.leaf}
        sites.append((model, [[tip[t] for t in taxa]]))
    return sites


def _net_of_shape(shape, n, rng):
    if shape in ("caterpillar", "balanced"):
        def nwk(lo, hi):
            if hi - lo == 1:
                return f"t{lo}:{rng.uniform(0.3, 1.2):.6f}"
            mid = lo + 1 if shape == "caterpillar" else (lo + hi) // 2
            return f"({nwk(lo, mid)},{nwk(mid, hi)}):{rng.uniform(0.3, 1.2):.6f}"
        net = ON.read_newick(nwk(0, n).rsplit(":", 1)[0] + ";")
        return net, list(net.tip_names)
    if shape == "families":
        net, taxa, _ = FR._tree_net(FR.tree_with_families(n))
        return net, taxa
    from pgbp_amd import synth
    net, taxa, _ = FR._tree_net(synth.random_tree(n, rng))
    return net, taxa


@functools.lru_cache(maxsize=None)
def ou_shape(shape, n, ns=64, root="fixed", seed=0, draw="model"):
    """an OU batch with per-site parameters on a tree of a given shape: "caterpillar" / "balanced" / "random" with n tips,
    "families" with n families (odd n: polytomies)"""
    rng = np.random.default_rng(2600 + 31 * n + seed)
    net, taxa = _net_of_shape(shape, n, rng)
    return FR._case(f"ou {shape} {n} {root}", net, taxa, _sample_sites(net, taxa, ns, root, rng, draw))


def with_shifts_noise(base, seed=0):
    """per-site shifts on three edges and per-site noise on every second tip, the first noisy tip under a shifted edge"""
    rng = np.random.default_rng(2700 + seed)
    c = types.SimpleNamespace(**base.__dict__)
    ns = len(c.sites)
    tips = [int(f) for f in LR.tip_families(c.fam)]
    fams = tips[::2]
    edges = [(fams[0], 0), (fams[-1], 0), (len(c.fam["cluster"]) // 2, 0)]
    c.shifts = (edges, rng.normal(size=(ns, len(edges))))
    K = max(1, int(c.fam["max_parents"]))
    V = np.array([[NR.family_variance(c.fam, np.array([[[m.gamma2]]]), f, "ou", m.alpha) for f in fams] for m, _ in c.sites])
    c.noise = (fams, V.reshape(ns, len(fams)) * rng.uniform(0.05, 2.0, size=(ns, len(fams))))
    c.name = base.name + " + shifts + noise"
    return c


def with_mask(base, n, seed=0):
    mask, pl = SM.draw_mask(base, n, seed=seed, every=False)
    return SM.masked_case(base, mask, pl)


def with_optima(case, seed=0):
    """two regimes painted on two disjoint clades with per-site values: the scan is then the increment"""
    rng = np.random.default_rng(2800 + seed)
    c = types.SimpleNamespace(**case.__dict__)
    nf = len(c.fam["cluster"])
    h = heights(c.fam)
    inner = [f for f in range(nf) if h[f] >= 1 and int(c.fam["n_parents"][f]) == 1]
    a = inner[len(inner) // 3]
    ea = {e.number for e in clade_edges(c, a)}
    b = next(f for f in reversed(inner) if not ea & {e.number for e in clade_edges(c, f)})
    reg = {n: 1 for n in ea}
    reg.update({e.number: 2 for e in clade_edges(c, b)})
    c.optima = (reg, 2.0 * rng.normal(size=(len(c.sites), 2)))
    c.painted = (a, b)
    c.name = case.name + " + 2 regimes"
    return c


@functools.lru_cache(maxsize=None)
def case(key):
    """the cases by name; every one is used by both test files"""
    if key == "main":           # 40 tips, 257 sites: run at 8 (plain layout), 64, 65 and 257 sites
        return ou_shape("random", 40, ns=257)
    if key in ("fixed", "random", "improper"):
        return ou_shape("random", 30, root=key, seed=1)
    if key == "two tips":
        return ou_shape("random", 2, ns=8, seed=2)
    if key in ("caterpillar", "balanced"):
        return ou_shape(key, 12)
    if key.startswith("families"):
        return ou_shape("families", int(key[8:]))
    if key == "shifts+noise":
        return with_shifts_noise(ou_shape("random", 40, ns=65, seed=3))
    if key == "mask":
        return with_mask(ou_shape("random", 40, ns=65, seed=3), 65, seed=4)
    if key == "mask improper":
        return with_mask(ou_shape("random", 30, root="improper", seed=1), 64, seed=5)
    if key == "optima":
        return with_optima(ou_shape("random", 40, ns=65, seed=3), seed=6)
    if key == "everything":     # optima + shifts + noise + mask
        return with_optima(with_mask(with_shifts_noise(ou_shape("random", 40, ns=65, seed=3)), 65, seed=7), seed=8)
    raise KeyError(key)


# (key, the site counts the GPU file runs it at)
CASES = [("main", (8, 64, 65, 257)), ("fixed", (64,)), ("random", (64,)), ("improper", (64,)), ("two tips", (8,)),
         ("caterpillar", (64,)), ("balanced", (64,)), ("families63", (64,)), ("families64", (64,)), ("families65", (64,)),
         ("families130", (64,)), ("shifts+noise", (65,)), ("mask", (65,)), ("mask improper", (64,)), ("optima", (65,)),
         ("everything", (65,))]


def checked_sites(c, n):
    """one site in eight; the planted sites of a mask always"""
    extra = {0, 1, 2, 3, 63, 64} if getattr(c, "mask", None) is not None else set()
    return sorted(x for x in set(range(0, n, 8)) | extra if x < n)

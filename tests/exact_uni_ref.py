"""Cases and comparators of the closed-form BM fit of every site of a univariate batch (pgbp_bm_exact_stats_sites /
bm_exact_stats_sites / calibrate_exact_sites_), host side, shared by test_exact_uni_cpu.py and test_gpu_exact_uni.py (tests only).

(a) `sweep`: a numpy restatement of the family sweep for ONE site -- per family that is not skipped t = sum gamma^2 length,
    r = x_child - sum gamma_k x_k - d (d: the shifts' displacement), e = E[r], C = Var(r), the terms e^2 / t and 1 - C / t added
    in the device's order (blocks of 64 families, then the blocks) -- over the DENSE flat-prior posterior moments of all node
    states given the tips the site observes (fam_uni_ref.flat_posterior: no message passing, what a clique tree calibrated under
    R = 1 and an improper root holds whatever its scopes).
(b) `gls`: per-site generalised least squares on the observed tips -- mu_hat, the REML rate r'C^-1 r / (n_obs - 1), and the
    maximum of the log-likelihood of the fixed-root model -- with the shifts' displacement of the tips taken off the data.
(c) the cases: BM with an improper root (R = 1, mu = 0: what calibrate_exact_sites_ fills) built with the builders of
    fam_uni_ref and site_missing_ref, each with the fixed-root case on the same network for the score; the masks of
    site_missing_ref.draw_mask plus a clade of at least 3 tips wholly masked at one site; every masked site observes at least 3
    tips (asserted when the case is built)."""
import functools
import types

import numpy as np

import fam_uni_ref as FR
import post_uni_ref as PU
import site_missing_ref as SM
from oracle import models as OM
from shift_ref import family_edge

BLOCK = FR.BLOCK
CLADE_SITE = 4   # the site where a whole clade is masked


# ----------------------------------------------------------------------------- (a) the restatement

def sweep(fam, data, moments, shifts=None):
    """One site.  fam: the table at p = 1 (child_mask bit 0 cleared at the tips this site does not observe); data [n_rows, 1];
    moments(c) -> (J^-1 h, J^-1) of cluster c; shifts {f * K + k: s}.  Returns (num, den, terms [n_fam, 2] with NaN at the
    skipped families)."""
    K, nf = max(1, int(fam["max_parents"])), len(fam["cluster"])
    shifts = shifts or {}
    cm, pm = fam.get("child_mask"), fam.get("parent_mask")
    terms = np.full((nf, 2), np.nan)
    for f in range(nf):
        npar, cpos = int(fam["n_parents"][f]), int(fam["child_pos"][f])
        t = 0.0
        for k in range(npar):
            g = float(fam["gamma"][f * K + k])
            t = t + g * g * float(fam["length"][f * K + k])
        if npar == 0 or t == 0.0 or (cm is not None and not int(cm[f]) & 1):
            continue
        if cpos < 0 and pm is not None and int(pm[f * K]) == 0:
            continue
        m, S = moments(int(fam["cluster"][f]))
        if len(m) == 0:
            continue
        u = np.zeros(len(m))
        cst = 0.0
        if cpos >= 0:
            u[cpos] = 1.0
        else:
            cst = float(np.asarray(data, float)[fam["data_row"][f], 0])
        d = 0.0
        for k in range(npar):
            g = float(fam["gamma"][f * K + k])
            u[int(fam["parent_pos"][f * K + k])] -= g
            d = d + g * shifts.get(f * K + k, 0.0)
        e = float(u @ m) + cst - d
        C = float(u @ S @ u)
        terms[f] = (e * e / t, 1.0 - C / t)
    tot = [0.0, 0.0]
    for b in range(0, nf, BLOCK):
        part = [0.0, 0.0]
        for f in range(b, min(b + BLOCK, nf)):
            if not np.isnan(terms[f, 0]):
                part = [part[0] + terms[f, 0], part[1] + terms[f, 1]]
        tot = [tot[0] + part[0], tot[1] + part[1]]
    return tot[0], tot[1], terms


def reference_site(case, s):
    """dict(num, den, mu, terms) of site s: `sweep` over the dense flat-prior posterior of the tips the site observes"""
    if case.mask is None:
        fam = case.fam
        data = np.array([[float(v)] for v in case.sites[s][1][0]])
    else:
        fam, data = SM.site_table(case, s)
    K = max(1, int(fam["max_parents"]))
    shifts = {f * K + k: v for (f, k), v in FR.site_shifts(case, s).items()}
    num, den, terms = sweep(fam, data, SM.dense_moments(case, s), shifts)
    pm, _ = PU.dense_posterior(case, s)
    return dict(num=num, den=den, mu=float(pm[case.root_node]), terms=terms)


@functools.lru_cache(maxsize=None)
def reference(key, n):
    """reference_site of the first n sites of case `key`, as arrays (computed once per case and site count)"""
    case = get(key, n)
    per = [reference_site(case, s) for s in range(n)]
    return {k: np.array([r[k] for r in per]) for k in ("num", "den", "mu")} | dict(terms=np.stack([r["terms"] for r in per]))


# ----------------------------------------------------------------------------- (b) GLS

def tip_displacement(case, s):
    """[n_rows]: the displacement of every tip by the shifts of site s (a tree: the shifts on the edges above the tip)"""
    d = np.zeros(len(case.taxa))
    for (f, k), v in FR.site_shifts(case, s).items():
        ed = family_edge(case.net, case.ocgb0, case.fam, f, k)
        for name in FR._tips_below(case.net, ed.child):
            d[case.taxa.index(name)] += v
    return d


def observed(case, s):
    return np.arange(len(case.taxa)) if case.mask is None else np.flatnonzero(~case.mask[s])


def site_values(case, s):
    """the complete data of site s, [n_rows]"""
    base = case if case.mask is None else case.base
    return np.array([float(v) for v in base.sites[s][1][0]])


def gls(case, s):
    """(mu_hat, REML rate, n_obs, log-likelihood at the ML optimum (mu_hat, REML (n_obs - 1) / n_obs)) of site s"""
    obs = observed(case, s)
    y = site_values(case, s) - tip_displacement(case, s)
    mu, s2, ll = SM.gls_bm(case.cov, y, obs)
    n = len(obs)
    return mu, s2 * n / (n - 1), n, ll


@functools.lru_cache(maxsize=None)
def gls_all(key, n):
    case = get(key, n)
    per = [gls(case, s) for s in range(n)]
    return dict(mu=np.array([p[0] for p in per]), R=np.array([p[1] for p in per]), n_obs=np.array([p[2] for p in per]),
                loglik=np.array([p[3] for p in per]))


# ----------------------------------------------------------------------------- (c) the cases

def _bm(v=None):
    return OM.UnivariateBrownianMotion(1.0, 0.0) if v is None else OM.UnivariateBrownianMotion(1.0, 0.0, v)


def _pair(name, net, taxa, values):
    """The improper-root case of a network and its tip values [n_sites][n_rows] under R = 1, mu = 0, with .fixed (the fixed-root
    case on the same network, for the score), .root (cluster, position of the root variable), .root_node, .cov, .mask = None"""
    free = FR._case(name, net, taxa, [(_bm(np.inf), [[float(x) for x in v]]) for v in values])
    free.fixed = FR._case(name + ", fixed root", net, taxa, [(_bm(), [[float(x) for x in v]]) for v in values])
    free.root_node = next(i for i, nd in enumerate(net.vec_node) if not net.parent_edges(nd))
    _, _, _, _, vn, off = PU.layout(free)
    c = next(c for c in range(len(off) - 1) if any(n == free.root_node for n, _ in vn[off[c]: off[c + 1]]))
    free.root = (c, [n for n, _ in vn[off[c]: off[c + 1]]].index(free.root_node))
    free.cov = SM.bm_cov(free)
    free.mask = None
    free.n = len(values)
    return free


def _values(base, n):
    return [tbl[0] for _, tbl in base.sites[:n]]


@functools.lru_cache(maxsize=None)
def tree40(n=600):
    """the 40-tip tree and the data of fam_uni_ref.bm_case"""
    b = FR.bm_case()
    return _pair("bm40", b.net, b.taxa, _values(b, n))


@functools.lru_cache(maxsize=None)
def shaped(kind, n):
    """the trees of post_uni_ref.shape_case: `n` families (63 / 64 / 65 / 130: the block boundary of the partial sums), a
    caterpillar and a balanced tree of n tips; 64 sites"""
    b = PU.shape_case(kind, n)
    c = _pair(f"{kind}{n}", b.net, b.taxa, _values(b, 64))
    assert kind != "families" or len(c.fam["cluster"]) == n
    return c


@functools.lru_cache(maxsize=None)
def random30():
    """a 30-tip random tree, 65 sites"""
    from pgbp_amd import synth
    rng = np.random.default_rng(415)
    tree = synth.random_tree(30, rng)
    net, taxa, tipnode = FR._tree_net(tree)
    X = synth.simulate_bm_uni_sites(tree, rng.uniform(0.5, 2.0, 65), rng.normal(size=65), rng)
    return _pair("random30", net, taxa, [[X[s, i] for i in tipnode] for s in range(65)])


def _clade(case):
    """the data rows of the tips of a smallest clade of at least 3 tips that leaves at least 3 others"""
    nt = len(case.taxa)
    best = None
    for nd in case.net.vec_node:
        rows = [case.taxa.index(t) for t in FR._tips_below(case.net, nd)]
        if 3 <= len(rows) <= nt - 3 and (best is None or len(rows) < len(best)):
            best = rows
    assert best is not None
    return best


def masked(base, n, seed, min_obs=3):
    """`base` under a mask [n, n_rows]: site_missing_ref.draw_mask (about 30 % at random; site 1 masks nothing; a cherry wholly
    masked at site 2; bits at lanes 0 and 63 and at site 64) plus a clade of at least 3 tips wholly masked at site CLADE_SITE;
    every site observes at least min_obs tips"""
    mask, pl = SM.draw_mask(base, n, seed=seed, every=False)
    rows, _ = SM.tip_rows(base)
    rng = np.random.default_rng(9000 + seed)
    planted = {}
    if pl["cherry"]:
        planted[pl["cherry"][0]] = set(pl["cherry"][2])
    if n > CLADE_SITE:
        cl = _clade(base)
        mask[CLADE_SITE, cl] = True
        planted[CLADE_SITE] = set(cl)
        pl["clade"] = (CLADE_SITE, cl)
    for s in range(n):
        while (~mask[s, rows]).sum() < min_obs:
            mask[s, rng.choice([r for r in rows[mask[s, rows]] if r not in planted.get(s, ())])] = False
    assert np.all((~mask[:, rows]).sum(axis=1) >= min_obs) and not mask[1].any()
    return SM.masked_case(base, mask, pl)


@functools.lru_cache(maxsize=None)
def shifted(n, with_mask):
    """tree40 with per-site shift values on two edges (a pendant edge and an internal one)"""
    b = tree40()
    c = types.SimpleNamespace(**b.__dict__)
    tips = [int(f) for f in FR.LR.tip_families(b.fam)]
    inner = next(f for f in range(len(b.fam["cluster"])) if int(b.fam["child_pos"][f]) >= 0 and int(b.fam["n_parents"][f]) == 1)
    c.shifts = ([(tips[3], 0), (inner, 0)], np.random.default_rng(416).normal(size=(600, 2)) * 2.0)
    c.name = "bm40 + shifts"
    c.sites, c.n = b.sites[:n], n
    return masked(c, n, 50 + n) if with_mask else c


@functools.lru_cache(maxsize=None)
def get(key, n):
    """the case of a key at n sites: "bm40" | "bm40+mask" | "shifts" | "shifts+mask" | "random30[+mask]" | "<kind><n>[+mask]" """
    name, _, m = key.partition("+")
    if name == "shifts":
        return shifted(n, m == "mask")
    if name == "bm40":
        base = tree40()
    elif name == "random30":
        base = random30()
    else:
        kind = name.rstrip("0123456789")
        base = shaped(kind, int(name[len(kind):]))
    if m == "mask":
        return masked(base, n, sum(map(ord, name)) + n)
    c = types.SimpleNamespace(**base.__dict__)
    c.sites, c.n = base.sites[:n], n
    return c


SHAPES = ["families63", "families64", "families65", "families130", "caterpillar12", "balanced12"]
# (key, site counts): 8 sites: the plain layout; 64 and 65: site-minor and the second mask word; 257: a second workgroup
PLAIN = [("bm40", (8, 64, 65, 257)), ("random30", (65,))] + [(k, (64,)) for k in SHAPES]
MASKED = [("bm40+mask", (8, 64, 65, 257)), ("random30+mask", (65,)), ("shifts+mask", (65,)), ("shifts", (64,))] + \
         [(k + "+mask", (64,)) for k in SHAPES]


def smallest_den():
    """the smallest number of observed tips less one over every masked case"""
    low = np.inf
    for key, counts in MASKED:
        for n in counts:
            c = get(key, n)
            if c.mask is not None:
                rows, _ = SM.tip_rows(c)
                low = min(low, int((~c.mask[:, rows]).sum(axis=1).min()) - 1)
    return low

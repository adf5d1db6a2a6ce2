"""Cases and comparators of per-site missing tips in a univariate batch (pgbp_lg_set_site_missing / set_site_missing_lg), host
side, shared by test_site_missing_cpu.py and test_gpu_site_missing.py (tests only).

A masked case is a complete-data case of fam_uni_ref / post_uni_ref (its family table, cluster graph and scopes are those of
the COMPLETE data: a per-site mask changes no scope) plus a mask [n_sites, n_rows]; its `sites` carry None at the masked tips,
which is what every dense statement of the project reads (oracle.densemvn.loglik, posterior_node_moments, fam_uni_ref.dense,
post_uni_ref.dense_impute).

(a) `reference_site`: the numpy restatement with a per-site mask -- fam_uni_ref.sweeps and post_uni_ref.impute_rows on the
    complete table with the masked tips of that site skipped, over the moments of each cluster taken from the DENSE posterior
    of all node states given the observed tips (no message passing: what a calibrated clique tree holds whatever its scopes),
    laid out as the device lays its results out: the leave-one-out over the static tip list with the code NOT_OBSERVED at a
    masked tip and a total in blocks of 64 static tips, the imputation over every tip masked at some site.
(b) `gls_bm`: the closed-form GLS optimum of a BM with a fixed root on the observed tips of a site, its log-likelihood and the
    gradient of the log-likelihood in (sigma2, mu) at any parameters.
(c) the masks: about 30 % at random per site plus the planted entries the issue lists."""
import functools
import types

import numpy as np

import fam_uni_ref as FR
import loo_ref as LR
import post_uni_ref as PU
from helpers import lg_inputs_from_oracle
from oracle import densemvn as OD
from shift_ref import family_nodes

NOT_OBSERVED = -2   # PGBP_INFO_NOT_OBSERVED of include/pgbp.h
BLOCK = FR.BLOCK


# ----------------------------------------------------------------------------- (c) masks and cases

def tip_rows(case):
    """data rows of the tip families of the (complete) table, in family order, and the family of each row"""
    tips = [int(f) for f in LR.tip_families(case.fam)]
    return np.array([int(case.fam["data_row"][f]) for f in tips]), {int(case.fam["data_row"][f]): f for f in tips}


def cherry(case):
    """(family of the internal node, [rows of its two tips]) of a cherry of the network none of whose tips is a hybrid, or None"""
    nodes = family_nodes(case.ocgb0, case.fam)
    for f, i in enumerate(nodes):
        nd = case.net.vec_node[i]
        kids = [e.child for e in case.net.child_edges(nd)]
        if len(kids) == 2 and all(k.leaf and len(case.net.parent_edges(k)) == 1 for k in kids) and int(case.fam["n_parents"][f]) == 1:
            return f, [case.taxa.index(k.name) for k in kids]
    return None


def draw_mask(case, n, seed=0, frac=0.3, every=True):
    """mask [n, n_rows]: about `frac` at random per site, then the planted entries -- site 1 masks nothing; a cherry wholly
    masked at site 2 and observed at sites 1 and 3; one row masked at lanes 0 and 63 of word 0 and at site 64; `every`: one
    tip masked at every site but site 1 -- and at least two observed tips at every site.  Returns (mask, planted) with
    planted = dict(clean=1, cherry=(site, family, rows) or None, every=row or None)."""
    rng = np.random.default_rng(7000 + seed)
    rows, _ = tip_rows(case)
    nr = len(case.taxa)
    mask = np.zeros((n, nr), bool)
    mask[:, rows] = rng.random((n, len(rows))) < frac
    ch = cherry(case)
    planted = dict(clean=1, cherry=None, every=None)
    free = [int(r) for r in rows if ch is None or int(r) not in ch[1]]
    lane_row = free[0]
    mask[0, lane_row] = True
    if n > 63:
        mask[63, lane_row] = True
    if n > 64:
        mask[64, lane_row] = True
    if every:
        planted["every"] = free[1]
        mask[:, free[1]] = True
    if ch is not None and n > 3:
        mask[2, ch[1]] = True
        mask[3, ch[1]] = False
        planted["cherry"] = (2, ch[0], ch[1])
    mask[1] = False
    return at_least_two(mask, rows, rng), planted


def at_least_two(mask, rows, rng, keep=()):
    """unmask tips at random (never the rows `keep`) until every site observes at least two"""
    for s in range(mask.shape[0]):
        while mask[s, rows].sum() > len(rows) - 2:
            mask[s, rng.choice([r for r in rows[mask[s, rows]] if r not in keep])] = False
    return mask


def masked_case(base, mask, planted=None):
    """`base` with the mask: the table, graph and scopes of the complete data, sites with None at the masked tips"""
    n = mask.shape[0]
    sites = [(m, [[None if mask[s, r] else v for r, v in enumerate(tbl[0])]]) for s, (m, tbl) in enumerate(base.sites[:n])]
    c = types.SimpleNamespace(**base.__dict__)
    c.base, c.sites, c.mask, c.planted_mask, c.n = base, sites, mask, planted, n
    c.name = base.name + " + mask"
    return c


@functools.lru_cache(maxsize=None)
def bm(n, every=True):
    base = FR.bm_case()
    mask, pl = draw_mask(base, n, seed=n, every=every)
    return masked_case(base, mask, pl)


@functools.lru_cache(maxsize=None)
def ou(root):
    base = FR.ou_case(root)
    mask, pl = draw_mask(base, 64, seed={"fixed": 1, "random": 2, "improper": 3}[root])
    return masked_case(base, mask, pl)


@functools.lru_cache(maxsize=None)
def shifts_noise(n=65):
    """per-site parameters, shifts and tip noise; the tip masked at every site is a noisy one"""
    base = FR.bm_case(65, True)
    mask, pl = draw_mask(base, n, seed=11, every=False)
    row = int(base.fam["data_row"][int(base.noise[0][0])])
    mask[:, row] = True
    mask[1] = False
    pl["every"] = row
    return masked_case(base, mask, pl)


@functools.lru_cache(maxsize=None)
def hybrid(name, kind, n=65):
    base = FR.hybrid_case(name, kind)
    mask, pl = draw_mask(base, n, seed=20 + int(name[1]), every=False)
    hyb = [base.taxa.index(nd.name) for nd in base.net.vec_node if nd.leaf and len(base.net.parent_edges(nd)) == 2]
    assert hyb                   # the hybrid tip (two parents, a 2-variable sepset) masked at site 5, observed at site 6
    mask[5, hyb[0]], mask[6, hyb[0]] = True, False
    mask = at_least_two(mask, tip_rows(base)[0], np.random.default_rng(int(name[1])), keep=(hyb[0],))
    pl["hybrid"] = hyb[0]
    return masked_case(base, mask, pl)


@functools.lru_cache(maxsize=None)
def shape(kind, n):
    base = PU.shape_case(kind, n)
    mask, pl = draw_mask(base, 64, seed=100 + n)
    return masked_case(base, mask, pl)


def sweep_cases():
    """(case, site counts) of the sweeps' tests: BM at 8 (plain layout), 64, 65 (second mask word) and 257 sites (second
    workgroup); OU with a fixed, random and improper root; shifts + noise; the block boundary; two tree shapes; N1 .. N4"""
    yield "bm", lambda n: bm(n), (8, 64, 65, 257)
    for root in ("fixed", "random", "improper"):
        yield f"ou-{root}", lambda n, root=root: ou(root), (64,)
    yield "shifts+noise", lambda n: shifts_noise(n), (65,)
    for nf in (63, 64, 65):
        yield f"families{nf}", lambda n, nf=nf: shape("families", nf), (64,)
    for k in ("caterpillar", "balanced"):
        yield k, lambda n, k=k: shape(k, 12), (64,)
    for name in ("N1", "N2", "N3", "N4"):
        yield name, lambda n, name=name: hybrid(name, "bm", n), (65,)


def checked_sites(case):
    """one site in eight, site 0 and the planted sites always"""
    return sorted(x for x in set(range(0, case.n, 8)) | {0, 1, 2, 3, 5, 6, 63, 64} if x < case.n)


# ----------------------------------------------------------------------------- (a) the restatement

def site_table(case, s):
    """the complete table with the tips masked at site s skipped (child_mask bit 0 cleared), and the data with 0 there"""
    fam = dict(case.fam)
    cm = np.ones(len(fam["cluster"]), np.uint64) if fam.get("child_mask") is None else np.array(fam["child_mask"], np.uint64)
    _, fam_of = tip_rows(case)
    for r in np.flatnonzero(case.mask[s]):
        cm[fam_of[int(r)]] = 0
    fam["child_mask"] = cm
    data = np.array([[0.0 if case.mask[s, r] else float(v)] for r, v in enumerate(case.base.sites[s][1][0])])
    return fam, data


def dense_moments(case, s):
    """moments(c) of the clusters of the COMPLETE graph from the dense posterior of all node states given the observed tips"""
    _, _, _, _, vn, off = PU.layout(case)
    pm, pc = PU.dense_posterior(case, s)

    def mom(c):
        flat = np.array([n for n, _ in vn[off[c]: off[c + 1]]], dtype=int)
        return pm[flat], pc[np.ix_(flat, flat)]
    return mom


def block_total_masked(lpd, masked):
    """the device's total: blocks of 64 STATIC tips, the tips of a block added in order, a masked tip adding nothing"""
    acc = 0.0
    for b in range(0, len(lpd), BLOCK):
        part = 0.0
        for v, m in zip(lpd[b:b + BLOCK], masked[b:b + BLOCK]):
            if not m:
                part = part + v
        acc = acc + part
    return float(acc)


def site_kw(case, s):
    import pgbp_amd
    model, tbl = case.base.sites[s]
    return lg_inputs_from_oracle(pgbp_amd, case.net, case.ocgb0, model, tbl, case.taxa)[2]


def reference_site(case, s, min_info=1e-8, moments=None):
    """The three family sweeps and the imputation of site s, restated, in the device's layout: dict(scan, edge, loo, impute)."""
    fam, data = site_table(case, s)
    kw = site_kw(case, s)
    K = max(1, int(fam["max_parents"]))
    mom = moments or dense_moments(case, s)
    shifts = {f * K + k: v for (f, k), v in FR.site_shifts(case, s).items()}
    noise = FR.site_noise(case, s)
    sw = FR.sweeps(fam, data, kw["R"], kw["mu"], mom, kw.get("model", "bm"), kw.get("alpha"), kw.get("theta"), shifts, noise, min_info)
    # the leave-one-out over the static tip list
    static = [int(f) for f in LR.tip_families(case.fam)]
    live = {int(f): i for i, f in enumerate(sw["loo"]["families"])}
    nt = len(static)
    lo = dict(families=np.array(static, np.int32), mean=np.full(nt, np.nan), var=np.full(nt, np.nan), lpd=np.full(nt, np.nan),
              relD=np.full(nt, np.nan), info=np.full(nt, NOT_OBSERVED, np.int32))
    for ti, f in enumerate(static):
        if f in live:
            for k in ("mean", "var", "lpd", "relD", "info"):
                lo[k][ti] = sw["loo"][k][live[f]]
    lo["masked"] = lo["info"] == NOT_OBSERVED
    lo["total"] = block_total_masked(lo["lpd"], lo["masked"])
    # the imputation over every tip masked at some site (this module's cases have no statically missing tip)
    _, fam_of = tip_rows(case)
    listed = sorted(fam_of[int(r)] for r in np.flatnonzero(case.mask.any(axis=0)))
    fi = dict(fam)
    fi["parent_mask"] = np.ones(len(fam["cluster"]) * K, np.uint64) if fam.get("parent_mask") is None else fam["parent_mask"]
    ir = PU.impute_rows(fi, kw["R"], kw["mu"], mom, kw.get("model", "bm"), kw.get("alpha"), kw.get("theta"), shifts, noise)
    at = {int(f): i for i, f in enumerate(ir["families"])}
    im = dict(families=np.array(listed, np.int32), rows=np.asarray(case.fam["data_row"])[listed], mean=np.full(len(listed), np.nan),
              var=np.full(len(listed), np.nan), info=np.full(len(listed), NOT_OBSERVED, np.int32))
    for i, f in enumerate(listed):
        if f in at:
            im["mean"][i], im["var"][i], im["info"][i] = ir["mean"][at[f]], ir["var"][at[f]], ir["info"][at[f]]
    return dict(scan=sw["scan"], edge=sw["edge"], loo=lo, impute=im, raw=sw), fam


def dense_site(case, s, min_info=1e-8):
    """fam_uni_ref.dense with None at the masked tips of site s (the table is the complete one: family -> node, edges)"""
    model, tbl = case.sites[s]
    return FR.dense(case.net, case.ocgb0, case.fam, model, tbl, case.taxa, FR.site_shifts(case, s), FR.site_noise(case, s), min_info)


def dense_loglik(case, s):
    model, tbl = case.sites[s]
    return float(OD.loglik(case.net, PU.site_model(case, s), tbl, case.taxa))


# ----------------------------------------------------------------------------- (b) BM with a fixed root, closed form

def bm_cov(case):
    """C [n_rows, n_rows] with Cov(tips) = sigma2 C under a BM with a fixed root, rows in taxon order"""
    from oracle import models as OM
    m0, S, _ = OD.node_moments(case.net, OM.UnivariateBrownianMotion(1.0, 0.0))
    at = {nd.name: i for i, nd in enumerate(case.net.vec_node)}
    idx = [at[t] for t in case.taxa]
    return S[np.ix_(idx, idx)]


def gls_bm(C, y, obs, sigma2=None, mu=None):
    """observed rows `obs`: (mu_hat, sigma2_hat, loglik at the optimum) or, with parameters given, (loglik, dll/dsigma2, dll/dmu)"""
    Co, yo = C[np.ix_(obs, obs)], np.asarray(y, float)[obs]
    n = len(yo)
    one = np.ones(n)
    Ci1, Ciy = np.linalg.solve(Co, one), np.linalg.solve(Co, yo)
    ld = np.linalg.slogdet(Co)[1]
    if sigma2 is None:
        mu_h = float(one @ Ciy) / float(one @ Ci1)
        r = yo - mu_h
        s2 = float(r @ np.linalg.solve(Co, r)) / n
        return mu_h, s2, -0.5 * (n * np.log(2 * np.pi) + n * np.log(s2) + ld + n)
    r = yo - mu
    q = float(r @ np.linalg.solve(Co, r))
    ll = -0.5 * (n * np.log(2 * np.pi) + n * np.log(sigma2) + ld + q / sigma2)
    return ll, -0.5 * n / sigma2 + 0.5 * q / sigma2 ** 2, float(one @ np.linalg.solve(Co, r)) / sigma2

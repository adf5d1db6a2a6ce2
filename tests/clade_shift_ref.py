"""Comparators of the per-site clade shifts of the OU optimum (pgbp_lg_set_clade_shifts_sites and the calls around it), host
side, shared by test_clade_shift_cpu.py and test_gpu_clade_shifts.py (tests only).  None of them is the code under test.

A setting is (family [n_slots, n_sites], delta [n_slots, n_sites]), -1 = an empty slot.  At one site it is the same model as
painted optima that give every edge of the union of the site's clades a regime of its own, at (theta or the painted value) +
the sum of the deltas whose clade holds the edge -- `painted(case, s, family, delta)` builds that case, and everything of
optimum_scan_ref then applies to it unchanged:
(1) the dense log-likelihood (oracle.densemvn through shift_ref.ShiftedModel with the equivalent explicit shifts
    (1 - exp(-alpha t_e)) sum_j delta_j [e in clade(v_j)]), the dense posterior moments of every cluster, the restated scan;
(2) the dense GLS statement: the design C (observed tips x slots) by the preorder recursion of optimum_scan_ref.gls,
    g = C' V^-1 (y - m), H = C' V^-1 C, the joint solve and a greedy path built from it;
(3) an existing engine painted with `device_painting` (set_optima_lg), for the records."""
import functools
import types

import numpy as np

import fam_uni_ref as FR
import optimum_scan_ref as OS
from oracle import densemvn as OD

MIN_INFO = OS.MIN_INFO


def slots_of(family, delta, s):
    """[(family, delta)] of the used slots of site s, in slot order"""
    return [(int(v), float(d)) for v, d in zip(np.asarray(family)[:, s], np.asarray(delta)[:, s]) if v >= 0]


def painted(case, s, family, delta):
    """the case whose painted optima ARE site s's model under the setting (the other sites' values are copies of site s's:
    only site s is to be read)"""
    c = types.SimpleNamespace(**case.__dict__)
    reg = dict(case.optima[0]) if getattr(case, "optima", None) is not None else {}
    old = OS.site_values(case, s)
    theta = case.sites[s][0].theta
    add = {}
    for v, d in slots_of(family, delta, s):
        for e in OS.clade_edges(case, v):
            add[e.number] = add.get(e.number, 0.0) + d
    vals = [] if old is None else [float(x) for x in old]
    new = dict(reg)
    for number in sorted(add):
        r = reg.get(number, 0)
        vals.append((vals[r - 1] if r > 0 else theta) + add[number])
        new[number] = len(vals)
    if not vals:
        c.optima = None
        return c
    c.optima = (new, np.tile(np.array(vals), (len(case.sites), 1)))
    return c


def device_painting(case, s, family, delta):
    """(regime map [n_families, K], values [n_regimes]) of set_optima_lg for site s's model"""
    c = painted(case, s, family, delta)
    return OS.device_regime(c), np.asarray(c.optima[1][s], float)


def loglik(case, s, family, delta):
    return OS.loglik_with(painted(case, s, family, delta), s)


def reference_scan(case, s, family, delta):
    """the restated scan of site s with the setting in force"""
    return OS.reference_site(painted(case, s, family, delta), s)


def dense_parts(case, s, family, delta):
    """(Vi, r, column): the (projected) inverse covariance of the observed tips, the residual y - m under the setting, and
    column(f) = the derivative of the observed tips' means in an increment of the optimum of clade(f)"""
    c = painted(case, s, family, delta)
    model, _ = c.sites[s]
    w = OS.site_model(c, s)
    pre = c.net.vec_node
    pos = {id(n): i for i, n in enumerate(pre)}
    improper = FR.is_improper(model)
    if improper:
        m, V, A = OD.node_moments(c.net, w, np.zeros(1), np.zeros((1, 1)))
    else:
        m, V, A = OD.node_moments(c.net, w)
    obs, y = OS._observed(c, s)
    Vi = np.linalg.inv(V[np.ix_(obs, obs)])
    if improper:
        Ao = A[obs]
        Vi = Vi - Vi @ Ao @ np.linalg.solve(Ao.T @ Vi @ Ao, Ao.T @ Vi)

    def column(f):
        inside = {e.number for e in OS.clade_edges(c, f)}
        dm = np.zeros(len(pre))
        for i in range(1, len(pre)):
            (e,) = c.net.parent_edges(pre[i])
            a = np.exp(-model.alpha * e.length)
            dm[i] = a * dm[pos[id(e.parent)]] + ((1.0 - a) if e.number in inside else 0.0)
        return dm[obs]
    return Vi, y - m[obs], column


def dense_score(case, s, family, delta):
    """g [slots used], H [used, used] of site s at the setting, over its used slots in slot order"""
    Vi, r, column = dense_parts(case, s, family, delta)
    C = np.array([column(v) for v, _ in slots_of(family, delta, s)]).T.reshape(len(r), -1)
    return C.T @ Vi @ r, C.T @ Vi @ C


def relative_pivots(H):
    """the pivots of the elimination of H in slot order, each relative to its diagonal entry"""
    A = np.array(H, float)
    out = []
    for k in range(len(A)):
        out.append(A[k, k] / H[k, k] if H[k, k] > 0 else 0.0)
        if A[k, k] > 1e-14 * H[k, k]:
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:]) / A[k, k]
        A[k + 1:, k] = A[k, k + 1:] = 0.0
    return np.array(out)


def dense_fit(case, s, family, delta):
    """the joint ML of the used slots' deltas: dict(delta, H, se, loglik, pivot) with pivot the smallest relative pivot of
    the elimination of H in slot order; singular (pivot < 1e-10: the slots are not jointly identified): H and pivot only"""
    g, H = dense_score(case, s, family, delta)
    d0 = np.array([d for _, d in slots_of(family, delta, s)])
    if len(d0) == 0:
        return dict(delta=d0, H=H, se=d0, loglik=loglik(case, s, family, delta), pivot=np.inf, singular=False)
    pivot = float(relative_pivots(H).min())
    if pivot < 1e-10:
        return dict(H=H, pivot=pivot, singular=True)
    d = d0 + np.linalg.solve(H, g)
    new = np.asarray(delta, float).copy()
    new[np.asarray(family)[:, s] >= 0, s] = d
    return dict(delta=d, H=H, se=np.sqrt(np.diag(np.linalg.inv(H))), loglik=loglik(case, s, family, new), pivot=pivot, singular=False)


def dense_candidates(case, s, family, delta):
    """lr [n_families] of the next increment at the setting: g^2 / H where the clade observes a tip, -inf elsewhere"""
    Vi, r, column = dense_parts(case, s, family, delta)
    nf = len(case.fam["cluster"])
    lr = np.full(nf, -np.inf)
    obs, _ = OS._observed(case, s)
    pos = {id(n): i for i, n in enumerate(case.net.vec_node)}
    for f in range(nf):
        if int(case.fam["n_parents"][f]) < 1:
            continue
        below = {pos[id(e.child)] for e in OS.clade_edges(case, f)}
        if not any(i in below for i in obs):
            continue
        c = column(f)
        lr[f] = float(c @ Vi @ r) ** 2 / float(c @ Vi @ c)
    return lr


def dense_greedy(case, s, max_shifts, min_lr):
    """forward selection at site s from the dense statement alone: dict(family, delta, lr, loglik, gap) with gap the
    smallest (largest lr - second largest) / largest over the steps taken"""
    n = len(case.sites)
    fam = np.full((max_shifts, n), -1)
    delta = np.zeros((max_shifts, n))
    lrs, path, gap = [], [loglik(case, s, fam, delta)], np.inf
    for step in range(max_shifts):
        lr = dense_candidates(case, s, fam, delta)
        f = int(np.argmax(lr))
        if not lr[f] > min_lr:
            break
        two = np.sort(lr)[-2:]
        gap = min(gap, float((two[1] - two[0]) / two[1]))
        fam[step, s] = f
        lrs.append(float(lr[f]))
        fit = dense_fit(case, s, fam, delta)
        delta[:step + 1, s] = fit["delta"]
        path.append(fit["loglik"])
    k = len(lrs)
    return dict(family=fam[:, s].copy(), delta=delta[:, s].copy(), lr=np.array(lrs), loglik=np.array(path), n_shifts=k, gap=gap)


# ----------------------------------------------------------------------------- settings the tests use

def clade_tips(case, f):
    """does clade(f) consist of a single tip?"""
    return len(OS.clade_edges(case, f)) == 1


def draw_setting(case, n, n_slots, seed=0):
    """family / delta [n_slots, n] with 0, 1 and all slots used at different sites: site 1 none, site 2 one, site 0 and every
    fourth site all; the rest a random number.  Site 0: a clade nested inside another, then disjoint ones; site 3: a single
    tip.  Lanes 0 and 63 and site 64 (where they exist) carry slot 0."""
    rng = np.random.default_rng(2900 + seed)
    nf = len(case.fam["cluster"])
    real = [f for f in range(nf) if int(case.fam["n_parents"][f]) >= 1]
    h = OS.heights(case.fam)
    kids = OS.children_of(case.fam)
    fam = np.full((n_slots, n), -1, np.int32)
    for s in range(n):
        k = n_slots if (s % 4 == 0 or s in (63, 64)) else (0 if s == 1 else (1 if s == 2 else int(rng.integers(0, n_slots + 1))))
        pick = [int(x) for x in rng.choice(real, size=min(k, len(real)), replace=False)]
        if s == 0 and n_slots >= 2:
            outer = [f for f in real if h[f] >= 1]
            if outer:
                a = outer[len(outer) // 2]
                pick = [a, kids[a][0]] + [f for f in pick if f not in (a, kids[a][0])][: n_slots - 2]
        if s == 3 and pick:
            tip = next(f for f in real if h[f] == 0)
            pick = [tip] + [f for f in pick if f != tip][: len(pick) - 1]
        fam[:len(pick), s] = pick
    delta = np.where(fam >= 0, rng.normal(size=fam.shape) * 1.5, 0.0)
    return fam, delta


def _plant_in_case(case, fam, n):
    """the configurations the issue names, where the case has them: a noisy tip inside a shifted clade (site 4), a cherry
    wholly masked inside a shifted clade and as a slot of its own (the planted site of the mask)"""
    nf = len(case.fam["cluster"])
    pf = np.asarray(case.fam["parent_family"]).reshape(nf, -1)[:, 0]
    real = np.asarray(case.fam["n_parents"]) >= 1

    def put(s, j, v):
        if j < fam.shape[0] and s < n and 0 <= v < nf and real[v] and v not in fam[:, s]:
            fam[j, s] = v
    if getattr(case, "noise", None) is not None and n > 4:
        tip = int(case.noise[0][0])
        put(4, 0, int(pf[tip]) if pf[tip] >= 0 and real[pf[tip]] else tip)
    if getattr(case, "mask", None) is not None and case.planted_mask["cherry"] is not None:
        site, f, _ = case.planted_mask["cherry"]
        a, ident = int(pf[f]), OS.reference_site(case, site)["identified"]
        while a >= 0 and real[a] and not ident[a] and pf[a] >= 0 and real[pf[a]]:
            a = int(pf[a])       # (the nearest ancestor whose clade still observes a tip at that site, if there is one)
        put(site, 0, a)
        put(site, 1, int(f))
    return fam


_draw_plain = draw_setting


def draw_setting(case, n, n_slots, seed=0):   # noqa: F811  (the drawn setting with the case's planted configurations)
    fam, delta = _draw_plain(case, n, n_slots, seed)
    fam = _plant_in_case(case, fam, n)
    rng = np.random.default_rng(3000 + seed)
    return fam, np.where(fam >= 0, np.where(delta != 0.0, delta, rng.normal(size=fam.shape)), 0.0)


# (case, sites, slots) of the parity tests: 8 sites (plain layout), 64, 65 (a second row word), 257 (a second workgroup)
PARITY = [("main", 8, 3), ("main", 64, 1), ("main", 65, 8), ("main", 257, 3), ("fixed", 64, 3), ("random", 64, 3), ("improper", 64, 3),
          ("two tips", 8, 1), ("caterpillar", 64, 3), ("balanced", 64, 8), ("families63", 64, 3), ("families64", 64, 1),
          ("families65", 64, 3), ("families130", 64, 8), ("shifts+noise", 65, 3), ("mask", 65, 3), ("optima", 65, 8),
          ("everything", 65, 3)]


def checked_sites(case, n):
    """the sites compared against the dense statements: the planted ones, lanes 0 and 63, site 64, the last"""
    extra = set()
    if getattr(case, "mask", None) is not None and case.planted_mask["cherry"] is not None:
        extra.add(int(case.planted_mask["cherry"][0]))
    return sorted(x for x in {0, 1, 2, 3, 4, 63, 64, n - 1} | extra if x < n)


# ----------------------------------------------------------------------------- forward selection

SELECT_SITES = 64
MAX_SHIFTS = 3
MIN_LR = 3.0


@functools.lru_cache(maxsize=None)
def select_case(key):
    """"fixed": the 30-tip case as it is.  "planted": its models with two disjoint clades per site, different at different
    sites, shifted in opposite directions by 12 to 20 standard deviations of the stationary distribution, the data drawn in numpy from that model"""
    base = OS.case("fixed")
    if key == "fixed":
        return base
    rng = np.random.default_rng(3100)
    c = types.SimpleNamespace(**base.__dict__)
    nf = len(c.fam["cluster"])
    tips = {f: sum(1 for e in OS.clade_edges(c, f) if e.child.leaf) for f in range(nf) if int(c.fam["n_parents"][f]) >= 1}
    big = [f for f, k in tips.items() if 2 <= k <= 6]
    edges = {f: {e.number for e in OS.clade_edges(c, f)} for f in big}
    n = len(c.sites)
    fam = np.full((2, n), -1, np.int32)
    delta = np.zeros((2, n))
    sites = []
    for s, (model, tbl) in enumerate(c.sites):
        while True:
            a, b = (int(x) for x in rng.choice(big, size=2, replace=False))
            if not edges[a] & edges[b]:
                break
        fam[:, s] = (a, b)
        sd = np.sqrt(model.gamma2)
        delta[:, s] = rng.choice([-1.0, 1.0]) * np.array([1.0, -1.0]) * rng.uniform(12.0, 20.0, size=2) * sd
        w = OS.site_model(painted(base, s, fam, delta), s)
        m0, S, _ = OD.node_moments(c.net, w)
        x = rng.multivariate_normal(m0, S)
        tip = {nd.name: float(x[i]) for i, nd in enumerate(c.net.vec_node) if nd.leaf}
        sites.append((model, [[tip[t] for t in c.taxa]]))
    c.sites = sites
    c.planted = (fam, delta)
    c.name = base.name + " + 2 planted clades"
    return c


@functools.lru_cache(maxsize=None)
def greedy(key, s):
    return dense_greedy(select_case(key), s, MAX_SHIFTS, MIN_LR)

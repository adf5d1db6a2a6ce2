"""Comparators and cases of the lanes-are-sites family sweeps of a univariate batch (pgbp_lg_shift_scan_sites,
pgbp_lg_edge_gradient_sites, pgbp_lg_loo_sites), host side, shared by test_fam_uni_cpu.py and test_gpu_fam_uni.py (tests only).

(a) `sweeps`: a numpy restatement of the three closed forms at p = 1, over the family table and J^-1 h, J^-1 of each family's
    cluster (0, 1 or 2 variables) -- r = u'x + const - w, e = E[r], C = u' Sigma u, j = 1 / V, g_w = j e;
      scan:  H = j - j C j, identified iff H > min_info j, jump = g_w / H, lr = g_w^2 / H;
      edge:  G_V = (j (C + e^2) j - j) / 2, g_qk = j (e x_k + (Sigma u)[v_k]), dX_k = dvc G_V R_k + dwc theta g_w + dqc g_qk;
      loo:   D = V - C, determined iff D > 2^-40 V and V > 0, var = V^2 / D, mean = y - V e / D,
             lpd = -(log 2pi + 2 log V - log D + e^2 / D) / 2.
    It also returns the figures the GPU tests' conditions are about: H / j of every family and D / V of every tip.
(b) `dense`: the dense statements the project already has, in the family table's layout: noise_ref.family_statement (the scan
    of scan_ref.family_scan and the derivatives of edge_ref.family_edge_gradient, with shifts and tip noise) on the dense
    posterior of the node states, and loo_ref.dense_loo.  An improper root takes the flat-prior posterior (`flat_posterior`,
    the universal kriging of loo_ref.dense_loo over all nodes).
(c) the cases both test files run: (a) on the oracle's calibrated clique tree is pinned to (b) on the CPU for every case the
    GPU file uses."""
import functools
import types

import numpy as np

import loo_ref as LR
import noise_ref as NR
import uni_net_ref as N
from edge_ref import edge_coefs
from helpers import lg_inputs_from_oracle, oracle_setup
from oracle import calibration as OC
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from shift_ref import ShiftedModel, family_edge, family_nodes

BLOCK = 64   # families a thread walks; the order of every reduction over families follows it
LOG2PI = float(np.log(2.0 * np.pi))
LOO_FLOOR = 2.0 ** -40


# ----------------------------------------------------------------------------- (a) the closed forms, restated

def block_total(lpd):
    """the device's order of the total: the tips of a block of 64 added in order, then the blocks in order"""
    lpd = np.asarray(lpd, float)
    acc = 0.0
    for b in range(0, len(lpd), BLOCK):
        part = 0.0
        for v in lpd[b:b + BLOCK]:
            part = part + v
        acc = acc + part
    return float(acc)


def top_of(lr, identified, n_parents):
    """(top_lr, top_family) over the families with an edge, identified, lr finite; ties to the lowest family"""
    ok = (np.asarray(n_parents) >= 1) & np.asarray(identified, bool) & np.isfinite(lr)
    v = np.where(ok, lr, -np.inf)
    f = int(np.argmax(v)) if len(v) else -1
    if f < 0 or not np.isfinite(v[f]):
        return -np.inf, -1
    return float(v[f]), f


def sweeps(fam, data, R, mu, moments, model="bm", alpha=None, theta=None, shifts=None, noise=None, min_info=1e-8):
    """fam: the table of lg_families at p = 1; data [n_rows, 1]; R [n_rates]; moments(c) -> (J^-1 h, J^-1) of cluster c;
    shifts {f * K + k: s}; noise {f: E_f}.  One site.  Returns dict(scan, edge, loo) of dicts in the layouts of
    shift_scan_lg / edge_gradient_lg / loo_lg at p = 1 (without the trait axes), scan with relH [F] = H / j (NaN where there
    is no edge or the family is skipped), top_lr, top_family; loo with relD [n_tip] = D / V."""
    ou = model == "ou"
    K, nf = max(1, int(fam["max_parents"])), len(fam["cluster"])
    R = np.asarray(R, float).reshape(-1)
    mu = float(np.ravel(mu)[0])
    th = float(np.ravel(theta)[0]) if ou else 0.0
    shifts, noise = shifts or {}, noise or {}
    cm = fam.get("child_mask")
    jump, lr, H, relH = (np.full(nf, np.nan) for _ in range(4))
    dlen, dgam, dshift = np.full((nf, K), np.nan), np.full((nf, K), np.nan), np.zeros(nf)
    tips = LR.tip_families(fam)
    tip_of = {int(f): i for i, f in enumerate(tips)}
    nt = len(tips)
    mean, var, lpd, relD = (np.full(nt, np.nan) for _ in range(4))
    info = np.ones(nt, np.int32)
    for f in range(nf):
        npar, cpos = int(fam["n_parents"][f]), int(fam["child_pos"][f])
        if (cm is not None and not int(cm[f]) & 1) or (npar == 0 and cpos < 0):   # skipped by the factor fill
            lr[f] = np.nan if npar == 0 else 0.0
            dlen[f, :npar] = dgam[f, :npar] = 0.0
            continue
        ppos = [int(fam["parent_pos"][f * K + k]) for k in range(npar)]
        if cpos >= 0 or any(q >= 0 for q in ppos):
            m, S = moments(int(fam["cluster"][f]))
        else:
            m, S = np.zeros(0), np.zeros((0, 0))
        u = np.zeros(len(m))
        cst = y = 0.0
        if cpos >= 0:
            u[cpos] = 1.0
        elif fam["data_row"][f] >= 0:
            cst = y = float(np.asarray(data, float)[fam["data_row"][f], 0])
        co = [edge_coefs(alpha if ou else None, fam["length"][f * K + k], fam["gamma"][f * K + k]) for k in range(npar)]
        col = [int(fam["color"][f * K + k]) for k in range(npar)]
        if npar == 0:
            V, w = R[int(fam["color"][f * K])], mu
        else:
            V = sum(c[0][1] * R[cc] for c, cc in zip(co, col))
            w = sum(c[0][2] for c in co) * th + sum(fam["gamma"][f * K + k] * shifts.get(f * K + k, 0.0) for k in range(npar))
            for c, q in zip(co, ppos):
                if q >= 0:
                    u[q] -= c[0][0]
                else:
                    cst -= c[0][0] * mu   # the fixed root
        V = V + noise.get(f, 0.0)
        e = float(u @ m) + cst - w
        su = S @ u
        C = float(u @ su)
        j = 1.0 / V
        gw = j * e
        dshift[f] = gw
        if npar > 0:
            Hf = j - j * C * j
            relH[f] = Hf / j
            if Hf > min_info * j:
                jump[f], lr[f], H[f] = gw / Hf, gw * gw / Hf, Hf
            else:
                lr[f] = 0.0
            G = 0.5 * (j * (C + e * e) * j - j)
            for k in range(npar):
                xk, suk = (m[ppos[k]], su[ppos[k]]) if ppos[k] >= 0 else (mu, 0.0)
                gq, trGR, thg = j * (e * xk + suk), G * R[col[k]], th * gw
                _, dt, dg = co[k]
                dlen[f, k] = dt[1] * trGR + dt[2] * thg + dt[0] * gq
                dgam[f, k] = dg[1] * trGR + dg[2] * thg + dg[0] * gq + shifts.get(f * K + k, 0.0) * gw
        if f in tip_of:
            ti = tip_of[f]
            D = V - C
            relD[ti] = D / V
            if D > LOO_FLOOR * V and V > 0:
                info[ti] = 0
                var[ti], mean[ti] = V * V / D, y - V * e / D
                lpd[ti] = -0.5 * (LOG2PI + 2 * np.log(V) - np.log(D) + e * e / D)
    ident = ~np.isnan(jump)
    top_lr, top_family = top_of(lr, ident, fam["n_parents"])
    return dict(scan=dict(jump=jump, lr=lr, H=H, identified=ident, relH=relH, top_lr=top_lr, top_family=top_family),
                edge=dict(dlength=dlen, dgamma=dgam, dshift=dshift),
                loo=dict(families=tips, mean=mean, var=var, lpd=lpd, info=info, relD=relD, total=block_total(lpd)))


# ----------------------------------------------------------------------------- (b) the dense statements, per family

def flat_posterior(net, model, tbl, taxa):
    """densemvn.posterior_node_moments for an improper root: the flat prior on the root state (universal kriging, as
    loo_ref.dense_loo does for the left-out tip), over all node states."""
    p = model.dimension()
    m0, S, A = OD.node_moments(net, model, np.zeros(p), np.zeros((p, p)))
    obs = np.array([i * p + t for i, _, t in LR._observed(net, tbl, taxa, p)], dtype=int)
    y = np.array([float(tbl[t][r]) for _, r, t in LR._observed(net, tbl, taxa, p)])
    Soo, Ao, res = S[np.ix_(obs, obs)], A[obs], y - m0[obs]
    Kt = np.linalg.solve(Soo, S[obs, :]).T
    M = Ao.T @ np.linalg.solve(Soo, Ao)
    b = np.linalg.solve(M, Ao.T @ np.linalg.solve(Soo, res))
    B = A - Kt @ Ao
    return m0 + A @ b + Kt @ (res - Ao @ b), S - Kt @ S[obs, :] + B @ np.linalg.solve(M, B.T)


def is_improper(model):
    v = np.atleast_2d(np.asarray(model.rootpriorvariance(), float))
    return (not model.isrootfixed()) and bool(np.any(np.isinf(np.diag(v))))


def dense(net, ocgb, fam, model, tbl, taxa, shifts=None, noise=None, min_info=1e-8, loo=True):
    """The dense statements in the family table's layout for one site: shifts {(f, k): s}, noise {f: E_f}.
    dict(jump, lr, identified [F], dlength, dgamma [F, K], dshift [F], loo = loo_ref.dense_loo of the (wrapped) model)."""
    shifts, noise = shifts or {}, noise or {}
    sh = {family_edge(net, ocgb, fam, f, k).number: np.array([v]) for (f, k), v in shifts.items()}
    inner = ShiftedModel(model, sh) if sh else model
    fams = sorted(noise)
    E = np.array([noise[f] for f in fams]).reshape(-1, 1, 1)
    w = NR.wrapper(net, ocgb, fam, inner, fams, E) if fams else inner
    nn, sc = NR.node_noise(ocgb, fam, fams, E, np.ones(len(fams)))
    pm, pc = flat_posterior(net, w, tbl, taxa) if is_improper(model) else OD.posterior_node_moments(net, w, tbl, taxa)
    st = NR.family_statement(net, model, sh, nn, sc, pm, pc, min_info)
    nodes = family_nodes(ocgb, fam)
    K = max(1, int(fam["max_parents"]))
    out = dict(jump=st["jump"][nodes][:, 0], lr=st["lr"][nodes], identified=st["identified"][nodes][:, 0],
               dshift=st["dshift"][nodes][:, 0], dlength=np.full((len(nodes), K), np.nan), dgamma=np.full((len(nodes), K), np.nan))
    for f, i in enumerate(nodes):
        for k in range(int(fam["n_parents"][f])):
            ed = family_edge(net, ocgb, fam, f, k)
            kk = next(q for q, e2 in enumerate(st["edges"][i]) if e2 is ed)
            out["dlength"][f, k], out["dgamma"][f, k] = st["dlength"][i, kk], st["dgamma"][i, kk]
    if loo:
        out["loo"] = LR.dense_loo(net, w, tbl, taxa)
    return out


def rel(got, want):
    """max |got - want| relative to max(1, |want|_inf) over the entries that exist; the NaN patterns must be the same"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN patterns differ"
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - want[ok]))) / max(1.0, float(np.max(np.abs(want[ok]))))


def against_dense(sw, dn, fam, rows_of_tips, skip_tips=()):
    """worst rel of the restated sweeps `sw` (or a device result in the same layout) against the dense statements `dn`, over
    the families that have a factor: a skipped family (child_mask == 0) is no family of the dense statement.  skip_tips: tip
    indices the dense leave-one-out does not state (not determined)."""
    cm = fam.get("child_mask")
    live = np.array([cm is None or bool(int(cm[f]) & 1) for f in range(len(fam["cluster"]))])
    edge = live & (np.asarray(fam["n_parents"]) >= 1)
    worst = {}
    assert np.array_equal(sw["scan"]["identified"][edge], dn["identified"][edge])
    worst["jump"] = rel(sw["scan"]["jump"][edge], dn["jump"][edge])
    worst["lr"] = rel(sw["scan"]["lr"][edge], dn["lr"][edge])
    for k in ("dlength", "dgamma"):
        worst[k] = rel(sw["edge"][k][edge], dn[k][edge])
    has = live & ~np.isnan(dn["dshift"])
    worst["dshift"] = rel(sw["edge"]["dshift"][has], dn["dshift"][has])
    lw = 0.0
    for ti, r in enumerate(rows_of_tips):
        if ti in skip_tips:
            continue
        _, mean, cov, lpd = dn["loo"][int(r)]
        assert sw["loo"]["info"][ti] == 0, (ti, sw["loo"]["info"][ti])
        lw = max(lw, rel(sw["loo"]["mean"][ti], mean[0]), rel(sw["loo"]["var"][ti], cov[0, 0]), rel(sw["loo"]["lpd"][ti], lpd))
    worst["loo"] = lw
    return worst


# ----------------------------------------------------------------------------- (c) the cases

def _case(name, net, taxa, sites, **kw):
    """A case: the oracle network, its taxa, [(model, tbl)] per site; the oracle's clique tree, the family table and the
    schedule of site 0 (the same for every site: one missing pattern).  shifts: (edges [(f, k)], values [sites, n]) or None;
    noise: (families [n], E [sites, n]) or None."""
    cg = OCG.cliquetree(net)
    ocgb0 = oracle_setup(net, cg, sites[0][0], sites[0][1], taxa)
    fam, _, _ = lg_inputs_from_oracle(_product(), net, ocgb0, sites[0][0], sites[0][1], taxa)
    c = types.SimpleNamespace(name=name, net=net, taxa=taxa, sites=sites, cg=cg, ocgb0=ocgb0, fam=fam,
                              spt=OCG.spanningtree_clusterlist(cg, OCG.default_rootcluster(cg, net)),
                              shifts=None, noise=None, identification=False, top=False, planted=None, undetermined=None)
    c.__dict__.update(kw)
    return c


def _product():
    import pgbp_amd
    return pgbp_amd


def site_shifts(case, s):
    return {} if case.shifts is None else {fk: float(v) for fk, v in zip(case.shifts[0], case.shifts[1][s])}


def site_noise(case, s):
    return {} if case.noise is None else {int(f): float(e) for f, e in zip(case.noise[0], case.noise[1][s])}


def oracle_site(case, s):
    """(calibrated oracle beliefs, family table, data, assignfactors keywords) of site s; shifts and noise of the case are
    in the oracle's factors through the wrappers of shift_ref / noise_ref"""
    model, tbl = case.sites[s]
    sh = {family_edge(case.net, case.ocgb0, case.fam, f, k).number: np.array([v]) for (f, k), v in site_shifts(case, s).items()}
    w = ShiftedModel(model, sh) if sh else model
    nz = site_noise(case, s)
    if nz:
        fams = sorted(nz)
        w = NR.wrapper(case.net, case.ocgb0, case.fam, w, fams, np.array([nz[f] for f in fams]).reshape(-1, 1, 1))
    ocgb = oracle_setup(case.net, case.cg, w, tbl, case.taxa)
    fam, data, kw = lg_inputs_from_oracle(_product(), case.net, case.ocgb0, model, tbl, case.taxa)
    assert OC.calibrate(ocgb, [case.spt], verbose=False)[0]
    return ocgb, fam, data, kw


def reference_site(case, s, min_info=1e-8):
    """`sweeps` of site s on the oracle's calibrated clique tree: (result, family table)"""
    ocgb, fam, data, kw = oracle_site(case, s)
    K = max(1, int(fam["max_parents"]))
    sw = sweeps(fam, data, kw["R"], kw["mu"], LR.oracle_moments(ocgb), kw.get("model", "bm"), kw.get("alpha"), kw.get("theta"),
                {f * K + k: v for (f, k), v in site_shifts(case, s).items()}, site_noise(case, s), min_info)
    return sw, fam


def dense_site(case, s, min_info=1e-8, loo=True):
    model, tbl = case.sites[s]
    return dense(case.net, case.ocgb0, case.fam, model, tbl, case.taxa, site_shifts(case, s), site_noise(case, s), min_info, loo)


def top_margin(case, s, min_info=1e-8):
    """(largest lr, second largest lr, family of the largest) of site s over the eligible families, from the dense statement"""
    dn = dense_site(case, s, min_info, loo=False)
    cm = case.fam.get("child_mask")
    live = np.array([cm is None or bool(int(cm[f]) & 1) for f in range(len(case.fam["cluster"]))])
    ok = live & (np.asarray(case.fam["n_parents"]) >= 1) & dn["identified"] & np.isfinite(dn["lr"])
    v = np.where(ok, dn["lr"], -np.inf)
    order = np.argsort(-v, kind="stable")
    return float(v[order[0]]), float(v[order[1]]), int(order[0])


def _tree_net(tree):
    net = ON.read_newick(tree.newick())
    taxa = list(net.tip_names)
    return net, taxa, [int(t[1:]) for t in taxa]


def _tips_below(net, node):
    out, stack = [], [node]
    while stack:
        n = stack.pop()
        ch = [e.child for e in net.child_edges(n)]
        if not ch:
            out.append(n.name)
        stack += ch
    return out


@functools.lru_cache(maxsize=None)
def bm_case(n_sites=600, shifts_and_noise=False):
    """40-tip tree, fixed root, per-site data, rate and mu (600 sites: the GPU tests take the first 8 / 64 / 65 / 257 / 600);
    shifts_and_noise: per-site shifts on three edges and per-site noise on every second tip (65 sites)."""
    from pgbp_amd import synth
    rng = np.random.default_rng(410)
    tree = synth.random_tree(40, rng)
    net, taxa, tipnode = _tree_net(tree)
    s2, mu = rng.uniform(0.5, 2.0, n_sites), rng.normal(size=n_sites)
    X = synth.simulate_bm_uni_sites(tree, s2, mu, rng)
    sites = [(OM.UnivariateBrownianMotion(s2[s], mu[s]), [[float(X[s, i]) for i in tipnode]]) for s in range(n_sites)]
    c = _case("bm+shifts+noise" if shifts_and_noise else "bm", net, taxa, sites)
    if shifts_and_noise:
        tips = [int(f) for f in LR.tip_families(c.fam)]
        fams = tips[::2]
        edges = [(fams[0], 0), (fams[-1], 0), (len(c.fam["cluster"]) // 2, 0)]
        c.shifts = (edges, rng.normal(size=(n_sites, len(edges))))
        K = max(1, int(c.fam["max_parents"]))
        V = np.array([[c.fam["length"][f * K] * s2[s] for f in fams] for s in range(n_sites)])
        c.noise = (fams, V * rng.uniform(0.05, 2.0, size=V.shape))
    return c


@functools.lru_cache(maxsize=None)
def ou_case(root):
    """30-tip tree, 64 sites with their own alpha, theta, stationary variance and mu; fixed, random or improper root"""
    from pgbp_amd import synth
    rng = np.random.default_rng(411)
    ns = 64
    tree = synth.random_tree(30, rng)
    net, taxa, tipnode = _tree_net(tree)
    alpha, gam2 = rng.uniform(0.3, 1.5, ns), rng.uniform(0.5, 2.0, ns)
    theta, mu = rng.normal(size=ns), rng.normal(size=ns)
    X = synth.simulate_ou_uni_sites(tree, 2 * alpha * gam2, alpha, theta, mu, rng)
    v = {"fixed": None, "random": 0.8, "improper": np.inf}[root]
    sites = [(OM.UnivariateOrnsteinUhlenbeck(2 * alpha[s] * gam2[s], alpha[s], theta[s], mu[s], v),
              [[float(X[s, i]) for i in tipnode]]) for s in range(ns)]
    return _case(f"ou/{root}", net, taxa, sites)


@functools.lru_cache(maxsize=None)
def missing_case():
    """65 sites on a 24-tip tree; a whole cherry and two more tips carry no data: the cherry's internal family is skipped by
    the fill (child_mask 0) -- a clade without data, not identified -- next to identified families"""
    from pgbp_amd import synth
    rng = np.random.default_rng(412)
    tree = synth.random_tree(24, rng)
    kids = [np.nonzero(tree.parent == i)[0] for i in range(tree.nnodes)]
    inner = next(i for i in range(1, tree.nnodes) if len(kids[i]) == 2 and tree.is_leaf[kids[i]].all())
    others = [i for i in np.nonzero(tree.is_leaf)[0] if i not in kids[inner]]
    ns = 65
    net, taxa, tipnode = _tree_net(tree)
    s2, mu = rng.uniform(0.5, 2, ns), rng.normal(size=ns)
    X = synth.simulate_bm_uni_sites(tree, s2, mu, rng)
    # two more tips, neither the cherry's sibling nor each other's (the reference's factor assignment does not take a clade
    # without data inside a clade without data)
    up = lambda i: int(tree.parent[i])
    more = [int(i) for i in others if up(i) != up(inner)]
    more = [more[0]] + [i for i in more[1:] if up(i) != up(more[0]) and up(up(i)) != up(more[0]) and up(i) != up(up(more[0]))][:1]
    gone = [int(i) for i in kids[inner]] + more
    assert len(gone) == 4
    # one large jump on a tip of a cherry with complete data: with a tip missing, the edge above its sibling and the edge
    # above their parent have the same lr exactly (the data cannot tell them apart), so the largest lr is planted elsewhere
    full = next(int(i) for i in np.nonzero(tree.is_leaf)[0]
                if all(tree.is_leaf[k] and int(k) not in gone for k in kids[up(i)]) and len(kids[up(i)]) == 2)
    X[:, full] += 25.0 * np.sqrt(s2)
    sites = [(OM.UnivariateBrownianMotion(s2[s], mu[s]), [[None if i in gone else float(X[s, i]) for i in tipnode]])
             for s in range(ns)]
    c = _case("missing", net, taxa, sites, identification=True, top=True)
    c.planted = next(f for f, i in enumerate(family_nodes(c.ocgb0, c.fam)) if net.vec_node[i].name == f"n{full}")
    return c


@functools.lru_cache(maxsize=None)
def hybrid_case(name, kind):
    """N1 .. N4 of uni_net_ref (hybrid tips: two-parent families, 2- and 0-variable clusters, a fixed-root parent), fixed
    root, 65 sites"""
    net, taxa = N.network(name)
    return _case(f"{name}/{kind}", net, taxa, list(N.sites(name, "fixed", kind)))


def tree_with_families(n_fam):
    """a synth tree with exactly n_fam node families (= nodes - 1): bifurcating when n_fam is even, else with polytomies"""
    from pgbp_amd import synth
    if n_fam % 2 == 0:
        return synth.random_tree(n_fam // 2 + 1, np.random.default_rng(n_fam))
    for seed in range(200):
        for ntips in range(n_fam // 2 + 2, n_fam):
            tr = synth.random_multifurcating_tree(ntips, 4, np.random.default_rng(1000 * seed + ntips))
            if tr.nnodes - 1 == n_fam:
                return tr
    raise AssertionError(n_fam)


@functools.lru_cache(maxsize=None)
def block_case(n_fam, planted):
    """A tree with n_fam families, fixed root, 64 sites (16, the plain layout, for the 398 families: its dense statements
    take a second per site), and one large jump planted in the data of every site on the edge of family `planted`: every tip
    below it moved by 25 standard deviations of a unit edge"""
    from pgbp_amd import synth
    rng = np.random.default_rng(413 + n_fam)
    ns = 64 if n_fam <= 200 else 16
    tree = tree_with_families(n_fam)
    net, taxa, tipnode = _tree_net(tree)
    s2, mu = rng.uniform(0.5, 2.0, ns), rng.normal(size=ns)
    X = synth.simulate_bm_uni_sites(tree, s2, mu, rng)
    sites0 = [(OM.UnivariateBrownianMotion(s2[s], mu[s]), [[float(X[s, i]) for i in tipnode]]) for s in range(ns)]
    c = _case(f"{n_fam} families, jump at {planted}", net, taxa, sites0, top=True, planted=planted)
    assert len(c.fam["cluster"]) == n_fam and int(c.fam["n_parents"][planted]) == 1
    below = set(_tips_below(net, net.vec_node[family_nodes(c.ocgb0, c.fam)[planted]]))
    for s in range(ns):
        row = c.sites[s][1][0]
        for r, t in enumerate(taxa):
            if t in below:
                row[r] += 25.0 * np.sqrt(s2[s])
    return c


@functools.lru_cache(maxsize=None)
def undetermined_case():
    """12-tip tree, improper root, 8 sites, two rates: the pendant edges of every tip but the first have a rate of their own,
    which at site 5 is 1e22 -- there the other data leave the first tip's parent undetermined to rounding (D = V - S is 0 in
    floating point), every other tip is predicted (from the first, with a huge variance)."""
    from pgbp_amd import synth
    rng = np.random.default_rng(414)
    ns = 8
    tree = synth.random_tree(12, rng)
    net, taxa, tipnode = _tree_net(tree)
    first = taxa[0]
    ecol = {e.number: (2 if (e.child.leaf and e.child.name != first) else 1) for e in net.edges}
    rates = rng.uniform(0.5, 2.0, size=(ns, 2))
    rates[5, 1] = 1e22
    X = synth.simulate_bm_uni_sites(tree, rates[:, 0], np.zeros(ns), rng)
    sites = [(OM.HeterogeneousBrownianMotion([np.array([[r]]) for r in rates[s]], ecol, np.array([0.0]), np.array([[np.inf]])),
              [[float(X[s, i]) for i in tipnode]]) for s in range(ns)]
    c = _case("undetermined", net, taxa, sites)
    tips = LR.tip_families(c.fam)
    c.undetermined = (5, int(np.flatnonzero(c.fam["data_row"][tips] == 0)[0]))   # (site, tip index)
    return c


def plain_cases():
    """every case whose three sweeps the GPU file compares: (case, the site counts it runs at)"""
    yield bm_case(), (8, 64, 65, 257)
    for root in ("fixed", "random", "improper"):
        yield ou_case(root), (64,)
    yield missing_case(), (65,)
    for name in ("N1", "N2", "N3", "N4"):
        for kind in ("bm", "ou"):
            yield hybrid_case(name, kind), (8, 64, 65)
    yield bm_case(65, True), (8, 65)


BLOCKS = [(63, 62), (64, 63), (65, 63), (65, 64), (130, 63), (130, 64), (398, 63), (398, 64)]


def checked_sites(n):
    """one site in eight"""
    return range(0, n, 8)

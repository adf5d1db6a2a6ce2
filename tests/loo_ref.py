"""Comparators of the leave-one-out sweep (pgbp_lg_loo / ClusterGraphBelief.loo_lg), host side, shared by test_loo_cpu.py
and test_gpu_loo.py (tests only):

(a) `dense_loo`: the DENSE comparator on oracle/densemvn.py alone (no message passing): lpd of a tip = loglik(all data) -
    loglik(the data with that tip's entries None) -- fixed, random and improper roots; mean and covariance by conditioning
    the joint of node_moments on the other observations, with the flat root prior (universal kriging) for an improper root;
(b) `loo_sweep`: a numpy restatement of the device sweep from J^-1 h and J^-1 of each tip family's cluster;
and the cases both test files run, so that (b) is pinned to (a) on the CPU for every input the GPU tests use."""
import zlib

import numpy as np

from helpers import goldens, lg_inputs_from_oracle, make_model, oracle_setup
from oracle import calibration as OC
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON

LOG2PI = float(np.log(2.0 * np.pi))
G = goldens()


# ----------------------------------------------------------------------------- (a) the dense comparator

def _observed(net, tbl, taxa, p):
    """[(node index in preorder, taxon row, trait)] of every observed tip value, in densemvn.loglik's order."""
    out = []
    for i, n in enumerate(net.vec_node):
        if n.leaf:
            r = list(taxa).index(n.name)
            out += [(i, r, t) for t in range(p) if tbl[t][r] is not None]
    return out


def dense_loo(net, model, tbl, taxa, tips=None):
    """{taxon row: (observed traits, mean, cov, lpd)} of the leave-one-out predictive of every tip with data (or of the
    rows `tips`)."""
    p = model.dimension()
    v = np.atleast_2d(np.asarray(model.rootpriorvariance(), float))
    improper = bool(np.any(np.isinf(np.diag(v))))
    if improper:
        m0, S, A = OD.node_moments(net, model, np.zeros(p), np.zeros((p, p)))
    else:
        m0, S, A = OD.node_moments(net, model)
    obs = _observed(net, tbl, taxa, p)
    pos = np.array([i * p + t for i, _, t in obs], dtype=int)
    y = np.array([float(tbl[t][r]) for _, r, t in obs])
    rows = np.array([r for _, r, _ in obs])
    ll_all = OD.loglik(net, model, tbl, taxa)
    out = {}
    for r in (sorted(set(rows.tolist())) if tips is None else tips):
        it, io = np.flatnonzero(rows == r), np.flatnonzero(rows != r)
        less = [[None if k == r else val for k, val in enumerate(col)] for col in tbl]
        lpd = ll_all - OD.loglik(net, model, less, taxa)
        pt, po = pos[it], pos[io]
        Soo, Sto, Stt = S[np.ix_(po, po)], S[np.ix_(pt, po)], S[np.ix_(pt, pt)]
        res = y[io] - m0[po]
        G_ = np.linalg.solve(Soo, Sto.T).T                     # S_t- S_--^-1
        if improper:
            Ao, At = A[po], A[pt]
            M = Ao.T @ np.linalg.solve(Soo, Ao)
            b = np.linalg.solve(M, Ao.T @ np.linalg.solve(Soo, res))
            B = At - G_ @ Ao
            mean = m0[pt] + At @ b + G_ @ (res - Ao @ b)
            cov = Stt - G_ @ Sto.T + B @ np.linalg.solve(M, B.T)
        else:
            mean = m0[pt] + G_ @ res
            cov = Stt - G_ @ Sto.T
        out[r] = (np.array([obs[i][2] for i in it], dtype=int), mean, cov, float(lpd))
    return out


# ----------------------------------------------------------------------------- (b) the sweep, restated

def tree_total(lpd):
    """The device's fixed order of the total: partial sum r of 256 = the tips r, r + 256, ... added in order; the 256 partial
    sums by a halving tree."""
    lpd = np.asarray(lpd, float)
    part = np.zeros(256)
    for f in range(len(lpd)):
        part[f % 256] = part[f % 256] + lpd[f]
    w = 128
    while w > 0:
        part[:w] = part[:w] + part[w:2 * w]
        w //= 2
    return float(part[0])


def tip_families(fam):
    cm = fam.get("child_mask")
    return np.array([f for f in range(len(fam["cluster"]))
                     if fam["child_pos"][f] < 0 and fam["data_row"][f] >= 0 and (cm is None or int(cm[f]) != 0)], dtype=np.int32)


def loo_sweep(fam, data, R, mu, moments, model="bm", alpha=None, theta=None):
    """fam: the table of lg_families; data [n_rows, p]; R [n_rates, p, p]; moments(c) -> (J^-1 h, J^-1) of cluster c (None
    when the belief is not positive definite).  Returns the dict of loo_lg for one site."""
    p, K = int(fam["p"]), max(1, int(fam["max_parents"]))
    R = np.asarray(R, float).reshape(-1, p, p)
    mu = np.asarray(mu, float).reshape(p)
    tips = tip_families(fam)
    nt = len(tips)
    mean, cov = np.full((nt, p), np.nan), np.full((nt, p, p), np.nan)
    lpd, info = np.full(nt, np.nan), np.zeros(nt, np.int32)
    rank = lambda mask, t: bin(int(mask) & ((1 << t) - 1)).count("1")
    for ti, f in enumerate(tips):
        full = (1 << p) - 1
        O = int(fam["child_mask"][f]) if fam.get("child_mask") is not None else full
        o = [t for t in range(p) if (O >> t) & 1]
        npar = int(fam["n_parents"][f])
        y = np.asarray(data, float)[fam["data_row"][f], o]
        qc, vc, wc = [], [], []
        for k in range(npar):
            t_, g_ = fam["length"][f * K + k], fam["gamma"][f * K + k]
            if model == "ou":
                a = np.exp(-alpha * t_)
                qc.append(g_ * a); vc.append(g_ * g_ * (1 - a * a)); wc.append(g_ * (1 - a))
            else:
                qc.append(g_); vc.append(g_ * g_ * t_); wc.append(0.0)
        V = sum(vc[k] * R[fam["color"][f * K + k]] for k in range(npar))[np.ix_(o, o)]
        w = sum(wc) * np.asarray(theta, float).reshape(p)[o] if model == "ou" else np.zeros(len(o))
        in_scope = [k for k in range(npar) if fam["parent_pos"][f * K + k] >= 0]
        m_u = np.zeros(len(o))
        S = np.zeros((len(o), len(o)))
        for k in range(npar):
            if k not in in_scope:
                m_u = m_u + qc[k] * mu[o]
        if in_scope:
            mom = moments(int(fam["cluster"][f]))
            if mom is None:
                info[ti] = 1
                continue
            cm, cS = mom
            idx = {}
            for k in in_scope:
                mk = int(fam["parent_mask"][f * K + k]) if fam.get("parent_mask") is not None else full
                idx[k] = [int(fam["parent_pos"][f * K + k]) + rank(mk, t) for t in o]
                m_u = m_u + qc[k] * cm[idx[k]]
            for a in in_scope:
                for b in in_scope:
                    S = S + qc[a] * qc[b] * cS[np.ix_(idx[a], idx[b])]
        r = y - w - m_u
        D = V - S
        try:
            LD, LV = np.linalg.cholesky(D), np.linalg.cholesky(V)
        except np.linalg.LinAlgError:
            info[ti] = 1
            continue
        if np.any(np.diag(LD) ** 2 <= 2.0 ** -40 * np.diag(V)):
            info[ti] = 1
            continue
        Y = np.linalg.solve(LD, V)
        z = np.linalg.solve(LD, r)
        mean[ti, o] = y - Y.T @ z
        cov[np.ix_([ti], o, o)] = Y.T @ Y
        lpd[ti] = -0.5 * (len(o) * LOG2PI + 4 * np.sum(np.log(np.diag(LV))) - 2 * np.sum(np.log(np.diag(LD))) + z @ z)
    return dict(families=tips, mean=mean, cov=cov, lpd=lpd, total=tree_total(lpd), info=info)


def oracle_moments(ocgb):
    """moments(c) of loo_sweep from (calibrated) oracle beliefs."""
    def mom(c):
        b = ocgb.belief[c]
        try:
            np.linalg.cholesky(b.J)
        except np.linalg.LinAlgError:
            return None
        Sg = np.linalg.inv(b.J)
        return Sg @ b.h, (Sg + Sg.T) / 2
    return mom


def oracle_loo(net, model, tbl, taxa):
    """(b) on the oracle's calibrated clique tree: (families' taxon rows, loo dict)."""
    import pgbp_amd as P
    cg = OCG.cliquetree(net)
    ocgb = oracle_setup(net, cg, model, tbl, taxa)
    fam, data, kw = lg_inputs_from_oracle(P, net, ocgb, model, tbl, taxa)
    spt = OCG.spanningtree_clusterlist(cg, OCG.default_rootcluster(cg, net))
    assert OC.calibrate(ocgb, [spt], verbose=False)[0]
    d = loo_sweep(fam, data, kw["R"], kw["mu"], oracle_moments(ocgb), kw.get("model", "bm"), kw.get("alpha"), kw.get("theta"))
    return fam["data_row"][d["families"]], d


# ----------------------------------------------------------------------------- comparison

def rel_block(got, want):
    """max |got - want| relative to the largest entry of the block (rel_block of test_gradient_cpu.py)."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300))


def worst_error(rows, d, dense, p):
    """Largest rel_block of mean / cov / lpd of the tips of `d` (taxon rows `rows`) that `dense` holds; asserts the NaN
    pattern: predictions cover exactly the observed traits."""
    worst = 0.0
    for ti, r in enumerate(rows):
        if int(r) not in dense:
            continue
        o, mean, cov, lpd = dense[int(r)]
        assert d["info"][ti] == 0, (r, d["info"][ti])
        seen = np.isfinite(d["mean"][ti])
        assert np.array_equal(np.flatnonzero(seen), o), (r, seen, o)
        assert np.array_equal(np.isfinite(d["cov"][ti]), np.outer(seen, seen)), r
        worst = max(worst, rel_block(d["mean"][ti][o], mean), rel_block(d["cov"][ti][np.ix_(o, o)], cov),
                    abs(d["lpd"][ti] - lpd) / max(abs(lpd), 1.0))
    return worst


# ----------------------------------------------------------------------------- the cases

def bm(p, rng, root):
    A = rng.normal(size=(p, p))
    R = A @ A.T / p + np.eye(p)
    if root == "fixed":
        return OM.MvFullBrownianMotion(R, rng.normal(size=p))
    if root == "random":
        B = rng.normal(size=(p, p))
        return OM.MvFullBrownianMotion(R, rng.normal(size=p), B @ B.T / p + 0.5 * np.eye(p))
    return OM.MvFullBrownianMotion(R, np.zeros(p), np.diag(np.full(p, np.inf)))


def golden_networks():
    g = G["exact_reml_level1"]
    yield "level1_1trait", g["net"], g["taxa"], [g["y"]]
    yield "level1_2traits", g["net"], g["taxa"], [g["x"], g["y"]]
    g = G["optimization_mateescu"]
    yield "mateescu", G["joingraph_mateescu"]["net"], g["taxa"], [g["y"]]
    c = G["optimization_level1"]["cliquetree"]
    yield "optimization_level1", c["net"], c["taxa"], [c["y"]]
    g = G["optimization_sun2023"]
    yield "sun2023", g["net"], g["taxa_in_file_order"], [g["y1"], g["y2"]]


def reference_case(name, root):
    """The networks of the reference's own tests, full BM with a fixed / proper random / improper root."""
    _, netstr, taxa, cols = next(c for c in golden_networks() if c[0] == name)
    tbl = [[None if v is None else float(v) for v in col] for col in cols]
    return ON.read_newick(netstr), bm(len(cols), np.random.default_rng(11), root), tbl, taxa


REFERENCE = [(n, r) for n in ("level1_1trait", "level1_2traits", "mateescu", "optimization_level1", "sun2023")
             for r in ("fixed", "random", "improper")]
RANDOM = [("bm_fixed", 1), ("bm_improper", 2), ("bm_random", 4), ("hetero_random", 2), ("ou_fixed", 1), ("ou_random", 1),
          ("ou_improper", 1)]


def random_case(which, p):
    """24 tips, 6 hybrid nodes: BM, heterogeneous BM with 3 colours, the univariate OU."""
    rng = np.random.default_rng(zlib.crc32(f"loo-{which}-{p}".encode()))
    net = ON.random_network(24, 6, rng)
    taxa = net.tip_names
    kind, root = which.split("_")
    if kind == "bm":
        model = bm(p, rng, root)
    elif kind == "hetero":
        base = bm(p, rng, root)
        colors = {e.number: 1 + int(rng.integers(3)) for e in net.edges}
        model = OM.HeterogeneousBrownianMotion([base.R * s for s in (0.5, 1.0, 2.5)], colors, base.mu,
                                               None if root == "fixed" else base.v)
    else:
        model = OM.UnivariateOrnsteinUhlenbeck(rng.uniform(0.5, 2), rng.uniform(0.1, 1), rng.normal(), rng.normal(),
                                               {"fixed": 0.0, "random": 0.8, "improper": np.inf}[root])
    tbl = [list(rng.normal(size=len(taxa))) for _ in range(p)]
    return net, model, tbl, taxa


def missing_case():
    """p = 3 on a random network (20 tips, 4 hybrids), 30 % of the values missing (the pattern of
    test_gradient_missing_values); every tip keeps at least one value."""
    rng = np.random.default_rng(21)
    net = ON.random_network(20, 4, rng)
    taxa = net.tip_names
    p = 3
    tbl = [[None if rng.random() < 0.3 else float(rng.normal()) for _ in taxa] for _ in range(p)]
    for r in range(len(taxa)):
        if all(tbl[t][r] is None for t in range(p)):
            tbl[0][r] = float(rng.normal())
    return net, bm(p, rng, "random"), tbl, taxa


def no_data_case(root="random"):
    """exact_reml_missing of the reference's tests: a subtree whose tips have no value -- they are not tip families."""
    g = G["exact_reml_missing"]
    return ON.read_newick(g["net"]), bm(1, np.random.default_rng(3), root), [g["x"]], g["taxa"]


def wavefront_case():
    """A 12-tip tree at p = 16: clusters of 32 variables, packed (BS16) after a calibration."""
    rng = np.random.default_rng(5)
    tree = ON.random_network(12, 0, rng)
    tbl = [list(rng.normal(size=12)) for _ in range(16)]
    return tree, bm(16, rng, "random"), tbl, tree.tip_names


def star_case(n=9, p=2):
    """A star tree with a fixed root: no parent is in scope, every S = 0."""
    rng = np.random.default_rng(33)
    nwk = "(" + ",".join(f"t{i}:{rng.uniform(0.2, 1.5):.6f}" for i in range(n)) + ");"
    net = ON.read_newick(nwk)
    taxa = net.tip_names
    return net, bm(p, rng, "fixed"), [list(rng.normal(size=n)) for _ in range(p)], taxa


def two_tip_case():
    """Two tips, an improper root, p = 2, tip a observed at trait 0 only and tip b at trait 1 only: without either tip the
    root's matching trait has no information (flat prior): D = V - S is singular for each tip."""
    net = ON.read_newick("(a:0.7,b:1.3);")
    return net, bm(2, np.random.default_rng(4), "improper"), [[0.3, None], [None, -1.1]], net.tip_names


def two_tip_complete_case():
    """The same two-tip tree with complete data: the other tip determines the root, the prediction of a tip is proper
    (N(y_other, (t_a + t_b) R))."""
    net = ON.read_newick("(a:0.7,b:1.3);")
    return net, bm(2, np.random.default_rng(4), "improper"), [[0.3, 0.9], [0.4, -1.1]], net.tip_names


def batch_case(p, n_sites=64, ntips=40):
    """A 40-tip tree, fixed root, 64 sites with their own data and parameters: (newick, taxa, data [sites, tips, p],
    R [sites, p, p], mu [sites, p])."""
    from pgbp_amd import synth as S
    rng = np.random.default_rng(70 + p)
    tr = S.random_tree(ntips, rng)
    names = [f"n{i}" for i in range(tr.nnodes)]
    taxa = [names[i] for i in range(tr.nnodes) if tr.is_leaf[i]]
    data = rng.normal(size=(n_sites, len(taxa), p))
    Rs = np.stack([(lambda A: A @ A.T / p + np.eye(p))(rng.normal(size=(p, p))) for _ in range(n_sites)])
    return tr.newick(names), taxa, data, Rs, rng.normal(size=(n_sites, p))


def batch_site(p, s):
    """Site s of batch_case as an oracle case."""
    import pgbp_amd as P
    nwk, taxa, data, Rs, mus = batch_case(p)
    onet = ON.read_newick(nwk)
    onet.set_preorder(P.read_newick(nwk)[1])
    return onet, OM.MvFullBrownianMotion(Rs[s], mus[s]), [list(data[s][:, t]) for t in range(p)], taxa

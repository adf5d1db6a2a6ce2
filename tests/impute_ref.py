"""Comparators of the imputation sweep (pgbp_lg_impute / ClusterGraphBelief.impute_lg), host side, shared by
test_impute_cpu.py and test_gpu_impute.py (tests only):

(a) `dense_impute`: the DENSE comparator on oracle/densemvn.py alone (no message passing): the joint of node_moments
    conditioned on ALL observed tip values, with the flat root prior (universal kriging) for an improper root, exactly as
    loo_ref.dense_loo does -- for every missing entry of every tip;
(b) `impute_sweep`: a numpy restatement of the device sweep from J^-1 h and J^-1 of each listed family's cluster;
and the cases both test files run, so that (b) is pinned to (a) on the CPU for every input the GPU tests use."""
import numpy as np

import loo_ref as LR
from helpers import lg_inputs_from_oracle, oracle_setup
from oracle import calibration as OC
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import network as ON


# ----------------------------------------------------------------------------- (a) the dense comparator

def dense_impute(net, model, tbl, taxa):
    """{taxon row: (missing traits, mean, cov)} of the posterior of every missing entry given all observed tip values."""
    p = model.dimension()
    v = np.atleast_2d(np.asarray(model.rootpriorvariance(), float))
    improper = bool(np.any(np.isinf(np.diag(v))))
    if improper:
        m0, S, A = OD.node_moments(net, model, np.zeros(p), np.zeros((p, p)))
    else:
        m0, S, A = OD.node_moments(net, model)
    obs = LR._observed(net, tbl, taxa, p)
    po = np.array([i * p + t for i, _, t in obs], dtype=int)
    y = np.array([float(tbl[t][r]) for _, r, t in obs])
    Soo = S[np.ix_(po, po)]
    res = y - m0[po]
    out = {}
    for i, n in enumerate(net.vec_node):
        if not n.leaf:
            continue
        r = list(taxa).index(n.name)
        miss = [t for t in range(p) if tbl[t][r] is None]
        if not miss:
            continue
        pt = np.array([i * p + t for t in miss], dtype=int)
        Sto, Stt = S[np.ix_(pt, po)], S[np.ix_(pt, pt)]
        G_ = np.linalg.solve(Soo, Sto.T).T
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
        out[r] = (np.array(miss, dtype=int), mean, cov)
    return out


# ----------------------------------------------------------------------------- (b) the sweep, restated

def listed_families(fam):
    """(families, predicted masks) of the table: the tip families with a missing trait, and per family the missing traits
    every cluster parent holds in scope."""
    cm, pm = fam.get("child_mask"), fam.get("parent_mask")
    fams, pred = [], []
    if cm is None:
        return np.zeros(0, np.int32), np.zeros(0, np.uint64)
    p, K = int(fam["p"]), max(1, int(fam["max_parents"]))
    full = (1 << p) - 1
    for f in range(len(fam["cluster"])):
        if not (fam["child_pos"][f] < 0 and fam["data_row"][f] >= 0 and fam["n_parents"][f] >= 1):
            continue
        M = full & ~int(cm[f])
        if not M:
            continue
        P = M
        for k in range(int(fam["n_parents"][f])):
            mk = int(pm[f * K + k]) & full
            if not (fam["parent_pos"][f * K + k] < 0 and mk == full):      # a cluster parent
                P &= mk
        fams.append(f)
        pred.append(P)
    return np.array(fams, np.int32), np.array(pred, np.uint64)


def mask_bits(masks, p):
    return np.array([[(int(m) >> t) & 1 for t in range(p)] for m in masks], dtype=bool).reshape(len(masks), p)


def impute_sweep(fam, data, R, mu, moments, model="bm", alpha=None, theta=None):
    """fam: the table of lg_families; data [n_rows, p]; R [n_rates, p, p]; moments(c) -> (J^-1 h, J^-1) of cluster c (None
    when the belief is not positive definite).  Returns the dict of impute_lg for one site."""
    p, K = int(fam["p"]), max(1, int(fam["max_parents"]))
    R = np.asarray(R, float).reshape(-1, p, p)
    mu = np.asarray(mu, float).reshape(p)
    fams, pred = listed_families(fam)
    n = len(fams)
    mean, cov = np.full((n, p), np.nan), np.full((n, p, p), np.nan)
    info = np.zeros(n, np.int32)
    full = (1 << p) - 1
    rank = lambda mask, t: bin(int(mask) & ((1 << t) - 1)).count("1")
    th = np.asarray(theta, float).reshape(p) if model == "ou" else np.zeros(p)
    for ti, f in enumerate(fams):
        Pm = int(pred[ti])
        if not Pm:
            info[ti] = -1
            continue
        O = int(fam["child_mask"][f]) & full
        o = [t for t in range(p) if (O >> t) & 1]
        q = [t for t in range(p) if (Pm >> t) & 1]
        z = o + q
        no = len(o)
        npar = int(fam["n_parents"][f])
        qc, vc, wc = [], [], []
        for k in range(npar):
            t_, g_ = fam["length"][f * K + k], fam["gamma"][f * K + k]
            if model == "ou":
                a = np.exp(-alpha * t_)
                qc.append(g_ * a); vc.append(g_ * g_ * (1 - a * a)); wc.append(g_ * (1 - a))
            else:
                qc.append(g_); vc.append(g_ * g_ * t_); wc.append(0.0)
        V = sum(vc[k] * R[fam["color"][f * K + k]] for k in range(npar))[np.ix_(z, z)]
        w = sum(wc) * th[z]
        eu = np.zeros(len(z))
        Cu = np.zeros((len(z), len(z)))
        cluster = []
        for k in range(npar):
            mk = int(fam["parent_mask"][f * K + k]) & full
            if fam["parent_pos"][f * K + k] < 0 and mk == full:
                eu = eu + qc[k] * mu[z]
            else:
                cluster.append((k, mk))
        if cluster:
            mom = moments(int(fam["cluster"][f]))
            if mom is None:
                info[ti] = 1
                continue
            cm_, cS = mom
            idx = {k: [int(fam["parent_pos"][f * K + k]) + rank(mk, t) for t in z] for k, mk in cluster}
            for k, _ in cluster:
                eu = eu + qc[k] * cm_[idx[k]]
            for a, _ in cluster:
                for b, _ in cluster:
                    Cu = Cu + qc[a] * qc[b] * cS[np.ix_(idx[a], idx[b])]
        y = np.asarray(data, float)[fam["data_row"][f], o]
        Voo, Vop, Vpp = V[:no, :no], V[:no, no:], V[no:, no:]
        try:
            if no:
                np.linalg.cholesky(Voo)
            B = np.linalg.solve(Voo, Vop).T if no else np.zeros((len(q), 0))
            C = Vpp - B @ Vop
            np.linalg.cholesky(C)
        except np.linalg.LinAlgError:
            info[ti] = 1
            continue
        T = np.hstack([-B, np.eye(len(q))])
        mean[ti, q] = eu[no:] + w[no:] + B @ (y - w[:no] - eu[:no])
        cov[np.ix_([ti], q, q)] = T @ Cu @ T.T + C
    return dict(families=fams, rows=np.asarray(fam["data_row"])[fams], predicted=mask_bits(pred, p), mean=mean, cov=cov,
                info=info)


def oracle_impute(net, model, tbl, taxa):
    """(b) on the oracle's calibrated clique tree: (impute dict, the family table)."""
    import pgbp_amd as P
    cg = OCG.cliquetree(net)
    ocgb = oracle_setup(net, cg, model, tbl, taxa)
    fam, data, kw = lg_inputs_from_oracle(P, net, ocgb, model, tbl, taxa)
    spt = OCG.spanningtree_clusterlist(cg, OCG.default_rootcluster(cg, net))
    assert OC.calibrate(ocgb, [spt], verbose=False)[0]
    d = impute_sweep(fam, data, kw["R"], kw["mu"], LR.oracle_moments(ocgb), kw.get("model", "bm"), kw.get("alpha"),
                     kw.get("theta"))
    return d, fam


# ----------------------------------------------------------------------------- comparison

def counts(tbl, d):
    """(missing entries of the table, predicted entries of the dict)."""
    return sum(v is None for col in tbl for v in col), int(np.sum(d["predicted"]))


def worst_error(d, dense, symmetric=False):
    """Largest rel_block of mean / cov of the listed tips of `d` against `dense`; asserts that every tip with a missing entry
    is listed, that the NaN pattern of mean and cov equals `predicted`, and info (0 where something is predicted, else -1);
    symmetric: cov must be symmetric to the bit (the device mirrors one triangle)."""
    rows = [int(r) for r in d["rows"]]
    assert sorted(rows) == sorted(dense), (rows, sorted(dense))
    worst = 0.0
    for ti, r in enumerate(rows):
        miss, mean, cov = dense[r]
        pr = d["predicted"][ti]
        assert not np.any(pr[[t for t in range(len(pr)) if t not in set(miss.tolist())]]), (r, pr, miss)
        assert d["info"][ti] == (0 if pr.any() else -1), (r, d["info"][ti])
        assert np.array_equal(np.isfinite(d["mean"][ti]), pr), (r, d["mean"][ti], pr)
        assert np.array_equal(np.isfinite(d["cov"][ti]), np.outer(pr, pr)), r
        if not pr.any():
            continue
        q = np.flatnonzero(pr)
        sel = np.array([list(miss).index(t) for t in q])
        worst = max(worst, LR.rel_block(d["mean"][ti][q], mean[sel]),
                    LR.rel_block(d["cov"][ti][np.ix_(q, q)], cov[np.ix_(sel, sel)]))
        assert not symmetric or np.array_equal(d["cov"][ti][np.ix_(q, q)], d["cov"][ti][np.ix_(q, q)].T), r
    return worst


# ----------------------------------------------------------------------------- the cases

def masked(tbl, seed, frac):
    """The table with each entry dropped with probability frac (rows outer, traits inner); whole tips may lose all data."""
    rng = np.random.default_rng(seed)
    tbl = [list(col) for col in tbl]
    for r in range(len(tbl[0])):
        for t in range(len(tbl)):
            if rng.random() < frac:
                tbl[t][r] = None
    return tbl


def masked_random_case(which, p, seed, frac):
    net, model, tbl, taxa = LR.random_case(which, p)
    return net, model, masked(tbl, seed, frac), taxa


def tree_case(n, p, seed, frac):
    rng = np.random.default_rng(seed)
    tree = ON.random_network(n, 0, rng)
    tbl = [[None if rng.random() < frac else float(rng.normal()) for _ in range(n)] for _ in range(p)]
    for r in range(n):
        if all(tbl[t][r] is None for t in range(p)):
            tbl[0][r] = float(rng.normal())
    return tree, LR.bm(p, rng, "random"), tbl, tree.tip_names


def missing_case(root="random"):
    """loo_ref.missing_case; fixed / improper: the same network and table under loo_ref.bm(3, default_rng(2), root)."""
    net, model, tbl, taxa = LR.missing_case()
    if root != "random":
        model = LR.bm(3, np.random.default_rng(2), root)
    return net, model, tbl, taxa


# (which, p, seed, frac, (missing, predicted))
MASKED = [("bm_fixed", 2, 0, 0.15, (7, 7)), ("bm_fixed", 2, 2, 0.15, (4, 2)), ("bm_improper", 2, 0, 0.15, (7, 3)),
          ("bm_improper", 2, 1, 0.15, (6, 5)), ("bm_random", 4, 1, 0.15, (12, 10)), ("bm_random", 4, 2, 0.15, (15, 11)),
          ("ou_random", 1, 1, 0.15, (3, 3)), ("ou_random", 1, 3, 0.15, (4, 3)), ("ou_improper", 1, 3, 0.15, (4, 3)),
          ("ou_fixed", 1, 5, 0.25, (6, 5)), ("hetero_random", 2, 5, 0.25, (13, 10))]
MISSING_ROOTS = [("random", (17, 14)), ("fixed", (17, 14)), ("improper", (17, 14))]
WAVEFRONT = ((12, 16, 0, 0.1), (22, 20))     # clusters of 32 variables
WORKGROUP = ((6, 40, 2, 0.05), (11, 9))      # clusters of 80 variables
PACKED_COUNTS = (54, 54)                    # packed_case: every missing entry is predicted
TOO_BIG = (5, 64, 0, 0.03)                   # clusters of 128 variables: over the LDS


def batch_pattern(p=2):
    """One NaN pattern [tips, p] (True = missing) for loo_ref.batch_case(p): tips in taxon order, a tip is masked (trait 0,
    trait 1 or both, in turn) with probability 0.3 unless a sibling tip is masked already -- at most one tip of any cherry,
    so that every internal node keeps its full scope."""
    import pgbp_amd as P
    nwk, taxa, *_ = LR.batch_case(p)
    net, names = P.read_newick(nwk)
    row = {t: r for r, t in enumerate(taxa)}
    parent = {names[i]: net.node2family[i][1] for i in range(net.nnodes) if net.is_leaf[i]}
    rng = np.random.default_rng(9)
    miss = np.zeros((len(taxa), p), bool)
    taken, kind = set(), 0
    for t in taxa:
        if rng.random() < 0.3 and parent[t] not in taken:
            taken.add(parent[t])
            miss[row[t]] = [(True, False), (False, True), (True, True)][kind % 3][:p] if p > 1 else [True]
            kind += 1
    return miss


def batch_site(p, s):
    """Site s of loo_ref.batch_case(p) under batch_pattern as an oracle case."""
    onet, model, tbl, taxa = LR.batch_site(p, s)
    miss = batch_pattern(p)
    tbl = [[None if miss[r, t] else tbl[t][r] for r in range(len(taxa))] for t in range(p)]
    return onet, model, tbl, taxa


def packed_case():
    """loo_ref.wavefront_case (a 12-tip tree at p = 16, complete data) with entries of at most one tip of any cherry masked
    (each trait of a chosen tip with probability 0.4; one tip loses everything): every internal node keeps its full scope, every
    cluster has 16 or 32 variables and the engine holds them in the packed (BS16) layout after a calibration."""
    net, model, tbl, taxa = LR.wavefront_case()
    rng = np.random.default_rng(17)
    tbl = [list(col) for col in tbl]
    taken, first = set(), True
    for n in net.vec_node:
        if not n.leaf:
            continue
        par = id(net.parent_edges(n)[0].parent)
        if par in taken or rng.random() >= 0.6:
            continue
        taken.add(par)
        r = list(taxa).index(n.name)
        for t in range(16):
            if first or rng.random() < 0.4:
                tbl[t][r] = None
        first = False
    return net, model, tbl, taxa


def tree_newick(tree):
    """Newick string of an oracle TREE, every node named, lengths written so that they read back to the same doubles."""
    def sub(n):
        kids = tree.child_edges(n)
        s = ("(" + ",".join(sub(e.child) + ":" + repr(float(e.length)) for e in kids) + ")") if kids else ""
        return s + n.name
    return sub(tree.root) + ";"


def full_scope_setup(tree, model, tbl, taxa):
    """An oracle tree case (full BM, proper random root) set up with the product's own host side and EVERY trait of every
    internal node in scope (allocate_scopes without `data`), whatever the tips below observe: the same joint distribution on a
    clique tree whose clusters all have p or 2p variables -- a trait no tip below a node observes stays a variable that only
    the edge above informs.  Returns a dict: arrays (arguments of ClusterGraphBelief.from_arrays), spt (schedule tree), fam
    (family table), data [rows, p], kw (keyword arguments of assignfactors_lg_), clusters (scopes), names (node names)."""
    import pgbp_amd as P
    p = model.dimension()
    net, names = P.read_newick(tree_newick(tree))
    row = {t: r for r, t in enumerate(taxa)}
    data = np.array([[np.nan if tbl[t][r] is None else float(tbl[t][r]) for t in range(p)] for r in range(len(taxa))])
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=False)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], p, n_rates=2, root_prior_color=1, data=data)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    kw = dict(R=np.stack([np.asarray(model.R, float), np.asarray(model.rootpriorvariance(), float)]),
              mu=model.rootpriormeanvector())
    return dict(arrays=(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None), spt=spt, fam=fam, data=data, kw=kw,
                clusters=st.clusters, names=names)


def dense_cluster_moments(tree, model, tbl, taxa, setup):
    """moments(c) of impute_sweep for the clusters of full_scope_setup from the DENSE posterior of all node states
    (oracle/densemvn.posterior_node_moments: no message passing): what a calibrated clique tree holds."""
    p = model.dimension()
    pm, pc = OD.posterior_node_moments(tree, model, tbl, taxa)
    at = {n.name: i for i, n in enumerate(tree.vec_node)}

    def mom(c):
        b = setup["clusters"][c]
        insc = np.asarray(b.inscope, bool)
        idx = [at[setup["names"][lab - 1]] * p + t for j, lab in enumerate(b.nodelabel) for t in range(p) if insc[t, j]]
        return pm[idx], pc[np.ix_(idx, idx)]
    return mom

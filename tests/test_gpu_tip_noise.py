"""Measurement error at the tips on the device: pgbp_lg_set_tip_noise / set_tip_noise_lg, the correction of the factor fill
(csrc/pgbp_noise.hip), the five sweeps under noise and dsigma_e.

Comparator: noise_ref.NoisyTipModel around the untouched oracle -- densely (densemvn: loglik, posterior_node_moments, and
through it loo_ref.dense_loo, impute_ref.dense_impute) and as belief propagation (oracle.beliefs.assignfactors of the generic
factors) --, both pinned to each other and to finite differences in test_tip_noise_cpu.py.  Noise is drawn with diag(E)
between 0.01 and 100 times diag(V) of each tip (noise_ref.draw_noise asserts it), where the statement itself stays inside
1e-8 (test_tip_noise_cpu.py).  Every comparison at 1e-8 relative to the largest entry of the block; the measured figure of
every case is printed."""
import numpy as np
import pytest

import impute_ref as IR
import loo_ref as LR
import noise_ref as NR
from edge_ref import rel_block_nan
from helpers import lg_inputs_from_oracle, oracle_setup, product_beliefs_from_oracle
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from shift_ref import ShiftedModel, family_edge, family_nodes
from test_gpu_shifts import MODELS, _bytes, _device, _edges_values, _model_case, _pick, _records_error
from test_gradient_cpu import rel_block, richardson

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


# ----------------------------------------------------------------------------- set-up

def _tips(fam):
    cm = fam.get("child_mask")
    return [f for f in range(len(fam["cluster"])) if fam["child_pos"][f] < 0 and fam["data_row"][f] >= 0
            and fam["n_parents"][f] >= 1 and (cm is None or int(cm[f]) != 0)]


def _noisy(fam):
    """The noisy tips of a case: every second tip family, and with them every hybrid tip (several parent edges), every tip with
    a partial child_mask and a pair of tips that share a cluster, where the table has such."""
    tips = _tips(fam)
    pick = set(tips[::2])
    pick |= {f for f in tips if fam["n_parents"][f] >= 2}
    cm = fam.get("child_mask")
    if cm is not None:
        full = (1 << int(fam["p"])) - 1
        pick |= {f for f in tips if int(cm[f]) != full}
    by_cl = {}
    for f in tips:
        by_cl.setdefault(int(fam["cluster"][f]), []).append(f)
    pair = next((v for v in by_cl.values() if len(v) >= 2), None)
    if pair:
        pick |= set(pair[:2])
    return np.array(sorted(pick), np.int32)


def _draw(fam, kw, families, seed, with_se2=True):
    return NR.draw_noise(fam, kw["R"], families, np.random.default_rng(seed), model=kw.get("model", "bm"), alpha=kw.get("alpha"),
                         with_se2=with_se2)


def _set(pcgb, fam, kw, seed=3, with_se2=True):
    """Draw and set the noise of a one-site case: (families, scale, sigma_e, se2, E [n, p, p])."""
    families = _noisy(fam)
    scale, sigma_e, se2 = _draw(fam, kw, families, seed, with_se2)
    pcgb.set_tip_noise_lg(families, sigma_e, scale, se2)
    assert pcgb.tip_noise_count_lg() == len(families)
    return families, scale, sigma_e, se2, NR.tip_noise(scale, sigma_e, se2)


# ----------------------------------------------------------------------------- 1: the fill, record by record

@pytest.mark.parametrize("graph", ["cliquetree", "bethe", "joingraph"])
@pytest.mark.parametrize("which,p", MODELS)
def test_fill_records_against_the_wrapper(P, which, p, graph):
    """set_tip_noise_lg + assignfactors_lg_ against the oracle's assignfactors of the wrapper, every cluster's (J, h, g), on
    the clique tree, the Bethe graph and a join graph of the 24-tip networks (complete data): heterogeneous BM, the OU with a
    fixed and a random root, an improper root.  (These networks have no hybrid TIP: the two tests of section 3b do.)"""
    net, model, tbl, taxa = LR.random_case(which, p)
    cg, ocgb, pcgb, fam, kw, _ = _device(P, net, model, tbl, taxa, graph, assign=False)
    families, scale, sigma_e, se2, E = _set(pcgb, fam, kw)
    pcgb.assignfactors_lg_(**kw)
    ocgb_w = oracle_setup(net, cg, NR.wrapper(net, ocgb, fam, model, families, E), tbl, taxa)
    err, plain = _records_error(pcgb, ocgb_w), _records_error(pcgb, ocgb)
    nh = int(np.sum(np.asarray(fam["n_parents"])[families] >= 2))
    print(f"{which}/p{p}/{graph}: {len(families)} noisy tips ({nh} below a hybrid), records vs the oracle's {err:.2e} "
          f"(vs the noiseless {plain:.2e})")
    assert err <= TOL and plain > 1e-3


# ----------------------------------------------------------------------------- 2: the likelihood

def _missing(root):
    return IR.missing_case(root)


LOGLIK = [(w, p, None) for w, p in MODELS] + [("bm_fixed", 1, None), ("bm_random", 4, None)] + \
         [("missing", 3, r) for r in ("random", "fixed", "improper")]


@pytest.mark.parametrize("which,p,root", LOGLIK)
def test_loglik_under_noise(P, which, p, root):
    """loglik_lg against densemvn.loglik of the wrapper: the 24-tip networks, and the p = 3 network with 30 % missing values
    under a random, a fixed and an improper root.  reps = 3 returns the bytes of reps = 1; noise with and without se2."""
    net, model, tbl, taxa = _missing(root) if which == "missing" else LR.random_case(which, p)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa, oracle_factors=(which != "missing"))
    pcgb._ensure_schedule([spt])
    plain = OD.loglik(net, model, tbl, taxa)
    for with_se2 in (True, False):
        families, scale, sigma_e, se2, E = _set(pcgb, fam, kw, with_se2=with_se2)
        ll, info = pcgb.loglik_lg()
        dense = OD.loglik(net, NR.wrapper(net, ocgb, fam, model, families, E), tbl, taxa)
        ll3, _ = pcgb.loglik_lg(reps=3)
        e1 = abs(ll[0] - dense) / max(1.0, abs(dense))
        print(f"{which}/p{p}/{root} se2={with_se2}: loglik vs dense {e1:.2e} ({dense:.6f}, noiseless {plain:.6f})")
        assert info[0] == 0 and e1 <= TOL and ll3.tobytes() == ll.tobytes()
        assert abs(dense - plain) > 1e-3


def test_loglik_against_the_pendant_node_engine(P):
    """What a user had to do before: a second node under every noisy tip on an edge of its own rate colour, heterogeneous
    BM.  Two device engines -- the tree with set_tip_noise_lg, the doubled tree without -- give the same log-likelihood."""
    rng = np.random.default_rng(12)
    p, n = 2, 12
    tree = ON.random_network(n, 0, rng)
    tree.name_internal_nodes()
    taxa = tree.tip_names
    tbl = [list(rng.normal(size=n)) for _ in range(p)]
    model = LR.bm(p, rng, "random")
    cg, ocgb, pcgb, fam, kw, spt = _device(P, tree, model, tbl, taxa)
    pcgb._ensure_schedule([spt])
    families = np.array(_tips(fam)[::2], np.int32)
    names = [tree.vec_node[family_nodes(ocgb, fam)[f]].name for f in families]
    scale = rng.uniform(0.05, 1.0, size=len(families))
    A = rng.normal(size=(p, p))
    sigma_e = A @ A.T / p + 0.3 * np.eye(p)
    pcgb.set_tip_noise_lg(families, sigma_e, scale)
    ll, info = pcgb.loglik_lg()
    net2, model2 = NR.pendant_case(tree, model.R, sigma_e, model.rootpriormeanvector(), model.rootpriorvariance(), names, scale)
    _, _, pend, _, _, spt2 = _device(P, net2, model2, tbl, taxa)
    pend._ensure_schedule([spt2])
    ll2, info2 = pend.loglik_lg()
    err = abs(ll[0] - ll2[0]) / max(1.0, abs(ll2[0]))
    print(f"tip noise {ll[0]:.10f} vs pendant nodes {ll2[0]:.10f}: {err:.2e} ({pend.nclusters} clusters instead of {pcgb.nclusters})")
    assert info[0] == 0 and info2[0] == 0 and err <= TOL


# ----------------------------------------------------------------------------- 3: the layouts

def _tree_setup(P, p, seed, oracle_scopes=False):
    """A 12-tip tree with a proper random root: (tree, model, tbl, device beliefs, schedule tree, assignfactors_lg_ keywords,
    family table, oracle node index of every family).  p = 16: loo_ref.wavefront_case on the oracle's clique tree (packed
    after a calibration); oracle_scopes: impute_ref.tree_case at p = 16 with missing values, clusters of 15, 16, 31 and 32
    variables (plain); else the product's own host side (impute_ref.full_scope_setup: clusters of p or 2p variables)."""
    rng = np.random.default_rng(seed)
    if p == 16 or oracle_scopes:
        tree, model, tbl, taxa = IR.tree_case(*IR.WAVEFRONT[0]) if oracle_scopes else LR.wavefront_case()
        cg, ocgb, pcgb, fam, kw, spt = _device(P, tree, model, tbl, taxa, oracle_factors=not oracle_scopes)
        return tree, model, tbl, pcgb, spt, kw, fam, family_nodes(ocgb, fam)
    tree = ON.random_network(12, 0, rng)
    tbl = [list(rng.normal(size=12)) for _ in range(p)]
    model = LR.bm(p, rng, "random")
    su = IR.full_scope_setup(tree, model, tbl, tree.tip_names)
    pcgb = P.ClusterGraphBelief.from_arrays(*su["arrays"])
    pcgb.lg_setup(su["fam"], su["data"])
    pcgb.assignfactors_lg_(**su["kw"])
    at = {n.name: i for i, n in enumerate(tree.vec_node)}
    return tree, model, tbl, pcgb, su["spt"], su["kw"], su["fam"], [at[su["names"][f]] for f in range(len(su["fam"]["cluster"]))]


def _tree_wrapper(tree, model, nodes, families, E):
    pre = tree.vec_node
    return NR.NoisyTipModel(model, {tree.parent_edges(pre[nodes[int(f)]])[0].number: e for f, e in zip(families, E)})


@pytest.mark.parametrize("p,layout,oracle_scopes", [(2, 1, False), (16, 1, False), (16, 0, True), (3, 0, False), (40, 0, False)])
def test_layouts_plain_packed_and_large_p(P, p, layout, oracle_scopes):
    """A 12-tip tree: p = 2 and p = 16 are held in the packed BS16 layout after a calibration, and the correction then writes
    packed records, both triangles of the diagonal 2 x 2 blocks (the layout is asserted before and after); p = 16 with the
    scopes the oracle allocates from data with missing values (clusters of 15 / 31 variables) and p = 3 stay plain; p = 40
    needs more than 64 KB of LDS and the 256-thread instances of the sweeps.  loglik_lg, and a second assignfactors_lg_ + full
    calibration + gradient, against the dense wrapper."""
    tree, model, tbl, pcgb, spt, kw, fam, nodes = _tree_setup(P, p, 40 + p, oracle_scopes)
    pcgb._ensure_schedule([spt])
    ll0, _ = pcgb.loglik_and_edge_gradient_lg(spt)   # (a calibration: the engine takes the layout its kernels want)
    assert pcgb._lib.pgbp_layout(pcgb._eng) == layout, (p, pcgb._lib.pgbp_layout(pcgb._eng))
    if oracle_scopes:
        assert sorted(set(int(m) for m in pcgb._dims[: pcgb.nclusters])) == [15, 16, 31, 32]
    families, scale, sigma_e, se2, E = _set(pcgb, fam, kw)
    ll, info = pcgb.loglik_lg()
    assert pcgb._lib.pgbp_layout(pcgb._eng) == layout
    w = _tree_wrapper(tree, model, nodes, families, E)
    dense = OD.loglik(tree, w, tbl, tree.tip_names)
    pcgb.assignfactors_lg_(**kw)            # beliefs and factors, in the layout the engine is in
    assert pcgb._lib.pgbp_layout(pcgb._eng) == layout
    ll2, g = pcgb.loglik_and_gradient_lg(spt)
    st = NR.dense_statement(tree, w, model, {}, {nodes[int(f)]: e for f, e in zip(families, E)},
                            {nodes[int(f)]: s for f, s in zip(families, scale)}, tbl, tree.tip_names)
    e1, e2 = abs(ll[0] - dense) / abs(dense), abs(ll2 - dense) / abs(dense)
    e3, e4 = rel_block(g["dsigma_e"], st["dsigma_e"]), rel_block(g["dR"][0], st["dR"][0])
    print(f"12-tip tree p={p} layout {layout}: loglik_lg vs dense {e1:.2e}, after assignfactors + calibrate {e2:.2e}, "
          f"dsigma_e {e3:.2e}, dR {e4:.2e}")
    assert info[0] == 0 and max(e1, e2, e3, e4) <= TOL
    assert abs(ll[0] - ll0) > 1e-3


def test_packed_and_plain_setups_of_the_p16_tree_agree(P):
    """The same p = 16 tree and noise on an engine that is in the packed layout (after a calibration) and on a fresh one in
    the plain layout: the filled records agree to 1e-12 of each record's largest entry."""
    recs = []
    for calibrate_first in (True, False):
        tree, model, tbl, pcgb, spt, kw, fam, nodes = _tree_setup(P, 16, 56)
        if calibrate_first:
            pcgb.loglik_and_edge_gradient_lg(spt)
        assert pcgb._lib.pgbp_layout(pcgb._eng) == (1 if calibrate_first else 0)
        _set(pcgb, fam, kw)
        pcgb.assignfactors_lg_(**kw)
        assert pcgb._lib.pgbp_layout(pcgb._eng) == (1 if calibrate_first else 0)
        pcgb.pull()
        recs.append([tuple(np.array(x, float).copy() for x in pcgb._views(0, c)) for c in range(pcgb.nclusters)])
    worst = 0.0
    for a, b in zip(*recs):
        for x, y in zip(a, b):
            if x.size:
                worst = max(worst, float(np.max(np.abs(np.triu(x) - np.triu(y)) if x.ndim == 2 else np.abs(x - y)))
                            / max(float(np.max(np.abs(y))), 1.0))
    print(f"p = 16 tree, packed vs plain fill with noise: {worst:.2e}")
    assert worst <= 1e-12


def _batch(P, p, n_sites):
    """loo_ref.batch_case at n_sites: a 40-tip tree, fixed root, every site its own data and parameters."""
    nwk, taxa, data, Rs, mus = LR.batch_case(p, n_sites=n_sites)
    net, names = P.read_newick(nwk)
    row = {t: r for r, t in enumerate(taxa)}
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=True)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], p)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=n_sites)
    cgb.lg_setup(fam, data)
    cgb.assignfactors_lg_(Rs[:, None], mus)

    def site(s):
        onet = ON.read_newick(nwk)
        onet.set_preorder(names)
        return onet, OM.MvFullBrownianMotion(Rs[s], mus[s]), [list(data[s][:, t]) for t in range(p)], taxa
    site.mus = mus
    return cgb, spt, fam, Rs, site


def _batch_noise(fam, Rs, n_sites, p, seed):
    """Per-site sigma_e and se2 for every second tip of the batch: scale [n], sigma_e [sites, p, p], se2 [sites, n, p]."""
    families = np.array(_tips(fam)[::2], np.int32)
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.2, 1.0, size=len(families))
    sig, se2 = np.zeros((n_sites, p, p)), np.zeros((n_sites, len(families), p))
    for s in range(n_sites):
        sc, sg, s2 = NR.draw_noise(fam, Rs[s][None], families, rng)
        # (one scale per tip for all sites: fold the site's own scale into its se2, which keeps diag(E) where it was drawn)
        sig[s] = sg
        se2[s] = s2 + (sc - scale)[:, None] * np.diag(sg)[None, :]
        se2[s][se2[s] < 0] = 0.0
        Vd = np.array([np.diag(NR.family_variance(fam, Rs[s][None], int(f))) for f in families])
        r = (scale[:, None] * np.diag(sg)[None, :] + se2[s]) / Vd
        assert 0.01 <= r.min() and r.max() <= 100.0, (r.min(), r.max())
    return families, scale, sig, se2


@pytest.mark.parametrize("n_sites", [8, 64, 65])
def test_site_minor_batch_per_site_noise(P, n_sites):
    """p = 1: 8 sites stay in the plain layout, 64 and 65 take the site-minor one (thread = site, a second workgroup row at
    65) -- per-site sigma_e and se2 (the [entry][site] copy): loglik_lg of every site against the dense wrapper, then shared
    noise on the same engine, then noise together with per-site shifts."""
    cgb, spt, fam, Rs, site = _batch(P, 1, n_sites)
    cgb._ensure_schedule([spt])
    families, scale, sig, se2 = _batch_noise(fam, Rs, n_sites, 1, 9)
    cgb.set_tip_noise_lg(families, sig, scale, se2)
    ll, info = cgb.loglik_lg()
    assert bool(cgb._lib.pgbp_layout(cgb._eng) & 2) == (n_sites >= 64)
    sites = range(n_sites) if n_sites <= 8 else (0, 1, 31, 63, n_sites - 1)

    def dense(s, sg, s2, shifts=None):
        onet, model, tbl, taxa = site(s)
        pre = onet.vec_node
        inner = model if shifts is None else ShiftedModel(model, {onet.parent_edges(pre[f + 1])[0].number: v for f, v in shifts})
        E = NR.tip_noise(scale, sg, s2)
        return OD.loglik(onet, NR.NoisyTipModel(inner, {onet.parent_edges(pre[int(f) + 1])[0].number: e
                                                        for f, e in zip(families, E)}), tbl, taxa)
    worst = max(abs(ll[s] - dense(s, sig[s], se2[s])) / max(1.0, abs(ll[s])) for s in sites)
    cgb.set_tip_noise_lg(families, sig[1], scale, se2[1])
    lls, _ = cgb.loglik_lg()
    shared = max(abs(lls[s] - dense(s, sig[1], se2[1])) / max(1.0, abs(lls[s])) for s in sites)
    edges = [(int(families[0]), 0), (int(families[-1]), 0), (len(fam["cluster"]) // 2, 0)]
    values = np.random.default_rng(10).normal(size=(n_sites, len(edges), 1))
    cgb.set_tip_noise_lg(families, sig, scale, se2)
    cgb.set_shifts_lg(edges, values)
    assert cgb.tip_noise_count_lg() == len(families)      # (the noise survives set_shifts_lg)
    llb, _ = cgb.loglik_lg()
    both = max(abs(llb[s] - dense(s, sig[s], se2[s], [(f, v) for (f, _), v in zip(edges, values[s])])) / max(1.0, abs(llb[s]))
               for s in sites)
    print(f"univariate batch, {n_sites} sites: per-site noise {worst:.2e}, shared {shared:.2e}, with per-site shifts {both:.2e}")
    assert not info.any() and max(worst, shared, both) <= TOL


# ----------------------------------------------------------------------------- 3b: a tip below a hybrid

@pytest.mark.parametrize("graph_kind", ["cliquetree", "bethe"])
@pytest.mark.parametrize("name,kind", [("N1", "bm"), ("N1", "ou"), ("N4", "bm")])
def test_noise_on_a_hybrid_tip_univariate_batches(P, name, kind, graph_kind):
    """The networks of uni_net_ref whose hybrid node is a tip (a tip family with two parent edges; in N4 one of them is the
    fixed root), 8, 64 and 65 univariate sites with per-site parameters, sigma_e and se2; the hybrid tip and one more tip are
    noisy.  8 sites: the wavefront kernel; 64 and 65: the thread-per-site kernel.  Every site's records against the oracle's
    assignfactors of the wrapper (E_f / gamma^2 on the tip's first parent edge: V_f gains exactly E_f), loglik_lg against the
    dense wrapper on the clique trees."""
    import uni_net_ref as N
    rng = np.random.default_rng(17)
    for n in (8, 64, 65):
        b = N.device_batch(P, name, "fixed", kind, graph_kind, n, assign=False)
        hyb = int(np.flatnonzero(b.fam["n_parents"] >= 2)[0])
        assert b.fam["child_pos"][hyb] < 0 and b.fam["data_row"][hyb] >= 0
        families = np.array(sorted({hyb, next(f for f in _tips(b.fam) if f != hyb)}), np.int32)
        nodes = family_nodes(b.ocgb0, b.fam)
        pre = b.net.vec_node
        V = np.array([[float(NR.oracle_tip_variance(b.net, b.sites[s][0], pre[nodes[int(f)]])[0, 0]) for f in families]
                      for s in range(n)])
        E = np.exp(rng.uniform(np.log(0.05), np.log(100.0), size=V.shape)) * V     # diag(E) = 0.05 .. 100 x diag(V)
        scale = rng.uniform(0.2, 1.0, size=len(families))
        sig = 0.02 * V.min(axis=1)
        se2 = E - scale[None, :] * sig[:, None]
        assert se2.min() > 0
        b.pcgb.set_tip_noise_lg(families, sig.reshape(n, 1, 1), scale, se2.reshape(n, len(families), 1))
        b.pcgb.assignfactors_lg_(**b.kw)
        if n >= 64:
            assert b.pcgb._lib.pgbp_layout(b.pcgb._eng) & 2
        b.pcgb.pull()
        got = b.pcgb._packed_raw.copy()
        d = b.dims[:b.pcgb.nclusters].astype(np.int64)
        nclu = int(np.sum(d * d + d + 1))
        if graph_kind == "cliquetree":
            b.pcgb._ensure_schedule(b.sched)
            ll, info = b.pcgb.loglik_lg()
            assert not info.any()
        worst = plain = wll = 0.0
        for s in range(n):
            model, tbl = b.sites[s]
            w = NR.wrapper(b.net, b.ocgb0, b.fam, model, families, E[s].reshape(-1, 1, 1))
            want = N.pack(oracle_setup(b.net, b.cg, w, tbl, b.taxa))
            worst = max(worst, N.records_error(got[s, :nclu], want[:nclu], d))
            plain = max(plain, N.records_error(got[s, :nclu], N.oracle_factors(name, "fixed", kind, graph_kind, s)[:nclu], d))
            if graph_kind == "cliquetree":
                dense = OD.loglik(b.net, w, tbl, b.taxa)
                wll = max(wll, abs(ll[s] - dense) / max(1.0, abs(dense)))
        print(f"hybrid tip {name}/{kind}/{graph_kind}/{n} sites: records {worst:.2e} (vs the noiseless {plain:.2e}), "
              f"loglik vs dense {wll:.2e}")
        assert worst <= TOL and wll <= TOL and plain > 1e-3


@pytest.mark.parametrize("graph", ["cliquetree", "bethe"])
def test_noise_on_a_hybrid_tip_two_traits(P, graph):
    """N1 of uni_net_ref at p = 2, full BM with a random root: the hybrid tip's family (two parents in scope, both blocks
    and their cross blocks of Delta J) in the wavefront kernel: records against the oracle's assignfactors of the wrapper,
    loglik_lg and the sweeps against the dense wrapper."""
    import uni_net_ref as N
    net, taxa = N.network("N1")
    rng = np.random.default_rng(23)
    p = 2
    model = LR.bm(p, rng, "random")
    tbl = [list(rng.normal(size=len(taxa))) for _ in range(p)]
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa, graph, assign=False)
    families, scale, sigma_e, se2, E = _set(pcgb, fam, kw)
    assert (np.asarray(fam["n_parents"])[families] >= 2).any()
    pcgb.assignfactors_lg_(**kw)
    ocgb_w = oracle_setup(net, cg, NR.wrapper(net, ocgb, fam, model, families, E), tbl, taxa)
    err, plain = _records_error(pcgb, ocgb_w), _records_error(pcgb, ocgb)
    print(f"N1 at p = 2, {graph}: records vs the oracle's {err:.2e} (vs the noiseless {plain:.2e})")
    assert err <= TOL and plain > 1e-3
    if graph == "cliquetree":
        worst, _ = _sweep_errors(P, pcgb, spt, net, model, tbl, taxa, ocgb, fam, families, scale, E, [], np.zeros((0, p)))
        print("N1 at p = 2, sweeps: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        for k, v in worst.items():
            assert v <= TOL, (k, v)


# ----------------------------------------------------------------------------- 4: the sweeps under noise

def _sweep_errors(P, pcgb, spt, net, model, tbl, taxa, ocgb, fam, families, scale, E, edges, values):
    p = model.dimension()
    sh = {family_edge(net, ocgb, fam, f, k).number: v for (f, k), v in zip(edges, values)}
    w = NR.wrapper(net, ocgb, fam, ShiftedModel(model, sh) if sh else model, families, E)
    ll, got = pcgb.loglik_and_gradient_lg(spt)
    dense = OD.loglik(net, w, tbl, taxa)
    worst = dict(loglik=abs(ll - dense) / max(1.0, abs(dense)))
    noise, scales = NR.node_noise(ocgb, fam, families, E, scale)
    st = NR.dense_statement(net, w, model, sh, noise, scales, tbl, taxa)
    for k in ("dR", "dmu", "dalpha", "dtheta", "dsigma_e"):
        a, g = np.atleast_1d(np.asarray(st[k], float)), np.atleast_1d(np.asarray(got[k], float))
        if np.any(a) or np.any(g):
            worst[k] = rel_block(g, a)
    nodes = family_nodes(ocgb, fam)
    K = max(1, int(fam["max_parents"]))
    eg = pcgb.edge_gradient_lg()
    want = {k: np.full((len(nodes), K), np.nan) for k in ("dlength", "dgamma")}
    for f, i in enumerate(nodes):
        for k in range(int(fam["n_parents"][f])):
            ed = family_edge(net, ocgb, fam, f, k)
            kk = next(q for q, e2 in enumerate(st["edges"][i]) if e2 is ed)
            want["dlength"][f, k], want["dgamma"][f, k] = st["dlength"][i, kk], st["dgamma"][i, kk]
    for k in ("dlength", "dgamma"):
        worst[k] = rel_block_nan(eg[k], want[k])
    worst["dshift"] = rel_block_nan(eg["dshift"], st["dshift"][nodes])
    sc = pcgb.shift_scan_lg()
    real = np.asarray(fam["n_parents"]) >= 1
    assert np.array_equal(sc["identified"][real], st["identified"][nodes][real])
    worst["scan_jump"] = rel_block_nan(sc["jump"][real], st["jump"][nodes][real])
    worst["scan_lr"] = rel_block(sc["lr"][real], st["lr"][nodes][real])
    loo = pcgb.loo_lg()
    worst["loo"] = LR.worst_error(fam["data_row"][loo["families"]], loo, LR.dense_loo(net, w, tbl, taxa), p)
    if fam.get("child_mask") is not None:
        imp = pcgb.impute_lg()
        if len(imp["families"]):
            worst["impute"] = IR.worst_error(imp, IR.dense_impute(net, w, tbl, taxa))
    pm, _ = OD.posterior_node_moments(net, w, tbl, taxa)
    mom = pcgb.moments_(cov=False)
    e = 0.0
    for c in range(ocgb.nclusters):
        b = ocgb.belief[c]
        insc = np.asarray(b.inscope, bool)
        idx = [(lab - 1) * p + t for j, lab in enumerate(b.nodelabel) for t in range(p) if insc[t, j]]
        if idx:
            e = max(e, float(np.max(np.abs(mom[c][0] - pm[idx]))) / max(float(np.max(np.abs(pm))), 1e-300))
    worst["moments"] = e
    return worst, got


@pytest.mark.parametrize("shifted", [False, True], ids=["noise", "noise+shifts"])
@pytest.mark.parametrize("which,p", [("bm_random", 4), ("hetero_random", 2), ("ou_fixed", 1), ("ou_random", 1), ("missing", 3)])
def test_sweeps_under_noise(P, which, p, shifted):
    """Calibrated clique tree under noise, and under noise and shifts together: gradient_lg (dsigma_e among its outputs),
    edge_gradient_lg and shift_scan_lg against noise_ref.family_statement on the dense posterior of the wrapper (pinned in
    test_tip_noise_cpu.py), loo_lg against dense_loo(wrapper) and impute_lg against dense_impute(wrapper) -- both predict the
    OBSERVATION of a noisy tip --, moments_ means against posterior_node_moments(wrapper)."""
    net, model, tbl, taxa = _model_case(which, p)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    families, scale, sigma_e, se2, E = _set(pcgb, fam, kw)
    edges, values = _edges_values(_pick(fam, both_hybrid=True), p) if shifted else ([], np.zeros((0, p)))
    if shifted:
        pcgb.set_shifts_lg(edges, values)
    pcgb.assignfactors_lg_(**kw)
    worst, got = _sweep_errors(P, pcgb, spt, net, model, tbl, taxa, ocgb, fam, families, scale, E, edges, values)
    print(f"{which}/p{p}{' with shifts' if shifted else ''}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (k, v)
    assert np.max(np.abs(got["dsigma_e"])) > 1e-9 and np.array_equal(got["dsigma_e"], got["dsigma_e"].T)


@pytest.mark.parametrize("which,p", [("bm_random", 4), ("missing", 3)])
def test_dsigma_e_is_the_derivative_of_the_device_loglik(P, which, p):
    """tr(dsigma_e B) against the Richardson central difference of the device's own loglik_lg along symmetric directions B."""
    net, model, tbl, taxa = _model_case(which, p)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    families, scale, sigma_e, se2, E = _set(pcgb, fam, kw)
    pcgb.assignfactors_lg_(**kw)
    _, g = pcgb.loglik_and_gradient_lg(spt)
    rng = np.random.default_rng(4)
    worst = 0.0
    for _ in range(3):
        B = rng.normal(size=(p, p))
        B = (B + B.T) / 2 * np.sqrt(np.outer(np.diag(sigma_e), np.diag(sigma_e)))

        def f(s):
            pcgb.set_tip_noise_lg(families, sigma_e + s * B, scale, se2)
            return float(pcgb.loglik_lg()[0][0])
        fd = richardson(f, 1e-3)
        worst = max(worst, abs(float(np.sum(g["dsigma_e"] * B)) - fd) / max(abs(fd), 1e-300))
    print(f"{which}/p{p}: tr(dsigma_e B) vs the difference of loglik_lg, three directions {worst:.2e}")
    assert worst <= TOL


# ----------------------------------------------------------------------------- 4b: the joint fit

@pytest.mark.parametrize("gradient", ["analytic", "central"])
def test_joint_fit_of_R_mu_and_sigma_e(P, gradient):
    """calibrate_optimize_cliquetree_(..., sigma_e0=...) on data simulated from the noisy model on an 80-tip tree (p = 2,
    fixed root).  Half of the tips, at random, are single individuals (scale_f = 1), the others means of a hundred (0.01),
    the edges are short (0.02 .. 0.2) and Sigma_e has the size of R: the near-exact tips identify R, the others Sigma_e, and
    the maximum is interior (the dense likelihood on the host reaches the same one from three starts).  With edges of
    0.1 .. 1 and scale_f = 1 / (1 .. 8) on 40 to 120 tips the maximum sat on the boundary det Sigma_e = 0 or det R = 0, where
    the score does not vanish.  The score in (R, mu, Sigma_e) at the estimate is below 1e-6 of its size at the start,
    and the log-likelihood is not below that at the generating values."""
    rng = np.random.default_rng(31)
    p, n = 2, 80
    tree = ON.random_network(n, 0, rng, 0.02, 0.2)
    taxa = tree.tip_names
    A, B = rng.normal(size=(p, p)), rng.normal(size=(p, p))
    R_true, S_true, mu_true = A @ A.T / p + 0.5 * np.eye(p), B @ B.T / p + 0.5 * np.eye(p), rng.normal(size=p)
    truth = OM.MvFullBrownianMotion(R_true, mu_true)
    pre = tree.vec_node
    tips = [i for i, nd in enumerate(pre) if nd.leaf]
    sc = {pre[i].name: (1.0 if rng.integers(0, 2) else 0.01) for i in tips}
    w_true = NR.NoisyTipModel(truth, {tree.parent_edges(pre[i])[0].number: sc[pre[i].name] * S_true for i in tips})
    mean, cov, _ = OD.node_moments(tree, w_true)
    idx = np.array([i * p + t for i in tips for t in range(p)])
    x = rng.multivariate_normal(mean[idx], cov[np.ix_(idx, idx)]).reshape(len(tips), p)
    tbl = [[None] * n for _ in range(p)]
    for q, i in enumerate(tips):
        for t in range(p):
            tbl[t][list(taxa).index(pre[i].name)] = float(x[q, t])
    cg, ocgb, pcgb, fam, kw, spt = _device(P, tree, truth, tbl, taxa)
    nodes = family_nodes(ocgb, fam)
    families = np.array(_tips(fam), np.int32)
    scale = np.array([sc[pre[nodes[int(f)]].name] for f in families])
    extra = list(np.asarray(kw["R"], float).reshape(-1, p, p)[1:])

    def at(R, mu, S):
        pcgb.set_tip_noise_lg(families, S, scale)
        pcgb.assignfactors_lg_(np.stack([R] + extra), mu)
        ll, g = pcgb.loglik_and_gradient_lg(spt)
        return ll, np.concatenate([g["dR"][0].ravel(), g["dmu"], g["dsigma_e"].ravel()])
    R0, mu0, S0 = np.eye(p), np.zeros(p), 0.5 * np.eye(p)
    ll0, g0 = at(R0, mu0, S0)
    ll_true, _ = at(R_true, mu_true, S_true)
    pcgb.set_tip_noise_lg(families, S0, scale)
    R, mu, ll, opt = P.calibrate_optimize_cliquetree_(pcgb, spt, R0, mu0, extra_rates=extra, gradient=gradient, sigma_e0=S0)
    ll1, g1 = at(R, mu, opt.sigma_e)
    ratio = float(np.max(np.abs(g1)) / np.max(np.abs(g0)))
    print(f"joint fit ({gradient}): loglik {ll0:.4f} -> {ll:.6f} (at the generating values {ll_true:.6f}), score at the estimate "
          f"/ at the start {ratio:.2e}, {opt.n_device_evals} device evaluations\n  R {R.ravel()} (true {R_true.ravel()})\n"
          f"  Sigma_e {opt.sigma_e.ravel()} (true {S_true.ravel()})")
    assert abs(ll1 - ll) <= TOL * abs(ll) and ratio <= 1e-6 and ll >= ll_true
    assert pcgb.tip_noise_count_lg() == len(families)


# ----------------------------------------------------------------------------- 5: invariants

def _state_case(P):
    net, model, tbl, taxa = LR.missing_case()
    return (net, model, tbl, taxa) + _device(P, net, model, tbl, taxa)


def _all_sweeps(pcgb, spt):
    ll, g = pcgb.loglik_and_gradient_lg(spt)
    d = dict(ll=np.array(ll), **{k: np.asarray(v) for k, v in g.items() if k != "dsigma_e"})
    d.update({"e_" + k: np.asarray(v) for k, v in pcgb.edge_gradient_lg().items()})
    d.update({"s_" + k: np.asarray(v) for k, v in pcgb.shift_scan_lg().items()})
    d.update({"l_" + k: np.asarray(v) for k, v in pcgb.loo_lg().items()})
    d.update({"i_" + k: np.asarray(v) for k, v in pcgb.impute_lg().items()})
    return d


def test_set_clear_replace_and_survival(P):
    net, model, tbl, taxa, cg, ocgb, pcgb, fam, kw, spt = _state_case(P)
    _, _, never, _, _, spt0 = _device(P, net, model, tbl, taxa)
    base = _bytes(never)
    base_sweeps = _all_sweeps(never, spt0)
    families, scale, sigma_e, se2, E = _set(pcgb, fam, kw)
    pcgb.assignfactors_lg_(**kw)
    noisy = _bytes(pcgb)
    assert noisy != base
    # the same bytes on every call, fill and sweeps
    one = _all_sweeps(pcgb, spt)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == noisy
    two = _all_sweeps(pcgb, spt)
    for k in one:
        assert one[k].tobytes() == two[k].tobytes(), k
    assert one["ll"].tobytes() != base_sweeps["ll"].tobytes()
    # setting twice replaces, it does not add
    pcgb.set_tip_noise_lg(families[:2], 3.0 * sigma_e, scale[:2])
    assert pcgb.tip_noise_count_lg() == 2
    pcgb.set_tip_noise_lg(families, sigma_e, scale, se2)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == noisy and pcgb.tip_noise_count_lg() == len(families)
    # set_edges_lg and set_shifts_lg keep the noise
    pcgb.set_edges_lg(length=fam["length"], gamma=fam["gamma"])
    pcgb.set_shifts_lg([(int(families[0]), 0)], np.ones((1, 3)))
    pcgb.clear_shifts_lg()
    assert pcgb.tip_noise_count_lg() == len(families)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == noisy
    # clear: the fill and every sweep bit for bit as on an engine that never had noise
    pcgb.clear_tip_noise_lg()
    assert pcgb.tip_noise_count_lg() == 0
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == base
    cleared = _all_sweeps(pcgb, spt)
    assert cleared.keys() == base_sweeps.keys() and len(cleared["i_families"]) > 0
    for k in cleared:
        assert cleared[k].tobytes() == base_sweeps[k].tobytes(), k
    assert "dsigma_e" not in pcgb.gradient_lg()
    # a new lg_setup clears it
    pcgb.set_tip_noise_lg(families, sigma_e, scale, se2)
    data = lg_inputs_from_oracle(P, net, ocgb, model, tbl, taxa)[1]
    pcgb.lg_setup(fam, data)
    assert pcgb.tip_noise_count_lg() == 0
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == base


def test_invalid_entries_leave_the_previous_noise(P):
    from pgbp_amd import _lib as L
    net, model, tbl, taxa, cg, ocgb, pcgb, fam, kw, spt = _state_case(P)
    families, scale, sigma_e, se2, E = _set(pcgb, fam, kw)
    pcgb.assignfactors_lg_(**kw)
    noisy = _bytes(pcgb)
    nf = len(fam["cluster"])
    tip = int(families[0])
    inner = int(np.flatnonzero(np.asarray(fam["child_pos"]) >= 0)[0])
    S = np.eye(3)
    asym = S.copy(); asym[0, 1] = 0.3
    negd = S.copy(); negd[2, 2] = -1.0
    nanS = S.copy(); nanS[1, 1] = np.nan
    bad = [("out of range", [nf], S, [1.0], None), ("out of range", [-1], S, [1.0], None),
           ("not a tip family", [inner], S, [1.0], None), ("listed twice", [tip, tip], S, [1.0, 1.0], None),
           ("scale is not finite", [tip], S, [np.inf], None), ("scale is negative", [tip], S, [-0.5], None),
           ("not symmetric", [tip], asym, [1.0], None), ("is negative", [tip], negd, [1.0], None),
           ("not finite", [tip], nanS, [1.0], None), ("se2 of trait 1 is negative", [tip], S, [1.0], [[0.1, -0.1, 0.1]]),
           ("se2 of trait 2 is not finite", [tip], S, [1.0], [[0.1, 0.1, np.nan]])]
    for text, f, sg, sc, s2 in bad:
        with pytest.raises(L.PgbpError) as ex:
            pcgb.set_tip_noise_lg(np.array(f), sg, np.array(sc), None if s2 is None else np.array(s2))
        assert ex.value.code == L.ERR_INVALID and text in ex.value.msg, (text, ex.value.msg)
        assert ("entry" in ex.value.msg) or ("sigma_e" in ex.value.msg), ex.value.msg
        assert pcgb.tip_noise_count_lg() == len(families)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == noisy
    # no family table: PGBP_ERR_STATE, and the count says so
    bare = P.ClusterGraphBelief(product_beliefs_from_oracle(ocgb.belief), ocgb.node2cluster, ocgb.node2family, ocgb.node2fixed,
                                ocgb.cluster2nodes)
    f = np.zeros(1, np.int32)
    assert bare._lib.pgbp_lg_set_tip_noise(bare._eng, 1, L.i32p(f), L.f64p(np.ones(1)), L.f64p(np.eye(3)), None, 0) == L.ERR_STATE
    assert bare._lib.pgbp_lg_tip_noise_count(bare._eng) == -1


def test_every_split_of_the_site_range_gives_the_same_bytes(P):
    """p = 2, 8 sites with per-site noise: pgbp_lg_gradient_noise, the edge sweep, loo and the scan over [0, 8) and over
    every split [0, a) + [a, 8) return the same bytes."""
    from pgbp_amd import _lib as L
    n_sites, p = 8, 2
    cgb, spt, fam, Rs, site = _batch(P, p, n_sites)
    families, scale, sig, se2 = _batch_noise(fam, Rs, n_sites, p, 11)
    cgb.set_tip_noise_lg(families, sig, scale, se2)
    cgb.assignfactors_lg_(Rs[:, None], site.mus)
    ll, whole = cgb.loglik_and_gradient_lg(spt, all_sites=True)
    assert not whole["info"].any()
    onet, model, tbl, taxa = site(5)
    E = NR.tip_noise(scale, sig[5], se2[5])
    pre = onet.vec_node
    w = NR.NoisyTipModel(model, {onet.parent_edges(pre[int(f) + 1])[0].number: e for f, e in zip(families, E)})
    st = NR.dense_statement(onet, w, model, {}, {int(f) + 1: e for f, e in zip(families, E)},
                            {int(f) + 1: s for f, s in zip(families, scale)}, tbl, taxa)
    err = max(rel_block(whole["dsigma_e"][5], st["dsigma_e"]), rel_block(whole["dR"][5][0], st["dR"][0]),
              abs(ll[5] - OD.loglik(onet, w, tbl, taxa)) / abs(ll[5]))
    print(f"batch of 8, per-site noise, site 5: loglik, dR and dsigma_e vs dense {err:.2e}")
    assert err <= TOL
    nr = cgb._lg_nrates

    def grad(a, b):
        n = b - a
        out = [np.zeros((n, nr, p, p)), np.zeros((n, p)), np.zeros(n), np.zeros((n, p)), np.zeros((n, p, p))]
        info = np.zeros(n, np.int32)
        assert cgb._lib.pgbp_lg_gradient_noise(cgb._eng, a, b, *[L.f64p(x) for x in out], L.i32p(info)) == 0
        return out
    full = grad(0, n_sites)
    for a in range(1, n_sites):
        lo, hi = grad(0, a), grad(a, n_sites)
        for x, y, z in zip(full, lo, hi):
            assert x.tobytes() == np.concatenate([y, z]).tobytes(), a
    eg, loo, scn = cgb.edge_gradient_lg(all_sites=True), cgb.loo_lg(all_sites=True), cgb.shift_scan_lg(all_sites=True)
    for s in range(n_sites):
        cgb.site = s
        e1, l1, s1 = cgb.edge_gradient_lg(), cgb.loo_lg(), cgb.shift_scan_lg()
        for k in ("dlength", "dgamma", "dshift"):
            assert eg[k][s].tobytes() == e1[k].tobytes(), (k, s)
        for k in ("mean", "cov", "lpd"):
            assert loo[k][s].tobytes() == l1[k].tobytes(), (k, s)
        for k in ("jump", "lr"):
            assert scn[k][s].tobytes() == s1[k].tobytes(), (k, s)
    cgb.site = 0


def test_group_and_patterns_handles_take_the_call_per_engine(P):
    """An engine borrowed from a pgbp_group (the device listed twice, 4 + 4 sites) and from a pgbp_patterns handle takes
    set_tip_noise_lg like any other: the handle's loglik against the dense wrapper, site by site."""
    from pgbp_amd.sharding import EngineGroup, PatternGroup
    n_sites, p = 8, 1
    nwk, taxa, data, Rs, mus = LR.batch_case(p, n_sites=n_sites)
    cgb, spt, fam, _, site = _batch(P, p, n_sites)
    families, scale, sig, se2 = _batch_noise(fam, Rs, n_sites, p, 13)
    want = []
    for s in range(n_sites):
        onet, model, tbl, tx = site(s)
        pre = onet.vec_node
        E = NR.tip_noise(scale, sig[s], se2[s])
        want.append(OD.loglik(onet, NR.NoisyTipModel(model, {onet.parent_edges(pre[int(f) + 1])[0].number: e
                                                             for f, e in zip(families, E)}), tbl, tx))
    want = np.array(want)
    arrays = (cgb._dims.copy(), cgb._sepcl.reshape(-1).copy(), cgb._scope_off.copy(), cgb._scope_idx.copy())
    grp = EngineGroup(*arrays, n_sites, [0, 0])
    grp.set_schedule([spt])
    keep = []
    for k in range(grp.size):
        a, n = grp.range(k)
        b = P.ClusterGraphBelief.from_arrays(*arrays, None, n_sites=n, engine=grp.engine(k))
        b.lg_setup(fam, data[a:a + n])
        b.assignfactors_lg_(Rs[a:a + n, None], mus[a:a + n])
        b.set_tip_noise_lg(families, sig[a:a + n], scale, se2[a:a + n])
        assert b.tip_noise_count_lg() == len(families)
        keep.append(b)
    grp.enqueue_loglik(lg=True)
    ll, info = grp.fetch_loglik()
    e1 = float(np.max(np.abs(ll - want) / np.maximum(1.0, np.abs(want))))
    for b in keep:
        b._eng = None
    grp.close()
    half = n_sites // 2
    pats = PatternGroup([arrays + (list(range(0, n_sites, 2)),), arrays + (list(range(1, n_sites, 2)),)])
    pats.set_schedule([spt])
    for k in range(2):
        idx = list(range(k, n_sites, 2))
        b = pats.beliefs[k]
        b.lg_setup(fam, data[idx])
        b.assignfactors_lg_(Rs[idx][:, None], mus[idx])
        b.set_tip_noise_lg(families, sig[idx], scale, se2[idx])
    ll2, info2 = pats.loglik_lg()
    e2 = float(np.max(np.abs(ll2 - want) / np.maximum(1.0, np.abs(want))))
    pats.close()
    print(f"group handle {e1:.2e}, patterns handle {e2:.2e} (8 sites, per-site noise, {half} + {half})")
    assert not info.any() and not info2.any() and max(e1, e2) <= TOL

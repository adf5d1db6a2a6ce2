"""Mean shifts on edges on the device: pgbp_lg_set_shifts / set_shifts_lg, the correction of the factor fill
(csrc/pgbp_shift.hip), the four sweeps under shifts and the driver fit_shifts_lg.

Comparator: shift_ref.ShiftedModel around the untouched oracle -- densely (densemvn: loglik, posterior_node_moments, and
through it loo_ref.dense_loo, impute_ref.dense_impute) and as belief propagation (oracle.beliefs.assignfactors) --, both
pinned to each other and to finite differences in test_shift_cpu.py.  Every comparison at 1e-8 relative to the largest
entry of the block; the measured figure of every case is printed."""
import numpy as np
import pytest

import impute_ref as IR
import loo_ref as LR
from edge_ref import rel_block_nan
from helpers import lg_inputs_from_oracle, oracle_setup, product_beliefs_from_oracle
from oracle import beliefs as OB
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from shift_ref import (ShiftedModel, dense_statement, device_layout, family_edge, family_nodes, family_of_edge, fit_edges,
                       gls_fit)
from test_gradient_cpu import _case, _more_cases, rel_block
from test_shift_cpu import moved_data

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


# ----------------------------------------------------------------------------- set-up

def _graph(net, graph):
    if graph == "cliquetree":
        return OCG.cliquetree(net)
    if graph == "bethe":
        return OCG.bethe(net)
    return OCG.joingraph(net, 3)


def _device(P, net, model, tbl, taxa, graph="cliquetree", assign=True, oracle_factors=True):
    """One-site engine on a cluster graph of an oracle network: (cg, plain oracle beliefs, device beliefs, family table,
    keyword arguments of assignfactors_lg_, schedule tree of a clique tree).  oracle_factors=False: the oracle allocates the
    scopes only (allocatebeliefs), its assignfactors is not run and the oracle beliefs returned hold no factor -- for inputs
    on which the oracle's own factor code raises, compared densely."""
    cg = _graph(net, graph)
    if oracle_factors:
        ocgb = oracle_setup(net, cg, model, tbl, taxa)
    else:
        b, (n2c, n2f, n2fix, _, c2n) = OB.allocatebeliefs(tbl, taxa, net, cg, model)
        ocgb = OB.ClusterGraphBelief(b, n2c, n2f, n2fix, c2n)
    pb = product_beliefs_from_oracle(ocgb.belief)
    for b in pb:
        b.J[...] = 0.0
        b.h[...] = 0.0
        b.g[...] = 0.0
    pcgb = P.ClusterGraphBelief(pb, ocgb.node2cluster, ocgb.node2family, ocgb.node2fixed, ocgb.cluster2nodes)
    fam, data, kw = lg_inputs_from_oracle(P, net, ocgb, model, tbl, taxa)
    pcgb.lg_setup(fam, data)
    if assign:
        pcgb.assignfactors_lg_(**kw)
    spt = OCG.spanningtree_clusterlist(cg, OCG.default_rootcluster(cg, net)) if graph == "cliquetree" else None
    return cg, ocgb, pcgb, fam, kw, spt


def _pick(fam, both_hybrid=False):
    """The shifted set of the fill tests as {kind: [(f, k), ...]}: a tip edge, an edge whose parent is the fixed root, one edge
    (or both) of a hybrid family, two families of one cluster, a family with a partial child_mask."""
    K = max(1, int(fam["max_parents"]))
    nf = len(fam["cluster"])
    npar, cpos, ppos = fam["n_parents"], fam["child_pos"], fam["parent_pos"].reshape(nf, K)
    kinds = {}
    tips = [f for f in range(nf) if cpos[f] < 0 and npar[f] == 1]
    if tips:
        kinds["tip"] = [(tips[0], 0)]
    froot = [(f, k) for f in range(nf) for k in range(npar[f]) if ppos[f, k] < 0]
    if froot:
        kinds["fixed_root_parent"] = [froot[-1]]
    hyb = [f for f in range(nf) if npar[f] >= 2]
    if hyb:
        kinds["hybrid"] = [(hyb[0], k) for k in range(npar[hyb[0]] if both_hybrid else 1)]
    for c in np.unique(fam["cluster"]):
        fs = [f for f in range(nf) if fam["cluster"][f] == c and npar[f] >= 1]
        if len(fs) >= 2:
            kinds["same_cluster"] = [(fs[0], 0), (fs[1], 0)]
            break
    cm = fam.get("child_mask")
    if cm is not None:
        full = (1 << int(fam["p"])) - 1
        part = [f for f in range(nf) if npar[f] >= 1 and int(cm[f]) not in (0, full)]
        if part:
            kinds["partial_mask"] = [(part[0], 0)]
    return kinds


def _edges_values(kinds, p, seed=5):
    edges = sorted({e for v in kinds.values() for e in v})
    rng = np.random.default_rng(seed)
    return edges, rng.uniform(0.5, 1.5, size=(len(edges), p)) * rng.choice([-1.0, 1.0], size=(len(edges), p))


def _wrapper(net, ocgb, fam, model, edges, values):
    """The shifted oracle model of a device case.  Its BP factors (the wrapped model's own factor plus the shift's terms:
    shift_ref.ShiftedModel) are checked here, on every family of the case, against the GENERIC factors that
    oracle.models.EvolutionaryModel derives from branch_qwv alone, at 1e-12: the comparator of the fill is then as independent
    of the kernel's formula as the generic code is."""
    w = ShiftedModel(model, {family_edge(net, ocgb, fam, f, k).number: v for (f, k), v in zip(edges, values)})
    for n in net.vec_node[1:]:
        pae = net.parent_edges(n)
        mine = w.factor_treeedge(pae[0]) if len(pae) == 1 else w.factor_hybridnode(pae)
        for a, b in zip(mine, w.generic_factor(pae)):
            a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
            assert float(np.max(np.abs(a - b))) <= 1e-12 * max(1.0, float(np.max(np.abs(b)))), (n.name, a, b)
    return w


def _records_error(pcgb, ocgb_w):
    """Largest error of (J, h, g) over the clusters, each block relative to its largest entry (g: to max(|g|, 1))."""
    pcgb.pull()
    worst = 0.0
    for c in range(ocgb_w.nclusters):
        J, h, g = pcgb._views(0, c)
        b = ocgb_w.belief[c]
        if b.J.size:
            worst = max(worst, rel_block(J, b.J) if np.any(b.J) else float(np.max(np.abs(J))))
            worst = max(worst, float(np.max(np.abs(h - b.h))) / max(float(np.max(np.abs(b.h))), 1e-300) if np.any(b.h)
                        else float(np.max(np.abs(h))))
        worst = max(worst, abs(float(g[0]) - float(b.g[0])) / max(abs(float(b.g[0])), 1.0))
    return worst


# ----------------------------------------------------------------------------- 1: the fill, record by record

@pytest.mark.parametrize("graph", ["cliquetree", "bethe", "joingraph"])
@pytest.mark.parametrize("root", ["fixed", "random", "improper"])
@pytest.mark.parametrize("name", ["level1_1trait", "level1_2traits", "mateescu", "optimization_level1", "sun2023"])
def test_fill_reference_networks(P, name, root, graph):
    """set_shifts_lg + assignfactors_lg_ against the oracle's assignfactors of the wrapper, every cluster's (J, h, g), on the
    clique tree, the Bethe graph and a join graph of the reference's networks; full BM with each kind of root.  The `random`
    cases shift both edges of a hybrid family, the others one."""
    net, model, tbl, taxa = LR.reference_case(name, root)
    cg, ocgb, pcgb, fam, kw, _ = _device(P, net, model, tbl, taxa, graph, assign=False)
    kinds = _pick(fam, both_hybrid=(root == "random"))
    assert "tip" in kinds and "hybrid" in kinds
    assert len(kinds["hybrid"]) == (2 if root == "random" else 1)
    assert ("fixed_root_parent" in kinds) == (root == "fixed")
    if graph == "cliquetree":
        assert "same_cluster" in kinds
    edges, values = _edges_values(kinds, model.dimension())
    pcgb.set_shifts_lg(edges, values)
    assert pcgb.shift_count_lg() == len(edges)
    pcgb.assignfactors_lg_(**kw)
    ocgb_w = oracle_setup(net, cg, _wrapper(net, ocgb, fam, model, edges, values), tbl, taxa)
    err = _records_error(pcgb, ocgb_w)
    plain = _records_error(pcgb, ocgb)
    print(f"{name}/{root}/{graph}: {len(edges)} shifted edges, records vs the oracle's {err:.2e} (vs the unshifted {plain:.2e})")
    assert err <= TOL and plain > 1e-3


MODELS = [("hetero_random", 2), ("ou_fixed", 1), ("ou_random", 1), ("bm_improper", 2)]


def _model_case(which, p):
    return LR.missing_case() if which == "missing" else LR.random_case(which, p)


@pytest.mark.parametrize("which,p", MODELS + [("missing", 3)])
def test_fill_models_and_missing_data(P, which, p):
    """Heterogeneous BM with three colours, the OU at p = 1 (fixed and random root), an improper root, and the missing-data
    case (p = 3): there one shifted family keeps fewer than p components, and its shift is not zero outside them."""
    net, model, tbl, taxa = _model_case(which, p)
    cg, ocgb, pcgb, fam, kw, _ = _device(P, net, model, tbl, taxa, assign=False)
    kinds = _pick(fam, both_hybrid=True)
    assert "tip" in kinds and len(kinds["hybrid"]) == 2 and "same_cluster" in kinds
    edges, values = _edges_values(kinds, p)
    if which == "missing":
        f = kinds["partial_mask"][0][0]
        O = int(fam["child_mask"][f])
        outside = [t for t in range(p) if not (O >> t) & 1]
        assert outside and np.all(values[edges.index((f, 0))][outside] != 0.0)
    pcgb.set_shifts_lg(edges, values)
    pcgb.assignfactors_lg_(**kw)
    ocgb_w = oracle_setup(net, cg, _wrapper(net, ocgb, fam, model, edges, values), tbl, taxa)
    err = _records_error(pcgb, ocgb_w)
    print(f"{which}/p{p}: {len(edges)} shifted edges, records vs the oracle's {err:.2e}")
    assert err <= TOL


# ----------------------------------------------------------------------------- 2: the likelihood

@pytest.mark.parametrize("which,p", MODELS + [("missing", 3), ("bm_fixed", 1), ("bm_random", 4)])
def test_loglik_under_shifts(P, which, p):
    """loglik_lg against densemvn.loglik of the wrapper; against a fresh engine without shifts on the transformed data (two
    device results); reps = 3 returns the bytes of reps = 1."""
    net, model, tbl, taxa = _model_case(which, p)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    pcgb._ensure_schedule([spt])
    edges, values = _edges_values(_pick(fam, both_hybrid=True), p)
    pcgb.set_shifts_lg(edges, values)
    ll, info = pcgb.loglik_lg()
    wrapper = _wrapper(net, ocgb, fam, model, edges, values)
    dense = OD.loglik(net, wrapper, tbl, taxa)
    ll3, _ = pcgb.loglik_lg(reps=3)
    moved, _ = moved_data(net, model, wrapper.shifts, tbl, taxa)
    _, _, fresh, _, _, spt2 = _device(P, net, model, moved, taxa)
    fresh._ensure_schedule([spt2])
    ll0, _ = fresh.loglik_lg()
    e1, e2 = abs(ll[0] - dense) / max(1.0, abs(dense)), abs(ll[0] - ll0[0]) / max(1.0, abs(dense))
    print(f"{which}/p{p}: loglik vs dense {e1:.2e}, vs the engine on transformed data {e2:.2e}")
    assert info[0] == 0 and e1 <= TOL and e2 <= TOL
    assert ll3.tobytes() == ll.tobytes()
    assert abs(dense - OD.loglik(net, model, tbl, taxa)) > 1e-3


# ----------------------------------------------------------------------------- 3: the layouts

def _tree_batch(P, p, n_sites=64, masked=False):
    """loo_ref.batch_case: a 40-tip tree, fixed root, 64 sites with their own data and parameters.  masked: under
    impute_ref.batch_pattern (some tip values missing, every internal node keeps its full scope)."""
    nwk, taxa, data, Rs, mus = LR.batch_case(p, n_sites=n_sites)
    if masked:
        data = data.copy()
        data[:, IR.batch_pattern(p)] = np.nan
    net, names = P.read_newick(nwk)
    row = {t: r for r, t in enumerate(taxa)}
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=True)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], p, data=data[0] if masked else None)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=n_sites)
    cgb.lg_setup(fam, data)
    cgb.assignfactors_lg_(Rs[:, None], mus)
    return cgb, spt, fam


def _batch_dense(p, s, fam_nodes, edges, values_s, what=OD.loglik):
    """Site s of the batch under its shifts, densely.  A family of the table is node f + 1 (fixed root: no root family)."""
    onet, model, tbl, taxa = LR.batch_site(p, s)
    pre = onet.vec_node
    sh = {onet.parent_edges(pre[fam_nodes[f]])[0].number: v for (f, _), v in zip(edges, values_s)}
    return what(onet, ShiftedModel(model, sh), tbl, taxa)


def test_site_minor_tree_per_site_values(P):
    """p = 1, 64 sites (the smallest batch that takes the site-minor layout), the clique tree of a tree -- one family per
    cluster, the `simple` table of the thread-per-site fill -- with one set of shifts per site: every site against the dense
    wrapper.  Shared values on the same engine as well."""
    cgb, spt, fam = _tree_batch(P, 1)
    cgb._ensure_schedule([spt])
    nf = len(fam["cluster"])
    nodes = list(range(1, nf + 1))
    tips = [f for f in range(nf) if fam["child_pos"][f] < 0]
    inner = [f for f in range(nf) if fam["child_pos"][f] >= 0]
    edges = [(tips[0], 0), (inner[0], 0), (inner[len(inner) // 2], 0), (int(np.flatnonzero(fam["parent_pos"] < 0)[0]), 0)]
    edges = sorted(set(edges))
    values = np.random.default_rng(9).normal(size=(64, len(edges), 1))
    cgb.set_shifts_lg(edges, values)
    ll, info = cgb.loglik_lg()
    assert cgb._lib.pgbp_layout(cgb._eng) & 2, "a univariate batch of 64 sites is expected in the site-minor layout"
    worst = 0.0
    for s in range(64):
        dense = _batch_dense(1, s, nodes, edges, values[s])
        worst = max(worst, abs(ll[s] - dense) / max(1.0, abs(dense)))
    print(f"site-minor tree, per-site shifts: loglik vs dense, worst of 64 sites {worst:.2e}")
    assert not info.any() and worst <= TOL
    cgb.set_shifts_lg(edges, values[3])
    ll, _ = cgb.loglik_lg()
    worst = max(abs(ll[s] - _batch_dense(1, s, nodes, edges, values[3])) for s in (0, 3, 63))
    print(f"site-minor tree, shared shifts: {worst:.2e}")
    assert worst <= TOL * max(1.0, float(np.max(np.abs(ll))))


def test_site_minor_general_table(P):
    """p = 1, 64 sites, the Bethe graph of the same tree: the variable clusters hold no family, so the fill walks the general
    family table; site-minor layout, per-site shifts.  The record of every family's cluster of three sites against the oracle's
    assignfactors of the wrapper on its own Bethe graph (clusters matched through the family they hold)."""
    nwk, taxa, data, Rs, mus = LR.batch_case(1)
    net, names = P.read_newick(nwk)
    row = {t: r for r, t in enumerate(taxa)}
    cn, ed, sn = P.bethe(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, 1, fixedroot=True)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], 1)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=64)
    cgb.lg_setup(fam, data)
    nf = len(fam["cluster"])
    assert nf < len(cn), "variable clusters hold no family: the general table"
    edges = sorted({(0, 0), (nf // 2, 0), (nf - 1, 0)})
    values = np.random.default_rng(10).normal(size=(64, len(edges), 1))
    cgb.set_shifts_lg(edges, values)
    cgb.assignfactors_lg_(Rs[:, None], mus)
    assert cgb._lib.pgbp_layout(cgb._eng) & 2
    cgb.pull()
    got = cgb._packed_raw.copy()
    sites = [0, 17, 63]
    worst = 0.0
    for s in sites:
        onet, model, tbl, tx = LR.batch_site(1, s)
        ocg = OCG.bethe(onet)
        sh = {onet.parent_edges(onet.vec_node[f + 1])[0].number: v for (f, _), v in zip(edges, values[s])}
        ow = oracle_setup(onet, ocg, ShiftedModel(model, sh), tbl, tx)
        # match clusters by their family: cluster of family f on both sides
        o_fam = lg_inputs_from_oracle(P, onet, oracle_setup(onet, ocg, model, tbl, tx), model, tbl, tx)[0]
        for f in range(nf):
            c_dev, c_or = int(fam["cluster"][f]), int(o_fam["cluster"][f])
            m = int(cgb._dims[c_dev])
            rec = got[s, cgb._poff[c_dev]: cgb._poff[c_dev + 1]]
            b = ow.belief[c_or]
            assert b.J.shape == (m, m)
            want = np.concatenate([b.J.reshape(-1, order="F"), b.h, [b.g[0]]])
            worst = max(worst, float(np.max(np.abs(rec[: len(want)] - want))) / max(1.0, float(np.max(np.abs(want)))))
    print(f"site-minor general table, per-site shifts: records of 3 sites vs the oracle's {worst:.2e}")
    assert worst <= TOL


def _tree_case(P, p, seed):
    """A complete-data 12-tip tree with a proper random root and three shifted edges: (tree, model, tbl, device beliefs,
    schedule tree, assignfactors_lg_ keywords, edges, values, {oracle edge number: value}).  p = 16: loo_ref.wavefront_case on
    the oracle's clique tree, as test_gpu_loo.py sets it up (packed after a calibration); else the product's own host side
    (impute_ref.full_scope_setup: clusters of p or 2p variables)."""
    rng = np.random.default_rng(seed)
    if p == 16:
        tree, model, tbl, taxa = LR.wavefront_case()
        cg, ocgb, pcgb, fam, kw, spt = _device(P, tree, model, tbl, taxa)
        real = [f for f in range(len(fam["cluster"])) if fam["n_parents"][f] == 1]
        edges = sorted({(real[0], 0), (real[len(real) // 2], 0), (real[-1], 0)})
        values = rng.normal(size=(len(edges), p))
        sh = {family_edge(tree, ocgb, fam, f, k).number: v for (f, k), v in zip(edges, values)}
        return tree, model, tbl, pcgb, spt, kw, edges, values, sh
    tree = ON.random_network(12, 0, rng)
    tbl = [list(rng.normal(size=12)) for _ in range(p)]
    model = LR.bm(p, rng, "random")
    su = IR.full_scope_setup(tree, model, tbl, tree.tip_names)
    pcgb = P.ClusterGraphBelief.from_arrays(*su["arrays"])
    pcgb.lg_setup(su["fam"], su["data"])
    pcgb.assignfactors_lg_(**su["kw"])
    fam = su["fam"]
    real = [f for f in range(len(fam["cluster"])) if fam["n_parents"][f] == 1]
    edges = sorted({(real[0], 0), (real[len(real) // 2], 0), (real[-1], 0)})
    values = rng.normal(size=(len(edges), p))
    # family f of the product's table is node f of its preorder (the root's prior family is node 0); by name to the oracle
    byname = {n.name: n for n in tree.vec_node}
    sh = {tree.parent_edges(byname[su["names"][f]])[0].number: v for (f, _), v in zip(edges, values)}
    return tree, model, tbl, pcgb, su["spt"], su["kw"], edges, values, sh


@pytest.mark.parametrize("p,layout", [(2, 1), (16, 1), (3, 0), (40, 0)])
def test_layouts_plain_packed_and_large_p(P, p, layout):
    """A 12-tip tree: p = 2 and p = 16 are held in the packed BS16 layout after a calibration, and the fill -- with its
    correction -- then writes packed records (the layout is asserted before and after); p = 3 stays plain; p = 40 needs
    more than 64 KB of LDS in the fill.  loglik_lg and a second assignfactors_lg_ + calibration against the dense wrapper."""
    tree, model, tbl, pcgb, spt, kw, edges, values, sh = _tree_case(P, p, 40 + p)
    pcgb._ensure_schedule([spt])
    ll0, _ = pcgb.loglik_and_edge_gradient_lg(spt)   # (a calibration: the engine takes the layout its kernels want)
    assert pcgb._lib.pgbp_layout(pcgb._eng) == layout, (p, pcgb._lib.pgbp_layout(pcgb._eng))
    pcgb.set_shifts_lg(edges, values)
    ll, info = pcgb.loglik_lg()
    assert pcgb._lib.pgbp_layout(pcgb._eng) == layout
    dense = OD.loglik(tree, ShiftedModel(model, sh), tbl, tree.tip_names)
    pcgb.assignfactors_lg_(**kw)            # beliefs and factors, in the layout the engine is in
    assert pcgb._lib.pgbp_layout(pcgb._eng) == layout
    ll2, g = pcgb.loglik_and_shift_gradient_lg(spt)
    e1, e2 = abs(ll[0] - dense) / abs(dense), abs(ll2 - dense) / abs(dense)
    print(f"12-tip tree p={p} layout {layout}: loglik_lg vs dense {e1:.2e}, after assignfactors + calibrate {e2:.2e}")
    assert info[0] == 0 and e1 <= TOL and e2 <= TOL
    assert abs(ll[0] - ll0) > 1e-3 and g.shape == (len(edges), p)


# ----------------------------------------------------------------------------- 4: state

def _state_case(P):
    net, model, tbl, taxa = LR.random_case("hetero_random", 2)
    return (net, model, tbl, taxa) + _device(P, net, model, tbl, taxa)


def _bytes(pcgb):
    pcgb.pull()
    return pcgb._packed_raw.tobytes()


def test_set_clear_replace_and_survival(P):
    net, model, tbl, taxa, cg, ocgb, pcgb, fam, kw, spt = _state_case(P)
    _, _, never, _, _, _ = _device(P, net, model, tbl, taxa)
    base = _bytes(never)
    edges, values = _edges_values(_pick(fam, both_hybrid=True), 2)
    pcgb.set_shifts_lg(edges, values)
    pcgb.assignfactors_lg_(**kw)
    shifted = _bytes(pcgb)
    assert shifted != base
    # clear: byte-identical to an engine that never had shifts
    pcgb.clear_shifts_lg()
    assert pcgb.shift_count_lg() == 0
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == base
    # setting twice replaces, it does not add
    pcgb.set_shifts_lg(edges[:2], values[:2] * 3.0)
    pcgb.set_shifts_lg(edges, values)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == shifted and pcgb.shift_count_lg() == len(edges)
    # the same bytes on every call
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == shifted
    # set_edges_lg keeps the shifts
    pcgb.set_edges_lg(length=fam["length"], gamma=fam["gamma"])
    assert pcgb.shift_count_lg() == len(edges)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == shifted
    # a new lg_setup clears them
    data = lg_inputs_from_oracle(P, net, ocgb, model, tbl, taxa)[1]
    pcgb.lg_setup(fam, data)
    assert pcgb.shift_count_lg() == 0
    assert pcgb._lg_shift_edges.size == 0      # (the host's copy of the edge list goes with them)
    with pytest.raises(P.PgbpError, match="assignfactors_lg_"):   # ... and the new table has no parameters yet
        pcgb.loglik_and_shift_gradient_lg(spt)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == base


def test_invalid_entries_leave_the_previous_shifts(P):
    from pgbp_amd import _lib as L
    net, model, tbl, taxa, cg, ocgb, pcgb, fam, kw, spt = _state_case(P)
    K = int(fam["max_parents"])
    nf = len(fam["cluster"])
    npar = fam["n_parents"]
    edges, values = _edges_values(_pick(fam), 2)
    pcgb.set_shifts_lg(edges, values)
    pcgb.assignfactors_lg_(**kw)
    shifted = _bytes(pcgb)
    tree_f = int(np.flatnonzero(npar == 1)[0])
    root_f = int(np.flatnonzero(npar == 0)[0])
    good = np.ones((1, 2))
    bad = [("out of range", [nf * K], good), ("out of range", [-1], good), ("no edge 1", [tree_f * K + 1], good),
           ("root prior", [root_f * K], good), ("listed twice", [tree_f * K, tree_f * K], np.ones((2, 2))),
           ("not finite", [tree_f * K], np.array([[1.0, np.nan]])), ("not finite", [tree_f * K], np.array([[np.inf, 0.0]]))]
    for text, e, v in bad:
        with pytest.raises(L.PgbpError) as ex:
            pcgb.set_shifts_lg(np.array(e), v)
        assert ex.value.code == L.ERR_INVALID and text in ex.value.msg and "entry" in ex.value.msg, (text, ex.value.msg)
        assert pcgb.shift_count_lg() == len(edges)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == shifted
    # no family table: PGBP_ERR_STATE, and the count says so
    bare = P.ClusterGraphBelief(product_beliefs_from_oracle(ocgb.belief), ocgb.node2cluster, ocgb.node2family, ocgb.node2fixed,
                                ocgb.cluster2nodes)
    e = np.zeros(1, np.int32)
    assert bare._lib.pgbp_lg_set_shifts(bare._eng, 1, L.i32p(e), L.f64p(np.ones(2)), 0) == L.ERR_STATE
    assert bare._lib.pgbp_lg_shift_count(bare._eng) == -1


def test_sweeps_without_shifts_return_the_same_bytes(P):
    """With no shifts set -- never set on one engine, set and cleared on the other -- each of the four sweeps returns equal
    bytes (missing-data case: the imputation lists families)."""
    net, model, tbl, taxa = LR.missing_case()
    out = []
    for had in (False, True):
        cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
        if had:
            edges, values = _edges_values(_pick(fam), 3)
            pcgb.set_shifts_lg(edges, values)
            pcgb.assignfactors_lg_(**kw)
            pcgb.clear_shifts_lg()
            pcgb.assignfactors_lg_(**kw)
        ll, g = pcgb.loglik_and_gradient_lg(spt)
        d = dict(ll=np.array(ll), **{k: np.asarray(v) for k, v in g.items()})
        d.update({"e_" + k: np.asarray(v) for k, v in pcgb.edge_gradient_lg().items()})
        d.update({"l_" + k: np.asarray(v) for k, v in pcgb.loo_lg().items()})
        d.update({"i_" + k: np.asarray(v) for k, v in pcgb.impute_lg().items()})
        out.append(d)
    assert out[0].keys() == out[1].keys() and len(out[0]["i_families"]) > 0
    for k in out[0]:
        assert out[0][k].tobytes() == out[1][k].tobytes(), k


# ----------------------------------------------------------------------------- 5: the sweeps under shifts

@pytest.mark.parametrize("which,p", [("bm_random", 4), ("hetero_random", 2), ("ou_fixed", 1), ("ou_random", 1), ("missing", 3)])
def test_sweeps_under_shifts(P, which, p):
    """Calibrated clique tree under shifts: gradient_lg and edge_gradient_lg against shift_ref.family_statement on the dense
    posterior of the wrapper (pinned in test_shift_cpu.py), loo_lg against dense_loo(wrapper), impute_lg against
    dense_impute(wrapper) (the missing-data case), moments_ means against posterior_node_moments(wrapper)."""
    net, model, tbl, taxa = _model_case(which, p)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    edges, values = _edges_values(_pick(fam, both_hybrid=True), p)
    wrapper = _wrapper(net, ocgb, fam, model, edges, values)
    pcgb.set_shifts_lg(edges, values)
    ll, gs = pcgb.loglik_and_shift_gradient_lg(spt)
    dense = OD.loglik(net, wrapper, tbl, taxa)
    assert abs(ll - dense) <= TOL * max(1.0, abs(dense))
    st = dense_statement(net, model, wrapper.shifts, tbl, taxa)
    got = pcgb.gradient_lg()
    worst = {}
    for k in ("dR", "dmu", "dalpha", "dtheta"):
        w, g = np.atleast_1d(np.asarray(st[k], float)), np.atleast_1d(np.asarray(got[k], float))
        if np.any(w) or np.any(g):
            worst[k] = rel_block(g, w)
    eg = pcgb.edge_gradient_lg()
    want = device_layout(st, net, ocgb, fam)
    from edge_ref import rel_block_nan
    for k in ("dlength", "dgamma", "dshift"):
        worst[k] = rel_block_nan(eg[k], want[k])
    K = int(fam["max_parents"])
    want_gs = np.array([fam["gamma"][f * K + k] * want["dshift"][f] for f, k in edges])
    worst["shift_gradient"] = rel_block(gs, want_gs)
    assert np.array_equal(pcgb.shift_gradient_lg(), gs)
    loo = pcgb.loo_lg()
    worst["loo"] = LR.worst_error(fam["data_row"][loo["families"]], loo, LR.dense_loo(net, wrapper, tbl, taxa), p)
    if which == "missing":
        worst["impute"] = IR.worst_error(pcgb.impute_lg(), IR.dense_impute(net, wrapper, tbl, taxa))
    pm, _ = OD.posterior_node_moments(net, wrapper, tbl, taxa)
    mom = pcgb.moments_(cov=False)
    e = 0.0
    for c in range(ocgb.nclusters):
        b = ocgb.belief[c]
        insc = np.asarray(b.inscope, bool)
        idx = [(lab - 1) * p + t for j, lab in enumerate(b.nodelabel) for t in range(p) if insc[t, j]]
        if idx:
            e = max(e, float(np.max(np.abs(mom[c][0] - pm[idx]))) / max(float(np.max(np.abs(pm))), 1e-300))
    worst["moments"] = e
    print(f"{which}/p{p}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (k, v)
    # the new term of dgamma is in: a shifted hybrid edge's entry differs from the unshifted formula's by s_k' g_w
    f, k = next((f, k) for f, k in edges if fam["n_parents"][f] >= 2)
    assert abs(float(values[edges.index((f, k))] @ eg["dshift"][f])) > 1e-9


def test_sweeps_batch_per_site_shifts_in_chunks(P):
    """64 sites with their own data, parameters and shifts (p = 2, some tip values missing): the per-site indexing of the
    shifts in all four sweeps.  Sites 0, 31 and 63: gradient_lg, edge_gradient_lg (dlength, dgamma, dshift) and the shift
    gradient against shift_ref.family_statement on the dense posterior of that site's wrapper, loo_lg against dense_loo,
    impute_lg against dense_impute, the log-likelihood against densemvn.  loo_lg and impute_lg in one chunk of sites and in
    two (pgbp_loo_scratch_limit, pgbp_impute_scratch_limit) return equal bytes (the other two sweeps have no such knob).
    Then fit_shifts_lg(all_sites=True): every site's own fit, the same three sites against dense GLS."""
    p = 2
    cgb, spt, fam = _tree_batch(P, p, masked=True)
    nf = len(fam["cluster"])
    nodes = list(range(1, nf + 1))      # (fixed root: family f is node f + 1, one parent edge each)
    edges = sorted({(0, 0), (nf // 3, 0), (nf - 1, 0)})
    values = np.random.default_rng(13).normal(size=(64, len(edges), p))
    cgb.set_shifts_lg(edges, values)
    ll, gs = cgb.loglik_and_shift_gradient_lg(spt, all_sites=True)
    grad = cgb.gradient_lg(all_sites=True)
    eg = cgb.edge_gradient_lg(all_sites=True)
    one, imp = cgb.loo_lg(all_sites=True), cgb.impute_lg(all_sites=True)
    assert len(imp["families"]) > 0 and gs.shape == (64, len(edges), p)
    cgb._lib.pgbp_loo_scratch_limit(len(one["families"]) * (p + p * p + 1) * 32)
    cgb._lib.pgbp_impute_scratch_limit(len(imp["families"]) * (p + p * p) * 32)
    try:
        two, imp2 = cgb.loo_lg(all_sites=True), cgb.impute_lg(all_sites=True)
    finally:
        cgb._lib.pgbp_loo_scratch_limit(0)
        cgb._lib.pgbp_impute_scratch_limit(0)
    for k in ("mean", "cov", "lpd", "total", "info"):
        assert one[k].tobytes() == two[k].tobytes(), k
    for k in ("mean", "cov", "info"):
        assert imp[k].tobytes() == imp2[k].tobytes(), k
    sites = (0, 31, 63)
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), float(v))
    cases = {}
    for s in sites:
        onet, model, tbl, taxa = IR.batch_site(p, s)
        pre = onet.vec_node
        oe = [onet.parent_edges(pre[nodes[f]])[0] for f, _ in edges]
        sh = {ed.number: v for ed, v in zip(oe, values[s])}
        w = ShiftedModel(model, sh)
        cases[s] = (onet, model, tbl, taxa, oe)
        dense = OD.loglik(onet, w, tbl, taxa)
        note("loglik", abs(ll[s] - dense) / max(1.0, abs(dense)))
        st = dense_statement(onet, model, sh, tbl, taxa)
        note("dR", rel_block(grad["dR"][s], st["dR"]))
        note("dmu", rel_block(grad["dmu"][s], st["dmu"]))
        for k in ("dlength", "dgamma", "dshift"):
            note(k, rel_block_nan(eg[k][s], st[k][1:]))
        note("shift_gradient", rel_block(gs[s], np.array([ed.gamma * st["dshift"][nodes[f]] for (f, _), ed in zip(edges, oe)])))
        d = {k: (v[s] if k != "families" else v) for k, v in one.items()}
        note("loo", LR.worst_error(fam["data_row"][one["families"]], d, LR.dense_loo(onet, w, tbl, taxa), p))
        di = {k: (v[s] if k in ("mean", "cov", "info") else v) for k, v in imp.items()}
        note("impute", IR.worst_error(di, IR.dense_impute(onet, w, tbl, taxa)))
    print("batch, per-site shifts, sites 0 / 31 / 63: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (k, v)
    # every site's own fit
    # (the edge set of the fit tests: three internal edges with at least three tips below; the tree is the same at every site)
    onet, model = cases[0][0], cases[0][1]
    fit_nodes = [next(i for i, n in enumerate(onet.vec_node) if n is ed.child) for ed in fit_edges(onet, model)]
    edges = [(i - 1, 0) for i in fit_nodes]
    cgb.set_shifts_lg(edges, np.zeros((len(edges), p)))
    _, gs = cgb.loglik_and_shift_gradient_lg(spt, all_sites=True)
    fit = P.fit_shifts_lg(cgb, spt, edges, all_sites=True)
    assert fit["shifts"].shape == (64, len(edges), p) and fit["H"].shape == (64, len(edges) * p, len(edges) * p)
    g1 = cgb.shift_gradient_lg(all_sites=True)
    wf = {}
    for s in sites:
        onet, model, tbl, taxa, _ = cases[s]
        oe = [onet.parent_edges(onet.vec_node[i])[0] for i in fit_nodes]
        shat_d, H_d, ll_d = gls_fit(onet, model, tbl, taxa, oe)
        assert np.linalg.cond(H_d) <= 100.0
        for k, v in (("shat", rel_block(fit["shifts"][s], shat_d)), ("H", rel_block(fit["H"][s], H_d)),
                     ("loglik", abs(fit["loglik"][s] - ll_d) / abs(ll_d)),
                     ("se", rel_block(fit["se"][s].reshape(-1), np.sqrt(np.diag(np.linalg.inv(H_d))))),
                     ("score", np.max(np.abs(g1[s])) / np.max(np.abs(gs[s])))):
            wf[k] = max(wf.get(k, 0.0), float(v))
    print("batch, fit of every site, sites 0 / 31 / 63 vs dense GLS: " + ", ".join(f"{k} {v:.2e}" for k, v in wf.items()))
    for k, v in wf.items():
        assert v <= TOL, (k, v)
    assert cgb.shift_count_lg() == len(edges)


# ----------------------------------------------------------------------------- 6: the fit

def _fit_cases():
    for which in ("bm", "ou"):
        yield (f"{which}_random_root",) + _case(which)
    yield from _more_cases()


@pytest.mark.parametrize("case", list(_fit_cases()), ids=lambda c: c[0])
def test_fit_shifts_against_dense_gls(P, case):
    """fit_shifts_lg on the edge sets of test_shift_cpu.test_fit_is_dense_gls: shat, H and the log-likelihood at shat against
    dense GLS; the shift gradient at shat is at most 1e-8 of its size at 0."""
    name, net, model, tbl, taxa = case
    # (the oracle allocates the scopes; its own assignfactors, which raises on the two missing-data inputs for the plain model
    # already -- test_shift_cpu.py --, is not needed: the comparator is dense)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa, oracle_factors=False)
    oe = fit_edges(net, model)
    edges = [family_of_edge(net, ocgb, fam, ed) for ed in oe]
    shat_d, H_d, ll_d = gls_fit(net, model, tbl, taxa, oe)
    assert np.linalg.cond(H_d) <= 100.0
    pcgb.set_shifts_lg(edges, np.zeros((len(edges), model.dimension())))
    _, g0 = pcgb.loglik_and_shift_gradient_lg(spt)
    fit = P.fit_shifts_lg(pcgb, spt, edges)
    g1 = pcgb.shift_gradient_lg()
    e = dict(shat=rel_block(fit["shifts"], shat_d), H=rel_block(fit["H"], H_d), loglik=abs(fit["loglik"] - ll_d) / abs(ll_d),
             se=rel_block(fit["se"].reshape(-1), np.sqrt(np.diag(np.linalg.inv(H_d)))),
             score=float(np.max(np.abs(g1)) / np.max(np.abs(g0))))
    print(f"{name}: cond(H) {np.linalg.cond(H_d):.2f}, " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v <= TOL, (k, v)
    assert pcgb.shift_count_lg() == len(edges)


def test_fit_refuses_an_unidentifiable_pair(P):
    """Both child edges of the root under an improper root: only their difference is identified; ValueError names the entry."""
    net, model, tbl, taxa = LR.reference_case("level1_2traits", "improper")
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    pre = net.vec_node
    kids = [ed for ed in net.edges if ed.parent is pre[0]]
    assert len(kids) == 2 and not any(ed.hybrid for ed in kids)
    edges = [family_of_edge(net, ocgb, fam, ed) for ed in kids]
    with pytest.raises(ValueError, match=rf"family {edges[1][0]}, parent {edges[1][1]}\), trait 0"):
        P.fit_shifts_lg(pcgb, spt, edges)

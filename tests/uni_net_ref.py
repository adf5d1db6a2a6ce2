"""Tests only: four small networks whose HYBRID NODE IS A TIP, with per-site data and parameters, built on the oracle's host
side (and read by the product's), shared by tests/test_uni_cases_cpu.py and tests/test_gpu_uni_networks.py.

A hybrid tip puts a family with two parents into a cluster that absorbs data, and with univariate traits every belief keeps
at most 2 variables: the one input class that reaches, off clique trees of trees, the thread-per-site kernels (every belief
<= 2 variables, >= 8 sites) -- 2-variable sepsets (bp_level_uni), 0-variable clusters and sepsets, the hybrid branch of the
site-minor fill and of the site-minor shift correction, and loopy Bethe graphs.  oracle.network.random_network only makes
internal hybrids.

The oracle reads `#H1` without children as a hybrid node; `network()` marks it a leaf, which is what pgbp_amd.read_newick
does by itself.  Every device engine of the GPU tests is built from the ORACLE's cluster graph (helpers.lg_inputs_from_oracle
+ engine_arrays): the product's own cliquetree triangulates N1 differently and gets a 3-variable cluster.
"""
import functools
import types

import numpy as np

from helpers import lg_inputs_from_oracle, oracle_setup
from oracle import calibration as OC
from oracle import clustergraph as OCG
from oracle import models as OM
from oracle import network as ON

NEWICK = {
    "N1": "((t1:1.0,(t3:0.2,#H1:0.3::0.4)c:0.4)a:0.5,(t2:1.0,#H1:0.4::0.6)b:0.7)r;",
    "N2": "((t1:1.0,#H1:0.3::0.4,#H2:0.2::0.7)a:0.5,(t2:1.0,#H1:0.4::0.6,#H2:0.5::0.3)b:0.7)r;",
    "N3": "((t1:1.0,#H1:0.3::0.4)a:0.5,(t2:1.0,#H1:0.4::0.6)b:0.7,(t3:0.3,t4:0.6)c:0.2)r;",
    "N4": "((t1:1,#H1:0.3::0.4)a:0.5,t2:1.0,#H1:0.4::0.6)r;",     # one parent of the hybrid tip is the root
}
ROOTS = {"N1": ("fixed", "random"), "N2": ("fixed", "random"), "N3": ("fixed", "random"), "N4": ("fixed",)}
MAX_SITES = 65
# the loopy calibrations of tests/test_gpu_uni_networks.py (random root: every sepset of the Bethe graph holds one variable),
# compared with the oracle after each of LOOPY_STEPS iterations at every site
LOOPY_CASES = (("N1", "random", "bm"), ("N2", "random", "bm"), ("N3", "random", "bm"), ("N1", "random", "ou"))
LOOPY_STEPS = (1, 2, 30)


def network(name):
    """(oracle Network with its childless hybrids marked as leaves, taxa = its tips in preorder)"""
    net = ON.read_newick(NEWICK[name])
    for n in net.nodes:
        if n.hybrid and not net.child_edges(n):
            n.leaf = True
    return net, list(net.tip_names)


def graph(net, kind):
    return OCG.cliquetree(net) if kind == "cliquetree" else OCG.bethe(net)


@functools.lru_cache(maxsize=None)
def sites(name, root, kind):
    """MAX_SITES sites of one case: [(model, tbl)] with their own (sigma2, mu) -- and (alpha, theta) for kind "ou", a prior
    variance for a random root -- and their own tip values.  An engine of n sites takes the first n."""
    net, taxa = network(name)
    rng = np.random.default_rng([ord(c) for c in name + root + kind])
    out = []
    for _ in range(MAX_SITES):
        sigma2, mu = float(rng.uniform(0.5, 2.0)), float(rng.normal())
        v = float(rng.uniform(0.5, 2.0)) if root == "random" else None
        if kind == "ou":
            model = OM.UnivariateOrnsteinUhlenbeck(sigma2, float(rng.uniform(0.3, 1.5)), float(rng.normal()), mu, v)
        else:
            model = OM.UnivariateBrownianMotion(sigma2, mu, v)
        tbl = [[float(x) for x in 1.5 * rng.normal(size=len(taxa))]]
        out.append((model, tbl))
    return out


def dims_of(net, cg, model, tbl, taxa):
    """(cluster dimensions, sepset dimensions) of the oracle's beliefs"""
    ocgb = oracle_setup(net, cg, model, tbl, taxa)
    d = [b.dimension for b in ocgb.belief]
    return d[:ocgb.nclusters], d[ocgb.nclusters:]


def engine_arrays(P, ocgb):
    """The description arrays of include/pgbp.h (dims, sepset_clusters, scope_off, scope_idx) of the oracle's beliefs, as
    pgbp_amd.ClusterGraphBelief.__init__ derives them for one site."""
    from helpers import product_beliefs_from_oracle
    from pgbp_amd.beliefs import scopeindex
    pb = product_beliefs_from_oracle(ocgb.belief)
    nc = ocgb.nclusters
    cdict = {pb[j].metadata: j for j in range(nc)}
    dims = np.array([b.dimension for b in pb], np.int32)
    sepcl, off, idx = [], [0], []
    for j in range(nc, len(pb)):
        a, b = (cdict[x] for x in pb[j].metadata)
        sepcl += [a, b]
        for c in (a, b):
            ind = np.asarray(scopeindex(pb[j], pb[c]), np.int32)
            idx.append(ind)
            off.append(off[-1] + len(ind))
    idx = np.concatenate(idx).astype(np.int32) if idx else np.zeros(0, np.int32)
    return dims, np.array(sepcl, np.int32), np.array(off, np.int64), idx


def pack(ocgb):
    return np.concatenate([np.concatenate([b.J.reshape(-1, order="F"), b.h, [b.g[0]]]) for b in ocgb.belief])


def schedule(net, cg, graph_kind):
    if graph_kind == "cliquetree":
        return [OCG.spanningtree_clusterlist(cg, OCG.default_rootcluster(cg, net))]
    return OCG.spanningtrees_clusterlist(cg, net)


def device_batch(P, name, root, kind, graph_kind, n_sites, assign=True):
    """An n_sites engine of a case on the oracle's cluster graph, filled on the device with per-site parameters:
    namespace(net, taxa, cg, sched, fam, kw (per-site keyword arguments of assignfactors_lg_), pcgb, sites, ocgb0)."""
    net, taxa = network(name)
    cg = graph(net, graph_kind)
    ss = sites(name, root, kind)[:n_sites]
    ocgb0 = oracle_setup(net, cg, ss[0][0], ss[0][1], taxa)
    dims, sepcl, so, si = engine_arrays(P, ocgb0)
    per = [lg_inputs_from_oracle(P, net, ocgb0, m, t, taxa) for m, t in ss]
    fam = per[0][0]
    data = np.stack([d for _, d, _ in per])
    kw = dict(R=np.stack([k["R"] for _, _, k in per]), mu=np.stack([k["mu"] for _, _, k in per]))
    if kind == "ou":
        kw.update(model="ou", alpha=np.array([k["alpha"] for _, _, k in per]), theta=np.stack([k["theta"] for _, _, k in per]))
    pcgb = P.ClusterGraphBelief.from_arrays(dims, sepcl, so, si, None, n_sites=n_sites)
    pcgb.lg_setup(fam, data)
    if assign:
        pcgb.assignfactors_lg_(**kw)
    return types.SimpleNamespace(net=net, taxa=taxa, cg=cg, sched=schedule(net, cg, graph_kind), fam=fam, kw=kw, pcgb=pcgb,
                                 sites=ss, ocgb0=ocgb0, dims=dims)


@functools.lru_cache(maxsize=None)
def oracle_factors(name, root, kind, graph_kind, site):
    """packed beliefs of the oracle's assignfactors of one site (sepsets: the constant 1)"""
    net, taxa = network(name)
    m, t = sites(name, root, kind)[site]
    return pack(oracle_setup(net, graph(net, graph_kind), m, t, taxa))


def _snapshot(ocgb, got):
    """the state of an oracle calibration: packed beliefs, and per directed message (in the device's order: sepset k, received
    by its first cluster, then by its second) the residual flag and the two norms iscalibrated_residnorm! compares with atol"""
    mrs = list(ocgb.messageresidual.values())
    nrm = lambda x: float(np.max(np.abs(x))) / np.sqrt(x.size) if x.size else 0.0
    return types.SimpleNamespace(packed=pack(ocgb), got=got, flags=np.array([bool(m.iscalibrated_resid) for m in mrs]),
                                 nh=np.array([nrm(m.dh) for m in mrs]), nJ=np.array([nrm(m.dJ) for m in mrs]))


@functools.lru_cache(maxsize=None)
def oracle_calibration(name, root, kind, graph_kind, site, steps=(1,)):
    """{n: snapshot after n iterations} of the oracle's calibrate! on one site, and the oracle's beliefs after the last.
    calibrate!(n) is run in pieces (steps increasing): the loop of src/calibration.jl:46 carries no state between iterations."""
    net, taxa = network(name)
    cg = graph(net, graph_kind)
    m, t = sites(name, root, kind)[site]
    ocgb = oracle_setup(net, cg, m, t, taxa)
    sched = schedule(net, cg, graph_kind)
    out, done = {}, 0
    for n in steps:
        got = OC.calibrate(ocgb, sched, n - done, verbose=False)
        done = n
        out[n] = _snapshot(ocgb, got)
    return out, ocgb


def records_error(got, want, dims):
    """worst |got - want| over the records of a packed belief vector, each relative to max(1, |want record|_inf)"""
    d = np.asarray(dims, np.int64)
    off = np.concatenate([[0], np.cumsum(d * d + d + 1)])
    worst = 0.0
    for i in range(len(d)):
        a, b = got[off[i]:off[i + 1]], want[off[i]:off[i + 1]]
        worst = max(worst, float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b)))))
    return worst


def hybrid_factor_error(net, model):
    """The model's own factor of every family against the GENERIC one that oracle.models.EvolutionaryModel derives from
    branch_qwv alone: (worst relative difference, number of hybrid families)."""
    worst, nh = 0.0, 0
    for n in net.vec_node[1:]:
        pae = net.parent_edges(n)
        if len(pae) == 1:
            mine, gen = model.factor_treeedge(pae[0]), OM.EvolutionaryModel.factor_treeedge(model, pae[0])
        else:
            nh += 1
            mine, gen = model.factor_hybridnode(pae), OM.EvolutionaryModel.factor_hybridnode(model, pae)
        for a, b in zip(mine, gen):
            a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
            worst = max(worst, float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b)))))
    return worst, nh

"""pgbp_lg_gradient / ClusterGraphBelief.gradient_lg: the exact gradient of the log-likelihood from calibrated beliefs, one
sweep over the node families on the device.

Comparators: (a) the numpy statement of Fisher's identity on the DENSE oracle's posterior moments
(test_gradient_cpu.dense_gradient, itself pinned to finite differences of densemvn.loglik there), asserted at 1e-8 relative
to the largest entry of each gradient block; (b) where the dense posterior does not apply (improper root; the loopy case),
Richardson central differences of densemvn.loglik (of the device's free energy) with two step pairs (1e-3 / 5e-4 and
2e-3 / 1e-3): their disagreement is the comparator's uncertainty, the assertion is at max(10 x that, 1e-8), and the figures
are printed."""
import ctypes as C

import numpy as np
import pytest

from helpers import goldens, lg_inputs_from_oracle, make_model, oracle_setup, product_beliefs_from_oracle
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from test_gradient_cpu import dense_gradient, fd_gradient, rel_block

pytestmark = pytest.mark.gpu
G = goldens()
BLOCKS = ("dR", "dmu", "dalpha", "dtheta")


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _device(P, net, model, tbl, taxa, graph="cliquetree"):
    """One-site engine on the clique tree (or Bethe graph) of an oracle network, families set up, factors assigned."""
    cg = OCG.cliquetree(net) if graph == "cliquetree" else OCG.bethe(net)
    ocgb = oracle_setup(net, cg, model, tbl, taxa)
    pb = product_beliefs_from_oracle(ocgb.belief)
    for b in pb:
        b.J[...] = 0.0
        b.h[...] = 0.0
        b.g[...] = 0.0
    pcgb = P.ClusterGraphBelief(pb, ocgb.node2cluster, ocgb.node2family, ocgb.node2fixed, ocgb.cluster2nodes)
    fam, data, kw = lg_inputs_from_oracle(P, net, ocgb, model, tbl, taxa)
    pcgb.lg_setup(fam, data)
    pcgb.assignfactors_lg_(**kw)
    spt = OCG.spanningtree_clusterlist(cg, OCG.default_rootcluster(cg, net)) if graph == "cliquetree" else None
    return cg, ocgb, pcgb, spt


def _is_proper(model):
    v = np.atleast_2d(np.asarray(model.rootpriorvariance(), float))
    return not np.any(np.isinf(np.diag(v)))


def _assert_blocks(tag, got, want, tol, per_color=True):
    worst = 0.0
    for k in BLOCKS:
        w = np.atleast_1d(np.asarray(want[k], float))
        g = np.atleast_1d(np.asarray(got[k], float))
        if not np.any(w) and not np.any(g):
            continue
        parts = list(zip(g, w)) if (k == "dR" and per_color) else [(g, w)]
        for c, (gg, ww) in enumerate(parts):
            err = rel_block(gg, ww)
            worst = max(worst, err)
            print(f"{tag} {k}[{c}]: {err:.2e} (tolerance {tol:.1e})")
            assert err <= tol, (tag, k, c, gg, ww)
    return worst


def _check_against_oracle(P, tag, net, model, tbl, taxa):
    """Device gradient (and log-likelihood) of one case against the dense statement (proper or fixed root) or against
    finite differences with a measured uncertainty (improper root)."""
    cg, ocgb, pcgb, spt = _device(P, net, model, tbl, taxa)
    ll, got = pcgb.loglik_and_gradient_lg(spt)
    dense = OD.loglik(net, model, tbl, taxa)
    assert abs(ll - dense) <= 1e-8 * max(1.0, abs(dense)), (tag, ll, dense)
    if _is_proper(model):
        return pcgb, spt, _assert_blocks(tag, got, dense_gradient(net, model, tbl, taxa), 1e-8)
    a, b = fd_gradient(net, model, tbl, taxa, 1e-3), fd_gradient(net, model, tbl, taxa, 2e-3)
    unc = max(rel_block(a[k], b[k]) for k in BLOCKS if np.any(np.atleast_1d(a[k])))
    print(f"{tag}: finite-difference comparator uncertainty {unc:.2e}")
    return pcgb, spt, _assert_blocks(tag, got, a, max(10 * unc, 1e-8))


def _bm(p, rng, root):
    A = rng.normal(size=(p, p))
    R = A @ A.T / p + np.eye(p)
    if root == "fixed":
        return OM.MvFullBrownianMotion(R, rng.normal(size=p))
    if root == "random":
        B = rng.normal(size=(p, p))
        return OM.MvFullBrownianMotion(R, rng.normal(size=p), B @ B.T / p + 0.5 * np.eye(p))
    return OM.MvFullBrownianMotion(R, np.zeros(p), np.diag(np.full(p, np.inf)))


# ----------------------------------------------------------------------------- 1: the reference's networks

def _golden_cases():
    g = G["exact_reml_level1"]
    yield "level1_1trait", g["net"], g["taxa"], [g["y"]]
    yield "level1_2traits", g["net"], g["taxa"], [g["x"], g["y"]]
    g = G["optimization_mateescu"]
    yield "mateescu", G["joingraph_mateescu"]["net"], g["taxa"], [g["y"]]
    c = G["optimization_level1"]["cliquetree"]
    yield "optimization_level1", c["net"], c["taxa"], [c["y"]]
    g = G["optimization_sun2023"]
    yield "sun2023", g["net"], g["taxa_in_file_order"], [g["y1"], g["y2"]]


@pytest.mark.parametrize("root", ["fixed", "random", "improper"])
@pytest.mark.parametrize("case", list(_golden_cases()), ids=lambda c: c[0])
def test_gradient_reference_networks(P, case, root):
    """The networks of the reference's own tests, full BM with a fixed, a proper random and an improper root.  Measured
    (MI355X): every block passes at 1e-8; the finite-difference comparator's own uncertainty on the improper-root cases is
    9e-13 .. 2.1e-11 (3.9e-11 at most on the random networks below), so those are asserted at 1e-8 as well."""
    name, netstr, taxa, cols = case
    net = ON.read_newick(netstr)
    p = len(cols)
    rng = np.random.default_rng(11)
    tbl = [[None if v is None else float(v) for v in col] for col in cols]
    _check_against_oracle(P, f"{name}/{root}", net, _bm(p, rng, root), tbl, taxa)


# ----------------------------------------------------------------------------- 2: random networks, every model

@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("which,p", [("bm_fixed", 1), ("bm_random", 2), ("bm_improper", 2), ("bm_random", 4), ("hetero_fixed", 2),
                                     ("hetero_random", 4), ("hetero_improper", 1), ("ou_fixed", 1), ("ou_random", 1), ("ou_improper", 1)])
def test_gradient_random_networks(P, which, p, seed):
    """24 tips, 6 hybrid nodes: homogeneous BM, heterogeneous BM with 3 colours (each dR[c] asserted on its own), the
    univariate OU (dalpha, dtheta, dR), fixed / random / improper root."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"{which}-{p}-{seed}".encode()))
    net = ON.random_network(24, 6, rng)
    taxa = net.tip_names
    kind, root = which.split("_")
    if kind == "bm":
        model = _bm(p, rng, root)
    elif kind == "hetero":
        base = _bm(p, rng, root)
        rates = [base.R * s for s in (0.5, 1.0, 2.5)]
        colors = {e.number: 1 + int(rng.integers(3)) for e in net.edges}
        model = OM.HeterogeneousBrownianMotion(rates, colors, base.mu, None if root == "fixed" else base.v)
    else:
        model = OM.UnivariateOrnsteinUhlenbeck(rng.uniform(0.5, 2), rng.uniform(0.1, 1), rng.normal(), rng.normal(),
                                               {"fixed": 0.0, "random": 0.8, "improper": np.inf}[root])
    tbl = [list(rng.normal(size=len(taxa))) for _ in range(p)]
    pcgb, spt, _ = _check_against_oracle(P, f"{which}/p{p}/s{seed}", net, model, tbl, taxa)
    if kind == "hetero":
        assert pcgb.gradient_lg()["dR"].shape[0] == 3 + (root == "random")


# ----------------------------------------------------------------------------- 3: missing tip values (scope masks)

def test_gradient_missing_values(P):
    """calibration_tree_2traits_missing (y2 observed at one tip only), exact_reml_missing (a subtree without data: its
    families are skipped) and a random pattern on a random network."""
    g = G["calibration_tree_2traits_missing"]
    _check_against_oracle(P, "tree_2traits_missing", ON.read_newick(g["net"]), make_model(g["model"]), [g["y1"], g["y2"]],
                          g["taxa"])
    g = G["exact_reml_missing"]
    for root in ("random", "improper"):
        _check_against_oracle(P, f"exact_reml_missing/{root}", ON.read_newick(g["net"]), _bm(1, np.random.default_rng(3), root),
                              [g["x"]], g["taxa"])
    rng = np.random.default_rng(21)
    net = ON.random_network(20, 4, rng)
    taxa = net.tip_names
    for p, root in ((3, "random"), (2, "fixed")):
        tbl = [[None if rng.random() < 0.3 else float(rng.normal()) for _ in taxa] for _ in range(p)]
        for r in range(len(taxa)):           # (every tip keeps at least one value)
            if all(tbl[t][r] is None for t in range(p)):
                tbl[0][r] = float(rng.normal())
        _check_against_oracle(P, f"random_pattern/p{p}/{root}", net, _bm(p, rng, root), tbl, taxa)


# ----------------------------------------------------------------------------- 4: every dimension class of the solve

def _muller(P, p):
    """The clique tree of the Mueller et al. (2022) network (tests/golden/muller_2022.phy: 801 nodes, 361 hybrids, a clique of
    54 nodes), fixed root, BM data simulated on the network; the oracle network with the same preorder for the dense side."""
    import os
    from helpers import HERE, network_from_newick_file
    net, names, onet, _ = network_from_newick_file(P, os.path.join(HERE, "golden", "muller_2022.phy"))
    tips = [names[i] for i in range(net.nnodes) if net.is_leaf[i]]
    cn, ed, sn = P.cliquetree(net.node2family)
    assert len(cn) == G["clustergraphs_muller2022"]["cliquetree"]["clusters"] and max(len(c) for c in cn) == 54
    st = P.allocate_scopes(cn, ed, sn, net, p)
    rng = np.random.default_rng(2)
    A = rng.normal(size=(p, p))
    R = A @ A.T / p + np.eye(p)
    mu = rng.normal(size=p)
    X = P.simulate_bm_network(net, R[None], mu, rng)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, list(range(net.nnodes)), p, n_rates=1)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(fam, X)
    cgb.assignfactors_lg_(R[None], mu)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    node_of = {names[i]: i for i in range(net.nnodes)}
    tbl = [[float(X[node_of[t], k]) for t in tips] for k in range(p)]
    return cgb, spt, st, onet, OM.MvFullBrownianMotion(R, mu), tbl, tips


def test_gradient_wavefront_class_and_layouts(P):
    """A tree with p = 16: clusters of 32 variables (the wavefront class) against the dense statement.  After the calibration
    the engine holds its beliefs in the packed BS16 layout (asserted through pgbp_layout); the sweep on the SAME beliefs
    converted to the plain layout (pgbp_get_belief converts) gives the same values.  Not the same bytes: a packed record
    keeps both triangles of its diagonal 16 x 16 tiles as the message kernels left them (equal up to the last bit), and the
    elimination takes its multipliers from the stored lower triangle there but from the mirrored upper triangle of a plain
    record (PDMat(Symmetric(J))), as pgbp_moments does.  The two solves differ by roundings of 2^-53 amplified by the
    conditioning of 32 x 32 systems: asserted at 1e-12 relative to the largest entry of a block, the bound the batch test
    uses for its two fill routes; the measured figure is printed (MI355X: 1.8e-16 dR, 9.2e-17 dmu)."""
    from pgbp_amd import _lib as L
    rng = np.random.default_rng(5)
    tree = ON.random_network(12, 0, rng)
    assert max(len(nodes) for _, nodes in OCG.cliquetree(tree).clusters) * 16 == 32
    tbl = [list(rng.normal(size=12)) for _ in range(16)]
    pcgb, spt, _ = _check_against_oracle(P, "tree/p16", tree, _bm(16, rng, "random"), tbl, tree.tip_names)
    lib, eng = pcgb._lib, pcgb._eng
    assert lib.pgbp_layout(eng) == 1, "the p = 16 tree is expected in the packed layout after a calibration"
    packed = pcgb.gradient_lg()
    rec = np.zeros(int(pcgb._dims[0]) ** 2 + int(pcgb._dims[0]) + 1)
    assert lib.pgbp_get_belief(eng, 0, 0, L.f64p(rec)) == L.PGBP_OK
    assert lib.pgbp_layout(eng) == 0
    plain = pcgb.gradient_lg()
    for k in ("dR", "dmu"):
        err = rel_block(packed[k], plain[k])
        print(f"packed vs plain layout, {k}: {err:.2e}")
        assert err <= 1e-12, k


def test_gradient_workgroup_class_muller_2_traits(P):
    """The Mueller clique tree at 2 traits: beliefs of up to 108 variables (the workgroup class, 65 .. 128), 1 160 families;
    log-likelihood and every gradient block against the dense oracle at 1e-8."""
    cgb, spt, st, onet, model, tbl, tips = _muller(P, 2)
    assert 64 < int(st.dims.max()) <= 128
    print("Mueller, 2 traits: largest belief", int(st.dims.max()), "variables")
    ll, got = cgb.loglik_and_gradient_lg(spt)
    dense = OD.loglik(onet, model, tbl, tips)
    assert abs(ll - dense) <= 1e-8 * abs(dense), (ll, dense)
    _assert_blocks("muller/p2", got, dense_gradient(onet, model, tbl, tips), 1e-8)


def test_gradient_refuses_clusters_above_128_variables(P):
    """The Mueller clique tree at 3 traits has beliefs of more than 128 variables: PGBP_ERR_INVALID before any launch, the
    family and its cluster named."""
    from pgbp_amd import _lib as L
    cgb, spt, st, *_ = _muller(P, 3)
    assert int(st.dims.max()) > 128
    assert P.calibrate_(cgb, [spt])[0]
    with pytest.raises(L.PgbpError) as ex:
        cgb.gradient_lg()
    assert ex.value.code == L.ERR_INVALID and "more than 128 variables" in ex.value.msg and "family" in ex.value.msg


def test_gradient_refuses_what_does_not_fit_the_lds(P):
    """p = 64 on a tree: clusters of 128 variables (133 KB of working matrix) plus the p x p scratch of the family exceed the
    160 KB of LDS: PGBP_ERR_INVALID before any launch."""
    from pgbp_amd import _lib as L
    rng = np.random.default_rng(8)
    tree = ON.random_network(5, 0, rng)
    tbl = [list(rng.normal(size=5)) for _ in range(64)]
    _, _, pcgb, spt = _device(P, tree, _bm(64, rng, "random"), tbl, tree.tip_names)
    with pytest.raises(L.PgbpError) as ex:
        pcgb.gradient_lg()
    assert ex.value.code == L.ERR_INVALID and "bytes of LDS" in ex.value.msg


# ----------------------------------------------------------------------------- 5: batches, determinism, refusals, info

def _tree_batch(P, n_sites, p, seed, fixedroot):
    from test_gpu_exact_bm import _random_tree
    S, rng, tr, nwk, taxa = _random_tree(20, seed)
    net, names = P.read_newick(nwk)
    row = {t: r for r, t in enumerate(taxa)}
    data_row = [row.get(names[i], -1) for i in range(net.nnodes)]
    cn, ed, sn = P.cliquetree(net.node2family)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=fixedroot)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed, pe, data_row, p)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    data = rng.normal(size=(n_sites, len(taxa), p))
    Rs = np.stack([(lambda A: A @ A.T / p + np.eye(p))(rng.normal(size=(p, p))) for _ in range(n_sites)])
    mus = rng.normal(size=(n_sites, p))

    def engine(sites):
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=len(sites))
        cgb.lg_setup(fam, data[sites])
        cgb.assignfactors_lg_(Rs[sites][:, None], mus[sites])
        return cgb
    onet = ON.read_newick(nwk)
    onet.set_preorder(names)
    return engine, spt, onet, taxa, data, Rs, mus


@pytest.mark.parametrize("p", [1, 2])
def test_gradient_batch_of_64_sites(P, p):
    """64 sites with their own data and parameters equal 64 one-site calls.  p = 2: both engines run the same kernels on the
    same plain layout, so every block is the same bytes.  p = 1: the batch is filled and calibrated by the thread-per-site
    kernels of the site-minor layout (closed forms at dimension <= 2), the one-site engine by the wavefront kernels: the
    beliefs the sweep reads agree to rounding, so 1e-12 relative there.  Sites 0 and 63 equal the dense statement; a site
    range returns the rows of the full call; two calls return identical bytes."""
    engine, spt, onet, taxa, data, Rs, mus = _tree_batch(P, 64, p, 40 + p, True)
    cgb = engine(np.arange(64))
    ll, got = cgb.loglik_and_gradient_lg(spt, all_sites=True)
    assert not got["info"].any()
    again = cgb.gradient_lg(all_sites=True)
    for k in BLOCKS:
        assert np.array_equal(got[k], again[k]), k
    for s in range(64):
        one = engine(np.array([s]))
        ll1, g1 = one.loglik_and_gradient_lg(spt, all_sites=True)
        for k in ("dR", "dmu"):
            if p == 2:
                assert np.array_equal(got[k][s], g1[k][0]), (s, k)
            else:
                assert rel_block(got[k][s], g1[k][0]) <= 1e-12, (s, k)
        assert abs(ll[s] - ll1[0]) <= 1e-12 * abs(ll1[0])
    for s in (0, 63):
        model = OM.MvFullBrownianMotion(Rs[s], mus[s])
        tbl = [list(data[s][:, t]) for t in range(p)]
        want = dense_gradient(onet, model, tbl, taxa)
        _assert_blocks(f"site {s}", {k: got[k][s] for k in BLOCKS}, want, 1e-8)
        dense = OD.loglik(onet, model, tbl, taxa)
        assert abs(ll[s] - dense) <= 1e-8 * abs(dense)
    # a site range
    n = 7
    dR = np.zeros((n, 1, p, p)); dmu = np.zeros((n, p)); info = np.ones(n, np.int32)
    from pgbp_amd import _lib as L
    rc = cgb._lib.pgbp_lg_gradient(cgb._eng, 20, 27, L.f64p(dR), L.f64p(dmu), None, None, L.i32p(info))
    assert rc == L.PGBP_OK and not info.any()
    assert np.array_equal(dR.transpose(0, 1, 3, 2), got["dR"][20:27]) and np.array_equal(dmu, got["dmu"][20:27])


def test_gradient_refusals_and_info(P):
    """No family table / no parameters: PGBP_ERR_STATE; a site range out of bounds, dalpha / dtheta NULL on an OU engine:
    PGBP_ERR_INVALID; a site whose rate matrix is not positive definite reports info and NaN, its neighbours are right."""
    from pgbp_amd import _lib as L
    engine, spt, onet, taxa, data, Rs, mus = _tree_batch(P, 3, 2, 50, True)
    cgb = engine(np.arange(3))
    lib, eng = cgb._lib, cgb._eng
    dR = np.zeros((3, 1, 2, 2)); dmu = np.zeros((3, 2)); info = np.zeros(3, np.int32)
    args = (L.f64p(dR), L.f64p(dmu), None, None, L.i32p(info))
    assert lib.pgbp_lg_gradient(eng, 0, 4, *args) == L.ERR_INVALID
    assert lib.pgbp_lg_gradient(eng, -1, 2, *args) == L.ERR_INVALID
    assert lib.pgbp_lg_gradient(eng, 2, 1, *args) == L.ERR_INVALID
    # a fresh engine: no family table; with a table but before the first assignfactors: no parameters
    from test_gpu_exact_bm import _random_tree
    S, rng, tr, nwk, taxa2 = _random_tree(8, 3)
    net, names = P.read_newick(nwk)
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, 1)
    fresh = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    one = (L.f64p(np.zeros(1)), L.f64p(np.zeros(1)), None, None, None)
    assert fresh._lib.pgbp_lg_gradient(fresh._eng, 0, 1, *one) == L.ERR_STATE
    assert b"pgbp_lg_setup" in fresh._lib.pgbp_last_error(fresh._eng)
    row = {t: r for r, t in enumerate(taxa2)}
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], 1)
    fresh.lg_setup(fam, rng.normal(size=(len(taxa2), 1)))
    assert fresh._lib.pgbp_lg_gradient(fresh._eng, 0, 1, *one) == L.ERR_STATE
    assert b"pgbp_lg_assignfactors" in fresh._lib.pgbp_last_error(fresh._eng)
    fresh.assignfactors_lg_(np.array([[[1.0]]]), [0.0], model="ou", alpha=0.5, theta=[0.1])
    assert fresh._lib.pgbp_lg_gradient(fresh._eng, 0, 1, *one) == L.ERR_INVALID
    assert b"dalpha" in fresh._lib.pgbp_last_error(fresh._eng)
    # site 1: a rate matrix that is not positive definite
    bad = Rs.copy()
    bad[1] = np.array([[1.0, 2.0], [2.0, 1.0]])
    good_ll, good = cgb.loglik_and_gradient_lg(spt, all_sites=True)
    cgb.assignfactors_lg_(bad[:, None], mus)
    ll, got = cgb.loglik_and_gradient_lg(spt, all_sites=True)
    assert got["info"][1] != 0 and got["info"][0] == 0 and got["info"][2] == 0
    assert np.isnan(got["dR"][1]).all() and np.isnan(got["dmu"][1]).all() and np.isnan(ll[1])
    for s in (0, 2):
        for k in ("dR", "dmu"):
            assert np.array_equal(got[k][s], good[k][s]), (s, k)


# ----------------------------------------------------------------------------- 6: the optimiser

def test_gradient_vanishes_at_the_optimum_and_analytic_fit(P):
    """Mateescu network (test/test_optimization.jl:5-26): at the optimum of the existing central-difference fit the analytic
    gradient in the optimiser's coordinates is ~ 0 -- bound: _minimise accepts an end point whose central-difference gradient
    norm is <= 1e-5 max(1, |f|), and that gradient carries ~1e-7 of its start size in truncation / rounding, so
    |g_opt| <= 1e-5 max(1, |ll|) + 1e-6 |g_start|.  gradient="analytic" reaches the reference's optimum within the tolerances
    of test_calibrate_optimize_cliquetree_golden with fewer device evaluations (both counts printed)."""
    from pgbp_amd.optimize import _BMTransform
    from test_gpu_lgfill import _mateescu_on_device
    g, net, (cn, ed, sn), cgb = _mateescu_on_device(P, "cliquetree")
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    start = ([[g["start"]["sigma2"]]], [g["start"]["mu"]])
    tf = _BMTransform(1)

    def theta_gradient(R, mu):
        cgb.assignfactors_lg_(np.asarray(R, float)[None], mu)
        ll, d = cgb.loglik_and_gradient_lg(spt)
        return ll, tf.pullback(tf.forward(R, mu), d["dR"][0], d["dmu"])
    _, g0 = theta_gradient(*start)
    R, mu, ll, opt = P.calibrate_optimize_cliquetree_(cgb, spt, *start)
    ll1, g1 = theta_gradient(R, mu)
    print("gradient norm: start", np.linalg.norm(g0), "optimum", np.linalg.norm(g1), "central evaluations", opt.n_device_evals)
    assert abs(ll1 - ll) <= 1e-12 * abs(ll)
    assert np.linalg.norm(g1) <= 1e-5 * max(1.0, abs(ll)) + 1e-6 * np.linalg.norm(g0)
    Ra, mua, lla, opta = P.calibrate_optimize_cliquetree_(cgb, spt, *start, gradient="analytic")
    print("analytic evaluations", opta.n_device_evals, "ll", lla, "sigma2", Ra[0, 0], "mu", mua[0])
    assert abs(lla - g["ref_ll"]) <= 1e-12 * abs(g["ref_ll"])
    assert abs(Ra[0, 0] - g["ref_sigma2"]) <= 1e-7 * g["ref_sigma2"]
    assert abs(mua[0] - g["ref_mu"]) <= 1e-7 * abs(g["ref_mu"])
    assert opta.n_device_evals < opt.n_device_evals
    with pytest.raises(ValueError):
        P.calibrate_optimize_cliquetree_(cgb, spt, *start, gradient="forward")


def test_analytic_fit_sun2023_bivariate_improper_root(P):
    """test/test_optimization.jl:52-100 with gradient="analytic": the recorded maximum -32.22404541422671 and rate matrix
    within the tolerances of test_calibrate_optimize_sun2023_bivariate_improper_root."""
    g = G["optimization_sun2023"]
    net, names = P.read_newick(g["net"])
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, 2, fixedroot=False)
    row = {t: r for r, t in enumerate(g["taxa_in_file_order"])}
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], 2)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(fam, np.stack([g["y1"], g["y2"]], axis=1))
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    R, mu, ll, opt = P.calibrate_optimize_cliquetree_(cgb, spt, g["start_R"], [0.0, 0.0], maxiter=500, gradient="analytic")
    print("sun2023 analytic: ll", ll, "device evaluations", opt.n_device_evals)
    assert abs(ll - g["ll_max"]) <= 1e-9 * abs(g["ll_max"]), (ll, opt.nfev)
    assert np.allclose(R * g["R_scale"], g["R_recorded"], rtol=1e-4, atol=0), R


# ----------------------------------------------------------------------------- 7: a loopy cluster graph

def test_gradient_of_the_factored_energy_on_a_loopy_graph(P):
    """calibration_bethe_level1 (Bethe cluster graph, univariate BM, fixed root), calibrated with niter = 200, auto=False:
    minus the sweep's (dR, dmu) against Richardson central differences of the device's own free_energy pipeline
    (assignfactors -> calibrate 200 -> free_energy), two step pairs; asserted at max(10 x their disagreement, 1e-8).
    Measured (MI355X): comparator uncertainty 4.6e-8, error 3.1e-9."""
    g = G["calibration_bethe_level1"]
    net = ON.read_newick(g["net"])
    model = make_model(g["model"])
    cg, ocgb, pcgb, _ = _device(P, net, model, [g["y"]], g["taxa"], graph="bethe")
    sched = OCG.spanningtrees_clusterlist(cg, net)
    s2, mu = float(model.R[0, 0]), float(model.mu[0])

    def fe(ds, dm):
        pcgb.assignfactors_lg_(np.array([[[s2 + ds]]]), [mu + dm])
        assert P.calibrate_(pcgb, sched, 200, auto=False, sync=False)[0]
        return pcgb.free_energy(all_sites=True)[0][0, 2]

    def rich(f, h):
        return (4 * (f(h / 2) - f(-h / 2)) / h - (f(h) - f(-h)) / (2 * h)) / 3
    # (steps relative to sigma2 = 0.086)
    fd = [np.array([rich(lambda s: fe(s, 0.0), h * s2), rich(lambda s: fe(0.0, s), h)]) for h in (1e-2, 2e-2)]
    fe(0.0, 0.0)
    d = pcgb.gradient_lg()
    got = -np.array([d["dR"][0, 0, 0], d["dmu"][0]])
    unc = float(np.max(np.abs(fd[0] - fd[1]) / np.abs(fd[0])))
    err = float(np.max(np.abs(got - fd[0]) / np.abs(fd[0])))
    print(f"loopy: sweep {got}, finite differences {fd[0]}, comparator uncertainty {unc:.2e}, error {err:.2e}")
    assert err <= max(10 * unc, 1e-8)


def test_analytic_fit_through_the_bethe_graph(P):
    """calibrate_optimize_clustergraph_(gradient="analytic") on calibration_bethe_level1 (Bethe graph, loopy) against the
    central-difference fit of the same objective.  The sweep is the gradient of the factored energy only at a converged
    calibration and calibrate!(auto) stops at its residual tolerance (1e-5), so the two optima are compared at 1e-4
    relative, the tolerance the reference itself uses for estimates through a Bethe graph (test/test_calibration.jl:187-305)."""
    from test_gpu_lgfill import _on_device_from_newick
    g = G["calibration_bethe_level1"]
    out = {}
    for mode in ("central", "analytic"):
        net, (cn, ed, sn), cgb = _on_device_from_newick(P, g["net"], g["taxa"], [g["y"]], "bethe")
        sched = P.spanningtrees_clusterlist(len(cn), ed, cn, net.is_leaf)
        R, mu, fe, opt = P.calibrate_optimize_clustergraph_(cgb, sched, [[0.5]], [0.0], gradient=mode)
        out[mode] = (R[0, 0], mu[0], fe, opt.n_device_evals)
        print(mode, "sigma2", R[0, 0], "mu", mu[0], "factored energy", fe, "device evaluations", opt.n_device_evals)
    for a, c in zip(out["analytic"][:3], out["central"][:3]):
        assert abs(a - c) <= 1e-4 * abs(c), out

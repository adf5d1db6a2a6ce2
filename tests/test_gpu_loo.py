"""pgbp_lg_loo / ClusterGraphBelief.loo_lg: the leave-one-out predictive mean, covariance and log density of every tip from
one calibration, one sweep over the tip families on the device.

Comparators (tests/loo_ref.py): (a) the DENSE comparator on oracle/densemvn.py alone, asserted at 1e-8 relative to the largest
entry of a block (the project's parity bound); (b) the numpy restatement of the sweep, pinned to (a) on the CPU by
test_loo_cpu.py for every case used here (worst 1.8e-13).  The measured worst error of every case is printed."""
import os

import numpy as np
import pytest

import loo_ref as LR
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from test_gpu_gradient import _device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _rows(pcgb, d):
    return pcgb._lg["data_row"][d["families"]]


def _check(P, tag, net, model, tbl, taxa, tips=None):
    """One-site engine on the clique tree of an oracle case: log-likelihood and every tip's prediction against (a)."""
    cg, ocgb, pcgb, spt = _device(P, net, model, tbl, taxa)
    ll, d = pcgb.loo_and_loglik_lg(spt)
    dense_ll = OD.loglik(net, model, tbl, taxa)
    assert abs(ll - dense_ll) <= 1e-8 * max(1.0, abs(dense_ll)), (tag, ll, dense_ll)
    dense = LR.dense_loo(net, model, tbl, taxa, tips)
    rows = _rows(pcgb, d)
    assert sorted(int(r) for r in rows) == sorted({r for r in range(len(taxa)) if any(col[r] is not None for col in tbl)})
    err = LR.worst_error(rows, d, dense, model.dimension())
    print(f"{tag}: device vs dense comparator {err:.2e} over {len(dense)} tips (tolerance 1e-8)")
    assert err <= 1e-8, tag
    assert d["total"] == LR.tree_total(d["lpd"]), tag      # the sum in family order by the fixed tree, bit for bit
    return pcgb, spt, d


# ----------------------------------------------------------------------------- 1, 2, 3: networks, models, missing values

@pytest.mark.parametrize("name,root", LR.REFERENCE)
def test_loo_reference_networks(P, name, root):
    """The networks of the reference's own tests, full BM, fixed / proper random / improper root."""
    _check(P, f"{name}/{root}", *LR.reference_case(name, root))


@pytest.mark.parametrize("which,p", LR.RANDOM)
def test_loo_random_networks(P, which, p):
    """24 tips, 6 hybrid nodes: BM at p = 1, 2, 4, heterogeneous BM with 3 colours, the univariate OU with each root."""
    _check(P, f"{which}/p{p}", *LR.random_case(which, p))


def test_loo_missing_values(P):
    """p = 3 with 30 % of the values missing: the predictions cover exactly the observed traits (NaN elsewhere: asserted by
    worst_error); exact_reml_missing: tips without any value are not tip families."""
    net, model, tbl, taxa = LR.missing_case()
    _, _, d = _check(P, "missing/p3", net, model, tbl, taxa)
    assert len(d["families"]) == len(taxa) and np.isnan(d["mean"]).any()
    z = P.loo_zscores(d)
    assert np.array_equal(np.isfinite(z), np.isfinite(d["mean"]))
    for root in ("random", "fixed"):
        net, model, tbl, taxa = LR.no_data_case(root)
        pcgb, _, d = _check(P, f"exact_reml_missing/{root}", net, model, tbl, taxa)
        assert 0 < len(d["families"]) < len(taxa)
        assert pcgb._lib.pgbp_lg_loo_count(pcgb._eng) == len(d["families"])


# ----------------------------------------------------------------------------- 4, 5: the dimension classes of the solve

def test_loo_wavefront_class_and_layouts(P):
    """A tree at p = 16: clusters of 32 variables (the wavefront class).  After the calibration the engine holds its beliefs
    in the packed BS16 layout (pgbp_layout == 1); pgbp_get_belief converts them to the plain one (pgbp_layout == 0): the
    sweep returns the same bytes on both (a packed record is read through its upper triangle, as a plain one is)."""
    from pgbp_amd import _lib as L
    net, model, tbl, taxa = LR.wavefront_case()
    pcgb, spt, packed = _check(P, "tree/p16", net, model, tbl, taxa)
    assert 17 <= int(pcgb._dims[: pcgb.nclusters].max()) <= 64
    lib, eng = pcgb._lib, pcgb._eng
    assert lib.pgbp_layout(eng) == 1, "the p = 16 tree is expected in the packed layout after a calibration"
    rec = np.zeros(int(pcgb._dims[0]) ** 2 + int(pcgb._dims[0]) + 1)
    assert lib.pgbp_get_belief(eng, 0, 0, L.f64p(rec)) == L.PGBP_OK
    assert lib.pgbp_layout(eng) == 0
    plain = pcgb.loo_lg()
    for k in ("mean", "cov", "lpd", "info"):
        assert packed[k].tobytes() == plain[k].tobytes(), k
    assert packed["total"] == plain["total"]


def _muller(P, p):
    """The clique tree of the Mueller et al. (2022) network (tests/golden/muller_2022.phy), fixed root, BM data simulated on
    the network (the setup of test_gpu_gradient._muller, with the family table and the tips' node indices kept)."""
    from helpers import HERE, network_from_newick_file
    net, names, onet, _ = network_from_newick_file(P, os.path.join(HERE, "golden", "muller_2022.phy"))
    tipnodes = [i for i in range(net.nnodes) if net.is_leaf[i]]
    cn, ed, sn = P.cliquetree(net.node2family)
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
    tips = [names[i] for i in tipnodes]
    tbl = [[float(X[i, k]) for i in tipnodes] for k in range(p)]
    return cgb, spt, st, fam, X, R, mu, onet, OM.MvFullBrownianMotion(R, mu), tbl, tips, tipnodes


def test_loo_workgroup_class_muller_2_traits(P):
    """The Mueller clique tree at 2 traits: beliefs of up to 108 variables (the workgroup class, 65 .. 128).  Every tip against
    the restatement (b) on the device's own pgbp_moments of the calibrated clusters, a sample of 10 tips against the dense
    comparator (a), both at 1e-8."""
    cgb, spt, st, fam, X, R, mu, onet, model, tbl, tips, tipnodes = _muller(P, 2)
    assert 64 < int(st.dims.max()) <= 128
    ll, d = cgb.loo_and_loglik_lg(spt)
    assert not d["info"].any() and len(d["families"]) == len(tips)
    mom = cgb.moments_()
    want = LR.loo_sweep(fam, X, R[None], mu, lambda c: (mom[c][0], mom[c][1]))
    assert np.array_equal(want["families"], d["families"])
    errs = [LR.rel_block(d[k][i], want[k][i]) for k in ("mean", "cov") for i in range(len(tips))]
    errs += list(np.abs(d["lpd"] - want["lpd"]) / np.maximum(np.abs(want["lpd"]), 1.0))
    print(f"Mueller, 2 traits ({int(st.dims.max())} variables): device vs restatement {max(errs):.2e} over {len(tips)} tips")
    assert max(errs) <= 1e-8
    assert d["total"] == LR.tree_total(d["lpd"])
    row_of_node = {n: r for r, n in enumerate(tipnodes)}
    rows = np.array([row_of_node[int(n)] for n in cgb._lg["data_row"][d["families"]]])
    sample = [int(r) for r in np.random.default_rng(0).choice(len(tips), 10, replace=False)]
    err = LR.worst_error(rows, d, LR.dense_loo(onet, model, tbl, tips, sample), 2)
    print(f"Mueller, 2 traits: device vs dense comparator {err:.2e} over 10 tips")
    assert err <= 1e-8


# ----------------------------------------------------------------------------- 6: refusals

def test_loo_refuses_clusters_above_128_variables(P):
    """The Mueller clique tree at 3 traits has tip families in clusters of more than 128 variables: PGBP_ERR_INVALID before
    any launch, the family and its cluster named, the outputs untouched."""
    from pgbp_amd import _lib as L
    cgb, spt, st, *_ = _muller(P, 3)
    assert int(st.dims.max()) > 128
    nt = cgb._lib.pgbp_lg_loo_count(cgb._eng)
    lpd, total = np.full(nt, 7.0), np.full(1, 7.0)
    rc = cgb._lib.pgbp_lg_loo(cgb._eng, 0, 1, None, None, L.f64p(lpd), L.f64p(total), None)
    msg = cgb._lib.pgbp_last_error(cgb._eng)
    assert rc == L.ERR_INVALID and b"more than 128 variables" in msg and b"family" in msg and b"cluster" in msg
    assert np.all(lpd == 7.0) and total[0] == 7.0
    with pytest.raises(L.PgbpError):
        cgb.loo_lg()


def test_loo_refuses_what_does_not_fit_the_lds(P):
    """p = 64 on a tree: clusters of 128 variables (133 KB of working matrix) plus the p x p scratch exceed the 160 KB of
    LDS: PGBP_ERR_INVALID before any launch."""
    from pgbp_amd import _lib as L
    rng = np.random.default_rng(8)
    tree = ON.random_network(5, 0, rng)
    tbl = [list(rng.normal(size=5)) for _ in range(64)]
    _, _, pcgb, spt = _device(P, tree, LR.bm(64, rng, "random"), tbl, tree.tip_names)
    with pytest.raises(L.PgbpError) as ex:
        pcgb.loo_lg()
    assert ex.value.code == L.ERR_INVALID and "bytes of LDS" in ex.value.msg


def _tree_batch(P, p, fixedroot=True):
    nwk, taxa, data, Rs, mus = LR.batch_case(p)
    net, names = P.read_newick(nwk)
    row = {t: r for r, t in enumerate(taxa)}
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=fixedroot)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], p)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))

    def engine(sites, assign=True, setup=True):
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=len(sites))
        if setup:
            cgb.lg_setup(fam, data[sites])
        if assign:
            cgb.assignfactors_lg_(Rs[sites][:, None], mus[sites])
        return cgb
    return engine, spt, fam, taxa, data, Rs, mus


def test_loo_state_and_argument_refusals(P):
    """No family table, no parameters yet: PGBP_ERR_STATE; a bad site range, lpd NULL: PGBP_ERR_INVALID."""
    from pgbp_amd import _lib as L
    engine, spt, fam, taxa, data, Rs, mus = _tree_batch(P, 2)
    sites = np.arange(3)
    lpd = np.zeros((3, len(taxa)))
    bare = engine(sites, assign=False, setup=False)
    assert bare._lib.pgbp_lg_loo(bare._eng, 0, 3, None, None, L.f64p(lpd), None, None) == L.ERR_STATE
    assert b"pgbp_lg_setup" in bare._lib.pgbp_last_error(bare._eng)
    assert bare._lib.pgbp_lg_loo_count(bare._eng) == -1
    table = engine(sites, assign=False)
    assert table._lib.pgbp_lg_loo_count(table._eng) == len(taxa)
    assert table._lib.pgbp_lg_loo(table._eng, 0, 3, None, None, L.f64p(lpd), None, None) == L.ERR_STATE
    assert b"pgbp_lg_assignfactors" in table._lib.pgbp_last_error(table._eng)
    cgb = engine(sites)
    lib, eng = cgb._lib, cgb._eng
    for s0, s1 in ((0, 4), (-1, 2), (2, 1)):
        assert lib.pgbp_lg_loo(eng, s0, s1, None, None, L.f64p(lpd), None, None) == L.ERR_INVALID
    assert lib.pgbp_lg_loo(eng, 0, 3, None, None, None, None, None) == L.ERR_INVALID
    assert b"lpd" in lib.pgbp_last_error(eng)
    assert not lpd.any()
    assert lib.pgbp_lg_loo(eng, 1, 1, None, None, L.f64p(lpd), None, None) == L.PGBP_OK and not lpd.any()   # an empty range


# ----------------------------------------------------------------------------- 7: a batch

@pytest.mark.parametrize("p", [1, 2])
def test_loo_batch_of_64_sites(P, p):
    """64 sites with their own data and parameters on a 40-tip tree (p = 1: the site-minor univariate layout, converted to
    the plain one by the call).  Every site against the restatement (b) on the device's pgbp_moments; sites 0, 31 and 63
    against the dense comparator (a); two calls return the same bytes; a site range equals the slice of the full call;
    two chunks of sites (pgbp_loo_scratch_limit) change nothing."""
    from pgbp_amd import _lib as L
    engine, spt, fam, taxa, data, Rs, mus = _tree_batch(P, p)
    cgb = engine(np.arange(64))
    ll, d = cgb.loo_and_loglik_lg(spt, all_sites=True)
    assert not d["info"].any() and d["lpd"].shape == (64, 40)
    again = cgb.loo_lg(all_sites=True)
    keys = ("mean", "cov", "lpd", "total", "info")
    for k in keys:
        assert d[k].tobytes() == again[k].tobytes(), k
    mom = cgb.moments_(all_sites=True)
    worst = 0.0
    for s in range(64):
        want = LR.loo_sweep(fam, data[s], Rs[s][None], mus[s], lambda c: (mom[c][0][s], mom[c][1][s]))
        for k in ("mean", "cov"):
            worst = max([worst] + [LR.rel_block(d[k][s][i], want[k][i]) for i in range(40)])
        worst = max(worst, float(np.max(np.abs(d["lpd"][s] - want["lpd"]) / np.maximum(np.abs(want["lpd"]), 1.0))))
        assert d["total"][s] == LR.tree_total(d["lpd"][s])
    print(f"batch p={p}: device vs restatement, worst over 64 sites {worst:.2e}")
    assert worst <= 1e-8
    rows = _rows(cgb, d)
    for s in (0, 31, 63):
        onet, model, tbl, _ = LR.batch_site(p, s)
        one = {k: d[k][s] for k in keys}
        err = LR.worst_error(rows, one, LR.dense_loo(onet, model, tbl, taxa), p)
        dense_ll = OD.loglik(onet, model, tbl, taxa)
        print(f"batch p={p} site {s}: device vs dense comparator {err:.2e}")
        assert err <= 1e-8 and abs(ll[s] - dense_ll) <= 1e-8 * abs(dense_ll)
    # a site range
    n = 7
    mean = np.zeros((n, 40, p)); cov = np.zeros((n, 40, p, p)); lpd = np.zeros((n, 40)); tot = np.zeros(n)
    info = np.ones((n, 40), np.int32)
    rc = cgb._lib.pgbp_lg_loo(cgb._eng, 20, 27, L.f64p(mean), L.f64p(cov), L.f64p(lpd), L.f64p(tot), L.i32p(info))
    assert rc == L.PGBP_OK and not info.any()
    assert np.array_equal(mean, d["mean"][20:27]) and np.array_equal(cov.transpose(0, 1, 3, 2), d["cov"][20:27])
    assert np.array_equal(lpd, d["lpd"][20:27]) and np.array_equal(tot, d["total"][20:27])
    # two chunks of sites
    per_site = 40 * (1 + p + p * p)
    cgb._lib.pgbp_loo_scratch_limit(per_site * 33)
    try:
        cut = cgb.loo_lg(all_sites=True)
    finally:
        cgb._lib.pgbp_loo_scratch_limit(0)
    for k in keys:
        assert d[k].tobytes() == cut[k].tobytes(), k


# ----------------------------------------------------------------------------- 8, 9: info, consistency

def test_loo_info_of_a_bad_site_and_of_an_undetermined_prediction(P):
    """A site whose rate matrix is not positive definite: its tips are NaN with info != 0, its total NaN, the neighbouring
    sites are the same bytes as without it.  Two tips under an improper root: with complete data the other tip determines
    the root and the prediction is proper (against the dense comparator); observed at disjoint traits, the other tip leaves
    the root's matching trait flat and D = V - S is singular for each tip: info == 1, NaN, no error."""
    engine, spt, fam, taxa, data, Rs, mus = _tree_batch(P, 2)
    sites = np.arange(3)
    cgb = engine(sites)
    _, good = cgb.loo_and_loglik_lg(spt, all_sites=True)
    assert not good["info"].any()
    bad = Rs[sites].copy()
    bad[1] = np.array([[1.0, 2.0], [2.0, 1.0]])
    cgb.assignfactors_lg_(bad[:, None], mus[sites])
    ll, got = cgb.loo_and_loglik_lg(spt, all_sites=True)
    assert np.all(got["info"][1] != 0) and not got["info"][0].any() and not got["info"][2].any()
    assert np.isnan(got["mean"][1]).all() and np.isnan(got["cov"][1]).all() and np.isnan(got["lpd"][1]).all()
    assert np.isnan(got["total"][1])
    for s in (0, 2):
        for k in ("mean", "cov", "lpd", "total"):
            assert good[k][s].tobytes() == got[k][s].tobytes(), (s, k)
    _check(P, "two tips, complete", *LR.two_tip_complete_case())
    net, model, tbl, taxa2 = LR.two_tip_case()
    _, _, pcgb, spt2 = _device(P, net, model, tbl, taxa2)
    ll2, d = pcgb.loo_and_loglik_lg(spt2)
    assert len(d["families"]) == 2 and np.all(d["info"] == 1)
    assert np.isnan(d["lpd"]).all() and np.isnan(d["mean"]).all() and np.isnan(d["cov"]).all() and np.isnan(d["total"])


def test_loo_total_is_the_loglikelihood_on_a_star_tree(P):
    """sum_f lpd is not the log-likelihood in general (asserted on a random network); on a star tree with a fixed root the
    tips are independent, every S = 0 and total == loglik to 1e-12."""
    net, model, tbl, taxa = LR.star_case()
    pcgb, spt, d = _check(P, "star", net, model, tbl, taxa)
    ll = OD.loglik(net, model, tbl, taxa)
    print(f"star tree: total {d['total']!r}, loglik {ll!r}")
    assert abs(d["total"] - ll) <= 1e-12 * abs(ll)
    net, model, tbl, taxa = LR.random_case("bm_random", 4)
    _, _, pcgb, spt = _device(P, net, model, tbl, taxa)
    ll, d = pcgb.loo_and_loglik_lg(spt)
    assert abs(d["total"] - ll) > 1e-3 * abs(ll)

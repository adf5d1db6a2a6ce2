"""pgbp_lg_edge_gradient / ClusterGraphBelief.edge_gradient_lg: the derivative of the log-likelihood in every edge length, in
every inheritance and in a mean shift on every edge, one sweep over the node families on the device; pgbp_lg_set_edges /
set_edges_lg: new lengths and inheritances without a new set-up.

Comparators, as in test_gpu_gradient.py: (a) the numpy statement edge_ref.family_edge_gradient on the DENSE oracle's posterior
moments (itself pinned to finite differences of densemvn.loglik in test_edge_gradient_cpu.py), asserted at 1e-8 relative to
the largest entry of each block (dlength, dgamma, dshift) for fixed and proper roots; (b) for an improper root, Richardson
central differences of densemvn.loglik with two step pairs (1e-3 / 5e-4 and 2e-3 / 1e-3): their disagreement is the
comparator's uncertainty, the assertion is at max(10 x that, 1e-8), and the figures are printed."""
import zlib

import numpy as np
import pytest

from edge_ref import dense_edge_gradient, fd_edge_gradient, rel_block_nan
from helpers import goldens, make_model
from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from test_gpu_gradient import _bm, _device, _golden_cases, _is_proper, _muller
from test_gradient_cpu import model_params, richardson

pytestmark = pytest.mark.gpu
G = goldens()
BLOCKS = ("dlength", "dgamma", "dshift")


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


# ----------------------------------------------------------------------------- the reference in the device's layout

def _oracle_order(net, ocgb):
    """node -> its parent edges in the order of the family table lg_inputs_from_oracle builds (node2family)."""
    pre = net.vec_node
    return lambda i: [next(e for e in pre[p1 - 1].edges if e.child is pre[i]) for p1 in ocgb.node2family[i][1:]]


def _number_order(net):
    """the same for a table built from plain network arrays (network_from_newick_file, read_newick): edge-number order."""
    pre = net.vec_node
    return lambda i: sorted((e for e in pre[i].edges if e.child is pre[i]), key=lambda e: e.number)


def _device_layout(ref, order, root_family):
    """The arrays of family_edge_gradient / fd_edge_gradient (rows = nodes in preorder, columns = net.parent_edges order) as
    the device returns them: rows = families (the root's only when it has a prior factor), columns = the table's order."""
    N, K = ref["dlength"].shape
    rows = list(range(0 if root_family else 1, N))
    out = {k: np.full((len(rows), K), np.nan) for k in ("dlength", "dgamma")}
    out["dshift"] = ref["dshift"][rows].copy()
    for f, i in enumerate(rows):
        for k, ed in enumerate(order(i)):
            kk = next(q for q, e2 in enumerate(ref["edges"][i]) if e2 is ed)
            out["dlength"][f, k] = ref["dlength"][i, kk]
            out["dgamma"][f, k] = ref["dgamma"][i, kk]
    return out


def _assert_blocks(tag, got, want, tol):
    worst = 0.0
    for k in BLOCKS:
        err = rel_block_nan(got[k], want[k])
        worst = max(worst, err)
        print(f"{tag} {k}: {err:.2e} (tolerance {tol:.1e})")
        assert err <= tol, (tag, k, got[k], want[k])
    return worst


def _reference(tag, net, model, tbl, taxa, order):
    """(reference in the device's layout, tolerance): the dense statement, or finite differences with their uncertainty."""
    root_family = model_params(model)[1] is not None
    if _is_proper(model):
        return _device_layout(dense_edge_gradient(net, model, tbl, taxa), order, root_family), 1e-8
    a, b = (_device_layout(fd, order, root_family) for fd in fd_edge_gradient(net, model, tbl, taxa, steps=(1e-3, 2e-3)))
    unc = max(rel_block_nan(b[k], a[k]) for k in BLOCKS)
    print(f"{tag}: finite-difference comparator uncertainty {unc:.2e}")
    return a, max(10 * unc, 1e-8)


def _check_against_oracle(P, tag, net, model, tbl, taxa):
    cg, ocgb, pcgb, spt = _device(P, net, model, tbl, taxa)
    ll, got = pcgb.loglik_and_edge_gradient_lg(spt)
    dense = OD.loglik(net, model, tbl, taxa)
    assert abs(ll - dense) <= 1e-8 * max(1.0, abs(dense)), (tag, ll, dense)
    want, tol = _reference(tag, net, model, tbl, taxa, _oracle_order(net, ocgb))
    _assert_blocks(tag, got, want, tol)
    return pcgb, spt, got


# ----------------------------------------------------------------------------- 1: the reference's networks

@pytest.mark.parametrize("root", ["fixed", "random", "improper"])
@pytest.mark.parametrize("case", list(_golden_cases()), ids=lambda c: c[0])
def test_edge_gradient_reference_networks(P, case, root):
    """The networks of the reference's own tests, full BM with a fixed, a proper random and an improper root."""
    name, netstr, taxa, cols = case
    net = ON.read_newick(netstr)
    rng = np.random.default_rng(11)
    tbl = [[None if v is None else float(v) for v in col] for col in cols]
    _check_against_oracle(P, f"{name}/{root}", net, _bm(len(cols), rng, root), tbl, taxa)


# ----------------------------------------------------------------------------- 2: random networks, every model

@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("root", ["fixed", "random", "improper"])
@pytest.mark.parametrize("kind,p", [("bm", 1), ("bm", 2), ("bm", 4), ("hetero", 2), ("ou", 1)])
def test_edge_gradient_random_networks(P, kind, p, root, seed):
    """24 tips, 6 hybrid nodes: homogeneous BM (p = 1, 2, 4), heterogeneous BM with 3 colours, the univariate OU, each with a
    fixed / random / improper root.  A hybrid family fills both of its K = 2 entries, a tree family has NaN at k = 1."""
    rng = np.random.default_rng(zlib.crc32(f"edge-{kind}-{p}-{root}-{seed}".encode()))
    net = ON.random_network(24, 6, rng)
    taxa = net.tip_names
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
    pcgb, spt, got = _check_against_oracle(P, f"{kind}/p{p}/{root}/s{seed}", net, model, tbl, taxa)
    n_par = pcgb._lg["n_parents"]
    assert got["dlength"].shape == (len(n_par), 2) and got["dshift"].shape == (len(n_par), p)
    assert int(np.sum(n_par == 2)) == 6
    for name in ("dlength", "dgamma"):
        assert np.isfinite(got[name][n_par == 2]).all()
        assert np.isfinite(got[name][n_par == 1, 0]).all() and np.isnan(got[name][n_par == 1, 1]).all()
        assert np.isnan(got[name][n_par == 0]).all()
    assert np.isfinite(got["dshift"]).all()
    assert int(np.sum(n_par == 0)) == (1 if root == "random" else 0)


# ----------------------------------------------------------------------------- 3: missing tip values (scope masks)

def test_edge_gradient_missing_values(P):
    """The cases of test_gradient_missing_values: calibration_tree_2traits_missing (y2 observed at one tip only),
    exact_reml_missing (a subtree without data: its families are skipped and write zeros, not NaN) and a random pattern on a
    random network."""
    g = G["calibration_tree_2traits_missing"]
    _check_against_oracle(P, "tree_2traits_missing", ON.read_newick(g["net"]), make_model(g["model"]), [g["y1"], g["y2"]],
                          g["taxa"])
    g = G["exact_reml_missing"]
    for root in ("random", "improper"):
        pcgb, _, got = _check_against_oracle(P, f"exact_reml_missing/{root}", ON.read_newick(g["net"]),
                                             _bm(1, np.random.default_rng(3), root), [g["x"]], g["taxa"])
        skipped = pcgb._lg["child_mask"] == 0
        assert skipped.any()
        n_par = pcgb._lg["n_parents"]
        for f in np.nonzero(skipped)[0]:
            assert np.all(got["dlength"][f, :n_par[f]] == 0.0) and np.all(got["dgamma"][f, :n_par[f]] == 0.0)
            assert np.all(got["dshift"][f] == 0.0)
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

def test_edge_gradient_wavefront_class_and_layouts(P):
    """A tree with p = 16: clusters of 32 variables (the 64-thread class) against the dense statement.  After the
    calibration the engine holds its beliefs in the packed BS16 layout; the sweep on the SAME beliefs converted to the plain
    layout gives the same values at 1e-12 relative to the largest entry of a block (not the same bytes, for the reason given in
    test_gradient_wavefront_class_and_layouts); the measured figure is printed."""
    from pgbp_amd import _lib as L
    rng = np.random.default_rng(5)
    tree = ON.random_network(12, 0, rng)
    assert max(len(nodes) for _, nodes in OCG.cliquetree(tree).clusters) * 16 == 32
    tbl = [list(rng.normal(size=12)) for _ in range(16)]
    pcgb, spt, _ = _check_against_oracle(P, "tree/p16", tree, _bm(16, rng, "random"), tbl, tree.tip_names)
    lib, eng = pcgb._lib, pcgb._eng
    assert lib.pgbp_layout(eng) == 1, "the p = 16 tree is expected in the packed layout after a calibration"
    packed = pcgb.edge_gradient_lg()
    rec = np.zeros(int(pcgb._dims[0]) ** 2 + int(pcgb._dims[0]) + 1)
    assert lib.pgbp_get_belief(eng, 0, 0, L.f64p(rec)) == L.PGBP_OK
    assert lib.pgbp_layout(eng) == 0
    plain = pcgb.edge_gradient_lg()
    for k in BLOCKS:
        err = rel_block_nan(packed[k], plain[k])
        print(f"packed vs plain layout, {k}: {err:.2e}")
        assert err <= 1e-12, k


def test_edge_gradient_workgroup_class_muller_2_traits(P):
    """The Mueller clique tree at 2 traits: beliefs of up to 108 variables (the 256-thread class), 361 hybrid families;
    log-likelihood and every block against the dense statement at 1e-8."""
    cgb, spt, st, onet, model, tbl, tips = _muller(P, 2)
    assert 64 < int(st.dims.max()) <= 128
    ll, got = cgb.loglik_and_edge_gradient_lg(spt)
    dense = OD.loglik(onet, model, tbl, tips)
    assert abs(ll - dense) <= 1e-8 * abs(dense), (ll, dense)
    want = _device_layout(dense_edge_gradient(onet, model, tbl, tips), _number_order(onet), False)
    _assert_blocks("muller/p2", got, want, 1e-8)
    n_par = cgb._lg["n_parents"]
    assert int(np.sum(n_par == 2)) == 361 and _same(np.isfinite(got["dgamma"][:, 1]), n_par == 2)


def test_edge_gradient_refuses_clusters_above_128_variables(P):
    """The Mueller clique tree at 3 traits has beliefs of more than 128 variables: PGBP_ERR_INVALID before any launch, the
    family and its cluster named."""
    from pgbp_amd import _lib as L
    cgb, spt, st, *_ = _muller(P, 3)
    assert int(st.dims.max()) > 128
    assert P.calibrate_(cgb, [spt])[0]
    with pytest.raises(L.PgbpError) as ex:
        cgb.edge_gradient_lg()
    assert ex.value.code == L.ERR_INVALID and "more than 128 variables" in ex.value.msg and "family" in ex.value.msg
    assert "cluster" in ex.value.msg and "pgbp_lg_edge_gradient" in ex.value.msg


def test_edge_gradient_refuses_what_does_not_fit_the_lds(P):
    """p = 64 on a tree: clusters of 128 variables (133 KB of working matrix) plus the family's scratch exceed the 160 KB of
    LDS: PGBP_ERR_INVALID before any launch."""
    from pgbp_amd import _lib as L
    rng = np.random.default_rng(8)
    tree = ON.random_network(5, 0, rng)
    tbl = [list(rng.normal(size=5)) for _ in range(64)]
    _, _, pcgb, spt = _device(P, tree, _bm(64, rng, "random"), tbl, tree.tip_names)
    with pytest.raises(L.PgbpError) as ex:
        pcgb.edge_gradient_lg()
    assert ex.value.code == L.ERR_INVALID and "bytes of LDS" in ex.value.msg


# ----------------------------------------------------------------------------- 5: batches, determinism, NULL outputs, info

def _tree_problem(P, ntips, n_sites, p, seed, fixedroot=True):
    """A random tree's clique tree with its family table, tip data and per-site parameters; engine(sites, fam) builds an
    engine of those sites on a (possibly edited) table."""
    from test_gpu_exact_bm import _random_tree
    S, rng, tr, nwk, taxa = _random_tree(ntips, seed)
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

    def engine(sites, table=fam):
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=len(sites))
        cgb.lg_setup(table, data[sites])
        cgb.assignfactors_lg_(Rs[sites][:, None], mus[sites])
        return cgb
    onet = ON.read_newick(nwk)
    onet.set_preorder(names)
    return dict(engine=engine, fam=fam, spt=spt, onet=onet, taxa=taxa, data=data, Rs=Rs, mus=mus, rng=rng)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("p", [1, 2])
def test_edge_gradient_batch_of_64_sites(P, p):
    """64 sites with their own data and parameters equal 64 one-site engines: p = 2 the same bytes, p = 1 at 1e-12 (the batch
    is filled and calibrated by the thread-per-site kernels of the site-minor layout, the one-site engine by the wavefront
    kernels: test_gradient_batch_of_64_sites).  Sites 0 and 63 equal the dense statement; a site range returns the rows of the
    full call; two calls return identical bytes; each output NULL in turn leaves the other two unchanged."""
    from pgbp_amd import _lib as L
    T = _tree_problem(P, 20, 64, p, 40 + p)
    cgb = T["engine"](np.arange(64))
    ll, got = cgb.loglik_and_edge_gradient_lg(T["spt"], all_sites=True)
    assert not got["info"].any()
    again = cgb.edge_gradient_lg(all_sites=True)
    for k in BLOCKS:
        assert _same(got[k], again[k]), k
    for s in range(64):
        one = T["engine"](np.array([s]))
        ll1, g1 = one.loglik_and_edge_gradient_lg(T["spt"], all_sites=True)
        for k in BLOCKS:
            if p == 2:
                assert _same(got[k][s], g1[k][0]), (s, k)
            else:
                assert rel_block_nan(got[k][s], g1[k][0]) <= 1e-12, (s, k)
        assert abs(ll[s] - ll1[0]) <= 1e-12 * abs(ll1[0])
    for s in (0, 63):
        model = OM.MvFullBrownianMotion(T["Rs"][s], T["mus"][s])
        tbl = [list(T["data"][s][:, t]) for t in range(p)]
        want = _device_layout(dense_edge_gradient(T["onet"], model, tbl, T["taxa"]), _number_order(T["onet"]), False)
        _assert_blocks(f"site {s}", {k: got[k][s] for k in BLOCKS}, want, 1e-8)
    nf, K = got["dlength"].shape[1:]
    lib, eng = cgb._lib, cgb._eng

    def call(s0, s1, which):
        n = s1 - s0
        out = dict(dlength=np.full((n, nf, K), 7.0), dgamma=np.full((n, nf, K), 7.0), dshift=np.full((n, nf, p), 7.0))
        info = np.ones(n, np.int32)
        args = [L.f64p(out[k]) if k in which else None for k in BLOCKS]
        assert lib.pgbp_lg_edge_gradient(eng, s0, s1, *args, L.i32p(info)) == L.PGBP_OK and not info.any()
        return out
    rows = call(20, 27, BLOCKS)
    for k in BLOCKS:
        assert _same(rows[k], got[k][20:27]), k
    for left_out in BLOCKS:
        out = call(0, 64, [k for k in BLOCKS if k != left_out])
        for k in BLOCKS:
            assert _same(out[k], got[k]) if k != left_out else np.all(out[k] == 7.0), (left_out, k)


def test_edge_gradient_info_of_one_bad_site(P):
    """A site whose rate matrix is not positive definite reports info and NaN everywhere; its neighbours hold the bytes of a
    clean run."""
    T = _tree_problem(P, 20, 3, 2, 50)
    cgb = T["engine"](np.arange(3))
    good_ll, good = cgb.loglik_and_edge_gradient_lg(T["spt"], all_sites=True)
    assert not good["info"].any()
    bad = T["Rs"].copy()
    bad[1] = np.array([[1.0, 2.0], [2.0, 1.0]])
    cgb.assignfactors_lg_(bad[:, None], T["mus"])
    ll, got = cgb.loglik_and_edge_gradient_lg(T["spt"], all_sites=True)
    assert got["info"][1] != 0 and got["info"][0] == 0 and got["info"][2] == 0 and np.isnan(ll[1])
    for k in BLOCKS:
        assert np.isnan(got[k][1]).all(), k
        for s in (0, 2):
            assert _same(got[k][s], good[k][s]), (s, k)
    cgb.site = 1
    with pytest.raises(np.linalg.LinAlgError):
        cgb.edge_gradient_lg()


# ----------------------------------------------------------------------------- 6: state errors

def test_edge_gradient_and_set_edges_state_errors(P):
    """No family table / no parameters: PGBP_ERR_STATE with the missing call named; a site range out of bounds and all three
    outputs NULL: PGBP_ERR_INVALID."""
    from pgbp_amd import _lib as L
    from test_gpu_exact_bm import _random_tree
    S, rng, tr, nwk, taxa = _random_tree(8, 3)
    net, names = P.read_newick(nwk)
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, 1)
    fresh = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    lib, eng = fresh._lib, fresh._eng
    row = {t: r for r, t in enumerate(taxa)}
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], 1)
    nf = len(fam["cluster"])
    bufs = [np.zeros((nf, 1)) for _ in range(3)]
    args = [L.f64p(b) for b in bufs] + [None]
    assert lib.pgbp_lg_edge_gradient(eng, 0, 1, *args) == L.ERR_STATE
    assert b"pgbp_lg_setup" in lib.pgbp_last_error(eng)
    assert lib.pgbp_lg_set_edges(eng, L.f64p(np.ones(nf)), None) == L.ERR_STATE
    assert b"pgbp_lg_setup" in lib.pgbp_last_error(eng)
    fresh.lg_setup(fam, rng.normal(size=(len(taxa), 1)))
    assert lib.pgbp_lg_edge_gradient(eng, 0, 1, *args) == L.ERR_STATE
    assert b"pgbp_lg_assignfactors" in lib.pgbp_last_error(eng)
    fresh.assignfactors_lg_(np.array([[[1.0]]]), [0.0])
    assert lib.pgbp_lg_edge_gradient(eng, 0, 1, None, None, None, None) == L.ERR_INVALID
    assert b"no output buffer" in lib.pgbp_last_error(eng)
    for s0, s1 in ((0, 2), (-1, 1), (1, 0)):
        assert lib.pgbp_lg_edge_gradient(eng, s0, s1, *args) == L.ERR_INVALID
        assert b"site range" in lib.pgbp_last_error(eng)


# ----------------------------------------------------------------------------- 7: pgbp_lg_set_edges

def _all_beliefs(cgb):
    from pgbp_amd import _lib as L
    buf = np.zeros((cgb.n_sites, int(cgb._poff[-1])))
    assert cgb._lib.pgbp_get_beliefs(cgb._eng, L.f64p(buf)) == L.PGBP_OK
    return buf


def _assert_set_edges_equals_fresh_setup(P, old, fresh_with, fam, spt, assign, rng):
    """`old`: an engine set up with `fam` and assigned; fresh_with(table): a new engine on an edited table, assigned."""
    from pgbp_amd import _lib as L
    real = np.arange(fam["length"].size) % fam["max_parents"] < np.repeat(fam["n_parents"], fam["max_parents"])
    length = fam["length"] * np.where(real, rng.uniform(0.7, 1.4, fam["length"].size), 1.0)
    gamma = fam["gamma"] * np.where(real, rng.uniform(0.8, 1.1, fam["gamma"].size), 1.0)
    def fresh(table):
        cgb = fresh_with(table)
        cgb._ensure_schedule([spt])   # (loglik_lg walks the postorder of schedule tree 0)
        return cgb
    old._ensure_schedule([spt])
    before = old.loglik_lg()[0].copy()
    old.set_edges_lg(length=length, gamma=gamma)
    new = fresh(dict(fam, length=length, gamma=gamma))
    ll_old, ll_new = old.loglik_lg()[0], new.loglik_lg()[0]
    assert np.array_equal(ll_old, ll_new) and not np.array_equal(ll_old, before)
    assign(old)
    for cgb in (old, new):
        cgb.loglik_and_edge_gradient_lg(spt, all_sites=True)
    assert np.array_equal(_all_beliefs(old), _all_beliefs(new))
    # a length that is zero or NaN: refused, nothing changed (a valid gamma in the same call included)
    f = int(np.nonzero(fam["n_parents"] > 0)[0][-1]) * fam["max_parents"]
    for bad_value in (0.0, np.nan):
        bad = length.copy()
        bad[f] = bad_value
        with pytest.raises(L.PgbpError) as ex:
            old.set_edges_lg(length=bad, gamma=fam["gamma"])
        assert ex.value.code == L.ERR_INVALID and "length" in ex.value.msg
        assert np.array_equal(old.loglik_lg()[0], ll_new)
    # one of the two only
    old.set_edges_lg(gamma=fam["gamma"])
    assert np.array_equal(old.loglik_lg()[0], fresh(dict(fam, length=length)).loglik_lg()[0])


@pytest.mark.parametrize("which", ["tree_batch", "univariate_batch"])
def test_set_edges_equals_a_fresh_setup_on_tree_batches(P, which):
    """A 20-tip tree: 3 sites of 2 traits (the plain layout) and 64 univariate sites (the site-minor layout: the
    thread-per-site fill and its per-cluster records).  After set_edges_lg with perturbed lengths and inheritances, loglik_lg
    and every calibrated belief are the bytes of a fresh engine set up with the perturbed table."""
    n_sites, p = (3, 2) if which == "tree_batch" else (64, 1)
    T = _tree_problem(P, 20, n_sites, p, 60 + p)
    sites = np.arange(n_sites)
    old = T["engine"](sites)
    _assert_set_edges_equals_fresh_setup(P, old, lambda table: T["engine"](sites, table), T["fam"], T["spt"],
                                         lambda cgb: cgb.assignfactors_lg_(T["Rs"][:, None], T["mus"]), T["rng"])
    assert bool(old._lib.pgbp_layout(old._eng) & 2) == (which == "univariate_batch")   # (loglik_lg ran last: its own layout)


def test_set_edges_equals_a_fresh_setup_on_a_network(P):
    """The same on a random network of 24 tips and 6 hybrid nodes (K = 2), heterogeneous BM with a random root."""
    from helpers import lg_inputs_from_oracle, oracle_setup, product_beliefs_from_oracle
    rng = np.random.default_rng(71)
    net = ON.random_network(24, 6, rng)
    taxa = net.tip_names
    base = _bm(2, rng, "random")
    colors = {e.number: 1 + int(rng.integers(3)) for e in net.edges}
    model = OM.HeterogeneousBrownianMotion([base.R * s for s in (0.5, 1.0, 2.5)], colors, base.mu, base.v)
    tbl = [list(rng.normal(size=len(taxa))) for _ in range(2)]
    cg, ocgb, pcgb, spt = _device(P, net, model, tbl, taxa)
    fam, data, kw = lg_inputs_from_oracle(P, net, ocgb, model, tbl, taxa)

    def fresh_with(table):
        pb = product_beliefs_from_oracle(oracle_setup(net, cg, model, tbl, taxa).belief)
        for b in pb:
            b.J[...] = 0.0
            b.h[...] = 0.0
            b.g[...] = 0.0
        new = P.ClusterGraphBelief(pb, ocgb.node2cluster, ocgb.node2family, ocgb.node2fixed, ocgb.cluster2nodes)
        new.lg_setup(table, data)
        new.assignfactors_lg_(**kw)
        return new
    _assert_set_edges_equals_fresh_setup(P, pcgb, fresh_with, fam, spt, lambda cgb: cgb.assignfactors_lg_(**kw), rng)


# ----------------------------------------------------------------------------- 8: beyond the dense oracle's reach

def test_edge_gradient_directional_derivative_on_2000_tips(P):
    """A 2 000-tip random tree, 4 traits, fixed root, one site: for one seeded random direction d over all edge lengths, the
    Richardson central difference of the device's own loglik_lg through set_edges_lg(length (1 + h d)) -- the existing
    likelihood path is the comparator -- against sum dlength (length d).  Two step pairs (1e-3 / 5e-4, 2e-3 / 1e-3), asserted
    at max(10 x their disagreement, 1e-8) relative; the figures are printed."""
    T = _tree_problem(P, 2000, 1, 4, 80)
    cgb = T["engine"](np.arange(1))
    ll, got = cgb.loglik_and_edge_gradient_lg(T["spt"])
    length = T["fam"]["length"].copy()
    assert got["dlength"].shape == (len(length), 1) and np.isfinite(got["dlength"]).all()
    d = np.random.default_rng(81).normal(size=len(length))
    have = float(np.sum(got["dlength"][:, 0] * length * d))

    def f(h):
        cgb.set_edges_lg(length=length * (1.0 + h * d))
        return float(cgb.loglik_lg()[0][0])
    a, b = richardson(f, 1e-3), richardson(f, 2e-3)
    cgb.set_edges_lg(length=length)
    assert float(cgb.loglik_lg()[0][0]) == pytest.approx(ll, rel=1e-12)
    unc = abs(a - b) / abs(a)
    err = abs(have - a) / abs(a)
    print(f"2000 tips: sweep {have:.10e}, finite differences {a:.10e}, comparator uncertainty {unc:.2e}, error {err:.2e}")
    assert err <= max(10 * unc, 1e-8)

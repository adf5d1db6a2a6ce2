"""pgbp_lg_gradient_sites / ClusterGraphBelief.gradient_sites_lg, the lanes-are-sites gradient sweep of univariate batches, and
optimize.fit_sites_lg on top of it.

Comparators, none of them the code under test: the dense oracle's gradient (test_gradient_cpu.dense_gradient; Richardson
differences of densemvn.loglik where the root is improper, as tests/test_gpu_gradient.py does), the existing gradient_lg on
the SAME beliefs, Richardson differences of synth's pruning log-likelihoods, and dense-covariance closed forms in numpy.
Every parity assertion is at 1e-8 relative to max(1, |block|_inf); each test prints its worst figure."""
import ctypes as C

import numpy as np
import pytest

from oracle import clustergraph as OCG
from oracle import densemvn as OD
from oracle import models as OM
from oracle import network as ON
from test_gradient_cpu import dense_gradient, fd_gradient, richardson

pytestmark = pytest.mark.gpu
TOL = 1e-8
BLOCKS = ("dR", "dmu", "dalpha", "dtheta")


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _rel(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))


def _against_existing(tag, cgb, got, keys=BLOCKS):
    """every site and block against gradient_lg(all_sites=True) on the same beliefs (it moves the pool to the plain layout:
    call it after everything that needs the layout the calibration left)"""
    ref = cgb.gradient_lg(all_sites=True)
    assert np.array_equal(ref["info"], got["info"]) and not got["info"].any(), (tag, got["info"], ref["info"])
    worst = 0.0
    for k in keys:
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        for s in range(got[k].shape[0]):
            worst = max(worst, _rel(got[k][s], ref[k][s]))
    print(f"{tag}: worst block against gradient_lg {worst:.2e}")
    assert worst <= TOL, tag
    return worst


def _against_dense(tag, got, s, net, model, tbl, taxa):
    """site s against the dense oracle (proper or fixed root), or against Richardson differences of the dense log-likelihood
    with their own measured uncertainty (improper root: max(10 x the disagreement of two step pairs, 1e-8))"""
    v = np.atleast_2d(np.asarray(model.rootpriorvariance(), float))
    tol = TOL
    if model.isrootfixed() or not np.any(np.isinf(np.diag(v))):
        want = dense_gradient(net, model, tbl, taxa)
    else:
        want, b = fd_gradient(net, model, tbl, taxa, 1e-3), fd_gradient(net, model, tbl, taxa, 2e-3)
        unc = max(_rel(want[k], b[k]) for k in BLOCKS)
        print(f"{tag}: finite-difference comparator uncertainty {unc:.2e}")
        tol = max(10 * unc, TOL)
    worst = 0.0
    for k in BLOCKS:
        w = np.atleast_1d(np.asarray(want[k], float)).reshape(-1)
        g = np.atleast_1d(np.asarray(got[k][s], float)).reshape(-1)
        worst = max(worst, _rel(g, w))
    print(f"{tag}, site {s}: worst block against the dense oracle {worst:.2e} (tolerance {tol:.1e})")
    assert worst <= tol, (tag, s)
    return worst


def _oracle_batch(P, net, taxa, models, tbls):
    """An engine of len(models) sites on the oracle's clique tree of `net`, per-site models and tip tables (same missing
    pattern at every site), factors assigned: (cgb, schedule tree, fam)."""
    from helpers import lg_inputs_from_oracle, oracle_setup
    import uni_net_ref as N
    cg = OCG.cliquetree(net)
    ocgb0 = oracle_setup(net, cg, models[0], tbls[0], taxa)
    dims, sepcl, so, si = N.engine_arrays(P, ocgb0)
    per = [lg_inputs_from_oracle(P, net, ocgb0, m, t, taxa) for m, t in zip(models, tbls)]
    fam = per[0][0]
    kw = dict(R=np.stack([k["R"] for _, _, k in per]), mu=np.stack([k["mu"] for _, _, k in per]))
    if isinstance(models[0], OM.UnivariateOrnsteinUhlenbeck):
        kw.update(model="ou", alpha=np.array([k["alpha"] for _, _, k in per]), theta=np.stack([k["theta"] for _, _, k in per]))
    cgb = P.ClusterGraphBelief.from_arrays(dims, sepcl, so, si, None, n_sites=len(models))
    cgb.lg_setup(fam, np.stack([d for _, d, _ in per]))
    cgb.assignfactors_lg_(**kw)
    return cgb, OCG.spanningtree_clusterlist(cg, OCG.default_rootcluster(cg, net)), fam


def _synth_engine(P, tree, X, colors=None):
    """An engine on synth's clique tree of a tree (fixed root), one site per row of X [n_sites, N]: (cgb, schedule tree, fam)"""
    from pgbp_amd import synth
    prob = synth.cliquetree_of_tree(tree, 1)
    fam = synth.lg_tree_table(tree, prob, 1, colors=colors)
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=X.shape[0])
    cgb.lg_setup(fam, np.ascontiguousarray(X[:, :, None]))
    return cgb, prob.schedule[0], fam


def _oracle_tree(tree):
    """(oracle network of a synth tree, its tip names, the node index of each tip name)"""
    net = ON.read_newick(tree.newick())
    taxa = list(net.tip_names)
    return net, taxa, [int(t[1:]) for t in taxa]


def _layout(cgb):
    return int(cgb._lib.pgbp_layout(cgb._eng))


# ----------------------------------------------------------------------------- 1: BM, the three site counts

@pytest.mark.parametrize("n_sites", [8, 64, 65])
def test_bm_per_site_batches(P, n_sites):
    """40-tip tree, fixed root, per-site data and parameters: 8 sites (plain layout), 64 (site-minor, one full wavefront), 65
    (a tail lane).  Every site against gradient_lg, sites 0 and last against the dense oracle."""
    from test_gpu_tip_noise import _batch
    cgb, spt, fam, Rs, site = _batch(P, 1, n_sites)
    ll, got = cgb.loglik_and_gradient_sites_lg(spt)
    assert bool(_layout(cgb) & 2) == (n_sites >= 64)
    assert got["dR"].shape == (n_sites, 1, 1, 1) and got["dmu"].shape == (n_sites, 1) and got["dalpha"].shape == (n_sites,)
    assert not got["dalpha"].any() and not got["dtheta"].any()
    for s in (0, n_sites - 1):
        onet, model, tbl, taxa = site(s)
        _against_dense(f"bm/{n_sites}", got, s, onet, model, tbl, taxa)
        dense = OD.loglik(onet, model, tbl, taxa)
        assert abs(ll[s] - dense) <= TOL * max(1.0, abs(dense))
    _against_existing(f"bm/{n_sites}", cgb, got)


# ----------------------------------------------------------------------------- 2: OU, three kinds of root

@pytest.mark.parametrize("root", ["fixed", "random", "improper"])
def test_ou_per_site_batch(P, root):
    """64 sites with their own alpha, theta, stationary variance and mu on a 30-tip tree.  Every site against gradient_lg,
    sites 0 and 63 against the dense oracle; fixed root: dalpha and dtheta of every site also against Richardson differences
    (relative steps 1e-3 / 5e-4) of synth.ou_loglik_pruning_uni_sites; improper root: dmu = 0."""
    from pgbp_amd import synth
    rng = np.random.default_rng(31)
    ns = 64
    tree = synth.random_tree(30, rng)
    net, taxa, tipnode = _oracle_tree(tree)
    alpha, gam2 = rng.uniform(0.3, 1.5, ns), rng.uniform(0.5, 2.0, ns)
    theta, mu = rng.normal(size=ns), rng.normal(size=ns)
    X = synth.simulate_ou_uni_sites(tree, 2 * alpha * gam2, alpha, theta, mu, rng)
    v = {"fixed": None, "random": 0.8, "improper": np.inf}[root]
    models = [OM.UnivariateOrnsteinUhlenbeck(2 * alpha[s] * gam2[s], alpha[s], theta[s], mu[s], v) for s in range(ns)]
    tbls = [[[float(X[s, i]) for i in tipnode]] for s in range(ns)]
    cgb, spt, fam = _oracle_batch(P, net, taxa, models, tbls)
    ll, got = cgb.loglik_and_gradient_sites_lg(spt)
    assert _layout(cgb) & 2 and not got["info"].any()
    if root == "improper":
        assert not got["dmu"].any()
    if root == "fixed":
        pr = synth.ou_loglik_pruning_uni_sites(tree, 2 * alpha * gam2, alpha, theta, mu, X)
        assert np.max(np.abs(ll - pr) / np.maximum(1.0, np.abs(pr))) <= TOL
        da = richardson(lambda h: synth.ou_loglik_pruning_uni_sites(tree, 2 * alpha * (1 + h) * gam2, alpha * (1 + h), theta, mu, X), 1e-3) / alpha
        dt = richardson(lambda h: synth.ou_loglik_pruning_uni_sites(tree, 2 * alpha * gam2, alpha, theta + h, mu, X), 1e-3)
        ea, et = _rel(got["dalpha"], da), _rel(got["dtheta"][:, 0], dt)
        print(f"ou/fixed: dalpha {ea:.2e}, dtheta {et:.2e} against Richardson differences of the pruning log-likelihood")
        assert ea <= TOL and et <= TOL
    for s in (0, ns - 1):
        _against_dense(f"ou/{root}", got, s, net, models[s], tbls[s], taxa)
    _against_existing(f"ou/{root}", cgb, got)


# ----------------------------------------------------------------------------- 3: tips without data, skipped families

def test_missing_tips_and_skipped_families(P):
    """65 sites on a 24-tip tree; a whole cherry and two more tips carry no data, so the cherry's internal family is skipped
    by the fill (child_mask 0) and must contribute nothing."""
    from pgbp_amd import synth
    rng = np.random.default_rng(32)
    tree = synth.random_tree(24, rng)
    kids = [np.nonzero(tree.parent == i)[0] for i in range(tree.nnodes)]
    inner = next(i for i in range(1, tree.nnodes) if len(kids[i]) == 2 and tree.is_leaf[kids[i]].all())
    others = [i for i in np.nonzero(tree.is_leaf)[0] if i not in kids[inner]]
    gone = [int(i) for i in kids[inner]] + [int(others[3]), int(others[4])]
    ns = 65
    s2, mu = rng.uniform(0.5, 2, ns), rng.normal(size=ns)
    X = synth.simulate_bm_uni_sites(tree, s2, mu, rng)
    X[:, gone] = np.nan
    net, names = P.read_newick(tree.newick())
    data_row = [int(names[i][1:]) if net.is_leaf[i] else -1 for i in range(net.nnodes)]
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, 1, fixedroot=True, data=X[0][:, None], data_row=data_row)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)], data_row, 1,
                        data=X[0][:, None])
    mask = np.asarray(fam["child_mask"])
    # four tips, and the cherry's own family at least
    assert int(np.sum(mask == 0)) >= 5 and np.any((mask == 0) & (np.asarray(fam["data_row"]) < 0)) and int(np.max(st.dims)) <= 2
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=ns)
    cgb.lg_setup(fam, np.ascontiguousarray(X[:, :, None]))
    cgb.assignfactors_lg_(s2.reshape(ns, 1, 1, 1), mu[:, None])
    ll, got = cgb.loglik_and_gradient_sites_lg(spt)
    assert _layout(cgb) & 2
    onet, taxa, tipnode = _oracle_tree(tree)
    for s in (0, ns - 1):
        tbl = [[None if i in gone else float(X[s, i]) for i in tipnode]]
        _against_dense("missing", got, s, onet, OM.UnivariateBrownianMotion(s2[s], mu[s]), tbl, taxa)
    _against_existing("missing", cgb, got)


# ----------------------------------------------------------------------------- 4: hybrid tips

@pytest.mark.parametrize("kind", ["bm", "ou"])
@pytest.mark.parametrize("name", ["N1", "N2", "N3", "N4"])
def test_hybrid_tip_networks(P, name, kind):
    """The four networks of uni_net_ref (two-parent families, 2-variable sepsets, 0-variable clusters) at 8 / 64 / 65 sites,
    fixed root: with a random root their clique trees hold a 3-variable cluster and are not thread-per-site engines."""
    import uni_net_ref as N
    root = "fixed"
    for n in (8, 64, 65):
        b = N.device_batch(P, name, root, kind, "cliquetree", n)
        assert int(np.max(b.dims)) <= 2
        ll, got = b.pcgb.loglik_and_gradient_sites_lg(b.sched[0])
        assert bool(_layout(b.pcgb) & 2) == (n >= 64)
        for s in (0, n - 1):
            _against_dense(f"{name}/{root}/{kind}/{n}", got, s, b.net, b.sites[s][0], b.sites[s][1], b.taxa)
        _against_existing(f"{name}/{root}/{kind}/{n}", b.pcgb, got)


# ----------------------------------------------------------------------------- 5: shifts and tip noise

@pytest.mark.parametrize("n_sites", [8, 65])
def test_shifts_and_tip_noise(P, n_sites):
    """Per-site shifts on three edges and per-site tip noise (sigma_e, se2) on every second tip, then the same shared over the
    sites: every block and dsigma_e against gradient_lg (pgbp_lg_gradient_noise) on the same beliefs."""
    from test_gpu_tip_noise import _batch, _batch_noise
    cgb, spt, fam, Rs, site = _batch(P, 1, n_sites)
    families, scale, sig, se2 = _batch_noise(fam, Rs, n_sites, 1, 9)
    edges = [(int(families[0]), 0), (int(families[-1]), 0), (len(fam["cluster"]) // 2, 0)]
    values = np.random.default_rng(10).normal(size=(n_sites, len(edges), 1))
    for tag, args in (("per-site", (sig, se2, values)), ("shared", (sig[1], se2[1], values[1]))):
        cgb.set_tip_noise_lg(families, args[0], scale, args[1])
        cgb.set_shifts_lg(edges, args[2])
        cgb.assignfactors_lg_(Rs[:, None], site.mus)
        ll, got = cgb.loglik_and_gradient_sites_lg(spt)
        assert "dsigma_e" in got and got["dsigma_e"].shape == (n_sites, 1, 1) and np.all(got["dsigma_e"] != 0)
        _against_existing(f"shifts+noise/{tag}/{n_sites}", cgb, got, BLOCKS + ("dsigma_e",))


# ----------------------------------------------------------------------------- 6: family-block boundaries, several rates

def _tree_with_families(n_fam):
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


@pytest.mark.parametrize("n_fam,n_rates", [(63, 1), (64, 1), (65, 1), (128, 1), (398, 1), (130, 6)])
def test_family_block_boundaries(P, n_fam, n_rates):
    """A thread walks blocks of 64 families: trees with 63, 64, 65 and 128 families, a 200-tip tree (398 families, 7 blocks),
    and 6 rates (more than one launch's 4 registers of rates).  64 sites against gradient_lg, site 0 against the dense oracle."""
    from pgbp_amd import synth
    tree = _tree_with_families(n_fam)
    assert tree.nnodes - 1 == n_fam
    rng = np.random.default_rng(33)
    ns = 64
    colors = rng.integers(n_rates, size=tree.nnodes) if n_rates > 1 else None
    if colors is not None:
        colors[1:n_rates + 1] = np.arange(n_rates)   # (every rate is used)
    rates = rng.uniform(0.5, 2.0, size=(ns, n_rates))
    mu = rng.normal(size=ns)
    X = synth.simulate_bm_uni_sites(tree, rates[:, 0], mu, rng)
    cgb, spt, fam = _synth_engine(P, tree, X, colors=colors)
    assert fam["n_rates"] == n_rates
    cgb.assignfactors_lg_(rates[:, :, None, None], mu[:, None])
    ll, got = cgb.loglik_and_gradient_sites_lg(spt)
    assert got["dR"].shape == (ns, n_rates, 1, 1)
    net, taxa, tipnode = _oracle_tree(tree)
    if n_rates == 1:
        model = OM.UnivariateBrownianMotion(rates[0, 0], mu[0])
    else:
        ecol = {e.number: 1 + int(colors[int(e.child.name[1:])]) for e in net.edges}
        model = OM.HeterogeneousBrownianMotion([np.array([[r]]) for r in rates[0]], ecol, np.array([mu[0]]), None)
    _against_dense(f"{n_fam} families/{n_rates} rates", got, 0, net, model, [[float(X[0, i]) for i in tipnode]], taxa)
    _against_existing(f"{n_fam} families/{n_rates} rates", cgb, got)


# ----------------------------------------------------------------------------- 7: determinism, read-only

def _raw(cgb, a, b, n_rates=1):
    n = b - a
    out = [np.zeros((n, n_rates)), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)]
    info = np.ones(n, np.int32)
    from pgbp_amd import _lib as L
    rc = cgb._lib.pgbp_lg_gradient_sites(cgb._eng, a, b, *[L.f64p(x) for x in out], L.i32p(info))
    assert rc == L.PGBP_OK
    return out, info


def test_determinism_and_read_only(P):
    from test_gpu_tip_noise import _batch
    cgb, spt, fam, Rs, site = _batch(P, 1, 65)
    ll, got = cgb.loglik_and_gradient_sites_lg(spt)
    assert _layout(cgb) == 2
    again = cgb.gradient_sites_lg()
    assert _layout(cgb) == 2
    for k in BLOCKS:
        assert np.array_equal(got[k], again[k]), k
    # every split of the site range gives the same bytes
    full, finfo = _raw(cgb, 0, 65)
    lo, _ = _raw(cgb, 0, 20)
    hi, _ = _raw(cgb, 20, 65)
    for f, a, b in zip(full, lo, hi):
        assert np.array_equal(f, np.concatenate([a, b]))
    assert np.array_equal(full[0].reshape(-1), got["dR"].reshape(-1)) and _layout(cgb) == 2
    # between two calibrations the layout never leaves site-minor
    ll2, got2 = cgb.loglik_and_gradient_sites_lg(spt)
    assert _layout(cgb) == 2
    for k in BLOCKS:
        assert np.array_equal(got[k], got2[k]), k
    # the pool after the sweep (the transfer moves it to the plain layout, an exact copy) ...
    cgb.pull()
    after = cgb._packed_raw.copy()
    assert _layout(cgb) == 0
    # ... the plain instance on the same 65 sites reads the same values: the same bytes, and still the same pool
    plain = cgb.gradient_sites_lg()
    assert _layout(cgb) == 0
    for k in BLOCKS:
        assert np.array_equal(got[k], plain[k]), k
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)
    # ... and equals the pool of a calibration that no sweep followed (the calibration returns the same bytes each time)
    o = cgb._opts()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    assert _layout(cgb) == 2
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)


def test_chunks_of_the_scratch_limit(P):
    """600 sites of an OU model with 6 rates (two rate groups of the kernel) on a tree of 66 families (two family blocks): the
    call at the default scratch limit and the call at pgbp_sites_sweep_scratch_limit(1) -- one workgroup's sites per chunk,
    256 + 256 + 88 -- return the same bytes in every output, info included; and the call on [256, 600) returns rows 256.. of
    the full call."""
    from pgbp_amd import synth
    rng = np.random.default_rng(36)
    ns, n_rates = 600, 6
    tree = synth.random_tree(34, rng)
    assert tree.nnodes - 1 == 66
    colors = rng.integers(n_rates, size=tree.nnodes)
    colors[1:n_rates + 1] = np.arange(n_rates)   # (every rate is used)
    alpha, theta, mu = rng.uniform(0.3, 1.5, ns), rng.normal(size=ns), rng.normal(size=ns)
    gam2 = rng.uniform(0.5, 2.0, size=(ns, n_rates))
    X = synth.simulate_ou_uni_sites(tree, 2 * alpha * gam2[:, 0], alpha, theta, mu, rng)
    cgb, spt, fam = _synth_engine(P, tree, X, colors=colors)
    assert fam["n_rates"] == n_rates and len(fam["cluster"]) >= 65
    cgb.assignfactors_lg_(gam2[:, :, None, None], mu[:, None], model="ou", alpha=alpha, theta=theta[:, None])
    ll, got = cgb.loglik_and_gradient_sites_lg(spt)
    assert _layout(cgb) == 2 and not got["info"].any()
    full, finfo = _raw(cgb, 0, ns, n_rates)
    assert np.array_equal(full[0].reshape(-1), got["dR"].reshape(-1)) and all(np.all(np.isfinite(x)) for x in full)
    assert np.all(full[0] != 0) and np.all(full[2] != 0) and np.all(full[3] != 0)   # (every rate, dalpha and dtheta are live)
    cgb._lib.pgbp_sites_sweep_scratch_limit(1)
    try:
        cut, cinfo = _raw(cgb, 0, ns, n_rates)
        hi, hinfo = _raw(cgb, 256, ns, n_rates)
    finally:
        cgb._lib.pgbp_sites_sweep_scratch_limit(0)
    for f, c, h in zip(full + [finfo], cut + [cinfo], hi + [hinfo]):
        assert f.tobytes() == c.tobytes() and f[256:].tobytes() == h.tobytes()
    whole, winfo = _raw(cgb, 256, ns, n_rates)   # (the slice at the default limit as well)
    for h, w in zip(hi + [hinfo], whole + [winfo]):
        assert h.tobytes() == w.tobytes()
    assert _layout(cgb) == 2


# ----------------------------------------------------------------------------- 8: one bad lane

def test_one_bad_lane(P):
    from test_gpu_tip_noise import _batch
    cgb, spt, fam, Rs, site = _batch(P, 1, 64)
    good_ll, good = cgb.loglik_and_gradient_sites_lg(spt)
    bad = Rs.copy()
    bad[37] = -1.0
    cgb.assignfactors_lg_(bad[:, None], site.mus)
    ll, got = cgb.loglik_and_gradient_sites_lg(spt)
    assert got["info"][37] != 0 and not np.delete(got["info"], 37).any()
    assert np.isnan(ll[37]) and all(np.isnan(got[k][37]).all() for k in BLOCKS)
    keep = np.arange(64) != 37
    for k in BLOCKS:
        assert np.array_equal(got[k][keep], good[k][keep]), k
    assert np.array_equal(ll[keep], good_ll[keep])
    # the sweep alone, on the beliefs that calibration left
    raw, info = _raw(cgb, 0, 64)
    assert info[37] != 0 and not np.delete(info, 37).any() and np.isnan(raw[0][37]).all() and np.isnan(raw[1][37])
    assert np.array_equal(raw[0][keep].reshape(-1), good["dR"][keep].reshape(-1))


# ----------------------------------------------------------------------------- 9: refusals

def _refused(cgb, code, word, a=0, b=None, ou_null=False):
    from pgbp_amd import _lib as L
    n = cgb.n_sites
    b = n if b is None else b
    out = [np.full(n, 7.0) for _ in range(5)]
    cgb.pull()
    before = cgb._packed_raw.copy()
    lay = _layout(cgb)
    args = [L.f64p(x) for x in out]
    if ou_null:
        args[2] = None
    rc = cgb._lib.pgbp_lg_gradient_sites(cgb._eng, a, b, *args, None)
    msg = cgb._lib.pgbp_last_error(cgb._eng)
    assert rc == code and word.encode() in msg, (rc, msg)
    assert all(np.all(x == 7.0) for x in out) and _layout(cgb) == lay
    cgb.pull()
    assert np.array_equal(before, cgb._packed_raw)


def test_refusals(P):
    from pgbp_amd import _lib as L
    from test_gpu_gradient import _tree_batch
    from test_gpu_tip_noise import _batch
    engine, spt, *_ = _tree_batch(P, 8, 2, 50, True)
    _refused(engine(np.arange(8)), L.ERR_INVALID, "2 traits")
    # p = 1 on a network whose clique tree has a cluster of 3 nodes
    rng = np.random.default_rng(34)
    net = ON.random_network(10, 2, rng)
    taxa = list(net.tip_names)
    models = [OM.UnivariateBrownianMotion(1.0, 0.0, 1.0)] * 8
    tbls = [[[float(x) for x in rng.normal(size=len(taxa))]] for _ in range(8)]
    cgb, _, _ = _oracle_batch(P, net, taxa, models, tbls)
    assert int(np.max(cgb._dims)) >= 3
    _refused(cgb, L.ERR_INVALID, "variables")
    cgb7, spt7, *_ = _batch(P, 1, 7)
    _refused(cgb7, L.ERR_INVALID, "7 sites")
    cgb8, spt8, fam8, Rs8, site8 = _batch(P, 1, 8)
    _refused(cgb8, L.ERR_INVALID, "site range", 0, 9)
    _refused(cgb8, L.ERR_INVALID, "site range", -1, 4)
    _refused(cgb8, L.ERR_INVALID, "site range", 5, 4)
    cgb8.assignfactors_lg_(Rs8[:, None], site8.mus, model="ou", alpha=np.full(8, 0.5), theta=np.zeros((8, 1)))
    _refused(cgb8, L.ERR_INVALID, "dalpha", ou_null=True)
    # no family table; a table but no parameters
    from pgbp_amd import synth
    tree = synth.random_tree(6, rng)
    prob = synth.cliquetree_of_tree(tree, 1)
    fresh = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=8)
    _refused(fresh, L.ERR_STATE, "pgbp_lg_setup")
    fresh.lg_setup(synth.lg_tree_table(tree, prob, 1), np.zeros((8, tree.nnodes, 1)))
    _refused(fresh, L.ERR_STATE, "pgbp_lg_assignfactors")


# ----------------------------------------------------------------------------- 10: the BM fit

def test_bm_fit_against_the_closed_form(P):
    """64 sites, 40-tip tree, fixed root: mu_hat = the GLS mean, sigma2_hat = r'C^-1 r / n from the dense covariance
    (test_fit_sites_cpu.bm_closed_form).  Every site converges; loglik >= the closed form's - 1e-8 max(1, |loglik|); the
    parameters within 1e-4 relative (a deficit eps of the log-likelihood allows an error of order sqrt(eps)); loglik_lg
    afterwards returns the fit's values (another entry point over the same factors: the postorder alone, 1e-12 relative); the
    sweep at the estimate meets the gtol criterion."""
    from pgbp_amd import synth
    from test_fit_sites_cpu import bm_closed_form
    rng = np.random.default_rng(35)
    tree = synth.random_tree(40, rng)
    ns = 64
    X = synth.simulate_bm_uni_sites(tree, rng.uniform(0.5, 2, ns), rng.normal(size=ns), rng)
    s2, mu, llc = bm_closed_form(tree, X)
    cgb, spt, fam = _synth_engine(P, tree, X)
    fit = P.fit_sites_lg(cgb, spt, "bm", np.ones(ns), np.zeros(ns), gtol=1e-8)
    print("BM fit: evaluations", fit["n_device_evals"], "iterations", fit["n_iter"].min(), "..", fit["n_iter"].max(),
          "worst loglik deficit", float(np.max((llc - fit["loglik"]) / np.maximum(1.0, np.abs(llc)))),
          "worst sigma2", float(np.max(np.abs(fit["R"] - s2) / s2)), "worst mu", float(np.max(np.abs(fit["mu"] - mu) / np.maximum(1.0, np.abs(mu)))))
    assert fit["converged"].all()
    assert np.all(fit["loglik"] >= llc - 1e-8 * np.maximum(1.0, np.abs(llc)))
    assert np.max(np.abs(fit["R"] - s2) / s2) <= 1e-4 and np.max(np.abs(fit["mu"] - mu) / np.maximum(1.0, np.abs(mu))) <= 1e-4
    assert _layout(cgb) == 2
    g = cgb.gradient_sites_lg()
    gt = np.stack([g["dR"][:, 0, 0, 0] * fit["R"], g["dmu"][:, 0]], axis=1)
    assert np.all(np.max(np.abs(gt), axis=1) <= 1e-8 * np.maximum(1.0, np.abs(fit["loglik"])))
    ll, info = cgb.loglik_lg()
    assert not info.any() and np.max(np.abs(ll - fit["loglik"]) / np.maximum(1.0, np.abs(ll))) <= 1e-12


# ----------------------------------------------------------------------------- 11: the OU fit

def ou_fit_case():
    from pgbp_amd import synth
    rng = np.random.default_rng(7)
    tree = synth.random_tree(96, rng)
    depth = np.zeros(tree.nnodes)
    for i in range(1, tree.nnodes):
        depth[i] = depth[tree.parent[i]] + tree.length[i]
    H = float(depth[tree.is_leaf].mean())
    alpha = rng.uniform(1, 3, 24) / H
    gam2 = rng.uniform(0.5, 2, 24)
    theta = rng.normal(0, 2, 24)
    mu = theta + rng.normal(0, 1, 24)
    X = synth.simulate_ou_uni_sites(tree, 2 * alpha * gam2, alpha, theta, mu, rng)
    return tree, H, X


def ou_reference(tree, H, X):
    """Per site: scipy L-BFGS-B on the pruning log-likelihood in (log gam2, log alpha, theta, mu) from (0, log(1 / H), tip
    mean, tip mean), log gam2 in [-8, 8], log alpha in [log(1e-3 / H), log(50 / H)], then a Nelder-Mead polish.
    Returns (loglik [n], on_bound [n], L-BFGS-B iterations [n])."""
    from pgbp_amd import synth
    from scipy.optimize import minimize
    import math
    bounds = [(-8.0, 8.0), (np.log(1e-3 / H), np.log(50.0 / H)), (None, None), (None, None)]
    n = X.shape[0]
    ll, on_bound, nit = np.zeros(n), np.zeros(n, bool), np.zeros(n, int)
    par, length, leaf = [int(v) for v in tree.parent], [float(v) for v in tree.length], [bool(v) for v in tree.is_leaf]
    N, log2pi = tree.nnodes, math.log(2 * math.pi)

    def pruning(g2, al, th, m0, x):
        """synth.ou_loglik_pruning_uni_sites for one site in plain floats (a few thousand evaluations per site: the vectorised
        one spends its time in numpy calls on arrays of one element); checked against it below"""
        A, B, Cc = [0.0] * N, [0.0] * N, [0.0] * N
        for i in range(N - 1, 0, -1):
            pa = par[i]
            q = math.exp(-al * length[i])
            w, V = (1.0 - q) * th, g2 * (1.0 - q * q)
            if leaf[i]:
                r = x[i] - w
                A[pa] += q * q / V
                B[pa] += q * r / V
                Cc[pa] += -0.5 * (r * r / V + log2pi + math.log(V))
            else:
                Pp, sc = A[i] + 1.0 / V, 1.0 / (1.0 + A[i] * V)
                A[pa] += A[i] * sc * q * q
                B[pa] += q * sc * (B[i] - A[i] * w)
                Cc[pa] += sc * (B[i] * w - 0.5 * A[i] * w * w) + 0.5 * B[i] * B[i] / Pp + Cc[i] - 0.5 * math.log1p(A[i] * V)
        return -0.5 * A[0] * m0 * m0 + B[0] * m0 + Cc[0]
    for s in range(n):
        Xs = X[s:s + 1]
        xs = [float(v) for v in X[s]]
        vec = synth.ou_loglik_pruning_uni_sites(tree, np.array([0.8]), np.array([0.5]), np.array([0.1]), np.array([0.2]), Xs)[0]
        assert abs(pruning(0.8, 0.5, 0.1, 0.2, xs) - vec) <= 1e-12 * abs(vec)

        def nll(t):
            try:
                v = -pruning(math.exp(t[0]), math.exp(t[1]), float(t[2]), float(t[3]), xs)
            except (OverflowError, ZeroDivisionError, ValueError):
                return 1e300
            return v if math.isfinite(v) else 1e300
        m = float(Xs[0, tree.is_leaf].mean())
        a = minimize(nll, [0.0, np.log(1.0 / H), m, m], method="L-BFGS-B", bounds=bounds, options={"ftol": 1e-15, "gtol": 1e-9})
        b = minimize(nll, a.x, method="Nelder-Mead", options={"xatol": 1e-9, "fatol": 1e-12, "maxiter": 2000})
        best = b if b.fun <= a.fun else a
        ll[s], nit[s] = -best.fun, a.nit
        on_bound[s] = any(lo is not None and (abs(best.x[k] - lo) <= 1e-6 or abs(best.x[k] - hi) <= 1e-6) for k, (lo, hi) in enumerate(bounds))
    return ll, on_bound, nit


def test_ou_fit_is_no_worse_than_the_scipy_reference(P):
    """24 sites on a 96-tip tree (rng 7; the recipe in ou_fit_case).  The device fit is no worse than the reference:
    loglik >= reference - 1e-8 max(1, |loglik|) at every site whose reference is off the bounds (at most 2 may be on one)."""
    tree, H, X = ou_fit_case()
    ref, on_bound, nit = ou_reference(tree, H, X)
    assert on_bound.sum() <= 2, on_bound
    cgb, spt, fam = _synth_engine(P, tree, X)
    tipmean = X[:, tree.is_leaf].mean(axis=1)
    fit = P.fit_sites_lg(cgb, spt, "ou", np.ones(24), tipmean, alpha0=np.full(24, 1.0 / H), theta0=tipmean, gtol=1e-8)
    gap = (ref - fit["loglik"]) / np.maximum(1.0, np.abs(ref))
    print("OU fit: evaluations", fit["n_device_evals"], "iterations", fit["n_iter"], "converged", int(fit["converged"].sum()),
          "reference L-BFGS-B iterations", int(nit.max()), "on a bound", int(on_bound.sum()),
          "worst deficit against the reference", float(gap[~on_bound].max()), "best gain", float(-gap[~on_bound].min()))
    assert np.all(np.isfinite(fit["loglik"]))
    assert np.all(gap[~on_bound] <= 1e-8)

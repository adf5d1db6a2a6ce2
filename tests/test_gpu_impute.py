"""pgbp_lg_impute / ClusterGraphBelief.impute_lg: the posterior mean and covariance of every missing tip value from one
calibration, one sweep over the tip families that miss a trait, on the device.

Comparator (tests/impute_ref.py): the DENSE conditioning of the joint distribution on oracle/densemvn.py alone
(dense_impute), asserted at 1e-8 relative to the largest entry of a block (the project's parity bound); the numpy
restatement of the sweep is pinned to it on the CPU by test_impute_cpu.py for every case used here (worst 3.1e-13), and
gives the rule the device's `predicted` masks must equal.  The measured worst error of every case is printed."""
import ctypes as C

import numpy as np
import pytest

import impute_ref as IR
import loo_ref as LR
from helpers import lg_inputs_from_oracle
from oracle import densemvn as OD
from test_gpu_gradient import _device

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _u64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _check(P, tag, net, model, tbl, taxa, want_counts):
    """One-site engine on the clique tree of an oracle case: log-likelihood, the listed families and their masks against the
    restatement's rule, every predicted entry against the dense comparator."""
    cg, ocgb, pcgb, spt = _device(P, net, model, tbl, taxa)
    ll, d = pcgb.impute_and_loglik_lg(spt)
    dense_ll = OD.loglik(net, model, tbl, taxa)
    assert abs(ll - dense_ll) <= 1e-8 * max(1.0, abs(dense_ll)), (tag, ll, dense_ll)
    fam, data, _ = lg_inputs_from_oracle(P, net, ocgb, model, tbl, taxa)      # (the table the engine was set up with)
    fams, pred = IR.listed_families(fam)
    assert np.array_equal(d["families"], fams), tag
    assert np.array_equal(d["predicted"], IR.mask_bits(pred, model.dimension())), tag
    assert np.array_equal(d["rows"], fam["data_row"][fams]), tag
    assert pcgb._lib.pgbp_lg_impute_count(pcgb._eng) == len(fams)
    assert IR.counts(tbl, d) == want_counts, (tag, IR.counts(tbl, d), want_counts)
    err = IR.worst_error(d, IR.dense_impute(net, model, tbl, taxa), symmetric=True)
    print(f"{tag}: device vs dense comparator {err:.2e} over {want_counts[1]} entries (tolerance 1e-8)")
    assert err <= 1e-8, tag
    return pcgb, spt, d, data


# ----------------------------------------------------------------------------- 1, 2, 3: networks, models, roots

@pytest.mark.parametrize("root,counts", IR.MISSING_ROOTS)
def test_impute_missing_case(P, root, counts):
    """p = 3 on a network with 4 hybrids, 30 % of the values missing, each root."""
    _check(P, f"missing/p3/{root}", *IR.missing_case(root), counts)


@pytest.mark.parametrize("which,p,seed,frac,counts", IR.MASKED)
def test_impute_masked_random_networks(P, which, p, seed, frac, counts):
    """24 tips, 6 hybrid nodes, entries masked at random (whole tips may lose all data: at p = 1 every missing entry is a
    tip without data, the family the fill skips)."""
    _check(P, f"{which}/p{p}/seed{seed}", *IR.masked_random_case(which, p, seed, frac), counts)


@pytest.mark.parametrize("root", ["fixed", "random"])
def test_impute_tips_without_data_under_a_parent_out_of_scope(P, root):
    """exact_reml_missing: the two tips without data are listed, nothing of them is predicted (their parent holds nothing in
    scope): info -1, all NaN; the internal node with nothing in scope is not listed."""
    net, model, tbl, taxa = LR.no_data_case(root)
    pcgb, spt, d, data = _check(P, f"exact_reml_missing/{root}", net, model, tbl, taxa, (2, 0))
    assert len(d["families"]) == 2 and not d["predicted"].any() and np.all(d["info"] == -1)
    assert np.isnan(d["mean"]).all() and np.isnan(d["cov"]).all()
    lg = pcgb._lg
    assert np.all(lg["data_row"][d["families"]] >= 0)
    assert np.sum((lg["child_pos"] < 0) & (lg["data_row"] < 0)) >= 1


# ----------------------------------------------------------------------------- 4, 5: the dimension classes of the solve

def _same_bytes_on_the_plain_layout(pcgb, first):
    """pgbp_get_belief puts the engine into the plain layout (pgbp_layout == 0): the sweep returns the same bytes as before.
    Returns the layout the engine was in."""
    from pgbp_amd import _lib as L
    lib, eng = pcgb._lib, pcgb._eng
    layout = lib.pgbp_layout(eng)
    rec = np.zeros(int(pcgb._dims[0]) ** 2 + int(pcgb._dims[0]) + 1)
    assert lib.pgbp_get_belief(eng, 0, 0, L.f64p(rec)) == L.PGBP_OK
    assert lib.pgbp_layout(eng) == 0
    plain = pcgb.impute_lg()
    for k in ("mean", "cov", "info", "predicted", "families"):
        assert first[k].tobytes() == plain[k].tobytes(), k
    return layout


def _both_layouts(P, tag, case, counts):
    """An oracle case after the calibration, and again on the plain layout.  Returns (layout the calibration left, cluster
    dimensions)."""
    pcgb, spt, first, _ = _check(P, tag, *case, counts)
    dims = pcgb._dims[: pcgb.nclusters]
    assert int(dims.max()) == 32
    return _same_bytes_on_the_plain_layout(pcgb, first), sorted(set(int(m) for m in dims))


def test_impute_wavefront_class_and_layouts(P):
    """tree(12, 16, 0, 0.1): clusters of 32 variables (the wavefront class).  After the calibration the engine holds its
    beliefs in the packed BS16 layout (pgbp_layout == 1); pgbp_get_belief converts them to the plain one (pgbp_layout == 0): the
    sweep returns the same bytes on both, and agrees with the dense comparator at 1e-8.
    The engine packs a graph only when every cluster has P or 2P variables, so it is set up here as the product's own host
    side sets a tree up without looking at the data: every trait of every internal node in scope
    (impute_ref.full_scope_setup; pinned on the CPU by test_impute_wavefront_tree_with_every_trait_in_scope).  All 22 missing
    entries are then predicted.  With the scopes the oracle allocates from the data (a parent below which no tip observes a
    trait drops it: clusters of 15, 16, 31 and 32 variables, counts 22 / 20) the engine stays in the plain layout; that set-up
    is run as well, for its masks, its parity and the equal bytes after pgbp_get_belief."""
    case = IR.tree_case(*IR.WAVEFRONT[0])
    tree, model, tbl, taxa = case
    su = IR.full_scope_setup(*case)
    pcgb = P.ClusterGraphBelief.from_arrays(*su["arrays"])
    pcgb.lg_setup(su["fam"], su["data"])
    pcgb.assignfactors_lg_(**su["kw"])
    ll, d = pcgb.impute_and_loglik_lg(su["spt"])
    dense_ll = OD.loglik(tree, model, tbl, taxa)
    assert abs(ll - dense_ll) <= 1e-8 * max(1.0, abs(dense_ll)), (ll, dense_ll)
    fams, pred = IR.listed_families(su["fam"])
    assert np.array_equal(d["families"], fams) and np.array_equal(d["predicted"], IR.mask_bits(pred, 16))
    assert IR.counts(tbl, d) == (22, 22)
    err = IR.worst_error(d, IR.dense_impute(*case), symmetric=True)
    print(f"tree/p16, every trait in scope: device vs dense comparator {err:.2e} over 22 entries (tolerance 1e-8)")
    assert err <= 1e-8
    dims = sorted(set(int(m) for m in pcgb._dims[: pcgb.nclusters]))
    assert dims == [16, 32]
    assert pcgb._lib.pgbp_layout(pcgb._eng) == 1, "the p = 16 tree is expected in the packed layout after a calibration"
    assert _same_bytes_on_the_plain_layout(pcgb, d) == 1
    # the oracle's scopes: 22 / 20
    layout, dims = _both_layouts(P, "tree/p16", case, IR.WAVEFRONT[1])
    print(f"tree/p16, the oracle's scopes: pgbp_layout after the calibration {layout}, cluster dimensions {dims}")
    assert dims == [15, 16, 31, 32]


def test_impute_packed_layout(P):
    """The complete 12-tip p = 16 tree of the leave-one-out tests with entries of at most one tip of any cherry masked (one
    tip loses everything): also with the scopes the oracle allocates every cluster has 16 or 32 variables, the engine is in
    the packed BS16 layout after the calibration (pgbp_layout == 1) and the sweep stages each record through its upper
    triangle: the same bytes as on the plain layout."""
    layout, dims = _both_layouts(P, "tree/p16/packed", IR.packed_case(), IR.PACKED_COUNTS)
    assert dims == [16, 32] and layout == 1


def test_impute_workgroup_class(P):
    """A tree at p = 40: clusters of 80 variables (the workgroup class, 65 .. 128)."""
    args, counts = IR.WORKGROUP
    pcgb, *_ = _check(P, "tree/p40", *IR.tree_case(*args), counts)
    assert int(pcgb._dims[: pcgb.nclusters].max()) == 80


# ----------------------------------------------------------------------------- 6: refusals

def _buffers(n, p, sites=1):
    return (np.full((sites, max(n, 1), p), SENTINEL), np.full((sites, max(n, 1), p * p), SENTINEL),
            np.full((sites, max(n, 1)), 77, np.int32))


def test_impute_refuses_what_does_not_fit_the_lds(P):
    """p = 64 on a tree: clusters of 128 variables (133 KB of working matrix) plus five p x p blocks exceed the 160 KB of
    LDS: PGBP_ERR_INVALID before any launch, the bytes named, the outputs untouched."""
    from pgbp_amd import _lib as L
    net, model, tbl, taxa = IR.tree_case(*IR.TOO_BIG)
    _, _, pcgb, spt = _device(P, net, model, tbl, taxa)
    assert int(pcgb._dims[: pcgb.nclusters].max()) == 128
    n = pcgb._lib.pgbp_lg_impute_count(pcgb._eng)
    assert n > 0
    mean, cov, info = _buffers(n, 64)
    rc = pcgb._lib.pgbp_lg_impute(pcgb._eng, 0, 1, L.f64p(mean), L.f64p(cov), L.i32p(info))
    msg = pcgb._lib.pgbp_last_error(pcgb._eng)
    assert rc == L.ERR_INVALID and b"bytes of LDS" in msg, msg
    assert np.all(mean == SENTINEL) and np.all(cov == SENTINEL) and np.all(info == 77)
    with pytest.raises(L.PgbpError) as ex:
        pcgb.impute_lg()
    assert ex.value.code == L.ERR_INVALID and "bytes of LDS" in ex.value.msg


def test_impute_refuses_clusters_above_128_variables(P):
    """The Mueller clique tree at 3 traits has clusters of more than 128 variables: PGBP_ERR_INVALID before any launch (and
    before the count of listed families is looked at: the data are complete), the family and its cluster named."""
    from pgbp_amd import _lib as L
    from test_gpu_loo import _muller
    cgb, spt, st, *_ = _muller(P, 3)
    assert int(st.dims.max()) > 128
    mean, cov, info = _buffers(1, 3)
    rc = cgb._lib.pgbp_lg_impute(cgb._eng, 0, 1, L.f64p(mean), L.f64p(cov), L.i32p(info))
    msg = cgb._lib.pgbp_last_error(cgb._eng)
    assert rc == L.ERR_INVALID and b"more than 128 variables" in msg and b"family" in msg and b"cluster" in msg
    assert np.all(mean == SENTINEL) and np.all(cov == SENTINEL) and np.all(info == 77)
    with pytest.raises(L.PgbpError):
        cgb.impute_lg()


def _tree_batch(P, p=2):
    """loo_ref.batch_case(p) under impute_ref.batch_pattern: engines over any list of its 64 sites."""
    nwk, taxa, data, Rs, mus = LR.batch_case(p)
    miss = IR.batch_pattern(p)
    data = data.copy()
    data[:, miss] = np.nan
    net, names = P.read_newick(nwk)
    row = {t: r for r, t in enumerate(taxa)}
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=True)
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], p, data=data[0])
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))

    def engine(sites, assign=True, setup=True):
        cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=len(sites))
        if setup:
            cgb.lg_setup(fam, data[sites])
        if assign:
            cgb.assignfactors_lg_(Rs[sites][:, None], mus[sites])
        return cgb
    return engine, spt, fam, taxa, miss


def test_impute_state_and_argument_refusals(P):
    """No family table, no parameters yet: PGBP_ERR_STATE; a bad site range, mean and cov both NULL: PGBP_ERR_INVALID; the
    outputs untouched every time."""
    from pgbp_amd import _lib as L
    engine, spt, fam, taxa, miss = _tree_batch(P)
    sites = np.arange(3)
    n = int(miss.any(axis=1).sum())
    mean, cov, info = _buffers(n, 2, 3)
    out = (L.f64p(mean), L.f64p(cov), L.i32p(info))
    bare = engine(sites, assign=False, setup=False)
    assert bare._lib.pgbp_lg_impute(bare._eng, 0, 3, *out) == L.ERR_STATE
    assert b"pgbp_lg_setup" in bare._lib.pgbp_last_error(bare._eng)
    assert bare._lib.pgbp_lg_impute_count(bare._eng) == -1
    assert bare._lib.pgbp_lg_impute_families(bare._eng, None, None) == L.ERR_STATE
    table = engine(sites, assign=False)
    assert table._lib.pgbp_lg_impute_count(table._eng) == n
    assert table._lib.pgbp_lg_impute(table._eng, 0, 3, *out) == L.ERR_STATE
    assert b"pgbp_lg_assignfactors" in table._lib.pgbp_last_error(table._eng)
    cgb = engine(sites)
    lib, eng = cgb._lib, cgb._eng
    for s0, s1 in ((0, 4), (-1, 2), (2, 1)):
        assert lib.pgbp_lg_impute(eng, s0, s1, *out) == L.ERR_INVALID
        assert b"site range" in lib.pgbp_last_error(eng)
    assert lib.pgbp_lg_impute(eng, 0, 3, None, None, L.i32p(info)) == L.ERR_INVALID
    assert b"both NULL" in lib.pgbp_last_error(eng)
    assert lib.pgbp_lg_impute(eng, 1, 1, *out) == L.PGBP_OK           # an empty range
    assert np.all(mean == SENTINEL) and np.all(cov == SENTINEL) and np.all(info == 77)
    fams = np.zeros(n, np.int32)
    pred = np.zeros(n, np.uint64)
    assert lib.pgbp_lg_impute_families(eng, L.i32p(fams), None) == L.PGBP_OK      # either pointer may be NULL
    assert lib.pgbp_lg_impute_families(eng, None, _u64p(pred)) == L.PGBP_OK
    want_f, want_p = IR.listed_families(fam)
    assert np.array_equal(fams, want_f) and np.array_equal(pred, want_p)


# ----------------------------------------------------------------------------- 7: complete data

def test_impute_complete_data_lists_nothing(P):
    from pgbp_amd import _lib as L
    net, model, tbl, taxa = LR.random_case("bm_random", 4)
    _, _, pcgb, spt = _device(P, net, model, tbl, taxa)
    assert pcgb._lib.pgbp_lg_impute_count(pcgb._eng) == 0
    mean, cov, info = _buffers(0, 4)
    assert pcgb._lib.pgbp_lg_impute(pcgb._eng, 0, 1, L.f64p(mean), L.f64p(cov), L.i32p(info)) == L.PGBP_OK
    assert np.all(mean == SENTINEL) and np.all(cov == SENTINEL) and np.all(info == 77)
    ll, d = pcgb.impute_and_loglik_lg(spt)
    assert len(d["families"]) == 0 and d["mean"].shape == (0, 4) and d["cov"].shape == (0, 4, 4) and d["predicted"].shape == (0, 4)


# ----------------------------------------------------------------------------- 8: a batch

def test_impute_batch_of_64_sites(P):
    """64 sites with their own data and parameters on a 40-tip tree at p = 2, one NaN pattern (at most one tip of a cherry:
    every missing entry is predicted).  Sites 0, 31 and 63 against the dense comparator; two calls return the same bytes;
    four chunks of sites (pgbp_impute_scratch_limit) change nothing; a site range equals the slice of the full call."""
    from pgbp_amd import _lib as L
    p = 2
    engine, spt, fam, taxa, miss = _tree_batch(P, p)
    cgb = engine(np.arange(64))
    ll, d = cgb.impute_and_loglik_lg(spt, all_sites=True)
    n = int(miss.any(axis=1).sum())
    assert d["mean"].shape == (64, n, p) and d["cov"].shape == (64, n, p, p) and not d["info"].any()
    assert np.array_equal(d["predicted"], miss[d["rows"]])
    again = cgb.impute_lg(all_sites=True)
    keys = ("mean", "cov", "info")
    for k in keys:
        assert d[k].tobytes() == again[k].tobytes(), k
    for s in (0, 31, 63):
        onet, model, tbl, _ = IR.batch_site(p, s)
        one = {k: (d[k][s] if k in keys else d[k]) for k in d}
        err = IR.worst_error(one, IR.dense_impute(onet, model, tbl, taxa), symmetric=True)
        dense_ll = OD.loglik(onet, model, tbl, taxa)
        print(f"batch site {s}: device vs dense comparator {err:.2e}")
        assert err <= 1e-8 and abs(ll[s] - dense_ll) <= 1e-8 * abs(dense_ll)
    # chunks of sites
    per_site = n * (1 + p + p * p)
    cgb._lib.pgbp_impute_scratch_limit(per_site * 21)          # 64 sites: 21 + 21 + 21 + 1
    try:
        cut = cgb.impute_lg(all_sites=True)
    finally:
        cgb._lib.pgbp_impute_scratch_limit(0)
    for k in keys:
        assert d[k].tobytes() == cut[k].tobytes(), k
    # a site range
    mean = np.zeros((21, n, p)); cov = np.zeros((21, n, p, p)); info = np.ones((21, n), np.int32)
    assert cgb._lib.pgbp_lg_impute(cgb._eng, 20, 41, L.f64p(mean), L.f64p(cov), L.i32p(info)) == L.PGBP_OK
    assert not info.any()
    assert mean.tobytes() == d["mean"][20:41].tobytes()
    assert np.ascontiguousarray(cov.transpose(0, 1, 3, 2)).tobytes() == np.ascontiguousarray(d["cov"][20:41]).tobytes()


# ----------------------------------------------------------------------------- 9: the filled table, one output alone

def test_imputed_data_and_single_outputs(P):
    """imputed_data fills exactly the predicted entries of the p = 3 case; mean = NULL or cov = NULL alone works and leaves the
    other output equal to the two-output call."""
    from pgbp_amd import _lib as L
    net, model, tbl, taxa = IR.missing_case("random")
    pcgb, spt, d, data = _check(P, "missing/p3/random", net, model, tbl, taxa, (17, 14))
    out = P.imputed_data(d, data)
    filled = np.isfinite(out) & ~np.isfinite(data)
    want = np.zeros_like(filled)
    want[d["rows"]] = d["predicted"]
    assert np.array_equal(filled, want) and filled.sum() == 14 and np.isnan(out).sum() == 3
    assert np.array_equal(out[np.isfinite(data)], data[np.isfinite(data)]) and np.isnan(data).sum() == 17
    assert np.array_equal(out[d["rows"]][d["predicted"]], d["mean"][d["predicted"]])
    n, p = len(d["families"]), 3
    lib, eng = pcgb._lib, pcgb._eng
    mean, cov, info = _buffers(n, p)
    assert lib.pgbp_lg_impute(eng, 0, 1, L.f64p(mean), None, L.i32p(info)) == L.PGBP_OK
    assert mean[0].tobytes() == d["mean"].tobytes() and np.all(cov == SENTINEL) and np.array_equal(info[0], d["info"])
    mean2, cov2, _ = _buffers(n, p)
    assert lib.pgbp_lg_impute(eng, 0, 1, None, L.f64p(cov2), None) == L.PGBP_OK
    assert np.all(mean2 == SENTINEL)
    got = cov2[0].reshape(n, p, p).transpose(0, 2, 1)
    assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(d["cov"]).tobytes()


# ----------------------------------------------------------------------------- info of a bad site

def test_impute_info_of_a_bad_site(P):
    """A site whose rate matrix is not positive definite: every listed tip of that site is NaN with info > 0, nothing raises,
    and the neighbouring sites are the same bytes as without it."""
    nwk, taxa0, data0, Rs, mus = LR.batch_case(2)
    engine, spt, fam, taxa, miss = _tree_batch(P)
    sites = np.arange(3)
    cgb = engine(sites)
    _, good = cgb.impute_and_loglik_lg(spt, all_sites=True)
    assert not good["info"].any()
    bad = Rs[sites].copy()
    bad[1] = np.array([[1.0, 2.0], [2.0, 1.0]])
    cgb.assignfactors_lg_(bad[:, None], mus[sites])
    ll, got = cgb.impute_and_loglik_lg(spt, all_sites=True)
    assert np.all(got["info"][1] > 0) and not got["info"][0].any() and not got["info"][2].any()
    assert np.isnan(got["mean"][1]).all() and np.isnan(got["cov"][1]).all()
    for s in (0, 2):
        for k in ("mean", "cov"):
            assert good[k][s].tobytes() == got[k][s].tobytes(), (s, k)

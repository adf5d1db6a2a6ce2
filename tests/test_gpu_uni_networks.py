"""Networks whose hybrid node is a TIP (tests/uni_net_ref.py: N1-N4, pinned on the CPU by tests/test_uni_cases_cpu.py) as
batches of 8, 64 and 65 univariate sites with per-site data and parameters: the thread-per-site kernels OFF clique trees of
trees.  Every existing test of a batch of tiny beliefs uses the clique tree of a tree, where every sepset holds one variable
and every family one parent; here the fixed-root clique trees have 2-variable sepsets (bp_level_uni<SM>) and 0-variable
clusters and sepsets, the hybrid tip's family has two parents (the hybrid branch of lg_fill_uni_sm_kernel and of
shift_uni_sm_kernel; in N4 one of them is the fixed root), and the random-root Bethe graphs are loopy with 1-variable
sepsets (bp_level_uni1 / bp_chunk_uni1 on a graph that is no tree).

Every device engine is built from the ORACLE's cluster graph (uni_net_ref.device_batch); every site of every engine is
compared with the oracle run on that site alone.  Gate: 1e-8 relative to max(1, the record's largest entry); each test
prints its measured figure.
"""
import numpy as np
import pytest

import uni_net_ref as N
from helpers import oracle_setup
from oracle import densemvn as OD
from shift_ref import ShiftedModel, family_edge

pytestmark = pytest.mark.gpu
TOL = 1e-8
SIZES = (8, 64, 65)
CASES = [(n, r, k) for n in N.NEWICK for r in N.ROOTS[n] for k in ("bm", "ou")]
FIXED = [c for c in CASES if c[1] == "fixed"]


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _thread_per_site(dims, n_sites):
    return int(np.max(dims)) <= 2 and n_sites >= 8


def _site_minor(pcgb):
    return bool(pcgb._lib.pgbp_layout(pcgb._eng) & 2)


def _cluster_part(b, packed):
    d = b.dims[:b.pcgb.nclusters].astype(np.int64)
    return packed[..., :int(np.sum(d * d + d + 1))]


# ----------------------------------------------------------------------------- the fill

@pytest.mark.parametrize("graph_kind", ["cliquetree", "bethe"])
@pytest.mark.parametrize("name,root,kind", CASES)
def test_fill_every_record_of_every_site(P, name, root, kind, graph_kind):
    """assignfactors_lg_ with per-site parameters against the oracle's assignfactors of each site: every cluster record,
    the sepsets the constant 1.  The Bethe graphs walk the general family table and, with a fixed root, hold 0-variable
    clusters; OU with a hybrid exercises qc = gamma a, wc = gamma (1 - a)."""
    for n in SIZES:
        b = N.device_batch(P, name, root, kind, graph_kind, n)
        if _thread_per_site(b.dims, n) and n >= 64:
            assert _site_minor(b.pcgb), "a batch of tiny beliefs of 64 sites and more is filled in the site-minor layout"
        hyb = int(np.sum(b.fam["n_parents"] >= 2))
        assert hyb == (2 if name == "N2" else 1)
        b.pcgb.pull()
        got = b.pcgb._packed_raw
        nclu = _cluster_part(b, got).shape[-1]
        worst = 0.0
        for s in range(n):
            want = N.oracle_factors(name, root, kind, graph_kind, s)
            assert not got[s, nclu:].any()
            worst = max(worst, N.records_error(got[s, :nclu], want[:nclu], b.dims[:b.pcgb.nclusters]))
        print(f"fill {name}/{root}/{kind}/{graph_kind}/{n} sites (largest belief {int(b.dims.max())}): "
              f"records vs the oracle's, worst of all sites {worst:.2e}")
        assert worst <= TOL


# ----------------------------------------------------------------------------- shifts on the edges of a hybrid tip

@pytest.mark.parametrize("graph_kind", ["cliquetree", "bethe"])
@pytest.mark.parametrize("name,kind", [("N1", "bm"), ("N1", "ou"), ("N2", "bm"), ("N4", "bm")])
def test_shifts_on_the_edges_of_a_hybrid_tip(P, name, kind, graph_kind):
    """set_shifts_lg on one edge and on both edges of a hybrid tip, per-site and shared values, 64 and 65 sites (the
    site-minor layout: the hybrid branch of shift_uni_sm_kernel) and 8: the records against the oracle's assignfactors of
    shift_ref.ShiftedModel, loglik_lg against densemvn.loglik of the same wrapper (clique trees), at every site."""
    rng = np.random.default_rng(11)
    for n in SIZES:
        b = N.device_batch(P, name, "fixed", kind, graph_kind, n, assign=False)
        f = int(np.flatnonzero(b.fam["n_parents"] >= 2)[0])
        nclu = None
        for edges in ([(f, 0)], [(f, 1)], [(f, 0), (f, 1)]):
            for per_site in (True, False):
                values = rng.uniform(0.5, 1.5, size=(n, len(edges), 1)) * rng.choice([-1.0, 1.0], size=(n, len(edges), 1))
                if not per_site:
                    values = np.broadcast_to(values[0], values.shape)
                b.pcgb.set_shifts_lg(edges, values if per_site else values[0])
                b.pcgb.assignfactors_lg_(**b.kw)
                if n >= 64:
                    assert _thread_per_site(b.dims, n) and _site_minor(b.pcgb)
                b.pcgb.pull()
                got = b.pcgb._packed_raw.copy()
                nclu = _cluster_part(b, got).shape[-1]
                if graph_kind == "cliquetree":
                    b.pcgb._ensure_schedule(b.sched)
                    ll, info = b.pcgb.loglik_lg()
                    assert not info.any()
                worst = plain = wll = 0.0
                for s in range(n):
                    model, tbl = b.sites[s]
                    w = ShiftedModel(model, {family_edge(b.net, b.ocgb0, b.fam, ff, k).number: v for (ff, k), v in zip(edges, values[s])})
                    want = N.pack(oracle_setup(b.net, b.cg, w, tbl, b.taxa))
                    worst = max(worst, N.records_error(got[s, :nclu], want[:nclu], b.dims[:b.pcgb.nclusters]))
                    plain = max(plain, N.records_error(got[s, :nclu], N.oracle_factors(name, "fixed", kind, graph_kind, s)[:nclu],
                                                       b.dims[:b.pcgb.nclusters]))
                    if graph_kind == "cliquetree":
                        dense = OD.loglik(b.net, w, tbl, b.taxa)
                        wll = max(wll, abs(ll[s] - dense) / max(1.0, abs(dense)))
                print(f"shifts {name}/{kind}/{graph_kind}/{n} sites, edges {edges}, {'per-site' if per_site else 'shared'}: records "
                      f"{worst:.2e} (vs the unshifted {plain:.2e}), loglik vs dense {wll:.2e}")
                assert worst <= TOL and wll <= TOL and plain > 1e-3


# ----------------------------------------------------------------------------- clique trees (fixed root: thread-per-site)

@pytest.mark.parametrize("name,root,kind", FIXED)
def test_clique_tree_loglik_and_calibration(P, name, root, kind):
    """loglik_lg of every site against densemvn.loglik; reps = 2 returns the bytes of reps = 1 (the sep_zero shortcut on
    bp_level_uni); after two calibrate_ iterations every belief of every site against the oracle's calibration of that site,
    both flags (True, True)."""
    for n in SIZES:
        b = N.device_batch(P, name, root, kind, "cliquetree", n)
        assert _thread_per_site(b.dims, n)
        if name in ("N1", "N2", "N3"):
            assert int(b.dims[b.pcgb.nclusters:].max()) == 2, "bp_level_uni: the engine's largest sepset holds 2 variables"
        b.pcgb._ensure_schedule(b.sched)
        ll, info = b.pcgb.loglik_lg()
        assert _site_minor(b.pcgb) == (n >= 64)
        ll2, info2 = b.pcgb.loglik_lg(reps=2)
        assert ll2.tobytes() == ll.tobytes() and not info.any() and not info2.any()
        wll = 0.0
        for s in range(n):
            dense = OD.loglik(b.net, b.sites[s][0], b.sites[s][1], b.taxa)
            wll = max(wll, abs(ll[s] - dense) / max(1.0, abs(dense)))
        b.pcgb.assignfactors_lg_(**b.kw)
        P.calibrate_(b.pcgb, b.sched, 2, verbose=False, sync=False)      # (a pull moves the state to the plain layout)
        assert _site_minor(b.pcgb) == (n >= 64)
        results = [(int(r.succ), int(r.iscal)) for r in b.pcgb.last_results]
        b.pcgb.pull()
        worst = 0.0
        for s in range(n):
            snaps, _ = N.oracle_calibration(name, root, kind, "cliquetree", s, (1, 2))
            assert snaps[2].got == (True, True) and results[s] == (1, 1), (s, results[s])
            worst = max(worst, N.records_error(b.pcgb._packed_raw[s], snaps[2].packed, b.dims))
        print(f"clique tree {name}/{root}/{kind}/{n} sites: loglik vs dense {wll:.2e}, beliefs after 2 iterations vs the oracle's {worst:.2e}")
        assert wll <= TOL and worst <= TOL


# ----------------------------------------------------------------------------- loopy Bethe graphs, random root

def _flags_agree(dev_flags, snap, tag):
    clear = (np.abs(snap.nh - 1e-5) > 1e-7) & (np.abs(snap.nJ - 1e-5) > 1e-7)    # not within rounding of the threshold
    assert np.array_equal(dev_flags.astype(bool)[clear], snap.flags[clear]), tag


@pytest.mark.parametrize("name,root,kind", N.LOOPY_CASES)
def test_loopy_bethe_calibration_at_every_site(P, name, root, kind):
    """Thread-per-site calibration of a LOOPY cluster graph (every sepset one variable: bp_level_uni1 / bp_chunk_uni1):
    after 1, 2 and 30 iterations of the same schedule every belief of every site against oracle.calibration.calibrate run
    the same number of iterations on that site; the residual flags agree wherever the residual is not within rounding of
    the threshold; (succ, iscal) agree."""
    for n in SIZES:
        b = N.device_batch(P, name, root, kind, "bethe", n)
        assert _thread_per_site(b.dims, n) and set(b.dims[b.pcgb.nclusters:].tolist()) == {1}
        assert b.pcgb.nsepsets > b.pcgb.nclusters - 1 and len(b.sched) >= 2, "a loopy graph"
        done = 0
        for it in N.LOOPY_STEPS:
            P.calibrate_(b.pcgb, b.sched, it - done, verbose=False, sync=False)
            done = it
            assert _site_minor(b.pcgb) == (n >= 64)
            results = [(bool(r.succ), bool(r.iscal)) for r in b.pcgb.last_results]
            b.pcgb.pull()
            worst = 0.0
            for s in range(n):
                snap = N.oracle_calibration(name, root, kind, "bethe", s, N.LOOPY_STEPS)[0][it]
                worst = max(worst, N.records_error(b.pcgb._packed_raw[s], snap.packed, b.dims))
                _flags_agree(b.pcgb._flg[s], snap, (name, n, it, s))
                clear = (np.abs(snap.nh - 1e-5) > 1e-7) & (np.abs(snap.nJ - 1e-5) > 1e-7)
                if clear.all():
                    assert results[s] == snap.got, (name, n, it, s, results[s], snap.got)
            print(f"loopy Bethe {name}/{root}/{kind}/{n} sites, {it} iterations: beliefs vs the oracle's, worst of all sites {worst:.2e}")
            assert worst <= TOL


@pytest.mark.parametrize("name,root,kind", N.LOOPY_CASES)
def test_loopy_bethe_auto_stops_each_site_where_the_c_engine_does(P, name, root, kind):
    """calibrate_(auto=True): iter_reached / tree_reached of every site equal the plain-C engine's run on that site alone
    (as test_gpu_parity.py checks multi-site networks), and so do the beliefs it stopped at."""
    from oracle import cengine
    for n in SIZES:
        b = N.device_batch(P, name, root, kind, "bethe", n)
        dims, sepcl, so, si = N.engine_arrays(P, b.ocgb0)
        P.calibrate_(b.pcgb, b.sched, 60, auto=True, verbose=False)
        b.pcgb.pull()
        seen = set()
        for s in range(n):
            ce = cengine.Engine(dims, sepcl, so, si, N.oracle_factors(name, root, kind, "bethe", s))
            reached = None
            for it in range(1, 61):
                for j, spt in enumerate(b.sched, start=1):
                    succ, iscal = ce.calibrate(spt[2], spt[3], 1, return_iscal=True)
                    assert succ
                    if iscal:
                        reached = (it, j)
                        break
                if reached:
                    break
            r = b.pcgb.last_results[s]
            assert reached and (r.succ, r.iscal) == (1, 1) and (r.iter_reached, r.tree_reached) == reached, (name, n, s, reached, (r.iter_reached, r.tree_reached))
            ref = ce.packed()
            assert N.records_error(b.pcgb._packed_raw[s], ref, dims) <= TOL, (name, n, s)
            seen.add(reached)
        print(f"auto {name}/{root}/{kind}/{n} sites: stops at {sorted(seen)}")


# ----------------------------------------------------------------------------- sweeps on the 64-site N1 batch, clique tree

def test_sweeps_on_the_64_site_n1_batch(P):
    """edge_gradient_lg at sites 0, 31 and 63 against edge_ref (the first dgamma of a real inheritance in the site-minor
    layout) and loo_lg -- the hybrid tip among its tips -- against loo_ref.dense_loo."""
    import loo_ref as LR
    from edge_ref import dense_edge_gradient, rel_block_nan
    from test_gpu_edge_gradient import BLOCKS, _device_layout, _oracle_order
    b = N.device_batch(P, "N1", "fixed", "bm", "cliquetree", 64)
    spt = b.sched[0]
    ll, got = b.pcgb.loglik_and_edge_gradient_lg(spt, all_sites=True)
    assert not got["info"].any()
    order = _oracle_order(b.net, b.ocgb0)
    f = int(np.flatnonzero(b.fam["n_parents"] >= 2)[0])
    for s in (0, 31, 63):
        model, tbl = b.sites[s]
        dense = OD.loglik(b.net, model, tbl, b.taxa)
        assert abs(ll[s] - dense) <= TOL * max(1.0, abs(dense))
        want = _device_layout(dense_edge_gradient(b.net, model, tbl, b.taxa), order, False)
        assert np.all(np.isfinite(want["dgamma"][f])) and np.all(np.abs(want["dgamma"][f]) > 1e-6)
        for k in BLOCKS:
            err = rel_block_nan(got[k][s], want[k])
            print(f"N1/64 sites, site {s}, {k}: {err:.2e}")
            assert err <= TOL, (s, k, got[k][s], want[k])
    ll2, d = b.pcgb.loo_and_loglik_lg(spt, all_sites=True)
    assert ll2.tobytes() == ll.tobytes() and not d["info"].any()
    rows = b.pcgb._lg["data_row"][d["families"]]
    assert b.taxa.index("H1") in [int(r) for r in rows]
    for s in (0, 31, 63):
        model, tbl = b.sites[s]
        one = {k: (v if k == "families" else v[s]) for k, v in d.items()}
        err = LR.worst_error(rows, one, LR.dense_loo(b.net, model, tbl, b.taxa), 1)
        print(f"N1/64 sites, site {s}, leave-one-out of {len(rows)} tips (the hybrid tip included): {err:.2e}")
        assert err <= TOL


# ----------------------------------------------------------------------------- the same input class off the thread-per-site path

def test_hybrid_tip_with_two_traits_on_one_site(P):
    """One site, p = 2, N1 with a random root: a tip family with two parents reaches the wave-per-task kernels nowhere else.
    Fill records against the oracle, loglik_lg against the dense value, loo_lg of every tip (the hybrid tip among them) and
    impute_lg with one trait of H1 missing against their dense comparators."""
    import impute_ref as IR
    import loo_ref as LR
    from test_gpu_gradient import _device
    rng = np.random.default_rng(2)
    net, taxa = N.network("N1")
    model = LR.bm(2, rng, "random")
    tbl = [[float(x) for x in rng.normal(size=len(taxa))] for _ in range(2)]
    cg, ocgb, pcgb, spt = _device(P, net, model, tbl, taxa)
    pcgb.pull()
    dims = [b.dimension for b in ocgb.belief]
    fill = N.records_error(pcgb._packed_raw[0], N.pack(ocgb), dims)
    ll, d = pcgb.loo_and_loglik_lg(spt)
    dense = OD.loglik(net, model, tbl, taxa)
    rows = pcgb._lg["data_row"][d["families"]]
    assert taxa.index("H1") in [int(r) for r in rows]
    loo = LR.worst_error(rows, d, LR.dense_loo(net, model, tbl, taxa), 2)
    print(f"N1, p = 2, one site: fill {fill:.2e}, loglik {abs(ll - dense) / max(1.0, abs(dense)):.2e}, leave-one-out {loo:.2e}")
    assert fill <= TOL and abs(ll - dense) <= TOL * max(1.0, abs(dense)) and loo <= TOL
    tbl[1][taxa.index("H1")] = None
    cg, ocgb, pcgb, spt = _device(P, net, model, tbl, taxa)
    ll, d = pcgb.impute_and_loglik_lg(spt)
    dense = OD.loglik(net, model, tbl, taxa)
    assert IR.counts(tbl, d) == (1, 1), IR.counts(tbl, d)
    imp = IR.worst_error(d, IR.dense_impute(net, model, tbl, taxa), symmetric=True)
    print(f"N1, p = 2, one site, trait 2 of H1 missing: loglik {abs(ll - dense) / max(1.0, abs(dense)):.2e}, imputed value {imp:.2e}")
    assert abs(ll - dense) <= TOL * max(1.0, abs(dense)) and imp <= TOL

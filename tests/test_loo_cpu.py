"""The leave-one-out sweep, host side (no GPU): the numpy restatement of the device sweep on the ORACLE's calibrated clique
tree (loo_ref.loo_sweep: J^-1 h and J^-1 of each tip family's cluster) against the dense comparator (loo_ref.dense_loo:
oracle/densemvn.py alone, no message passing), on every case test_gpu_loo.py runs.  1e-8 relative to the largest entry of a
block (the project's parity bound).  This pins the identity D = V - S, cov = V D^-1 V, mean = y - V D^-1 r,
lpd = -(o log 2pi + 2 log det V - log det D + r' D^-1 r) / 2 to an independent computation, and shows that the inputs the
GPU tests use are well enough conditioned (V - S does not cancel).  Measured worst error over all cases: see the printed
figures (below 1e-10 everywhere)."""
import numpy as np
import pytest

import loo_ref as LR


def _check(tag, net, model, tbl, taxa, tips=None):
    rows, d = LR.oracle_loo(net, model, tbl, taxa)
    dense = LR.dense_loo(net, model, tbl, taxa, tips)
    want_rows = sorted({r for r in range(len(taxa)) if any(col[r] is not None for col in tbl)})
    assert sorted(int(r) for r in rows) == want_rows          # a tip family per tip with data, no other
    assert not d["info"].any()
    err = LR.worst_error(rows, d, dense, model.dimension())
    print(f"{tag}: sweep on oracle beliefs vs dense comparator {err:.2e} over {len(dense)} tips")
    assert err <= 1e-8, tag
    assert d["total"] == LR.tree_total(d["lpd"]) and abs(d["total"] - float(np.sum(d["lpd"]))) <= 1e-12 * abs(d["total"])
    return d


@pytest.mark.parametrize("name,root", LR.REFERENCE)
def test_loo_reference_networks(name, root):
    _check(f"{name}/{root}", *LR.reference_case(name, root))


@pytest.mark.parametrize("which,p", LR.RANDOM)
def test_loo_random_networks(which, p):
    _check(f"{which}/p{p}", *LR.random_case(which, p))


def test_loo_missing_values():
    net, model, tbl, taxa = LR.missing_case()
    d = _check("missing/p3", net, model, tbl, taxa)
    assert len(d["families"]) == len(taxa) and np.isnan(d["mean"]).any()
    for root in ("random", "fixed"):   # (improper: the prediction of A is y_C = 0 exactly, no relative error to measure)
        net, model, tbl, taxa = LR.no_data_case(root)
        d = _check(f"exact_reml_missing/{root}", net, model, tbl, taxa)
        assert 0 < len(d["families"]) < len(taxa)              # a tip without any value is not a tip family


def test_loo_wavefront_case():
    _check("tree/p16", *LR.wavefront_case())


@pytest.mark.parametrize("p", [1, 2])
def test_loo_batch_sites(p):
    for s in (0, 31, 63):
        _check(f"batch/p{p}/site{s}", *LR.batch_site(p, s))


def test_loo_star_tree_total_is_the_loglikelihood():
    """Fixed root, star tree: the tips are independent given the root, every S = 0 and sum lpd = loglik."""
    from oracle import densemvn as OD
    net, model, tbl, taxa = LR.star_case()
    d = _check("star", net, model, tbl, taxa)
    ll = OD.loglik(net, model, tbl, taxa)
    assert abs(d["total"] - ll) <= 1e-12 * abs(ll)


def test_loo_two_tips_improper_root():
    """Complete data: the other tip determines the root and the prediction is proper (against the dense comparator).  Tips
    observed at disjoint traits: the other tip leaves the root's matching trait flat, D = V - S is singular: info 1, NaN."""
    _check("two tips, complete", *LR.two_tip_complete_case())
    rows, d = LR.oracle_loo(*LR.two_tip_case())
    assert len(rows) == 2 and np.all(d["info"] == 1)
    assert np.isnan(d["lpd"]).all() and np.isnan(d["mean"]).all() and np.isnan(d["cov"]).all() and np.isnan(d["total"])

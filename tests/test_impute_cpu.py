"""The imputation sweep, host side (no GPU): the numpy restatement of the device sweep on the ORACLE's calibrated clique tree
(impute_ref.impute_sweep: J^-1 h and J^-1 of each listed family's cluster) against the dense comparator
(impute_ref.dense_impute: oracle/densemvn.py alone, no message passing), on every case test_gpu_impute.py runs.  1e-8
relative to the largest entry of a block (the project's parity bound).  This pins
    B = V_PO V_OO^-1,  mean = E[u_P] + w_P + B (y_O - w_O - E[u_O]),  cov = [-B I] Cov(u_Z) [-B I]' + V_PP - B V_OP
to an independent computation.  Every case also asserts its exact counts of (missing entries, predicted entries): a
comparison cannot pass by predicting nothing.  The measured worst error of every case is printed (below 1e-12 everywhere)."""
import numpy as np
import pytest

import impute_ref as IR
import loo_ref as LR


def _check(tag, net, model, tbl, taxa, want_counts):
    d, fam = IR.oracle_impute(net, model, tbl, taxa)
    assert IR.counts(tbl, d) == want_counts, (tag, IR.counts(tbl, d), want_counts)
    err = IR.worst_error(d, IR.dense_impute(net, model, tbl, taxa))
    print(f"{tag}: sweep on oracle beliefs vs dense comparator {err:.2e} over {int(d['predicted'].sum())} entries")
    assert err <= 1e-8, tag
    return d, fam


@pytest.mark.parametrize("root,counts", IR.MISSING_ROOTS)
def test_impute_missing_case(root, counts):
    _check(f"missing/p3/{root}", *IR.missing_case(root), counts)


@pytest.mark.parametrize("which,p,seed,frac,counts", IR.MASKED)
def test_impute_masked_random_networks(which, p, seed, frac, counts):
    _check(f"{which}/p{p}/seed{seed}", *IR.masked_random_case(which, p, seed, frac), counts)


@pytest.mark.parametrize("root", ["fixed", "random"])
def test_impute_tips_without_data(root):
    """Two tips without any value under a parent that holds nothing in scope: listed, nothing predicted, info -1; the
    internal node with nothing in scope is not listed."""
    net, model, tbl, taxa = LR.no_data_case(root)
    d, fam = _check(f"exact_reml_missing/{root}", net, model, tbl, taxa, (2, 0))
    assert len(d["families"]) == 2 and not d["predicted"].any() and np.all(d["info"] == -1)
    assert np.isnan(d["mean"]).all() and np.isnan(d["cov"]).all()
    assert np.all(fam["data_row"][d["families"]] >= 0)
    assert np.sum((fam["child_pos"] < 0) & (fam["data_row"] < 0)) >= 1      # the internal node: not a tip


def test_impute_wavefront_and_workgroup_trees():
    for args, counts in (IR.WAVEFRONT, IR.WORKGROUP):
        _check("tree" + str(args), *IR.tree_case(*args), counts)


def test_impute_wavefront_tree_with_every_trait_in_scope():
    """tree(12, 16, 0, 0.1) set up with every trait of every internal node in scope (the set-up under which the engine packs
    it): every cluster has 16 or 32 variables, all 22 missing entries are predicted, and the restatement on the dense
    posterior moments of those clusters agrees with the dense comparator."""
    case = IR.tree_case(*IR.WAVEFRONT[0])
    su = IR.full_scope_setup(*case)
    assert sorted(set(int(m) for m in su["arrays"][0])) == [16, 32]
    d = IR.impute_sweep(su["fam"], su["data"], su["kw"]["R"], su["kw"]["mu"], IR.dense_cluster_moments(*case, su))
    assert IR.counts(case[2], d) == (22, 22)
    err = IR.worst_error(d, IR.dense_impute(*case))
    print(f"tree/p16, every trait in scope: sweep on dense cluster moments vs dense comparator {err:.2e}")
    assert err <= 1e-8


def test_impute_packed_case():
    """Every parent keeps its full scope: every cluster has 16 or 32 variables (what the packed layout needs)."""
    d, fam = _check("tree/p16/packed", *IR.packed_case(), IR.PACKED_COUNTS)
    assert np.all(fam["parent_mask"] == np.uint64(2 ** 16 - 1)) and (fam["child_mask"][d["families"]] == 0).any()


def test_impute_complete_data_lists_nothing():
    net, model, tbl, taxa = LR.random_case("bm_random", 4)
    d, fam = IR.oracle_impute(net, model, tbl, taxa)
    assert len(d["families"]) == 0 and fam.get("child_mask") is None


def test_impute_batch_sites():
    """The batch pattern masks at most one tip of any cherry: it sets up in the oracle, every parent keeps its full scope
    (every missing entry is predicted), and sites 0, 31 and 63 agree with the dense comparator."""
    miss = IR.batch_pattern(2)
    assert miss.any(axis=1).sum() >= 5 and miss.all(axis=1).any() and (miss[:, 0] & ~miss[:, 1]).any()
    for s in (0, 31, 63):
        net, model, tbl, taxa = IR.batch_site(2, s)
        d, fam = _check(f"batch/site{s}", net, model, tbl, taxa, (int(miss.sum()), int(miss.sum())))
        full = np.uint64(3)
        assert np.all(fam["parent_mask"] == full)

"""The scan of every edge for a mean shift, host side (no GPU): the dense statement scan_ref.family_scan -- what the device
sweep pgbp_lg_shift_scan is compared with in test_gpu_shift_scan.py -- pinned to one-edge dense GLS (scan_ref.gls_edge) and
to the dense oracle's log-likelihood on the eight cases of test_shift_cpu.CASES, every edge of every case.

(a) edge_jump = jump / gamma, gamma^2 H and lr against the one-edge GLS restricted to the traits the scan keeps, and
    lr = 2 (loglik at the GLS fit - loglik without it) of densemvn;
(b) the same with two shifts in force: the increment to that edge's shift, the others held;
(c) the missing-data cases yield families with exactly one identified trait, and the relative pivots leave a wide gap
    between what is dropped (rounding) and what is kept;
(d) the skip rule on a hand-made H with a zero direction.
Everything at 1e-8 relative to the largest entry of the block; the measured figures are printed."""
import numpy as np
import pytest

from scan_ref import dense_scan, gls_edge, restricted_solve, skip_cholesky
from shift_ref import fit_edges
from test_gradient_cpu import rel_block
from test_shift_cpu import CASES, IDS

TOL = 1e-8


def _against_gls(name, net, model, tbl, taxa, held):
    """Every parent edge of every node: the scan under `held` against gls_edge.  jump and H per edge, each relative to its
    own largest entry; lr as one block over the edges (a difference of two log-likelihoods carries their rounding).
    Returns the scan."""
    sc = dense_scan(net, model, held, tbl, taxa)
    worst = dict(jump=0.0, H=0.0)
    lr_scan, lr_gls, lr_ll = [], [], []
    for i in range(1, len(net.vec_node)):
        ks = np.flatnonzero(sc["identified"][i])
        if ks.size == 0:
            assert sc["lr"][i] == 0.0 and np.all(np.isnan(sc["jump"][i]))
            continue
        assert np.all(np.isnan(np.delete(sc["jump"][i], ks)))
        for ed in sc["edges"][i]:
            inc, H, ll1, ll0 = gls_edge(net, model, tbl, taxa, ed, ks, held)
            worst["jump"] = max(worst["jump"], rel_block(sc["jump"][i][ks] / ed.gamma, inc))
            worst["H"] = max(worst["H"], rel_block(ed.gamma ** 2 * sc["H"][i][np.ix_(ks, ks)], H))
            lr_scan.append(sc["lr"][i])
            lr_gls.append(float(inc @ H @ inc))
            lr_ll.append(2.0 * (ll1 - ll0))
    worst["lr_vs_gls"] = rel_block(lr_scan, lr_gls)
    worst["lr_vs_2dloglik"] = rel_block(lr_scan, lr_ll)
    print(f"{name}, {len(held)} shifts held, {len(lr_scan)} edges: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (name, k, v)
    return sc


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scan_is_the_restricted_one_edge_gls(case):
    name, net, model, tbl, taxa = case
    sc = _against_gls(name, net, model, tbl, taxa, {})
    # both parent edges of a hybrid: one lr, jumps in the ratio of their gamma (by construction of edge_jump); the gap of the
    # rule: what is dropped is rounding, what is kept is far above min_info
    rel = sc["relpivot"][1:]
    kept = sc["identified"][1:]
    if (~kept).any():
        assert np.max(np.abs(rel[~kept])) <= 1e-13
    assert np.min(rel[kept]) >= 1e-3
    print(f"{name}: relative pivots kept >= {np.min(rel[kept]):.2e}, dropped <= "
          f"{np.max(np.abs(rel[~kept])) if (~kept).any() else 0.0:.2e}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scan_under_shifts_is_the_increment(case):
    """Two shifts in force (one of them far from its optimum): every edge's scan is the GLS increment with the others held;
    for the shifted edges themselves it is the increment to their own shift."""
    name, net, model, tbl, taxa = case
    e = fit_edges(net, model)
    rng = np.random.default_rng(21)
    held = {int(e[0].number): rng.normal(size=model.dimension()), int(e[3].number): 3.0 + rng.normal(size=model.dimension())}
    _against_gls(name, net, model, tbl, taxa, held)


def test_missing_data_gives_partly_identified_families():
    n_one = 0
    for name, net, model, tbl, taxa in CASES:
        if not name.startswith("missing"):
            continue
        sc = dense_scan(net, model, {}, tbl, taxa)
        dof = sc["identified"][1:].sum(axis=1)
        assert (dof == 1).any(), name
        n_one += int((dof == 1).sum())
        for i in np.flatnonzero(dof == 1) + 1:   # the dropped trait's entries are NaN, the kept one's are numbers
            k = int(np.flatnonzero(sc["identified"][i])[0])
            assert np.isfinite(sc["jump"][i, k]) and np.isnan(sc["jump"][i, 1 - k])
            assert np.isfinite(sc["H"][i, k, k]) and np.isnan(sc["H"][i, 1 - k, 1 - k]) and np.isnan(sc["H"][i, 0, 1])
    print(f"families with exactly one identified trait in the two missing-data cases: {n_one}")
    assert n_one >= 2


def test_skip_rule_on_a_zero_direction():
    """H = B diag(2, 0, 1) B' with B unit lower triangular: in index order trait 1 has pivot 0 given trait 0 and is dropped;
    the solve is the 2 x 2 one on traits 0 and 2.  With every trait kept (H + I) it is the full solve."""
    B = np.array([[1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [-0.25, 2.0, 1.0]])
    H = B @ np.diag([2.0, 0.0, 1.0]) @ B.T
    g = np.array([1.0, -2.0, 0.5])
    scale = np.ones(3)
    kept, L, rel = skip_cholesky(H, scale, 1e-8)
    assert kept.tolist() == [True, False, True] and abs(rel[1]) <= 1e-15
    assert np.all(L[1] == 0.0) and np.all(L[:, 1] == 0.0)
    ks = [0, 2]
    assert np.allclose(L[np.ix_(ks, ks)] @ L[np.ix_(ks, ks)].T, H[np.ix_(ks, ks)], rtol=0, atol=1e-15)
    kept, d, lr, _ = restricted_solve(H, g, scale, 1e-8)
    want = np.linalg.solve(H[np.ix_(ks, ks)], g[ks])
    assert np.isnan(d[1]) and np.allclose(d[ks], want, rtol=1e-14) and abs(lr - g[ks] @ want) <= 1e-14 * abs(lr)
    # min_info above a kept pivot's share drops that trait too and moves the other to its own one-trait fit
    kept1, d1, lr1, _ = restricted_solve(H, g, np.array([1.0, 1.0, 1e3]), 0.5)   # trait 2 now needs a pivot above 500
    assert kept1.tolist() == [True, False, False] and np.all(np.isnan(d1[1:]))
    assert abs(d1[0] - g[0] / H[0, 0]) <= 1e-15 and abs(lr1 - g[0] ** 2 / H[0, 0]) <= 1e-15
    # nothing kept: lr 0, all NaN
    kept0, d0, lr0, _ = restricted_solve(np.zeros((2, 2)), np.ones(2), np.ones(2), 0.0)
    assert not kept0.any() and np.all(np.isnan(d0)) and lr0 == 0.0
    kept, d, lr, _ = restricted_solve(H + np.eye(3), g, scale, 1e-8)
    assert kept.all() and np.allclose(d, np.linalg.solve(H + np.eye(3), g), rtol=1e-13)

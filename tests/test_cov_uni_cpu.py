"""The comparator of pgbp_posterior_cov_sites (tests/cov_uni_ref.py: the numpy restatement of w, k and the block-ordered gram in
site-minor rows) pinned to independent statements, on the oracle's calibrated clique tree of every case
tests/test_gpu_cov_uni.py uses, one site in eight, at 1e-8 relative to max(1, |block|_inf):
  * w and k against cov_ref.posterior_cov_ref, the restatement of the general call (numpy's Cholesky and solves);
  * with c = I, k and w w' against the dense posterior covariance of all node states (post_uni_ref.dense_posterior: the
    oracle), on every pair of entries;
  * gram against w w' from numpy, and its packing and block order against a plain statement.
It also asserts, from the reference alone, the condition the GPU tolerances rely on: the smallest pivot of a conditional J_RR
relative to its diagonal entry (post_uni_ref.pivot_margin) over every case and checked site."""
import numpy as np
import pytest

import cov_ref as CR
import cov_uni_ref as CU
import fam_uni_ref as FR
import post_uni_ref as PR

TOL = 1e-8
CASES = [(c, max(counts)) for c, counts, _ in PR.cases()]
# The floor is the figure test_post_uni_cpu.py records for these cases, 8.0e-2 to the two digits it is stated with: computed here
# it is 7.987e-02 (ou/improper, site 0; that file prints it as 7.99e-02), so the margin is compared at that precision.  A new
# case below it is changed, not the bound.
PIVOT_FLOOR = 8.0e-2


def _margin_ok(pivot):
    return float(f"{pivot:.1e}") >= PIVOT_FLOOR

_DONE = {}


def _pin_site(case, s):
    """(worst errors, smallest relative pivot) of one site of a case; computed once"""
    if (case.name, s) in _DONE:
        return _DONE[case.name, s]
    ocgb, fam, data, kw = FR.oracle_site(case, s)
    dims, sepcl, soff, sidx, vn, off = PR.layout(case)
    nc = ocgb.nclusters
    rec = PR.records_of(ocgb)[:nc]
    D = int(off[-1])
    pa, ch = case.spt[2], case.spt[3]
    c = np.vstack([np.eye(D), CU.functionals(D)])
    w, k, info = CU.cov_rows(rec, dims, sepcl, soff, sidx, pa, ch, c)
    rw, rk, rinfo = CR.posterior_cov_ref(rec, dims, sepcl, soff, sidx, pa, ch, c)
    assert info == 0 and rinfo == 0 and not np.isnan(w).any() and not np.isnan(k).any()
    worst = dict(w=FR.rel(w, rw), k=FR.rel(k, rk))
    _, pc = PR.dense_posterior(case, s)
    flat = np.array([n for n, _ in vn], dtype=int)
    dense = pc[np.ix_(flat, flat)]
    worst["k, c = I"] = FR.rel(k[:D], dense)
    worst["w w', c = I"] = FR.rel(w[:D] @ w[:D].T, dense)
    worst["k symmetric"] = FR.rel(k[:D], k[:D].T)
    tri = CU.gram_rows(w[D:, :, None])
    worst["gram"] = FR.rel(CU.gram_full(tri, 3)[0], w[D:] @ w[D:].T)
    worst["gram, dense"] = FR.rel(CU.gram_full(tri, 3)[0], c[D:] @ dense @ c[D:].T)
    # structure: +0.0 (sign bit included) where the sampler conditions, a shared variable the same bits in every copy
    spos = CR.s_positions(dims, sepcl, soff, sidx, pa, ch, nc)
    assert np.all(w[:, spos] == 0.0) and not np.signbit(w[:, spos]).any()
    first = {}
    for e, nt in enumerate(vn):
        if nt in first:
            assert k[:, e].tobytes() == k[:, first[nt]].tobytes()
        else:
            first[nt] = e
    pivot = PR.pivot_margin(rec, dims, sepcl, soff, sidx, pa, ch)
    _DONE[case.name, s] = worst, pivot, D
    return _DONE[case.name, s]


def _pin(case, sites):
    worst, pivot, D = {}, np.inf, 0
    for s in sites:
        w, pv, D = _pin_site(case, s)
        pivot = min(pivot, pv)
        for key, val in w.items():
            worst[key] = max(worst.get(key, 0.0), val)
    print(f"{case.name}: size {D}: " + ", ".join(f"{key} {v:.2e}" for key, v in worst.items()) + f"; smallest relative pivot {pivot:.3e}")
    for key, v in worst.items():
        assert v <= TOL, (case.name, key, v)
    return pivot, D


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c, _ in CASES])
def test_restatement_against_the_general_restatement_and_the_dense_oracle(i):
    case, n = CASES[i]
    pivot, _ = _pin(case, FR.checked_sites(n))
    assert _margin_ok(pivot), pivot


@pytest.mark.parametrize("shape,n", CU.SHAPES)
def test_shape_cases(shape, n):
    """63, 64, 65 and 130 families, the caterpillar and the balanced tree, and the trees whose layout size falls on either side
    of a multiple of 64 entries (63 | 66, 191 | 192 | 194): sites 0 and 56"""
    pivot, D = _pin(PR.shape_case(shape, n), (0, 56))
    assert CU.SIZES.get((shape, n), D) == D, (shape, n, D)
    assert _margin_ok(pivot), pivot


def test_layout_sizes_on_both_sides_of_a_block_boundary():
    sizes = sorted(CU.SIZES.values())
    print("layout sizes of the block-boundary trees:", sizes)
    for mult in (64, 192):
        assert any(s == mult - 1 for s in sizes) and any(mult <= s <= mult + 2 for s in sizes)
    assert 192 in sizes


def test_margin_of_the_gpu_tests():
    """the smallest pivot of a conditional J_RR relative to its diagonal entry, over every case and checked site the GPU file
    uses; far from the 0 at which the device's tests `> 0` could fall either way"""
    pivot = np.inf
    for case, n in CASES:
        for s in FR.checked_sites(n):
            pivot = min(pivot, _pin_site(case, s)[1])
    for sh in CU.SHAPES:
        for s in (0, 56):
            pivot = min(pivot, _pin_site(PR.shape_case(*sh), s)[1])
    print(f"margin: smallest relative pivot {pivot:.4e}")
    assert _margin_ok(pivot), pivot


def test_gram_rows_packing_and_block_order():
    """the pair (a <= b) sits at b (b + 1) / 2 + a; the sum is per block of 64 entries, then over the blocks: with entries chosen
    so that the order of the additions shows in the last bit, a plain left-to-right sum differs and the blocked one is met"""
    rng = np.random.default_rng(7)
    w = rng.standard_normal((3, 130, 5)) * 10.0 ** rng.integers(-6, 6, (3, 130, 5))
    tri = CU.gram_rows(w)
    assert tri.shape == (6, 5)
    for b in range(3):
        for a in range(b + 1):
            want = np.zeros(5)
            for lo, hi in ((0, 64), (64, 128), (128, 130)):
                acc = np.zeros(5)
                for e in range(lo, hi):
                    acc = acc + w[a, e] * w[b, e]
                want = want + acc
            assert tri[b * (b + 1) // 2 + a].tobytes() == want.tobytes()
    plain = np.zeros(5)
    for e in range(130):
        plain = plain + w[0, e] * w[1, e]
    assert plain.tobytes() != tri[1].tobytes()
    G = CU.gram_full(tri, 3)
    assert G.shape == (5, 3, 3) and np.array_equal(G, G.transpose(0, 2, 1)) and np.array_equal(G[:, 0, 2], tri[3])


def test_restatement_reports_what_is_planted():
    """the first cluster in preorder whose J_RR is not positive definite, all NaN, as the general restatement"""
    case = FR.bm_case()
    ocgb, fam, data, kw = FR.oracle_site(case, 0)
    dims, sepcl, soff, sidx, vn, off = PR.layout(case)
    nc = ocgb.nclusters
    rec = PR.records_of(ocgb)[:nc]
    order = [int(case.spt[2][0])] + [int(c) for c in case.spt[3]]
    bad = list(rec)
    for cl in (order[5], order[2]):
        J = rec[cl][0].copy()
        J[:] = -1.0
        bad[cl] = (J, rec[cl][1], rec[cl][2])
    c = CU.functionals(int(off[-1]))
    w, k, info = CU.cov_rows(bad, dims, sepcl, soff, sidx, case.spt[2], case.spt[3], c)
    rw, rk, rinfo = CR.posterior_cov_ref(bad, dims, sepcl, soff, sidx, case.spt[2], case.spt[3], c)
    assert info == rinfo == order[2] + 1 and np.isnan(w).all() and np.isnan(k).all()
    ws, ks, tri, infos = CU.posterior_cov_sites_rows([rec, bad, rec], dims, sepcl, soff, sidx, case.spt[2], case.spt[3], c)
    assert infos.tolist() == [0, order[2] + 1, 0] and np.isnan(tri[:, 1]).all() and not np.isnan(tri[:, [0, 2]]).any()
    assert ws[:, :, 0].tobytes() == ws[:, :, 2].tobytes() and tri[:, 0].tobytes() == tri[:, 2].tobytes()

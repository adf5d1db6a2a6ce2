"""The comparators of test_gpu_rate_uni.py pinned to each other, without a GPU: the numpy restatement U'U of rate_uni_ref.py
against dense generalised least squares -- Y'PY with P from the tips' covariance of oracle.densemvn -- and the rate matrix
against Y_c' C^-1 Y_c / (n - 1), on trees of 2, 3, 12 (caterpillar and balanced), 30 and 40 tips, with tips without data at
every site (a shared child_mask) and with shifts, per site and shared.  Also the margins the GPU tests lean on: the smallest
den, and the eigengap of the PCA case.  Every comparison at 1e-8 relative to max(1, |block|_max)."""
import numpy as np
import pytest

import exact_uni_ref as XR
import fam_uni_ref as FR
import rate_uni_ref as RR

TOL = 1e-8


@pytest.mark.parametrize("key,n", RR.CPU_CASES, ids=[f"{k}-{n}" for k, n in RR.CPU_CASES])
def test_restatement_against_dense_gls(key, n):
    """U'U = Y'PY on every pair of sites, and U'U / (n_obs - 1) = Y_c' C^-1 Y_c / (n_obs - 1)"""
    g = RR.gls(key, n)
    G = RR.gram(key, n)
    den = g["n_obs"] - 1.0
    worst = dict(gram=FR.rel(G, g["gram"]), R=FR.rel(G / den, g["R"]), sym=float(np.max(np.abs(G - G.T))))
    print(f"{key}/{n}: {RR.U(key, n).shape[0]} families, {g['n_obs']} observed tips: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert worst["gram"] <= TOL and worst["R"] <= TOL
    assert den >= 1.0


def test_the_diagonal_is_the_per_site_num():
    """the diagonal of the restatement is num of exact_uni_ref's restatement of the per-site sweep"""
    for key, n in (("bm40", 17), ("shifts", 17)):
        ref = XR.reference(key, n)
        assert FR.rel(np.diagonal(RR.gram(key, n)), ref["num"]) <= TOL
        assert FR.rel(ref["den"], np.full(n, RR.gls(key, n)["n_obs"] - 1.0)) <= TOL


def test_smallest_den():
    """every case of the GPU tests observes at least two tips: den >= 1"""
    low = min(RR.gls(k, min(n, 8))["n_obs"] - 1 for k, n in RR.SITE_CASES + RR.FAMILY_CASES + RR.OTHER_CASES)
    print(f"smallest den over the GPU cases: {low}")
    assert low >= 1


@pytest.mark.parametrize("mode", ["cov", "corr"])
def test_pca_eigengap(mode):
    """the components the GPU test compares are separated: relative eigengap at least 1e-3, so loadings compare up to sign"""
    key, n = RR.PCA_CASE
    g = RR.gls(key, n)
    A = g["R"] if mode == "cov" else g["R"] / np.sqrt(np.outer(np.diagonal(g["R"]), np.diagonal(g["R"])))
    gap = RR.eigengap(A, RR.PCA_K)
    print(f"{key}/{n}, {mode}: smallest relative gap of the first {RR.PCA_K + 1} eigenvalues {gap:.3e}")
    assert gap >= 1e-3
    w, V, Z = RR.pca(A, g["Yc"], RR.PCA_K)
    assert np.all(np.diff(w) < 0) and np.allclose(V.T @ V, np.eye(RR.PCA_K), atol=1e-12)
    assert np.allclose(RR.aligned(-V, V), V)

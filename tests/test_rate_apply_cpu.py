"""The comparators of test_gpu_rate_apply_uni.py pinned without a GPU, and exact.leading_eigenpairs as the pure numpy function
of its callback that it is.

1. rate_apply_ref.apply -- U'(U V) of the restatement -- against (Y'PY) V of dense GLS on the trees of test_rate_uni_cpu.py,
   the shared-mask case (three tips without data) and the shifted cases among them.
2. leading_eigenpairs with a dense apply on planted spectra (four Brownian factors of variance shares 8, 4, 2, 1, noise 0.05,
   the 30- and the 40-tip tree at 64 and 257 sites, rate matrix and correlations) against numpy.linalg.eigh: eigenvalues
   within 1e-8 lambda_1, sign-fixed vectors within 1e-8 absolute.  The margins this rests on are computed and asserted: the
   relative gaps of the first k + 1 eigenvalues are at least 0.05, so that a residual of rtol lambda_1 = 1e-10 lambda_1 bounds
   the vector error by rtol / gap = 2e-9 (Davis-Kahan); lambda_{block+1} / lambda_k <= 0.5; convergence within 100 of the 200
   iterations.
3. A matrix of rank below the block (the 2-tip tree: rank 1) terminates converged; k = n and block > n are clamped; not
   converging is reported, not raised."""
import numpy as np
import pytest

import fam_uni_ref as FR
import rate_apply_ref as AR
import rate_uni_ref as RR
from pgbp_amd.exact import leading_eigenpairs

TOL = 1e-8


@pytest.mark.parametrize("key,n", RR.CPU_CASES, ids=[f"{k}-{n}" for k, n in RR.CPU_CASES])
def test_restatement_times_v_against_dense_gls(key, n):
    """U'(U V) = (Y'PY) V for 1, 5 and n vectors"""
    rng = np.random.default_rng(2501)
    worst = 0.0
    for k in (1, 5, n):
        V = rng.standard_normal((n, k))
        worst = max(worst, FR.rel(AR.apply(key, n, V), AR.gls_apply(key, n, V)))
    print(f"{key}/{n}: U'(U V) against (Y'PY) V: {worst:.1e}")
    assert worst <= TOL


PLANTED = [(nt, n, m) for nt, n in AR.PLANTED for m in ("cov", "corr")]


@pytest.mark.parametrize("ntips,n,mode", PLANTED, ids=[f"{a}tips-{b}-{m}" for a, b, m in PLANTED])
def test_leading_eigenpairs_on_planted_spectra(ntips, n, mode):
    A, _ = AR.matrix(AR.planted_gls(ntips, n), mode)
    gap, tail = AR.margins(A)
    w, V = np.linalg.eigh(A)
    order = np.argsort(w)[::-1][: AR.K]
    w, V = w[order], V[:, order]
    got = leading_eigenpairs(lambda Q: A @ Q, n, AR.K)
    dv = float(np.max(np.abs(got["values"] - w)) / w[0])
    dx = float(np.max(np.abs(RR.aligned(got["vectors"], V) - V)))
    print(f"planted {ntips} tips / {n} sites, {mode}: smallest relative gap {gap:.3f}, lambda_{AR.BLOCK + 1} / lambda_{AR.K} {tail:.1e}, "
          f"{got['iterations']} iterations, worst residual / lambda_1 {np.max(got['residuals']) / w[0]:.1e}, values {dv:.1e}, vectors {dx:.1e}")
    assert gap >= 0.05 and tail <= 0.5
    assert got["converged"] and got["iterations"] <= 100
    assert np.all(got["residuals"] <= AR.RTOL * got["values"][0])
    assert dv <= TOL and dx <= TOL
    assert got["values"].shape == (AR.K,) and got["vectors"].shape == (n, AR.K) and np.all(np.diff(got["values"]) < 0)
    assert np.allclose(got["vectors"].T @ got["vectors"], np.eye(AR.K), atol=1e-12)


def test_one_apply_per_iteration_and_the_seed():
    """the callback is called once per iteration with an orthonormal [n, block] block; the same seed gives the same bytes"""
    A, _ = AR.matrix(AR.planted_gls(30, 64), "cov")
    calls = []

    def spy(Q):
        calls.append(Q.shape)
        assert np.allclose(Q.T @ Q, np.eye(Q.shape[1]), atol=1e-12)
        return A @ Q

    a = leading_eigenpairs(spy, 64, AR.K)
    b = leading_eigenpairs(lambda Q: A @ Q, 64, AR.K)
    assert len(calls) == a["iterations"] and set(calls) == {(64, AR.BLOCK)}
    assert all(np.array_equal(a[k], b[k]) for k in ("values", "vectors", "residuals"))
    c = leading_eigenpairs(lambda Q: A @ Q, 64, AR.K, seed=1)
    assert not np.array_equal(a["vectors"], c["vectors"]) and np.max(np.abs(a["values"] - c["values"])) <= TOL * a["values"][0]


def test_rank_below_the_block_terminates():
    """the gram matrix of the 2-tip tree has rank 1: the QR of a rank-deficient block does not break the iteration, which ends
    converged with values beyond the rank at rounding"""
    for n, block in ((9, None), (17, None), (17, 4)):   # block = n: one exact step; block < n: the QR of a rank-1 block is taken
        G = RR.gram("tree2", n)
        w = np.sort(np.linalg.eigvalsh(G))[::-1]
        assert w[1] <= 1e-12 * w[0]
        got = leading_eigenpairs(lambda Q: G @ Q, n, 4, block=block)
        print(f"rank 1 at {n} sites, k = 4, block {block}: {got['iterations']} iterations, values / lambda_1 {(got['values'] / w[0]).tolist()}")
        assert got["converged"] and got["iterations"] <= 100 and abs(got["values"][0] - w[0]) <= TOL * w[0]
        assert np.all(np.abs(got["values"][1:]) <= 1e-12 * w[0])
    zero = leading_eigenpairs(lambda Q: 0.0 * Q, 9, 2)
    assert zero["converged"] and not zero["values"].any()


def test_clamps_and_a_run_that_does_not_converge():
    A, _ = AR.matrix(AR.planted_gls(30, 64), "cov")
    w = np.sort(np.linalg.eigvalsh(A))[::-1]
    full = leading_eigenpairs(lambda Q: A @ Q, 64, 64)             # k = n: the block is n, one Rayleigh-Ritz step is exact
    assert full["converged"] and full["values"].shape == (64,) and np.max(np.abs(full["values"] - w)) <= TOL * w[0]
    over = leading_eigenpairs(lambda Q: A @ Q, 64, 100, block=500)  # k > n and block > n
    assert over["converged"] and over["vectors"].shape == (64, 64)
    shapes = []
    small = leading_eigenpairs(lambda Q: shapes.append(Q.shape) or A @ Q, 64, 4, block=2)   # a block below k is raised to k
    assert set(shapes) == {(64, 4)}
    short = leading_eigenpairs(lambda Q: A @ Q, 64, 4, block=4, maxiter=1)
    assert not short["converged"] and short["iterations"] == 1 and np.all(np.isfinite(short["values"]))
    assert small["iterations"] >= 1

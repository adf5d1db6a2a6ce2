"""Cases and comparators of the rate matrix applied to vectors (pgbp_bm_rate_apply_sites / bm_rate_apply_sites) and of the
leading phylogenetic principal components (leading_eigenpairs / phylo_pca_leading_sites), host side, shared by
test_rate_apply_cpu.py and test_gpu_rate_apply_uni.py (tests only).  None of them runs the device call.

(a) `apply`: rate_uni_ref's dense statement times V -- U'(U V) with U the numpy restatement of the residual rows;
    `gls_apply`: (Y'PY) V of dense generalised least squares on the tips (rate_uni_ref.gls).
(b) `planted`: data with a planted spectrum -- four Brownian factors on the tree (draws of N(0, C), C the tips' covariance)
    whose shares of the variance are 8, 4, 2, 1, random standard-normal loadings over the sites, noise of standard deviation
    0.05 -- on the 30- and the 40-tip tree; `planted_gls`: dense GLS of such a case; `matrix`: the rate matrix or the
    evolutionary correlations of it; `margins`: the gaps the eigenvector comparison rests on."""
import functools

import numpy as np

import exact_uni_ref as XR
import rate_uni_ref as RR

AMPLITUDES = (8.0, 4.0, 2.0, 1.0)
NOISE = 0.05
K = 4               # components compared
BLOCK = 16          # leading_eigenpairs' default block at k = 4
RTOL = 1e-10
# (tips, sites): the cases of the planted spectra; the seeds were chosen so that `margins` holds (asserted in test_rate_apply_cpu.py)
PLANTED = [(30, 64), (30, 257), (40, 64), (40, 257)]
SEED = {(30, 64): 3, (30, 257): 1, (40, 64): 1, (40, 257): 1}


def apply(key, n, V):
    """U'(U V) over the first n sites of case `key`"""
    u = RR.U(key, n)
    return u.T @ (u @ V)


def gls_apply(key, n, V):
    return RR.gls(key, n)["gram"] @ V


@functools.lru_cache(maxsize=None)
def planted(ntips, n):
    """the improper-root case of the 30- or the 40-tip tree with n sites of planted data"""
    base = XR.random30() if ntips == 30 else XR.tree40()
    rng = np.random.default_rng(2500 + 1000 * SEED[(ntips, n)] + ntips + n)
    nt = len(base.taxa)
    F = np.linalg.cholesky(base.cov) @ rng.standard_normal((nt, len(AMPLITUDES)))
    Lo = rng.standard_normal((n, len(AMPLITUDES)))
    X = (F * np.sqrt(np.array(AMPLITUDES))[None, :]) @ Lo.T + NOISE * rng.standard_normal((nt, n))   # [tips (data rows), sites]
    return XR._pair(f"planted{ntips}", base.net, base.taxa, [list(X[:, s]) for s in range(n)])


@functools.lru_cache(maxsize=None)
def planted_gls(ntips, n):
    """dict(gram = Y'PY, R, mu, n_obs, Y, Yc) of a planted case: rate_uni_ref.gls, written for a case without a key"""
    case = planted(ntips, n)
    Y = np.stack([np.array([float(v) for v in case.sites[s][1][0]]) for s in range(n)], axis=1)
    C = case.cov
    Ci = np.linalg.inv(C)
    one = np.ones(len(C))
    Ci1 = Ci @ one
    P = Ci - np.outer(Ci1, Ci1) / float(one @ Ci1)
    mu = (Ci1 @ Y) / float(one @ Ci1)
    Yc = Y - mu[None, :]
    return dict(gram=Y.T @ P @ Y, R=Yc.T @ np.linalg.solve(C, Yc) / (len(C) - 1), mu=mu, n_obs=len(C), Y=Y, Yc=Yc)


def matrix(g, mode):
    """(A, sd): the matrix decomposed -- R ("cov") or the evolutionary correlations ("corr") -- and the evolutionary standard
    deviations (None with "cov")"""
    if mode == "cov":
        return g["R"], None
    sd = np.sqrt(np.diagonal(g["R"]))
    return g["R"] / np.outer(sd, sd), sd


def margins(A, k=K, block=BLOCK):
    """(smallest relative gap (lambda_i - lambda_{i+1}) / lambda_1 over i <= k, lambda_{block+1} / lambda_k)"""
    w = np.sort(np.linalg.eigvalsh(A))[::-1]
    tail = w[block] / w[k - 1] if block < len(w) else 0.0
    return float(np.min(-np.diff(w[: k + 1])) / w[0]), float(max(tail, 0.0))

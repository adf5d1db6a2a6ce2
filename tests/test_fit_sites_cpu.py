"""optimize.lbfgs_sites, the batched L-BFGS behind fit_sites_lg, as a pure function of a batched value_and_grad callback:
no GPU.  Known minima (quadratics, Rosenbrock), the bytes of a converged site, the back-off from a NaN trial point, and the
pruning log-likelihood of a univariate BM batch with Richardson gradients against the closed-form estimates."""
import numpy as np

import pgbp_amd  # noqa: F401  (the package alias)
from pgbp_amd import synth
from pgbp_amd.optimize import lbfgs_sites


def _quadratics(n, d, seed):
    """f_i(x) = (x - c_i)' A_i (x - c_i) / 2 + b_i with condition numbers 1 .. 1e4"""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, d, d))
    for i in range(n):
        Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
        A[i] = Q @ np.diag(np.logspace(0, 4 * i / (n - 1), d)) @ Q.T
    c = rng.normal(size=(n, d))
    b = rng.normal(size=n)

    def vg(X):
        r = X - c
        Ar = np.einsum("nij,nj->ni", A, r)
        return 0.5 * np.sum(r * Ar, axis=1) + b, Ar
    return vg, c, b


def test_quadratics_every_site_reaches_its_minimum():
    vg, c, b = _quadratics(64, 5, 1)
    out = lbfgs_sites(vg, np.zeros((64, 5)), maxiter=200, gtol=1e-9)
    assert out["converged"].all(), out["n_iter"]
    # |x - c| <= |g| / lambda_min, lambda_min = 1, |g|_inf <= gtol max(1, |f|)
    assert np.max(np.abs(out["x"] - c)) <= 1e-7
    assert np.max(np.abs(out["f"] - b)) <= 1e-12 * np.maximum(1.0, np.abs(b)).max()
    assert out["n_iter"].min() < out["n_iter"].max()   # (the sites really have their own histories and stops)


def test_rosenbrock_batch():
    rng = np.random.default_rng(2)
    n = 16
    a = rng.uniform(0.5, 1.5, n)

    def vg(X):
        x, y = X[:, 0], X[:, 1]
        f = (a - x) ** 2 + 100.0 * (y - x * x) ** 2
        return f, np.stack([-2 * (a - x) - 400.0 * x * (y - x * x), 200.0 * (y - x * x)], axis=1)
    out = lbfgs_sites(vg, np.tile([-1.2, 1.0], (n, 1)), maxiter=500, gtol=1e-9)
    assert out["converged"].all(), (out["n_iter"], out["f"])
    assert np.max(np.abs(out["x"][:, 0] - a)) <= 1e-6 and np.max(np.abs(out["x"][:, 1] - a * a)) <= 1e-6


def test_a_converged_site_keeps_its_bytes_while_others_go_on():
    vg, c, b = _quadratics(8, 4, 3)
    seen = []

    def spy(X):
        seen.append(X.copy())
        return vg(X)
    out = lbfgs_sites(spy, np.zeros((8, 4)), gtol=1e-9)
    first = int(np.argmin(out["n_iter"]))
    assert out["n_iter"][first] < out["n_iter"].max()
    # from its last accepted step on, every later callback saw this site at exactly its final point
    later = [X[first] for X in seen[-(out["n_iter"].max() - out["n_iter"][first]):]]
    assert later and all(np.array_equal(r, out["x"][first]) for r in later)
    f, g = vg(out["x"])
    assert np.array_equal(f[first], out["f"][first]) and np.array_equal(g[first], out["g"][first])


def test_nan_at_a_trial_point_backs_off_and_still_converges():
    vg, c, b = _quadratics(8, 3, 4)
    hits = [0]

    def holed(X):
        f, g = vg(X)
        f = f.copy()
        # site 5: a region around the line from the start to the minimum, away from both, reports failure
        far = (np.linalg.norm(X[5] - c[5]) > 0.6 * np.linalg.norm(c[5])) and (np.linalg.norm(X[5]) > 0.3 * np.linalg.norm(c[5]))
        if far:
            hits[0] += 1
            f[5] = np.nan
        return f, g
    clean = lbfgs_sites(vg, np.zeros((8, 3)), gtol=1e-9)
    out = lbfgs_sites(holed, np.zeros((8, 3)), gtol=1e-9)
    assert out["converged"].all() and np.max(np.abs(out["x"] - c)) <= 1e-7
    if hits[0]:
        assert out["n_evals"] >= clean["n_evals"]
    keep = np.arange(8) != 5
    assert np.array_equal(out["x"][keep], clean["x"][keep])   # the other sites never noticed


def test_always_failing_start_stops_unconverged():
    vg, c, b = _quadratics(4, 2, 5)

    def dead(X):
        f, g = vg(X)
        f = f.copy()
        f[2] = np.nan
        return f, g
    out = lbfgs_sites(dead, np.zeros((4, 2)), gtol=1e-9)
    assert not out["converged"][2] and out["converged"][[0, 1, 3]].all() and out["n_iter"][2] == 0


def bm_closed_form(tree, X):
    """GLS mean and ML rate of a univariate BM with a fixed root at mu (= the root value) from the dense covariance of the
    tips: C_ij = depth of the last common ancestor; mu_hat = 1'C^-1 x / 1'C^-1 1, sigma2_hat = r'C^-1 r / n; and the
    log-likelihood there, per site (X: [n_sites, N])."""
    N = tree.nnodes
    tips = np.nonzero(tree.is_leaf)[0]
    anc = []
    for t in tips:
        a, v = {}, int(t)
        h = 0.0
        path = []
        while v > 0:
            path.append(v)
            v = int(tree.parent[v])
        for v in reversed(path):
            h += float(tree.length[v])
            a[v] = h
        anc.append(a)
    n = len(tips)
    Cm = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            common = set(anc[i]) & set(anc[j])
            Cm[i, j] = max((anc[i][v] for v in common), default=0.0)
    Ci = np.linalg.inv(Cm)
    one = np.ones(n)
    Y = X[:, tips]
    mu = (Y @ Ci @ one) / (one @ Ci @ one)
    r = Y - mu[:, None]
    s2 = np.einsum("si,ij,sj->s", r, Ci, r) / n
    ll = -0.5 * (n * np.log(2 * np.pi) + n * np.log(s2) + np.linalg.slogdet(Cm)[1] + n)
    return s2, mu, ll


def test_bm_pruning_loglik_against_the_closed_form():
    rng = np.random.default_rng(6)
    tree = synth.random_tree(40, rng)
    ns = 16
    X = synth.simulate_bm_uni_sites(tree, rng.uniform(0.5, 2, ns), rng.normal(size=ns), rng)
    s2, mu, ll = bm_closed_form(tree, X)
    # (the closed form states the likelihood the pruning computes)
    assert np.max(np.abs(synth.bm_loglik_pruning_uni_sites(tree, s2, mu, X) - ll)) <= 1e-10 * np.max(np.abs(ll))

    def nll(T):
        return -synth.bm_loglik_pruning_uni_sites(tree, np.exp(T[:, 0]), T[:, 1], X)

    def vg(T):
        g = np.zeros_like(T)
        for k in range(2):
            e = np.zeros(2); e[k] = 1.0
            rich = lambda h: (nll(T + h * e) - nll(T - h * e)) / (2 * h)
            g[:, k] = (4 * rich(5e-4) - rich(1e-3)) / 3
        return nll(T), g
    out = lbfgs_sites(vg, np.zeros((ns, 2)), gtol=1e-8)
    assert out["converged"].all()
    assert np.all(-out["f"] >= ll - 1e-8 * np.maximum(1.0, np.abs(ll)))
    assert np.max(np.abs(np.exp(out["x"][:, 0]) - s2) / s2) <= 1e-4 and np.max(np.abs(out["x"][:, 1] - mu)) <= 1e-4 * np.maximum(1, np.abs(mu)).max()

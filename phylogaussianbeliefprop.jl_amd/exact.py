"""calibrate_exact_cliquetree! (src/calibration.jl:404-517): the closed-form REML fit of a Brownian motion on a clique
tree -- two calibrations and one sweep over the node families, all on the device."""
import numpy as np

from . import _lib as L
from .calibration import calibrate_
from .clustergraphbeliefs import _check


def bm_exact_stats(beliefs, all_sites=False):
    """pgbp_bm_exact_stats on the current beliefs: (num [p, p], den) of src/calibration.jl:440-499, with a leading site axis
    and the info words when all_sites."""
    p = int(getattr(beliefs, "_lg_p", 1))   # (no family table: the call itself says so)
    s0, s1 = (0, beliefs.n_sites) if all_sites else (beliefs.site, beliefs.site + 1)
    num = np.zeros((s1 - s0, p, p))
    den = np.zeros(s1 - s0)
    info = np.zeros(s1 - s0, dtype=np.int32)
    _check(beliefs._lib.pgbp_bm_exact_stats(beliefs._eng, s0, s1, L.f64p(num), L.f64p(den), L.i32p(info)), beliefs._eng)
    num = num.transpose(0, 2, 1)   # (column-major p x p; symmetric up to rounding)
    if all_sites:
        return num, den, info
    if info[0]:
        raise np.linalg.LinAlgError(f"PosDefException: belief {info[0] - 1} is not positive definite")
    return num[0], float(den[0])


def bm_exact_stats_sites(beliefs, root=None):
    """pgbp_bm_exact_stats_sites on the current beliefs: the sweep of bm_exact_stats(all_sites=True) for a univariate batch on
    the thread-per-site kernels (p = 1, every belief of at most 2 variables, at least 8 sites; anything else raises
    PGBP_ERR_INVALID), lanes = sites, with the per-site mask of set_site_missing_lg and the shifts in force.  The beliefs are
    read in the layout they are in: nothing is converted.  root = (belief index, position of the root variable in it), or None.
    Returns (num [n_sites], den [n_sites], mu [n_sites] or None, info [n_sites]): den is the number of tips a site observes
    less one, to rounding; a site whose info is not 0 holds NaN."""
    n = beliefs.n_sites
    num, den = np.zeros(n), np.zeros(n)
    mu = np.zeros(n) if root is not None else None
    info = np.zeros(n, dtype=np.int32)
    rb, rp = (int(root[0]), int(root[1])) if root is not None else (0, 0)
    _check(beliefs._lib.pgbp_bm_exact_stats_sites(beliefs._eng, 0, n, rb, rp, L.f64p(num), L.f64p(den),
                                                  L.f64p(mu) if root is not None else None, L.i32p(info)), beliefs._eng)
    return num, den, mu, info


def calibrate_exact_sites_(beliefs, schedule_tree, root, beliefs_fixedroot=None):
    """calibrate_exact_cliquetree_ for every site of a univariate batch at once, on the thread-per-site kernels and in their
    layout: the closed-form REML fit of a Brownian motion at each site, from one calibration and one sweep -- no optimiser, no
    start values, no tolerance.  It works with a per-site mask of missing tips in force (set_site_missing_lg, on both engines)
    and with shifts set.

    beliefs: the engine of the batch on the clique tree, built with fixedroot=False and ONE rate, family table set up.
    root = (cluster index, position of the root variable in it).  Steps: factors of R = 1, mu = 0 -> one calibration (calibrate_'s
    postorder and preorder of `schedule_tree`, enqueued as loglik_and_gradient_sites_lg enqueues them) -> the sweep (bm_exact_stats_sites) -> R_hat = num / den, NaN where den < 0.5: den is the number of observed tips less one to
    rounding, and 0.5 separates a site that observes one tip from a site that observes two.  With beliefs_fixedroot (the engine
    of the same batch built with fixedroot=True) the returned model is scored there: a per-site fill at (R_hat, mu_hat) and
    loglik_lg.  Returns dict(R, mu, loglik, den [n_sites] float, info [n_sites] int32); a site whose info is not 0 (the sweep's
    code, or -1 where the calibration itself failed at that site) is NaN in R, mu and loglik and does not raise; loglik is NaN
    without beliefs_fixedroot and where R is."""
    n = beliefs.n_sites
    beliefs.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1))
    # reset from the factors, one calibration and the root integration enqueued without host synchronisation, as
    # loglik_and_gradient_sites_lg does; the sweep's fetch is the one wait, the pool stays in the site-minor layout and, like
    # loglik_lg, the host mirrors of the beliefs are not refreshed (beliefs.pull() does that)
    _, (num, den, mu, info), cal = beliefs._loglik_and_sites(schedule_tree, lambda: bm_exact_stats_sites(beliefs, root))
    info = np.where((cal != 0) & (info == 0), -1, info).astype(np.int32)   # (a message of that site was not positive definite)
    with np.errstate(divide="ignore", invalid="ignore"):
        R = np.where((den >= 0.5) & (info == 0), num / den, np.nan)
    mu = np.where(info == 0, mu, np.nan)
    ll = np.full(n, np.nan)
    if beliefs_fixedroot is not None:
        fx = beliefs_fixedroot
        fx._ensure_schedule([schedule_tree])
        ok = np.isfinite(R) & (R > 0) & np.isfinite(mu)
        fx.assignfactors_lg_(np.where(ok, R, 1.0).reshape(n, 1, 1, 1), np.where(ok, mu, 0.0).reshape(n, 1))
        norm, linfo = fx.loglik_lg()
        ll = np.where(ok & (linfo == 0), norm, np.nan)
    return dict(R=R, mu=mu, loglik=ll, den=den, info=info)


def _site_range(r, n):
    """(begin, end) of a site range given as None (all), (begin, end), a range or a slice with step 1"""
    if r is None:
        return 0, n
    if isinstance(r, slice):
        a, b, st = r.indices(n)
        if st != 1:
            raise ValueError("a site range is contiguous")
        return a, max(a, b)
    if isinstance(r, range):
        if r.step != 1:
            raise ValueError("a site range is contiguous")
        return r.start, max(r.start, r.stop)
    a, b = r
    return int(a), int(b)


def bm_rate_matrix_sites(beliefs, rows=None, cols=None, root=None):
    """pgbp_bm_rate_matrix_sites on the current beliefs (calibrated under R = 1, mu = 0, improper root): the cross-site form
    of bm_exact_stats_sites for a univariate batch on the thread-per-site kernels.  rows, cols: contiguous site ranges
    ((begin, end), a range, a slice; None: all sites) -- a matrix too large for one device block is tiled through them.
    Returns (gram [rows, cols] = (Y'PY)_ab = sum_f e_fa e_fb / t_f on the matrix cores, den, mu or None, info), the last three
    as pairs (of the row sites, of the column sites).  gram of a square query is symmetric to the byte, and a block of it has
    the bytes of the same entries of the whole; a site whose info is not 0 is NaN in its row or column, its den and its mu.
    Refused (PGBP_ERR_INVALID) with a per-site mask of missing tips in force, after an OU fill and with tip noise."""
    n = beliefs.n_sites
    r0, r1 = _site_range(rows, n)
    c0, c1 = _site_range(cols, n)
    nr, nc = max(0, r1 - r0), max(0, c1 - c0)
    gram = np.zeros((nr, nc))
    den = np.zeros(nr + nc)
    mu = np.zeros(nr + nc) if root is not None else None
    info = np.zeros(nr + nc, dtype=np.int32)
    rb, rp = (int(root[0]), int(root[1])) if root is not None else (0, 0)
    _check(beliefs._lib.pgbp_bm_rate_matrix_sites(beliefs._eng, r0, r1, c0, c1, rb, rp, L.f64p(gram), L.f64p(den),
                                                  L.f64p(mu) if root is not None else None, L.i32p(info)), beliefs._eng)
    split = lambda x: None if x is None else (x[:nr], x[nr:])
    return gram, split(den), split(mu), split(info)


def calibrate_rate_matrix_sites_(beliefs, schedule_tree, root, rows=None, cols=None):
    """The evolutionary rate matrix between the sites of a univariate batch (evol.vcv / ratematrix): the REML estimate
    R_hat = Y'PY / (n_tips - 1) under a multivariate Brownian motion whose traits are the sites, from one calibration of the
    univariate engine and one call, on the thread-per-site kernels and in their layout.

    beliefs: as for calibrate_exact_sites_ (fixedroot=False, ONE rate, family table set up); every site observes the same tips
    (a shared child_mask is fine, a per-site mask is refused); shifts in force are honoured.  Steps: factors of R = 1, mu = 0 ->
    one calibration enqueued without refreshing the host mirrors -> bm_rate_matrix_sites(rows, cols, root).  Returns
    dict(R [rows, cols] = gram / sqrt(den_a den_b), corr = R_ab / sqrt(var_a var_b) (the evolutionary correlations), gram, and
    the pairs (of the row sites, of the column sites) var (the sites' own rates R_aa), mu, den, info).  A site whose info is not
    0 (the call's code, or -1 where the calibration failed at that site) is NaN in its row or column and in mu; R is NaN where
    den < 0.5 (fewer than two observed tips)."""
    n = beliefs.n_sites
    r0, r1 = _site_range(rows, n)
    c0, c1 = _site_range(cols, n)
    beliefs.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1))
    _, (gram, den, mu, info), cal = beliefs._loglik_and_sites(
        schedule_tree, lambda: bm_rate_matrix_sites(beliefs, (r0, r1), (c0, c1), root))
    gram = gram.copy()
    cals = (cal[r0:r1], cal[c0:c1])
    info = tuple(np.where((c != 0) & (i == 0), -1, i).astype(np.int32) for c, i in zip(cals, info))
    gram[info[0] != 0, :] = np.nan
    gram[:, info[1] != 0] = np.nan
    den = tuple(np.where((d >= 0.5) & (i == 0), d, np.nan) for d, i in zip(den, info))
    mu = tuple(np.where(i == 0, m, np.nan) for m, i in zip(mu, info))
    # the sites' own rates gram_aa / den_a: the diagonal of a square query, else num of the per-site call on the same beliefs
    if (r0, r1) == (c0, c1):
        num_r = num_c = np.diagonal(gram).copy()
    else:
        num = bm_exact_stats_sites(beliefs, None)[0]
        num_r, num_c = num[r0:r1], num[c0:c1]
    with np.errstate(divide="ignore", invalid="ignore"):
        R = gram / np.sqrt(den[0][:, None] * den[1][None, :])
        var = (num_r / den[0], num_c / den[1])
        corr = R / np.sqrt(var[0][:, None] * var[1][None, :])
    return dict(R=R, corr=corr, var=var, mu=mu, den=den, info=info, gram=gram)


def _observed_tips(beliefs):
    """the data rows of the tips the family table observes (child_mask bit 0, a tip with a data row and a parent)"""
    k = beliefs._lg
    cm = k.get("child_mask")
    tip = (k["child_pos"] < 0) & (k["data_row"] >= 0) & (k["n_parents"] > 0)
    if cm is not None:
        tip &= (np.asarray(cm) & np.uint64(1)).astype(bool)
    return np.asarray(k["data_row"])[tip]


def phylo_pca_sites(beliefs, schedule_tree, root, mode="cov", n_components=None):
    """Phylogenetic principal components of a univariate batch (phyl.pca), the sites as the traits: the eigendecomposition of
    the evolutionary rate matrix (mode="cov") or of the evolutionary correlations (mode="corr") from
    calibrate_rate_matrix_sites_ over all sites.

    The rate matrix is formed on the device; the eigendecomposition is HOST work, numpy.linalg.eigh of the dense
    [n_sites, n_sites] matrix: O(n_sites^3) flops and 8 n_sites^2 bytes, seconds up to a few thousand sites and the wrong tool
    beyond some ten thousand (phylo_pca_leading_sites gives the leading components there, without forming R).
    Returns dict(values [k] in decreasing order, loadings [n_sites, k] (unit columns, sign free), scores [n_observed_tips, k]
    = (Y - 1 mu') V over the tips the table observes in data-row order (with mode="corr" the columns of Y - 1 mu' are divided
    by the evolutionary standard deviations), rows: those data rows, mu, R: the matrix decomposed).  The data are those given
    to lg_setup; displacements of shifts in force are not taken off the scores.  A site with info != 0 raises LinAlgError."""
    if mode not in ("cov", "corr"):
        raise ValueError("mode is 'cov' or 'corr'")
    fit = calibrate_rate_matrix_sites_(beliefs, schedule_tree, root)
    if fit["info"][0].any():
        raise np.linalg.LinAlgError(f"phylo_pca_sites: site {int(np.flatnonzero(fit['info'][0])[0])} has no rate estimate")
    A = fit["R"] if mode == "cov" else fit["corr"]
    w, V = np.linalg.eigh(A)
    order = np.argsort(w)[::-1][: (len(w) if n_components is None else int(n_components))]
    w, V = w[order], V[:, order]
    rows = _observed_tips(beliefs)
    Y = np.asarray(beliefs._lg["data"])[:, rows, 0].T - fit["mu"][0][None, :]
    if mode == "corr":
        Y = Y / np.sqrt(fit["var"][0])[None, :]
    return dict(values=w, loadings=V, scores=Y @ V, rows=rows, mu=fit["mu"][0], R=A)


RATE_APPLY_MAX_VECTORS = 64   # vectors per pgbp_bm_rate_apply_sites call


def bm_rate_apply_sites(beliefs, V, sites=None, root=None):
    """pgbp_bm_rate_apply_sites on the current beliefs (calibrated under R = 1, mu = 0, improper root): gram @ V with gram of
    bm_rate_matrix_sites(rows = cols = sites), the matrix never formed -- two skinny products with the residual rows U on the
    matrix cores, U recomputed per call.  V: [sites, k] or [sites]; sites: a contiguous range (None: all sites).  V travels
    as its [k][sites] transpose, in calls of at most 64 vectors; a vector's result does not depend on the vectors it travels
    with.  Returns (GV of V's shape, den, mu or None, info) over the sites of the range.  If any site has info != 0, GV is
    NaN in every entry (a bad site has no column of U and U V mixes all sites): check info once.  Refusals as
    bm_rate_matrix_sites."""
    n = beliefs.n_sites
    s0, s1 = _site_range(sites, n)
    ns = max(0, s1 - s0)
    V = np.asarray(V, dtype=float)
    flat = V.ndim == 1
    V2 = V.reshape(-1, 1) if flat else V
    if V2.ndim != 2 or V2.shape[0] != ns:
        raise ValueError(f"V has shape {V.shape}; the range holds {ns} sites")
    k = V2.shape[1]
    GV = np.zeros((k, ns))
    den = np.zeros(ns)
    mu = np.zeros(ns) if root is not None else None
    info = np.zeros(ns, dtype=np.int32)
    rb, rp = (int(root[0]), int(root[1])) if root is not None else (0, 0)
    for j0 in range(0, max(k, 1), RATE_APPLY_MAX_VECTORS):
        vt = np.ascontiguousarray(V2[:, j0: j0 + RATE_APPLY_MAX_VECTORS].T)
        out = np.zeros_like(vt)
        # (k = 0: the call itself refuses, as every other misuse)
        _check(beliefs._lib.pgbp_bm_rate_apply_sites(beliefs._eng, s0, s1, vt.shape[0], L.f64p(vt), rb, rp, L.f64p(out), L.f64p(den),
                                                     L.f64p(mu) if root is not None else None, L.i32p(info)), beliefs._eng)
        GV[j0: j0 + vt.shape[0]] = out
    GV = GV.T.copy()
    return (GV[:, 0] if flat else GV), den, mu, info


def leading_eigenpairs(apply, n, k, block=None, maxiter=200, rtol=1e-10, seed=0):
    """The k largest eigenpairs of a symmetric positive semidefinite operator of order n given as apply(Q [n, b]) -> G Q: block
    subspace iteration with Rayleigh-Ritz, a pure numpy function of its callback.

    Q0 = qr(standard normals from default_rng(seed)) [n, block]; per iteration ONE apply: Z = apply(Q), T = Q'Z symmetrised,
    eigh(T) -> Ritz pairs (theta_i, x_i = Q y_i) in decreasing order with residuals |Z y_i - theta_i x_i|_2; stop when the
    first k residuals are at most rtol * theta_1, else Q = qr(Z).  The error of theta_i is then at most its residual and that
    of x_i at most residual / gap (Davis-Kahan); the residuals shrink by about lambda_{block+1} / lambda_k per iteration, so
    the default block = min(n, 16 ceil((k + 8) / 16)) carries at least 8 guard vectors and is a whole number of the device
    call's tiles.  k and block are clamped to n (block to k from below).  Householder QR: a Z of rank below block gives an
    orthonormal Q all the same, the Ritz values beyond the rank are rounding, and the iteration stops as usual.
    Returns dict(values [k], vectors [n, k], residuals [k], iterations, converged); not converging within maxiter is reported,
    not raised."""
    n = int(n)
    k = max(1, min(int(k), n))
    b = 16 * -(-(k + 8) // 16) if block is None else int(block)
    b = max(k, min(n, b))
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, b)))[0]
    theta, X, res, it, done = np.zeros(b), Q, np.full(b, np.inf), 0, False
    for it in range(1, int(maxiter) + 1):
        Z = np.asarray(apply(Q), dtype=float)
        T = Q.T @ Z
        theta, Y = np.linalg.eigh(0.5 * (T + T.T))
        order = np.argsort(theta)[::-1]
        theta, Y = theta[order], Y[:, order]
        X = Q @ Y
        res = np.linalg.norm(Z @ Y - X * theta[None, :], axis=0)
        if not np.all(np.isfinite(res)):
            break
        if np.all(res[:k] <= rtol * abs(theta[0])):
            done = True
            break
        Q = np.linalg.qr(Z)[0]
    return dict(values=theta[:k].copy(), vectors=X[:, :k].copy(), residuals=res[:k].copy(), iterations=it, converged=done)


def phylo_pca_leading_sites(beliefs, schedule_tree, root, n_components, mode="cov", block=None, maxiter=200, rtol=1e-10, seed=0):
    """The leading n_components phylogenetic principal components of a univariate batch (phyl.pca, the sites as the traits)
    WITHOUT the [n_sites, n_sites] matrix: what phylo_pca_sites returns for its first components, for batches whose rate
    matrix does not fit or whose full eigendecomposition nobody wants.

    Steps: factors of R = 1, mu = 0 -> one calibration enqueued as calibrate_rate_matrix_sites_ does it (the host mirrors are
    not refreshed) -> one bm_exact_stats_sites for num, den, mu, info (any info != 0, or a site without a finite estimate, raises LinAlgError naming the site) ->
    leading_eigenpairs with apply(Q) = D (G (D Q)) / den, G by bm_rate_apply_sites (one device pass over the residual rows per
    iteration), D = I (mode="cov") or diag(1 / sqrt(num_a / den)) (mode="corr": the evolutionary correlations); the scaling is
    numpy on [n_sites, block].  den is one number: every site observes the same tips.
    Returns the keys of phylo_pca_sites without R -- values, loadings, scores = (Y - 1 mu') V (columns divided by the
    evolutionary standard deviations with mode="corr"), rows, mu -- and explained = values / trace (the trace from num / den;
    n_sites with mode="corr"), residuals, iterations, converged (False: maxiter reached; not raised)."""
    if mode not in ("cov", "corr"):
        raise ValueError("mode is 'cov' or 'corr'")
    n = beliefs.n_sites
    beliefs.assignfactors_lg_(np.ones((1, 1, 1)), np.zeros(1))
    _, (num, den, mu, info), cal = beliefs._loglik_and_sites(schedule_tree, lambda: bm_exact_stats_sites(beliefs, root))
    info = np.where((cal != 0) & (info == 0), -1, info)
    with np.errstate(divide="ignore", invalid="ignore"):
        var = num / den
    # (a site can be NaN with info 0 -- a cluster whose belief is the constant 1 --; it has no residual column either)
    none = (info != 0) | ~np.isfinite(var) | (den < 0.5)
    if none.any():
        raise np.linalg.LinAlgError(f"phylo_pca_leading_sites: site {int(np.flatnonzero(none)[0])} has no rate estimate")
    d = np.ones(n) if mode == "cov" else 1.0 / np.sqrt(var)
    den0 = float(den[0])   # (to rounding the same at every site: the observed tips less one)

    def apply(Q):
        GV, _, _, inf = bm_rate_apply_sites(beliefs, d[:, None] * Q)
        if inf.any():
            raise np.linalg.LinAlgError(f"phylo_pca_leading_sites: site {int(np.flatnonzero(inf)[0])} has no rate estimate")
        return d[:, None] * GV / den0

    eig = leading_eigenpairs(apply, n, n_components, block=block, maxiter=maxiter, rtol=rtol, seed=seed)
    w, V = eig["values"], eig["vectors"]
    rows = _observed_tips(beliefs)
    Y = np.asarray(beliefs._lg["data"])[:, rows, 0].T - mu[None, :]
    if mode == "corr":
        Y = Y / np.sqrt(var)[None, :]
    trace = float(np.sum(var)) if mode == "cov" else float(n)
    return dict(values=w, loadings=V, scores=Y @ V, rows=rows, mu=mu, explained=w / trace, residuals=eig["residuals"],
                iterations=eig["iterations"], converged=eig["converged"])


def calibrate_exact_cliquetree_(beliefs, schedule_tree, root, beliefs_fixedroot=None, all_sites=False):
    """calibrate_exact_cliquetree!(beliefs, spt, prenodes, tbl, taxa, evomodelfun) (src/calibration.jl:404-517) for a
    (univariate or full) Brownian motion.

    beliefs: an engine on the clique tree built with fixedroot=False and ONE rate, family table set up (lg_setup): the
    improper-root model the reference calibrates under (:423).  root = (cluster index, position of the root node's first
    variable in it).  Steps as the reference: factors of R = I, mu = 0 -> calibrate -> mu_hat = the root's posterior mean ->
    the family sweep (pgbp_bm_exact_stats) -> R_hat = num / den.  The reference then re-allocates the root's scope in
    place to score the returned fixed-root model (:507-514); here that model lives on a second engine on the same graph,
    beliefs_fixedroot (fixedroot=True, its own lg_setup): assignfactors_lg_(R_hat, mu_hat) + loglik_lg on it gives the
    score; without it the score is nan.  Returns (R_hat [p, p], mu_hat [p], loglik), each with a leading site axis when
    all_sites."""
    if not hasattr(beliefs, "_lg_p"):
        bm_exact_stats(beliefs)               # raises: no family table
    p = int(beliefs._lg_p)
    beliefs.assignfactors_lg_(np.eye(p)[None], np.zeros(p), sync=True)
    succ, _ = calibrate_(beliefs, [schedule_tree])
    if not succ:
        raise RuntimeError("calibrate_exact_cliquetree_: the calibration under R = I failed")
    ci, pos = int(root[0]), int(root[1])
    mom = beliefs.moments_([ci], cov=False, all_sites=all_sites)[0]
    num, den = bm_exact_stats(beliefs, all_sites=all_sites)[:2]
    if all_sites:
        if mom[3].any():
            raise np.linalg.LinAlgError("PosDefException: the root cluster of some site is not positive definite")
        mu_hat = mom[0][:, pos: pos + p].copy()
        R_hat = num / den[:, None, None]
    else:
        mu_hat = mom[0][pos: pos + p].copy()
        R_hat = num / den
    ll = np.full(beliefs.n_sites, np.nan) if all_sites else float("nan")
    if beliefs_fixedroot is not None:
        fx = beliefs_fixedroot
        fx.set_schedule([schedule_tree])
        if all_sites:
            fx.assignfactors_lg_(R_hat[:, None], mu_hat)
        else:
            fx.assignfactors_lg_(R_hat[None], mu_hat)
        norm, info = fx.loglik_lg()
        if all_sites:
            ll = np.where(info == 0, norm, np.nan)
        else:
            ll = float(norm[fx.site]) if info[fx.site] == 0 else float("nan")
    return R_hat, mu_hat, ll

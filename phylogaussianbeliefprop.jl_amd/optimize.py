"""Callers of the hot path: maximum-likelihood / maximum-factored-energy estimation of the model parameters
(calibrate_optimize_cliquetree!, calibrate_optimize_clustergraph!: src/calibration.jl:163-359) with the whole objective
on the device -- factors assigned from the candidate parameters, messages passed, root integrated (or the free energy
evaluated) without the belief state ever leaving HBM; only the parameters and one number per evaluation cross the bus.

The reference minimises with Optim.jl's LBFGS over unconstrained parameters; here the same transforms and the same
objective go to scipy's L-BFGS-B with central-difference gradients (the optimum is a property of the objective, not of
the optimiser).  The ClusterGraphBelief must have its node families set up (`lg_setup`)."""
import ctypes as C

import numpy as np

from . import _lib as L


class _BMTransform:
    """params_optimize / params_original of UnivariateBrownianMotion (log sigma2, mu:
    src/evomodels/homogeneousbrownianmotion.jl:48-49) and MvFullBrownianMotion (log-Cholesky of R, then mu: :130-157)."""

    def __init__(self, p, diagonal=False):
        self.p = p
        self.diagonal = diagonal   # MvDiagBrownianMotion: log of the rates, then mu (:89-90)

    def forward(self, R, mu):
        R = np.atleast_2d(np.asarray(R, float))
        if self.diagonal:
            return np.array(list(np.log(np.diag(R))) + list(np.asarray(mu, float).reshape(self.p)))
        U = np.linalg.cholesky(R).T
        p = self.p
        above = [U[i, j] for j in range(1, p) for i in range(j)]
        return np.array([np.log(U[i, i]) for i in range(p)] + above + list(np.asarray(mu, float).reshape(p)))

    def back(self, theta):
        p = self.p
        if self.diagonal:
            return np.diag(np.exp(np.asarray(theta[:p], float))), np.asarray(theta[p:2 * p], float)
        U = np.zeros((p, p))
        k = 0
        for i in range(p):
            U[i, i] = np.exp(theta[k]); k += 1
        for j in range(1, p):
            for i in range(j):
                U[i, j] = theta[k]; k += 1
        return U.T @ U, np.asarray(theta[k:k + p], float)

    def pullback(self, theta, dR, dmu):
        """Chain rule through `back`: the gradient in theta of a function whose gradient in (R, mu) is (dR, dmu), dR
        symmetric with d f = tr(dR dR_) (what gradient_lg returns).  Diagonal: R_ii = exp(theta_i).  Full: R = U'U, so
        d f / d U = 2 U dR on the upper triangle, the diagonal entries times U_ii for theta = log U_ii."""
        p = self.p
        dR = np.atleast_2d(np.asarray(dR, float))
        dR = (dR + dR.T) / 2
        dmu = np.asarray(dmu, float).reshape(p)
        if self.diagonal:
            return np.concatenate([np.diag(dR) * np.exp(np.asarray(theta[:p], float)), dmu])
        R, _ = self.back(theta)
        U = np.linalg.cholesky(R).T
        dU = 2.0 * U @ dR
        return np.array([dU[i, i] * U[i, i] for i in range(p)] + [dU[i, j] for j in range(1, p) for i in range(j)]
                        + list(dmu))


def _minimise(score, x0, maxiter, grad=None):
    from scipy.optimize import minimize

    def central(x):
        g = np.zeros_like(x)
        for i in range(len(x)):
            h = 1e-6 * max(1.0, abs(x[i]))
            e = np.zeros_like(x); e[i] = h
            g[i] = (score(x + e) - score(x - e)) / (2 * h)
        return g
    if grad is None:
        grad = central
    # L-BFGS-B, restarted from its own end point while it still improves (its line search gives up early on badly scaled
    # starts, e.g. rates two orders of magnitude off), then a Nelder-Mead polish when a restart stalls above the tolerance
    best = minimize(score, x0, jac=grad, method="L-BFGS-B", options={"maxiter": maxiter, "ftol": 1e-15, "gtol": 1e-9})
    for _ in range(20):
        nxt = minimize(score, best.x, jac=grad, method="L-BFGS-B", options={"maxiter": maxiter, "ftol": 1e-15, "gtol": 1e-9})
        improved = nxt.fun < best.fun - 1e-13 * max(1.0, abs(best.fun))
        nxt.nfev += best.nfev
        if nxt.fun <= best.fun:
            best = nxt
        if not improved:
            break
    if np.linalg.norm(grad(best.x)) > 1e-5 * max(1.0, abs(best.fun)):
        pol = minimize(score, best.x, method="Nelder-Mead", options={"xatol": 1e-10, "fatol": 1e-13, "maxiter": 400 * len(x0)})
        pol.nfev += best.nfev
        if pol.fun <= best.fun:
            best = pol
            nxt = minimize(score, best.x, jac=grad, method="L-BFGS-B", options={"maxiter": maxiter, "ftol": 1e-15, "gtol": 1e-9})
            if nxt.fun <= best.fun:
                nxt.nfev += best.nfev
                best = nxt
    return best


def _check_gradient_mode(gradient):
    if gradient not in ("central", "analytic"):
        raise ValueError(f"gradient must be 'central' or 'analytic', not {gradient!r}")


def calibrate_optimize_cliquetree_(beliefs, schedule_tree, R0, mu0, extra_rates=(), maxiter=200, diagonal=False,
                                   gradient="central", sigma_e0=None):
    """calibrate_optimize_cliquetree! (src/calibration.jl:183-221) for a homogeneous Brownian motion (univariate or full
    rate matrix): maximise the log-likelihood over (R, mu); the root prior variance, if the root is random, stays fixed
    (`extra_rates`: the matrices that follow R in the rate table of lg_setup, e.g. the root prior variance).
    Each evaluation = assignfactors! + postorder of `schedule_tree` + integratebelief! at its root, on the device.
    diagonal: MvDiagBrownianMotion (independent traits: only the diagonal of R is estimated).
    gradient: "central" (default) -- central differences, 2 n_theta evaluations per gradient; "analytic" -- value and
    exact gradient from ONE calibration and one sweep over the node families (loglik_and_gradient_lg), pulled back
    through the transform.  `opt.n_device_evals` counts the device evaluations either way.
    sigma_e0: None (default: nothing below applies), or the start value of the within-species covariance Sigma_e of the tip
    noise in force (set_tip_noise_lg: its families, scale and se2 stay as they are, shared over the sites).  Sigma_e is then
    estimated jointly with R and mu, through the same transform as R (log-Cholesky; its diagonal when `diagonal`), with
    either gradient mode ("analytic": dsigma_e of gradient_lg).  The estimate is returned as `opt.sigma_e` and left in force.
    Returns (R, mu, loglik, scipy result)."""
    _check_gradient_mode(gradient)
    p = beliefs._lg_p
    tf = _BMTransform(p, diagonal)
    beliefs._ensure_schedule([schedule_tree])
    if sigma_e0 is not None:
        return _optimize_with_sigma_e(beliefs, schedule_tree, tf, R0, mu0, extra_rates, maxiter, gradient, sigma_e0)
    count = [0]
    memo = {}

    def value_and_grad(theta):
        key = np.asarray(theta, float).tobytes()
        if key not in memo:
            memo.clear()
            R, mu = tf.back(theta)
            try:
                np.linalg.cholesky(R)
            except np.linalg.LinAlgError:
                memo[key] = (np.inf, np.zeros(len(theta)))
                return memo[key]
            rates = np.stack([R] + [np.atleast_2d(np.asarray(x, float)) for x in extra_rates])
            beliefs.assignfactors_lg_(rates, mu)
            count[0] += 1
            ll, g = beliefs.loglik_and_gradient_lg(schedule_tree, all_sites=True)
            if g["info"][0] or not np.isfinite(ll[0]):
                memo[key] = (np.inf, np.zeros(len(theta)))
            else:
                memo[key] = (-float(ll[0]), -tf.pullback(theta, g["dR"][0, 0], g["dmu"][0]))
        return memo[key]

    def score(theta):
        R, mu = tf.back(theta)
        try:
            np.linalg.cholesky(R)
        except np.linalg.LinAlgError:
            return np.inf
        rates = np.stack([R] + [np.atleast_2d(np.asarray(x, float)) for x in extra_rates])
        beliefs.assignfactors_lg_(rates, mu)
        count[0] += 1
        ll, info = beliefs.loglik_lg()
        return np.inf if (info[0] or not np.isfinite(ll[0])) else -float(ll[0])
    if gradient == "analytic":
        opt = _minimise(lambda x: value_and_grad(x)[0], tf.forward(R0, mu0), maxiter, grad=lambda x: value_and_grad(x)[1])
    else:
        opt = _minimise(score, tf.forward(R0, mu0), maxiter)
    opt.n_device_evals = count[0]
    R, mu = tf.back(opt.x)
    return R, mu, -float(opt.fun), opt


def _optimize_with_sigma_e(beliefs, schedule_tree, tf, R0, mu0, extra_rates, maxiter, gradient, sigma_e0):
    """calibrate_optimize_cliquetree_ over (R, mu, Sigma_e): theta = [transform of (R, mu) | transform of Sigma_e]."""
    p = tf.p
    noise = getattr(beliefs, "_lg_noise", None)
    if noise is None:
        raise ValueError("calibrate_optimize_cliquetree_: sigma_e0 given but no tip noise is set (call set_tip_noise_lg first)")
    if noise["per_site"]:
        raise ValueError("calibrate_optimize_cliquetree_: sigma_e0 needs a shared sigma_e, the noise in force is per site")
    nt = len(tf.forward(R0, mu0))
    zero = np.zeros(p)
    count = [0]
    memo = {}

    def unpack(theta):
        R, mu = tf.back(theta[:nt])
        S, _ = tf.back(np.concatenate([theta[nt:], zero]))
        return R, mu, S

    def fill(theta):
        """The factors under theta; False where R or Sigma_e is not positive definite."""
        R, mu, S = unpack(theta)
        try:
            np.linalg.cholesky(R)
            np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            return False
        beliefs.set_tip_noise_lg(noise["families"], S, noise["scale"], noise["se2"])
        beliefs.assignfactors_lg_(np.stack([R] + [np.atleast_2d(np.asarray(x, float)) for x in extra_rates]), mu)
        count[0] += 1
        return True

    def score(theta):
        if not fill(theta):
            return np.inf
        ll, info = beliefs.loglik_lg()
        return np.inf if (info[0] or not np.isfinite(ll[0])) else -float(ll[0])

    def value_and_grad(theta):
        key = np.asarray(theta, float).tobytes()
        if key not in memo:
            memo.clear()
            memo[key] = (np.inf, np.zeros(len(theta)))
            if fill(theta):
                ll, g = beliefs.loglik_and_gradient_lg(schedule_tree, all_sites=True)
                if not g["info"][0] and np.isfinite(ll[0]):
                    gs = tf.pullback(np.concatenate([theta[nt:], zero]), g["dsigma_e"][0], zero)[:len(theta) - nt]
                    memo[key] = (-float(ll[0]), -np.concatenate([tf.pullback(theta[:nt], g["dR"][0, 0], g["dmu"][0]), gs]))
        return memo[key]
    x0 = np.concatenate([tf.forward(R0, mu0), tf.forward(sigma_e0, zero)[:-p]])
    if gradient == "analytic":
        opt = _minimise(lambda x: value_and_grad(x)[0], x0, maxiter, grad=lambda x: value_and_grad(x)[1])
    else:
        opt = _minimise(score, x0, maxiter)
    opt.n_device_evals = count[0]
    R, mu, S = unpack(opt.x)
    fill(opt.x)
    opt.sigma_e = S
    return R, mu, -float(opt.fun), opt


def calibrate_optimize_clustergraph_(beliefs, schedule, R0, mu0, extra_rates=(), maxiter_calibration=100, maxiter=200,
                                     diagonal=False, gradient="central"):
    """calibrate_optimize_clustergraph! (src/calibration.jl:309-359): maximise the factored energy (= minus the Bethe free
    energy; the log-likelihood on a clique tree) over (R, mu).  Each evaluation = assignfactors! + factors from beliefs +
    regularizebeliefs_bycluster! + calibrate!(schedule, maxiter_calibration; auto=true) + free_energy, on the device.
    gradient: "central" (default), or "analytic": the family sweep (gradient_lg) on the beliefs the calibration left.
    That is the gradient of the factored energy ONLY at a converged calibration (the Bethe free energy is stationary in
    the beliefs at a fixed point); where calibrate! stops at maxiter_calibration before convergence it is approximate.
    Returns (R, mu, factored energy, scipy result)."""
    from .calibration import calibrate_
    _check_gradient_mode(gradient)
    p = beliefs._lg_p
    tf = _BMTransform(p, diagonal)
    lib = beliefs._lib
    count = [0]

    def score(theta):
        R, mu = tf.back(theta)
        try:
            np.linalg.cholesky(R)
        except np.linalg.LinAlgError:
            return np.inf
        rates = np.stack([R] + [np.atleast_2d(np.asarray(x, float)) for x in extra_rates])
        beliefs.assignfactors_lg_(rates, mu)               # also snapshots the factors and resets the flags
        count[0] += 1
        if lib.pgbp_regularize_bycluster(beliefs._eng) != L.PGBP_OK:
            return np.inf
        succ, _ = calibrate_(beliefs, schedule, maxiter_calibration, auto=True, verbose=False, sync=False)
        if not succ:
            return np.inf
        out, info = beliefs.free_energy(all_sites=True)
        return np.inf if info[0] or not np.isfinite(out[0, 2]) else float(out[0, 2])
    memo = {}

    def value_and_grad(theta):
        key = np.asarray(theta, float).tobytes()
        if key not in memo:
            memo.clear()
            f = score(theta)
            g = np.zeros(len(theta))
            if np.isfinite(f):
                d = beliefs.gradient_lg(all_sites=True)    # (on the beliefs the calibration inside score() left)
                if d["info"][0]:
                    f = np.inf
                else:
                    g = -tf.pullback(theta, d["dR"][0, 0], d["dmu"][0])
            memo[key] = (f, g)
        return memo[key]
    if gradient == "analytic":
        opt = _minimise(lambda x: value_and_grad(x)[0], tf.forward(R0, mu0), maxiter, grad=lambda x: value_and_grad(x)[1])
    else:
        opt = _minimise(score, tf.forward(R0, mu0), maxiter)
    opt.n_device_evals = count[0]
    R, mu = tf.back(opt.x)
    return R, mu, -float(opt.fun), opt


def fit_shifts_lg(beliefs, schedule_tree, edges, all_sites=False):
    """The exact maximum-likelihood mean shifts on a GIVEN set of edges, at the parameters of the last assignfactors_lg_.
    The log-likelihood is quadratic in the shifts, its score linear: g(s) = g(0) - H s.  One evaluation of
    loglik_and_shift_gradient_lg at s = 0 and one per unit vector (step 1: exact up to rounding, no step size to choose)
    give g(0) and the columns of H -- n p + 1 evaluations for n edges of p traits; H is symmetrised and H s = g(0) solved
    by Cholesky on the host; one more evaluation at the solution leaves the engine (shifts, factors and calibrated beliefs)
    at it and gives its log-likelihood: n p + 2 evaluations (fill + calibrate + edge sweep each) in all.  EXACT ON A CLIQUE TREE ONLY, as the sweeps it calls; not verified.
    edges: (family, k) pairs or flat indices, as set_shifts_lg.  all_sites: one fit per site (the engine is left with one
    set of shifts per site), else the current site's fit, set for all sites.
    Returns a dict: shifts [n, p], loglik, H [n p, n p] (the observed information of the shifts, entries ordered edge-major,
    trait-minor: H^-1 is their covariance) and se [n, p]; with a leading site axis when all_sites.
    If H is not positive definite the shifts are not identified from these data (two shifts with the same tips below them,
    a trait that no tip below observes): ValueError names the (edge, trait) of the failing pivot."""
    e = beliefs._shift_edges(edges)
    n, p = int(e.size), beliefs._lg_p
    if n == 0:
        raise ValueError("fit_shifts_lg: no edge given")
    nf = len(beliefs._lg["cluster"])
    K = beliefs._lg["length"].size // nf
    sites = list(range(beliefs.n_sites)) if all_sites else [beliefs.site]

    def evaluate(values):
        beliefs.set_shifts_lg(e, values)
        ll, g = beliefs.loglik_and_shift_gradient_lg(schedule_tree, all_sites=True)
        if not np.all(np.isfinite(ll[sites])):
            raise np.linalg.LinAlgError("fit_shifts_lg: the calibration failed (a belief is not positive definite)")
        return ll, g.reshape(beliefs.n_sites, n * p)

    _, g0 = evaluate(np.zeros((n, p)))
    H = np.zeros((beliefs.n_sites, n * p, n * p))
    for j in range(n * p):
        unit = np.zeros(n * p)
        unit[j] = 1.0
        _, gj = evaluate(unit.reshape(n, p))
        H[:, :, j] = g0 - gj
    H = (H + H.transpose(0, 2, 1)) / 2
    shat = np.zeros((beliefs.n_sites, n * p))
    se = np.zeros((beliefs.n_sites, n * p))
    for s in sites:
        Lc = _cholesky_or_name(H[s], e, K, p)
        shat[s] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, g0[s]))
        Li = np.linalg.solve(Lc, np.eye(n * p))
        se[s] = np.sqrt(np.sum(Li * Li, axis=0))   # diag(H^-1) = column norms of L^-1
    if all_sites:
        ll, _ = evaluate(shat.reshape(beliefs.n_sites, n, p))
        return dict(shifts=shat.reshape(-1, n, p), loglik=ll, H=H, se=se.reshape(-1, n, p))
    s = beliefs.site
    ll, _ = evaluate(shat[s].reshape(n, p))
    return dict(shifts=shat[s].reshape(n, p), loglik=float(ll[s]), H=H[s], se=se[s].reshape(n, p))


def _cholesky_or_name(H, edges, K, p):
    """Lower Cholesky factor of H, or ValueError naming the (edge, trait) of the first pivot that is not positive.  A pivot
    at or below 1e-10 of its own diagonal entry counts as not positive: H is made of differences of scores that are exact
    to about 1e-13 relative, below that a pivot is rounding noise."""
    m = H.shape[0]
    Lc = np.zeros_like(H)
    for j in range(m):
        d = H[j, j] - Lc[j, :j] @ Lc[j, :j]
        if not (d > 1e-10 * abs(H[j, j])) or not np.isfinite(d):
            f, k = int(edges[j // p]) // K, int(edges[j // p]) % K
            raise ValueError(f"fit_shifts_lg: the shifts are not identified from these data: pivot {j} (edge (family {f}, "
                             f"parent {k}), trait {j % p}) of the information matrix is not positive ({d:.3g})")
        Lc[j, j] = np.sqrt(d)
        Lc[j + 1:, j] = (H[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    return Lc


def select_shifts_lg(beliefs, schedule_tree, max_shifts, min_lr=0.0, candidates=None, min_info=1e-8):
    """Greedy forward selection of mean shifts at the current site, on a clique tree, at the parameters of the last
    assignfactors_lg_.  It starts from no shift (shifts in force are cleared) and repeats:
      1. loglik_and_shift_scan_lg under the shifts chosen so far: per family the gain lr of a jump there, the others held;
      2. the candidates are one edge per family -- the parent edge with the largest gamma, ties to the lowest k (every
         parent edge of a hybrid has the family's lr) -- without the edges already chosen, the families outside `candidates`
         (family indices) when it is given, root-prior families and families with no identified trait;
      3. the largest lr (ties to the lowest family) enters, unless it is below min_lr or max_shifts is reached; ALL chosen
         shifts are then refitted jointly by fit_shifts_lg;
      4. if that refit raises because the joint information is not positive definite (the new shift is not identified next to
         the chosen ones), the previous shifts are put back on the engine, with its factors and calibrated beliefs, the
         candidate is excluded for good and the next one is taken.
    Returns a dict: path -- per step edge (family, k), lr and dof at entry, loglik after the joint refit and the shifts
    [step + 1, p] of all chosen edges --, edges [(family, k)] in order of entry, fit (the last fit_shifts_lg dict; None when
    nothing entered) and loglik0 (the log-likelihood without shifts).  The engine is left at the last fit.
    min_lr HAS NO STATISTICAL DEFAULT: lr is a maximum over all edges, not one chi-square draw.  Without any jump in the data
    the largest lr of the 39-node test networks reaches 13.1, so a per-edge rule such as AIC (lr > 2 dof) over-selects; choose
    min_lr from a null simulation of the network at hand, or fix max_shifts.  p-values are out of scope."""
    nf = len(beliefs._lg["cluster"])
    K = beliefs._lg["length"].size // nf
    p = beliefs._lg_p
    gam = np.asarray(beliefs._lg["gamma"], np.float64).reshape(nf, K)
    npar = np.asarray(beliefs._lg["n_parents"]).reshape(nf)
    best_k = np.array([int(np.argmax(gam[f, :npar[f]])) if npar[f] > 0 else -1 for f in range(nf)])   # (argmax: first of ties)
    allowed = np.ones(nf, bool) if candidates is None else np.isin(np.arange(nf), np.asarray(list(candidates), np.int64))
    allowed &= best_k >= 0
    chosen, values = [], np.zeros((0, p))
    path, fit, ll0 = [], None, None
    beliefs.clear_shifts_lg()
    while len(chosen) < int(max_shifts):
        ll, scan = beliefs.loglik_and_shift_scan_lg(schedule_tree, min_info=min_info)
        if ll0 is None:
            ll0 = ll
        lr = np.where(allowed & (scan["dof"] > 0) & np.isfinite(scan["lr"]), scan["lr"], -np.inf)
        for f, k in chosen:
            if best_k[f] == k:
                lr[f] = -np.inf
        entered = False
        for f in np.argsort(-lr, kind="stable"):
            if not np.isfinite(lr[f]) or lr[f] < min_lr:
                break
            edge = (int(f), int(best_k[f]))
            try:
                fit_new = fit_shifts_lg(beliefs, schedule_tree, chosen + [edge])
            except ValueError:
                allowed[f] = False
                if chosen:
                    beliefs.set_shifts_lg(chosen, values)
                else:
                    beliefs.clear_shifts_lg()
                beliefs.loglik_and_shift_gradient_lg(schedule_tree)   # factors and beliefs under the restored shifts
                continue
            fit = fit_new
            chosen.append(edge)
            values = fit["shifts"].copy()
            path.append(dict(edge=edge, lr=float(scan["lr"][f]), dof=int(scan["dof"][f]), loglik=fit["loglik"],
                             shifts=values.copy()))
            entered = True
            break
        if not entered:
            break
    return dict(path=path, edges=list(chosen), fit=fit, loglik0=ll0)


def bootstrap_shift_scan_lg(beliefs, schedule_tree, seed=None, z=None, min_info=1e-8, sites=False):
    """Parametric bootstrap of the shift scan on a clique tree: the null distribution of the LARGEST lr over all edges, which
    has no closed form.  On an engine with B sites -- B replicates of one network, built with n_sites = B and the fitted null
    model assigned (assignfactors_lg_, with the shifts and the tip noise that belong to the null in force) -- it
      1. reads the data in force (get_data_lg), so that the caller can put them back;
      2. simulates B data sets under the current model straight into the engine's data (simulate_lg(write_data=True,
         all_sites=True), with the device's generator from `seed` or from the caller's normals z [B, n_families, p]);
      3. fills, calibrates and scans every replicate at once (loglik_and_shift_scan_lg(all_sites=True, min_info=min_info));
      4. takes per replicate the largest lr over the families select_shifts_lg would consider (dof > 0, lr finite; ties to
         the lowest family) and the edge it would enter there (the parent edge with the largest gamma, ties to the lowest k).
    Returns a dict: max_lr [B] (-inf for a replicate without any identified family, NaN for one whose info is not 0),
    family [B] and edge [B, 2] = (family, k) of that maximum (-1 where there is none), loglik [B], info [B] (the simulation's,
    else the calibration's), x [B, n_families, p] (the simulated states), data [B, n_rows, p] (the simulated tip data, as the
    engine now holds them) and data_before (what it held: set_data_lg(out["data_before"]) restores it; nothing is refilled
    until the next assignfactors_lg_ / loglik_lg).
    sites=True (a thread-per-site engine: one trait, every belief of at most 2 variables, B >= 8): step 3 is
    loglik_and_shift_scan_sites_lg(tables=False), lanes = replicates -- the scan converts no layout and steps 3 and 4 fetch
    no table: the maximum and its family are taken on the device, the edge from that family.  The same keys; max_lr agrees
    with the default path to rounding.
    THRESHOLD: a quantile of max_lr calibrates select_shifts_lg -- min_lr = np.quantile(max_lr, 0.95) lets a first shift
    enter a data set WITHOUT any jump with probability about 5 % (Monte Carlo error of the quantile: about
    sqrt(0.05 * 0.95 / B) / density; B of a few hundred).  It is the threshold of the FIRST step; later steps scan under the
    chosen shifts, for which the same call, with those shifts in force, gives the matching null.  Exact on a clique tree
    only, like the scan."""
    before = beliefs.get_data_lg()
    x, sim_info = beliefs.simulate_lg(z=z, seed=seed, write_data=True, all_sites=True)
    nf = len(beliefs._lg["cluster"])
    K = beliefs._lg["length"].size // nf
    gam = np.asarray(beliefs._lg["gamma"], np.float64).reshape(nf, K)
    npar = np.asarray(beliefs._lg["n_parents"]).reshape(nf)
    best_k = np.array([int(np.argmax(gam[f, :npar[f]])) if npar[f] > 0 else -1 for f in range(nf)])
    if sites:
        ll, scan = beliefs.loglik_and_shift_scan_sites_lg(schedule_tree, min_info=min_info, tables=False)
        info = np.where(sim_info != 0, sim_info, scan["info"])
        fam = scan["top_family"].astype(np.int64)
        none = fam < 0
        edge = np.stack([fam, np.where(none, -1, best_k[fam])], axis=1)
        top = np.where(info != 0, np.nan, np.where(none, -np.inf, scan["top_lr"]))
        return dict(max_lr=top, family=fam, edge=edge, loglik=ll, info=info, x=x, data=beliefs.get_data_lg(), data_before=before)
    ll, scan = beliefs.loglik_and_shift_scan_lg(schedule_tree, all_sites=True, min_info=min_info)
    info = np.where(sim_info != 0, sim_info, scan["info"])
    lr = np.where((best_k >= 0)[None, :] & (scan["dof"] > 0) & np.isfinite(scan["lr"]), scan["lr"], -np.inf)
    fam = np.argmax(lr, axis=1)                        # (argmax: first of ties)
    top = lr[np.arange(lr.shape[0]), fam]
    none = ~np.isfinite(top)
    fam = np.where(none, -1, fam)
    edge = np.stack([fam, np.where(none, -1, best_k[fam])], axis=1)
    top = np.where(info != 0, np.nan, top)
    return dict(max_lr=top, family=fam, edge=edge, loglik=ll, info=info, x=x, data=beliefs.get_data_lg(), data_before=before)


def add_optimum_shift(regime, parent_family, family):
    """Refine a regime map by clade(family): the nested-shift parametrisation optimum_scan_sites_lg scans.  regime: the int
    map [n_families, K] (or flat) of set_optima_lg on a TREE (one parent per family: K = 1, or only column 0 in use), 0 = the
    edge keeps theta; parent_family [n_families * K]: what lg_families gives (the family of each parent, negative: a root);
    family: the family above whose edge the optimum shifts.  Every regime that meets the clade -- the edge above `family` and
    all edges below it -- is split: its edges inside the clade get a new regime, in the order the old regimes are first met
    in family order.  Returns (new_regime, origin): new_regime shaped as `regime`; origin[r - 1] is the regime the new map's
    regime r came from (0: theta; origin[r - 1] == r for the regimes the old map had).  A caller sets the values of a new
    regime r to value[origin[r - 1]] + delta (value[0] = theta) and keeps the others.  Pure numpy."""
    reg = np.array(regime, np.int32, copy=True)
    shape = reg.shape
    nf = shape[0] if reg.ndim >= 1 else 1    # (a flat map is that of a table with K = 1, as a tree's is)
    K = max(1, reg.size // max(1, nf))
    if np.asarray(parent_family).size != nf * K:
        raise ValueError(f"add_optimum_shift: parent_family has {np.asarray(parent_family).size} entries, the map {nf * K}")
    reg = reg.reshape(nf, K)
    pf = np.asarray(parent_family, np.int64).reshape(nf, K)[:, 0]
    family = int(family)
    if not 0 <= family < nf:
        raise ValueError(f"add_optimum_shift: family {family} out of range ({nf} families)")
    inside = np.zeros(nf, bool)
    inside[family] = True
    for f in range(family + 1, nf):          # families are in preorder: a parent comes before its children
        inside[f] = pf[f] >= 0 and inside[pf[f]]
    n_old = int(reg.max()) if reg.size else 0
    origin = list(range(1, n_old + 1))
    new_of = {}
    out = reg.copy()
    for f in np.flatnonzero(inside):
        r = int(reg[f, 0])
        if r not in new_of:
            origin.append(r)
            new_of[r] = len(origin)
        out[f, 0] = new_of[r]
    return out.reshape(shape), np.array(origin, np.int32)


def bootstrap_optimum_scan_lg(beliefs, schedule_tree, seed=None, z=None, min_info=1e-8):
    """Parametric bootstrap of the optimum-shift scan on a clique tree: the null distribution of the LARGEST lr over all edges
    of optimum_scan_sites_lg -- the twin of bootstrap_shift_scan_lg(sites=True).  On a thread-per-site engine with B sites (B
    replicates of one tree, the fitted null model assigned) it reads the data in force, simulates B data sets under the
    current model into the engine's data (simulate_lg(write_data=True, all_sites=True)), fills, calibrates and scans every
    replicate at once (loglik_and_optimum_scan_sites_lg(tables=False): no table is fetched, the maximum and its family are
    taken on the device).  Returns a dict: max_lr [B] (-inf for a replicate without any identified family, NaN where info is
    not 0), family [B] (-1 where there is none), loglik [B], info [B], x, data and data_before as bootstrap_shift_scan_lg.
    np.quantile(max_lr, 0.95) is the threshold at which a first clade's optimum shifts with probability about 5 % under the
    null.  WITH PAINTED OPTIMA IN FORCE the call inherits simulate_lg's refusal (the simulation does not honour them yet), so
    today it calibrates the FIRST shift only."""
    before = beliefs.get_data_lg()
    x, sim_info = beliefs.simulate_lg(z=z, seed=seed, write_data=True, all_sites=True)
    ll, scan = beliefs.loglik_and_optimum_scan_sites_lg(schedule_tree, min_info=min_info, tables=False)
    info = np.where(sim_info != 0, sim_info, scan["info"])
    fam = scan["top_family"].astype(np.int64)
    top = np.where(info != 0, np.nan, np.where(fam < 0, -np.inf, scan["top_lr"]))
    return dict(max_lr=top, family=fam, loglik=ll, info=info, x=x, data=beliefs.get_data_lg(), data_before=before)


def fit_clade_shifts_sites_lg(beliefs, schedule_tree, min_info=1e-8):
    """Exact joint ML of every site's clade-shift deltas for the families in force (set_clade_shifts_sites_lg), all sites side
    by side: fit_shifts_lg's device, batched over sites.  The log-likelihood of a site is quadratic in its deltas, so m + 1
    evaluations (fill, calibration, clade_shift_score_sites_lg -- each for all sites at once) at the current point and at a
    unit step in each of the m slots give the score g and the joint information H exactly: column k of H is g(d) - g(d + e_k).
    H step = g is solved per site on the host by an elimination in slot order; a pivot that is not above min_info Kt of its
    slot drops that slot AT THAT SITE (identified False, its delta left where it was) and does not raise.  One more
    evaluation leaves the engine filled and calibrated at the estimate.  alpha and the rates are held where the last
    assignfactors_lg_ put them.  Returns a dict: delta [m, n_sites], H [n_sites, m, m] (symmetrised; rows and columns of
    empty slots 0), se [m, n_sites] (NaN at empty or dropped slots), loglik [n_sites] at the estimate, identified
    [m, n_sites], g [m, n_sites] (the score at the starting point), info [n_sites]."""
    st = beliefs.clade_shifts_sites_lg()
    if st is None:
        raise ValueError("fit_clade_shifts_sites_lg: no clade shifts are set (call set_clade_shifts_sites_lg first)")
    fam, d0 = st["family"], st["delta"]
    m, n = fam.shape
    used = fam >= 0

    def evaluate(d):
        beliefs.update_clade_shifts_sites_lg(d)
        ll, sc = beliefs.loglik_and_clade_shift_score_sites_lg(schedule_tree, min_info=min_info)
        return ll, sc

    ll0, sc0 = evaluate(d0)
    g0 = np.where(used, sc0["g"], 0.0)
    kt = np.where(used, sc0["kt"], 0.0)
    H = np.zeros((n, m, m))
    for k in range(m):
        if not used[k].any():
            continue
        step = d0.copy()
        step[k] += 1.0
        _, sck = evaluate(step)
        H[:, :, k] = (g0 - np.where(used, sck["g"], 0.0)).T
    H = 0.5 * (H + H.transpose(0, 2, 1))
    H[~(used.T[:, :, None] & used.T[:, None, :])] = 0.0
    # elimination in slot order, vectorised over sites: which slots keep a positive pivot
    keep = used.T & np.isfinite(g0.T) & np.isfinite(H).all(axis=2)       # [n, m]
    Lc = np.zeros((n, m, m))
    for k in range(m):
        piv = H[:, k, k] - np.einsum("nj,nj->n", Lc[:, k, :k], Lc[:, k, :k])
        ok = keep[:, k] & (piv > min_info * kt[k]) & (piv > 0.0)
        keep[:, k] = ok
        rt = np.sqrt(np.where(ok, piv, 1.0))
        for i in range(k + 1, m):
            v = (H[:, i, k] - np.einsum("nj,nj->n", Lc[:, i, :k], Lc[:, k, :k])) / rt
            Lc[:, i, k] = np.where(ok, v, 0.0)
        Lc[:, k, k] = np.where(ok, rt, 0.0)
    pair = keep[:, :, None] & keep[:, None, :]
    Hk = np.where(pair, H, 0.0) + np.eye(m)[None] * (~keep)[:, :, None]   # dropped slots: an identity row and column
    gk = np.where(keep, g0.T, 0.0)
    step = np.linalg.solve(Hk, gk[:, :, None])[:, :, 0]
    cov = np.linalg.inv(Hk)
    se = np.where(keep, np.sqrt(np.abs(np.einsum("nkk->nk", cov))), np.nan).T
    delta = d0 + np.where(keep, step, 0.0).T
    ll, sc = evaluate(delta)
    return dict(delta=delta, H=np.where(used.T[:, :, None] & used.T[:, None, :], H, 0.0), se=se, loglik=ll, identified=keep.T.copy(),
                g=g0, score=sc, info=sc["info"])


def select_optimum_shifts_sites_lg(beliefs, schedule_tree, max_shifts, min_lr, min_info=1e-8):
    """Forward selection of clade shifts of the optimum for all sites of a univariate batch at once (the workflow of l1ou,
    bayou and PhylogeneticEM on the nested-shift parametrisation).  It starts from no clade shift (a setting in force is
    cleared; painted optima, shifts, noise and masks stay) and repeats up to max_shifts times: scan
    (optimum_scan_sites_lg(tables=False)); every site still going whose top_lr exceeds min_lr puts its top_family into its
    next empty slot, the others stop for good; joint refit of all slots (fit_clade_shifts_sites_lg), whose last evaluation
    leaves the engine calibrated for the next scan.  alpha and the rates are held at their fitted values, as PhylogeneticEM
    holds alpha.  min_lr: a threshold for the first step comes from bootstrap_optimum_scan_lg under the null fit; the
    simulation refuses while a setting is in force, so the later steps reuse that threshold -- an APPROXIMATION, since the null
    distribution of the largest lr changes once clades are in the model.
    Returns a dict: family int [max_shifts, n_sites] (-1: unused), delta [max_shifts, n_sites] (the final joint estimates),
    lr [max_shifts, n_sites] (top_lr at entry, NaN where unused), loglik [steps + 1, n_sites] (row 0: no shift; a site that
    has stopped keeps its value), n_shifts [n_sites], info [n_sites].  The engine is left with the selected setting in force."""
    max_shifts = int(max_shifts)
    n = beliefs.n_sites
    beliefs.clear_clade_shifts_sites_lg()
    fam = np.full((max(1, max_shifts), n), -1, np.int32)
    delta = np.zeros((max(1, max_shifts), n))
    lr = np.full((max(1, max_shifts), n), np.nan)
    ll, scan = beliefs.loglik_and_optimum_scan_sites_lg(schedule_tree, min_info=min_info, tables=False)
    path = [ll]
    info = scan["info"].copy()
    going = info == 0
    n_shifts = np.zeros(n, np.int64)
    for step in range(max_shifts):
        top, tf = scan["top_lr"], scan["top_family"].astype(np.int64)
        with np.errstate(invalid="ignore"):
            enter = going & (tf >= 0) & (top > float(min_lr))
        enter &= ~(fam == tf[None, :]).any(axis=0)      # (a family in force has lr ~ 0 after the refit: not reached)
        going = enter
        if not enter.any():
            break
        fam[step, enter] = tf[enter]
        lr[step, enter] = top[enter]
        n_shifts[enter] += 1
        beliefs.set_clade_shifts_sites_lg(fam, delta)
        fit = fit_clade_shifts_sites_lg(beliefs, schedule_tree, min_info=min_info)
        delta = fit["delta"]
        path.append(np.where(fit["info"] != 0, np.nan, fit["loglik"]))
        info = np.where(info != 0, info, fit["info"])
        going &= fit["info"] == 0
        if step + 1 < max_shifts:
            scan = beliefs.optimum_scan_sites_lg(min_info=min_info, tables=False)
    return dict(family=fam[:max_shifts], delta=delta[:max_shifts], lr=lr[:max_shifts], loglik=np.array(path), n_shifts=n_shifts,
                info=info)


def lbfgs_sites(value_and_grad, x0, maxiter=200, gtol=1e-8, memory=8, c1=1e-4):
    """Batched L-BFGS: minimises n independent functions of d variables side by side, one callback per step for all of them.
    value_and_grad(X [n, d]) -> (f [n], g [n, d]) evaluates every site at its row of X; a site whose value or gradient is
    not finite there has FAILED at that point (NaN is how the caller reports info != 0).  A pure function of the callback.
    Each site has its own history (`memory` pairs), direction and step.  Armijo backtracking: a site whose trial point
    fails f(x + t d) <= f(x) + c1 t g'd, or fails outright, halves its step; the others keep their accepted point (a site
    that is not moving is evaluated at its accepted point again and the result dropped: its x, f, g keep their bytes).  A
    pair (s, y) enters the history only when s'y > 1e-10 |s| |y|; a direction that is not a descent direction, or a step
    below 1e-12 of its first trial, drops the history and restarts from steepest descent; a steepest-descent step that small
    stops the site unconverged.  A site stops when max|g| <= gtol max(1, |f|), or after `maxiter` accepted steps.
    Returns a dict: x [n, d], f [n], g [n, d], converged [n], n_iter [n] (accepted steps), n_evals (callbacks)."""
    x = np.array(x0, np.float64, copy=True)
    n, d = x.shape
    m = int(memory)

    def evaluate(X):
        f, g = value_and_grad(X)
        f = np.array(f, np.float64, copy=True).reshape(n)
        g = np.array(g, np.float64, copy=True).reshape(n, d)
        ok = np.isfinite(f) & np.all(np.isfinite(g), axis=1)
        return f, g, ok

    f, g, ok = evaluate(x)
    n_evals = 1
    S, Y = np.zeros((m, n, d)), np.zeros((m, n, d))
    rho = np.zeros((m, n))
    n_hist = np.zeros(n, np.int64)
    n_iter = np.zeros(n, np.int64)

    def is_converged(f, g):
        return np.max(np.abs(g), axis=1, initial=0.0) <= gtol * np.maximum(1.0, np.abs(f))
    converged = ok & is_converged(np.where(ok, f, 0.0), np.where(ok[:, None], g, np.inf))
    stopped = converged | ~ok                     # (a start that fails cannot move: stopped, not converged)
    steepest = np.zeros(n, bool)

    def direction(sel):
        """-H g of the sites sel by the two-loop recursion over their own histories (slot m - 1 is the newest)"""
        q = g[sel].copy()
        nh = n_hist[sel]
        al = np.zeros((m, q.shape[0]))
        for j in range(m - 1, -1, -1):
            valid = j >= m - nh
            al[j] = np.where(valid, rho[j, sel] * np.sum(S[j, sel] * q, axis=1), 0.0)
            q -= al[j][:, None] * Y[j, sel]
        sy = np.sum(S[m - 1, sel] * Y[m - 1, sel], axis=1)
        yy = np.sum(Y[m - 1, sel] * Y[m - 1, sel], axis=1)
        gnorm = np.sqrt(np.sum(g[sel] * g[sel], axis=1))
        h0 = np.where(nh > 0, sy / np.where(yy > 0, yy, 1.0), 1.0 / np.maximum(1.0, gnorm))
        r = h0[:, None] * q
        for j in range(m):
            valid = j >= m - nh
            be = np.where(valid, rho[j, sel] * np.sum(Y[j, sel] * r, axis=1), 0.0)
            r += np.where(valid, al[j] - be, 0.0)[:, None] * S[j, sel]
        return -r

    dirn = np.zeros((n, d))
    slope = np.zeros(n)
    step = np.ones(n)

    def new_direction(sel):
        """direction, slope and first step of the sites sel (a boolean mask); steepest descent where L-BFGS gives no descent"""
        if not sel.any():
            return
        idx = np.nonzero(sel)[0]
        dd = direction(idx)
        sl = np.sum(dd * g[idx], axis=1)
        bad = ~(sl < 0.0) | ~np.all(np.isfinite(dd), axis=1)
        if bad.any():
            b = idx[bad]
            n_hist[b] = 0
            gn = np.sqrt(np.sum(g[b] * g[b], axis=1))
            dd[bad] = -g[b] / np.maximum(1.0, gn)[:, None]
            sl[bad] = np.sum(dd[bad] * g[b], axis=1)
        steepest[idx] = bad
        dirn[idx], slope[idx], step[idx] = dd, sl, 1.0

    new_direction(~stopped)
    while not stopped.all():
        active = ~stopped
        trial = np.where(active[:, None], x + step[:, None] * dirn, x)
        ft, gt, okt = evaluate(trial)
        n_evals += 1
        with np.errstate(invalid="ignore"):
            accept = active & okt & (ft <= f + c1 * step * slope)
        reject = active & ~accept
        if accept.any():
            a = np.nonzero(accept)[0]
            s = trial[a] - x[a]
            y = gt[a] - g[a]
            sy = np.sum(s * y, axis=1)
            keep = sy > 1e-10 * np.sqrt(np.sum(s * s, axis=1) * np.sum(y * y, axis=1))
            k = a[keep]
            if k.size:
                S[:-1, k], Y[:-1, k], rho[:-1, k] = S[1:, k], Y[1:, k], rho[1:, k]
                S[-1, k], Y[-1, k], rho[-1, k] = s[keep], y[keep], 1.0 / sy[keep]
                n_hist[k] = np.minimum(m, n_hist[k] + 1)
            x[a], f[a], g[a] = trial[a], ft[a], gt[a]
            n_iter[a] += 1
            conv = np.zeros(n, bool)
            conv[a] = is_converged(f[a], g[a])
            converged |= conv
            stopped |= conv | (accept & (n_iter >= maxiter))
            new_direction(accept & ~stopped)
        if reject.any():
            step[reject] *= 0.5
            tiny = reject & (step < 1e-12)
            give_up = tiny & steepest
            stopped |= give_up
            restart = tiny & ~steepest
            if restart.any():
                n_hist[restart] = 0
                new_direction(restart)      # (no history: steepest descent, from step 1)
                steepest[restart] = True
    return dict(x=x, f=f, g=g, converged=converged, n_iter=n_iter, n_evals=n_evals)


def fit_sites_lg(beliefs, schedule_tree, model, R0, mu0, alpha0=None, theta0=None, extra_rates=(), fit_mu=True, maxiter=200,
                 gtol=1e-8, memory=8, optima0=None):
    """Maximum-likelihood fit of EVERY SITE of a univariate batch at once, on a clique tree, on the thread-per-site kernels
    (p = 1, every belief of at most 2 variables, at least 8 sites).  model: "bm" or "ou".  Each site has its own free
    parameters: log R[0] (the BM rate; under OU the stationary variance), mu when fit_mu, and under OU log alpha and theta.
    R0, mu0, alpha0, theta0: scalars or [n_sites] start values; extra_rates: the rates that follow R[0] in the rate table of
    lg_setup (scalars or [n_sites], e.g. a random root's prior variance), held at these values.
    Every evaluation is ONE device pass for all sites -- assignfactors_lg_ with per-site parameters, then
    loglik_and_gradient_sites_lg (reset, calibrate, root integrate, the lanes-are-sites sweep) -- driven by lbfgs_sites.
    A site stops when max|g| <= gtol max(1, |loglik|) in the transformed parameters, or after maxiter steps.
    Returns a dict of per-site arrays R, mu, alpha, theta (alpha, theta: NaN under BM), loglik, converged, n_iter, and
    n_device_evals; the engine is left filled and calibrated at the estimates.
    A per-site mask of missing tips (set_site_missing_lg) needs no change here: every evaluation refills the factors, whose
    correction skips the masked tips of each site, and the gradient sweep reads the same mask -- each site is fitted to its
    own observed tips (tests/test_gpu_site_missing.py: against the closed-form GLS optimum of every site).
    optima0 ([n_regimes] or [n_sites, n_regimes]; OU only): painted optima (Hansen's model).  The regime map is the one in
    force (set_optima_lg first; its values are replaced); each site then also fits its own theta_r, one more free parameter
    per regime with the derivative doptima of the sweep, and the result gains optima [n_sites, n_regimes].  theta stays the
    optimum of the unpainted edges.  Every evaluation uploads n_sites x n_regimes numbers (update_optima_lg).  With the default the function
    is what it was."""
    if model not in ("bm", "ou"):
        raise ValueError(f"fit_sites_lg: model must be 'bm' or 'ou', not {model!r}")
    ou = model == "ou"
    if ou and (alpha0 is None or theta0 is None):
        raise ValueError("fit_sites_lg: the OU model needs alpha0 and theta0")
    n = beliefs.n_sites
    painted = optima0 is not None
    if painted:
        if not ou:
            raise ValueError("fit_sites_lg: optima0 needs the OU model (under BM the optima have no effect)")
        cur = beliefs.optima_lg()
        if cur is None:
            raise ValueError("fit_sites_lg: optima0 given but no regimes are painted (call set_optima_lg first)")
        regime, n_reg = cur["regime"], cur["values"].shape[-2]
        o0 = np.asarray(optima0, np.float64)
        if o0.shape not in ((n_reg,), (n, n_reg)):
            raise ValueError(f"fit_sites_lg: optima0 must be [{n_reg}] or [{n}, {n_reg}], not {list(o0.shape)}")
        o0 = np.broadcast_to(o0, (n, n_reg)).copy()
    site = lambda v: np.broadcast_to(np.asarray(v, np.float64).reshape(-1), (n,)).copy()
    extra = [site(r) for r in extra_rates]
    mu_fixed = site(mu0)
    cols = [np.log(site(R0))] + ([mu_fixed.copy()] if fit_mu else []) + ([np.log(site(alpha0)), site(theta0)] if ou else [])
    i_mu = 1 if fit_mu else None
    i_al = (2 if fit_mu else 1) if ou else None
    if painted:
        i_op = len(cols)
        cols = cols + [o0[:, r] for r in range(n_reg)]
    count = [0]

    def unpack(X):
        with np.errstate(over="ignore"):
            R = np.exp(X[:, 0])
            alpha = np.exp(X[:, i_al]) if ou else None
        return R, (X[:, i_mu] if fit_mu else mu_fixed), alpha, (X[:, i_al + 1] if ou else None)

    def value_and_grad(X):
        R, mu, alpha, theta = unpack(X)
        rates = np.stack([R] + extra, axis=1)[:, :, None, None]
        kw = dict(model="ou", alpha=alpha, theta=theta[:, None]) if ou else {}
        if painted:
            beliefs.update_optima_lg(X[:, i_op:])   # (the values alone: n_sites x n_regimes numbers)
        beliefs.assignfactors_lg_(rates, mu[:, None], **kw)
        count[0] += 1
        ll, d = beliefs.loglik_and_gradient_sites_lg(schedule_tree)
        g = [d["dR"][:, 0, 0, 0] * R] + ([d["dmu"][:, 0]] if fit_mu else []) + ([d["dalpha"] * alpha, d["dtheta"][:, 0]] if ou else [])
        if painted:
            g = g + [d["doptima"][:, r, 0] for r in range(n_reg)]
        f = np.where(d["info"] != 0, np.nan, -ll)
        return f, -np.stack(g, axis=1)

    if painted:   # per-site values from here on; every evaluation then moves the values alone
        beliefs.set_optima_lg(regime, o0[:, :, None])
    beliefs._ensure_schedule([schedule_tree])
    opt = lbfgs_sites(value_and_grad, np.stack(cols, axis=1), maxiter=maxiter, gtol=gtol, memory=memory)
    f_end, _ = value_and_grad(opt["x"])   # the engine filled and calibrated at the estimates (the last trial points are not)
    R, mu, alpha, theta = unpack(opt["x"])
    nan = np.full(n, np.nan)
    out = dict(R=R, mu=np.array(mu, copy=True), alpha=alpha if ou else nan, theta=np.array(theta, copy=True) if ou else nan.copy(),
               loglik=-opt["f"], converged=opt["converged"], n_iter=opt["n_iter"], n_device_evals=count[0])
    if painted:
        out["optima"] = np.array(opt["x"][:, i_op:], copy=True)
    return out

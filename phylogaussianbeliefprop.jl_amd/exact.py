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

"""The comparators of the closed-form BM fit of a univariate batch (tests/exact_uni_ref.py), pinned on the CPU: at every site of
every case the GPU file runs, the numpy restatement of the sweep over the dense flat-prior posterior against per-site generalised
least squares on the tips that site observes -- mu_hat, the REML rate r'C^-1 r / (n_obs - 1) with C = site_missing_ref.bm_cov
restricted to the observed rows, den against n_obs - 1, and under shifts GLS on y minus the displacement of the tips.

Tolerance: both sides are dense float64 solves of the same small systems (at most 131 nodes); their error is bounded by
cond x eps x size.  The worst condition number of an observed block of bm_cov is printed and asserted below 1e4, so
1e4 x 2.2e-16 x 131 = 3e-10 bounds the disagreement; 1e-9 relative to max(1, |value|) is asserted, the measured figures (printed)
are four to five orders below it."""
import numpy as np
import pytest

import exact_uni_ref as XR
import fam_uni_ref as FR
import site_missing_ref as SM
from shift_ref import family_nodes

TOL = 1e-9
ALL = [(k, n) for k, counts in XR.PLAIN + XR.MASKED for n in counts]


@pytest.mark.parametrize("key,n", ALL, ids=[f"{k}-{n}" for k, n in ALL])
def test_restatement_equals_gls(key, n):
    case = XR.get(key, n)
    ref, g = XR.reference(key, n), XR.gls_all(key, n)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    e_R, e_mu, e_den = rel(ref["num"] / ref["den"], g["R"]), rel(ref["mu"], g["mu"]), rel(ref["den"], g["n_obs"] - 1.0)
    cond = max(np.linalg.cond(case.cov[np.ix_(o, o)]) for o in (XR.observed(case, s) for s in range(n)))
    print(f"{key}/{n}: restatement against GLS at {n} sites: R_hat {e_R:.1e}, mu_hat {e_mu:.1e}, den against n_obs - 1 {e_den:.1e}; "
          f"smallest den {ref['den'].min():.3f}; worst cond of an observed block {cond:.1e}")
    assert cond < 1e4
    assert max(e_R, e_mu, e_den) <= TOL
    if case.mask is not None:
        rows, fam_of = SM.tip_rows(case)
        assert np.array_equal(g["n_obs"], (~case.mask[:, rows]).sum(axis=1))
        # a masked tip's family adds nothing; an internal family whose clade is wholly masked adds 0 to both sums
        for s, r in zip(*np.nonzero(case.mask)):
            assert np.isnan(ref["terms"][s, fam_of[int(r)], 0])
        if "clade" in case.planted_mask:
            s, cl = case.planted_mask["clade"]
            gone = {case.taxa[r] for r in np.flatnonzero(case.mask[s])}
            nodes = family_nodes(case.ocgb0, case.fam)
            inner = [f for f, i in enumerate(nodes) if int(case.fam["child_pos"][f]) >= 0 and int(case.fam["n_parents"][f]) > 0
                     and set(FR._tips_below(case.net, case.net.vec_node[i])) <= gone]
            worst = max(float(np.max(np.abs(ref["terms"][s, f]))) for f in inner)
            print(f"{key}/{n}: site {s} masks the clade of rows {cl}: its {len(inner)} internal families stay in the sweep and add "
                  f"at most {worst:.1e} to either sum")
            assert inner and worst <= 1e-12   # (e = 0 and C = t to rounding: terms of size eps)
    if case.shifts is not None:
        assert max(np.max(np.abs(XR.tip_displacement(case, s))) for s in range(n)) > 0.1


def test_smallest_den():
    """every masked site observes at least 3 tips: the smallest den is at least 2"""
    low = XR.smallest_den()
    print(f"smallest den over the masked cases: {low}")
    assert low >= 2


def test_planted_entries():
    """what the masks must hold: a site that masks nothing, a cherry and a clade of at least 3 tips wholly masked at one site
    each, bits at lanes 0 and 63 of word 0 and at site 64, about 30 % of the entries"""
    c = XR.get("bm40+mask", 65)
    rows, _ = SM.tip_rows(c)
    assert not c.mask[1].any() and c.mask[0].any() and c.mask[63].any() and c.mask[64].any()
    s, _, ch = c.planted_mask["cherry"]
    assert c.mask[s, ch].all()
    s, cl = c.planted_mask["clade"]
    assert len(cl) >= 3 and c.mask[s, cl].all()
    frac = c.mask[:, rows].mean()
    print(f"bm40+mask/65: {frac:.2f} of the entries masked")
    assert 0.2 <= frac <= 0.4

"""The comparator of the lanes-are-sites family sweeps (fam_uni_ref.sweeps: the three closed forms over the family table and
J^-1 h, J^-1 of the oracle's calibrated clique tree) pinned to the dense statements the project already has -- the scan and the
edge derivatives of noise_ref.family_statement (scan_ref / edge_ref with shifts and tip noise) on the dense posterior,
loo_ref.dense_loo -- on every case tests/test_gpu_fam_uni.py uses, one site in eight, at 1e-8 relative to max(1, |block|_inf).

It also checks, from the reference alone, the conditions the GPU tests rely on:
  * a case that claims to test identification has identified and non-identified families;
  * H / j of every family is a factor 1e3 away from min_info, D / V of every tip a factor 1e3 away from 2^-40;
  * where top_family is compared, the largest and the second-largest lr of a site differ by more than 1e-6 relative."""
import numpy as np
import pytest

import fam_uni_ref as FR

TOL = 1e-8
MIN_INFO = 1e-8


def _margins(tag, case, s, sw, fam):
    relH = sw["scan"]["relH"][np.isfinite(sw["scan"]["relH"])]
    assert np.all((relH >= 1e3 * MIN_INFO) | (relH <= MIN_INFO / 1e3)), (tag, s, relH)
    relD = sw["loo"]["relD"]
    assert np.all((relD >= 1e3 * FR.LOO_FLOOR) | (relD <= FR.LOO_FLOOR / 1e3)), (tag, s, relD)
    real = np.asarray(fam["n_parents"]) >= 1
    if case.identification:
        assert sw["scan"]["identified"][real].any() and not sw["scan"]["identified"][real].all(), (tag, s)
    if case.top:
        lr = np.sort(sw["scan"]["lr"][real & sw["scan"]["identified"] & np.isfinite(sw["scan"]["lr"])])
        assert len(lr) >= 2 and lr[-1] - lr[-2] > 1e-6 * lr[-1], (tag, s, lr[-2:])
    return (float(relH[relH >= 1e3 * MIN_INFO].min()) if (relH >= 1e3 * MIN_INFO).any() else np.inf), float(relD.min())


def _pin(case, sites, skip=None):
    worst, lowH, lowD = {}, np.inf, np.inf
    for s in sites:
        sw, fam = FR.reference_site(case, s, MIN_INFO)
        h, d = _margins(case.name, case, s, sw, fam)
        lowH, lowD = min(lowH, h), min(lowD, d)
        skip_tips = (skip[1],) if skip is not None and skip[0] == s else ()
        w = FR.against_dense(sw, FR.dense_site(case, s, MIN_INFO), fam, fam["data_row"][sw["loo"]["families"]], skip_tips)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if case.planted is not None:
            assert sw["scan"]["top_family"] == case.planted, (case.name, s, sw["scan"]["top_family"])
    if case.top:   # the margin of the largest lr at EVERY site the GPU test runs, from the dense statement
        gap = np.inf
        for s in range(len(case.sites)):
            a, b, f = FR.top_margin(case, s, MIN_INFO)
            assert a - b > 1e-6 * a and (case.planted is None or f == case.planted), (case.name, s, a, b, f)
            gap = min(gap, (a - b) / a)
        print(f"{case.name}: the largest lr leads the second by {gap:.2e} relative at the least, over {len(case.sites)} sites")
    print(f"{case.name}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          f"; smallest identified H/j {lowH:.2e}, smallest D/V {lowD:.2e}")
    for k, v in worst.items():
        assert v <= TOL, (case.name, k, v)


PLAIN = list(FR.plain_cases())


@pytest.mark.parametrize("i", range(len(PLAIN)), ids=[c.name for c, _ in PLAIN])
def test_closed_forms_against_the_dense_statements(i):
    case, counts = PLAIN[i]
    _pin(case, FR.checked_sites(max(counts)))


@pytest.mark.parametrize("n_fam,planted", FR.BLOCKS)
def test_block_boundary_cases(n_fam, planted):
    """the planted jump is the site's largest lr at every checked site, by the margin the GPU test needs"""
    case = FR.block_case(n_fam, planted)
    _pin(case, FR.checked_sites(len(case.sites)))


def test_undetermined_tip():
    """improper root: at one site the other data leave one tip's parent undetermined; the reference reports info 1 there (D / V
    below 2^-40 by more than 1e3) and predicts every other tip; the other sites are pinned as usual"""
    case = FR.undetermined_case()
    site, tip = case.undetermined
    for s in range(len(case.sites)):
        sw, fam = FR.reference_site(case, s, MIN_INFO)
        relD = sw["loo"]["relD"]
        assert np.all((relD >= 1e3 * FR.LOO_FLOOR) | (relD <= FR.LOO_FLOOR / 1e3)), (s, relD)
        bad = np.flatnonzero(sw["loo"]["info"])
        assert list(bad) == ([tip] if s == site else []), (s, bad)
        assert np.isnan(sw["loo"]["total"]) == (s == site)
    _pin(case, [0])
    # at the site itself every other tip against the dense leave-one-out
    sw, fam = FR.reference_site(case, site, MIN_INFO)
    dn = FR.dense_site(case, site, MIN_INFO)
    rows = fam["data_row"][sw["loo"]["families"]]
    worst = 0.0
    for ti, r in enumerate(rows):
        if ti == tip:
            continue
        _, mean, cov, lpd = dn["loo"][int(r)]
        worst = max(worst, FR.rel(sw["loo"]["mean"][ti], mean[0]), FR.rel(sw["loo"]["lpd"][ti], lpd),
                    abs(sw["loo"]["var"][ti] - cov[0, 0]) / cov[0, 0])
    print(f"undetermined: the other tips of site {site} against the dense leave-one-out {worst:.2e}")
    assert worst <= TOL


def test_reductions_follow_the_blocks():
    """top_of: ties to the lowest family, nothing eligible -> (-inf, -1); block_total: blocks of 64 in order"""
    lr = np.array([np.nan, 1.0, 3.0, 3.0, np.inf, 2.0])
    ident = np.array([False, True, True, True, True, True])
    npar = np.array([0, 1, 1, 1, 1, 1])
    assert FR.top_of(lr, ident, npar) == (3.0, 2)
    assert FR.top_of(lr[:1], ident[:1], npar[:1]) == (-np.inf, -1)
    x = np.random.default_rng(0).normal(size=200)
    want = (x[:64].sum() + x[64:128].sum()) + x[128:192].sum() + x[192:].sum()
    assert abs(FR.block_total(x) - want) <= 1e-12 * abs(want)

"""The comparators of the lanes-are-sites calls on a fitted univariate batch (tests/post_uni_ref.py: the numpy restatements of
pgbp_moments_sites, pgbp_sample_posterior_sites and pgbp_lg_impute_sites for one site) pinned to independent statements, on the
oracle's calibrated clique tree of every case tests/test_gpu_post_uni.py uses, one site in eight, at 1e-8 relative to
max(1, |block|_inf):
  * moments: mean and covariance of every belief (sepsets included) against the dense posterior of all node states, norm
    against the oracle's integratebelief;
  * draws: against sample_ref.sample_posterior_ref for random z, and z = [0; I] against the dense posterior (mean, A'A);
  * imputations: against impute_ref.dense_impute under the model with the case's shifts and tip noise wrapped in;
  * the generator: simulate_ref's Philox with the counter (entry, draw, site, 1).

It also checks, from the reference alone, the margins the GPU tests rely on (test_margins_of_the_gpu_tests): the smallest pivot
of a conditional J_RR relative to its diagonal entry, the smallest V and the smallest (u' Sigma u + V) / V of a predicted tip,
and that nothing is NaN and no info is set except where a case plants it (the two tips of missing_case's cherry, whose parent
lacks the trait: info -1, not predicted)."""
import numpy as np
import pytest

import fam_uni_ref as FR
import loo_ref as LR
import post_uni_ref as PR
import sample_ref as SR
import simulate_ref as SIM
from oracle import beliefupdates as OBU

TOL = 1e-8
CASES = list(PR.cases())
SHAPES = [PR.shape_case(*sh) for sh in PR.SHAPES]

# asserted floors, a factor 10 below what test_margins_of_the_gpu_tests computes over all the cases (printed by it):
# smallest relative pivot 7.99e-02 (ou/improper), smallest V 1.62e-01 (missing), smallest (u' Sigma u + V) / V 1.49 (missing)
PIVOT_FLOOR, V_FLOOR, TOTAL_FLOOR = 7.99e-3, 1.62e-2, 0.149


def _tri(S):
    m = S.shape[0]
    return np.array([S[a, b] for b in range(m) for a in range(b + 1)])


_DONE = {}


def _pin_site(case, s, impute):
    """one site of a case: (worst errors, smallest relative pivot, smallest V, smallest total / V, the imputation's dict);
    computed once per (case, site)"""
    if (case.name, s) not in _DONE:
        _DONE[case.name, s] = _pin_site_once(case, s, impute)
    return _DONE[case.name, s]


def _pin_site_once(case, s, impute):
    ocgb, fam, data, kw = FR.oracle_site(case, s)
    rec = PR.records_of(ocgb)
    nb = len(rec)
    mean, tri, norm, info = PR.moments_rows(rec, range(nb))
    assert not info.any() and not np.isnan(mean).any() and not np.isnan(norm).any()
    pm, pc = PR.dense_posterior(case, s)
    worst = dict(mean=0.0, cov=0.0, norm=0.0, draw=0.0, law=0.0, impute=0.0)
    am = at = 0
    for j, b in enumerate(ocgb.belief):
        nodes = PR.belief_nodes(b)
        m = len(nodes)
        assert m == len(rec[j][1]) <= 2
        if m:
            worst["mean"] = max(worst["mean"], FR.rel(mean[am: am + m], pm[nodes]))
            worst["cov"] = max(worst["cov"], FR.rel(tri[at: at + m * (m + 1) // 2], _tri(pc[np.ix_(nodes, nodes)])))
        _, want = OBU.integratebelief(b.h, b.J, float(np.ravel(b.g)[0]))
        worst["norm"] = max(worst["norm"], FR.rel(norm[j], want))
        am, at = am + m, at + m * (m + 1) // 2
    # draws
    dims, sepcl, soff, sidx, vn, off = PR.layout(case)
    D = int(off[-1])
    rng = np.random.default_rng(1000 + s)
    z = np.vstack([SR.unit_draws(D), rng.standard_normal((3, D))])
    nc = ocgb.nclusters
    x, xi = PR.sample_rows(rec[:nc], dims, sepcl, soff, sidx, case.spt[2], case.spt[3], z)
    want, wi = SR.sample_posterior_ref([(r[0], r[1]) for r in rec[:nc]], dims, sepcl, soff, sidx, case.spt[2], case.spt[3], z)
    assert xi == 0 and wi == 0 and not np.isnan(x).any()
    worst["draw"] = FR.rel(x, want)
    flat = np.array([n for n, _ in vn], dtype=int)
    A = x[1: 1 + D] - x[0]
    worst["law"] = max(FR.rel(x[0], pm[flat]), FR.rel(A.T @ A, pc[np.ix_(flat, flat)]))
    pivot = PR.pivot_margin(rec[:nc], dims, sepcl, soff, sidx, case.spt[2], case.spt[3])
    # imputations
    K = max(1, int(fam["max_parents"]))
    imp = PR.impute_rows(fam, kw["R"], kw["mu"], LR.oracle_moments(ocgb), kw.get("model", "bm"), kw.get("alpha"), kw.get("theta"),
                         {f * K + k: v for (f, k), v in FR.site_shifts(case, s).items()}, FR.site_noise(case, s))
    assert (len(imp["families"]) > 0) == impute, case.name
    lowV, lowT = np.inf, np.inf
    if impute:
        dn = PR.dense_impute(case, s)
        assert sorted(dn) == sorted(int(r) for r in imp["rows"])
        for ti, r in enumerate(int(r) for r in imp["rows"]):
            if not imp["predicted"][ti]:
                assert imp["info"][ti] == -1 and np.isnan(imp["mean"][ti]) and np.isnan(imp["var"][ti])
                continue
            assert imp["info"][ti] == 0
            worst["impute"] = max(worst["impute"], FR.rel(imp["mean"][ti], dn[r][0]), FR.rel(imp["var"][ti], dn[r][1]))
            lowV, lowT = min(lowV, imp["V"][ti]), min(lowT, imp["total"][ti] / imp["V"][ti])
    return worst, pivot, lowV, lowT, imp


def _pin(case, sites, impute):
    worst, pivot, lowV, lowT = {}, np.inf, np.inf, np.inf
    for s in sites:
        w, pv, v, t, _ = _pin_site(case, s, impute)
        pivot, lowV, lowT = min(pivot, pv), min(lowV, v), min(lowT, t)
        for k, val in w.items():
            worst[k] = max(worst.get(k, 0.0), val)
    print(f"{case.name}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          f"; smallest relative pivot {pivot:.2e}, smallest V {lowV:.2e}, smallest (u'Su + V) / V {lowT:.2e}")
    for k, v in worst.items():
        assert v <= TOL, (case.name, k, v)
    return pivot, lowV, lowT


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c, _, _ in CASES])
def test_restatements_against_the_independent_statements(i):
    case, counts, impute = CASES[i]
    pivot, lowV, lowT = _pin(case, FR.checked_sites(max(counts)), impute)
    assert pivot >= PIVOT_FLOOR and lowV >= V_FLOOR and lowT >= TOTAL_FLOOR


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[c.name for c in SHAPES])
def test_shape_cases(i):
    """the trees at the 64-belief block boundary, the caterpillar and the balanced tree: sites 0 and 56"""
    pivot, _, _ = _pin(SHAPES[i], (0, 56), False)
    assert pivot >= PIVOT_FLOOR


def test_margins_of_the_gpu_tests():
    """Over every case and every checked site, from the reference alone: the smallest pivot of a conditional J_RR relative to
    its diagonal entry, the smallest V of a predicted tip and the smallest (u' Sigma u + V) / V.  Computed here: 7.99e-02,
    1.62e-01 and 1.49; asserted a factor 10 lower (PIVOT_FLOOR, V_FLOOR, TOTAL_FLOOR), far from the 0 at which the device's
    tests `> 0` could fall either way.  The missing case lists four tips, two predicted and the cherry's two with info -1; the
    noisy case lists one, predicted, and its V holds the tip's noise."""
    pivot, lowV, lowT = np.inf, np.inf, np.inf
    for case, counts, impute in CASES:
        for s in FR.checked_sites(max(counts)):
            _, pv, v, t, imp = _pin_site(case, s, impute)
            pivot, lowV, lowT = min(pivot, pv), min(lowV, v), min(lowT, t)
            if case is FR.missing_case():
                assert sorted(imp["info"].tolist()) == [-1, -1, 0, 0]
            if case is PR.noisy_missing_case():
                f = case.gone_family
                assert imp["families"].tolist() == [f] and imp["info"].tolist() == [0]
                assert imp["V"][0] > FR.site_noise(case, s)[f] > 0
    print(f"margins: smallest relative pivot {pivot:.2e}, smallest V {lowV:.2e}, smallest (u'Su + V) / V {lowT:.2e}")
    assert pivot >= PIVOT_FLOOR and lowV >= V_FLOOR and lowT >= TOTAL_FLOOR


def test_restatement_reports_what_is_planted():
    """the all-zero belief, a belief without variables, a belief that is not positive definite (moments); the first cluster in
    preorder whose J_RR is not positive definite (draws); a tip whose variance is not positive (imputation)"""
    rec = [(np.zeros((2, 2)), np.zeros(2), 0.7), (np.zeros((0, 0)), np.zeros(0), -1.5), (np.array([[2.0, 3.0], [3.0, 1.0]]), np.ones(2), 0.0),
           (np.array([[-1.0]]), np.ones(1), 0.0), (np.array([[4.0]]), np.array([2.0]), 0.25)]
    mean, tri, norm, info = PR.moments_rows(rec, range(5))
    assert info.tolist() == [0, 0, 2, 1, 0]
    assert np.all(np.isinf(mean[:2])) and np.all(np.isnan(tri[:3])) and norm[0] == 0.7 and norm[1] == -1.5
    assert np.all(np.isnan(mean[2:5])) and np.all(np.isnan(tri[3:7])) and np.all(np.isnan(norm[2:4]))
    assert mean[5] == 0.5 and tri[7] == 0.25 and abs(norm[4] - (0.25 + 0.5 * (FR.LOG2PI - np.log(4.0) + 1.0))) < 1e-15
    case = FR.bm_case()
    ocgb, fam, data, kw = FR.oracle_site(case, 0)
    dims, sepcl, soff, sidx, vn, off = PR.layout(case)
    nc = ocgb.nclusters
    rec = PR.records_of(ocgb)[:nc]
    order = [int(case.spt[2][0])] + [int(c) for c in case.spt[3]]
    bad = list(rec)
    for c in (order[5], order[2]):   # two failures: the earlier one in preorder is reported
        J = rec[c][0].copy()
        J[:] = -1.0
        bad[c] = (J, rec[c][1], rec[c][2])
    z = np.zeros((2, int(off[-1])))
    x, xi = PR.sample_rows(bad, dims, sepcl, soff, sidx, case.spt[2], case.spt[3], z)
    want, wi = SR.sample_posterior_ref([(r[0], r[1]) for r in bad], dims, sepcl, soff, sidx, case.spt[2], case.spt[3], z)
    assert xi == wi == order[2] + 1 and np.isnan(x).all()
    mcase = FR.missing_case()
    ocgb, fam, data, kw = FR.oracle_site(mcase, 0)
    imp = PR.impute_rows(fam, -np.asarray(kw["R"]), kw["mu"], LR.oracle_moments(ocgb))
    pred = imp["predicted"]
    assert np.all(imp["info"][pred] == 1) and np.all(imp["info"][~pred] == -1) and np.isnan(imp["mean"]).all()


def test_generator_is_simulate_ref_s_philox_with_the_new_counter():
    """the same Philox and 53-bit uniforms as simulate_ref.normals: with the last counter word 0 and (entry, draw) in the
    places of (family, trait pair) the cosine is simulate_ref's even trait; with the word 1 every value differs from it, and
    a value depends on (entry, draw, site) alone"""
    seed, sites = PR.SEED, np.array([0, 3, 70, 8191])
    z = PR.normals(seed, sites, 5, 3)
    assert z.shape == (3, 5, 4) and np.isfinite(z).all()
    # one value by hand
    r = SIM.philox4x32_10(np.array([2, 1, 70, 1], np.uint64), np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
    u1, u2 = SIM.uniform53(r[0], r[1]), SIM.uniform53(r[2], r[3])
    assert z[1, 2, 2] == np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    # the stream of pgbp_lg_simulate under the same seed (word 0; trait pair 0 of a 2-trait table is its cosine) is another
    sim = SIM.normals(seed, sites, 5, 2)[:, :, 0]   # [site, family]: counter (family, 0, site, 0)
    assert not np.any(np.isclose(z[0].T, sim))
    # a value does not depend on what else is asked for
    assert np.array_equal(PR.normals(seed, sites[2:3], 5, 3)[:, :, 0], z[:, :, 2])
    assert np.array_equal(PR.normals(seed, sites, 4, 2), z[:2, :4])
    big = PR.normals(seed, np.arange(512), 16, 4).reshape(-1)
    m, v = SIM.moment_band(big)
    assert m < 5 and v < 5, (m, v)

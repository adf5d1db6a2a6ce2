"""Per-site missing tips of a univariate batch, host side: (1) the numpy restatement of tests/site_missing_ref.py -- the
family sweeps and the imputation with the masked tips of a site skipped, over the dense posterior moments of the clusters of
the COMPLETE graph -- is pinned to the dense statements with None at the masked tips of that site (oracle.densemvn.loglik
through posterior_node_moments, fam_uni_ref.dense, post_uni_ref.dense_impute); (2) the margins the GPU tests rely on, with the
seeds of the cases chosen so that the reference itself stays inside them; (3) the host packing and checks of the setter
(csrc/pgbp_sitemiss_host.cpp) run under the address and undefined-behaviour sanitizers as a stand-alone program
(tests/site_missing_check.cpp).  Nothing here needs a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fam_uni_ref as FR
import post_uni_ref as PU
import site_missing_ref as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phylogaussianbeliefprop.jl_amd", "csrc")
TOL = 1e-8
CASES = [(name, make, n) for name, make, counts in SM.sweep_cases() for n in counts if n <= 65]


@pytest.fixture(autouse=True)
def _the_interface_exists():
    from pgbp_amd import _lib as L
    assert "pgbp_lg_set_site_missing" in L.SYMBOLS and "pgbp_lg_site_missing_count" in L.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "pgbp.h")).read()
    assert "pgbp_lg_set_site_missing(pgbp_engine* e, const uint8_t* missing)" in hdr and "PGBP_INFO_NOT_OBSERVED" in hdr


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{c[0]}-{c[2]}" for c in CASES])
def test_restatement_against_the_dense_statements_and_margins(i):
    """At the checked sites: scan, edge derivatives and leave-one-out of the restatement against fam_uni_ref.dense, the
    imputation against post_uni_ref.dense_impute, every block at 1e-8 of max(1, |block|).  Margins at those sites: at least
    two observed tips, identified pivots H / j at least 1e-4 (min_info = 1e-8) and the planted unidentified one below 1e-12,
    D / V of every leave-one-out tip at least 1e-6 (the floor is 2^-40 = 9.1e-13), the smallest relative pivot of a
    conditional J_RR at least 1e-6 (ten orders above 2^-52: a clade without data leaves J_RR at the edge's own j)."""
    name, make, n = CASES[i]
    case = make(n)
    rows_all, _ = SM.tip_rows(case)
    assert np.all((~case.mask[:, rows_all]).sum(axis=1) >= 2) and not case.mask[1].any()
    worst, low_H, low_D, dead_H, low_piv = {}, np.inf, np.inf, 0.0, np.inf
    dims, sepcl, soff, sidx, _, _ = PU.layout(case)
    pl = case.planted_mask
    for s in SM.checked_sites(case):
        ref, fam_s = SM.reference_site(case, s)
        sw = ref["raw"]
        rows = np.asarray(case.fam["data_row"])[sw["loo"]["families"]]
        w = FR.against_dense(sw, SM.dense_site(case, s), fam_s, rows)
        di = PU.dense_impute(case, s)
        im = ref["impute"]
        for k, r in enumerate(im["rows"]):
            if case.mask[s, r]:
                assert im["info"][k] == 0
                w["impute"] = max(w.get("impute", 0.0), FR.rel(im["mean"][k], di[int(r)][0]), FR.rel(im["var"][k], di[int(r)][1]))
            else:
                assert im["info"][k] == SM.NOT_OBSERVED and np.isnan(im["mean"][k])
        assert sorted(int(r) for r in np.flatnonzero(case.mask[s])) == sorted(di)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        relH = sw["scan"]["relH"]
        edge = (np.asarray(fam_s["n_parents"]) >= 1) & (np.asarray(fam_s["child_mask"]) != 0)
        dead = np.zeros(len(relH), bool)
        if pl["cherry"] and s == pl["cherry"][0]:
            dead[pl["cherry"][1]] = True
            assert not sw["scan"]["identified"][pl["cherry"][1]] and sw["scan"]["lr"][pl["cherry"][1]] == 0.0
            dead_H = max(dead_H, abs(float(relH[pl["cherry"][1]])))
        elif pl["cherry"]:
            assert sw["scan"]["identified"][pl["cherry"][1]] or s not in (1, 3)
        ident = edge & sw["scan"]["identified"]
        if ident.any():
            low_H = min(low_H, float(np.min(relH[ident])))
        unid = edge & ~sw["scan"]["identified"]
        if unid.any():
            dead_H = max(dead_H, float(np.max(np.abs(relH[unid]))))
        # the smallest relative pivot of a conditional J_RR of the preorder sweep, on the beliefs a calibrated clique tree of
        # the COMPLETE graph holds under the mask: (J, h) = (S^-1, S^-1 m) of the dense posterior moments of each cluster
        mom, rec = SM.dense_moments(case, s), []
        for c in range(case.ocgb0.nclusters):
            m, S = mom(c)
            J = np.linalg.inv(S) if len(m) else np.zeros((0, 0))
            rec.append((J, J @ m, 0.0))
        low_piv = min(low_piv, PU.pivot_margin(rec, dims, sepcl, soff, sidx, case.spt[2], case.spt[3]))
        live = ~ref["loo"]["masked"]
        assert np.all(ref["loo"]["info"][live] == 0)
        low_D = min(low_D, float(np.min(ref["loo"]["relD"][live])))
    print(f"{name}/{n}: restatement against the dense statements: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) +
          f"; smallest identified H / j {low_H:.2e}, largest unidentified |H / j| {dead_H:.2e}, smallest D / V {low_D:.2e}, smallest relative pivot of a conditional J_RR {low_piv:.2e}")
    assert max(worst.values()) <= TOL, worst
    assert low_H >= 1e-4 and dead_H <= 1e-12 and low_D >= 1e-6 and low_piv >= 1e-6


def test_loglik_and_gradient_closed_form_bm():
    """gls_bm against densemvn.loglik on the observed tips, its gradient against central differences of it, and the optimum
    as a stationary point"""
    case = SM.bm(64)
    C = SM.bm_cov(case)
    for s in (0, 2, 9):
        model, tbl = case.sites[s]
        y = np.array([0.0 if v is None else v for v in tbl[0]])
        obs = np.flatnonzero(~case.mask[s])
        kw = SM.site_kw(case, s)
        s2, mu = float(np.ravel(kw["R"])[0]), float(np.ravel(kw["mu"])[0])
        ll, g2, gm = SM.gls_bm(C, y, obs, s2, mu)
        assert abs(ll - SM.dense_loglik(case, s)) <= 1e-10 * max(1.0, abs(ll))
        h = 1e-5
        f2 = (SM.gls_bm(C, y, obs, s2 + h, mu)[0] - SM.gls_bm(C, y, obs, s2 - h, mu)[0]) / (2 * h)
        fm = (SM.gls_bm(C, y, obs, s2, mu + h)[0] - SM.gls_bm(C, y, obs, s2, mu - h)[0]) / (2 * h)
        assert abs(f2 - g2) <= 1e-6 * max(1.0, abs(g2)) and abs(fm - gm) <= 1e-6 * max(1.0, abs(gm))
        mh, sh, lh = SM.gls_bm(C, y, obs)
        _, a, b = SM.gls_bm(C, y, obs, sh, mh)
        assert abs(a) <= 1e-9 and abs(b) <= 1e-9 and lh >= ll


def test_host_packing_and_checks_under_the_sanitizers(tmp_path):
    """tests/site_missing_check.cpp over csrc/pgbp_sitemiss_host.cpp, built with -fsanitize=address,undefined, as a process of
    its own."""
    if shutil.which("g++") is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "site_missing_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "site_missing_check.cpp"),
                           os.path.join(CSRC, "pgbp_sitemiss_host.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    for what in ("words of 65 sites", "lanes 0, 63 and site 64", "round trip", "families and clusters", "row without a tip",
                 "statically missing tip", "site with nothing observed", "output untouched", "shared row: both families listed",
                 "shared row: nothing observed", "empty mask"):
        assert "ok " + what in lines, out.stdout
    assert lines[-1] == "site missing ok", out.stdout

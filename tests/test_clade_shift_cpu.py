"""The comparators of the per-site clade shifts (tests/clade_shift_ref.py) pinned to each other on the cases
tests/test_gpu_clade_shifts.py uses, the margins those tests rely on from the reference alone, and the host plan of the setter
under the sanitizers.

  * statement 1 against statement 2: the dense log-likelihood of the model with the equivalent explicit shifts is quadratic in
    the deltas with the score and information of the dense GLS design -- ll(d + x) - ll(d) = g'x - x'Hx / 2 -- and the
    restated scan of the painted model returns g_v / H_vv at every slot; both at 1e-8 relative to max(1, |block|);
  * the smallest relative pivot of a joint H on the identified cases;
  * the planted unidentified slot (its whole clade masked at that site) against min_info;
  * at every step of every greedy path the gap between the largest and the second-largest lr, relative to the largest."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import clade_shift_ref as CS
import optimum_scan_ref as OS

TOL = 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phylogaussianbeliefprop.jl_amd", "csrc")


@pytest.mark.parametrize("key,n,m", CS.PARITY, ids=[f"{k}-{n}-{m}" for k, n, m in CS.PARITY])
def test_dense_loglik_is_the_quadratic_of_the_dense_design(key, n, m):
    c = OS.case(key)
    fam, delta = CS.draw_setting(c, n, m)
    rng = np.random.default_rng(11)
    worst_q, worst_s, piv, sing = 0.0, 0.0, np.inf, 0.0
    for s in CS.checked_sites(c, n):
        used = fam[:, s] >= 0
        if not used.any():
            assert CS.loglik(c, s, fam, delta) == OS.loglik_with(c, s)
            continue
        g, H = CS.dense_score(c, s, fam, delta)
        x = rng.normal(size=int(used.sum()))
        moved = delta.copy()
        moved[used, s] += x
        ll0, ll1 = CS.loglik(c, s, fam, delta), CS.loglik(c, s, fam, moved)
        worst_q = max(worst_q, abs((ll1 - ll0) - (g @ x - 0.5 * x @ H @ x)) / max(1.0, abs(ll0)))
        ref = CS.reference_scan(c, s, fam, delta)
        for i, v in enumerate(fam[used, s]):
            if ref["identified"][v]:
                worst_s = max(worst_s, abs(ref["delta"][v] * ref["H"][v] - g[i]) / max(1.0, abs(g[i])),
                              abs(ref["H"][v] - H[i, i]) / max(1.0, abs(H[i, i])))
            else:
                assert abs(H[i, i]) <= 1e-10 and abs(g[i]) <= 1e-10
        if np.all(np.diag(H) > 1e-10) and getattr(c, "mask", None) is None:
            fit = CS.dense_fit(c, s, fam, delta)
            if fit["singular"]:   # (a cherry's parent and both its tips: three columns over two tips)
                sing = max(sing, fit["pivot"])
            else:
                piv = min(piv, fit["pivot"])
    print(f"{c.name}/{n}/{m}: dense loglik against the quadratic of the design {worst_q:.2e}; restated scan at the slots against the "
          f"design {worst_s:.2e}; smallest relative pivot of a joint H {piv:.2e} (largest of the slot sets that are not jointly identified {sing:.2e})")
    assert worst_q <= TOL and worst_s <= TOL
    assert piv >= 1e-3 and sing <= 1e-12     # measured over the cases: 5.2e-2 (caterpillar) the smallest, exactly 0 the singular ones (balanced)


def test_planted_unidentified_slot_against_min_info():
    """a cherry wholly masked at one site: a slot on it has H / Kt <= min_info / 1e4 there, >= 1e4 min_info next to it"""
    c = OS.case("mask")
    site, f, _ = c.planted_mask["cherry"]
    for s, ident in ((site, False), (site - 1, True), (site + 1, True)):
        ref = OS.reference_site(c, s)
        assert bool(ref["identified"][f]) == ident
        assert (ref["relH"][f] >= 1e4 * CS.MIN_INFO) if ident else (abs(ref["relH"][f]) <= CS.MIN_INFO / 1e4)


@pytest.mark.parametrize("key", ["fixed", "planted"])
def test_greedy_paths_have_a_clear_argmax(key):
    """every step of every greedy path the GPU test follows: (largest lr - second largest) / largest, which must be far above
    the 1e-8 at which the device's lr is compared, or the argmax could flip"""
    c = CS.select_case(key)
    gap, steps = np.inf, 0
    for s in range(CS.SELECT_SITES):
        path = CS.greedy(key, s)
        gap, steps = min(gap, path["gap"]), steps + path["n_shifts"]
        assert np.all(np.diff(path["loglik"]) > 0)
        if key == "planted":
            assert sorted(path["family"][:2].tolist()) == sorted(c.planted[0][:, s].tolist()), s
    print(f"{c.name}: {steps} steps over {CS.SELECT_SITES} sites, smallest relative gap of the two largest lr {gap:.2e}")
    assert steps >= CS.SELECT_SITES
    assert gap >= 1e-4     # measured: 3.6e-4 ("fixed"), 5.9e-3 ("planted")


def test_host_plan_under_the_sanitizers(tmp_path):
    """tests/clade_shift_check.cpp over csrc/pgbp_cladeshift_host.cpp, built with -fsanitize=address,undefined, as a process of
    its own."""
    if shutil.which("g++") is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "clade_shift_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "clade_shift_check.cpp"),
                           os.path.join(CSRC, "pgbp_cladeshift_host.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    for what in ("fixed root ranks", "caterpillar membership", "levels ranks", "clusters: the union of the intervals", "nested clusters",
                 "duplicate names site and family", "root-prior family", "delta not finite", "plan cleared", "empty table"):
        assert "ok " + what in lines, out.stdout
    assert lines[-1] == "clade shift ok", out.stdout

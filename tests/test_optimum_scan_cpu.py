"""The comparators of the optimum-shift scan (tests/optimum_scan_ref.py) pinned to each other and to the dense oracle, on every
case tests/test_gpu_optimum_scan.py uses; the margins those tests rely on, from the reference alone; add_optimum_shift; and
the host plan of the scan under the sanitizers.

  * the numpy restatement of the recursion against the dense GLS statement (g, H, lr) at 1e-8 relative to max(1, |block|);
  * lr against 2 (ll(delta_hat) - ll(0)) of oracle.densemvn.loglik with the clade painted;
  * a restated scan at the painted delta_hat returns |delta| <= 1e-8 max(1, |delta_hat|) at that edge;
  * every (edge, site) classified by whether its clade observes a tip at that site: the observed ones are the identified ones
    and have H / Kt >= 1e4 min_info, the others H / Kt <= min_info / 1e4."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import optimum_scan_ref as OS

TOL = 1e-8
MIN_INFO = OS.MIN_INFO
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phylogaussianbeliefprop.jl_amd", "csrc")


def _classified(tag, c, s, ref, dn):
    """the margins of site s; returns (smallest observed H / Kt, largest unobserved |H / Kt|)"""
    real = np.asarray(c.fam["n_parents"]) >= 1
    seen = dn["clade_observed"]
    assert np.array_equal(ref["identified"][real], seen[real]), (tag, s)
    assert not ref["identified"][~real].any()
    hi = ref["relH"][real & seen]
    lo = ref["relH"][real & ~seen]
    lo = lo[np.isfinite(lo)]       # (a tip masked at the site is skipped: no H)
    assert np.all(hi >= 1e4 * MIN_INFO), (tag, s, float(hi.min()))
    assert np.all(np.abs(lo) <= MIN_INFO / 1e4), (tag, s, lo)
    return float(hi.min()), (float(np.abs(lo).max()) if len(lo) else 0.0)


@pytest.mark.parametrize("key,counts", OS.CASES, ids=[k for k, _ in OS.CASES])
def test_restatement_against_dense_gls_and_margins(key, counts):
    """every site the GPU tests run: the classification and its margins; one site in eight (the planted sites of a mask
    always): g, H and lr against the dense GLS statement"""
    c = OS.case(key)
    n = max(counts)
    worst, low, high = 0.0, np.inf, 0.0
    checked = set(OS.checked_sites(c, n))
    for s in range(n):
        ref = OS.reference_site(c, s)
        full = s in checked
        dn = OS.gls(c, s) if full else OS.gls(c, s, families=())
        if not full:   # the classification needs no solve: which clades observe a tip
            obs, _ = OS._observed(c, s)
            pos = {id(nd): i for i, nd in enumerate(c.net.vec_node)}
            for f in range(len(c.fam["cluster"])):
                if int(c.fam["n_parents"][f]) >= 1:
                    below = {pos[id(e.child)] for e in OS.clade_edges(c, f)}
                    dn["clade_observed"][f] = any(i in below for i in obs)
        a, b = _classified(c.name, c, s, ref, dn)
        low, high = min(low, a), max(high, b)
        if full:
            worst = max(worst, OS.against_gls(ref, dn))
    print(f"{c.name}: restatement against dense GLS {worst:.2e} over {len(checked)} sites; smallest observed H/Kt {low:.2e}, "
          f"largest unobserved |H/Kt| {high:.2e} over {n} sites")
    assert worst <= TOL
    if getattr(c, "mask", None) is not None and c.planted_mask["cherry"] is not None:
        site, f, rows = c.planted_mask["cherry"]
        assert not OS.reference_site(c, site)["identified"][f]
        assert OS.reference_site(c, site - 1)["identified"][f] and OS.reference_site(c, site + 1)["identified"][f]


@pytest.mark.parametrize("key", ["main", "random", "improper", "two tips", "families65", "shifts+noise", "mask", "optima", "everything"])
def test_lr_is_twice_the_gain_of_the_dense_loglik_and_the_scan_vanishes_there(key):
    """a few edges of a few sites: paint the clade by delta_hat in the dense oracle -- 2 (ll(delta_hat) - ll(0)) is lr, and the
    restated scan of the painted model returns delta = 0 at that edge"""
    c = OS.case(key)
    n = min(len(c.sites), 65)
    rng = np.random.default_rng(5)
    w_lr, w_d = 0.0, 0.0
    for s in sorted({0, 2, n - 1}):
        ref = OS.reference_site(c, s)
        ident = np.flatnonzero(ref["identified"])
        for f in sorted(set(int(x) for x in rng.choice(ident, size=min(3, len(ident)), replace=False)) | {int(ident[np.argmax(ref["lr"][ident])])}):
            ll0, ll1 = OS.loglik_with(c, s), OS.loglik_with(c, s, f, ref["delta"][f])
            w_lr = max(w_lr, abs(2 * (ll1 - ll0) - ref["lr"][f]) / max(1.0, abs(ll0)))
            # the painted model as a case of its own: clade(f) refined into regimes of its own, values + delta_hat
            reg = dict(c.optima[0]) if getattr(c, "optima", None) is not None else {}
            vals = [list(v) for v in c.optima[1]] if reg else [[] for _ in c.sites]
            new_of = {}
            for e in OS.clade_edges(c, f):
                r = reg.get(e.number, 0)
                if r not in new_of:
                    for t, v in enumerate(vals):
                        th = c.sites[t][0].theta
                        v.append((v[r - 1] if r > 0 else th) + (ref["delta"][f] if t == s else 0.0))
                    new_of[r] = len(vals[s])
                reg[e.number] = new_of[r]
            d = types.SimpleNamespace(**c.__dict__)
            d.optima = (reg, np.array(vals))
            again = OS.reference_site(d, s)
            assert again["identified"][f]
            w_d = max(w_d, abs(again["delta"][f]) / max(1.0, abs(ref["delta"][f])))
    print(f"{c.name}: lr against 2 (ll(delta_hat) - ll(0)) {w_lr:.2e} of max(1, |ll|); |delta| after painting {w_d:.2e} of max(1, |delta_hat|)")
    assert w_lr <= TOL and w_d <= TOL


def test_case_shapes():
    """what the GPU tests' shapes are meant to cover is there: heights, a trifurcation, the family counts, the planted mask"""
    h = lambda key: int(OS.heights(OS.case(key).fam).max())
    assert h("caterpillar") == 10 and h("balanced") == 3 and h("two tips") == 0
    for n in (63, 64, 65, 130):
        assert len(OS.case(f"families{n}").fam["cluster"]) == n
    assert max(len(k) for k in OS.children_of(OS.case("families65").fam)) >= 3
    c = OS.case("mask")
    assert c.planted_mask["cherry"][0] == 2 and not c.mask[1].any() and c.mask[0].any() and c.mask[63].any() and c.mask[64].any()
    assert 0.2 <= c.mask[:, OS.SM.tip_rows(c)[0]].mean() <= 0.4
    c = OS.case("everything")
    assert c.optima is not None and c.shifts is not None and c.noise is not None and c.mask is not None
    assert len(set(OS.device_regime(c).ravel())) == 3


def test_add_optimum_shift_on_nested_and_disjoint_clades():
    import pgbp_amd
    # ((3,4)1,(5,6)2)0 with the root's own edge: families 0 .. 6, parent_family of a fixed root
    pf = np.array([-1, 0, 0, 1, 1, 2, 2], np.int32)
    reg0 = np.zeros((7, 1), np.int32)
    r1, o1 = pgbp_amd.add_optimum_shift(reg0, pf, 1)
    assert r1.ravel().tolist() == [0, 1, 0, 1, 1, 0, 0] and o1.tolist() == [0] and r1.shape == (7, 1) and r1.dtype == np.int32
    assert not reg0.any()                                       # (pure: the input is untouched)
    r2, o2 = pgbp_amd.add_optimum_shift(r1, pf, 2)              # a disjoint clade: one more regime from theta
    assert r2.ravel().tolist() == [0, 1, 2, 1, 1, 2, 2] and o2.tolist() == [1, 0]
    r3, o3 = pgbp_amd.add_optimum_shift(r2, pf, 3)              # nested inside regime 1: split
    assert r3.ravel().tolist() == [0, 1, 2, 3, 1, 2, 2] and o3.tolist() == [1, 2, 1]
    r4, o4 = pgbp_amd.add_optimum_shift(r3, pf, 0)              # the whole tree: every regime it meets is split, in family order
    assert r4.ravel().tolist() == [4, 5, 6, 7, 5, 6, 6] and o4.tolist() == [1, 2, 3, 0, 1, 2, 3]
    r5, o5 = pgbp_amd.add_optimum_shift(r1.ravel(), pf, 4)      # a flat map; a tip
    assert r5.tolist() == [0, 1, 0, 1, 2, 0, 0] and o5.tolist() == [1, 1]
    with pytest.raises(ValueError):
        pgbp_amd.add_optimum_shift(reg0, pf, 7)
    with pytest.raises(ValueError):
        pgbp_amd.add_optimum_shift(reg0, pf[:5], 1)
    # a random root: the root-prior family 0 is the parent of the root's children and has no edge of its own to paint
    pf = np.array([0, 0, 0, 1, 1], np.int32)    # (entry 0 is not read: n_parents[0] == 0; here it points at itself)
    r, o = pgbp_amd.add_optimum_shift(np.zeros(5, np.int32), pf, 1)
    assert r.tolist() == [0, 1, 0, 1, 1] and o.tolist() == [0]


def test_host_plan_under_the_sanitizers(tmp_path):
    """tests/optimum_scan_check.cpp over csrc/pgbp_optscan_host.cpp, built with -fsanitize=address,undefined, as a process of
    its own."""
    if shutil.which("g++") is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "optimum_scan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "optimum_scan_check.cpp"),
                           os.path.join(CSRC, "pgbp_optscan_host.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    for what in ("fixed root heights", "caterpillar heights", "trifurcation", "hybrid named", "plan cleared", "empty table",
                 "scratch, top only"):
        assert "ok " + what in lines, out.stdout
    assert lines[-1] == "optimum scan ok", out.stdout

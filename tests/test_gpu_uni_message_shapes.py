"""Every THREAD-PER-SITE message kernel (csrc/pgbp_kernels.hip: bp_level_uni<SM>, bp_level_uni1<SM>, bp_chunk_uni1<SM>; every
belief at most 2 variables, at least 8 sites, lanes = sites) at every shape it takes -- every (mf, s, mt) <= 2 with every keep
and up map, three sepset kinds, both directions (tests/message_ref.py: uni_shape_cases) -- with 8 sites (plain layout), 64
(the smallest site-minor batch) and 65 (a padded site-minor row), EVERY site against the numpy.longdouble restatement of one
message on that site's own numbers.  tests/test_gpu_message_shapes.py pins the wave-per-task kernels and reaches none of
these: pgbp_propagate always takes the generic kernel, so here a message is sent by a postorder traversal
(tests/run_uni_message_shapes.py, which also says how the kernel that ran is derived from `dims`, pgbp_layout and the
planner's report).

Engines: "pair" sender -(s)- receiver; "chain2" sender -(s)- receiver -(2)- extra (one more link when the receiver has fewer
than 2 variables): the largest sepset is 2, which sends every shape through bp_level_uni, and the message out of the
receiver is its s = 2, ni = 0 copy; "chain1": two levels with sepsets <= 1, the loop mode bp_chunk_uni1.  Each case runs
from beliefs that hold a non-zero sepset (residual = new - old), again straight after init_beliefs_reset_fromfactors_(),
and once with update_residualkldiv=True (per-level launches in the plain layout, kldiv and its flag against the oracle's
residual_kldiv!).  The per-level kernels of the two-level chains are reached a second way in a child process per
PGBP_TUNING value that switches chunks off.

Tolerances: the project's gate 1e-8 * max(1, |.|_inf) per record, and the scheme of tests/test_gpu_message_shapes.py: the
device's error to the longdouble reference is at most MARGIN x the float64 C engine's error on the same inputs, floored at
max(1, mf) * eps * max(1, |.|_inf).  MARGIN = 4 x (the worst device / C-engine ratio over this sweep on an MI355X, rounded up
to a power of two): MEASURED_RATIO and MARGIN below.  Measured (MI355X, the whole sweep): worst ratio 3.449 -- the same
figure on bp_level_uni<false>, bp_level_uni<true>, bp_level_uni1<false>, bp_level_uni1<true> and bp_chunk_uni1<true> (the
bodies state the same expressions in the same order), 1.74 on bp_chunk_uni1<false> (8 sites only), integratebelief! 1.36
(1 variable) and 1.11 (2) -- so MARGIN = 4 x 4 = 16; worst error 1.53e-15 of max(1, |.|_inf) on every message kernel
(8.4e-16 on bp_chunk_uni1<false>), 4.9e-16 on integratebelief!.  The closed forms divide by the pivot three times where
the C engine takes one square root: a few units in the last place on records of which the C engine gets most exactly.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import message_ref as M
import run_uni_message_shapes as U

pytestmark = pytest.mark.gpu

MEASURED_RATIO = 3.449   # worst (device error) / max(C-engine error, max(1, mf) eps scale) over the sweep on an MI355X
MARGIN = 16.0            # 3.449 -> next power of two 4 -> x 4


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _kinds_of(case):
    return [k for k in M.UNI_KINDS if not (k == "chain1" and case.s > 1)]


def _expected_kernel_family(ub):
    """what the issue's table says must run, independent of run_uni_message_shapes.kernel_instance's derivation"""
    if ub.kind == "chain2" or ub.case.s == 2:
        return "bp_level_uni<"
    return "bp_chunk_uni1<" if ub.kind == "chain1" else "bp_level_uni1<"


@pytest.mark.parametrize("sep_kind", M.SEP_KINDS)
@pytest.mark.parametrize("n_sites", M.UNI_SITES)
@pytest.mark.parametrize("kind", M.UNI_KINDS)
def test_every_tiny_shape_at_every_site(P, kind, n_sites, sep_kind):
    """(a) uni_shape_cases(): from a non-zero sepset, after a reset, and with residual_kldiv! between the levels."""
    seen = set()
    for case in M.uni_shape_cases():
        if case.sep_kind != sep_kind or kind not in _kinds_of(case):
            continue
        ub = M.build_uni(case, kind, n_sites)
        tag = f"{case.name}/{kind}/{n_sites}"
        cgb = U.engine(P, ub)
        before = U.state_of(cgb)
        assert np.array_equal(before.packed, ub.packed)
        after, results, kernel = U.postorder(P, cgb, ub)
        assert kernel.startswith(_expected_kernel_family(ub)) and kernel.endswith("true>" if n_sites >= 64 else "false>"), (tag, kernel)
        U.check_pass(ub, before, after, results, kernel, MARGIN, tag)
        seen.add(kernel)
        if case.sep_kind != "zero" and case.s:     # the old sepset was subtracted: the residual is not the message itself
            (dJ, dh), _ = M.residual_of(ub, ub.msgs[0], after.res[0])
            sep = M.uni_records(ub, after.packed[0])[ub.nc]
            assert not np.array_equal(dh, sep[1]) and not np.array_equal(dJ, sep[0]), tag
        if case.sep_kind == "below" and case.mt and kind == "pair":
            _integrate_receiver(P, cgb, ub, after, tag)
        # straight after init_beliefs_reset_fromfactors_(): clusters = the factors, every sepset the constant 1
        cgb.init_beliefs_reset_fromfactors_(sync=False)
        before = U.state_of(cgb)
        off = M.record_offsets(ub.dims)
        assert np.array_equal(before.packed[:, :off[ub.nc]], ub.packed[:, :off[ub.nc]]) and not before.packed[:, off[ub.nc]:].any()
        after, results, k2 = U.postorder(P, cgb, ub)
        assert k2 == kernel
        U.check_pass(ub, before, after, results, kernel, MARGIN, tag + "/reset")
        # update_residualkldiv=True: per-level launches, plain layout, kldiv of every message
        cgb._packed[...] = ub.packed
        cgb.push()
        before = U.state_of(cgb)
        assert np.array_equal(before.packed, ub.packed)
        after, results, k3 = U.postorder(P, cgb, ub, kl=True)
        assert k3.endswith("false>") and not k3.startswith("bp_chunk"), (tag, k3)
        assert k3.startswith("bp_level_uni<" if kernel.startswith("bp_level_uni<") else "bp_level_uni1<"), (tag, k3)
        U.check_pass(ub, before, after, results, k3, MARGIN, tag + "/kl", kl=True)
        seen.add(k3)
    U.report()
    print("kernel instances of this test:", sorted(seen))
    assert seen


def _integrate_receiver(P, cgb, ub, after, tag):
    """integratebelief_ of the 1- or 2-variable receiver, all sites, against integrate_ld on the device's own record."""
    j = ub.msgs[0].i_to
    mu, norm, info = cgb.integratebelief_(j, all_sites=True)
    m = int(ub.dims[j])
    st = U.STATS.setdefault(f"integrate m={m}", {"abs": 0.0, "ratio": 0.0, "n": 0})
    for site in range(ub.n_sites):
        rec = M.uni_records(ub, after.packed[site])[j]
        rmu, rnorm, rinfo = M.integrate_ld(*rec)
        assert rinfo == 0 == info[site], (tag, site)
        ce_mu, ce_norm = _c_integrate(ub, after.packed[site], j)
        for got, cgot, want in (((mu[site],), (ce_mu,), (rmu,)), (([norm[site]],), ([ce_norm],), ([rnorm],))):
            err, scale = M.record_error(got, want)
            floor = max(M.record_error(cgot, want)[0], m * U.EPS * scale)
            st["abs"], st["ratio"], st["n"] = max(st["abs"], err / scale), max(st["ratio"], err / floor), st["n"] + 1
            assert err <= U.RTOL * scale and err <= MARGIN * floor, (tag, site, err / scale, err / floor)


def _c_integrate(ub, packed_site, j):
    from oracle import cengine
    return cengine.Engine(ub.dims, ub.sepcl, ub.scope_off, ub.scope_idx, packed_site).integrate(j)


@pytest.mark.parametrize("n_sites", M.UNI_SITES)
@pytest.mark.parametrize("kind", M.UNI_KINDS)
def test_all_zero_exit_and_its_threshold(P, kind, n_sites):
    """(b) J_I = c I, h_I = 0, J_KI = 0 in site 0 and in the event sites (not lane 0; site 64 of 65): c = eps is the all-zero
    exit -- the message is (J_K, h_K, g) exactly --, c = 2 eps is not: the same J and h, g shifted."""
    for case in M.uni_exit2_cases():
        if kind not in _kinds_of(case):
            continue
        ub = M.build_uni(case, kind, n_sites)
        tag = f"{case.name}/{kind}/{n_sites}"
        cgb = U.engine(P, ub)
        before = U.state_of(cgb)
        after, results, kernel = U.postorder(P, cgb, ub)
        assert kernel.startswith(_expected_kernel_family(ub)), (tag, kernel)
        U.check_pass(ub, before, after, results, kernel, MARGIN, tag)
        c = case.fail[1]
        m = ub.msgs[0]
        ni = case.mf - case.s
        for site in (0,) + M.UNI_EVENT_SITES[n_sites]:
            ref = M.uni_reference(ub, ub.packed[site])[0]
            assert ref[4] == (2 if c <= M.EPS else 0), (tag, site)
            J, h, g = M.uni_records(ub, ub.packed[site])[m.i_from]
            sJ, sh, sg = M.uni_records(ub, after.packed[site])[ub.nc]
            assert np.array_equal(sJ, J[np.ix_(m.keep, m.keep)]) and np.array_equal(sh, h[m.keep]), (tag, site)
            if c <= M.EPS:
                assert sg == g, (tag, site)
            else:
                shift = (ni * np.log(2 * np.pi) - ni * np.log(c)) / 2
                assert abs(sg - (g + shift)) <= U.RTOL * max(1.0, abs(g + shift)), (tag, site)
    U.report()


@pytest.mark.parametrize("n_sites", M.UNI_SITES)
@pytest.mark.parametrize("kind", M.UNI_KINDS)
def test_info_at_pivot_1_and_2_of_one_site(P, kind, n_sites):
    """(c) a failure placed at pivot k of the event sites: fail_info == k and succ == 0 there, succ == 1 elsewhere; that
    site's sepset, receiver, residual and flag bit for bit as before (a pass on good matrices filled them first); every
    other site updated correctly; on the chains the message out of the receiver is not sent in that site."""
    from pgbp_amd import _lib as L
    for case in M.uni_failure_cases():
        if kind not in _kinds_of(case):
            continue
        ub = M.build_uni(case, kind, n_sites)
        tag = f"{case.name}/{kind}/{n_sites}"
        assert ub.fail_sites == M.UNI_EVENT_SITES[n_sites]
        off = M.record_offsets(ub.dims)
        m = ub.msgs[0]
        good = ub.packed.copy()
        for site in ub.fail_sites:     # first every site good: the sepsets and residuals get real values
            good[site] = ub.packed[site - 1]
        cgb = U.engine(P, ub, good)
        _, results, kernel = U.postorder(P, cgb, ub)
        assert all(r[0] == 1 for r in results), tag
        for site in ub.fail_sites:
            rec = np.ascontiguousarray(ub.packed[site][off[m.i_from]:off[m.i_from + 1]])
            assert cgb._lib.pgbp_set_belief(cgb._eng, site, int(m.i_from), L.f64p(rec)) == 0
        before = U.state_of(cgb)
        for site in ub.fail_sites:
            assert before.res[site].any() or int(ub.dims[ub.nc:].max()) == 0, tag
        after, results, k2 = U.postorder(P, cgb, ub)
        assert k2 == kernel and kernel.startswith(_expected_kernel_family(ub)), (tag, kernel)
        print(f"{tag} {kernel}: fail_info {[results[s][1] for s in ub.fail_sites]} at sites {ub.fail_sites}")
        for site in ub.fail_sites:
            assert results[site][:2] == (0, case.fail[1]), (tag, site, results[site])
            assert np.array_equal(after.packed[site], before.packed[site]), (tag, site, "a failed pass changed a belief")
            assert np.array_equal(after.res[site], before.res[site]) and np.array_equal(after.flg[site], before.flg[site]), (tag, site)
        U.check_pass(ub, before, after, results, kernel, MARGIN, tag)
    U.report()


@pytest.mark.parametrize("n_sites", M.UNI_SITES)
@pytest.mark.parametrize("m", [1, 2])
def test_integrate_info_at_the_last_pivot(P, m, n_sites):
    """pgbp_integrate on 1- and 2-variable beliefs: info == m in the event sites, mean and constant correct elsewhere."""
    beliefs, dims, sepcl, so, si, packed = M.uni_integrate_inputs(m, n_sites)
    cgb = P.ClusterGraphBelief.from_arrays(dims, sepcl, so, si, packed, n_sites=n_sites)
    mu, norm, info = cgb.integratebelief_(0, all_sites=True)
    for site in range(n_sites):
        if site in M.UNI_EVENT_SITES[n_sites]:
            assert info[site] == m, (site, info[site])
            continue
        rmu, rnorm, rinfo = M.integrate_ld(*beliefs[site])
        cmu, cnorm, cinfo = M.c_engine_integrate(dims, sepcl, so, si, packed[site])
        assert info[site] == rinfo == cinfo == 0
        for got, cgot, want in (((mu[site],), (cmu,), (rmu,)), (([norm[site]],), ([cnorm],), ([rnorm],))):
            err, scale = M.record_error(got, want)
            floor = max(M.record_error(cgot, want)[0], m * U.EPS * scale)
            print(f"integrate m={m} n_sites={n_sites} site {site}: device {err / scale:.3e} ratio {err / floor:.2f}")
            assert err <= U.RTOL * scale and err <= MARGIN * floor, (site, err / scale, err / floor)


@pytest.mark.parametrize("tuning", ["no_chunks", "no_tail"])
def test_per_level_kernels_of_two_level_chains(P, tuning):
    """The per-level kernel bp_level_uni1 on engines whose default plan fuses the levels (bp_chunk_uni1): the two-level
    chains of every shape with s <= 1 in a child process under a PGBP_TUNING value that switches chunks off
    (tests/run_uni_message_shapes.py asserts from the planner's report that no chunk ran)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env["PGBP_TUNING"] = tuning
    out = subprocess.run([sys.executable, os.path.join(here, "run_uni_message_shapes.py"), "8", "65"], env=env,
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-1200:])
    assert out.returncode == 0 and "216 two-level chains ok" in out.stdout, (out.stdout[-1500:], out.stderr[-1500:])
    assert "bp_level_uni1<false>" in out.stdout and "bp_level_uni1<true>" in out.stdout and "bp_chunk" not in out.stdout

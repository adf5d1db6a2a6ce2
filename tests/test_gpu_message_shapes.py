"""Every wave-per-task message kernel (csrc/pgbp_kernels.hip, csrc/pgbp_pair.hip) placed on both sides of its shape limits,
with index maps chosen here, against the numpy.longdouble restatement of one message (tests/message_ref.py, pinned on the
CPU by tests/test_message_ref_cpu.py): (a) one message through pgbp_propagate at every limit, (b) the all-zero exit of
marginalize and its eps threshold, (c) PosDefException.info at a chosen pivot k -- not only k = 1 -- for the four bodies and
for integrate_kernel, (d) integratebelief! without failure, (e) the kernels that only a traversal reaches, on synthetic
clique trees in a child process per PGBP_TUNING value (tests/run_shape_trees.py).

Tolerances.  The project's gate, 1e-8 * max(1, |.|_inf) per record, and a tight one: the device's error to the longdouble
reference is at most MARGIN x the error of the float64 plain-C engine to the same reference on the same inputs, floored at
m * eps * max(1, |.|_inf) (m = the sender's dimension) so that an exact C result does not demand exactness.  MARGIN is the
worst device / C-engine ratio measured over the whole sweep on an MI355X, rounded up to the next power of two, times 4 (the
reciprocal-plus-Newton division, the different update order, the mantissa-product log-determinant):
MEASURED_RATIO and MARGIN below.  Measured (MI355X, whole sweep (a)-(d)): worst ratio 0.96 (the normalisation constant of
integratebelief!; messages: 0.57 small body, 0.42 in-LDS, 0.25 bp_level_big in LDS, 0.30 workspace), so MARGIN = 1 x 4 = 4;
worst error relative to max(1, |.|_inf): small body 1.3e-15, in-LDS 6.0e-15, big-LDS 7.1e-15, big-workspace 2.1e-14,
integrate 3.0e-15.

The per-message status word has no host accessor; it is written from the same register as the info word that pgbp_propagate
returns (checked here) and its one reader, residual_kldiv!, is covered by test_gpu_parity.py.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import message_ref as M

pytestmark = pytest.mark.gpu

RTOL = 1e-8            # tests/test_gpu_parity.py
EPS = M.EPS
MEASURED_RATIO = 0.962  # worst (device error) / max(C-engine error, m eps scale) over (a)-(d) on an MI355X
MARGIN = 4.0           # 0.962 -> next power of two 1 -> x 4


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


@functools.lru_cache(maxsize=None)
def _built(case):
    return M.build_case(case)


RATIOS = {}   # (body, record) -> worst ratio seen in this process (printed with every figure)


def _engine(P, b, packed):
    return P.ClusterGraphBelief.from_arrays(b.dims, b.sepcl, b.scope_off, b.scope_idx, packed, n_sites=2)


def _propagate(cgb, b):
    from pgbp_amd import _lib as L
    info = np.zeros(2, dtype=np.int32)
    o = cgb._opts()
    assert cgb._lib.pgbp_propagate(cgb._eng, int(b.i_to), 2, int(b.i_from), C.byref(o), L.i32p(info)) == 0
    cgb.pull()
    return info, cgb._packed_raw.copy(), cgb._res.copy(), cgb._flg.copy()


def _device_records(b, packed_site, res_site):
    snd, sep, rcv = M.records_of(b, packed_site)
    s = b.case.s
    d = 1 if b.i_to == 1 else 0
    r = res_site[d * (s * s + s):(d + 1) * (s * s + s)]
    return snd, sep, rcv, (r[:s * s].reshape(s, s, order="F"), r[s * s:]), d


def _check_good_site(b, site, before, after, res, flg, tag):
    """One site whose message must go through: gate and tight tolerance against propagate_ld on `before`, the sender and
    everything of the receiver outside the up map bit for bit as before, the flag by the reference's rule."""
    case = b.case
    ref = M.reference_of(b, site, before)
    assert ref[3] == 0
    cerr = M.c_engine_errors(b, site, ref, before)
    snd, sep, rcv, resid, d = _device_records(b, after, res)
    snd0, _, rcv0 = M.records_of(b, before)
    for x, y in zip(snd, snd0):
        assert np.array_equal(x, y), (tag, "the sender changed")
    out = np.setdiff1d(np.arange(case.mt), b.up)
    assert np.array_equal(rcv[0][np.ix_(out, out)], rcv0[0][np.ix_(out, out)]) and np.array_equal(rcv[1][out], rcv0[1][out]), tag
    if case.s:   # rows / columns of the up map against the others: untouched as well
        assert np.array_equal(rcv[0][np.ix_(b.up, out)], rcv0[0][np.ix_(b.up, out)]), tag
        assert np.array_equal(rcv[0][np.ix_(out, b.up)], rcv0[0][np.ix_(out, b.up)]), tag
    body = M.body_of(case.mf, case.s, case.mt)
    for name, got, want in (("sepset", sep, ref[0]), ("receiver", rcv, ref[1]), ("residual", resid, ref[2])):
        err, scale = M.record_error(got, want)
        floor = max(cerr[name][0], max(1, case.mf) * EPS * scale)
        ratio = err / floor
        RATIOS[(body, name)] = max(RATIOS.get((body, name), 0.0), ratio)
        RATIOS[(body, "abs")] = max(RATIOS.get((body, "abs"), 0.0), err / scale)
        print(f"{tag} site {site} {name}: device {err / scale:.3e} C {cerr[name][0] / scale:.3e} ratio {ratio:.2f}")
        assert err <= RTOL * scale, (tag, site, name, err / scale)
        assert err <= MARGIN * floor, (tag, site, name, err, floor, ratio)
    assert bool(flg[d]) == M.residnorm_flag_ld(*ref[2]), (tag, site)


@pytest.mark.parametrize("case", M.shape_cases(), ids=lambda c: c.name)
def test_one_message_at_every_shape_limit(P, case):
    """(a) bp_level_generic (small and in-LDS bodies) and bp_level_big (LDS and workspace), chosen by shape alone."""
    b = _built(case)
    info, after, res, flg = _propagate(_engine(P, b, b.packed), b)
    assert list(info) == [0, 0]
    for site in range(2):
        _check_good_site(b, site, b.packed[site], after[site], res[site], flg[site], case.name)


@pytest.mark.parametrize("body", M.BODIES)
def test_exit2_and_its_threshold(P, body):
    """(b) J_I = c I, h_I = 0, J_KI = 0: c = eps is the all-zero exit (the message is (h_K, J_K, g) exactly); c = 2 eps is
    not (the same J and h, g shifted by (ni log 2pi - ni log c) / 2)."""
    at_eps, above = [c for c in M.exit2_cases() if c.name.startswith(f"b-{body}-")]
    out = {}
    for case in (at_eps, above):
        b = _built(case)
        info, after, res, flg = _propagate(_engine(P, b, b.packed), b)
        assert list(info) == [0, 0]
        for site in range(2):
            _check_good_site(b, site, b.packed[site], after[site], res[site], flg[site], case.name)
        out[case] = (b, _device_records(b, after[0], res[0]))
    b, (snd, sep, rcv, resid, _) = out[at_eps]
    J, h, g = b.senders[0]
    assert M.reference_of(b, 0)[4] == 2
    assert np.array_equal(sep[0], J[np.ix_(b.keep, b.keep)]) and np.array_equal(sep[1], h[b.keep]) and sep[2] == g
    b2, (_, sep2, _, _, _) = out[above]
    assert M.reference_of(b2, 0)[4] == 0
    J2, h2, g2 = b2.senders[0]
    assert np.array_equal(sep2[0], J2[np.ix_(b2.keep, b2.keep)]) and np.array_equal(sep2[1], h2[b2.keep])
    ni = above.mf - above.s
    shift = (ni * np.log(2 * np.pi) - ni * np.log(2 * EPS)) / 2
    assert abs(sep2[2] - (g2 + shift)) <= RTOL * max(1.0, abs(g2 + shift))


@pytest.mark.parametrize("case", M.failure_cases(), ids=lambda c: c.name)
def test_info_at_a_chosen_pivot(P, case):
    """(c) a failure placed at pivot k of one site: info == k, that site's sepset, receiver, residual and flag bit for bit
    as before the call (a message sent before filled them), the other site -- a good matrix of the same shape -- updated
    correctly."""
    from pgbp_amd import _lib as L
    b = _built(case)
    bad_site, k, _ = case.fail
    good = b.packed.copy()
    good[bad_site] = b.packed[1 - bad_site]        # first both sites good: the residual and the sepset get real values
    cgb = _engine(P, b, good)
    info, after1, res1, flg1 = _propagate(cgb, b)
    assert list(info) == [0, 0]
    off = M.record_offsets(b.dims)
    rec = np.ascontiguousarray(b.packed[bad_site][off[b.i_from]:off[b.i_from + 1]])
    assert cgb._lib.pgbp_set_belief(cgb._eng, bad_site, int(b.i_from), L.f64p(rec)) == 0
    cgb.pull()
    before, res0, flg0 = cgb._packed_raw.copy(), cgb._res.copy(), cgb._flg.copy()
    assert np.array_equal(res0, res1) and np.array_equal(before[1 - bad_site], after1[1 - bad_site])
    info, after, res, flg = _propagate(cgb, b)
    print(f"{case.name}: info {list(info)}")
    assert info[bad_site] == k and info[1 - bad_site] == 0, (case.name, list(info))
    assert np.array_equal(after[bad_site], before[bad_site]), "a failed message changed a belief"
    assert np.array_equal(res[bad_site], res0[bad_site]) and np.array_equal(flg[bad_site], flg0[bad_site])
    assert res0[bad_site].any() or case.s == 0
    _check_good_site(b, 1 - bad_site, before[1 - bad_site], after[1 - bad_site], res[1 - bad_site], flg[1 - bad_site], case.name)


def _integrate(P, dims, sepcl, so, si, packed):
    cgb = P.ClusterGraphBelief.from_arrays(dims, sepcl, so, si, packed, n_sites=2)
    return cgb.integratebelief_(0, all_sites=True)


def _check_integrate_site(m, belief, dims, sepcl, so, si, packed_site, mu, norm, tag):
    rmu, rnorm, rinfo = M.integrate_ld(*belief)
    cmu, cnorm, cinfo = M.c_engine_integrate(dims, sepcl, so, si, packed_site)
    assert rinfo == cinfo == 0
    for name, got, cgot, want in (("mu", (mu,), (cmu,), (rmu,)), ("norm", ([norm],), ([cnorm],), ([rnorm],))):
        err, scale = M.record_error(got, want)
        floor = max(M.record_error(cgot, want)[0], m * EPS * scale)
        ratio = err / floor
        RATIOS[("integrate", name)] = max(RATIOS.get(("integrate", name), 0.0), ratio)
        RATIOS[("integrate", "abs")] = max(RATIOS.get(("integrate", "abs"), 0.0), err / scale)
        print(f"{tag} {name}: device {err / scale:.3e} ratio {ratio:.2f}")
        assert err <= RTOL * scale, (tag, name, err / scale)
        assert err <= MARGIN * floor, (tag, name, err, floor, ratio)


@pytest.mark.parametrize("m", M.INTEGRATE_DIMS)
def test_integrate_at_every_body_limit(P, m):
    """(d) integrate_kernel's three bodies (16 / 128) without failure: mean and normalisation constant."""
    beliefs, dims, sepcl, so, si, packed = M.integrate_inputs(m)
    mu, norm, info = _integrate(P, dims, sepcl, so, si, packed)
    assert list(info) == [0, 0]
    for site in range(2):
        _check_integrate_site(m, beliefs[site], dims, sepcl, so, si, packed[site], mu[site], norm[site], f"integrate-{m}-{site}")


@pytest.mark.parametrize("m,k,kind,site", M.integrate_failure_cases())
def test_integrate_info_at_a_chosen_pivot(P, m, k, kind, site):
    """(c) pgbp_integrate: info == k in the damaged site, the other site's mean and constant correct."""
    beliefs, dims, sepcl, so, si, packed = M.integrate_inputs(m, (site, k, kind))
    mu, norm, info = _integrate(P, dims, sepcl, so, si, packed)
    assert info[site] == k and info[1 - site] == 0, (m, k, kind, list(info))
    o = 1 - site
    _check_integrate_site(m, beliefs[o], dims, sepcl, so, si, packed[o], mu[o], norm[o], f"integrate-{m}-k{k}-{kind}")


@pytest.mark.parametrize("tuning", ["", "small4_min=0", "no_chunks", "pair=0", "no_tail", "mixed_fast_min=0"],
                         ids=["default", "four_tasks_per_wavefront", "no_chunks", "chunks_one_wavefront_per_task",
                              "levels_only", "mixed_levels_always_split"])
def test_kernels_that_only_a_traversal_reaches(P, tuning):
    """(e) tests/run_shape_trees.py: bp_level_small4 (rows as tasks and as messages), bp_chunk_pair, bp_chunk_generic,
    tasks of several messages on bp_level_generic, accumulating tasks on bp_level_big -- synthetic clique trees with
    dimensions from the shape limits against the plain-C engine, with pivot-placed failures at k > 1; the planner's own
    report says the intended class ran."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env.pop("PGBP_TUNING", None)
    if tuning:
        env["PGBP_TUNING"] = tuning
    out = subprocess.run([sys.executable, os.path.join(here, "run_shape_trees.py"), "24", "5"], env=env,
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-400:])
    assert out.returncode == 0 and "24 trees ok (48 placed failures" in out.stdout, (out.stdout[-1500:], out.stderr[-1500:])

"""tests/message_ref.py pinned without a GPU: the longdouble restatement of one message against the float64 restatement
(oracle/beliefupdates.py) and against the plain-C engine (oracle/cengine.py) on EVERY input of the device sweep of
tests/test_gpu_message_shapes.py -- both early exits of marginalize, both sides of the eps threshold, PosDefException.info at
every placed pivot -- so that the device tests compare with a reference that two independent float64 engines agree with.

No case is skipped or filtered: the C engine alone satisfies every assertion the device tests make (project gate 1e-8 per
record; info == k; a failed message changes nothing), which is checked here.  The error of the C engine against the
longdouble reference is the device tests' measuring stick; its bound here is 64 * mf * eps * max(1, |.|_inf): Cholesky and
the two triangular solves are backward stable with constants of a few n * eps, the inputs have condition number <= 10 by
construction, and 64 = 10 x (a constant of 6) leaves no room for a wrong entry (a wrong entry is an error of order 1).
"""
import numpy as np
import pytest

import message_ref as M
from oracle import beliefupdates as bu

EPS = M.EPS
ALL = M.all_message_cases()


def test_sweep_has_every_case_the_issue_lists():
    names = [c.name for c in ALL]
    assert len(set(names)) == len(names)
    shapes = {(c.mf, c.s) for c in M.shape_cases()}
    for ni, s in [(1, 1), (8, 8), (8, 1), (1, 8), (0, 8), (8, 0), (9, 8), (8, 9), (9, 9)]:
        assert (ni + s, s) in shapes
    for mf, ss in [(17, (0, 1, 8, 16, 17)), (64, (0, 1, 32, 63, 64)), (65, (1, 64)), (128, (1, 64, 127)), (129, (1, 128)),
                   (384, (1, 128, 383))]:
        assert all((mf, s) in shapes for s in ss)
    assert {c.mt for c in M.shape_cases() if (c.mf, c.s) == (4, 2)} >= {254, 255, 384}
    bodies = {b: [c for c in M.shape_cases() if M.body_of(c.mf, c.s, c.mt) == b] for b in M.BODIES}
    assert all(len(v) >= 7 for v in bodies.values())
    for body in M.BODIES:
        ks = {c.fail[1] for c in M.failure_cases() if c.name.startswith(f"c-{body}-sign")}
        mf, s = M._BODY_SHAPE[body][:2]
        assert ks == set(M.pivots_for(mf - s)) and min(ks) == 1 and max(ks) == mf - s
    assert {16, 17, 64, 65} <= set(M.pivots_for(127)) and {16, 17} <= set(M.pivots_for(63))


def _oracle_message(b, site):
    """oracle/beliefupdates.py on one site: (sepset, receiver, residual) or the exception's info."""
    J, h, g = b.senders[site]
    try:
        mh, mJ, mg = bu.marginalize(h, J, g, b.keep)
    except bu.BPPosDefException as ex:
        return ex.info
    sJ, sh, sg = b.sepsets[site]
    dh, dJ, dg = bu.divide(sh, sJ, sg, mh, mJ, mg)
    tJ, th, tg = b.receivers[site][0].copy(), b.receivers[site][1].copy(), np.array([b.receivers[site][2]])
    bu.mult_inplace(th, tJ, tg, b.up, dh, dJ, dg)
    return (mJ, mh, mg), (tJ, th, tg[0]), (dJ, dh)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_reference_agrees_with_both_float64_engines(case):
    b = M.build_case(case)
    bound = 64 * max(1, case.mf) * EPS
    for site in range(2):
        new_sep, new_rcv, resid, info, ex = M.reference_of(b, site)
        sep, rcv, res, snd, cinfo, cflag = M.c_engine_message(b, site)
        orc = _oracle_message(b, site)
        f = case.fail
        want_info = f[1] if f is not None and f[0] == site else 0
        assert info == cinfo == want_info, (site, info, cinfo, want_info)
        for x, y in zip(snd, b.senders[site]):           # the sender is read-only
            assert np.array_equal(np.asarray(x), np.asarray(y))
        if want_info:
            assert orc == want_info
            for got, start in ((sep, b.sepsets[site]), (rcv, b.receivers[site])):
                for x, y in zip(got, start):
                    assert np.array_equal(np.asarray(x), np.asarray(y))    # nothing is changed
            continue
        assert ex == (1 if case.s == case.mf else (2 if f is not None and f[0] == "exit2" and site == 0 and f[1] <= EPS else 0))
        for name, got, o, want in (("sepset", sep, orc[0], new_sep), ("receiver", rcv, orc[1], new_rcv),
                                   ("residual", res, orc[2], resid)):
            for eng, x in (("c", got), ("oracle", o)):
                err, scale = M.record_error(x, want)
                assert err <= bound * scale, (eng, name, site, err / scale, bound)
                assert err <= 1e-8 * scale                                  # the project's gate
        assert cflag == M.residnorm_flag_ld(*resid), site
        # variables of the receiver outside the up map: bit for bit as before
        out = np.setdiff1d(np.arange(case.mt), b.up)
        assert np.array_equal(rcv[0][np.ix_(out, out)], b.receivers[site][0][np.ix_(out, out)])
        assert np.array_equal(rcv[1][out], b.receivers[site][1][out])
    if case.sep_kind == "near" and case.fail is None and case.s:
        assert M.residnorm_flag_ld(*M.reference_of(b, 0)[2])
    if case.sep_kind != "near" and case.fail is None and case.s:
        assert not M.residnorm_flag_ld(*M.reference_of(b, 0)[2])


@pytest.mark.parametrize("case", M.exit2_cases(), ids=lambda c: c.name)
def test_exit2_and_its_threshold(case):
    """J_I = c I, h_I = 0, J_KI = 0: with c = eps the message is (h_K, J_K, g) exactly; with c = 2 eps it is no exit: the
    same J and h, g shifted by (ni log 2pi - ni log c) / 2 -- in the reference and in the C engine."""
    b = M.build_case(case)
    c = case.fail[1]
    J, h, g = b.senders[0]
    (mJ, mh, mg), _, _, info, ex = M.reference_of(b, 0)
    sep = M.c_engine_message(b, 0)[0]
    keep = b.keep
    assert info == 0 and ex == (2 if c <= EPS else 0)
    assert np.array_equal(mJ.astype(np.float64), J[np.ix_(keep, keep)]) and np.array_equal(mh.astype(np.float64), h[keep])
    assert np.array_equal(sep[0], J[np.ix_(keep, keep)]) and np.array_equal(sep[1], h[keep])
    ni = case.mf - case.s
    shift = 0.0 if c <= EPS else (ni * np.log(2 * np.pi) - ni * np.log(c)) / 2
    assert abs(float(mg) - (g + shift)) <= 8 * EPS * max(1.0, abs(g + shift))
    assert (sep[2] == g) if c <= EPS else abs(sep[2] - (g + shift)) <= 64 * ni * EPS * max(1.0, abs(g + shift))


@pytest.mark.parametrize("kind", ["sign", "zero"])
def test_pivot_placed_failures_fail_where_placed(kind):
    """The generators: info == k in longdouble and in float64, row-by-row Cholesky and LAPACK; the dyadic generator's J is
    exact (its float64 product equals the longdouble one) and both eliminations meet an exact 0.0 at pivot k."""
    from scipy.linalg import lapack
    for n in (8, 63, 127, 191, 384):
        for k in M.pivots_for(n):
            rng = np.random.default_rng(1000 * n + k)
            J = M.ldl_failure(rng, n, k, kind)
            _, ild, pld = M.chol_upper_rows(J, M.LD)
            _, i64, p64 = M.chol_upper_rows(J, np.float64)
            assert ild == i64 == k, (n, k, ild, i64)
            assert int(lapack.dpotrf(np.asfortranarray(J), lower=0)[1]) == k
            if kind == "zero":
                assert pld == 0 and p64 == 0.0
                # right-looking elimination (the kernels' order) in float64 meets the same exact zero
                W = J.copy()
                for j in range(k - 1):
                    assert W[j, j] > 0
                    W[j + 1:, j + 1:] -= np.outer(W[j + 1:, j] * (1.0 / W[j, j]), W[j, j + 1:])
                assert W[k - 1, k - 1] == 0.0
            else:
                assert pld < -0.5 and p64 < -0.5
                if k > 1:   # the minors before it are clearly positive
                    U = M.chol_upper_rows(J[:k - 1, :k - 1], M.LD)[0]
                    assert float(np.diag(U).min()) ** 2 >= 0.99


@pytest.mark.parametrize("m", M.INTEGRATE_DIMS)
def test_integrate_reference_agrees_with_the_c_engine(m):
    beliefs, dims, sepcl, so, si, packed = M.integrate_inputs(m)
    for site in range(2):
        mu, norm, info = M.integrate_ld(*beliefs[site])
        cmu, cnorm, cinfo = M.c_engine_integrate(dims, sepcl, so, si, packed[site])
        omu, onorm = bu.integratebelief(beliefs[site][1], beliefs[site][0], beliefs[site][2])
        assert info == cinfo == 0
        bound = 64 * m * EPS
        for x, n_ in ((cmu, cnorm), (omu, onorm)):
            assert M.record_error((x,), (mu,))[0] <= bound * M.record_error((x,), (mu,))[1]
            assert abs(float(M.LD(n_) - norm)) <= bound * max(1.0, abs(float(norm)))


@pytest.mark.parametrize("m,k,kind,site", M.integrate_failure_cases())
def test_integrate_failure_reference_agrees_with_the_c_engine(m, k, kind, site):
    beliefs, dims, sepcl, so, si, packed = M.integrate_inputs(m, (site, k, kind))
    for s in range(2):
        info = M.integrate_ld(*beliefs[s])[2]
        cinfo = M.c_engine_integrate(dims, sepcl, so, si, packed[s])[2]
        assert info == cinfo == (k if s == site else 0)


def test_integrate_constant_belief():
    mu, norm, info = M.integrate_ld(np.zeros((3, 3)), np.zeros(3), 1.5)
    assert info == 0 and np.all(np.isinf(mu)) and norm == 1.5

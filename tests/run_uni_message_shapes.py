#!/usr/bin/env python3
"""One message of every tiny shape through the thread-per-site kernels (csrc/pgbp_kernels.hip: bp_level_uni, bp_level_uni1,
bp_chunk_uni1; lanes = sites), every site against the numpy.longdouble restatement of tests/message_ref.py.  The checks are
functions used by tests/test_gpu_uni_message_shapes.py; as a program it runs the two-level chains (kind "chain1") under the
current PGBP_TUNING, which that test starts in a child process per tuning value that switches the loop mode off.

pgbp_propagate always takes the wave-per-task kernel, so a message is sent by a TRAVERSAL: the schedule tree is rooted at the
last cluster of the engine's chain (the receiver itself for a two-cluster engine) and one postorder pass sends the messages.

Which kernel ran is derived, not assumed: bp_level_uni against the uni1 pair from the engine's largest sepset (`dims`),
site-minor from pgbp_layout() & 2 read right after the pass, the loop mode (bp_chunk_uni1) from the planner's own report of
the same description under the same PGBP_TUNING (pgbp_plan_chunks: one chunk that covers every level) and not taken when
residual_kldiv! runs between the levels.

  python tests/run_uni_message_shapes.py [n_sites ...]
"""
import ctypes as C
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import message_ref as M  # noqa: E402

RTOL = 1e-8      # the project's gate: 1e-8 * max(1, |.|_inf) per record
EPS = M.EPS
STATS = {}       # kernel instance -> {"abs": worst error / scale, "ratio": worst device / max(C engine, floor), "n": messages}
_REFS = {}       # (case, kind, bytes of one site's beliefs) -> (uni_reference, uni_c_engine): shared by every engine size


def plan_report(P, ub):
    """(levels of the postorder, [(first level, one past the last level)] of its chunks) of the CPU plan of ub's
    description under the current PGBP_TUNING."""
    from pgbp_amd import _lib as L
    lib = P.load()
    desc, keep = L.make_desc(ub.dims, ub.sepcl, ub.scope_off, ub.scope_idx, ub.n_sites, 0)
    pl = C.c_void_p()
    assert lib.pgbp_plan_create(C.byref(desc), C.byref(pl)) == 0, lib.pgbp_plan_last_error(pl)
    off = np.array([0, len(ub.pa)], np.int32)
    assert lib.pgbp_plan_set_schedule(pl, 1, L.i32p(off), L.i32p(ub.pa), L.i32p(ub.ch)) == 0, lib.pgbp_plan_last_error(pl)
    nl, nt, ne, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.pgbp_plan_traversal_sizes(pl, 0, 0, C.byref(nl), C.byref(nt), C.byref(ne)) == 0
    assert lib.pgbp_plan_chunks(pl, 0, 0, C.byref(n), None, None, None) == 0
    info = np.zeros(4 * max(1, n.value), np.int32)
    assert lib.pgbp_plan_chunks(pl, 0, 0, C.byref(n), L.i32p(info), None, None) == 0
    lib.pgbp_plan_destroy(pl)
    return nl.value, [(int(info[4 * i]), int(info[4 * i + 1])) for i in range(n.value)]


def kernel_instance(P, ub, layout, kl):
    """The kernel that ran a postorder of this engine, from the facts that select it (csrc/pgbp_engine.hip: enqueue_levels,
    csrc/pgbp_kernels.hip: launch_level_uni)."""
    assert int(ub.dims.max()) <= 2 and ub.n_sites >= 8                  # thread-per-site at all
    sm = "true" if layout & 2 else "false"
    assert bool(layout & 2) == (ub.n_sites >= 64 and not kl)             # residual_kldiv! belongs to the plain layout
    if int(ub.dims[ub.nc:].max()) > 1:
        return f"bp_level_uni<{sm}>"
    nlev, chunks = plan_report(P, ub)
    assert nlev == len(ub.msgs)
    if chunks and not kl:
        assert chunks == [(0, nlev)], chunks                             # every level inside the one chunk
        return f"bp_chunk_uni1<{sm}>"
    return f"bp_level_uni1<{sm}>"


def engine(P, ub, packed=None):
    return P.ClusterGraphBelief.from_arrays(ub.dims, ub.sepcl, ub.scope_off, ub.scope_idx, ub.packed if packed is None else packed,
                                            n_sites=ub.n_sites)


def state_of(cgb):
    cgb.pull()
    return types.SimpleNamespace(packed=cgb._packed_raw.copy(), res=cgb._res.copy(), flg=cgb._flg.copy(), kl=cgb._kl.copy(),
                                 klflg=cgb._klflg.copy())


def postorder(P, cgb, ub, kl=False):
    """One postorder pass: (state after it, per-site results, kernel instance)."""
    P.propagate_1traversal_postorder_(cgb, None, None, ub.pa, ub.ch, verbose=False, update_residualkldiv=kl, sync=False)
    layout = int(cgb._lib.pgbp_layout(cgb._eng))
    results = [(int(r.succ), int(r.fail_info), int(r.fail_edge), int(r.fail_dir)) for r in cgb.last_results]
    return state_of(cgb), results, kernel_instance(P, ub, layout, kl)


def _refs(ub, before_site):
    key = (ub.case.name, ub.kind, before_site.tobytes())
    if key not in _REFS:
        _REFS[key] = (M.uni_reference(ub, before_site), M.uni_c_engine(ub, before_site))
    return _REFS[key]


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _oracle_kldiv(new_sep, resid):
    """residual_kldiv! (oracle/beliefs.py, src/beliefs.jl:1060-1075) on the reference's message: (kldiv, flag)."""
    from oracle import beliefs as OB
    s = new_sep[1].size
    res = types.SimpleNamespace(dJ=np.asarray(resid[0], np.float64), dh=np.asarray(resid[1], np.float64),
                                kldiv=0.0 if s == 0 else -1.0, iscalibrated_kl=s == 0)
    sep = types.SimpleNamespace(J=np.asarray(new_sep[0], np.float64), h=np.asarray(new_sep[1], np.float64), mu=None)
    OB.residual_kldiv(res, sep)
    return res.kldiv, bool(res.iscalibrated_kl)


def check_pass(ub, before, after, results, kernel, margin, tag, kl=False, verbose=False):
    """EVERY site of one postorder pass against the reference on that site's own numbers (`before` / `after`: state_of)."""
    st = STATS.setdefault(kernel, {"abs": 0.0, "ratio": 0.0, "n": 0})
    for site in range(ub.n_sites):
        refs, (cpk, cres, cflg, cinfos) = _refs(ub, before.packed[site])
        r0, r1 = M.uni_records(ub, before.packed[site]), M.uni_records(ub, after.packed[site])
        crec = M.uni_records(ub, cpk)
        first = ub.msgs[0]
        assert _same(r1[first.i_from], r0[first.i_from]), (tag, site, "the sender changed")
        want_fail = 0
        for j, (m, ref) in enumerate(zip(ub.msgs, refs)):
            sep_i = ub.nc + m.k
            (dJ, dh), d = M.residual_of(ub, m, after.res[site])
            (dJ0, dh0), _ = M.residual_of(ub, m, before.res[site])
            if ref is None or ref[3]:
                # a failed message, or the message out of a cluster whose own receipt failed: nothing is touched
                if ref is not None:
                    want_fail = want_fail or ref[3]
                    assert site in ub.fail_sites and ref[3] == ub.case.fail[1] and cinfos[j] == ref[3], (tag, site, j)
                assert _same(r1[sep_i], r0[sep_i]) and _same(r1[m.i_to], r0[m.i_to]), (tag, site, j, "a message that was not sent changed a belief")
                assert np.array_equal(dJ, dJ0) and np.array_equal(dh, dh0) and after.flg[site][d] == before.flg[site][d], (tag, site, j)
                continue
            mt = int(ub.dims[m.i_to])
            out = np.setdiff1d(np.arange(mt), m.up)
            J1, h1, _ = r1[m.i_to]
            J0, h0, _ = r0[m.i_to]
            assert np.array_equal(J1[np.ix_(out, out)], J0[np.ix_(out, out)]) and np.array_equal(h1[out], h0[out]), (tag, site, j)
            assert np.array_equal(J1[np.ix_(m.up, out)], J0[np.ix_(m.up, out)]) and np.array_equal(J1[np.ix_(out, m.up)], J0[np.ix_(out, m.up)]), (tag, site, j)
            (cdJ, cdh), _ = M.residual_of(ub, m, cres)
            mf = max(1, int(ub.dims[m.i_from]))
            for name, got, cgot, want in (("sepset", r1[sep_i], crec[sep_i], ref[0]), ("receiver", r1[m.i_to], crec[m.i_to], ref[1]),
                                          ("residual", (dJ, dh), (cdJ, cdh), ref[2])):
                err, scale = M.record_error(got, want)
                floor = max(M.record_error(cgot, want)[0], mf * EPS * scale)
                st["abs"], st["ratio"], st["n"] = max(st["abs"], err / scale), max(st["ratio"], err / floor), st["n"] + 1
                if verbose:
                    print(f"{tag} {kernel} site {site} message {j} {name}: device {err / scale:.3e} ratio {err / floor:.2f}")
                assert err <= RTOL * scale, (tag, kernel, site, j, name, err / scale)
                assert err <= margin * floor, (tag, kernel, site, j, name, err, floor, err / floor)
            assert bool(after.flg[site][d]) == M.residnorm_flag_ld(*ref[2]), (tag, site, j)
            if kl:
                okl, oflag = _oracle_kldiv(tuple(np.asarray(x, dtype=M.LD).astype(np.float64) for x in ref[0]), ref[2])
                got = float(after.kl[site][d])
                assert abs(got - okl) <= 1e-8 * max(1.0, abs(okl)), (tag, site, j, got, okl)
                if abs(abs(okl) - 1e-5) > 1e-7:     # not within rounding of the threshold
                    assert bool(after.klflg[site][d]) == oflag, (tag, site, j, got, okl)
        succ, fail_info = results[site][0], results[site][1]
        assert (succ, fail_info) == ((0, want_fail) if want_fail else (1, 0)), (tag, site, results[site], want_fail)
        assert bool(want_fail) == (site in ub.fail_sites), (tag, site)


def report():
    for kern in sorted(STATS):
        s = STATS[kern]
        print(f"{kern}: {s['n']} records, worst error {s['abs']:.3e} of max(1, |.|_inf), worst ratio to the C engine {s['ratio']:.3f}")


def main():
    import pgbp_amd as P
    P.load()
    from test_gpu_uni_message_shapes import MARGIN
    tuning = os.environ.get("PGBP_TUNING", "")
    sizes = [int(x) for x in sys.argv[1:]] or list(M.UNI_SITES)
    n = 0
    for ns in sizes:
        for case in M.uni_shape_cases():
            if case.s > 1:
                continue
            ub = M.build_uni(case, "chain1", ns)
            cgb = engine(P, ub)
            before = state_of(cgb)
            after, results, kernel = postorder(P, cgb, ub)
            if "no_chunks" in tuning or "no_tail" in tuning:
                assert kernel.startswith("bp_level_uni1<"), (tuning, kernel)
            check_pass(ub, before, after, results, kernel, MARGIN, f"{case.name}/{ns}")
            n += 1
    report()
    print(f"{n} two-level chains ok under PGBP_TUNING='{tuning}'")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The leaf-sepset shortcut and the message kernels' own "not calibrated" marks on small cluster graphs, under the
PGBP_TUNING of the environment (tests/test_gpu_leaf_sepset.py runs this in-process and, for no_tail / no_chunks, in a child
process each).  PGBP_TUNING is read when an engine is created, so the two engines of a case -- the default one and one with
`leaf_sepset=0` appended -- live in the same process.

Per case:
  * beliefs, sepsets, residuals, flags and (succ, iscal, failure key) after one and after three calibrate! are equal BIT FOR BIT
    between the two engines, and within the suite's parity tolerance (1e-8 * max(1, |.|) per belief) of the plain-C engine;
  * a preorder-only traversal and one pgbp_propagate into a leaf, each after the leaf's sepset was overwritten by hand: the
    stored sepset is what the message is divided by (bitwise equal to the engine that always loads it; the residual shows the
    overwrite);
  * a placed failure: same first-failure key and iscal on both engines and on the C engine;
  * exactly one false flag -- on the first message of the reference order, on the last, on one inside a fused chunk -- built
    from a calibrated state by shifting a sepset's h together with what the message lands on: iscal equals the AND over the
    flags of pgbp_get_residuals.

  python tests/run_leaf_sepset_cases.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import leaf_sepset_cases as K  # noqa: E402
import pgbp_amd as P  # noqa: E402
from oracle import cengine  # noqa: E402

RTOL = 1e-8
DONE = {}   # single-false-flag placements exercised by run(), by name
# (graph, tree, tips, p, sites): the planner test's shapes, then the smallest that reach the other paths -- the single edge
# (the pair turns inside the tail), odd p (plain layout, bp_fast16's own loop mode), three sites
CASES = [("cliquetree", "random", 2, 16, 1), ("cliquetree", "random", 3, 16, 1), ("cliquetree", "random", 40, 16, 1),
         ("cliquetree", "random", 45, 4, 1), ("cliquetree", "random", 50, 8, 1), ("cliquetree", "poly6", 70, 16, 1),
         ("cliquetree", "caterpillar", 30, 16, 1), ("bethe", "random", 50, 16, 1), ("edge", "", 2, 16, 1), ("edge", "", 2, 7, 1),
         ("cliquetree", "random", 40, 5, 1), ("cliquetree", "random", 12, 16, 3),
         ("cliquetree", "random", 12, 10, 1)]   # (a lane grid whose instances load the sepset and set no mark: leaf_mark_grid)


def make_engine(prob, packs, extra):
    base = os.environ.get("PGBP_TUNING")
    os.environ["PGBP_TUNING"] = ",".join(x for x in (base, extra) if x)
    try:
        eng = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, np.stack(packs),
                                               n_sites=len(packs))
    finally:
        if base is None:
            del os.environ["PGBP_TUNING"]
        else:
            os.environ["PGBP_TUNING"] = base
    eng.lazy = False
    return eng


def snapshot(eng):
    eng.pull()
    res = [(int(r.succ), int(r.iscal), int(r.fail_edge), int(r.fail_dir), int(r.fail_info), int(r.iter_reached), int(r.tree_reached))
           for r in eng.last_results]
    return eng._packed_raw.copy(), eng._res.copy(), eng._flg.copy(), res


def assert_same(a, b, tag):
    for name, x, y in zip(("beliefs", "residuals", "flags"), a[:3], b[:3]):
        assert np.array_equal(x, y), (tag, name, "differ between the default engine and leaf_sepset=0")
    assert a[3] == b[3], (tag, a[3], b[3])


def assert_parity(snap, refs, prob, tag):
    off = prob.packed_off
    for s, ref in enumerate(refs):
        want = ref.packed()
        for i in range(len(prob.dims)):
            x, y = snap[0][s, off[i]:off[i + 1]], want[off[i]:off[i + 1]]
            if len(y):
                err, scale = float(np.max(np.abs(x - y))), max(1.0, float(np.max(np.abs(y))))
                assert err <= RTOL * scale, (tag, s, i, err, scale)
        _, flags = ref.residuals()
        assert np.array_equal(snap[2][s].astype(bool)[:len(flags)], flags.astype(bool)), (tag, s, "flags")


def shift_h(eng, site, belief, idx, e):
    eng.site = site
    eng.belief[belief].h[idx] += e


def run_case(graph, kind, ntips, p, ns):
    tag = (graph, kind, ntips, p, ns, os.environ.get("PGBP_TUNING", ""))
    prob = K.problem(graph, kind, ntips, p)
    nc = prob.nclusters
    pa, ch = prob.schedule[0]
    sk = K.sepset_of_edge(prob)
    rng = np.random.default_rng(ntips + 31 * p + ns)
    packs = [K.spd_packed(prob, rng) for _ in range(ns)]
    marks, in_chunks = K.plan_marks(prob, ns)
    on, off = make_engine(prob, packs, ""), make_engine(prob, packs, "leaf_sepset=0")
    refs = [cengine.Engine(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, pk) for pk in packs]
    # ---- one and three calibrate!: bitwise between the engines, parity against the C engine
    for niter in (1, 2):
        for eng in (on, off):
            assert P.calibrate_(eng, prob.schedule, niter, sync=False)[0], tag
        a, b = snapshot(on), snapshot(off)
        assert_same(a, b, tag + (niter,))
        for s, ref in enumerate(refs):
            want = ref.calibrate(pa, ch, niter, return_iscal=True)
            assert (bool(a[3][s][0]), bool(a[3][s][1])) == want, (tag, s, a[3][s], want)
        assert_parity(a, refs, prob, tag + (niter,))
    marked = sorted(marks[1][1])
    if marked:
        # ---- the stored sepset still counts where the postorder of the same call did not fill it
        m = marked[len(marked) // 2]
        k = m // 2
        i = sk.index(k)
        leaf, par, s_dim = int(ch[i]), int(pa[i]), int(prob.dims[nc + k])
        for step in ("preorder", "propagate"):
            for eng in (on, off):
                eng.pull()   # (the traversals above ran without the write-back: the mirror is what gets uploaded)
                for s in range(ns):
                    eng.site = s
                    sep = eng.belief[nc + k]
                    sep.h[:] += 0.25
                    sep.J[np.arange(s_dim), np.arange(s_dim)] += 0.5
                eng.push()
                if step == "preorder":
                    assert P.propagate_1traversal_preorder_(eng, None, None, pa, ch, sync=False), tag
                else:
                    assert eng._propagate(leaf, nc + k, par, sync=False) is None, tag
            a, b = snapshot(on), snapshot(off)
            assert_same(a[:3] + ([],), b[:3] + ([],), tag + (step,))
            roff = on._roff
            for s in range(ns):   # the residual of the message into the leaf is (message - overwritten sepset): about -0.25 in h
                dh = a[1][s, roff[m] + s_dim * s_dim: roff[m + 1]]
                assert np.all(np.abs(dh + 0.25) < 1e-6), (tag, step, s, dh)
            for eng in (on, off):   # back to a calibrated state
                assert P.calibrate_(eng, prob.schedule, 2, sync=False)[0], tag
        assert_same(snapshot(on), snapshot(off), tag + ("recalibrated",))
        # ---- exactly one false flag; iscal against the AND over the downloaded flags
        site = ns // 2
        n = len(pa)
        last = n - 1
        picks = [("first", 0, last)]                                      # the postorder message of the last edge
        if K.msg_id(prob, sk[last], int(ch[last])) in marks[1][1]:
            picks.append(("last", 1, last))                               # the preorder message of the last edge, into its leaf
        chunk_edges = [e for e in range(n) if K.msg_id(prob, sk[e], int(pa[e])) in in_chunks[0] and prob.dims[nc + sk[e]] > 0]
        if chunk_edges:
            picks.append(("chunk", 0, chunk_edges[len(chunk_edges) // 2]))
        chunk_leaf = [e for e in range(n) if K.msg_id(prob, sk[e], int(ch[e])) in (in_chunks[1] & marks[1][1])]
        if chunk_leaf:
            picks.append(("chunk-leaf", 1, chunk_leaf[len(chunk_leaf) // 2]))
        for name, d, e in picks:
            k = sk[e]
            s_dim = int(prob.dims[nc + k])
            if s_dim == 0:
                continue
            DONE[name] = DONE.get(name, 0) + 1
            par, c = int(pa[e]), int(ch[e])
            target = par if d == 0 else c       # what the flagged message lands on
            flagged = K.msg_id(prob, k, target)
            side = 0 if int(np.asarray(prob.sepset_clusters).reshape(-1, 2)[k, 0]) == target else 1
            scope = prob.scope_idx[prob.scope_off[2 * k + side]:prob.scope_off[2 * k + side + 1]]
            for eng in (on, off):
                eng.pull()
                shift_h(eng, site, nc + k, slice(None), 0.5)
                shift_h(eng, site, target, scope, 0.5)
                eng.push()
                assert P.calibrate_(eng, prob.schedule, 1, sync=False)[0], tag
            a, b = snapshot(on), snapshot(off)
            assert_same(a, b, tag + (name,))
            for s in range(ns):
                bad = np.nonzero(a[2][s][:2 * len(sk)] == 0)[0].tolist()
                assert bad == ([flagged] if s == site else []), (tag, name, s, bad, flagged)
                assert bool(a[3][s][1]) == bool(np.all(a[2][s][:2 * len(sk)] != 0)), (tag, name, s, "iscal is not the AND of the flags")
        # ---- `auto`: the trees enqueued behind the one at which a site is calibrated do nothing for it, and its flags still count
        for eng in (on, off):
            assert P.calibrate_(eng, prob.schedule, 6, auto=True, sync=False) == (True, True), tag
        a, b = snapshot(on), snapshot(off)
        assert_same(a, b, tag + ("auto",))
        assert all(r[5] >= 1 for r in a[3]), (tag, "auto", a[3])
    del on, off
    # ---- a placed failure: the first cluster of 2p variables gets an indefinite block where it integrates
    big = [c for c in range(nc) if int(prob.dims[c]) == 2 * p and p > 0]
    if big:
        c = big[len(big) // 2]
        bad_site = ns - 1
        bad = [pk.copy() for pk in packs]
        o = int(prob.packed_off[c])
        m2 = 2 * p
        J = bad[bad_site][o:o + m2 * m2].reshape(m2, m2, order="F")
        edges_up = [i for i in range(len(pa)) if int(ch[i]) == c]
        k = sk[edges_up[0]] if edges_up else sk[[i for i in range(len(pa)) if int(pa[i]) == c][0]]
        side = 0 if int(np.asarray(prob.sepset_clusters).reshape(-1, 2)[k, 0]) == c else 1
        keep = prob.scope_idx[prob.scope_off[2 * k + side]:prob.scope_off[2 * k + side + 1]]
        integ = np.setdiff1d(np.arange(m2), keep)
        J[np.ix_(integ, integ)] = -1e6 * np.eye(len(integ))
        on, off = make_engine(prob, bad, ""), make_engine(prob, bad, "leaf_sepset=0")
        for eng in (on, off):
            P.calibrate_(eng, prob.schedule, 2, verbose=False, sync=False)
        a, b = snapshot(on), snapshot(off)
        assert a[3] == b[3], (tag, "failure", a[3], b[3])
        assert np.array_equal(a[2], b[2]), (tag, "failure", "flags")
        for s in range(ns):
            ref = cengine.Engine(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, bad[s])
            want = ref.calibrate(pa, ch, 2, return_iscal=True)
            assert (bool(a[3][s][0]), bool(a[3][s][1])) == want, (tag, "failure", s, a[3][s], want)
            if s == bad_site:
                assert not want[0], (tag, "the placed failure did not fail")
                assert a[3][s][2:5] == tuple(ref.last_failure()), (tag, "failure key", a[3][s], ref.last_failure())
    return len(marked), len(in_chunks[1] & marks[1][1])


def run():
    tot_marked = tot_chunk = 0
    DONE.clear()
    for case in CASES:
        nm, nchunk = run_case(*case)
        tot_marked += nm
        tot_chunk += nchunk
    tuning = os.environ.get("PGBP_TUNING", "")
    assert tot_marked > 0
    if "no_chunks" not in tuning and "no_tail" not in tuning:
        assert tot_chunk > 0, "no marked record inside a chunk: the loop kernel's consumer did not see one"
        assert DONE.get("chunk", 0) > 0 and DONE.get("chunk-leaf", 0) > 0, DONE
    # the single false flag was placed on the first and on the last message of the reference order under every tuning
    assert DONE.get("first", 0) > 0 and DONE.get("last", 0) > 0, DONE
    return tot_marked, tot_chunk


if __name__ == "__main__":
    nm, nchunk = run()
    print(f"{len(CASES)} cases ok: {nm} leaf-sepset records ({nchunk} inside chunks)")

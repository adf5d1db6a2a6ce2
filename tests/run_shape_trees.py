#!/usr/bin/env python3
"""Synthetic clique trees on plain arrays for the kernels that only a traversal reaches (run by
tests/test_gpu_message_shapes.py in a child process per PGBP_TUNING value; no phylogeny): bp_level_small4 with rows as tasks
and as messages, bp_chunk_pair, bp_chunk_generic, tasks of several messages on bp_level_generic, accumulating tasks on
bp_level_big.

A rooted tree of depth 7 with fan-in 1 to 5; cluster and sepset dimensions drawn from the kernels' shape limits -- a small
family (integrated and kept variables in {0, 1, 7, 8, 9}), a medium family (up to 64 variables) and one tree with a few
senders of 65 to 130 variables; keep and up maps from the four index patterns of tests/message_ref.py; every cluster a
well-conditioned SPD factor, every sepset the constant 1; 1 or 2 sites; calibrate!(2 iterations) against the plain-C
sequential engine: beliefs to 1e-8 * max|.|, residual flags, (succ, iscal).  Then once more with one pivot-placed failure at
pivot k > 1, in a cluster at the leaf end and in one next to the root: the same (fail_edge, fail_dir, fail_info).

A CPU plan of the same description (under the same PGBP_TUNING) says which class the planner chose: no fast-class task
anywhere (no tree holds a message of the register-resident kernel's shape: checked when the tree is drawn, the same trees
under every tuning), rows present under small4_min=0, chunks present unless no_chunks / no_tail.

  python tests/run_shape_trees.py [n_trees] [seed]
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import message_ref as M  # noqa: E402
import pgbp_amd as P  # noqa: E402
from oracle import cengine  # noqa: E402
from pgbp_amd import _lib as L  # noqa: E402

SMALL = (0, 1, 7, 8, 9)
MEDIUM = (1, 2, 8, 9, 16, 17, 31, 32)


def draw_tree(rng, family):
    """(dims, sepset_clusters, scope_off, scope_idx, pa, ch, depth, ni): clusters in breadth-first order (a preorder)."""
    pick = SMALL if family == "small" else MEDIUM
    m = [int(max(1, rng.choice(pick) + rng.choice(pick)))]
    depth, pa, ch, sdim, ni_of = [0], [], [], [], [0]
    frontier = [0]
    for d in range(1, 8):
        nxt = []
        for par in frontier:
            for _ in range(int(rng.integers(1, 6))):
                s = int(rng.choice([x for x in pick if x <= m[par]] or [0]))
                ni = int(rng.choice(pick))
                if ni + s == 0:
                    ni = 1
                c = len(m)
                m.append(ni + s)
                depth.append(d)
                ni_of.append(ni)
                pa.append(par)
                ch.append(c)
                sdim.append(s)
                nxt.append(c)
        frontier = [int(x) for x in rng.choice(nxt, min(len(nxt), 3 if family == "small" else 2), replace=False)]
    if family == "large":   # a few senders of 65 to 130 variables at the leaf end (their sepsets stay as drawn)
        fan = np.bincount(pa, minlength=len(m))
        leaves = [c for c, par in zip(ch, pa) if fan[c] == 0 and fan[par] > 1]   # (siblings: accumulating tasks)
        for c in rng.choice(leaves, 3, replace=False):
            e = ch.index(int(c))
            m[c] = int(rng.choice([65, 96, 128, 130]))
            ni_of[c] = m[c] - sdim[e]
    nc = len(m)
    sepcl, off, idx = [], [0], []
    for e in range(len(pa)):
        keep = M.index_pattern(M.PATTERNS[int(rng.integers(4))], m[ch[e]], sdim[e], rng)
        up = M.index_pattern(M.PATTERNS[int(rng.integers(4))], m[pa[e]], sdim[e], rng)
        if rng.random() < 0.5:
            sepcl += [pa[e], ch[e]]
            sides = (up, keep)
        else:
            sepcl += [ch[e], pa[e]]
            sides = (keep, up)
        for x in sides:
            idx.append(x)
            off.append(off[-1] + len(x))
    dims = np.array(m + sdim, np.int32)
    return (dims, np.array(sepcl, np.int32), np.array(off, np.int64), np.concatenate(idx).astype(np.int32),
            np.array(pa, np.int32), np.array(ch, np.int32), np.array(depth), np.array(ni_of), nc)


def has_fast_shape(dims, sepcl, scope_off, scope_idx, nc):
    """csrc/pgbp_plan.cpp's shape class of the register-resident kernel, restated: does any directed message have it?"""
    sd = dims[nc:]
    cnt = {q: int(np.sum(sd == q)) for q in range(2, 17)}
    best, Pq = 0, 0
    for q in range(16, 1, -1):
        if cnt[q] > best:
            best, Pq = cnt[q], q
    if Pq == 0:
        return False

    def first_if_contiguous(ix):
        return int(ix[0]) if len(ix) and np.all(np.diff(ix) == 1) else -1
    for k in range(len(sd)):
        s = int(sd[k])
        side = [scope_idx[scope_off[2 * k + j]:scope_off[2 * k + j + 1]] for j in (0, 1)]
        for frm in (0, 1):
            mf, mt = int(dims[sepcl[2 * k + frm]]), int(dims[sepcl[2 * k + 1 - frm]])
            if s == 0:
                if mf == Pq or mf == 0:
                    return True
                continue
            if s != Pq:
                continue
            k0, u0 = first_if_contiguous(side[frm]), first_if_contiguous(side[1 - frm])
            snd = (mf == Pq and k0 == 0) or (mf == 2 * Pq and k0 in (0, Pq))
            rcv = (mt == Pq and u0 == 0) or (mt == 2 * Pq and u0 in (0, Pq))
            if snd and rcv:
                return True
    return False


def plan_classes(dims, sepcl, scope_off, scope_idx, pa, ch, n_sites):
    """(fast-class tasks, rows, chunks) of the CPU plan of this description under the current PGBP_TUNING."""
    lib = P.load()
    desc, keep = L.make_desc(dims, sepcl, scope_off, scope_idx, n_sites, 0)
    pl = C.c_void_p()
    assert lib.pgbp_plan_create(C.byref(desc), C.byref(pl)) == 0, lib.pgbp_plan_last_error(pl)
    off = np.array([0, len(pa)], np.int32)
    assert lib.pgbp_plan_set_schedule(pl, 1, L.i32p(off), L.i32p(pa), L.i32p(ch)) == 0, lib.pgbp_plan_last_error(pl)
    nfast = nrows = nchunks = 0
    for d in (0, 1):
        nl, nt, ne = C.c_int32(), C.c_int32(), C.c_int32()
        assert lib.pgbp_plan_traversal_sizes(pl, 0, d, C.byref(nl), C.byref(nt), C.byref(ne)) == 0
        nf = np.zeros(max(1, nl.value), np.int32)
        assert lib.pgbp_plan_level_nfast(pl, 0, d, L.i32p(nf)) == 0
        nfast += int(nf.sum())
        nr = C.c_int64()
        assert lib.pgbp_plan_rows(pl, 0, d, C.byref(nr), None, None, None) == 0
        nrows += int(nr.value)
        n = C.c_int32()
        assert lib.pgbp_plan_chunks(pl, 0, d, C.byref(n), None, None, None) == 0
        nchunks += int(n.value)
    lib.pgbp_plan_destroy(pl)
    return nfast, nrows, nchunks


def compare(eng, ce_packs, dims, sepcl, scope_off, scope_idx, pa, ch, sched, desc, bad_site=-1):
    """calibrate!(2 iterations) on the device and on the C engine, site by site.  Returns (worst error, failures seen)."""
    got = P.calibrate_(eng, sched, 2, verbose=False)
    worst, nfail = 0.0, 0
    off = M.record_offsets(dims)
    for s, start in enumerate(ce_packs):
        ref = cengine.Engine(dims, sepcl, scope_off, scope_idx, start)
        want = ref.calibrate(pa, ch, 2, return_iscal=True)
        eng.site = s
        r = eng.last_results[s]
        assert (bool(r.succ), bool(r.iscal)) == want, (desc, s, want, (r.succ, r.iscal))
        if not want[0]:
            assert s == bad_site, (desc, s)
            fe, fd, fi = ref.last_failure()
            assert (r.fail_edge, r.fail_dir, r.fail_info) == (fe, fd, fi), (desc, s, (r.fail_edge, r.fail_dir, r.fail_info), (fe, fd, fi))
            assert fi > 1, (desc, fi)
            nfail += 1
            continue
        assert s != bad_site, (desc, "the placed failure did not fail")
        a, b = eng._packed[s], ref.packed()
        for i in range(len(dims)):
            x, y = a[off[i]:off[i + 1]], b[off[i]:off[i + 1]]
            err = float(np.max(np.abs(x - y))) / max(1.0, float(np.max(np.abs(y))))
            worst = max(worst, err)
            assert err <= 1e-8, (desc, s, i, err)
        _, flags = ref.residuals()
        assert np.array_equal(eng._flags().astype(bool), flags.astype(bool)), (desc, s)
    assert got == (bool(eng.last_results[0].succ), bool(eng.last_results[0].iscal))
    return worst, nfail


def run(n_trees, seed):
    rng = np.random.default_rng(seed)
    tuning = os.environ.get("PGBP_TUNING", "")
    worst, nfail, tot_rows, tot_chunks, n_multi, n_big_acc = 0.0, 0, 0, 0, 0, 0
    for t in range(n_trees):
        family = "large" if t == 0 else ("small" if t % 3 else "medium")
        while True:
            dims, sepcl, so, si, pa, ch, depth, ni_of, nc = draw_tree(rng, family)
            if not has_fast_shape(dims, sepcl, so, si, nc):
                break
        ns = int(rng.integers(1, 3))
        off = M.record_offsets(dims)
        packs = []
        for _ in range(ns):
            pk = np.zeros(int(off[-1]))
            for c in range(nc):
                m = int(dims[c])
                pk[off[c]:off[c + 1]] = M.pack_record(M.spd(rng, m), rng.standard_normal(m), rng.standard_normal())
            packs.append(pk)
        nfast, nrows, nchunks = plan_classes(dims, sepcl, so, si, pa, ch, ns)
        assert nfast == 0, (t, family, nfast)
        tot_rows += nrows
        tot_chunks += nchunks
        fan = np.bincount(pa, minlength=nc)
        n_multi += int(np.sum(fan > 1))
        n_big_acc += int(np.sum([fan[c] > 1 and any(dims[x] > 64 for x in ch[pa == c]) for c in range(nc)]))
        sched = [(pa, ch)]
        desc = (t, family, nc, ns, tuning)
        eng = P.ClusterGraphBelief.from_arrays(dims, sepcl, so, si, np.stack(packs), n_sites=ns)
        w, _ = compare(eng, packs, dims, sepcl, so, si, pa, ch, sched, desc)
        worst = max(worst, w)
        del eng
        # one pivot-placed failure at k > 1: a cluster at the leaf end, then one next to the root
        leaves = [c for c in range(1, nc) if fan[c] == 0 and ni_of[c] >= 2]
        leaf = max(leaves, key=lambda c: (depth[c], c))
        near = min((c for c in range(1, nc) if ni_of[c] >= 2), key=lambda c: (depth[c], c))
        for c in (leaf, near):
            e = int(np.nonzero(ch == c)[0][0])
            side = 0 if sepcl[2 * e] == c else 1
            keep = si[so[2 * e + side]:so[2 * e + side + 1]]
            integ = np.setdiff1d(np.arange(dims[c]), keep)
            k = int(rng.integers(2, len(integ) + 1))
            bad_site = int(rng.integers(ns))
            bad = [p.copy() for p in packs]
            J, _, _ = M.unpack_record(bad[bad_site][off[c]:off[c + 1]], int(dims[c]))
            # (scaled: the pivots of the cluster's belief once its children's messages are in stay those of the factor)
            J[np.ix_(integ, integ)] = 4096.0 * M.ldl_failure(rng, len(integ), k, "sign" if c == near or rng.random() < 0.5 else "zero")
            eng = P.ClusterGraphBelief.from_arrays(dims, sepcl, so, si, np.stack(bad), n_sites=ns)
            w, nf = compare(eng, bad, dims, sepcl, so, si, pa, ch, sched, desc + (c, k), bad_site)
            assert nf == 1, desc
            nfail += nf
            del eng
    assert n_multi > 0 and n_big_acc > 0, (n_multi, n_big_acc)
    if "small4_min=0" in tuning:
        assert tot_rows > 0, "no level has a row form: bp_level_small4 did not run"
    if "no_chunks" not in tuning and "no_tail" not in tuning:   # (no_tail: level launches only)
        assert tot_chunks > 0, "the planner fused no levels: the chunk kernels did not run"
    return nfail, worst, tot_rows, tot_chunks


def main():
    n_trees = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    nfail, worst, rows, chunks = run(n_trees, seed)
    print(f"{n_trees} trees ok ({nfail} placed failures reported identically, {rows} rows, {chunks} chunks), "
          f"worst relative belief error {worst:.2e}")


if __name__ == "__main__":
    main()

"""Shapes and plan queries shared by tests/test_plan_leaf_sepset_cpu.py, tests/test_gpu_leaf_sepset.py and
tests/run_leaf_sepset_cases.py: the LEAF SEPSET mark of the planner (pgbp_plan_leaf_sepset: a preorder record into a leaf of
the schedule tree whose postorder message is its whole belief) and the small cluster graphs it is checked on."""
import ctypes as C

import numpy as np

import pgbp_amd
from pgbp_amd import _lib as L
from pgbp_amd import synth as S


def tree_of(kind, ntips, rng):
    if kind == "random":
        return S.random_tree(ntips, rng)
    if kind == "caterpillar":
        return S.caterpillar_tree(ntips, rng)
    return S.random_multifurcating_tree(ntips, int(kind[4:]), rng)


def problem(graph, kind, ntips, p, seed=0):
    """the clique tree / Bethe graph of a synthetic tree, or `edge`: ONE schedule edge -- a 2p-dimensional root cluster and
    a p-dimensional leaf over its second block (the traversal pair turns on it)"""
    if graph == "edge":
        dims = np.array([2 * p, p, p], np.int32)
        prob = S.Problem(dims=dims, sepset_clusters=np.array([[0, 1]], np.int32), scope_off=np.array([0, p, 2 * p], np.int64),
                         scope_idx=np.concatenate([np.arange(p, 2 * p), np.arange(p)]).astype(np.int32),
                         schedule=[(np.array([0], np.int32), np.array([1], np.int32))], nclusters=2, root_cluster=0)
        m = dims.astype(np.int64)
        prob.packed_off = np.concatenate([[0], np.cumsum(m * m + m + 1)])
        return prob
    tr = tree_of(kind, ntips, np.random.default_rng(100 * ntips + p + seed))
    return S.bethe_of_tree(tr, p) if graph == "bethe" else S.cliquetree_of_tree(tr, p)


def tall_leaves_problem(ntips, p, seed=0):
    """a clique tree none of whose clusters drops its child's variables (no node counts as a tip): every leaf cluster holds
    2p variables behind a p-dimensional sepset"""
    tr = S.random_tree(ntips, np.random.default_rng(seed))
    return S.cliquetree_of_tree(S.Tree(tr.parent, tr.length, np.zeros_like(tr.is_leaf)), p)


def generic_star():
    """leaves whose whole belief is the message (3 variables, sepsets of 3) around a 5-variable centre: s == mf and ni == 0,
    but no message has the register-resident kernel's shape (the receiver is neither P nor 2P wide)"""
    dims = np.array([5, 3, 3, 3, 3], np.int32)
    prob = S.Problem(dims=dims, sepset_clusters=np.array([[0, 1], [0, 2]], np.int32),
                     scope_off=np.array([0, 3, 6, 9, 12], np.int64),
                     scope_idx=np.array([0, 1, 2, 0, 1, 2, 2, 3, 4, 0, 1, 2], np.int32),
                     schedule=[(np.array([0, 0], np.int32), np.array([1, 2], np.int32))], nclusters=3, root_cluster=0)
    return prob


def spd_packed(prob, rng):
    """random symmetric positive-definite cluster beliefs in the ABI's packed records, sepsets the constant 1"""
    off = prob.packed_off
    out = np.zeros(int(off[-1]))
    for i in range(prob.nclusters):
        m, o = int(prob.dims[i]), int(off[i])
        A = rng.standard_normal((m, m))
        J = A @ A.T + max(1, m) * np.eye(m)
        out[o:o + m * m] = ((J + J.T) / 2).reshape(-1, order="F")
        out[o + m * m:o + m * m + m] = rng.standard_normal(m)
        out[o + m * m + m] = rng.standard_normal()
    return out


def sepset_of_edge(prob):
    """per schedule edge of tree 0: sepset index k"""
    key = {(int(min(a, b)), int(max(a, b))): k for k, (a, b) in enumerate(np.asarray(prob.sepset_clusters).reshape(-1, 2))}
    pa, ch = prob.schedule[0]
    return [key[(int(min(a, c)), int(max(a, c)))] for a, c in zip(pa, ch)]


def msg_id(prob, k, receiver):
    """directed message over sepset k = (a, b): 2k when a receives"""
    return 2 * k + (0 if int(np.asarray(prob.sepset_clusters).reshape(-1, 2)[k, 0]) == int(receiver) else 1)


def leaf_messages(prob):
    """the preorder messages into the leaves of schedule tree 0 whose postorder message integrates nothing and fills its
    sepset (ni == 0, s == mf), from the description alone"""
    pa, ch = prob.schedule[0]
    senders = set(int(x) for x in pa)
    out = set()
    for i, k in enumerate(sepset_of_edge(prob)):
        c = int(ch[i])
        if c not in senders and int(prob.dims[c]) == int(prob.dims[prob.nclusters + k]):
            out.add(msg_id(prob, k, c))
    return out


def plan_marks(prob, n_sites=1):
    """{direction: (messages of the register-resident records, those marked LEAF SEPSET)} over the level groups, the tail
    and the chunks of the CPU plan under the current PGBP_TUNING; plus the messages of the chunks' records per direction"""
    lib = pgbp_amd.load()
    desc, keep = L.make_desc(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, n_sites, 0)
    pl = C.c_void_p()
    assert lib.pgbp_plan_create(C.byref(desc), C.byref(pl)) == 0, lib.pgbp_plan_last_error(pl)
    pa, ch = prob.schedule[0]
    off = np.array([0, len(pa)], np.int32)
    assert lib.pgbp_plan_set_schedule(pl, 1, L.i32p(off), L.i32p(np.ascontiguousarray(pa, np.int32)),
                                      L.i32p(np.ascontiguousarray(ch, np.int32))) == 0, lib.pgbp_plan_last_error(pl)
    out, in_chunks = {}, {}
    for d in (0, 1):
        nl = C.c_int32()
        assert lib.pgbp_plan_traversal_sizes(pl, 0, d, C.byref(nl), None, None) == 0
        ng = np.zeros(max(1, nl.value), np.int32)
        tl = C.c_int32()
        assert lib.pgbp_plan_groups(pl, 0, d, L.i32p(ng), C.byref(tl), None, None) == 0
        rec = np.zeros((max(1, 4 * int(ng[:nl.value].sum())), 6), np.int32)
        trec = np.zeros((max(1, 8 * tl.value), 6), np.int32)
        assert lib.pgbp_plan_groups(pl, 0, d, None, None, L.i32p(rec), L.i32p(trec)) == 0
        nch = C.c_int32()
        assert lib.pgbp_plan_chunks(pl, 0, d, C.byref(nch), None, None, None) == 0
        info = np.zeros((max(1, nch.value), 4), np.int32)
        assert lib.pgbp_plan_chunks(pl, 0, d, C.byref(nch), L.i32p(info), None, None) == 0
        info = info[:nch.value]
        crec = np.zeros((max(1, 8 * int(np.abs(info[:, 3]).sum())), 6), np.int32)
        assert lib.pgbp_plan_chunks(pl, 0, d, C.byref(nch), None, None, L.i32p(crec)) == 0
        generic = np.repeat(info[:, 3] < 0, 8 * np.abs(info[:, 3])) if len(info) else np.zeros(0, bool)
        lv, tv, cv = (np.zeros(len(x), np.int32) for x in (rec, trec, crec))
        assert lib.pgbp_plan_leaf_sepset(pl, 0, d, L.i32p(lv), L.i32p(tv), L.i32p(cv)) == 0
        msgs, marked = set(), set()
        for r, v, gen in ((rec, lv, None), (trec, tv, None), (crec, cv, generic)):
            for i in range(len(r)):
                if gen is not None and i < len(gen) and gen[i]:
                    assert v[i] == 0, "a chunk of generic-class tasks carries no mark"
                    continue
                if r[i, 0]:
                    msgs.add(int(r[i, 1]))
                    if v[i]:
                        marked.add(int(r[i, 1]))
                else:
                    assert v[i] == 0, "an invalid record carries no mark"
        out[d] = (msgs, marked)
        in_chunks[d] = set(int(crec[i, 1]) for i in range(len(crec)) if crec[i, 0] and not (i < len(generic) and generic[i]))
    lib.pgbp_plan_destroy(pl)
    return out, in_chunks

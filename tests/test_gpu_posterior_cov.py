"""pgbp_posterior_cov: exact posterior covariances between any two entries of the sampler's layout, one device call.

The device is compared with tests/cov_ref.py (the numpy restatement of the header's two recurrences, pinned to the dense
oracle in test_posterior_cov_cpu.py) on the beliefs read back from the device; the law itself is checked through the device
against oracle.densemvn.posterior_node_moments with c = I_D, on every pair of entries.  Every comparison is asserted at 1e-8
relative to the largest entry of its reference, the project's parity bound, and prints its measured figure first.  The
calibrated states are built with the helpers of test_gpu_sample.py; "the 6-tip, 2-trait tree" is that file's (seed 31).
Measured on the MI355X: device against the restatement w <= 4.3e-16, k <= 9.9e-16 over every case (largest at 128 variables);
the law through the device k <= 1.3e-15, node_cov <= 1.4e-15, the joint means <= 7.1e-16, functional_moments <= 9.8e-16; k
inside a cluster against moments_ 3.5e-16, k against its transpose 3.4e-17; packed against plain layout 0 (the same bytes)."""
import ctypes as C
import os

import numpy as np
import pytest

from cov_ref import posterior_cov_ref
from helpers import goldens, make_model
from oracle import densemvn as OD
from oracle import network as ON
from sample_ref import variable_nodes
from test_gpu_sample import (P, _bits, _bm, _err, _f64, _golden_cliquetree, _oracle_cliquetree, _raw, _records,  # noqa: F401
                             _set_record, _size, _synth_tree)

pytestmark = pytest.mark.gpu
G = goldens()
BOUND = 1e-8


# ----------------------------------------------------------------------------- raw calls

def _cov(cgb, tree, s0, s1, c, n_cols=None, w=None, k=None, info=None, null_c=False, want_w=True, want_k=True):
    """The C call itself: (status, w, k [n_cols, s1 - s0, size], info [s1 - s0]); the canvases start at -7 and -3."""
    c = np.ascontiguousarray(np.atleast_2d(c), dtype=np.float64)
    n_cols = c.shape[0] if n_cols is None else n_cols
    ns = max(s1 - s0, 1)
    shape = (max(n_cols, 1), ns, _size(cgb))
    w = np.full(shape, -7.0) if w is None else w
    k = np.full(shape, -7.0) if k is None else k
    info = np.full(ns, -3, dtype=np.int32) if info is None else info
    rc = cgb._lib.pgbp_posterior_cov(cgb._eng, tree, s0, s1, n_cols, None if null_c else _f64(c), _f64(w) if want_w else None,
                                     _f64(k) if want_k else None, info.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, w, k, info


def _ref(cgb, sched, c, site=0):
    """the restatement on the device's own beliefs of one site: (w, k, info)"""
    return posterior_cov_ref(_records(cgb, site), cgb._dims, cgb._sepcl, cgb._scope_off, cgb._scope_idx, sched[-2], sched[-1], c)


def _rel(got, want):
    return float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1e-300))


def _columns(cgb, seed=13):
    """5 random columns and one unit column"""
    D = _size(cgb)
    c = np.random.default_rng(seed).standard_normal((6, D))
    c[5] = 0.0
    c[5, D // 2] = 1.0
    return c


def _assert_device_is_restatement(cgb, sched, name, sites=(0,), n_sites=1):
    c = _columns(cgb)
    rc, w, k, info = _cov(cgb, 0, 0, n_sites, c)
    assert rc == 0, _err(cgb)
    assert not info.any()
    ew = ek = 0.0
    for s in sites:
        ww, wk, winfo = _ref(cgb, sched, c, site=s)
        assert winfo == 0
        ew, ek = max(ew, _rel(w[:, s], ww)), max(ek, _rel(k[:, s], wk))
    print(f"{name}: size {_size(cgb)}, largest cluster {int(cgb._dims[:cgb.nclusters].max())}, device vs restatement "
          f"w {ew:.2e}, k {ek:.2e}")
    assert ew <= BOUND and ek <= BOUND, (name, ew, ek)
    return c, w, k


def _distinct_sites(cgb):
    """The posterior covariance of a Gaussian model does not depend on the data, so the sites of a batch that share their
    parameters share w and k.  Site s gets every cluster's J scaled by 1 + s / 4 (a calibrated clique tree stays one: every
    marginal is scaled alike), which makes a mix-up of sites visible."""
    for s in range(1, cgb.n_sites):
        for b, (J, h) in enumerate(_records(cgb, s)):
            _set_record(cgb, s, b, (1.0 + s / 4.0) * J, h)


def _s_entries(cgb, sched):
    """the entries of the layout at S positions of non-root clusters"""
    off = np.concatenate([[0], np.cumsum(cgb._dims[: cgb.nclusters].astype(np.int64))])
    out = []
    for pa, ch in zip(sched[-2], sched[-1]):
        kk = next(q for q in range(cgb.nsepsets) if set(int(v) for v in cgb._sepcl[q]) == {int(pa), int(ch)})
        side = 0 if int(cgb._sepcl[kk][0]) == int(ch) else 1
        out += [int(off[int(ch)] + v) for v in cgb._scope_idx[cgb._scope_off[2 * kk + side]: cgb._scope_off[2 * kk + side + 1]]]
    return np.array(out, dtype=int)


# ----------------------------------------------------------------------------- device against the restatement

@pytest.mark.parametrize("p,ntips", [(1, 6), (8, 5), (24, 5), (40, 4), (64, 4)])
def test_cov_random_trees_all_classes(P, p, ntips):
    """Clusters of p and 2p variables at the smallest sizes that reach each class of the factor phase (2 and 16; 48; 80 and
    128 variables); in a binary tree both children of a node map their sepsets to the same parent variables, so every gather
    list with two children is exercised.  w is +0.0, sign included, at the entries the sampler conditions on."""
    prob, cgb = _synth_tree(P, ntips, p, 300 + p)
    sched = prob.schedule[0]
    assert int(cgb._dims[: cgb.nclusters].max()) == 2 * p
    assert max(np.bincount(np.asarray(sched[-2], dtype=int))) >= 2          # siblings
    c, w, k = _assert_device_is_restatement(cgb, sched, f"tree p={p}")
    S = _s_entries(cgb, sched)
    assert len(S) >= p and not _bits(w[:, :, S]).any()


def test_cov_ragged_cliquetree_golden(P):
    *_, pcgb, spt = _golden_cliquetree(P, "calibration_cliquetree_level1", ["y"])
    _assert_device_is_restatement(pcgb, spt, "golden level-1 clique tree")


def test_cov_missing_data_tree_dimension_zero_sepset(P):
    *_, pcgb, spt = _golden_cliquetree(P, "calibration_tree_2traits_missing", ["y1", "y2"])
    assert 0 in [int(d) for d in pcgb._dims[pcgb.nclusters:]]
    _assert_device_is_restatement(pcgb, spt, "golden missing-data tree")


def test_cov_level3_network_cliquetree(P):
    """The clique tree of test_gpu_sample.py's level-3 network (12 tips, 2 blobs, p = 2): sepsets that hold several nodes,
    parents with more than two children; a cluster that lies wholly inside the sepset to its parent (r = 0) is covered if the
    graph has one (printed)."""
    rng = np.random.default_rng(21)
    net = ON.random_level3_network(12, 2, rng)
    taxa = net.tip_names
    tbl = [list(rng.normal(size=len(taxa))) for _ in range(2)]
    ocgb, pcgb, spt = _oracle_cliquetree(P, net, _bm(2, rng, 0.6 * np.eye(2)), tbl, taxa)
    _assert_device_is_restatement(pcgb, spt, "level-3 network clique tree")
    n_r0 = 0
    for pa, ch in zip(spt[-2], spt[-1]):
        kk = next(q for q in range(pcgb.nsepsets) if set(int(v) for v in pcgb._sepcl[q]) == {int(pa), int(ch)})
        n_r0 += int(pcgb._dims[pcgb.nclusters + kk]) == int(pcgb._dims[int(ch)])
    print(f"level-3 network clique tree: {n_r0} clusters with r = 0")


# ----------------------------------------------------------------------------- the law, through the device

def _law_inputs(name):
    if name.startswith("tree6"):
        rng = np.random.default_rng(31)
        net = ON.random_network(6, 0, rng)
        tbl = [list(rng.normal(size=6)) for _ in range(2)]
        return net, _bm(2, rng, 0.8 * np.eye(2) if name.endswith("random_root") else None), tbl, net.tip_names
    g = G["canonicalform_six_messages"]
    md = dict(g["model"])
    if name.endswith("random_root"):
        md["v"] = 0.8
    return ON.read_newick(g["net"]), make_model(md), [g["y"]], g["taxa"]


@pytest.fixture(scope="module", params=["tree6_fixed_root", "tree6_random_root", "level1_fixed_root", "level1_random_root"])
def law(request, P):
    """one calibrated case: the labelled device object, the dense posterior moments, and the call with c = I_D (computed once)"""
    net, model, tbl, taxa = _law_inputs(request.param)
    ocgb, pcgb, spt = _oracle_cliquetree(P, net, model, tbl, taxa)
    D = _size(pcgb)
    vn = variable_nodes(ocgb.belief, ocgb.nclusters)
    assert len(vn) == D
    pm, pc = OD.posterior_node_moments(net, model, tbl, taxa)
    rc, w, k, info = _cov(pcgb, 0, 0, 1, np.eye(D))
    assert rc == 0 and info[0] == 0, _err(pcgb)
    p = model.dimension()
    flat = np.array([n * p + t for n, t in vn], dtype=int)
    return dict(name=request.param, net=net, cgb=pcgb, D=D, vn=vn, p=p, pm=pm, pc=pc, flat=flat, w=w[:, 0], k=k[:, 0])


def test_cov_law_k_is_the_dense_covariance_on_every_pair(law):
    want = law["pc"][np.ix_(law["flat"], law["flat"])]
    ek, eww = _rel(law["k"], want), _rel(law["w"] @ law["w"].T, want)
    print(f"{law['name']}: D = {law['D']}, k against the dense covariance {ek:.2e}, w w' {eww:.2e}")
    assert ek <= BOUND and eww <= BOUND


def _labels(law):
    """the node labels the clusters hold (label = 1 + the preorder index), and per label the traits in scope"""
    insc = {}
    for n, t in law["vn"]:
        insc.setdefault(n + 1, set()).add(t)
    return sorted(insc), insc


def test_cov_law_node_cov_and_joint_posterior_of_all_internal_nodes(law):
    cgb, p, pm, pc = law["cgb"], law["p"], law["pm"], law["pc"]
    labels, insc = _labels(law)
    for lab in labels:
        for t in range(p):
            e = cgb.sample_index(lab, t)
            assert (e >= 0) == (t in insc[lab]) and (e < 0 or law["vn"][e] == (lab - 1, t))
    blocks = cgb.node_cov(labels)
    mean, cov = cgb.nodes_joint_posterior(labels)
    n = len(labels)
    assert blocks.shape == (n, n, p, p) and mean.shape == (n, p) and cov.shape == (n * p, n * p)
    flat = np.array([(lab - 1) * p + t for lab in labels for t in range(p)])
    mask = np.array([t in insc[lab] for lab in labels for t in range(p)])
    want_c, want_m = pc[np.ix_(flat, flat)], pm[flat]
    assert np.all(np.isnan(cov[~mask])) and np.all(np.isnan(cov[:, ~mask])) and np.all(np.isnan(mean.reshape(-1)[~mask]))
    ec = _rel(cov[np.ix_(mask, mask)], want_c[np.ix_(mask, mask)])
    em = _rel(mean.reshape(-1)[mask], want_m[mask])
    print(f"{law['name']}: {n} nodes, joint covariance {ec:.2e}, mean {em:.2e}")
    assert ec <= BOUND and em <= BOUND
    assert np.array_equal(_bits(blocks.transpose(0, 2, 1, 3).reshape(n * p, n * p)[np.ix_(mask, mask)]), _bits(cov[np.ix_(mask, mask)]))
    # two lists: the blocks of the first against the second
    ab = cgb.node_cov(labels[:2], labels[1:])
    assert ab.shape == (2, n - 1, p, p)
    got = ab.transpose(0, 2, 1, 3).reshape(2 * p, (n - 1) * p)
    e2 = _rel(got[np.ix_(mask[: 2 * p], mask[p:])], want_c[: 2 * p, p:][np.ix_(mask[: 2 * p], mask[p:])])
    print(f"{law['name']}: node_cov of two lists {e2:.2e}")
    assert e2 <= BOUND


def test_cov_law_functional_moments_clade_mean_and_contrast(law):
    cgb, p, pm, pc, net = law["cgb"], law["p"], law["pm"], law["pc"], law["net"]
    labels, insc = _labels(law)
    full = [lab for lab in labels if len(insc[lab]) == p]
    index = {id(nd): i for i, nd in enumerate(net.vec_node)}

    def below(i):
        out, stack = set(), [net.vec_node[i]]
        while stack:
            nd = stack.pop()
            out.add(index[id(nd)] + 1)
            stack += net.children(nd)
        return out
    clades = [sorted(below(lab - 1) & set(full)) for lab in full]
    clade = max((cl for cl in clades if len(cl) < len(full)), key=len)
    assert len(clade) >= 2
    a, b = full[0], full[-1]
    # q = 2 p functionals: per trait the mean over the clade's internal nodes, then per trait x_a - x_b
    weights = {}
    for v in set(clade) | {a, b}:
        W = np.zeros((2 * p, p))
        if v in clade:
            W[:p] = np.eye(p) / len(clade)
        W[p:] += (v == a) * np.eye(p) - (v == b) * np.eye(p)
        weights[v] = W
    Cm = np.zeros((2 * p, len(pm)))
    for v, W in weights.items():
        Cm[:, (v - 1) * p: v * p] = W
    mean, cov = cgb.functional_moments(weights)
    ec, em = _rel(cov, Cm @ pc @ Cm.T), _rel(mean, Cm @ pm)
    print(f"{law['name']}: clade of {len(clade)} nodes and the contrast {a} - {b}: covariance {ec:.2e}, mean {em:.2e}")
    assert ec <= BOUND and em <= BOUND


# ----------------------------------------------------------------------------- consistency

def test_cov_unit_columns_against_moments_symmetry_and_copies(P):
    prob, cgb = _synth_tree(P, 7, 3, 41)
    D, nc = _size(cgb), cgb.nclusters
    rc, w, k, info = _cov(cgb, 0, 0, 1, np.eye(D))
    assert rc == 0 and info[0] == 0, _err(cgb)
    K = k[:, 0]
    off = np.concatenate([[0], np.cumsum(cgb._dims[:nc].astype(np.int64))])
    # k of a unit column at the entries of its own cluster = that column of moments_' Sigma
    worst = 0.0
    for b, (mu, Sig, norm) in enumerate(cgb.moments_()):
        worst = max(worst, _rel(K[off[b]: off[b + 1], off[b]: off[b + 1]], Sig))
    esym = _rel(K, K.T)
    print(f"k within a cluster against moments_ {worst:.2e}, k against its transpose {esym:.2e}")
    assert worst <= BOUND and esym <= BOUND
    # a variable that several clusters hold: the same bits of k in every copy, in every column
    n_shared = 0
    for q, (a, b) in enumerate(cgb._sepcl):
        ia = cgb._scope_idx[cgb._scope_off[2 * q]: cgb._scope_off[2 * q + 1]]
        ib = cgb._scope_idx[cgb._scope_off[2 * q + 1]: cgb._scope_off[2 * q + 2]]
        assert np.array_equal(_bits(K[:, off[a] + ia]), _bits(K[:, off[b] + ib])), q
        n_shared += len(ia)
    assert n_shared >= 9


# ----------------------------------------------------------------------------- equal bytes

def test_cov_equal_bytes_calls_ranges_chunks(P):
    prob, cgb = _synth_tree(P, 7, 3, 41, n_sites=3)
    _distinct_sites(cgb)
    c = _columns(cgb)
    rc, w, k, info = _cov(cgb, 0, 0, 3, c)
    assert rc == 0 and not info.any(), _err(cgb)
    assert not np.array_equal(k[:, 0], k[:, 1]) and not np.array_equal(k[:, 1], k[:, 2])
    assert _rel(k[:, 1], _ref(cgb, prob.schedule[0], c, site=1)[1]) <= BOUND
    rc, w2, k2, _ = _cov(cgb, 0, 0, 3, c)
    assert rc == 0 and np.array_equal(_bits(w), _bits(w2)) and np.array_equal(_bits(k), _bits(k2))
    # one site range against two half ranges
    rc, wa, ka, ia = _cov(cgb, 0, 0, 1, c)
    assert rc == 0 and ia.tolist() == [0]
    rc, wb, kb, ib = _cov(cgb, 0, 1, 3, c)
    assert rc == 0 and ib.tolist() == [0, 0]
    assert np.array_equal(_bits(np.concatenate([wa, wb], axis=1)), _bits(w))
    assert np.array_equal(_bits(np.concatenate([ka, kb], axis=1)), _bits(k))
    # every column its own chunk, every site its own factor chunk (strided copies of w and k)
    cgb._lib.pgbp_sample_scratch_limits(1, _size(cgb))
    try:
        rc, wc, kc, ic = _cov(cgb, 0, 0, 3, c)
    finally:
        cgb._lib.pgbp_sample_scratch_limits(0, 0)
    assert rc == 0 and not ic.any() and np.array_equal(_bits(wc), _bits(w)) and np.array_equal(_bits(kc), _bits(k))
    # only w, only k: the same bytes, the other canvas untouched
    rc, w3, k3, _ = _cov(cgb, 0, 0, 3, c, want_k=False)
    assert rc == 0 and np.array_equal(_bits(w3), _bits(w)) and np.all(k3 == -7.0)
    rc, w4, k4, _ = _cov(cgb, 0, 0, 3, c, want_w=False)
    assert rc == 0 and np.array_equal(_bits(k4), _bits(k)) and np.all(w4 == -7.0)
    # a column's bytes do not depend on the other columns of the call
    rc, w5, k5, _ = _cov(cgb, 0, 0, 3, c[2:3])
    assert rc == 0 and np.array_equal(_bits(w5[0]), _bits(w[2])) and np.array_equal(_bits(k5[0]), _bits(k[2]))


def test_cov_packed_layout_against_plain(P):
    """A tree with p = 16 is in the packed (BS16) layout after a calibration; the same beliefs converted to the plain layout
    (pgbp_get_belief converts) give the same bytes: both gathers read the same values, and the arithmetic is the same."""
    prob, cgb = _synth_tree(P, 8, 16, 51)
    assert cgb._lib.pgbp_layout(cgb._eng) == 1, "the p = 16 tree is expected in the packed layout after a calibration"
    c = _columns(cgb)
    rc, wp, kp, info = _cov(cgb, 0, 0, 1, c)
    assert rc == 0 and info[0] == 0, _err(cgb)
    assert cgb._lib.pgbp_layout(cgb._eng) == 1                  # (the call reads the packed records as they are)
    ww, wk, _ = _ref(cgb, prob.schedule[0], c)                  # (pgbp_get_belief: the engine is in the plain layout now)
    assert cgb._lib.pgbp_layout(cgb._eng) == 0
    rc, wq, kq, info = _cov(cgb, 0, 0, 1, c)
    assert rc == 0 and info[0] == 0
    ew, ek = _rel(wp[:, 0], ww), _rel(kp[:, 0], wk)
    print(f"packed vs plain layout: w {_rel(wp, wq):.2e}, k {_rel(kp, kq):.2e}; packed vs restatement w {ew:.2e}, k {ek:.2e}")
    assert np.array_equal(_bits(wp), _bits(wq)) and np.array_equal(_bits(kp), _bits(kq))
    assert ew <= BOUND and ek <= BOUND


def test_cov_site_minor_univariate_batch(P):
    """A univariate batch (p = 1, 64 sites) lives in the site-minor layout after a calibration: the call converts to the plain
    layout first, as the sampler, and the engine goes on working afterwards."""
    prob, cgb = _synth_tree(P, 9, 1, 77, n_sites=64)
    assert P.calibrate_(cgb, prob.schedule, 1, sync=False)[0]
    assert cgb._lib.pgbp_layout(cgb._eng) & 2, "a univariate batch is expected in the site-minor layout after a calibration"
    _assert_device_is_restatement(cgb, prob.schedule[0], "site-minor batch", sites=(0, 17, 63), n_sites=64)
    assert P.calibrate_(cgb, prob.schedule, 1)[0]


# ----------------------------------------------------------------------------- failure

def test_cov_indefinite_cluster_of_one_site(P):
    """One cluster of one site indefinite in its R block: info is what pgbp_sample_posterior reports, that site's w and k are
    NaN, the other sites keep the bytes of a call without the bad site."""
    prob, cgb = _synth_tree(P, 7, 3, 61, n_sites=3)
    _distinct_sites(cgb)
    c = _columns(cgb)
    rc, w0, k0, info = _cov(cgb, 0, 0, 3, c)
    assert rc == 0 and not info.any()
    pa, ch = prob.schedule[0][-2], prob.schedule[0][-1]
    bad = next(int(q) for q in ch if int(cgb._dims[int(q)]) == 6)
    kk = next(q for q in range(cgb.nsepsets) if bad in cgb._sepcl[q] and int(pa[list(ch).index(bad)]) in cgb._sepcl[q])
    side = 0 if cgb._sepcl[kk][0] == bad else 1
    S = set(cgb._scope_idx[cgb._scope_off[2 * kk + side]: cgb._scope_off[2 * kk + side + 1]].tolist())
    R = [v for v in range(6) if v not in S]
    J, h = _records(cgb, 1)[bad]
    J[R[1], R[1]] = -1.0                                            # the second pivot of J_RR is negative
    _set_record(cgb, 1, bad, J, h)
    rc, w, k, info = _cov(cgb, 0, 0, 3, c)
    assert rc == 0, _err(cgb)
    rc, _, sinfo = _raw(cgb, 0, 0, 3, 1, np.zeros((1, 3, _size(cgb))))
    assert rc == 0 and info.tolist() == sinfo.tolist() == [0, bad + 1, 0]
    assert np.all(np.isnan(w[:, 1])) and np.all(np.isnan(k[:, 1]))
    assert np.array_equal(_bits(w[:, [0, 2]]), _bits(w0[:, [0, 2]])) and np.array_equal(_bits(k[:, [0, 2]]), _bits(k0[:, [0, 2]]))
    rc, wa, ka, _ = _cov(cgb, 0, 0, 1, c)
    rc2, wb, kb, _ = _cov(cgb, 0, 2, 3, c)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(_bits(k[:, 0]), _bits(ka[:, 0])) and np.array_equal(_bits(k[:, 2]), _bits(kb[:, 0]))
    assert np.array_equal(_bits(w[:, 0]), _bits(wa[:, 0])) and np.array_equal(_bits(w[:, 2]), _bits(wb[:, 0]))
    assert _ref(cgb, prob.schedule[0], c, site=1)[2] == bad + 1


# ----------------------------------------------------------------------------- refusals

def test_cov_refusals(P):
    prob, cgb = _synth_tree(P, 6, 2, 71, n_sites=2)
    D = _size(cgb)
    c = np.zeros((1, D))
    wc, kc, ic = np.full((1, 2, D), 9.0), np.full((1, 2, D), 9.0), np.full(2, 5, dtype=np.int32)
    for (tree, s0, s1, n_cols), word in (((5, 0, 2, 1), b"tree 5"), ((-1, 0, 2, 1), b"tree -1"), ((0, 0, 2, 0), b"n_cols = 0"),
                                         ((0, 0, 2, -2), b"n_cols = -2"), ((0, -1, 2, 1), b"site range"),
                                         ((0, 2, 1, 1), b"site range"), ((0, 0, 3, 1), b"site range")):
        rc, _, _, _ = _cov(cgb, tree, s0, s1, c, n_cols=n_cols, w=wc, k=kc, info=ic)
        assert rc == 1 and word in _err(cgb) and _err(cgb).startswith(b"pgbp_posterior_cov: "), ((tree, s0, s1, n_cols), _err(cgb))
    rc, _, _, _ = _cov(cgb, 0, 0, 2, c, w=wc, k=kc, info=ic, null_c=True)
    assert rc == 1 and b"pgbp_posterior_cov: no input buffer c" in _err(cgb)
    rc, _, _, _ = _cov(cgb, 0, 0, 2, c, w=wc, k=kc, info=ic, want_w=False, want_k=False)
    assert rc == 1 and b"w and k are both NULL" in _err(cgb)
    assert np.all(wc == 9.0) and np.all(kc == 9.0) and np.all(ic == 5)
    with pytest.raises(P.PgbpError):
        cgb.posterior_cov_(c, schedule_tree=3)
    with pytest.raises(ValueError):
        cgb.posterior_cov_(np.zeros((1, D + 1)))
    # no schedule set
    _, fresh = _synth_tree(P, 6, 2, 71, calibrate=False)
    rc, w, k, info = _cov(fresh, 0, 0, 1, c)
    assert rc == 6 and b"pgbp_posterior_cov: no schedule" in _err(fresh)
    assert np.all(w == -7.0) and np.all(k == -7.0) and np.all(info == -3)


def test_cov_refuses_a_bethe_graph(P):
    g = G["joingraph_mateescu"]
    net, names = P.read_newick(g["net"])
    cn, ed, sn = P.bethe(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, 2)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.set_schedule(P.spanningtrees_clusterlist(len(cn), ed, cn, net.is_leaf))
    rc, w, k, info = _cov(cgb, 0, 0, 1, np.zeros((1, _size(cgb))))
    assert rc == 1 and b"pgbp_posterior_cov: " in _err(cgb) and b"clique tree only" in _err(cgb)
    assert np.all(w == -7.0) and np.all(k == -7.0) and np.all(info == -3)


def test_cov_refuses_muller_cliquetree_three_traits(P):
    """The clique tree of the Mueller et al. network at 3 traits has a cluster of 162 variables: refused as the sampler does."""
    from helpers import network_from_newick_file
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "muller_2022.phy")
    net, names, _, _ = network_from_newick_file(P, path)
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, 3)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.set_schedule([P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))])
    big = next(b for b in range(cgb.nclusters) if int(cgb._dims[b]) > 128)
    D = _size(cgb)
    rc, w, k, info = _cov(cgb, 0, 0, 1, np.zeros((1, D)))
    msg = _err(cgb).decode()
    assert rc == 1 and msg.startswith("pgbp_posterior_cov: ")
    assert f"belief {big} has {int(cgb._dims[big])} variables, more than the 128" in msg
    assert np.all(w == -7.0) and np.all(k == -7.0)
    rc, x, _ = _raw(cgb, 0, 0, 1, 1, np.zeros((1, 1, D)))
    assert rc == 1 and _err(cgb).decode() == msg.replace("pgbp_posterior_cov", "pgbp_sample_posterior")


# ----------------------------------------------------------------------------- the host mirror

def test_cov_wrappers(P):
    prob, cgb = _synth_tree(P, 7, 3, 41, n_sites=3)
    _distinct_sites(cgb)
    c = _columns(cgb)
    rc, w, k, info = _cov(cgb, 0, 0, 3, c)
    assert rc == 0
    w1, k1, i1 = cgb.posterior_cov_(c, all_sites=True)
    assert np.array_equal(_bits(w1), _bits(w)) and np.array_equal(_bits(k1), _bits(k)) and i1.tolist() == info.tolist()
    w2, k2, i2 = cgb.posterior_cov_(c[0], want_w=False)
    assert w2 is None and k2.shape == (1, 1, _size(cgb)) and np.array_equal(_bits(k2[0, 0]), _bits(k[0, cgb.site])) and i2.tolist() == [0]
    w3, k3, _ = cgb.posterior_cov_(c, want_k=False)
    assert k3 is None and np.array_equal(_bits(w3[:, 0]), _bits(w[:, cgb.site]))
    # the node-level helpers need labelled beliefs
    for call in (lambda: cgb.sample_index(1, 0), lambda: cgb.node_cov([1, 2]), lambda: cgb.nodes_joint_posterior([1, 2]),
                 lambda: cgb.functional_moments({1: np.ones((1, 3))})):
        with pytest.raises(ValueError, match="labelled beliefs"):
            call()

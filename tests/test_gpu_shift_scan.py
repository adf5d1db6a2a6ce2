"""The scan of every edge for a mean shift on the device: pgbp_lg_shift_scan / shift_scan_lg / loglik_and_shift_scan_lg
(csrc/pgbp_scan.hip) and the forward selection select_shifts_lg.

Comparators: scan_ref.family_scan on the dense oracle's posterior moments of the shift_ref.ShiftedModel wrapper (pinned to
one-edge dense GLS and to the dense log-likelihood in test_shift_scan_cpu.py), scan_ref.gls_edge itself, the device's own
exact one-edge fit fit_shifts_lg (pinned to dense GLS in test_gpu_shifts.py), and scan_ref.dense_greedy for the selection.
Every comparison at 1e-8 relative to the largest entry of the block (rel_block); the measured figures are printed."""
import numpy as np
import pytest

import impute_ref as IR
import loo_ref as LR
import scan_ref as SR
from edge_ref import rel_block_nan
from helpers import lg_inputs_from_oracle
from oracle import densemvn as OD
from oracle import network as ON
from shift_ref import ShiftedModel, family_edge, family_nodes, family_of_edge, fit_edges, tips_below
from test_gpu_shifts import _device, _tree_batch, _tree_case
from test_gradient_cpu import rel_block
from test_shift_cpu import CASES, IDS, moved_data

pytestmark = pytest.mark.gpu
TOL = 1e-8
DENSE = [c for c in CASES if not c[0].startswith("missing")]
DENSE_IDS = [c[0] for c in DENSE]
BLOCKS = ("jump", "lr", "H", "edge_jump", "se")


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _se_of(H, identified):
    se = np.full(identified.shape, np.nan)
    for f in range(len(H)):
        ks = np.flatnonzero(identified[f])
        if ks.size:
            se[f, ks] = np.sqrt(np.diag(np.linalg.inv(H[f][np.ix_(ks, ks)])))
    return se


def _assert_scan(tag, got, want):
    """got: a site of shift_scan_lg(information=True); want: scan_ref.device_layout.  The kept traits must be the same;
    every block at 1e-8 relative to its largest entry, the NaN patterns equal."""
    assert np.array_equal(got["identified"], want["identified"]), tag
    assert np.array_equal(got["dof"], want["identified"].sum(axis=1)), tag
    want = dict(want, se=_se_of(want["H"], want["identified"]))
    worst = {k: rel_block_nan(got[k], want[k]) for k in BLOCKS}
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (tag, k, v)
    assert _same(got["H"], got["H"].transpose(0, 2, 1))
    return worst


def _check_dense(P, tag, net, model, tbl, taxa, min_info=1e-8):
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa, oracle_factors=False)
    ll, got = pcgb.loglik_and_shift_scan_lg(spt, min_info=min_info, information=True)
    dense = OD.loglik(net, model, tbl, taxa)
    assert abs(ll - dense) <= TOL * max(1.0, abs(dense)), (tag, ll, dense)
    sc = SR.dense_scan(net, model, {}, tbl, taxa, min_info)
    _assert_scan(tag, got, SR.device_layout(sc, net, ocgb, fam))
    return pcgb, spt, fam, ocgb, got, sc


# ----------------------------------------------------------------------------- 1: the reference statement

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scan_against_the_dense_statement(P, case):
    """The six dense cases and the two missing-data cases on the clique tree.  A root-prior family is all NaN with nothing
    identified; the missing-data cases hold families with exactly one identified trait."""
    name, net, model, tbl, taxa = case
    pcgb, spt, fam, ocgb, got, sc = _check_dense(P, name, net, model, tbl, taxa)
    for f in np.flatnonzero(np.asarray(fam["n_parents"]) == 0):
        assert np.isnan(got["lr"][f]) and np.isnan(got["jump"][f]).all() and not got["identified"][f].any()
    if name.startswith("missing"):
        assert (got["dof"][np.asarray(fam["n_parents"]) > 0] == 1).any()
    # both parent edges of a hybrid: the family's lr, jumps in the ratio of their gamma
    K = int(fam["max_parents"])
    gam = np.asarray(fam["gamma"]).reshape(-1, K)
    hyb = np.flatnonzero(np.asarray(fam["n_parents"]) == 2)
    assert hyb.size
    for f in hyb:
        assert rel_block_nan(got["edge_jump"][f, 0] * gam[f, 0], got["edge_jump"][f, 1] * gam[f, 1]) <= 1e-14


@pytest.mark.parametrize("root", ["fixed", "random", "improper"])
def test_scan_roots_of_level1_2traits(P, root):
    """The reference's level-1 network at two traits.  Fixed and proper random root against the dense statement; under the
    improper root (no dense posterior) against the device's single-edge fit_shifts_lg on four edges: shift, H, gain."""
    net, model, tbl, taxa = LR.reference_case("level1_2traits", root)
    if root != "improper":
        _check_dense(P, f"level1_2traits/{root}", net, model, tbl, taxa)
        return
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    ll0, got = pcgb.loglik_and_shift_scan_lg(spt, information=True)
    K, p = int(fam["max_parents"]), model.dimension()
    gam = np.asarray(fam["gamma"]).reshape(-1, K)
    full = np.flatnonzero((got["dof"] == p) & (np.asarray(fam["n_parents"]) >= 1))
    hyb = [f for f in full if fam["n_parents"][f] == 2]
    picks = [(int(full[0]), 0), (int(full[len(full) // 2]), 0), (int(full[-1]), 0), (int(hyb[0]), 1)]
    assert len(set(picks)) == 4
    worst = {}
    for f, k in picks:
        fit = P.fit_shifts_lg(pcgb, spt, [(f, k)])
        e = dict(shift=rel_block(got["edge_jump"][f, k], fit["shifts"][0]), H=rel_block(gam[f, k] ** 2 * got["H"][f], fit["H"]),
                 gain=abs(got["lr"][f] - 2.0 * (fit["loglik"] - ll0)) / max(abs(got["lr"][f]), 1.0),
                 se=rel_block(got["se"][f] / abs(gam[f, k]), fit["se"][0]))
        for q, v in e.items():
            worst[q] = max(worst.get(q, 0.0), v)
    print("level1_2traits/improper, four edges vs fit_shifts_lg: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (k, v)


# ----------------------------------------------------------------------------- 2: edge fits, shifts in force

@pytest.mark.parametrize("case", DENSE, ids=DENSE_IDS)
def test_scan_against_single_edge_fits(P, case):
    """On shift_ref.fit_edges (three tree edges, one hybrid edge) and the hybrid's other parent edge: the scan at zero shifts
    against fit_shifts_lg of each edge alone.  Then, with the first edge's fit in force: that edge's lr is at most 1e-8 of its
    value at zero shifts, and another edge's scan is the dense conditional fit (scan_ref.gls_edge, the first shift held)."""
    name, net, model, tbl, taxa = case
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa, oracle_factors=False)
    K = int(fam["max_parents"])
    gam = np.asarray(fam["gamma"]).reshape(-1, K)
    oe = fit_edges(net, model)
    edges = [family_of_edge(net, ocgb, fam, ed) for ed in oe]
    fh, kh = edges[3]
    edges.append((fh, 1 - kh))
    ll0, got = pcgb.loglik_and_shift_scan_lg(spt, information=True)
    assert got["lr"][fh] > 0 and gam[fh, 0] != gam[fh, 1]
    worst = {}
    fits = []
    for f, k in edges:
        fit = P.fit_shifts_lg(pcgb, spt, [(f, k)])
        fits.append(fit)
        e = dict(shift=rel_block(got["edge_jump"][f, k], fit["shifts"][0]), H=rel_block(gam[f, k] ** 2 * got["H"][f], fit["H"]),
                 gain=abs(got["lr"][f] - 2.0 * (fit["loglik"] - ll0)) / max(abs(got["lr"][f]), 1.0))
        for q, v in e.items():
            worst[q] = max(worst.get(q, 0.0), v)
    # the two parent edges of the hybrid: equal gain, shifts in the inverse ratio of their gamma
    worst["hybrid_ratio"] = rel_block(fits[3]["shifts"][0] * gam[fh, kh], fits[4]["shifts"][0] * gam[fh, 1 - kh])
    worst["hybrid_gain"] = abs(fits[3]["loglik"] - fits[4]["loglik"]) / abs(fits[3]["loglik"])
    print(f"{name}, five edges vs fit_shifts_lg: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (k, v)
    # shifts in force
    f0, k0 = edges[0]
    fit = P.fit_shifts_lg(pcgb, spt, [(f0, k0)])       # (leaves the engine at the fit, calibrated)
    held = {int(oe[0].number): fit["shifts"][0]}
    after = pcgb.shift_scan_lg(information=True)
    print(f"{name}: lr of the fitted edge {after['lr'][f0]:.3e} (at zero shifts {got['lr'][f0]:.3e})")
    assert after["lr"][f0] <= TOL * got["lr"][f0]
    f2, k2 = edges[2]
    inc, H, ll1, llh = SR.gls_edge(net, model, tbl, taxa, oe[2], range(model.dimension()), held)
    e = dict(increment=rel_block(after["edge_jump"][f2, k2], inc), H=rel_block(gam[f2, k2] ** 2 * after["H"][f2], H),
             gain=abs(after["lr"][f2] - 2.0 * (ll1 - llh)) / max(abs(after["lr"][f2]), 1.0))
    print(f"{name}, another edge with the first fit held vs the conditional dense fit: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v <= TOL, (k, v)
    _assert_scan(f"{name}, under the fit", after, SR.device_layout(SR.dense_scan(net, model, held, tbl, taxa), net, ocgb, fam))
    assert _same(after["H"], got["H"])      # (the information does not move with the shifts)


# ----------------------------------------------------------------------------- 3: layouts and launch classes

def _tree_family_nodes(pcgb, tree):
    """Preorder node of every family of a tree's table (0: the root-prior family), through the distinct edge lengths."""
    pre = tree.vec_node
    lens = np.array([tree.parent_edges(pre[i])[0].length for i in range(1, len(pre))])
    assert len(np.unique(lens)) == len(lens)
    out = []
    for f in range(len(pcgb._lg["cluster"])):
        if pcgb._lg["n_parents"][f] == 0:
            out.append(0)
            continue
        i = int(np.argmin(np.abs(lens - pcgb._lg["length"][f])))
        assert abs(lens[i] - pcgb._lg["length"][f]) <= 1e-12
        out.append(i + 1)
    assert len(set(out)) == len(out)
    return out


@pytest.mark.parametrize("p,layout", [(2, 1), (16, 1), (3, 0), (40, 0)])
def test_scan_layouts_and_launch_classes(P, p, layout):
    """test_gpu_shifts._tree_case, three shifts in force: p = 2 and p = 16 packed (BS16) after a calibration, p = 3 plain,
    p = 40 with clusters of 80 variables (the 256-thread instance, more than 64 KB of LDS).  Against the dense statement; on
    the packed engines the same beliefs converted to the plain layout return the same bytes."""
    from pgbp_amd import _lib as L
    tree, model, tbl, pcgb, spt, kw, edges, values, sh = _tree_case(P, p, 40 + p)
    pcgb.set_shifts_lg(edges, values)
    ll, got = pcgb.loglik_and_shift_scan_lg(spt, information=True)
    lib, eng = pcgb._lib, pcgb._eng
    assert lib.pgbp_layout(eng) == layout, (p, lib.pgbp_layout(eng))
    assert (int(pcgb._dims[: pcgb.nclusters].max()) > 64) == (p == 40)
    dense = OD.loglik(tree, ShiftedModel(model, sh), tbl, tree.tip_names)
    assert abs(ll - dense) <= TOL * abs(dense)
    sc = SR.dense_scan(tree, model, sh, tbl, tree.tip_names)
    nodes = _tree_family_nodes(pcgb, tree)
    want = {k: sc[k][nodes].copy() for k in ("jump", "lr", "identified", "H")}
    want["edge_jump"] = want["jump"][:, None, :].copy()      # (a tree: gamma = 1)
    _assert_scan(f"12-tip tree p={p} layout {layout}", got, want)
    if layout == 1:
        rec = np.zeros(int(pcgb._dims[0]) ** 2 + int(pcgb._dims[0]) + 1)
        assert lib.pgbp_get_belief(eng, 0, 0, L.f64p(rec)) == L.PGBP_OK      # (converts the engine to the plain layout)
        assert lib.pgbp_layout(eng) == 0
        plain = pcgb.shift_scan_lg(information=True)
        for k in BLOCKS + ("identified",):
            assert _same(got[k], plain[k]), k


# ----------------------------------------------------------------------------- 4: site batches

def test_scan_site_minor_batch_per_site_everything(P):
    """p = 1, 64 sites in the site-minor layout with their own data, parameters and shifts, some tips without a value: every
    site against the dense statement.  Two site ranges joined equal one call byte for byte; two calls return equal bytes."""
    from pgbp_amd import _lib as L
    p = 1
    cgb, spt, fam = _tree_batch(P, p, masked=True)
    nf = len(fam["cluster"])
    inner = [f for f in range(nf) if fam["child_pos"][f] >= 0]
    tips = [f for f in range(nf) if fam["child_pos"][f] < 0 and int(fam["child_mask"][f]) != 0]
    edges = sorted({(tips[0], 0), (inner[0], 0), (inner[len(inner) // 2], 0)})
    values = np.random.default_rng(19).normal(size=(64, len(edges), p))
    cgb.set_shifts_lg(edges, values)
    cgb._ensure_schedule([spt])
    cgb.loglik_lg()
    assert cgb._lib.pgbp_layout(cgb._eng) & 2, "a univariate batch of 64 sites is expected in the site-minor layout"
    ll, got = cgb.loglik_and_shift_scan_lg(spt, all_sites=True, information=True)   # (the sweep converts, as the edge sweep does)
    assert not got["info"].any()
    skipped = np.flatnonzero(np.asarray(fam["child_mask"]) == 0)
    assert skipped.size and np.all(got["lr"][:, skipped] == 0.0) and np.isnan(got["jump"][:, skipped]).all()
    assert not got["identified"][:, skipped].any()
    worst = {}
    for s in range(64):
        onet, model, tbl, taxa = IR.batch_site(p, s)
        pre = onet.vec_node
        sh = {onet.parent_edges(pre[f + 1])[0].number: v for (f, _), v in zip(edges, values[s])}   # (fixed root: family f = node f + 1)
        dense = OD.loglik(onet, ShiftedModel(model, sh), tbl, taxa)
        assert abs(ll[s] - dense) <= TOL * max(1.0, abs(dense))
        sc = SR.dense_scan(onet, model, sh, tbl, taxa)
        assert np.array_equal(got["identified"][s], sc["identified"][1:]), s
        for k, w in (("jump", sc["jump"][1:]), ("lr", sc["lr"][1:]), ("H", sc["H"][1:])):
            worst[k] = max(worst.get(k, 0.0), rel_block_nan(got[k][s], w))
    print("site-minor batch, 64 sites vs the dense statement: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (k, v)
    lib, eng = cgb._lib, cgb._eng
    import ctypes as C

    def call(s0, s1):
        n = s1 - s0
        out = dict(jump=np.full((n, nf, p), 7.0), lr=np.full((n, nf), 7.0), identified=np.full((n, nf), 7, np.uint64),
                   H=np.full((n, nf, p, p), 7.0))
        info = np.ones(n, np.int32)
        assert lib.pgbp_lg_shift_scan(eng, s0, s1, 1e-8, L.f64p(out["jump"]), L.f64p(out["lr"]),
                                      out["identified"].ctypes.data_as(C.POINTER(C.c_uint64)), L.f64p(out["H"]),
                                      L.i32p(info)) == L.PGBP_OK and not info.any()
        return out
    whole, again, a, b = call(0, 64), call(0, 64), call(0, 23), call(23, 64)
    for k in whole:
        assert whole[k].tobytes() == again[k].tobytes(), k
        assert whole[k].tobytes() == np.concatenate([a[k], b[k]]).tobytes(), k
    assert _same(whole["jump"], got["jump"]) and _same(whole["H"], got["H"]) and _same(whole["lr"], got["lr"])


# ----------------------------------------------------------------------------- 5: the information does not see the data

def test_information_is_independent_of_the_data(P):
    """One engine, the data of hetero3_random_root and the same data with a jump of 1e4 planted on an edge: `information` is
    byte-equal (H_f = j - j C j is formed from C itself; taken out of M = C + e e' it would lose the digits of g_w g_w'),
    and the jump and lr of that edge still meet 1e-8 against the dense one-edge fit."""
    name, net, model, tbl, taxa = next(c for c in CASES if c[0] == "hetero3_random_root")
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    _, first = pcgb.loglik_and_shift_scan_lg(spt, information=True)
    ed = fit_edges(net, model)[1]
    f, k = family_of_edge(net, ocgb, fam, ed)
    p = model.dimension()
    planted, _ = moved_data(net, model, {ed.number: -1e4 * np.ones(p)}, tbl, taxa)
    fam2, data2, kw2 = lg_inputs_from_oracle(P, net, ocgb, model, planted, taxa)
    pcgb.lg_setup(fam2, data2)
    pcgb.assignfactors_lg_(**kw2)
    _, second = pcgb.loglik_and_shift_scan_lg(spt, information=True)
    assert second["H"].tobytes() == first["H"].tobytes()
    assert np.array_equal(second["identified"], first["identified"])
    inc, H, ll1, ll0 = SR.gls_edge(net, model, planted, taxa, ed, range(p))
    e = dict(jump=rel_block(second["edge_jump"][f, k], inc), lr=abs(second["lr"][f] - float(inc @ H @ inc)) / float(inc @ H @ inc))
    print(f"jump of 1e4 planted: recovered {second['edge_jump'][f, k]}, lr {second['lr'][f]:.6e} (without {first['lr'][f]:.3e}); "
          + ", ".join(f"{q} {v:.2e}" for q, v in e.items()))
    assert np.all(np.abs(second["edge_jump"][f, k] - 1e4) < 50.0) and second["lr"][f] > 1e4 * first["lr"][f]
    for q, v in e.items():
        assert v <= TOL, (q, v)


# ----------------------------------------------------------------------------- 6: identification

def test_min_info_above_a_pivot_drops_the_trait(P):
    """missing_fixed_root (p = 2): a family with both traits kept at the default, a trait t of it with the relative pivot r
    (scan_ref: pivot / j_ii, given the kept traits before it) and min_info = 1.02 r, chosen on the dense statement so that t
    is dropped and the other trait stays.  The device drops t, the other trait moves to its own one-trait fit (dense GLS
    restricted to it), and the whole scan equals the dense statement under the same rule."""
    name, net, model, tbl, taxa = next(c for c in CASES if c[0] == "missing_fixed_root")
    pcgb, spt, fam, ocgb, got, sc = _check_dense(P, name, net, model, tbl, taxa)
    nodes = family_nodes(ocgb, fam)
    pick = None
    for f in np.flatnonzero(got["dof"] == 2):
        i = nodes[f]
        for t in (0, 1):
            cut = 1.02 * sc["relpivot"][i, t]
            kept, _, _, rel = SR.restricted_solve(sc["H"][i], sc["gw"][i], sc["jdiag"][i], cut)
            if cut < 1.0 and not kept[t] and kept[1 - t] and rel[1 - t] > 1.02 * cut and pick is None:
                pick = (int(f), t, cut)
    assert pick is not None
    f, t, cut = pick
    sc2 = SR.dense_scan(net, model, {}, tbl, taxa, cut)
    raised = pcgb.shift_scan_lg(min_info=cut, information=True)
    _assert_scan(f"{name}, min_info {cut:.3e}", raised, SR.device_layout(sc2, net, ocgb, fam))
    assert not raised["identified"][f, t] and raised["identified"][f, 1 - t] and got["identified"][f].all()
    ed = family_edge(net, ocgb, fam, f, 0)
    inc, H, _, _ = SR.gls_edge(net, model, tbl, taxa, ed, [1 - t])
    assert abs(raised["edge_jump"][f, 0, 1 - t] - inc[0]) <= TOL * abs(inc[0]) and np.isnan(raised["jump"][f, t])
    assert abs(raised["jump"][f, 1 - t] - got["jump"][f, 1 - t]) > 1e-6 * abs(got["jump"][f, 1 - t])
    assert raised["dof"].sum() < got["dof"].sum()
    print(f"{name}: family {f}, trait {t} dropped at min_info {cut:.3e}; {got['dof'].sum()} -> {raised['dof'].sum()} kept traits")


def test_trait_that_no_tip_below_observes_is_not_identified(P):
    """bm_fixed_root with trait 1 blanked at every tip below an internal node: that node's family reports trait 1 as not
    identified at the default min_info, and trait 0 as the one-trait fit; the whole scan against the dense statement."""
    name, net, model, tbl, taxa = next(c for c in CASES if c[0] == "bm_fixed_root")
    pre = net.vec_node
    inner = [i for i in range(1, len(pre)) if not pre[i].leaf and len(net.parent_edges(pre[i])) == 1
             and 2 <= len(tips_below(net, model, i)) <= 4]
    c = inner[0]
    blank = [list(col) for col in tbl]
    for i in tips_below(net, model, c):
        blank[1][list(taxa).index(pre[i].name)] = None
    pcgb, spt, fam, ocgb, got, sc = _check_dense(P, f"{name}, trait 1 unobserved below node {c}", net, model, blank, taxa)
    f = family_nodes(ocgb, fam).index(c)
    assert got["identified"][f].tolist() == [True, False] and got["dof"][f] == 1
    assert np.isfinite(got["jump"][f, 0]) and np.isnan(got["jump"][f, 1]) and np.isnan(got["H"][f, 1, 1]) and got["lr"][f] > 0.0


# ----------------------------------------------------------------------------- 7: the selection

@pytest.mark.parametrize("case", DENSE, ids=DENSE_IDS)
def test_select_shifts_returns_the_dense_greedy_path(P, case):
    """Jumps of -6 and +5 (all traits) planted on fit_edges[0] and fit_edges[2]: select_shifts_lg(max_shifts=2) returns the
    path of scan_ref.dense_greedy -- the same edges, lr and log-likelihoods at 1e-8.  Condition, asserted on the dense path:
    the best lr exceeds the second by at least 1 % at both steps."""
    name, net, model, tbl, taxa = case
    oe = fit_edges(net, model)
    p = model.dimension()
    planted, _ = moved_data(net, model, {oe[0].number: 6.0 * np.ones(p), oe[2].number: -5.0 * np.ones(p)}, tbl, taxa)
    path = SR.dense_greedy(net, model, planted, taxa, 2)
    assert len(path) == 2
    for st in path:
        print(f"{name} dense step: node {st['node']}, lr {st['lr']:.4f} (second {st['second']:.4f}), loglik {st['loglik']:.6f}")
        assert st["lr"] >= 1.01 * st["second"]
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, planted, taxa, oracle_factors=False)
    sel = P.select_shifts_lg(pcgb, spt, 2)
    nodes = family_nodes(ocgb, fam)
    assert [nodes[f] for f, _ in sel["edges"]] == [st["node"] for st in path]
    worst = {}
    for got, want in zip(sel["path"], path):
        f, k = got["edge"]
        ed = family_edge(net, ocgb, fam, f, k)
        assert ed.gamma == max(e.gamma for e in net.parent_edges(ed.child)) and got["dof"] == p
        e = dict(lr=abs(got["lr"] - want["lr"]) / abs(want["lr"]), loglik=abs(got["loglik"] - want["loglik"]) / abs(want["loglik"]))
        for q, v in e.items():
            worst[q] = max(worst.get(q, 0.0), v)
    print(f"{name}: device path vs dense greedy: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (k, v)
    assert sel["fit"]["loglik"] == sel["path"][-1]["loglik"] and pcgb.shift_count_lg() == 2
    assert abs(sel["loglik0"] - OD.loglik(net, model, planted, taxa)) <= TOL * abs(sel["loglik0"])


def test_select_shifts_excludes_an_unidentifiable_second(P):
    """The pair test_fit_refuses_an_unidentifiable_pair refuses (both child edges of the root under an improper root) as the
    only two candidates: one enters, the joint refit with the other raises, it is excluded and the engine is left at the
    first fit."""
    net, model, tbl, taxa = LR.reference_case("level1_2traits", "improper")
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    kids = [ed for ed in net.edges if ed.parent is net.vec_node[0]]
    edges = [family_of_edge(net, ocgb, fam, ed) for ed in kids]
    with pytest.raises(ValueError):
        P.fit_shifts_lg(pcgb, spt, edges)
    sel = P.select_shifts_lg(pcgb, spt, 2, candidates=[f for f, _ in edges])
    assert len(sel["path"]) == 1 and sel["edges"][0] in edges
    alone = sel["path"][0]
    assert pcgb.shift_count_lg() == 1
    ll, g = pcgb.loglik_and_shift_gradient_lg(spt)
    assert abs(ll - alone["loglik"]) <= TOL * abs(ll) and g.shape == (1, model.dimension())
    ll0, first = pcgb.loglik_and_shift_scan_lg(spt)
    assert abs(ll0 - alone["loglik"]) <= TOL * abs(ll0)
    assert first["lr"][sel["edges"][0][0]] <= TOL * alone["lr"]      # (the engine sits at the first fit)


# ----------------------------------------------------------------------------- 8: refusals

def test_refusals_leave_the_outputs_untouched(P):
    import ctypes as C
    from pgbp_amd import _lib as L
    from test_gpu_exact_bm import _random_tree
    S, rng, tr, nwk, taxa = _random_tree(8, 3)
    net, names = P.read_newick(nwk)
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, 1)
    fresh = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    lib, eng = fresh._lib, fresh._eng
    row = {t: r for r, t in enumerate(taxa)}
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], 1)
    nf = len(fam["cluster"])
    bufs = dict(jump=np.full((nf, 1), 7.0), lr=np.full(nf, 7.0), ident=np.full(nf, 7, np.uint64), H=np.full((nf, 1, 1), 7.0),
                info=np.full(1, 7, np.int32))

    def call(e, s0=0, s1=1, min_info=1e-8, none=False):
        args = [None] * 4 if none else [L.f64p(bufs["jump"]), L.f64p(bufs["lr"]),
                                        bufs["ident"].ctypes.data_as(C.POINTER(C.c_uint64)), L.f64p(bufs["H"])]
        return e._lib.pgbp_lg_shift_scan(e._eng, s0, s1, min_info, *args, L.i32p(bufs["info"]))

    def untouched():
        return all(np.all(v == 7) for v in bufs.values())
    assert call(fresh) == L.ERR_STATE and b"pgbp_lg_setup" in lib.pgbp_last_error(eng) and untouched()
    fresh.lg_setup(fam, rng.normal(size=(len(taxa), 1)))
    assert call(fresh) == L.ERR_STATE and b"pgbp_lg_assignfactors" in lib.pgbp_last_error(eng) and untouched()
    fresh.assignfactors_lg_(np.array([[[1.0]]]), [0.0])
    assert call(fresh, none=True) == L.ERR_INVALID and b"no output buffer" in lib.pgbp_last_error(eng) and untouched()
    for s0, s1 in ((0, 2), (-1, 1), (1, 0)):
        assert call(fresh, s0, s1) == L.ERR_INVALID and b"site range" in lib.pgbp_last_error(eng) and untouched()
    for bad in (-1e-3, 1.0, 2.0, float("nan"), float("inf")):
        assert call(fresh, min_info=bad) == L.ERR_INVALID and b"min_info" in lib.pgbp_last_error(eng) and untouched()
    assert call(fresh, min_info=0.0) == L.PGBP_OK and not untouched()


def test_refuses_clusters_above_128_variables(P):
    """The Mueller clique tree at 3 traits has beliefs of more than 128 variables: PGBP_ERR_INVALID before any launch, the
    family and its cluster named."""
    from pgbp_amd import _lib as L
    from test_gpu_gradient import _muller
    cgb, spt, st, *_ = _muller(P, 3)
    assert int(st.dims.max()) > 128
    assert P.calibrate_(cgb, [spt])[0]
    with pytest.raises(L.PgbpError) as ex:
        cgb.shift_scan_lg()
    assert ex.value.code == L.ERR_INVALID and "more than 128 variables" in ex.value.msg and "family" in ex.value.msg
    assert "cluster" in ex.value.msg and "pgbp_lg_shift_scan" in ex.value.msg


def test_refuses_what_does_not_fit_the_lds(P):
    """p = 40 on a five-tip network with one reticulation: the hybrid family's cluster has 120 variables (117 KB of working
    matrix, which the factor fill and the calibration hold) and the scan's family scratch at 40 traits brings the need to
    184 KB, above the 160 KB of LDS: PGBP_ERR_INVALID before any launch, the outputs untouched."""
    import ctypes as C
    from pgbp_amd import _lib as L
    p = 40
    rng = np.random.default_rng(8)
    net = ON.random_network(5, 1, rng)
    tbl = [list(rng.normal(size=5)) for _ in range(p)]
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, LR.bm(p, rng, "random"), tbl, net.tip_names)
    assert int(pcgb._dims[: pcgb.nclusters].max()) == 120
    pcgb._ensure_schedule([spt])
    ll, info = pcgb.loglik_lg()
    assert info[0] == 0 and np.isfinite(ll[0])
    nf = len(fam["cluster"])
    jump, lr, ident = np.full((nf, p), 7.0), np.full(nf, 7.0), np.full(nf, 7, np.uint64)
    rc = pcgb._lib.pgbp_lg_shift_scan(pcgb._eng, 0, 1, 1e-8, L.f64p(jump), L.f64p(lr), ident.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      None, None)
    msg = pcgb._lib.pgbp_last_error(pcgb._eng)
    assert rc == L.ERR_INVALID and b"bytes of LDS" in msg and b"pgbp_lg_shift_scan" in msg and b"120 variables" in msg
    assert np.all(jump == 7.0) and np.all(lr == 7.0) and np.all(ident == 7)


def test_refuses_more_than_64_traits(P):
    """p = 65 on a four-tip tree with a fixed root (clusters of 65 variables; the host's lg_families stops at 64 traits, so
    its p = 64 table -- every position is 0 or none on this tree -- is given to pgbp_lg_setup with p = 65): the trait mask
    holds 64, and the table is refused as soon as it is known, the outputs untouched."""
    import ctypes as C
    from pgbp_amd import _lib as L
    net, names = P.read_newick("((a:0.7,b:1.3):0.5,(c:1.0,d:0.4):0.6);")
    cn, ed, sn = P.cliquetree(net.node2family)
    row = {"a": 0, "b": 1, "c": 2, "d": 3}
    st64 = P.allocate_scopes(cn, ed, sn, net, 64, fixedroot=True)
    fam = P.lg_families(st64.clusters, st64.node2cluster, net.node2family, st64.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], 64)
    assert set(np.unique(fam["child_pos"])) <= {-1, 0} and set(np.unique(fam["parent_pos"])) <= {-1, 0}
    p = 65
    st = P.allocate_scopes(cn, ed, sn, net, p, fixedroot=True)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(dict(fam, p=p), np.random.default_rng(2).normal(size=(4, p)))
    nf = len(fam["cluster"])
    jump, lr, ident = np.full((nf, p), 7.0), np.full(nf, 7.0), np.full(nf, 7, np.uint64)
    rc = cgb._lib.pgbp_lg_shift_scan(cgb._eng, 0, 1, 1e-8, L.f64p(jump), L.f64p(lr), ident.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     None, None)
    msg = cgb._lib.pgbp_last_error(cgb._eng)
    assert rc == L.ERR_INVALID and b"p = 65" in msg and b"64" in msg
    assert np.all(jump == 7.0) and np.all(lr == 7.0) and np.all(ident == 7)

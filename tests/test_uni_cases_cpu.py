"""The inputs of the thread-per-site GPU tests pinned without a GPU, so that their preconditions rest on the reference alone.

(1) tests/message_ref.py's tiny shapes (uni_shape_cases and the special cases, on the two-cluster engine and on both
chains): the case list is complete, the first sites keep their bytes whatever the engine's size, the longdouble restatement
agrees with the plain-C engine at every site of every case, the placed failures fail where placed and stop the message out
of the receiver, and the planner reports what tests/run_uni_message_shapes.py relies on.
(2) tests/uni_net_ref.py's networks with hybrid tips: both host sides read them alike, the oracle's cluster graphs have the
dimensions the GPU tests need (2-variable sepsets, 0-variable clusters and sepsets, a loopy Bethe graph of 1-variable
sepsets), belief propagation on the clique trees gives the dense log-likelihood, 30 iterations on the Bethe graphs succeed at
every site, and the models' own hybrid factors agree with the generic ones.
"""
import numpy as np
import pytest

import message_ref as M
import uni_net_ref as N
from oracle import clustergraph as OCG
from oracle import densemvn as OD

EPS = M.EPS


# ---------------------------------------------------------------------------------------------------------------------
# (1) the tiny shapes
# ---------------------------------------------------------------------------------------------------------------------

def test_the_case_list_is_the_whole_enumeration():
    cases = M.uni_shape_cases()
    assert len({c.name for c in cases}) == len(cases) == 114
    want = set()
    for mf in range(3):
        for mt in range(3):
            for s in range(min(mf, mt) + 1):
                for keep in ([()] if s == 0 else [(0,)] if (s, mf) == (1, 1) else [(0,), (1,)] if s == 1 else [(0, 1)]):
                    for up in ([()] if s == 0 else [(0,)] if (s, mt) == (1, 1) else [(0,), (1,)] if s == 1 else [(0, 1)]):
                        want.add((mf, s, mt, keep, up))
    assert len(want) == 19
    got = {}
    for c in cases:
        b = M.build_case(c)
        key = (c.mf, c.s, c.mt, tuple(int(x) for x in b.keep), tuple(int(x) for x in b.up))
        got.setdefault(key, set()).add((c.sep_kind, c.flip))
    assert set(got) == want
    assert all(v == {(k, f) for k in M.SEP_KINDS for f in (False, True)} for v in got.values())
    assert {(c.mf - c.s, c.s, c.fail[1]) for c in M.uni_exit2_cases()} == {(ni, s, c) for ni, s in ((1, 1), (1, 0), (2, 0)) for c in (EPS, 2 * EPS)}
    assert {(c.mf - c.s, c.fail[1]) for c in M.uni_failure_cases()} == {(1, 1), (2, 1), (2, 2)}
    for n, ev in M.UNI_EVENT_SITES.items():
        assert all(0 < s < n and s % 64 != 0 for s in ev if s != 64) and (64 in ev) == (n == 65)


def test_more_sites_keep_the_bytes_of_the_first():
    for case in M.all_message_cases()[::7] + M.uni_shape_cases()[::5]:
        two, many = M.build_case(case), M.build_case(case, 9)
        assert np.array_equal(two.packed, many.packed[:2]) and np.array_equal(two.keep, many.keep) and np.array_equal(two.up, many.up)
    for case in M.uni_shape_cases()[::11]:
        for kind in M.UNI_KINDS:
            if kind == "chain1" and case.s > 1:
                continue
            a, b = M.build_uni(case, kind, 8), M.build_uni(case, kind, 65)
            assert np.array_equal(a.packed, b.packed[:8]) and np.array_equal(a.dims, b.dims)


def _check_against_c_engine(ub):
    """every site: the longdouble reference and the C engine agree on info, records, residuals and flags"""
    worst = 0.0
    for site in range(ub.n_sites):
        refs = M.uni_reference(ub, ub.packed[site])
        pk, res, flg, infos = M.uni_c_engine(ub, ub.packed[site])
        recs, start = M.uni_records(ub, pk), M.uni_records(ub, ub.packed[site])
        for j, (m, r, info) in enumerate(zip(ub.msgs, refs, infos)):
            sep_i = ub.nc + m.k
            if r is None or r[3]:
                assert (r is None and info is None) or (r[3] == info == ub.case.fail[1] and site in ub.fail_sites and j == 0)
                for a, b in zip(recs[sep_i] + recs[m.i_to], start[sep_i] + start[m.i_to]):
                    assert np.array_equal(np.asarray(a), np.asarray(b))
                continue
            assert info == 0
            bound = 64 * max(1, int(ub.dims[m.i_from])) * EPS       # tests/test_message_ref_cpu.py
            (dJ, dh), d = M.residual_of(ub, m, res)
            for got, want in ((recs[sep_i], r[0]), (recs[m.i_to], r[1]), ((dJ, dh), r[2])):
                err, scale = M.record_error(got, want)
                worst = max(worst, err / scale)
                assert err <= bound * scale, (ub.case.name, ub.kind, site, j, err / scale)
            assert bool(flg[d]) == M.residnorm_flag_ld(*r[2]), (ub.case.name, ub.kind, site, j)
        assert (refs[0][3] != 0) == (site in ub.fail_sites)
        if site in ub.fail_sites:
            assert all(r is None for r in refs[1:])
    return worst


@pytest.mark.parametrize("kind", M.UNI_KINDS)
def test_reference_agrees_with_the_c_engine_on_every_tiny_shape(kind):
    worst = 0.0
    for case in M.uni_shape_cases():
        if not (kind == "chain1" and case.s > 1):
            ub = M.build_uni(case, kind, 8)
            assert int(ub.dims.max()) <= 2
            assert int(ub.dims[ub.nc:].max()) == (2 if kind == "chain2" else case.s if kind == "pair" else min(1, max(case.s, case.mt)))
            worst = max(worst, _check_against_c_engine(ub))
    print(f"{kind}: C engine vs longdouble, worst {worst:.2e} of max(1, |.|_inf)")


@pytest.mark.parametrize("kind", M.UNI_KINDS)
def test_special_cases_do_what_they_are_placed_for(kind):
    for case in M.uni_exit2_cases() + M.uni_failure_cases():
        if kind == "chain1" and case.s > 1:
            continue
        for n in (8, 65):
            ub = M.build_uni(case, kind, n)
            _check_against_c_engine(ub)
            if case.fail[0] == "exit2":
                for site in (0,) + M.UNI_EVENT_SITES[n]:
                    assert M.uni_reference(ub, ub.packed[site])[0][4] == (2 if case.fail[1] <= EPS else 0)
                assert M.uni_reference(ub, ub.packed[1])[0][4] == 0
            else:
                assert ub.fail_sites == M.UNI_EVENT_SITES[n]


def test_the_planner_fuses_the_two_level_chains_only():
    import pgbp_amd as P
    import run_uni_message_shapes as U
    P.load()
    for case in M.uni_shape_cases()[::9]:
        for n in (8, 65):
            assert U.plan_report(P, M.build_uni(case, "pair", n)) == (1, [])
            if case.s <= 1:
                assert U.plan_report(P, M.build_uni(case, "chain1", n)) == (2, [(0, 2)])


# ---------------------------------------------------------------------------------------------------------------------
# (2) the networks with hybrid tips
# ---------------------------------------------------------------------------------------------------------------------

CASES = [(n, r, k) for n in N.NEWICK for r in N.ROOTS[n] for k in ("bm", "ou")]


@pytest.mark.parametrize("name", list(N.NEWICK))
def test_both_host_sides_read_a_hybrid_tip_as_a_leaf(name):
    import pgbp_amd as P
    net, taxa = N.network(name)
    pnet, names = P.read_newick(N.NEWICK[name])
    hyb = [n for n in net.vec_node if n.hybrid]
    assert hyb and all(n.leaf and len(net.parent_edges(n)) == 2 for n in hyb) and all(n.name in taxa for n in hyb)
    assert sorted(names) == sorted(n.name for n in net.vec_node)
    pos = {nm: i for i, nm in enumerate(names)}
    for n in net.vec_node:
        i = pos[n.name]
        assert bool(pnet.is_leaf[i]) == n.leaf
        assert sorted(names[q - 1] for q in pnet.node2family[i][1:]) == sorted(e.parent.name for e in net.parent_edges(n))
        got = {names[q - 1]: (t, g) for q, t, g in zip(pnet.node2family[i][1:], pnet.length[i], pnet.gamma[i])}
        for e in net.parent_edges(n):
            assert got[e.parent.name] == (e.length, e.gamma if n.hybrid else 1.0)
    if name == "N4":
        assert any(e.parent is net.root for e in net.parent_edges(hyb[0]))


def _dims(name, root, graph_kind):
    net, taxa = N.network(name)
    m, t = N.sites(name, root, "bm")[0]
    return N.dims_of(net, N.graph(net, graph_kind), m, t, taxa)


def test_cluster_and_sepset_dimensions():
    assert _dims("N1", "fixed", "cliquetree") == ([2, 1, 1, 1, 2, 2], [2, 1, 1, 1, 1])
    assert _dims("N2", "fixed", "cliquetree") == ([2, 2, 1, 2, 1], [2, 2, 1, 1])
    cd, sd = _dims("N3", "fixed", "cliquetree")
    assert max(cd) == 2 and 2 in sd and 0 in sd
    cd, sd = _dims("N4", "fixed", "cliquetree")
    assert max(cd) <= 2 and 0 in cd          # the root-parented hybrid tip: a cluster of dimension 0
    for name in ("N1", "N2", "N3"):
        net, _ = N.network(name)
        cd, sd = _dims(name, "random", "bethe")
        assert max(cd) == 2 and set(sd) == {1}
        assert len(sd) > len(cd) - 1, "a loopy graph has more edges than a tree"
        assert len(N.schedule(net, N.graph(net, "bethe"), "bethe")) >= 2
        cd, sd = _dims(name, "fixed", "bethe")
        assert max(cd) <= 2 and 0 in cd and 0 in sd
        assert max(_dims(name, "random", "cliquetree")[0]) == 3     # NOT a thread-per-site engine: the wave-per-task kernels


def test_the_products_cliquetree_of_n1_has_a_three_variable_cluster():
    """why every device engine of tests/test_gpu_uni_networks.py is built from the oracle's cluster graph"""
    import pgbp_amd as P
    pnet, _ = P.read_newick(N.NEWICK["N1"])
    cn, ed, sn = P.cliquetree(pnet.node2family)
    st = P.allocate_scopes(cn, ed, sn, pnet, 1, fixedroot=True)
    assert int(np.max(st.dims)) == 3


@pytest.mark.parametrize("name,root,kind", CASES)
def test_clique_tree_loglik_is_the_dense_one(name, root, kind):
    net, taxa = N.network(name)
    cg = N.graph(net, "cliquetree")
    rootj = OCG.default_rootcluster(cg, net)
    worst = 0.0
    for site in range(8):
        snaps, ocgb = N.oracle_calibration(name, root, kind, "cliquetree", site)
        assert snaps[1].got[0]
        m, t = N.sites(name, root, kind)[site]
        dense = OD.loglik(net, m, t, taxa)
        worst = max(worst, abs(ocgb.integratebelief(rootj)[1] - dense) / max(1.0, abs(dense)))
    print(f"{name}/{root}/{kind}: integratebelief vs densemvn.loglik, worst of 8 sites {worst:.2e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("name,root,kind", CASES)
def test_bethe_calibration_succeeds_at_every_site(name, root, kind):
    """30 iterations of the oracle's calibrate! on the Bethe graph: at EVERY site of the cases the GPU test calibrates
    (uni_net_ref.LOOPY_CASES), at the first 8 sites of the others."""
    n = N.MAX_SITES if (name, root, kind) in N.LOOPY_CASES else 8
    for site in range(n):
        snaps, _ = N.oracle_calibration(name, root, kind, "bethe", site, N.LOOPY_STEPS)
        assert all(s.got[0] for s in snaps.values()), (name, root, kind, site)
        assert snaps[30].got[1], "30 iterations reach calibration"


@pytest.mark.parametrize("name,root,kind", CASES)
def test_hybrid_factors_agree_with_the_generic_ones(name, root, kind):
    net, _ = N.network(name)
    worst = 0.0
    for m, _ in N.sites(name, root, kind)[:8]:
        err, nh = N.hybrid_factor_error(net, m)
        assert nh == (2 if name == "N2" else 1)
        worst = max(worst, err)
    print(f"{name}/{root}/{kind}: own factors vs the generic ones {worst:.2e}")
    assert worst <= 1e-12

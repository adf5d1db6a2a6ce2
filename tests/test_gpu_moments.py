"""pgbp_moments: posterior mean, covariance and normalisation constant of many beliefs in one device call.

mu / norm / info are compared bit for bit with the single-belief path (pgbp_integrate, called with a mean buffer); the
covariance with numpy's float64 inverse of the symmetrised upper triangle at 1e-8 relative (the project's parity gate),
after checking on the very same matrices that numpy's inverse is itself within 1e-10 of a numpy.longdouble Cholesky
inverse (the hundredfold headroom the gate needs, asserted per belief; measured worst over every case below: 7.8e-16; the
device's covariance was at most 2.1e-15 from numpy's on the same matrices)."""
import ctypes as C

import numpy as np
import pytest

from helpers import goldens, make_model, oracle_setup, product_beliefs_from_oracle
from oracle import clustergraph as OCG
from oracle import network as ON

pytestmark = pytest.mark.gpu
G = goldens()


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


# ----------------------------------------------------------------------------- raw calls

def _dims(cgb):
    return [int(cgb._lib.pgbp_belief_dim(cgb._eng, b)) for b in range(cgb.nbeliefs)]


def _record(cgb, site, b):
    m = int(cgb._lib.pgbp_belief_dim(cgb._eng, b))
    rec = np.zeros(m * m + m + 1)
    assert cgb._lib.pgbp_get_belief(cgb._eng, site, b, rec.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return rec[: m * m].reshape(m, m, order="F").copy(), rec[m * m: m * m + m].copy(), float(rec[-1])


def _set_record(cgb, site, b, J, h, g):
    rec = np.concatenate([np.asarray(J, float).reshape(-1, order="F"), np.asarray(h, float), [float(g)]])
    assert cgb._lib.pgbp_set_belief(cgb._eng, site, b, rec.ctypes.data_as(C.POINTER(C.c_double))) == 0


def _moments_raw(cgb, beliefs, s0, s1, cov, out=None, info=None):
    """The C call itself; returns (status, out [s1 - s0, per], info [s1 - s0, n])."""
    lib = cgb._lib
    if beliefs is None:
        ptr, n, nl = None, 0, cgb.nclusters
    else:
        arr = np.ascontiguousarray(beliefs, dtype=np.int32)
        ptr, n, nl = arr.ctypes.data_as(C.POINTER(C.c_int32)), int(arr.size), int(arr.size)
    per = int(lib.pgbp_moments_size(cgb._eng, n, ptr, int(cov)))
    if per < 0:
        return lib.pgbp_moments(cgb._eng, n, ptr, s0, s1, int(cov), None, None), None, None
    if out is None:
        out = np.zeros((max(s1 - s0, 1), max(per, 1)))
    if info is None:
        info = np.zeros((max(s1 - s0, 1), max(nl, 1)), dtype=np.int32)
    rc = lib.pgbp_moments(cgb._eng, n, ptr, s0, s1, int(cov), out.ctypes.data_as(C.POINTER(C.c_double)),
                          info.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out, info


def _integrate_raw(cgb, b):
    m = int(cgb._lib.pgbp_belief_dim(cgb._eng, b))
    ns = cgb.n_sites
    mu = np.full((ns, max(1, m)), -7.0)
    norm = np.zeros(ns)
    info = np.zeros(ns, dtype=np.int32)
    assert cgb._lib.pgbp_integrate(cgb._eng, b, mu.ctypes.data_as(C.POINTER(C.c_double)),
                                   norm.ctypes.data_as(C.POINTER(C.c_double)), info.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    return mu.reshape(-1)[: ns * m].reshape(ns, m), norm, info


def _split(out_row, dims, beliefs, cov):
    res, at = [], 0
    for b in beliefs:
        m = dims[b]
        Sig = None
        if cov:
            Sig = out_row[at: at + m * m].reshape(m, m, order="F")
            at += m * m
        res.append((out_row[at: at + m], Sig, out_row[at + m]))
        at += m + 1
    assert at == out_row.size or (at == 0 and out_row.size == 1)
    return res


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same_as_integrate(cgb, beliefs=None, exact=True):
    """mu, norm, info of pgbp_moments (with and without the covariance) against pgbp_integrate, belief by belief."""
    dims = _dims(cgb)
    lst = list(range(cgb.nbeliefs)) if beliefs is None else list(beliefs)
    ns = cgb.n_sites
    got = {}
    for cov in (1, 0):
        rc, out, info = _moments_raw(cgb, lst, 0, ns, cov)
        assert rc == 0, cgb._lib.pgbp_last_error(cgb._eng)
        got[cov] = ([_split(out[s], dims, lst, cov) for s in range(ns)], info)
    assert np.array_equal(got[1][1], got[0][1])
    for i, b in enumerate(lst):
        mu, norm, info = _integrate_raw(cgb, b)
        for s in range(ns):
            for cov in (1, 0):
                gmu, _, gnorm = got[cov][0][s][i]
                assert got[cov][1][s, i] == info[s], (b, s)
                if info[s] != 0:
                    assert np.isnan(gnorm) and np.all(np.isnan(gmu))
                    continue
                if exact:
                    assert np.array_equal(_bits(gnorm), _bits(norm[s])), (b, s, gnorm, norm[s])
                    assert np.array_equal(_bits(gmu), _bits(mu[s])), (b, s, gmu, mu[s])
                else:
                    assert abs(gnorm - norm[s]) <= 1e-12 * max(1.0, abs(norm[s])), (b, s, gnorm, norm[s])
                    assert np.all(np.abs(gmu - mu[s]) <= 1e-12 * np.maximum(1.0, np.abs(mu[s]))), (b, s)
    return got[1][0], lst, dims


def _longdouble_inverse(A):
    """Inverse of a symmetric positive definite matrix through a Cholesky factor, all in numpy.longdouble."""
    A = np.asarray(A, dtype=np.longdouble)
    m = A.shape[0]
    Lc = np.zeros((m, m), dtype=np.longdouble)
    for j in range(m):
        v = A[j:, j] - Lc[j:, :j] @ Lc[j, :j]
        Lc[j:, j] = v / np.sqrt(v[0])
    Y = np.zeros((m, m), dtype=np.longdouble)   # L Y = I
    for i in range(m):
        e = np.zeros(m, dtype=np.longdouble)
        e[i] = 1
        Y[i] = (e - Lc[i, :i] @ Y[:i]) / Lc[i, i]
    return Y.T @ Y


def _assert_covariances(cgb, moments, lst, dims, site=0):
    """max|Sigma_dev - inv(J)| <= 1e-8 max|inv(J)| and max|J Sigma_dev - I| <= 1e-8 m, numpy float64 inv on the symmetrised
    upper triangle -- after numpy's own inverse showed at most 1e-10 against the longdouble Cholesky inverse."""
    n_checked = 0
    for i, b in enumerate(lst):
        m = dims[b]
        J, h, _ = _record(cgb, site, b)
        if m == 0 or not (np.any(J) or np.any(h)):
            continue
        Js = np.triu(J) + np.triu(J, 1).T
        if np.isnan(moments[site][i][2]):                         # the device says not positive definite: numpy must agree
            assert np.min(np.linalg.eigvalsh(Js)) <= 1e-12 * np.max(np.abs(Js)), (b, m)
            continue
        ref = np.linalg.inv(Js)
        scale = float(np.max(np.abs(ref)))
        ref_err = float(np.max(np.abs(ref - _longdouble_inverse(Js).astype(np.float64)))) / scale
        assert ref_err <= 1e-10, f"belief {b}: numpy inv is {ref_err:.2e} from the longdouble inverse: pick other inputs"
        Sig = moments[site][i][1]
        assert np.array_equal(Sig, Sig.T), b                      # both triangles written, the same bits
        err = float(np.max(np.abs(Sig - ref))) / scale
        res = float(np.max(np.abs(Js @ Sig - np.eye(m)))) / m
        print(f"belief {b} m={m}: |Sigma - inv J| / max|inv J| = {err:.2e}, |J Sigma - I| / m = {res:.2e}, numpy vs longdouble {ref_err:.2e}")
        assert err <= 1e-8, (b, m, err)
        assert res <= 1e-8, (b, m, res)
        n_checked += 1
    return n_checked


# ----------------------------------------------------------------------------- calibrated states

def _synth_tree(P, ntips, p, seed, n_sites=1, calibrate=True):
    from pgbp_amd import synth as S
    rng = np.random.default_rng(seed)
    tr = S.random_tree(ntips, rng)
    R = S.random_rate_matrix(p, rng)
    prob = S.cliquetree_of_tree(tr, p)
    packed = np.stack([S.bm_factors_cliquetree(tr, prob, R, np.zeros(p), S.simulate_bm(tr, R, np.zeros(p), rng))
                       for _ in range(n_sites)])
    cgb = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx,
                                           packed if n_sites > 1 else packed[0], n_sites=n_sites)
    if calibrate:
        assert P.calibrate_(cgb, prob.schedule, 2) == (True, True)
    return prob, cgb


def _golden_cliquetree(P, key, traits):
    g = G[key]
    net = ON.read_newick(g["net"])
    ct = OCG.cliquetree(net)
    spt = OCG.spanningtree_clusterlist(ct, OCG.default_rootcluster(ct, net))
    ocgb = oracle_setup(net, ct, make_model(g["model"]), [g[t] for t in traits], g["taxa"])
    pcgb = P.ClusterGraphBelief(product_beliefs_from_oracle(ocgb.belief), ocgb.node2cluster, ocgb.node2family,
                                ocgb.node2fixed, ocgb.cluster2nodes)
    assert P.calibrate_(pcgb, [spt])[0]
    return g, net, ocgb, pcgb


def _level3_graph(P, graph, p=2):
    """Bethe / join graph of the level-3 golden network, factors of a BM on simulated-looking data, calibrated."""
    g = G["joingraph_mateescu"]
    net, names = P.read_newick(g["net"])
    cn, ed, sn = P.bethe(net.node2family) if graph == "bethe" else P.joingraph(net.node2family, 3)
    st = P.allocate_scopes(cn, ed, sn, net, p)
    tips = [names[i] for i in range(net.nnodes) if net.is_leaf[i]]
    row = {t: r for r, t in enumerate(tips)}
    rng = np.random.default_rng(11)
    data = rng.standard_normal((len(tips), p))
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], p)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(fam, data)
    A = rng.standard_normal((p, p))
    cgb.assignfactors_lg_(R=(A @ A.T + p * np.eye(p))[None], mu=np.zeros(p), sync=True)
    sched = P.spanningtrees_clusterlist(len(cn), ed, cn, net.is_leaf)
    P.regularizebeliefs_bycluster_(cgb)
    P.calibrate_(cgb, sched, 8)
    return cgb


# ----------------------------------------------------------------------------- 1, 2: bit identity and covariance

def test_moments_ragged_cliquetree_golden(P):
    """calibration_cliquetree_level1: ragged scopes (clusters of one to three variables)."""
    _, _, _, pcgb = _golden_cliquetree(P, "calibration_cliquetree_level1", ["y"])
    mom, lst, dims = _assert_same_as_integrate(pcgb)
    assert _assert_covariances(pcgb, mom, lst, dims) >= 5


def test_moments_missing_data_tree_dimension_zero_sepset(P):
    """calibration_tree_2traits_missing: a dimension-0 sepset (norm = g, nothing else written) and the all-zero exit."""
    _, _, _, pcgb = _golden_cliquetree(P, "calibration_tree_2traits_missing", ["y1", "y2"])
    dims = _dims(pcgb)
    assert 0 in dims
    mom, lst, dims = _assert_same_as_integrate(pcgb)
    b0 = dims.index(0)
    assert mom[0][b0][0].size == 0 and mom[0][b0][1].size == 0 and mom[0][b0][2] == _record(pcgb, 0, b0)[2]
    _assert_covariances(pcgb, mom, lst, dims)


@pytest.mark.parametrize("graph", ["bethe", "joingraph"])
def test_moments_level3_network_graphs(P, graph):
    cgb = _level3_graph(P, graph)
    mom, lst, dims = _assert_same_as_integrate(cgb)
    assert _assert_covariances(cgb, mom, lst, dims) >= 5


@pytest.mark.parametrize("p,ntips", [(3, 40), (8, 40), (16, 48), (32, 24)])
def test_moments_random_trees_all_classes(P, p, ntips):
    """Clusters of p and 2p variables: the row-of-16-lanes class (3, 6, 8, 16), the wavefront class (32, 64); p = 16 is
    the packed (BS16) layout after a calibration."""
    prob, cgb = _synth_tree(P, ntips, p, 100 + p)
    mom, lst, dims = _assert_same_as_integrate(cgb)
    assert max(dims) == 2 * p
    assert _assert_covariances(cgb, mom, lst, dims) >= ntips


@pytest.mark.parametrize("p", [40, 64])
def test_moments_workgroup_class(P, p):
    """Beliefs of 80 and of 128 variables: the workgroup class, the in-place inverse in LDS."""
    prob, cgb = _synth_tree(P, 12, p, 7 + p)
    mom, lst, dims = _assert_same_as_integrate(cgb)
    assert max(dims) == 2 * p
    assert _assert_covariances(cgb, mom, lst, dims) >= 12


# ----------------------------------------------------------------------------- 3: golden

def test_moments_exactBM_tree_golden(P):
    """exactBM_tree_calibrate: conditional expectations, variances and covariances with the parent of every internal
    node as R's PhylogeneticEM gives them (seven digits: atol 1e-6), from Sigma and mu of the clusters."""
    g, net, ocgb, pcgb = _golden_cliquetree(P, "exactBM_tree_calibrate", ["y"])
    name_of = {"root": net.vec_node[0].name}
    by_name = {n.name: n for n in net.vec_node}
    name_of["AB"] = net.parents(by_name["A"])[0].name
    name_of["DE"] = net.parents(by_name["D"])[0].name
    name_of["CDE"] = net.parents(by_name["C"])[0].name
    want = {name_of[r]: (g["condexp"][k], g["condvar"][k], g["condcovar_with_parent"][k])
            for k, r in enumerate(g["R_node_names"]) if r in name_of}
    mom = pcgb.moments_()
    seen, seen_cov = set(), set()
    for ci in range(pcgb.nclusters):
        ob = ocgb.belief[ci]
        mu, Sig, _ = mom[ci]
        labs = [lab for k, lab in enumerate(ob.nodelabel) if ob.inscope[0, k]]
        assert len(labs) == mu.size
        for a, la in enumerate(labs):
            na = net.vec_node[la - 1]
            if na.name not in want:
                continue
            assert abs(mu[a] - want[na.name][0]) <= g["atol"], (ci, na.name)
            assert abs(Sig[a, a] - want[na.name][1]) <= g["atol"], (ci, na.name)
            seen.add(na.name)
            for b, lb in enumerate(labs):
                if net.vec_node[lb - 1] in net.parents(na) and want[na.name][2] is not None:
                    assert abs(Sig[a, b] - want[na.name][2]) <= g["atol"], (ci, na.name)
                    seen_cov.add(na.name)
    assert seen == set(want) and seen_cov == {name_of["AB"], name_of["CDE"], name_of["DE"]}


# ----------------------------------------------------------------------------- 4: edge cases

def test_moments_edge_cases(P):
    prob, cgb = _synth_tree(P, 20, 3, 5, n_sites=3)
    dims = _dims(cgb)
    nb = cgb.nbeliefs
    allb = list(range(nb))
    rc, base, binfo = _moments_raw(cgb, allb, 0, 3, 1)
    assert rc == 0 and not binfo.any()
    # several sites with different data: every site its own values, equal to the single-belief path
    _assert_same_as_integrate(cgb)
    assert not np.array_equal(base[0], base[1])
    # two consecutive calls: identical bytes
    rc, again, _ = _moments_raw(cgb, allb, 0, 3, 1)
    assert rc == 0 and np.array_equal(_bits(base), _bits(again))
    # beliefs = NULL: all clusters, in index order
    rc, outc, infoc = _moments_raw(cgb, None, 0, 3, 1)
    rc2, outl, _ = _moments_raw(cgb, list(range(cgb.nclusters)), 0, 3, 1)
    assert rc == 0 and rc2 == 0 and infoc.shape == (3, cgb.nclusters) and np.array_equal(_bits(outc), _bits(outl))
    # a strict subset of the sites: only its rows are written
    per = base.shape[1]
    canvas = np.full((3, per), 123.25)
    cinfo = np.full((3, nb), -5, dtype=np.int32)
    rc, _, _ = _moments_raw(cgb, allb, 1, 2, 1, out=canvas[1:2], info=cinfo[1:2])
    assert rc == 0 and np.array_equal(_bits(canvas[1]), _bits(base[1]))
    assert np.all(canvas[[0, 2]] == 123.25) and np.all(cinfo[[0, 2]] == -5) and not cinfo[1].any()
    # a list in another order, with a repetition
    lst = [nb - 1, 0, 2, 0]
    rc, outp, _ = _moments_raw(cgb, lst, 0, 3, 1)
    ref = _split(base[2], dims, allb, 1)
    for (mu, Sig, norm), b in zip(_split(outp[2], dims, lst, 1), lst):
        assert np.array_equal(mu, ref[b][0]) and np.array_equal(Sig, ref[b][1]) and norm == ref[b][2]
    # an all-zero belief and a belief that is not positive definite among good ones (site 1 only)
    zb, bad = 1, 4
    m = dims[bad]
    assert m >= 3 and dims[zb] > 0
    _set_record(cgb, 1, zb, np.zeros((dims[zb], dims[zb])), np.zeros(dims[zb]), -2.5)
    Jb = 2.0 * np.eye(m)
    Jb[0, 1] = Jb[1, 0] = 2.5          # second pivot 2 - 2.5^2 / 2 < 0: info = 2
    _set_record(cgb, 1, bad, Jb, np.ones(m), 0.0)
    rc, out2, info2 = _moments_raw(cgb, allb, 0, 3, 1)
    assert rc == 0
    for s in (0, 2):
        assert np.array_equal(_bits(out2[s]), _bits(base[s])) and not info2[s].any()
    got, was = _split(out2[1], dims, allb, 1), _split(base[1], dims, allb, 1)
    for b in allb:
        mu, Sig, norm = got[b]
        if b == zb:
            assert info2[1, b] == 0 and np.all(np.isposinf(mu)) and np.all(np.isnan(Sig)) and norm == -2.5
        elif b == bad:
            assert info2[1, b] == 2 and np.all(np.isnan(mu)) and np.all(np.isnan(Sig)) and np.isnan(norm)
        else:
            assert info2[1, b] == 0 and np.array_equal(mu, was[b][0]) and np.array_equal(Sig, was[b][1]) and norm == was[b][2]
    _assert_same_as_integrate(cgb)
    # the host mirror: the current site's non-PD belief raises integratebelief_'s error, another site does not
    cgb.site = 1
    with pytest.raises(np.linalg.LinAlgError, match=r"PosDefException: matrix is not positive definite; Cholesky factorization failed \(info=2\)"):
        cgb.moments_([0, bad])
    cgb.site = 0
    (mu0, Sig0, n0), = cgb.moments_([bad])
    assert np.array_equal(Sig0, _split(base[0], dims, allb, 1)[bad][1]) and cgb.moments_([bad], cov=False)[0][1] is None
    res = cgb.moments_(all_sites=True)
    assert len(res) == cgb.nclusters and res[0][0].shape == (3, dims[0]) and res[0][1].shape == (3, dims[0], dims[0])
    assert res[bad][3].tolist() == [0, 2, 0]
    # refusals: nothing is launched, the message names the culprit
    for lst_bad in ([0, nb], [-1]):
        rc, _, _ = _moments_raw(cgb, lst_bad, 0, 3, 1)
        assert rc == 1 and str(lst_bad[-1]).encode() in cgb._lib.pgbp_last_error(cgb._eng)
    for s0, s1 in ((-1, 2), (2, 1), (0, 4)):
        rc, _, _ = _moments_raw(cgb, [0], s0, s1, 1)
        assert rc == 1 and b"site range" in cgb._lib.pgbp_last_error(cgb._eng)
    with pytest.raises(P.PgbpError):
        cgb.moments_([nb])


def test_moments_refuses_beliefs_above_128_variables(P):
    prob, cgb = _synth_tree(P, 6, 70, 3, calibrate=False)
    dims = _dims(cgb)
    big = next(b for b in range(cgb.nbeliefs) if dims[b] == 140)
    small = [b for b in range(cgb.nbeliefs) if dims[b] == 70]
    canvas = np.full((1, 70 * 70 + 71 + 140 * 140 + 141), 9.0)
    arr = np.array([small[0], big], dtype=np.int32)
    rc = cgb._lib.pgbp_moments(cgb._eng, 2, arr.ctypes.data_as(C.POINTER(C.c_int32)), 0, 1, 1,
                               canvas.ctypes.data_as(C.POINTER(C.c_double)), None)
    msg = cgb._lib.pgbp_last_error(cgb._eng).decode()
    assert rc == 1 and f"belief {big} " in msg and "140" in msg and np.all(canvas == 9.0)
    assert cgb._lib.pgbp_moments_size(cgb._eng, 2, arr.ctypes.data_as(C.POINTER(C.c_int32)), 1) == -1
    # ... while the 70-variable beliefs of the same graph are served
    mom, lst, dims = _assert_same_as_integrate(cgb, small)
    assert _assert_covariances(cgb, mom, lst, dims) >= 4      # (the clusters; the sepsets still hold the constant 1)


def test_moments_site_minor_univariate_batch(P):
    """A univariate batch (64 sites, every dimension <= 2) lives in the site-minor layout after a calibration: the call
    converts to the plain layout first.  pgbp_integrate has a closed form of its own there, so mu and norm agree to
    1e-12 relative, not bit for bit; the covariance gate is the same."""
    prob, cgb = _synth_tree(P, 30, 1, 77, n_sites=64)
    mom, lst, dims = _assert_same_as_integrate(cgb, exact=False)
    for s in (0, 17, 63):
        assert _assert_covariances(cgb, mom, lst, dims, site=s) >= 30
    assert P.calibrate_(cgb, prob.schedule, 1)[0]      # the engine goes on working (back to its own layout)
    mom2, _, _ = _assert_same_as_integrate(cgb, exact=False)
    for s in (0, 63):
        for a, b in zip(mom[s], mom2[s]):
            assert np.allclose(a[0], b[0], rtol=1e-10, atol=1e-12) and np.allclose(a[1], b[1], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("p", [32, 40])
def test_moments_bad_and_constant_beliefs_in_the_lds_classes(P, p):
    """The wavefront class (clusters of 32 / 64 variables) and the workgroup class (80): a belief that is not positive
    definite (info = its first bad pivot) and an all-zero belief among good ones, every other belief untouched."""
    prob, cgb = _synth_tree(P, 10, p, 50 + p)
    dims = _dims(cgb)
    allb = list(range(cgb.nbeliefs))
    rc, base, _ = _moments_raw(cgb, allb, 0, 1, 1)
    assert rc == 0
    big = [b for b in allb if dims[b] == 2 * p]
    bad, zb = big[0], big[1]
    m = 2 * p
    Jb = 2.0 * np.eye(m)
    Jb[m - 3, m - 2] = Jb[m - 2, m - 3] = 2.5          # pivot m - 1 (1-based) is 2 - 2.5^2 / 2 < 0
    _set_record(cgb, 0, bad, Jb, np.ones(m), 0.0)
    _set_record(cgb, 0, zb, np.zeros((m, m)), np.zeros(m), 1.25)
    rc, out, info = _moments_raw(cgb, allb, 0, 1, 1)
    assert rc == 0
    got, was = _split(out[0], dims, allb, 1), _split(base[0], dims, allb, 1)
    for b in allb:
        mu, Sig, norm = got[b]
        if b == bad:
            assert info[0, b] == m - 1 and np.all(np.isnan(mu)) and np.all(np.isnan(Sig)) and np.isnan(norm)
        elif b == zb:
            assert info[0, b] == 0 and np.all(np.isposinf(mu)) and np.all(np.isnan(Sig)) and norm == 1.25
        else:
            assert info[0, b] == 0 and np.array_equal(mu, was[b][0]) and np.array_equal(Sig, was[b][1]) and norm == was[b][2]
    _assert_same_as_integrate(cgb)


def test_moments_muller_cliquetree_two_traits(P):
    """The clique tree of the Mueller et al. network at 2 traits: ragged dimensions from 2 to 108 variables, every class in
    one call, different dimensions under one LDS size inside the workgroup-class launch."""
    import os
    from helpers import network_from_newick_file
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "muller_2022.phy")
    net, names, _, _ = network_from_newick_file(P, path)
    tips = [names[i] for i in range(net.nnodes) if net.is_leaf[i]]
    p = 2
    cn, ed, sn = P.cliquetree(net.node2family)
    st = P.allocate_scopes(cn, ed, sn, net, p)
    row = {t: r for r, t in enumerate(tips)}
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], p)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    rng = np.random.default_rng(8)
    cgb.lg_setup(fam, rng.standard_normal((len(tips), p)))
    cgb.assignfactors_lg_(np.array([[[1.0, 0.3], [0.3, 2.0]]]), np.zeros(p), sync=True)
    spt = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    assert P.calibrate_(cgb, [spt])[0]
    dims = _dims(cgb)
    blockclass = sorted({d for d in dims if 64 < d <= 128})
    assert len(blockclass) >= 2 and max(dims) <= 128, sorted(set(dims))
    mom, lst, dims = _assert_same_as_integrate(cgb)
    assert _assert_covariances(cgb, mom, lst, dims) >= len(cn)

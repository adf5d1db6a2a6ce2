"""Painted optima under OU on the device: pgbp_lg_set_optima / set_optima_lg, the displacement correction of the factor fill
(csrc/pgbp_shift.hip, and the tip-noise and per-site-mask corrections), pgbp_lg_gradient_optima, the lanes-are-sites
pgbp_lg_gradient_sites_optima, the refusals of the sweeps that do not honour the optima, and fit_sites_lg(optima0=...).

Comparators (tests/optima_ref.py, pinned on the host in test_optima_cpu.py): shift_ref.ShiftedModel around the oracle's OU
with the equivalent shifts -- as belief propagation record by record and densely --, the numpy statement of doptima, dtheta
and dalpha over the dense posterior, the GLS statement of the optima, and a SECOND ENGINE that carries the equivalent
explicit shifts and no optima, with the chain rule through edge_gradient_lg's dshift.  The oracle's OU is univariate: at
p > 1 (plain, packed, missing data) the second engine is the comparator.  Every comparison at 1e-8 relative to
max(1, |block|); the measured figure of every case is printed."""
import numpy as np
import pytest

import loo_ref as LR
import optima_ref as OR
from helpers import oracle_setup
from oracle import densemvn as OD
from oracle import models as OM
from test_gpu_gradient_sites import _layout, _oracle_tree, _synth_engine, _tree_with_families
from test_gpu_shifts import _bytes, _device, _records_error, _tree_case

pytestmark = pytest.mark.gpu
TOL = 1e-8
BLOCKS = ("dR", "dmu", "dalpha", "dtheta", "doptima")


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _rel(got, want):
    got, want = np.atleast_1d(np.asarray(got, float)), np.atleast_1d(np.asarray(want, float))
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))


def _ou(net_case, root, seed=3):
    """The univariate OU on a golden network (its first trait), with each kind of root."""
    net, _, tbl, taxa = net_case
    rng = np.random.default_rng(seed)
    v = {"fixed": 0.0, "random": 0.8, "improper": np.inf}[root]
    return net, OM.UnivariateOrnsteinUhlenbeck(rng.uniform(0.5, 2), rng.uniform(0.3, 1), rng.normal(), rng.normal(), v), tbl[:1], taxa


N_REG = 3                       # regimes 1 and 3 are carried by edges, regime 2 by none
VALUES = np.array([1.7, -4.0, -0.9])


def _paint(net):
    reg = OR.paint(net, 4, N_REG, unused=2)
    assert {1, 3} <= set(reg.values()) and 2 not in reg.values()
    hyb = [n for n in net.vec_node[1:] if len(net.parent_edges(n)) >= 2]
    if hyb:   # a hybrid family whose two parent edges carry different regimes
        a, b = net.parent_edges(hyb[0])[:2]
        assert reg[a.number] != reg[b.number] and reg[a.number] > 0
    return reg


def _chain(fam, regime, values, alpha, theta, g, eg):
    """The painted gradient from an engine with the equivalent EXPLICIT shifts: g = its gradient_lg, eg = its
    edge_gradient_lg.  The derivative in the shift of edge (f, k) is gamma_k dshift[f], and the shift is
    (1 - a)(theta_r - theta), a = exp(-alpha t)."""
    nf = len(fam["cluster"])
    K = max(1, int(fam["max_parents"]))
    length, gamma = (np.asarray(fam[k], float).reshape(nf, K) for k in ("length", "gamma"))
    values, theta = np.asarray(values, float), np.asarray(theta, float).reshape(-1)
    out = dict(dR=g["dR"], dmu=g["dmu"], dalpha=float(g["dalpha"]), dtheta=np.array(g["dtheta"], float), doptima=np.zeros_like(values))
    for f in range(nf):
        for k in range(int(fam["n_parents"][f])):
            r = int(regime[f, k])
            if r > 0:
                a = np.exp(-alpha * length[f, k])
                gs = gamma[f, k] * np.nan_to_num(eg["dshift"][f])
                out["doptima"][r - 1] += (1 - a) * gs
                out["dtheta"] -= (1 - a) * gs
                out["dalpha"] += length[f, k] * a * float((values[r - 1] - theta) @ gs)
    return out


def _worst(tag, got, want, keys=BLOCKS):
    worst = max(_rel(got[k], want[k]) for k in keys)
    print(f"{tag}: worst block {worst:.2e}")
    return worst


# ----------------------------------------------------------------------------- 1: general engine, p = 1 on the golden networks

@pytest.mark.parametrize("graph", ["cliquetree", "bethe", "joingraph"])
@pytest.mark.parametrize("root", ["fixed", "random", "improper"])
@pytest.mark.parametrize("name", ["level1_1trait", "mateescu", "optimization_level1", "sun2023"])
def test_fill_reference_networks(P, name, root, graph):
    """Every cluster's (J, h, g) against the oracle's assignfactors of the wrapper; on the clique tree loglik_lg against the
    dense wrapper as well."""
    net, model, tbl, taxa = _ou(LR.reference_case(name, root), root)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa, graph, assign=False)
    reg = _paint(net)
    regime = OR.device_regime(net, ocgb, fam, reg)
    pcgb.set_optima_lg(regime, VALUES)
    assert pcgb.optima_count_lg() == N_REG and np.array_equal(pcgb.optima_lg()["regime"], regime)
    pcgb.assignfactors_lg_(**kw)
    w = OR.painted_model(model, net, reg, VALUES)
    err = _records_error(pcgb, oracle_setup(net, cg, w, tbl, taxa))
    plain = _records_error(pcgb, ocgb)
    print(f"{name}/{root}/{graph}: records vs the oracle's {err:.2e} (vs the unpainted {plain:.2e})")
    assert err <= TOL and plain > 1e-3
    if graph == "cliquetree":
        pcgb._ensure_schedule([spt])
        ll, info = pcgb.loglik_lg()
        dense = OD.loglik(net, w, tbl, taxa)
        assert info[0] == 0 and abs(ll[0] - dense) <= TOL * max(1.0, abs(dense))


@pytest.mark.parametrize("which", ["ou_fixed", "ou_random", "ou_improper"])
def test_gradient_statement_and_chain_rule(P, which):
    """24 tips, 6 hybrid nodes.  gradient_lg's blocks against the numpy statement over the dense posterior (a proper or fixed
    root) and against the chain rule through edge_gradient_lg's dshift on a second engine with the explicit shifts."""
    net, model, tbl, taxa = LR.random_case(which, 1)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    reg = _paint(net)
    regime = OR.device_regime(net, ocgb, fam, reg)
    pcgb.set_optima_lg(regime, VALUES)
    pcgb.assignfactors_lg_(**kw)   # (the setter refills nothing)
    ll, got = pcgb.loglik_and_gradient_lg(spt)
    assert got["doptima"].shape == (N_REG, 1) and not got["doptima"][1].any() and got["doptima"][0, 0] != 0
    w = OR.painted_model(model, net, reg, VALUES)
    dense = OD.loglik(net, w, tbl, taxa)
    assert abs(ll - dense) <= TOL * max(1.0, abs(dense))
    if which != "ou_improper":
        st = OR.dense_statement(net, model, reg, VALUES, tbl, taxa)
        st["doptima"] = st["doptima"][:, None]
        st["dR"] = np.asarray(st["dR"]).reshape(got["dR"].shape)
        assert _worst(f"{which}: gradient_lg vs the dense statement", got, st) <= TOL
    # the explicit-shift engine
    _, _, other, _, _, spt2 = _device(P, net, model, tbl, taxa)
    edges, sv = OR.explicit_shifts(fam, regime, VALUES[:, None], model.alpha, [model.theta])
    other.set_shifts_lg(edges, sv)
    other.assignfactors_lg_(**kw)
    ll2, g2 = other.loglik_and_gradient_lg(spt2)
    assert "doptima" not in g2 and abs(ll2 - ll) <= TOL * max(1.0, abs(ll))
    want = _chain(fam, regime, VALUES[:, None], model.alpha, [model.theta], g2, other.edge_gradient_lg())
    assert _worst(f"{which}: gradient_lg vs the chain rule on the explicit-shift engine", got, want) <= TOL
    assert abs(got["dalpha"] - g2["dalpha"]) > 1e-6   # (dalpha of the imitation does not know that the shift moves)
    # two calls, the same bytes
    again = pcgb.gradient_lg()
    assert all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in BLOCKS)


# ----------------------------------------------------------------------------- 2: p > 1 -- plain, packed, missing data

def _ou_kw(kw, p, seed):
    rng = np.random.default_rng(seed)
    out = dict(kw)
    out.update(model="ou", alpha=float(rng.uniform(0.4, 1.2)), theta=rng.normal(size=p))
    return out


def _regime_of_table(fam, seed, n_reg=N_REG, unused=2):
    nf, K = len(fam["cluster"]), max(1, int(fam["max_parents"]))
    rng = np.random.default_rng(seed)
    pool = [r for r in range(n_reg + 1) if r != unused]
    m = np.zeros((nf, K), np.int32)
    for f in range(nf):
        m[f, : int(fam["n_parents"][f])] = rng.choice(pool, size=int(fam["n_parents"][f]))
    hyb = [f for f in range(nf) if fam["n_parents"][f] >= 2]
    if hyb:
        m[hyb[0], :2] = (1, 3)
    assert {1, 3} <= set(m.reshape(-1).tolist())
    return m


@pytest.mark.parametrize("p,layout", [(2, 0), (2, 1), (16, 1), (3, 0)])
def test_layouts_against_the_explicit_shift_engine(P, p, layout):
    """A 12-tip tree at p = 2 (plain right after the set-up; packed after a calibration), p = 16 (packed) and p = 3 (plain):
    records, loglik_lg and every block of gradient_lg against a second engine that carries the equivalent explicit shifts."""
    case = lambda: _tree_case(P, p, 40 + p)
    tree, model, tbl, A, spt, kw, *_ = case()
    B = case()[3]
    fam = A._lg
    fam = dict(fam, max_parents=fam["length"].size // len(fam["cluster"]))
    okw = _ou_kw(kw, p, 50 + p)
    regime = _regime_of_table(fam, 60 + p)
    values = np.random.default_rng(70 + p).normal(size=(N_REG, p)) * 2.0
    edges, sv = OR.explicit_shifts(fam, regime, values, okw["alpha"], okw["theta"])
    for eng in (A, B):
        eng.assignfactors_lg_(**okw)
        if layout:
            eng.loglik_and_gradient_lg(spt)   # (a calibration: the engine takes the layout its kernels want)
        assert eng._lib.pgbp_layout(eng._eng) == layout, (p, eng._lib.pgbp_layout(eng._eng))
    A.set_optima_lg(regime, values)
    B.set_shifts_lg(edges, sv)
    recs = []
    for eng in (A, B):
        eng.assignfactors_lg_(**okw)
        assert eng._lib.pgbp_layout(eng._eng) == layout
        eng.pull()
        recs.append(eng._packed_raw.copy())
    e0 = _rel(recs[0], recs[1])
    llA, gA = A.loglik_and_gradient_lg(spt)
    llB, gB = B.loglik_and_gradient_lg(spt)
    want = _chain(fam, regime, values, okw["alpha"], okw["theta"], gB, B.edge_gradient_lg())
    print(f"p={p} layout {layout}: records {e0:.2e}, loglik {abs(llA - llB) / max(1.0, abs(llB)):.2e}")
    assert e0 <= TOL and abs(llA - llB) <= TOL * max(1.0, abs(llB))
    assert _worst(f"p={p} layout {layout}: gradient_lg vs the chain rule", gA, want) <= TOL
    assert np.all(gA["doptima"][[0, 2]] != 0) and not gA["doptima"][1].any()


def test_missing_data_network_against_the_explicit_shift_engine(P):
    """p = 3 on a network with 30 % of the values missing: a painted family keeps fewer than p components."""
    net, model, tbl, taxa = LR.missing_case()
    cg, ocgb, A, fam, kw, spt = _device(P, net, model, tbl, taxa)
    B = _device(P, net, model, tbl, taxa)[2]
    okw = _ou_kw(kw, 3, 81)
    regime = _regime_of_table(fam, 82)
    values = np.random.default_rng(83).normal(size=(N_REG, 3)) * 2.0
    edges, sv = OR.explicit_shifts(fam, regime, values, okw["alpha"], okw["theta"])
    A.set_optima_lg(regime, values)
    B.set_shifts_lg(edges, sv)
    recs = []
    for eng in (A, B):
        eng.assignfactors_lg_(**okw)
        eng.pull()
        recs.append(eng._packed_raw.copy())
    llA, gA = A.loglik_and_gradient_lg(spt)
    llB, gB = B.loglik_and_gradient_lg(spt)
    want = _chain(fam, regime, values, okw["alpha"], okw["theta"], gB, B.edge_gradient_lg())
    e0 = _rel(recs[0], recs[1])
    print(f"missing p=3: records {e0:.2e}, loglik {abs(llA - llB) / max(1.0, abs(llB)):.2e}")
    assert e0 <= TOL and abs(llA - llB) <= TOL * max(1.0, abs(llB))
    assert _worst("missing p=3: gradient_lg vs the chain rule", gA, want) <= TOL


# ----------------------------------------------------------------------------- 3: the batch, lanes = sites

def _node_regimes(tree, n_reg, unused, seed):
    rng = np.random.default_rng(seed)
    pool = [r for r in range(n_reg + 1) if r != unused]
    nr = rng.choice(pool, size=tree.nnodes)
    for i, r in enumerate([r for r in pool if r > 0]):
        nr[1 + i] = r   # (every painted regime of the pool is carried)
    nr[0] = 0
    return nr.astype(np.int32)


def _ou_batch(P, n_fam, ns, seed):
    from pgbp_amd import synth
    rng = np.random.default_rng(seed)
    tree = _tree_with_families(n_fam)
    alpha, gam2 = rng.uniform(0.3, 1.5, ns), rng.uniform(0.5, 2.0, ns)
    theta, mu = rng.normal(size=ns), rng.normal(size=ns)
    X = synth.simulate_ou_uni_sites(tree, 2 * alpha * gam2, alpha, theta, mu, rng)
    cgb, spt, fam = _synth_engine(P, tree, X)
    kw = dict(R=gam2[:, None, None, None], mu=mu[:, None], model="ou", alpha=alpha, theta=theta[:, None])
    return tree, X, cgb, spt, fam, kw


def _site_values(values, s):
    return values[s] if values.ndim == 3 else values


def _explicit_batch(fam, regime, values, kw, ns):
    """per-site explicit shifts [ns, n_edges, 1] of a batch (values shared [n, 1] or per site [ns, n, 1])"""
    per = [OR.explicit_shifts(fam, regime, _site_values(values, s), kw["alpha"][s], kw["theta"][s]) for s in range(ns)]
    return per[0][0], np.stack([v for _, v in per])


def _batch_checks(P, tag, A, B, sptA, sptB, fam, regime, values, kw, ns, dense_site=None, general=True, own=None):
    """A: the painted engine (set, not yet filled); B: a twin without optima.  gradient_sites_lg of A at every site against
    the general call on the same beliefs and against the chain rule on B under the explicit shifts; at one site in eight
    against the dense statement.  own: (edges, values [ns, n, 1]) of shifts that A carries besides its optima."""
    A.assignfactors_lg_(**kw)
    ll, got = A.loglik_and_gradient_sites_lg(sptA)
    n_reg = got["doptima"].shape[1]
    assert got["doptima"].shape == (ns, n_reg, 1) and not got["info"].any()
    assert bool(_layout(A) & 2) == (ns >= 64)
    edges, sv = _explicit_batch(fam, regime, values, kw, ns)
    if own is not None:   # (a shift of the case's own on a painted edge adds to the explicit one)
        allv = {e: v for e, v in zip(edges, np.moveaxis(sv, 1, 0))}
        for e, v in zip(own[0], np.moveaxis(own[1], 1, 0)):
            allv[e] = allv.get(e, 0.0) + v
        edges = sorted(allv)
        sv = np.stack([allv[e] for e in edges], axis=1)
    B.set_shifts_lg(edges, sv)
    B.assignfactors_lg_(**kw)
    llB, gB = B.loglik_and_gradient_sites_lg(sptB)
    eB = B.edge_gradient_sites_lg()
    assert np.max(np.abs(ll - llB) / np.maximum(1.0, np.abs(llB))) <= TOL
    worst = 0.0
    for s in range(ns):
        gs = {k: gB[k][s] for k in ("dR", "dmu", "dalpha", "dtheta")}
        want = _chain(fam, regime, _site_values(values, s), kw["alpha"][s], kw["theta"][s], gs, dict(dshift=eB["dshift"][s]))
        worst = max(worst, max(_rel(got[k][s], want[k]) for k in BLOCKS))
    print(f"{tag}: every site vs the chain rule on the explicit-shift engine {worst:.2e}")
    assert worst <= TOL
    if dense_site is not None:
        worst = 0.0
        for s in range(0, ns, 8):
            st, dense = dense_site(s)
            worst = max(worst, abs(ll[s] - dense) / max(1.0, abs(dense)),
                        max(_rel(np.ravel(got[k][s]), np.ravel(st[k])) for k in BLOCKS))
        print(f"{tag}: one site in eight vs the dense statement {worst:.2e}")
        assert worst <= TOL
    if general:   # (last: it moves the pool to the plain layout)
        ref = A.gradient_lg(all_sites=True)
        worst = max(_rel(got[k][s], ref[k][s]) for k in BLOCKS for s in range(ns))
        print(f"{tag}: every site vs gradient_lg on the same beliefs {worst:.2e}")
        assert worst <= TOL and not ref["info"].any()
    return got


@pytest.mark.parametrize("n_fam,ns,n_reg,per_site", [(63, 8, 1, False), (64, 64, 4, True), (65, 65, 5, True), (130, 257, 5, False)])
def test_batch_on_trees(P, n_fam, ns, n_reg, per_site):
    """Trees of 63 / 64 / 65 / 130 families (one, one, two and three family blocks) at 8 (plain), 64, 65 and 257 sites; 1, 4
    and 5 regimes (5: two launches of the painted instance), one of them carried by no edge where there are several; shared
    and per-site optima."""
    tree, X, A, spt, fam, kw = _ou_batch(P, n_fam, ns, 100 + n_fam)
    _, _, B, sptB, _, _ = _ou_batch(P, n_fam, ns, 100 + n_fam)
    unused = 2 if n_reg > 1 else None
    node_reg = _node_regimes(tree, n_reg, unused, 200 + n_fam)
    regime = node_reg[1:, None].copy()   # (family f of synth's table is node f + 1, one parent)
    rng = np.random.default_rng(300 + n_fam)
    values = rng.normal(size=(ns, n_reg, 1) if per_site else (n_reg, 1)) * 2.0
    A.set_optima_lg(regime, values)
    net, taxa, tipnode = _oracle_tree(tree)
    ereg = {e.number: int(node_reg[int(e.child.name[1:])]) for e in net.edges}

    def dense_site(s):
        m = OM.UnivariateOrnsteinUhlenbeck(2 * kw["alpha"][s] * kw["R"][s, 0, 0, 0], kw["alpha"][s], kw["theta"][s, 0], kw["mu"][s, 0], None)
        tbl = [[float(X[s, i]) for i in tipnode]]
        v = _site_values(values, s)[:, 0]
        st = OR.dense_statement(net, m, ereg, v, tbl, taxa)
        return st, OD.loglik(net, OR.painted_model(m, net, ereg, v), tbl, taxa)
    got = _batch_checks(P, f"{n_fam} families/{ns} sites/{n_reg} regimes", A, B, spt, sptB, fam, regime, values, kw, ns, dense_site)
    if unused:
        assert not got["doptima"][:, unused - 1].any()
    assert np.all(got["doptima"][:, 0] != 0)


@pytest.mark.parametrize("name", ["N1", "N2", "N3", "N4"])
def test_batch_on_hybrid_tip_networks(P, name):
    """The four networks of uni_net_ref (two-parent families, 0-variable clusters), fixed root, 65 sites, the two parent edges
    of a hybrid tip in different regimes, per-site optima."""
    import uni_net_ref as N
    ns = 65
    a, b = (N.device_batch(P, name, "fixed", "ou", "cliquetree", ns, assign=False) for _ in range(2))
    reg = OR.paint(a.net, 5, 2)
    hyb = next(n for n in a.net.vec_node[1:] if len(a.net.parent_edges(n)) >= 2)
    assert len({reg[e.number] for e in a.net.parent_edges(hyb)[:2]}) == 2
    regime = OR.device_regime(a.net, a.ocgb0, a.fam, reg)
    values = np.random.default_rng(6).normal(size=(ns, 2, 1)) * 2.0
    a.pcgb.set_optima_lg(regime, values)
    kw = dict(a.kw, alpha=np.asarray(a.kw["alpha"], float), theta=np.asarray(a.kw["theta"], float).reshape(ns, 1))

    def dense_site(s):
        m, tbl = a.sites[s]
        st = OR.dense_statement(a.net, m, reg, values[s, :, 0], tbl, a.taxa)
        return st, OD.loglik(a.net, OR.painted_model(m, a.net, reg, values[s, :, 0]), tbl, a.taxa)
    _batch_checks(P, f"{name}/65 sites", a.pcgb, b.pcgb, a.sched[0], b.sched[0], a.fam, regime, values, kw, ns, dense_site)


def test_batch_with_shifts_tip_noise_and_site_mask(P):
    """Optima together with shifts and tip noise (against the general call and the explicit-shift twin), then with a per-site
    mask of missing tips on top (the general call refuses a mask: the explicit-shift twin alone)."""
    ns, n_fam = 65, 64
    tree, X, A, spt, fam, kw = _ou_batch(P, n_fam, ns, 400)
    _, _, B, sptB, _, _ = _ou_batch(P, n_fam, ns, 400)
    node_reg = _node_regimes(tree, 4, 2, 401)
    regime = node_reg[1:, None].copy()
    rng = np.random.default_rng(402)
    values = rng.normal(size=(ns, 4, 1)) * 2.0
    tips = np.flatnonzero(np.asarray(fam["child_pos"]) < 0)
    own_edges = [(int(tips[0]), 0), (int(n_fam // 2), 0), (int(tips[-1]), 0)]
    own_vals = rng.normal(size=(ns, 3, 1))
    sig = rng.uniform(0.1, 0.5, size=(ns, 1, 1))
    for eng in (A, B):
        eng.set_tip_noise_lg(tips[::2], sig)
    A.set_shifts_lg(own_edges, own_vals)
    own = (own_edges, own_vals)
    A.set_optima_lg(regime, values)
    got = _batch_checks(P, "optima + shifts + noise", A, B, spt, sptB, fam, regime, values, kw, ns, own=own)
    assert "dsigma_e" in got
    mask = np.zeros((ns, tree.nnodes), bool)
    mask[np.arange(ns), np.flatnonzero(tree.is_leaf)[np.arange(ns) % int(tree.is_leaf.sum())]] = True
    for eng in (A, B):
        eng.set_site_missing_lg(mask)
    _batch_checks(P, "optima + shifts + noise + mask", A, B, spt, sptB, fam, regime, values, kw, ns, general=False, own=own)


# ----------------------------------------------------------------------------- 4: determinism, inertness, refusals

def _raw(cgb, a, b, n_reg):
    from pgbp_amd import _lib as L
    n = b - a
    out = [np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((n, n_reg))]
    info = np.ones(n, np.int32)
    rc = cgb._lib.pgbp_lg_gradient_sites_optima(cgb._eng, a, b, L.f64p(out[0]), L.f64p(out[1]), L.f64p(out[2]), L.f64p(out[3]),
                                                None, L.f64p(out[4]), L.i32p(info))
    assert rc == L.PGBP_OK, cgb._lib.pgbp_last_error(cgb._eng)
    return out + [info]


def test_equal_bytes_for_calls_ranges_chunks_and_layouts(P):
    """300 sites, 130 families, 5 regimes with per-site values: two calls; the ranges split at 37 and 130; one workgroup's
    sites per chunk; the site-minor and the plain instance -- the same bytes in every output, and the pool untouched."""
    ns, n_reg = 300, 5
    tree, X, A, spt, fam, kw = _ou_batch(P, 130, ns, 500)
    regime = _node_regimes(tree, n_reg, 2, 501)[1:, None].copy()
    A.set_optima_lg(regime, np.random.default_rng(502).normal(size=(ns, n_reg, 1)))
    A.assignfactors_lg_(**kw)
    ll, got = A.loglik_and_gradient_sites_lg(spt)
    assert _layout(A) == 2
    full = _raw(A, 0, ns, n_reg)
    again = _raw(A, 0, ns, n_reg)
    parts = [_raw(A, a, b, n_reg) for a, b in ((0, 37), (37, 130), (130, ns))]
    A._lib.pgbp_sites_sweep_scratch_limit(1)
    try:
        cut = _raw(A, 0, ns, n_reg)
    finally:
        A._lib.pgbp_sites_sweep_scratch_limit(0)
    for i, f in enumerate(full):
        assert f.tobytes() == again[i].tobytes() == cut[i].tobytes(), i
        assert f.tobytes() == np.concatenate([q[i] for q in parts]).tobytes(), i
    assert full[4].tobytes() == got["doptima"].tobytes() and np.all(full[4][:, [0, 2, 3, 4]] != 0) and not full[4][:, 1].any()
    assert _layout(A) == 2
    A.pull()              # (the transfer moves the pool to the plain layout, an exact copy)
    after = A._packed_raw.copy()
    assert _layout(A) == 0
    plain = _raw(A, 0, ns, n_reg)
    for i, f in enumerate(full):
        assert f.tobytes() == plain[i].tobytes(), i
    A.pull()
    assert np.array_equal(after, A._packed_raw)


def test_set_clear_bm_and_survival(P):
    """Set-then-clear and a BM fill give the bytes of an engine that never had optima; the setting survives set_edges_lg and
    set_shifts_lg, a new lg_setup clears it; a following calibration keeps its bytes."""
    net, model, tbl, taxa = LR.random_case("ou_random", 1)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    never = _device(P, net, model, tbl, taxa)[2]
    base = _bytes(never)
    ll0, g0 = never.loglik_and_gradient_lg(spt)
    regime = OR.device_regime(net, ocgb, fam, _paint(net))
    pcgb.set_optima_lg(regime, VALUES)
    pcgb.assignfactors_lg_(**kw)
    painted = _bytes(pcgb)
    assert painted != base
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == painted                       # the same bytes on every call
    pcgb.set_edges_lg(length=fam["length"], gamma=fam["gamma"])
    pcgb.set_shifts_lg([(int(np.flatnonzero(np.asarray(fam["n_parents"]) >= 1)[0]), 0)], np.ones((1, 1)))
    pcgb.clear_shifts_lg()
    assert pcgb.optima_count_lg() == N_REG
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == painted
    # BM: the optima have no effect; the gradient runs, doptima = 0, every other byte is the unpainted engine's
    bm = dict(R=kw["R"], mu=kw["mu"])
    pcgb.assignfactors_lg_(**bm)
    never.assignfactors_lg_(**bm)
    assert _bytes(pcgb) == _bytes(never)
    llb, gb = pcgb.loglik_and_gradient_lg(spt)
    lln, gn = never.loglik_and_gradient_lg(spt)
    assert llb == lln and not gb["doptima"].any() and all(np.asarray(gb[k]).tobytes() == np.asarray(gn[k]).tobytes() for k in gn)
    pcgb.edge_gradient_lg(), pcgb.loo_lg()               # (under BM nothing refuses)
    # clear
    pcgb.clear_optima_lg()
    assert pcgb.optima_count_lg() == 0 and pcgb.optima_lg() is None
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == base
    ll1, g1 = pcgb.loglik_and_gradient_lg(spt)
    assert ll1 == ll0 and g1.keys() == g0.keys() and all(np.asarray(g1[k]).tobytes() == np.asarray(g0[k]).tobytes() for k in g0)
    # a new table
    pcgb.set_optima_lg(regime, VALUES)
    from helpers import lg_inputs_from_oracle
    pcgb.lg_setup(fam, lg_inputs_from_oracle(P, net, ocgb, model, tbl, taxa)[1])
    assert pcgb.optima_count_lg() == 0 and pcgb.optima_lg() is None


def test_refusals_leave_everything_untouched(P):
    """The setter's bad entries and every sweep that does not honour the optima: PGBP_ERR_INVALID with a text that names the
    reason; outputs, layout, pool and the setting in force as they were."""
    from pgbp_amd import _lib as L
    net, model, tbl, taxa = LR.random_case("ou_random", 1)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    regime = OR.device_regime(net, ocgb, fam, _paint(net))
    pcgb.set_optima_lg(regime, VALUES)
    pcgb.assignfactors_lg_(**kw)
    painted = _bytes(pcgb)
    ll, g = pcgb.loglik_and_gradient_lg(spt)
    pcgb.pull()
    pool, lay = pcgb._packed_raw.copy(), pcgb._lib.pgbp_layout(pcgb._eng)
    f_tree = int(np.flatnonzero(np.asarray(fam["n_parents"]) == 1)[0])
    K = max(1, int(fam["max_parents"]))
    for text, mod, vals in (("is not in 0 ..", N_REG + 1, VALUES), ("is not in 0 ..", -1, VALUES),
                            ("not finite", None, np.array([1.0, np.nan, 0.0])), ("not finite", None, np.array([np.inf, 0.0, 0.0]))):
        bad = regime.copy()
        if mod is not None:
            bad[f_tree, 0] = mod
        with pytest.raises(L.PgbpError) as ex:
            pcgb.set_optima_lg(bad, vals)
        assert ex.value.code == L.ERR_INVALID and text in ex.value.msg, ex.value.msg
        if mod is not None:
            assert f"entry {f_tree * K}" in ex.value.msg
    assert pcgb.optima_count_lg() == N_REG
    # the values-only update refuses a value that is not finite, and without optima
    with pytest.raises(L.PgbpError) as ex:
        pcgb.update_optima_lg(np.array([1.0, np.nan, 0.0]))
    assert ex.value.code == L.ERR_INVALID and "regime 2" in ex.value.msg, ex.value.msg
    # ... and after all these refused calls the PREVIOUS map and values are in force: a refill gives the bytes it gave, and the
    # calibration that follows the pool and the numbers it gave
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == painted
    ll1, g1 = pcgb.loglik_and_gradient_lg(spt)
    assert ll1 == ll and all(np.asarray(g1[k]).tobytes() == np.asarray(g[k]).tobytes() for k in g)
    pcgb.pull()
    assert np.array_equal(pool, pcgb._packed_raw)
    # entries of a root-prior family and of k >= n_parents are ignored
    loose = regime.copy()
    loose[np.asarray(fam["n_parents"]) == 0] = 99
    if K > 1:
        loose[f_tree, 1] = 99
    pcgb.set_optima_lg(loose, VALUES)

    def refused(call, *outs):
        with pytest.raises(L.PgbpError) as ex:
            call()
        assert ex.value.code == L.ERR_INVALID and "optima" in ex.value.msg, ex.value.msg
    for call in (pcgb.edge_gradient_lg, pcgb.loo_lg, pcgb.impute_lg, pcgb.shift_scan_lg):
        refused(call)
    # the C calls: the outputs keep their bytes
    n = 1
    out = [np.full(64, 7.0) for _ in range(4)]
    rc = pcgb._lib.pgbp_lg_gradient(pcgb._eng, 0, n, *[L.f64p(x) for x in out], None)
    assert rc == L.ERR_INVALID and b"pgbp_lg_gradient_optima" in pcgb._lib.pgbp_last_error(pcgb._eng)
    nf = len(fam["cluster"])
    eo = [np.full(nf * K, 7.0), np.full(nf * K, 7.0), np.full(nf, 7.0)]
    rc = pcgb._lib.pgbp_lg_edge_gradient(pcgb._eng, 0, n, *[L.f64p(x) for x in eo], None)
    assert rc == L.ERR_INVALID and b"optima" in pcgb._lib.pgbp_last_error(pcgb._eng)
    assert all(np.all(x == 7.0) for x in out + eo)
    assert pcgb._lib.pgbp_layout(pcgb._eng) == lay and pcgb.optima_count_lg() == N_REG
    pcgb.pull()
    assert np.array_equal(pool, pcgb._packed_raw)
    ll2, g2 = pcgb.loglik_and_gradient_lg(spt)
    assert ll2 == ll and all(np.asarray(g2[k]).tobytes() == np.asarray(g[k]).tobytes() for k in g)
    # no family table
    from helpers import product_beliefs_from_oracle
    bare = P.ClusterGraphBelief(product_beliefs_from_oracle(ocgb.belief), ocgb.node2cluster, ocgb.node2family, ocgb.node2fixed,
                                ocgb.cluster2nodes)
    assert bare._lib.pgbp_lg_set_optima(bare._eng, 1, L.i32p(np.zeros(4, np.int32)), L.f64p(np.ones(1)), 0) == L.ERR_STATE
    assert bare._lib.pgbp_lg_optima_count(bare._eng) == -1
    assert bare._lib.pgbp_lg_update_optima(bare._eng, L.f64p(np.ones(1))) == L.ERR_STATE
    never = _device(P, net, model, tbl, taxa)[2]
    assert never._lib.pgbp_lg_update_optima(never._eng, L.f64p(np.ones(3))) == L.ERR_STATE
    assert b"pgbp_lg_set_optima" in never._lib.pgbp_last_error(never._eng)


def test_sites_refusals_leave_everything_untouched(P):
    """The lanes-are-sites twins: gradient_sites without doptima, scan, edge gradient, leave-one-out, imputation."""
    from pgbp_amd import _lib as L
    ns = 64
    tree, X, A, spt, fam, kw = _ou_batch(P, 64, ns, 600)
    regime = _node_regimes(tree, 2, None, 601)[1:, None].copy()
    A.set_optima_lg(regime, np.array([1.0, -2.0]))
    A.assignfactors_lg_(**kw)
    ll, got = A.loglik_and_gradient_sites_lg(spt)
    A.pull()
    pool = A._packed_raw.copy()
    o = A._opts()
    import ctypes as C
    assert A._lib.pgbp_enqueue_calibrate(A._eng, 1, 1, C.byref(o)) == 0
    lay = _layout(A)
    out = [np.full(ns, 7.0) for _ in range(4)]
    rc = A._lib.pgbp_lg_gradient_sites(A._eng, 0, ns, *[L.f64p(x) for x in out], None, None)
    assert rc == L.ERR_INVALID and b"pgbp_lg_gradient_sites_optima" in A._lib.pgbp_last_error(A._eng)
    assert all(np.all(x == 7.0) for x in out)
    for call in (A.shift_scan_sites_lg, A.edge_gradient_sites_lg, A.loo_sites_lg, A.impute_sites_lg):
        with pytest.raises(L.PgbpError) as ex:
            call()
        assert ex.value.code == L.ERR_INVALID and "optima" in ex.value.msg, ex.value.msg
    assert _layout(A) == lay and A.optima_count_lg() == 2
    A.pull()
    assert np.array_equal(pool, A._packed_raw)


def _simulate_raw(cgb, write_data, seed=11):
    """pgbp_lg_simulate on every site with outputs preset to 7: (rc, message, x, z_out, info)"""
    from pgbp_amd import _lib as L
    ns, nf = cgb.n_sites, len(cgb._lg["cluster"])
    x, zo, info = np.full((ns, nf, 1), 7.0), np.full((ns, nf, 1), 7.0), np.full(ns, 7, np.int32)
    rc = cgb._lib.pgbp_lg_simulate(cgb._eng, 0, ns, None, seed, L.f64p(x), L.f64p(zo), int(write_data), L.i32p(info))
    return rc, cgb._lib.pgbp_last_error(cgb._eng), x, zo, info


def test_simulate_refusals_leave_everything_untouched(P):
    """pgbp_lg_simulate -- the one refused call that could write the engine's tip data -- without and with write_data, through
    simulate_lg, and through bootstrap_shift_scan_lg (general and lanes-are-sites), which simulates first: PGBP_ERR_INVALID
    naming the optima; x, z_out and info, the engine's data, the pool, the layout and the setting as they were.  Under BM
    the same engine simulates."""
    from pgbp_amd import _lib as L
    ns = 64
    tree, X, A, spt, fam, kw = _ou_batch(P, 64, ns, 700)
    assert "parent_family" in fam   # (the topology the simulation needs: its check comes before the optima's)
    regime = _node_regimes(tree, 2, None, 701)[1:, None].copy()
    A.set_optima_lg(regime, np.array([1.0, -2.0]))
    A.assignfactors_lg_(**kw)
    A.loglik_and_gradient_sites_lg(spt)
    data = A.get_data_lg()
    assert np.array_equal(data[:, :, 0], X)
    A.pull()
    pool = A._packed_raw.copy()
    lay = _layout(A)

    def untouched():
        assert np.array_equal(A.get_data_lg(), data) and A.optima_count_lg() == 2 and _layout(A) == lay
        A.pull()
        assert np.array_equal(pool, A._packed_raw)
    for write_data in (0, 1):
        rc, msg, x, zo, info = _simulate_raw(A, write_data)
        assert rc == L.ERR_INVALID and b"optima" in msg and b"pgbp_lg_simulate" in msg, (rc, msg)
        assert np.all(x == 7.0) and np.all(zo == 7.0) and np.all(info == 7)
        untouched()
        with pytest.raises(L.PgbpError) as ex:
            A.simulate_lg(seed=3, write_data=bool(write_data), all_sites=True)
        assert ex.value.code == L.ERR_INVALID and "optima" in ex.value.msg, ex.value.msg
        untouched()
    for sites in (False, True):
        with pytest.raises(L.PgbpError) as ex:
            P.bootstrap_shift_scan_lg(A, spt, seed=5, sites=sites)
        assert ex.value.code == L.ERR_INVALID and "optima" in ex.value.msg, ex.value.msg
        untouched()
    # under BM the optima have no effect and nothing refuses: the simulation runs and equals that of an engine without optima
    _, _, B, _, _, _ = _ou_batch(P, 64, ns, 700)
    bm = dict(R=kw["R"], mu=kw["mu"])
    A.assignfactors_lg_(**bm)
    B.assignfactors_lg_(**bm)
    xa, ia = A.simulate_lg(seed=3, all_sites=True)
    xb, ib = B.simulate_lg(seed=3, all_sites=True)
    assert xa.tobytes() == xb.tobytes() and not ia.any() and np.all(np.isfinite(xa))


def test_values_only_update_and_the_dict_form(P):
    """update_optima_lg after a setting with other values gives the bytes of the full setter with those values -- shared
    values on a network, per-site values of a batch (records and the lanes-are-sites gradient) --, and the dict form of
    set_optima_lg gives the dense map."""
    net, model, tbl, taxa = LR.random_case("ou_random", 1)
    cg, ocgb, pcgb, fam, kw, spt = _device(P, net, model, tbl, taxa)
    regime = OR.device_regime(net, ocgb, fam, _paint(net))
    pcgb.set_optima_lg(regime, VALUES)
    pcgb.assignfactors_lg_(**kw)
    painted = _bytes(pcgb)
    pcgb.set_optima_lg(regime, 3.0 * VALUES + 1.0)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) != painted
    pcgb.update_optima_lg(VALUES)
    assert np.array_equal(pcgb.optima_lg()["values"][:, 0], VALUES)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == painted
    # the dict: (family, k) pairs and flat indices f * K + k, every other edge 0
    K = max(1, int(fam["max_parents"]))
    pairs = [(int(f), int(k)) for f, k in zip(*np.nonzero(regime))]
    d = {(f, k) if i % 2 else f * K + k: int(regime[f, k]) for i, (f, k) in enumerate(pairs)}
    pcgb.clear_optima_lg()
    pcgb.set_optima_lg(d, VALUES)
    assert np.array_equal(pcgb.optima_lg()["regime"], regime)
    pcgb.assignfactors_lg_(**kw)
    assert _bytes(pcgb) == painted
    # per-site values of a univariate batch: the [regime][site] rows are updated too
    ns = 65
    tree, X, A, sptA, famA, kwA = _ou_batch(P, 64, ns, 800)
    _, _, B, sptB, _, _ = _ou_batch(P, 64, ns, 800)
    reg = _node_regimes(tree, 3, None, 801)[1:, None].copy()
    rng = np.random.default_rng(802)
    v0, v1 = rng.normal(size=(ns, 3, 1)), rng.normal(size=(ns, 3, 1))
    A.set_optima_lg(reg, v0)
    A.assignfactors_lg_(**kwA)
    A.update_optima_lg(v1[:, :, 0])
    B.set_optima_lg(reg, v1)
    out = []
    for eng, sp in ((A, sptA), (B, sptB)):
        eng.assignfactors_lg_(**kwA)
        ll, g = eng.loglik_and_gradient_sites_lg(sp)
        out.append((ll, g))
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert all(out[0][1][k].tobytes() == out[1][1][k].tobytes() for k in BLOCKS)
    assert _bytes(A) == _bytes(B)


# ----------------------------------------------------------------------------- 5: the fit

def test_fit_sites_with_two_painted_clades(P):
    """24 sites of a 96-tip tree, two clades painted (test_optima_cpu.fit_case).  Each site's log-likelihood is no worse than
    scipy's optimum of the dense painted log-likelihood by more than 1e-8 max(1, |loglik|); at the returned alpha and R the
    returned mu (fixed here), theta and optima satisfy the GLS normal equations to the stopping rule."""
    from test_optima_cpu import fit_case
    tree, net, taxa, tipnode, reg, node_reg, X, true = fit_case()
    ns = X.shape[0]
    cgb, spt, fam = _synth_engine(P, tree, X)
    cgb.set_optima_lg(node_reg[1:, None].copy(), np.zeros((2, 1)))
    tipmean = X[:, tree.is_leaf].mean(axis=1)
    gtol = 1e-8
    fit = P.fit_sites_lg(cgb, spt, "ou", np.ones(ns), true["mu"], alpha0=np.ones(ns), theta0=tipmean, fit_mu=False, gtol=gtol,
                         optima0=np.stack([tipmean, tipmean], axis=1))
    assert fit["optima"].shape == (ns, 2) and np.all(np.isfinite(fit["loglik"]))
    print("painted fit: evaluations", fit["n_device_evals"], "iterations", fit["n_iter"].min(), "..", fit["n_iter"].max(),
          "converged", int(fit["converged"].sum()))
    from scipy.optimize import minimize_scalar
    obs = [i for i, n in enumerate(net.vec_node) if n.leaf]
    n_obs = len(obs)
    # depth of every tip and of the last common ancestor of every two tips, in the order of obs
    tip_ids = [int(net.vec_node[i].name[1:]) for i in obs]
    depth = np.zeros(tree.nnodes)
    for i in range(1, tree.nnodes):
        depth[i] = depth[tree.parent[i]] + tree.length[i]
    anc = []
    for i in tip_ids:
        path, j = [], i
        while j >= 0:
            path.append(j)
            j = int(tree.parent[j])
        anc.append(path)
    sets = [set(a_) for a_ in anc]
    Tmrca = np.array([[depth[next(j for j in anc[a_] if j in sets[b_])] for b_ in range(n_obs)] for a_ in range(n_obs)])
    dtip = depth[tip_ids]
    worst_gap, worst_ne = -np.inf, 0.0
    for s in range(ns):
        tbl = [[float(v) for v in X[s, tipnode]]]
        y = np.array([X[s, int(net.vec_node[i].name[1:])] for i in obs])

        def profile(log_alpha):
            """the dense painted log-likelihood maximised in closed form over (theta, theta_1, theta_2) (GLS) and the
            stationary variance (r'C^-1 r / n) at this alpha: (-loglik, parameters).  Tips i, j of an OU on a tree with a
            fixed root: Cov = g2 exp(-alpha (d_i + d_j - 2 T_ij)) (1 - exp(-2 alpha T_ij)), T_ij the depth of their last
            common ancestor (checked against densemvn.loglik at the optimum below)"""
            al = float(np.exp(log_alpha))
            C1 = np.exp(-al * (dtip[:, None] + dtip[None, :] - 2 * Tmrca)) * (1.0 - np.exp(-2 * al * Tmrca))
            Dm = OR.tip_design(net, al, reg, 2)[obs]
            r0 = y - Dm[:, 0] * true["mu"][s]
            Lc = np.linalg.cholesky(C1)
            Xw, rw = np.linalg.solve(Lc, Dm[:, 1:]), np.linalg.solve(Lc, r0)
            b = np.linalg.lstsq(Xw, rw, rcond=None)[0]
            q = float(np.sum((rw - Xw @ b) ** 2))
            g2 = q / n_obs
            ll = -0.5 * (n_obs * np.log(2 * np.pi * g2) + 2 * float(np.sum(np.log(np.diag(Lc)))) + n_obs)
            return -ll, (g2, al, b)
        # a grid over log alpha first (the profile may have more than one local optimum), then scipy's bounded search
        # between the neighbours of the best grid point
        grid = np.linspace(np.log(1e-3), np.log(50.0), 41)
        k = int(np.argmin([profile(t)[0] for t in grid]))
        res = minimize_scalar(lambda t: profile(t)[0], bounds=(grid[max(k - 1, 0)], grid[min(k + 1, 40)]), method="bounded",
                              options={"xatol": 1e-12})
        ref, (g2, al, b) = -res.fun, profile(res.x)[1]
        m = OM.UnivariateOrnsteinUhlenbeck(2 * al * g2, al, b[0], true["mu"][s], None)
        dense = OD.loglik(net, OR.painted_model(m, net, reg, b[1:]), tbl, taxa)   # (the comparator's own closed form, checked)
        assert abs(dense - ref) <= 1e-10 * max(1.0, abs(ref)), (s, dense, ref)
        worst_gap = max(worst_gap, (ref - fit["loglik"][s]) / max(1.0, abs(ref)))
        # the GLS normal equations at the returned alpha and R
        m = OM.UnivariateOrnsteinUhlenbeck(2 * fit["alpha"][s] * fit["R"][s], fit["alpha"][s], fit["theta"][s], true["mu"][s], None)
        bhat, Xd, S, r0 = OR.gls_optima(net, m, reg, 2, tbl, taxa, free=(1, 2, 3))
        bf = np.array([fit["theta"][s], *fit["optima"][s]])
        score = Xd.T @ np.linalg.solve(S, r0 - Xd @ bf)
        worst_ne = max(worst_ne, float(np.max(np.abs(score))) / max(1.0, abs(fit["loglik"][s])))
    print(f"painted fit: worst deficit against scipy {worst_gap:.2e}, worst normal-equation residual / max(1, |loglik|) {worst_ne:.2e}")
    assert worst_gap <= 1e-8
    assert worst_ne <= gtol

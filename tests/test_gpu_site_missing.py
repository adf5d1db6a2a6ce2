"""Per-site missing tips of a univariate batch on the device: pgbp_lg_set_site_missing / set_site_missing_lg, the correction of
the factor fill (csrc/pgbp_sitemiss.hip), the lanes-are-sites sweeps under a mask, the refusals and fit_sites_lg.

Comparators, never the new code itself: at every site the numpy restatement of tests/site_missing_ref.py over the DENSE
posterior moments (pinned to the dense statements in test_site_missing_cpu.py, which also checks the margins these tests rely
on) and oracle.densemvn.loglik of the site's observed tips; at one site in eight (site 0 and the planted sites always) the
dense statements themselves and an engine set up with that site's pattern as a STATIC child_mask on the same cluster graph,
driven through the general calls -- a path that runs none of the new code.  Every comparison is asserted at 1e-8 relative to
max(1, |block|_inf); each test prints its worst figure."""
import ctypes as C

import numpy as np
import pytest

import fam_uni_ref as FR
import post_uni_ref as PU
import site_missing_ref as SM
import uni_net_ref as N
from helpers import lg_inputs_from_oracle, oracle_setup
from test_gpu_fam_uni import _engine, _layout, _own_top

pytestmark = pytest.mark.gpu
TOL = 1e-8
CASES = [(name, make, n) for name, make, counts in SM.sweep_cases() for n in counts]
IDS = [f"{c[0]}-{c[2]}" for c in CASES]


@pytest.fixture(scope="module")
def P():
    import pgbp_amd
    pgbp_amd.load()
    return pgbp_amd


def _rel(got, want):
    return FR.rel(got, want)


def _masked_engine(P, case, mask=True):
    """the engine of the complete data of the case's first n sites (test_gpu_fam_uni._engine: per-site parameters, shifts and
    noise in force) with the case's mask set and the factors assigned again"""
    cgb = _engine(P, case.base, case.n)
    if mask:
        cgb.set_site_missing_lg(case.mask)
        assert cgb.site_missing_count_lg() == int(case.mask.sum()) and np.array_equal(cgb.site_missing_lg(), case.mask)
    cgb.assignfactors_lg_(**cgb._fam_uni_kw, sync=True)
    return cgb


def _pools(cgb):
    """(belief pool, factor pool) [n_sites, doubles] after the last assignfactors_lg_"""
    cgb.pull()
    pool = cgb._packed_raw.copy()
    cgb.init_beliefs_reset_fromfactors_()
    cgb.pull()
    return pool, cgb._packed_raw.copy()


def _record(cgb, c):
    return slice(int(cgb._poff[c]), int(cgb._poff[c + 1]))


# ----------------------------------------------------------------------------- 1: the fill

@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fill_and_loglik(P, i):
    """loglik_lg of every site against densemvn.loglik of that site's observed tips; a lone masked tip's cluster record is +0.0
    in every entry, in pool and factor pool; the records of the (cluster, site) pairs without a masked family are the bytes of
    the same engine with no mask; after clearing the mask and refilling the whole pool is those bytes."""
    name, make, n = CASES[i]
    case = make(n)
    plain = _masked_engine(P, case, mask=False)
    pool0, fpool0 = _pools(plain)
    cgb = _masked_engine(P, case)
    pool, fpool = _pools(cgb)
    assert np.array_equal(pool, fpool)
    _, fam_of = SM.tip_rows(case)
    fcl = np.asarray(case.fam["cluster"])
    per_cluster = np.bincount(fcl, minlength=cgb.nclusters)
    touched = np.zeros((case.n, cgb.nclusters), bool)
    lone = 0
    for s, r in zip(*np.nonzero(case.mask)):
        c = int(fcl[fam_of[int(r)]])
        touched[s, c] = True
        if per_cluster[c] == 1:
            rec = pool[s, _record(cgb, c)]
            assert np.all(rec == 0.0) and not np.signbit(rec).any() and not np.signbit(fpool[s, _record(cgb, c)]).any(), (s, c)
            lone += 1
    assert lone > 0 or name.startswith("N")
    for c in range(cgb.nclusters):
        keep = ~touched[:, c]
        assert np.array_equal(pool[keep][:, _record(cgb, c)], pool0[keep][:, _record(cgb, c)]), c
        assert not np.array_equal(pool[~keep][:, _record(cgb, c)], pool0[~keep][:, _record(cgb, c)]) or not (~keep).any(), c
    cgb._ensure_schedule([case.spt])
    ll, info = cgb.loglik_lg()
    assert not info.any()
    want = np.array([SM.dense_loglik(case, s) for s in range(case.n)])
    worst = float(np.max(np.abs(ll - want) / np.maximum(1.0, np.abs(want))))
    print(f"{name}/{n}: loglik of {case.n} sites ({int(case.mask.sum())} masked entries, {lone} lone clusters) against densemvn {worst:.2e}")
    assert worst <= TOL
    assert bool(_layout(cgb) & 2) == (case.n >= 64)
    # (the data keep the 0.0 the setter stored: the wrapper wants the values back with the call that uncovers them)
    with pytest.raises(ValueError, match="uncovered"):
        cgb.set_site_missing_lg(None)
    assert cgb.site_missing_count_lg() == int(case.mask.sum())
    cgb.set_site_missing_lg(None, data=plain.get_data_lg())
    assert cgb.site_missing_count_lg() == 0 and not cgb.site_missing_lg().any()
    cgb.assignfactors_lg_(**cgb._fam_uni_kw, sync=True)
    back, fback = _pools(cgb)
    assert np.array_equal(back, pool0) and np.array_equal(fback, fpool0)


def test_placeholders(P):
    """Placeholder values of 0, 1, 1e300 and (through set_data_lg) NaN at the masked entries give the same bytes, in the pool
    and the factor pool; the setter itself zeroes what the set-up was given; with a mask in force set_data_lg still refuses a
    value that is not finite at an observed entry and leaves the data as they were."""
    case = SM.bm(65)
    cgb = _masked_engine(P, case)
    pool, fpool = _pools(cgb)
    data0 = cgb.get_data_lg()
    assert np.all(data0[case.mask] == 0.0)
    for val in (1e300, np.nan, 1.0):
        d = data0.copy()
        d[case.mask] = val
        cgb.set_data_lg(d)
        assert np.all(cgb.get_data_lg()[case.mask] == 0.0)
        cgb.assignfactors_lg_(**cgb._fam_uni_kw, sync=True)
        p2, f2 = _pools(cgb)
        assert np.array_equal(p2, pool) and np.array_equal(f2, fpool), val
    bad = data0.copy()
    s_, r_ = np.argwhere(~case.mask)[3]
    bad[s_, r_, 0] = np.nan
    with pytest.raises(P.PgbpError, match="per-site mask"):
        cgb.set_data_lg(bad)
    assert np.array_equal(cgb.get_data_lg(), data0)
    # the setter itself zeroes a placeholder: an engine set up with 1e300 at the gaps
    base = case.base
    import copy
    big = copy.copy(base)
    big.sites = [(m, [[1e300 if case.mask[s, r] else v for r, v in enumerate(tbl[0])]]) for s, (m, tbl) in enumerate(base.sites[:case.n])]
    other = _engine(P, big, case.n)
    other.set_site_missing_lg(case.mask)
    other.assignfactors_lg_(**other._fam_uni_kw, sync=True)
    p3, f3 = _pools(other)
    assert np.array_equal(p3, pool) and np.array_equal(f3, fpool)


def test_fill_on_a_bethe_graph(P):
    """The Bethe cluster graphs of N1 .. N4 (fill and loglik_lg; the sweeps are exact on a clique tree): a masked hybrid tip has two
    parents.  The records of the (cluster, site) pairs without a masked family keep the bytes of the engine with no mask, a
    lone masked tip's cluster is +0.0, and the factors of every site add up to the clique tree's: the sum of g over the
    clusters and the log-likelihood of a calibrated clique tree of the same mask are the dense one's (test_fill_and_loglik),
    so here the sum over the clusters of each record's g is compared between the two graphs -- the same families, filled by
    the same arithmetic in another grouping.  loglik_lg on the Bethe graph: _bethe_loglik below."""
    for name in ("N1", "N2", "N3", "N4"):
        hc = SM.hybrid(name, "bm", 65)
        out = {}
        n_ll = 0
        for kind in ("bethe", "cliquetree"):
            b = N.device_batch(P, name, "fixed", "bm", kind, 65)
            assert np.array_equal(b.fam["data_row"], hc.base.fam["data_row"]) and b.taxa == hc.taxa   # (hc.mask is indexed by these rows)
            b.pcgb.assignfactors_lg_(**b.kw, sync=True)
            pool0, _ = _pools(b.pcgb)
            b.pcgb.set_site_missing_lg(hc.mask)
            b.pcgb.assignfactors_lg_(**b.kw, sync=True)
            pool, fpool = _pools(b.pcgb)
            assert np.array_equal(pool, fpool)
            fcl = np.asarray(b.fam["cluster"])
            row_fam = {int(r): f for f, r in enumerate(b.fam["data_row"]) if r >= 0 and b.fam["child_pos"][f] < 0}
            touched = np.zeros((65, b.pcgb.nclusters), bool)
            for s, r in zip(*np.nonzero(hc.mask)):
                touched[s, int(fcl[row_fam[int(r)]])] = True
            gsum = np.zeros(65)
            for c in range(b.pcgb.nclusters):
                rec = _record(b.pcgb, c)
                assert np.array_equal(pool[~touched[:, c]][:, rec], pool0[~touched[:, c]][:, rec]), (name, kind, c)
                if np.sum(fcl == c) == 1:
                    assert np.all(pool[touched[:, c]][:, rec] == 0.0) and not np.signbit(pool[touched[:, c]][:, rec]).any()
                gsum += pool[:, rec.stop - 1]
            out[kind] = gsum
            if kind == "bethe":
                n_ll += _bethe_loglik(P, b, hc)
        err = float(np.max(np.abs(out["bethe"] - out["cliquetree"]) / np.maximum(1.0, np.abs(out["cliquetree"]))))
        print(f"{name}: sum of g over the clusters, Bethe against clique tree, 65 sites under a mask: {err:.2e}")
        assert err <= TOL
        assert n_ll == 3, (name, n_ll)   # (sites 0, 5 and 6 of all four keep the scopes of the complete data)


def _bethe_loglik(P, b, hc):
    """loglik_lg on the Bethe graph under the mask (one postorder pass of schedule tree 0 and the root integration: on a loopy
    graph an approximation, so the dense likelihood is no comparator) against a ONE-site engine with that site's pattern as
    the static child_mask on the same Bethe graph, through the general kernels -- at the sites 0, 5 (the hybrid tip masked)
    and 6 whose pattern the reference allocates with the scopes of the complete data, so that both engines do the same
    approximation.  Returns how many sites were compared."""
    from oracle.beliefupdates import BPPosDefException
    b.pcgb._ensure_schedule(b.sched)
    ll, info = b.pcgb.loglik_lg()
    assert not info.any() and np.all(np.isfinite(ll))
    full = [bb.dimension for bb in b.ocgb0.belief]
    done = 0
    for s in (0, 5, 6):
        model, tbl = hc.sites[s]
        try:
            ocgb = oracle_setup(b.net, b.cg, model, tbl, b.taxa)
        except BPPosDefException:
            continue
        if [bb.dimension for bb in ocgb.belief] != full:
            continue
        fam, data, kw = lg_inputs_from_oracle(P, b.net, ocgb, model, tbl, b.taxa)
        one = P.ClusterGraphBelief.from_arrays(*N.engine_arrays(P, ocgb), None, n_sites=1)
        one.lg_setup(fam, data[None])
        one.assignfactors_lg_(**kw)
        one._ensure_schedule(b.sched)
        l1, i1 = one.loglik_lg()
        assert not i1.any() and abs(ll[s] - l1[0]) <= TOL * max(1.0, abs(l1[0])), (s, ll[s], l1[0])
        done += 1
    return done


# ----------------------------------------------------------------------------- 2: calibrated state and sweeps

def _static_engine(P, case, s):
    """an engine of ONE site with the pattern of site s as the static child_mask of pgbp_lg_setup, on the same cluster graph:
    the general kernels, none of the new code.  None when the reference's allocation does not take the pattern: a clade
    without data inside a clade without data leaves it a belief it cannot integrate (BPPosDefException in its assignfactors)."""
    from oracle.beliefupdates import BPPosDefException
    model, tbl = case.sites[s]
    try:
        ocgb = oracle_setup(case.net, case.cg, model, tbl, case.taxa)
    except BPPosDefException:
        return None
    fam, data, kw = lg_inputs_from_oracle(P, case.net, ocgb, model, tbl, case.taxa)
    dims, sepcl, so, si = N.engine_arrays(P, ocgb)
    cgb = P.ClusterGraphBelief.from_arrays(dims, sepcl, so, si, None, n_sites=1)
    cgb.lg_setup(fam, data[None])
    cgb.assignfactors_lg_(**kw)
    return cgb, fam


def _site(got, s):
    """site s of the device dicts in site_missing_ref.reference_site's layout"""
    return dict(scan=dict(jump=got["scan"]["jump"][s, :, 0], lr=got["scan"]["lr"][s], identified=got["scan"]["identified"][s, :, 0],
                          H=got["scan"]["H"][s, :, 0, 0], top_lr=got["scan"]["top_lr"][s], top_family=got["scan"]["top_family"][s]),
                edge=dict(dlength=got["edge"]["dlength"][s], dgamma=got["edge"]["dgamma"][s], dshift=got["edge"]["dshift"][s, :, 0]),
                loo=dict(mean=got["loo"]["mean"][s, :, 0], var=got["loo"]["cov"][s, :, 0, 0], lpd=got["loo"]["lpd"][s],
                         info=got["loo"]["info"][s], total=got["loo"]["total"][s]),
                impute=dict(mean=got["impute"]["mean"][s, :, 0], var=got["impute"]["cov"][s, :, 0, 0], info=got["impute"]["info"][s]))


def _all_sweeps(cgb, spt):
    ll, grad = cgb.loglik_and_gradient_sites_lg(spt)
    lay = _layout(cgb)
    got = dict(grad=grad, scan=cgb.shift_scan_sites_lg(information=True), edge=cgb.edge_gradient_sites_lg(), loo=cgb.loo_sites_lg(),
               impute=cgb.impute_sites_lg())
    assert _layout(cgb) == lay
    return ll, got


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_sweeps_and_calibrated_state(P, i):
    """gradient_sites, shift_scan_sites, edge_gradient_sites, loo_sites and impute_sites under the mask: at every site against
    the restatement; at the checked sites against the dense statements and against the static-pattern engine through the
    general calls.  Codes and totals: the planted edge is unidentified at its site only, a masked (tip, site) carries
    PGBP_INFO_NOT_OBSERVED in loo and adds nothing to total, total is the block-ordered sum of the call's own lpd, impute at
    an observed site is NaN with the code.  moments_sites_ and sample_posterior_sites_ (z = 0) against the dense posterior."""
    name, make, n = CASES[i]
    case = make(n)
    cgb = _masked_engine(P, case)
    ll, got = _all_sweeps(cgb, case.spt)
    assert not got["grad"]["info"].any() and not got["scan"]["info"].any() and not got["edge"]["info"].any()
    _own_top(f"{name}/{n}", got["scan"], case.fam)
    _, fam_of = SM.tip_rows(case)
    static_tips = [int(f) for f in got["loo"]["families"]]
    tip_row = np.asarray(case.fam["data_row"])[static_tips]
    listed = sorted(fam_of[int(r)] for r in np.flatnonzero(case.mask.any(axis=0)))
    assert [int(f) for f in got["impute"]["families"]] == listed
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), v)

    checked = SM.checked_sites(case)
    proper = not FR.is_improper(case.base.sites[0][0])
    mom = cgb.moments_sites_() if proper else None
    draws = cgb.sample_posterior_sites_(n_draws=1, z=np.zeros((1, n, int(cgb._lib.pgbp_sample_size(cgb._eng))))) if proper else None
    n_static = n_refused = n_imp = 0
    for s in range(n):
        ref, fam_s = SM.reference_site(case, s)
        g = _site(got, s)
        note("loglik", abs(ll[s] - SM.dense_loglik(case, s)) / max(1.0, abs(ll[s])))
        assert np.array_equal(g["scan"]["identified"], ref["scan"]["identified"]), s
        for k in ("jump", "lr", "H"):
            note(k, _rel(g["scan"][k], ref["scan"][k]))
        # (the top family itself is not compared: under a mask exact ties are common -- with a tip missing the edge above its
        # sibling and the edge above their parent have the same lr -- and rounding decides them; the call's own table does)
        note("top_lr", _rel(g["scan"]["top_lr"], ref["scan"]["top_lr"]))
        for k in ("dlength", "dgamma", "dshift"):
            note(k, _rel(g["edge"][k], ref["edge"][k]))
        # leave-one-out: codes, NaN at the masked tips, the total
        assert np.array_equal(g["loo"]["info"], ref["loo"]["info"]), s
        assert np.array_equal(g["loo"]["info"] == SM.NOT_OBSERVED, case.mask[s, tip_row]), s
        for k in ("mean", "var", "lpd"):
            note("loo " + k, _rel(g["loo"][k], ref["loo"][k]))
        own = SM.block_total_masked(g["loo"]["lpd"], case.mask[s, tip_row])
        assert np.isfinite(g["loo"]["total"]) and abs(g["loo"]["total"] - own) <= 1e-12 * max(1.0, abs(own)), s
        note("loo total", _rel(g["loo"]["total"], ref["loo"]["total"]))
        # imputation: a prediction at the masked sites, NaN and the code at the observed ones
        assert np.array_equal(g["impute"]["info"], ref["impute"]["info"]), s
        assert np.array_equal(g["impute"]["info"] == SM.NOT_OBSERVED, ~case.mask[s, ref["impute"]["rows"]]), s
        for k in ("mean", "var"):
            note("impute " + k, _rel(g["impute"][k], ref["impute"][k]))
        if s not in checked:
            continue
        # the dense statements
        raw = dict(scan=g["scan"], edge=g["edge"],
                   loo={k: v[~ref["loo"]["masked"]] for k, v in g["loo"].items() if k != "total"})
        w = FR.against_dense(raw, SM.dense_site(case, s), fam_s, tip_row[~ref["loo"]["masked"]])
        for k, v in w.items():
            note("dense " + k, v)
        di = PU.dense_impute(case, s)
        for k, r in enumerate(ref["impute"]["rows"]):
            if case.mask[s, r]:
                note("dense impute", max(_rel(g["impute"]["mean"][k], di[int(r)][0]), _rel(g["impute"]["var"][k], di[int(r)][1])))
        if proper:
            pm, pc = PU.dense_posterior(case, s)
            _, _, _, _, vn, off = PU.layout(case)
            flat = np.array([v for v, _ in vn], dtype=int)
            note("moments mean", _rel(np.concatenate([m[0][s] for m in mom]), pm[flat]))
            note("moments var", _rel(np.concatenate([np.diag(m[1][s]) for m in mom]), np.diag(pc)[flat]))
            assert not any(m[3][s] for m in mom) and not draws[1][s]
            note("sample z=0", _rel(draws[0][0, s], pm[flat]))
        # the static-pattern engine, general calls (no shifts / noise: the pattern's engine has its own family indices' masks)
        if case.shifts is None and case.noise is None:
            st = _static_engine(P, case, s)
            if st is not None:
                n_static += 1
                one, fam_p = st
                l1, g1 = one.loglik_and_gradient_lg(case.spt)
                note("static loglik", abs(ll[s] - float(np.ravel(l1)[0])) / max(1.0, abs(ll[s])))
                for k in ("dR", "dmu", "dalpha", "dtheta"):
                    note("static " + k, _rel(np.ravel(got["grad"][k][s]), np.ravel(g1[k])))
                live = np.asarray(fam_p["child_mask"]) != 0 if fam_p.get("child_mask") is not None else np.ones(len(fam_s["cluster"]), bool)
                sc, eg = one.shift_scan_lg(information=True), one.edge_gradient_lg()
                e1 = live & (np.asarray(case.fam["n_parents"]) >= 1)
                note("static lr", _rel(g["scan"]["lr"][e1], np.asarray(sc["lr"]).reshape(-1)[e1]))
                note("static jump", _rel(g["scan"]["jump"][e1], np.asarray(sc["jump"]).reshape(-1)[e1]))
                note("static dlength", _rel(g["edge"]["dlength"][e1], np.asarray(eg["dlength"]).reshape(g["edge"]["dlength"].shape)[e1]))
                note("static dgamma", _rel(g["edge"]["dgamma"][e1], np.asarray(eg["dgamma"]).reshape(g["edge"]["dgamma"].shape)[e1]))
                note("static dshift", _rel(g["edge"]["dshift"][e1], np.asarray(eg["dshift"]).reshape(-1)[e1]))
                # leave-one-out: the static engine lists the observed tips of the pattern, ours every tip with the code
                lo1 = one.loo_lg()
                seen = ~case.mask[s, tip_row]
                assert [int(f) for f in lo1["families"]] == [f for f, o in zip(static_tips, seen) if o], s
                assert not np.asarray(lo1["info"]).any()
                note("static loo mean", _rel(g["loo"]["mean"][seen], np.asarray(lo1["mean"])[:, 0]))
                note("static loo var", _rel(g["loo"]["var"][seen], np.asarray(lo1["cov"])[:, 0, 0]))
                note("static loo lpd", _rel(g["loo"]["lpd"][seen], np.asarray(lo1["lpd"])))
                note("static loo total", _rel(g["loo"]["total"], float(lo1["total"])))
                # imputation: the static engine lists the masked tips of the pattern; where a parent is out of its (shrunk)
                # scope it predicts nothing (info -1) -- there only the dense statement above speaks
                im1 = one.impute_lg()
                gone = case.mask[s, ref["impute"]["rows"]]
                assert [int(f) for f in im1["families"]] == [int(f) for f, o in zip(got["impute"]["families"], gone) if o], s
                if gone.any():
                    ok1 = np.asarray(im1["info"]) == 0
                    assert np.all(np.asarray(im1["info"])[~ok1] == -1)
                    n_imp += int(ok1.sum())
                    note("static impute mean", _rel(g["impute"]["mean"][gone][ok1], np.asarray(im1["mean"])[ok1, 0]))
                    note("static impute var", _rel(g["impute"]["var"][gone][ok1], np.asarray(im1["cov"])[ok1, 0, 0]))
            else:
                n_refused += 1
    if case.shifts is None and case.noise is None:   # (the reference allocates most patterns; site 1 masks nothing)
        assert n_static >= max(2, len(checked) // 2) and n_static + n_refused == len(checked) and n_imp > 0, (n_static, n_refused, n_imp)
    # the planted cherry: its edge is not identified at its site and identified at the neighbours
    pl = case.planted_mask
    if pl["cherry"]:
        s0, f, _ = pl["cherry"]
        ident = got["scan"]["identified"][:, f, 0]
        assert not ident[s0] and ident[s0 - 1] and ident[s0 + 1] and got["scan"]["lr"][s0, f] == 0.0
        assert np.isnan(got["scan"]["jump"][s0, f, 0]) and got["scan"]["top_family"][s0] != f
    if pl["every"] is not None:
        ti = int(np.flatnonzero(tip_row == pl["every"])[0])
        others = np.arange(n) != 1
        assert np.all(got["loo"]["info"][others, ti] == SM.NOT_OBSERVED) and got["loo"]["info"][1, ti] == 0
    print(f"{name}/{n}: {n} sites against the restatement, {len(checked)} against the dense statements, {n_static} against a "
          f"static-pattern engine ({n_refused} patterns the reference does not allocate, {n_imp} imputations compared): " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= TOL, worst
    # imputed_data takes a site of the result
    table = np.array([[np.nan if case.mask[2, r] else v] for r, v in enumerate(case.base.sites[2][1][0])])
    d2 = {k: (v[2] if k in ("mean", "cov", "info") else v) for k, v in got["impute"].items()}
    filled = P.imputed_data(d2, table)
    assert not np.isnan(filled).any() and np.array_equal(filled[~case.mask[2]], table[~case.mask[2]])


def test_gradient_closed_form_and_fit(P):
    """BM with a fixed root, 64 sites: gradient_sites_lg of every site against the closed-form gradient of the GLS
    log-likelihood on the observed tips; fit_sites_lg against the per-site closed-form optimum -- the deficit of the
    log-likelihood against that optimum is asserted at 1e-8 of max(1, |ll|) -- and its evaluation count next to the no-mask
    count (printed)."""
    case = SM.bm(64)
    C = SM.bm_cov(case)
    cgb = _masked_engine(P, case)
    ll, grad = cgb.loglik_and_gradient_sites_lg(case.spt)
    worst = 0.0
    ys = []
    for s in range(64):
        y = np.array([0.0 if v is None else v for v in case.sites[s][1][0]])
        ys.append(y)
        kw = SM.site_kw(case, s)
        l0, g2, gm = SM.gls_bm(C, y, np.flatnonzero(~case.mask[s]), float(np.ravel(kw["R"])[0]), float(np.ravel(kw["mu"])[0]))
        worst = max(worst, abs(ll[s] - l0) / max(1.0, abs(l0)), abs(grad["dR"][s, 0, 0, 0] - g2) / max(1.0, abs(g2)),
                    abs(grad["dmu"][s, 0] - gm) / max(1.0, abs(gm)))
    print(f"gradient_sites_lg under a mask against the closed form: {worst:.2e}")
    assert worst <= TOL
    fit = P.fit_sites_lg(cgb, case.spt, "bm", 1.0, 0.0)
    best = np.array([SM.gls_bm(C, ys[s], np.flatnonzero(~case.mask[s])) for s in range(64)])
    deficit = float(np.max((best[:, 2] - fit["loglik"]) / np.maximum(1.0, np.abs(best[:, 2]))))
    plain = _masked_engine(P, case, mask=False)
    fit0 = P.fit_sites_lg(plain, case.spt, "bm", 1.0, 0.0)
    print(f"fit_sites_lg under a mask: largest deficit against the GLS optimum {deficit:.2e} of max(1, |ll|), "
          f"{fit['n_device_evals']} evaluations ({fit0['n_device_evals']} without the mask); "
          f"mu {float(np.max(np.abs(fit['mu'] - best[:, 0]))):.1e}, sigma2 rel {float(np.max(np.abs(fit['R'] / best[:, 1] - 1))):.1e}")
    assert fit["converged"].all() and abs(deficit) <= TOL


# ----------------------------------------------------------------------------- 3: determinism

def _raw_calls(cgb, a, b):
    """every lanes-are-sites call on [a, b) through the C ABI: one list of arrays (sentinel-filled first)"""
    from pgbp_amd import _lib as L
    n = b - a
    nf = len(cgb._lg["cluster"])
    K = cgb._lg["length"].size // nf
    nt = int(cgb._lib.pgbp_lg_loo_count(cgb._eng))
    nl = int(cgb._lib.pgbp_lg_impute_count(cgb._eng))
    f64 = lambda *shape: np.full(shape, 7.0)
    i32 = lambda *shape: np.full(shape, 7, np.int32)
    out = [f64(n, 1), f64(n), f64(n), i32(n),                                          # gradient
           f64(nf, n), f64(nf, n), f64(nf, n), f64(n), i32(n), i32(n),                 # scan
           f64(nf, K, n), f64(nf, K, n), f64(nf, n), i32(n),                           # edge
           f64(nt, n), f64(nt, n), f64(nt, n), f64(n), i32(nt, n),                     # loo
           f64(nl, n), f64(nl, n), i32(nl, n)]                                         # impute
    p = [L.f64p(x) if x.dtype == np.float64 else L.i32p(x) for x in out]
    lib, e = cgb._lib, cgb._eng
    assert lib.pgbp_lg_gradient_sites(e, a, b, p[0], p[1], None, None, None, p[3]) == 0
    assert lib.pgbp_lg_shift_scan_sites(e, a, b, 1e-8, p[4], p[5], p[6], p[7], p[8], p[9]) == 0
    assert lib.pgbp_lg_edge_gradient_sites(e, a, b, p[10], p[11], p[12], p[13]) == 0
    assert lib.pgbp_lg_loo_sites(e, a, b, p[14], p[15], p[16], p[17], p[18]) == 0
    assert lib.pgbp_lg_impute_sites(e, a, b, p[19], p[20], p[21]) == 0
    return out


def _same(x, y):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


def _cols(parts, total):
    """the per-range outputs put side by side along the site axis (the last)"""
    return [np.concatenate([p[i] for p in parts], axis=0 if i < 4 else -1) for i in range(len(total))]   # (the gradient: [site, ...])


def test_determinism_and_read_only(P):
    """Equal bytes for two calls, for site ranges split where the split is no multiple of 64, with one workgroup per chunk,
    and for the site-minor and the plain instance of the same beliefs; the fill gives the same bytes twice; the pool and a
    following calibrate_ keep their bytes after each sweep."""
    case = SM.bm(257)
    cgb = _masked_engine(P, case)
    p1 = _pools(cgb)
    cgb.assignfactors_lg_(**cgb._fam_uni_kw, sync=True)
    p2 = _pools(cgb)
    assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1])
    cgb._ensure_schedule([case.spt])
    o = cgb._opts()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    cgb.pull()
    after = cgb._packed_raw.copy()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    assert _layout(cgb) == 2
    whole = _raw_calls(cgb, 0, 257)
    assert _same(whole, _raw_calls(cgb, 0, 257)) and _layout(cgb) == 2
    parts = [_raw_calls(cgb, a, b) for a, b in ((0, 37), (37, 130), (130, 257))]
    assert _same(whole, _cols(parts, whole))
    cgb._lib.pgbp_sites_sweep_scratch_limit(256)      # one workgroup's sites per chunk
    try:
        assert _same(whole, _raw_calls(cgb, 0, 257))
    finally:
        cgb._lib.pgbp_sites_sweep_scratch_limit(0)
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    cgb.pull()
    assert np.array_equal(after, cgb._packed_raw)
    # the plain instance of the same beliefs: pull() left a host copy; an engine of the first 64 sites in each layout
    c64 = SM.bm(64)
    sm = _masked_engine(P, c64)
    sm._ensure_schedule([c64.spt])
    assert sm._lib.pgbp_enqueue_calibrate(sm._eng, 1, 1, C.byref(o)) == 0 and _layout(sm) == 2
    a = _raw_calls(sm, 0, 64)
    sm.pull()                                         # (get_beliefs converts the engine to the plain layout)
    assert _layout(sm) == 0
    assert _same(a, _raw_calls(sm, 0, 64)) and _layout(sm) == 0


# ----------------------------------------------------------------------------- 4: refusals

def test_refusals_and_lifetime(P):
    """Each refusal leaves mask, layout, pool and outputs untouched and its text names what the header says it names; the
    mask survives set_edges, set_shifts, set_tip_noise and set_data and is cleared by a new lg_setup; an engine borrowed from
    a pgbp_patterns handle takes the setter."""
    import copy
    from pgbp_amd import _lib as L
    from pgbp_amd.clustergraphbeliefs import _check
    case = copy.copy(SM.bm(65))
    # one more data row than the table has tips (row 40 belongs to no family): the refusal of a row without a tip
    wide = copy.copy(case.base)
    wide.sites = [(m, [list(tbl[0]) + [0.5]]) for m, tbl in case.base.sites[:65]]
    case.base = wide
    case.mask = np.concatenate([case.mask, np.zeros((65, 1), bool)], axis=1)
    free = case.mask.shape[1] - 1
    cgb = _masked_engine(P, case)
    cgb._ensure_schedule([case.spt])
    o = cgb._opts()
    assert cgb._lib.pgbp_enqueue_calibrate(cgb._eng, 1, 1, C.byref(o)) == 0
    cgb.pull()
    lay = _layout(cgb)
    before = cgb._packed_raw.copy()
    rows, fam_of = SM.tip_rows(case)

    def refused(mask, *words):
        m8 = np.ascontiguousarray(mask, np.uint8)   # (the C call: the wrapper has a check of its own before it)
        with pytest.raises(P.PgbpError) as ei:
            _check(cgb._lib.pgbp_lg_set_site_missing(cgb._eng, m8.ctypes.data_as(C.POINTER(C.c_uint8))), cgb._eng)
        assert ei.value.code == L.ERR_INVALID and all(w in str(ei.value) for w in words), str(ei.value)
        assert np.array_equal(cgb.site_missing_lg(), case.mask) and cgb.site_missing_count_lg() == int(case.mask.sum())
        assert _layout(cgb) == lay
        cgb.pull()
        assert np.array_equal(before, cgb._packed_raw)

    none = np.zeros_like(case.mask)
    m = none.copy()
    m[9, rows] = True
    refused(m, "site 9", "no observed tip")
    assert free not in fam_of
    m = case.mask.copy()
    m[4, free] = True
    refused(m, "site 4", f"row {free}", "no tip family")
    # the wrapper's own refusal: a mask that uncovers entries whose value the device no longer holds
    with pytest.raises(ValueError, match="uncovered"):
        cgb.set_site_missing_lg(none)
    assert np.array_equal(cgb.site_missing_lg(), case.mask)
    # every general sweep while a mask is in force: PGBP_ERR_INVALID, the _sites call named, outputs untouched
    for call, sites_call in ((lambda: cgb.gradient_lg(all_sites=True), "pgbp_lg_gradient_sites"),
                             (lambda: cgb.edge_gradient_lg(all_sites=True), "pgbp_lg_edge_gradient_sites"),
                             (lambda: cgb.shift_scan_lg(all_sites=True), "pgbp_lg_shift_scan_sites"),
                             (lambda: cgb.loo_lg(all_sites=True), "pgbp_lg_loo_sites"),
                             (lambda: cgb.impute_lg(all_sites=True), "pgbp_lg_impute_sites"),
                             (lambda: P.bm_exact_stats(cgb), "pgbp_lg_gradient_sites")):
        with pytest.raises(P.PgbpError) as ei:
            call()
        assert ei.value.code == L.ERR_INVALID and sites_call in str(ei.value) and "pgbp_lg_set_site_missing" in str(ei.value)
        assert _layout(cgb) == lay
    out = np.full((65, 1), 7.0)
    assert cgb._lib.pgbp_lg_gradient(cgb._eng, 0, 65, L.f64p(out), L.f64p(out), None, None, L.i32p(np.zeros(65, np.int32))) == L.ERR_INVALID
    assert np.all(out == 7.0)
    cgb.pull()
    assert np.array_equal(before, cgb._packed_raw) and np.array_equal(cgb.site_missing_lg(), case.mask)
    # lifetime
    nf = len(case.fam["cluster"])
    cgb.set_edges_lg(length=np.asarray(cgb._lg["length"]) * 1.0)
    cgb.set_shifts_lg([(int(fam_of[int(rows[0])]), 0)], np.zeros((1, 1)))
    cgb.set_tip_noise_lg(np.array([fam_of[int(rows[0])]], np.int32), np.zeros((1, 1)), np.ones(1), np.full((1, 1), 0.25))
    cgb.set_data_lg(cgb.get_data_lg())
    assert np.array_equal(cgb.site_missing_lg(), case.mask) and cgb.site_missing_count_lg() == int(case.mask.sum())
    cgb.clear_shifts_lg()
    cgb.clear_tip_noise_lg()
    assert nf > 0
    data = np.array([[[float(v)] for v in tbl[0]] for _, tbl in case.base.sites[:65]])
    cgb.lg_setup(case.fam, data)
    assert cgb.site_missing_count_lg() == 0 and not cgb.site_missing_lg().any()
    # engines the setter refuses: fewer than 8 sites, more than one trait
    small = _engine(P, case.base, 4)
    with pytest.raises(P.PgbpError, match="4 sites.*pgbp_patterns"):
        small.set_site_missing_lg(case.mask[:4])
    assert small.site_missing_count_lg() == 0
    small.set_site_missing_lg(None)   # (clearing is accepted on any engine with a table)
    from test_gpu_gradient import _tree_batch
    engine, *_ = _tree_batch(P, 8, 2, 50, True)
    two = engine(np.arange(8))
    with pytest.raises(P.PgbpError, match="2 traits.*pgbp_patterns"):
        two.set_site_missing_lg(np.zeros((8, two._lg["data"].shape[1]), bool))
    assert two.site_missing_count_lg() == 0
    two.set_site_missing_lg(None)


def test_a_table_with_nans(P):
    """The table-with-NaNs route: split_missing_data gives the finite table lg_setup takes and the mask; set_site_missing_lg
    with mask="nan" and data= installs mask and table in one call; "nan" without data reads the NaNs of the data last given
    (none after a complete-data set-up; those of a set_data_lg under the mask afterwards).  All three engines hold the bytes of
    the engine that was given the bool mask."""
    case = SM.bm(65)
    want_pool, want_f = _pools(_masked_engine(P, case))
    table = np.array([[np.nan if case.mask[s, r] else float(v) for r, v in enumerate(tbl[0])] for s, (m, tbl) in enumerate(case.base.sites[:65])])
    clean, mask = P.split_missing_data(table, fill=123.0)
    assert np.array_equal(mask, case.mask) and clean.shape == (65, table.shape[1], 1) and np.all(clean[mask] == 123.0)
    assert np.array_equal(clean[~mask], table[~mask][:, None])
    import copy
    filled = copy.copy(case.base)
    filled.sites = [(m, [list(clean[s, :, 0])]) for s, (m, _) in enumerate(case.base.sites[:65])]
    a = _engine(P, filled, 65)            # (a): the clean table at set-up, then the mask
    a.set_site_missing_lg(mask)
    b = _engine(P, case.base, 65)         # (b): the complete data at set-up, then mask="nan" with the table
    b.set_site_missing_lg("nan", data=table)
    c = _engine(P, case.base, 65)         # (c): "nan" without data: nothing after a complete-data set-up ...
    c.set_site_missing_lg("nan")
    assert c.site_missing_count_lg() == 0
    c.set_site_missing_lg(mask)           # ... the NaNs of a set_data_lg under the mask afterwards
    c.set_data_lg(table[:, :, None])
    c.set_site_missing_lg("nan")
    for e in (a, b, c):
        assert np.array_equal(e.site_missing_lg(), case.mask) and np.all(e.get_data_lg()[case.mask] == 0.0)
        e.assignfactors_lg_(**e._fam_uni_kw, sync=True)
        pool, fpool = _pools(e)
        assert np.array_equal(pool, want_pool) and np.array_equal(fpool, want_f)
    with pytest.raises(ValueError, match="bool array"):
        a.set_site_missing_lg("NaN")


def test_a_patterns_handle_takes_the_setter(P):
    """Two engines borrowed from a pgbp_patterns handle, 16 sites each, take their part of the mask like any other engine:
    the handle's loglik against densemvn, site by site."""
    from pgbp_amd.sharding import PatternGroup
    from test_gradient_cpu import model_params
    case = SM.bm(64)
    arrays = tuple(N.engine_arrays(P, case.ocgb0))
    parts = [list(range(0, 32, 2)), list(range(1, 32, 2))]
    pats = PatternGroup([arrays + (parts[0],), arrays + (parts[1],)])
    pats.set_schedule([case.spt])
    data = np.array([[[float(v)] for v in tbl[0]] for _, tbl in case.base.sites[:32]])
    par = [model_params(m) for m, _ in case.base.sites[:32]]
    R = np.stack([np.stack([np.atleast_2d(r) for r in q[0]]) for q in par])
    mu = np.stack([np.atleast_1d(q[2]) for q in par])
    for k in range(2):
        b = pats.beliefs[k]
        b.lg_setup(case.fam, data[parts[k]])
        b.set_site_missing_lg(case.mask[parts[k]])
        assert b.site_missing_count_lg() == int(case.mask[parts[k]].sum())
        b.assignfactors_lg_(R[parts[k]], mu[parts[k]])
    ll, info = pats.loglik_lg()
    want = np.array([SM.dense_loglik(case, s) for s in range(32)])
    err = float(np.max(np.abs(ll - want) / np.maximum(1.0, np.abs(want))))
    pats.close()
    print(f"patterns handle, 16 + 16 sites, each engine with its part of the mask: loglik against densemvn {err:.2e}")
    assert not np.asarray(info).any() and err <= TOL

#!/usr/bin/env python3
"""The reference's getting-started pipeline (docs/src/man/getting_started.md:30-292) on the MI355X engine, with the
product's own host side from the Newick string to the likelihood:

    network string -> clique tree -> belief scopes -> schedule -> factors on the device -> calibrate! -> log-likelihood

Network, trait values and the expected numbers are the doctest's (tests/golden/reference_goldens.json: doctest_lazaridis).
Needs a GPU:  python examples/getting_started.py [cliquetree|bethe|joingraph|ltrip]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pgbp_amd as P  # noqa: E402


def main():
    method = sys.argv[1] if len(sys.argv) > 1 else "cliquetree"
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        g = json.load(f)["doctest_lazaridis"]
    net, names = P.read_newick(g["net"])                         # readnewick + preprocessnet!
    build = {"cliquetree": P.cliquetree, "bethe": P.bethe, "ltrip": P.ltrip, "joingraph": lambda f: P.joingraph(f, 3)}[method]
    cn, ed, sn = build(net.node2family)                          # clustergraph!(net, method)
    print(f"{method}: {len(cn)} clusters, {len(ed)} sepsets, largest cluster {max(len(c) for c in cn)} nodes")
    st = P.allocate_scopes(cn, ed, sn, net, 1)                   # allocatebeliefs
    row = {t: r for r, t in enumerate(g["taxa"])}
    fam = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                        [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                        [row.get(names[i], -1) for i in range(net.nnodes)], 1)
    cgb = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
    cgb.lg_setup(fam, np.array(g["x"], float)[:, None])
    cgb.assignfactors_lg_(np.array([[[g["model"]["sigma2"]]]], float), [g["model"]["mu"]])   # UnivariateBrownianMotion(1, 0)
    exact = len(ed) == len(cn) - 1
    if not exact:
        P.load().pgbp_regularize_bycluster(cgb._eng)             # regularizebeliefs_bycluster!
    sched = P.spanningtrees_clusterlist(len(cn), ed, cn, net.is_leaf)
    succ, iscal = P.calibrate_(cgb, sched, 50, auto=True, info=True)
    r = cgb.last_results[0]
    print(f"calibrate!: succ {succ}, calibrated {iscal} (iteration {r.iter_reached}, schedule tree {r.tree_reached})")
    root = sched[0][2][0]
    mu, norm = cgb.integratebelief_(root)
    _, _, fe = cgb.factored_energy()
    print(f"integratebelief! at cluster {root}: {norm:.12f};  factored energy {fe:.12f};  doctest log-likelihood {g['ll']:.12f}"
          + ("" if exact else "  (loopy graph: approximations)"))
    if exact:
        assert abs(norm - g["ll"]) <= 1e-9 * abs(g["ll"])
        # an out-of-clique query from the same calibration: the difference between two internal nodes that may share no
        # cluster, with its standard error (posterior_cov_: w = A'c for the contrast c, Var(c'x | data) = |w|^2)
        off = np.concatenate([[0], np.cumsum(st.dims[: len(cn)])])
        where = {}                                               # internal node -> (its first cluster, position there)
        for ci, sc in enumerate(st.clusters):
            for pos, v in enumerate(np.array(sc.nodelabel)[sc.inscope[0]]):
                where.setdefault(int(v), (ci, pos))
        (ca, pa), (cb, pb) = where[min(where)], where[max(where)]
        contrast = np.zeros(int(off[-1]))
        contrast[off[ca] + pa], contrast[off[cb] + pb] = 1.0, -1.0
        w, _, _ = cgb.posterior_cov_(contrast, want_k=False)
        mom = cgb.moments_([ca, cb], cov=False)
        print(f"ancestral states: {names[min(where) - 1]} - {names[max(where) - 1]} = {mom[0][0][pa] - mom[1][0][pb]:.4f} "
              f"+- {np.linalg.norm(w):.4f} (clusters {ca} and {cb})")
        # leave-one-out cross-validation from the same calibration: how well do the other tips predict each tip?
        loo = cgb.loo_lg()
        z = P.loo_zscores(loo)[:, 0]
        worst = int(np.nanargmax(np.abs(z)))
        tip = g["taxa"][int(cgb._lg["data_row"][loo["families"][worst]])]
        print(f"leave-one-out: summed log predictive density {loo['total']:.6f}; largest |z| {abs(z[worst]):.3f} at tip {tip} "
              f"(observed {loo['y'][worst, 0]:.4f}, predicted {loo['mean'][worst, 0]:.4f} +- {np.sqrt(loo['cov'][worst, 0, 0]):.4f})")
        # derivatives in every edge from the same calibration: where would a shift of the mean help most, and which
        # inheritance do the traits pull at?  (no root-prior family here: family f is the family of node f + 1)
        dg = cgb.edge_gradient_lg()
        f = int(np.argmax(np.abs(dg["dshift"][:, 0])))
        parents = [names[q - 1] for q in net.node2family[f + 1][1:]]
        print(f"edge gradient: largest |dshift| {dg['dshift'][f, 0]:.4f} on the edge(s) {parents} -> {names[f + 1]}")
        hyb = np.nonzero(fam["n_parents"] == 2)[0]
        if len(hyb):
            h = int(hyb[0])
            print(f"first hybrid {names[h + 1]}: dgamma {dg['dgamma'][h]} (free partials; with gamma_2 = 1 - gamma_1: "
                  f"{dg['dgamma'][h, 0] - dg['dgamma'][h, 1]:.4f}), dlength {dg['dlength'][h]}")
        # the engine can hold such a shift: fit the jump on that edge (the exact ML value at these parameters, from
        # n p + 2 = 3 calibrations -- at 0, at the unit shift, and one that leaves the engine at the estimate: the
        # log-likelihood is quadratic in the shifts) and see what it buys
        fit = P.fit_shifts_lg(cgb, sched[0], [(f, 0)])
        print(f"fitted shift on {parents[0]} -> {names[f + 1]}: {fit['shifts'][0, 0]:.4f} +- {fit['se'][0, 0]:.4f}; "
              f"log-likelihood {norm:.6f} -> {fit['loglik']:.6f} (gain {fit['loglik'] - norm:.6f})")
        assert fit["loglik"] >= norm
        cgb.clear_shifts_lg()
        # which edge carries a jump, how big is it, what does it buy?  Plant a jump of +3 on the edge into an internal node
        # (every tip gains 3 x the share of its ancestry that passes through that edge), scan EVERY edge from one
        # calibration -- per edge the exact ML jump, its standard error and the gain 2 (ll(jump) - ll(0)) -- and let the
        # forward selection pick and refit it
        x = np.array(g["x"], float)[:, None]
        n = net.nnodes

        def share(c):   # what a unit displacement of node c adds to the mean of every node (BM: qc = gamma)
            tau = np.zeros(n)
            tau[c] = 1.0
            for i in range(c + 1, n):
                tau[i] = sum(gk * tau[q - 1] for gk, q in zip(net.gamma[i], net.node2family[i][1:]))
            return tau
        inner = [i for i in range(1, n) if not net.is_leaf[i] and len(net.node2family[i]) == 2]
        ntips = int(np.sum(net.is_leaf))
        c = min(inner, key=lambda i: abs(sum(1 for q in range(n) if net.is_leaf[q] and share(i)[q] > 0) - ntips / 3))
        tau = share(c)
        xj = x.copy()
        for i in range(n):
            if net.is_leaf[i] and names[i] in row:
                xj[row[names[i]], 0] += 3.0 * tau[i]
        cgb.lg_setup(fam, xj)
        cgb.assignfactors_lg_(np.array([[[g["model"]["sigma2"]]]], float), [g["model"]["mu"]])
        ll_j, scan = cgb.loglik_and_shift_scan_lg(sched[0], information=True)
        print(f"jump of +3 planted on the edge into {names[c]}; scan of {int(np.sum(fam['n_parents']))} edges, log-likelihood {ll_j:.6f}:")
        for f in np.argsort(-np.nan_to_num(scan["lr"], nan=-1.0))[:3]:
            k = int(np.argmax(fam["gamma"].reshape(len(scan["lr"]), -1)[f, :fam["n_parents"][f]]))
            gk = fam["gamma"].reshape(len(scan["lr"]), -1)[f, k]
            print(f"  {names[net.node2family[f + 1][1 + k] - 1]} -> {names[f + 1]}: jump {scan['edge_jump'][f, k, 0]:.4f} "
                  f"+- {scan['se'][f, 0] / abs(gk):.4f}, lr {scan['lr'][f]:.4f}")
        sel = P.select_shifts_lg(cgb, sched[0], 1)
        (fs, ks), step = sel["edges"][0], sel["path"][0]
        print(f"selected {names[net.node2family[fs + 1][1 + ks] - 1]} -> {names[fs + 1]}: shift {step['shifts'][0, 0]:.4f} "
              f"+- {sel['fit']['se'][0, 0]:.4f}, lr at entry {step['lr']:.4f}, log-likelihood {ll_j:.6f} -> {step['loglik']:.6f}")
        assert abs(2.0 * (step["loglik"] - ll_j) - step["lr"]) <= 1e-8 * step["lr"]
        cgb.clear_shifts_lg()
        # imputation: hide two values, set an engine up on the incomplete table and predict them from everything else
        x = np.array(g["x"], float)[:, None]
        hidden = [1, len(x) - 2]
        xm = x.copy()
        xm[hidden] = np.nan
        fam_m = P.lg_families(st.clusters, st.node2cluster, net.node2family, st.node2fixed,
                              [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)],
                              [row.get(names[i], -1) for i in range(net.nnodes)], 1, data=xm)
        cgm = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None)
        cgm.lg_setup(fam_m, xm)
        cgm.assignfactors_lg_(np.array([[[g["model"]["sigma2"]]]], float), [g["model"]["mu"]])
        ll_m, imp = cgm.impute_and_loglik_lg(sched[0])
        filled = P.imputed_data(imp, xm)
        for i, r in enumerate(imp["rows"]):
            print(f"imputed {g['taxa'][int(r)]}: {filled[int(r), 0]:.4f} +- {np.sqrt(imp['cov'][i, 0, 0]):.4f} "
                  f"(hidden value {x[int(r), 0]:.4f}); log-likelihood of the remaining data {ll_m:.6f}")
        # measurement error: the same data read as species means with a known standard error of 0.3 (se2 = 0.09 at every
        # tip; sigma_e = 0: no within-species covariance to scale), fitted with and without it
        cgb.lg_setup(fam, x)
        sigma2, mu0 = np.array([[g["model"]["sigma2"]]], float), [g["model"]["mu"]]
        R_plain, mu_plain, ll_plain, _ = P.calibrate_optimize_cliquetree_(cgb, sched[0], sigma2, mu0, gradient="analytic")
        tips = [f for f in range(len(fam["cluster"])) if fam["child_pos"][f] < 0 and fam["data_row"][f] >= 0]
        cgb.set_tip_noise_lg(tips, np.zeros((1, 1)), se2=np.full((len(tips), 1), 0.09))
        R_se, mu_se, ll_se, _ = P.calibrate_optimize_cliquetree_(cgb, sched[0], sigma2, mu0, gradient="analytic")
        print(f"fit without standard errors: sigma2 {R_plain[0, 0]:.4f}, mu {mu_plain[0]:.4f}, log-likelihood {ll_plain:.6f}; "
              f"with se = 0.3 at {len(tips)} tips: sigma2 {R_se[0, 0]:.4f}, mu {mu_se[0]:.4f}, log-likelihood {ll_se:.6f}")
        cgb.clear_tip_noise_lg()
        # the model run forwards: a data set simulated on the device under the fitted model, written straight into the
        # engine's data, and refitted
        cgb.assignfactors_lg_(R_plain[None], mu_plain)
        xs, _ = cgb.simulate_lg(seed=2024, write_data=True)
        R_sim, mu_sim, ll_sim, _ = P.calibrate_optimize_cliquetree_(cgb, sched[0], R_plain, mu_plain, gradient="analytic")
        print(f"simulated under sigma2 {R_plain[0, 0]:.4f}, mu {mu_plain[0]:.4f} ({xs.shape[1]} node states, "
              f"{len(tips)} of them tips): refit sigma2 {R_sim[0, 0]:.4f}, mu {mu_sim[0]:.4f}, log-likelihood {ll_sim:.6f}")
        # parametric bootstrap of the scan: the largest lr over all edges has no closed-form null law; 200 replicates (sites)
        # are simulated under the fitted model WITHOUT a jump and scanned at once.  Its 95 % quantile is a calibrated min_lr
        # for select_shifts_lg; the observed maximum is that of the data with the planted jump, scanned above.
        B = 200
        boot = P.ClusterGraphBelief.from_arrays(st.dims, st.sepset_clusters, st.scope_off, st.scope_idx, None, n_sites=B)
        boot.lg_setup(fam, np.repeat(x[None], B, axis=0))
        boot.assignfactors_lg_(R_plain[None], mu_plain)
        null = P.bootstrap_shift_scan_lg(boot, sched[0], seed=7)
        q95 = float(np.quantile(null["max_lr"], 0.95))
        print(f"largest lr of the scan: observed {float(np.nanmax(scan['lr'])):.2f} (jump planted), bootstrap 95 % quantile "
              f"without a jump {q95:.2f} ({B} replicates) -> min_lr of select_shifts_lg")
    # a batch of univariate problems fitted side by side: 32 OU sites on one 60-tip tree, each with its own stationary
    # variance, alpha, theta and mu; every evaluation is one device pass for all sites (fit_sites_lg)
    from pgbp_amd import synth as S
    rng = np.random.default_rng(3)
    tr = S.random_tree(60, rng)
    ns = 32
    depth = np.zeros(tr.nnodes)
    for i in range(1, tr.nnodes):
        depth[i] = depth[tr.parent[i]] + tr.length[i]
    H = float(depth[tr.is_leaf].mean())           # (alpha H of 1 .. 3: the root value is still identified at the tips)
    al, g2, th = rng.uniform(1, 3, ns) / H, rng.uniform(0.5, 2, ns), rng.normal(0, 2, ns)
    X = S.simulate_ou_uni_sites(tr, 2 * al * g2, al, th, th + rng.normal(size=ns), rng)
    prob = S.cliquetree_of_tree(tr, 1)
    batch = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=ns)
    batch.lg_setup(S.lg_tree_table(tr, prob, 1), np.ascontiguousarray(X[:, :, None]))
    tipmean = X[:, tr.is_leaf].mean(axis=1)
    fit = P.fit_sites_lg(batch, prob.schedule[0], "ou", np.ones(ns), tipmean, alpha0=np.full(ns, 1.0 / H), theta0=tipmean)
    print(f"OU batch: {int(fit['converged'].sum())} of {ns} sites converged in {fit['n_device_evals']} device passes; site 0: "
          f"alpha {fit['alpha'][0]:.3f} (simulated {al[0]:.3f}), theta {fit['theta'][0]:.3f} ({th[0]:.3f}), "
          f"stationary variance {fit['R'][0]:.3f} ({g2[0]:.3f}), log-likelihood {fit['loglik'][0]:.4f}")
    # the engine is left calibrated at the estimates: ancestral states of every site, lanes = sites (moments_sites_; the root is
    # fixed at mu, so the deepest ancestor with a posterior is the first internal node below it: variable 0 of its cluster)
    c = int(np.flatnonzero(prob.meta["child_dim"] > 0)[0])
    m, S, _, info = batch.moments_sites_([c])[0]
    print(f"ancestral state of node {c + 1} (below the root), posterior mean +- sd at the first four sites: " +
          ", ".join(f"{m[s, 0]:.3f} +- {np.sqrt(S[s, 0, 0]):.3f}" for s in range(4)) + f"; {int((info != 0).sum())} sites failed")
    x, _, _ = batch.sample_posterior_sites_(n_draws=200, seed=11)
    print(f"  and from 200 joint draws of all ancestral states (device generator): {x[:, 0, :].mean(axis=0)[int(prob.dims[:c].sum())]:.3f} "
          f"+- {x[:, 0, :].std(axis=0)[int(prob.dims[:c].sum())]:.3f} at site 0")
    # the difference of two ancestors that share no cluster, with its standard error, for every site at once: the contrast as
    # one column of posterior_cov_sites_, its variance folded on the device (gram) -- no table leaves it
    c2 = int(np.flatnonzero(prob.meta["child_dim"] > 0)[-1])
    e1, e2 = int(prob.dims[:c].sum()), int(prob.dims[:c2].sum())
    contrast = np.zeros((1, int(prob.dims[: batch.nclusters].sum())))
    contrast[0, e1], contrast[0, e2] = 1.0, -1.0
    _, _, gram, cinfo = batch.posterior_cov_sites_(contrast, want_w=False, want_k=False)
    m2 = batch.moments_sites_([c2], cov=False)[0][0]
    print(f"  node {c + 1} minus node {c2 + 1}, posterior mean +- se at the first four sites: " +
          ", ".join(f"{m[s, 0] - m2[s, 0]:.3f} +- {np.sqrt(gram[s, 0, 0]):.3f}" for s in range(4)) +
          f"; {int((cinfo != 0).sum())} sites failed")
    # Hansen's model: two clades in selective regimes of their own.  The optimum is painted on the edges (set_optima_lg, as
    # `color` paints rates): regime 1 and 2 on every edge of two clades, theta on the rest; each site fits its own theta_1 and
    # theta_2 beside alpha, theta and the stationary variance, with the derivative doptima of the lanes-are-sites sweep
    from pgbp_amd import synth   # (S is the covariance of the moments above by now)
    kids = [np.flatnonzero(tr.parent == i) for i in range(tr.nnodes)]
    def clade(i):
        out = [i]
        for c_ in kids[i]:
            out += clade(int(c_))
        return out
    size = {i: int(tr.is_leaf[clade(i)].sum()) for i in range(1, tr.nnodes)}
    k1 = min(size, key=lambda i: (abs(size[i] - 12), i))
    k2 = min((i for i in size if i not in clade(k1) and k1 not in clade(i)), key=lambda i: (abs(size[i] - 12), i))
    node_regime = np.zeros(tr.nnodes, np.int32)
    node_regime[clade(k1)], node_regime[clade(k2)] = 1, 2
    opt = th[:, None] + np.array([2.5, -2.5])               # the two clades' optima, per site
    rng_p = np.random.default_rng(5)                          # (a generator of its own: the draws below stay as they were)
    Xp = np.empty_like(X)
    Xp[:, 0] = X[:, 0]
    for i in range(1, tr.nnodes):
        a_ = np.exp(-al * tr.length[i])
        target = th if node_regime[i] == 0 else opt[:, node_regime[i] - 1]
        Xp[:, i] = a_ * Xp[:, tr.parent[i]] + (1 - a_) * target + np.sqrt(g2 * (1 - a_ * a_)) * rng_p.normal(size=ns)
    batch.lg_setup(synth.lg_tree_table(tr, prob, 1), np.ascontiguousarray(Xp[:, :, None]))
    batch.set_optima_lg(node_regime[1:, None], np.zeros((2, 1)))   # (family f of the table is node f + 1)
    tipmean_p = Xp[:, tr.is_leaf].mean(axis=1)
    fitp = P.fit_sites_lg(batch, prob.schedule[0], "ou", np.ones(ns), Xp[:, 0], alpha0=np.full(ns, 1.0 / H), theta0=tipmean_p,
                          fit_mu=False, optima0=np.stack([tipmean_p, tipmean_p], axis=1))
    print(f"painted optima: clades of {size[k1]} and {size[k2]} tips, {int(fitp['converged'].sum())} of {ns} sites converged in "
          f"{fitp['n_device_evals']} device passes; theta_1 - theta, theta_2 - theta at the first four sites (simulated +2.5, "
          f"-2.5): " + ", ".join(f"{fitp['optima'][s, 0] - fitp['theta'][s]:+.2f} {fitp['optima'][s, 1] - fitp['theta'][s]:+.2f}"
                                 for s in range(4)))
    # and when the regimes are NOT known: which clade is pulled to another optimum?  The plain OU model fitted to the same data,
    # then one sweep that scans every edge for a shift of the optimum of its whole clade (optimum_scan_sites_lg: the exact ML
    # increment and its likelihood ratio per edge and site, all edges from one calibration).  The clade that leads at most
    # sites is painted (add_optimum_shift refines the regime map) at each site's own increment, and the next scan looks for
    # the second one with the first in force.
    batch.clear_optima_lg()
    fit0 = P.fit_sites_lg(batch, prob.schedule[0], "ou", np.ones(ns), Xp[:, 0], alpha0=np.full(ns, 1.0 / H), theta0=tipmean_p,
                          fit_mu=False)
    ll0, sc = batch.loglik_and_optimum_scan_sites_lg(prob.schedule[0], information=True)
    lead = int(np.bincount(sc["top_family"][sc["top_family"] >= 0]).argmax())
    table = synth.lg_tree_table(tr, prob, 1)
    reg1, origin = P.add_optimum_shift(np.zeros((tr.nnodes - 1, 1), np.int32), table["parent_family"], lead)
    delta = np.nan_to_num(sc["delta"][:, lead])
    batch.set_optima_lg(reg1, (fit0["theta"] + delta)[:, None, None])        # (origin == [0]: the new regime came from theta)
    ll1, sc1 = batch.loglik_and_optimum_scan_sites_lg(prob.schedule[0])
    nxt = int(np.bincount(sc1["top_family"][sc1["top_family"] >= 0]).argmax())
    print(f"scan for a shifted optimum: the clade below node {lead + 1} ({size[lead + 1]} tips; the painted clades hang below nodes "
          f"{k1} and {k2}) leads at {int((sc['top_family'] == lead).sum())} of {ns} sites; delta +- se at the first four sites: " +
          ", ".join(f"{sc['delta'][s, lead]:+.2f} +- {sc['se'][s, lead]:.2f}" for s in range(4)) +
          f"; painting it gains 2 x {float(ll1[0] - ll0[0]):.3f} = lr {sc['lr'][0, lead]:.3f} at site 0; the next scan leads with the "
          f"clade below node {nxt + 1} ({size[nxt + 1]} tips)")
    # how large is the largest lr over all edges when NO clade has shifted?  200 replicates of site 0 simulated under its plain
    # OU fit and scanned at once (bootstrap_optimum_scan_lg, lanes = replicates)
    B = 200
    boot = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=B)
    boot.lg_setup(table, np.repeat(Xp[:1, :, None], B, axis=0))
    boot.assignfactors_lg_(np.array([[[fit0["R"][0]]]]), np.array([Xp[0, 0]]), model="ou", alpha=float(fit0["alpha"][0]),
                           theta=np.array([fit0["theta"][0]]))
    null = P.bootstrap_optimum_scan_lg(boot, prob.schedule[0], seed=7)
    print(f"  largest lr over all edges at site 0: observed {sc['top_lr'][0]:.2f}, bootstrap 95 % quantile without a shift "
          f"{float(np.quantile(null['max_lr'], 0.95)):.2f} ({B} replicates)")
    batch.clear_optima_lg()
    # in a real batch every site picks its own clades, so the shifts go in per site (set_clade_shifts_sites_lg: a short list of
    # (family, delta) per site, no regime map) and the whole forward selection runs for all sites side by side: scan, the
    # leading clade of each site into its next slot, exact joint refit of the site's deltas, next scan.  alpha and the rate stay
    # at the plain fit; the bootstrap threshold of the first step is reused for the second (an approximation).
    batch.assignfactors_lg_(fit0["R"].reshape(ns, 1, 1, 1), Xp[:, :1], model="ou", alpha=fit0["alpha"], theta=fit0["theta"][:, None])
    sel = P.select_optimum_shifts_sites_lg(batch, prob.schedule[0], 2, float(np.quantile(null["max_lr"], 0.95)))
    both = sum(sorted(sel["family"][:, s].tolist()) == sorted([k1 - 1, k2 - 1]) for s in range(ns))
    print(f"forward selection at all {ns} sites at once: {int((sel['n_shifts'] == 2).sum())} sites take two shifts, {both} of them exactly the "
          f"planted clades below nodes {k1} and {k2}; node: delta at the first four sites: " +
          "; ".join(", ".join(f"{int(sel['family'][j, s]) + 1}: {sel['delta'][j, s]:+.2f}" for j in range(2) if sel["family"][j, s] >= 0)
                    for s in range(4)) + f"; log-likelihood of site 0 along the path: " +
          " -> ".join(f"{v:.2f}" for v in sel["loglik"][:, 0]))
    batch.clear_clade_shifts_sites_lg()
    batch.lg_setup(synth.lg_tree_table(tr, prob, 1), np.ascontiguousarray(X[:, :, None]))   # (the unpainted batch again)
    # real batches have gaps, another set of unmeasured species at almost every site: a table with NaN at its gaps goes to
    # lg_setup with finite placeholders (split_missing_data) and its gaps to set_site_missing_lg; every site is then fitted to
    # its own observed tips and its gaps are imputed, all sites in one call each (lanes = sites)
    table = X.copy()
    leaves = np.flatnonzero(tr.is_leaf)
    gaps = np.zeros(table.shape, bool)
    gaps[:, leaves] = rng.random((ns, len(leaves))) < 0.2
    table[gaps] = np.nan
    clean, mask = P.split_missing_data(table)
    gappy = P.ClusterGraphBelief.from_arrays(prob.dims, prob.sepset_clusters, prob.scope_off, prob.scope_idx, None, n_sites=ns)
    gappy.lg_setup(synth.lg_tree_table(tr, prob, 1), clean)
    gappy.set_site_missing_lg(mask)
    obsmean = np.nanmean(table[:, leaves], axis=1)
    fit2 = P.fit_sites_lg(gappy, prob.schedule[0], "ou", np.ones(ns), obsmean, alpha0=np.full(ns, 1.0 / H), theta0=obsmean)
    imp = gappy.impute_sites_lg()
    site0 = {k: (v[0] if k in ("mean", "cov", "info") else v) for k, v in imp.items()}
    filled = P.imputed_data(site0, table[0][:, None])
    row = int(np.flatnonzero(gaps[0])[0])
    k = int(np.flatnonzero(imp["rows"] == row)[0])
    print(f"the same batch with 20 % of the tip values missing ({int(mask.sum())} gaps): {int(fit2['converged'].sum())} of {ns} sites "
          f"converged in {fit2['n_device_evals']} device passes; site 0: alpha {fit2['alpha'][0]:.3f} ({fit['alpha'][0]:.3f} from the "
          f"complete data); its first gap (row {row}) imputed as {filled[row, 0]:.3f} +- {np.sqrt(imp['cov'][0, k, 0, 0]):.3f}, "
          f"the value held back was {X[0, row]:.3f}")
    # under a Brownian motion the same gappy batch needs no optimiser: the REML rate and the root mean of every site in closed
    # form, from one calibration and one sweep (calibrate_exact_sites_), each site on its own observed tips.  The engine has an
    # improper root (fixedroot=False); the fixed-root engine of the same batch scores the returned model.
    names = [f"n{i}" for i in range(tr.nnodes)]
    net, nm = P.read_newick(tr.newick(names))
    rows = {names[i]: r for r, i in enumerate(leaves)}
    data_row = [rows.get(nm[i], -1) for i in range(net.nnodes)]
    cn, ed, sn = P.cliquetree(net.node2family)
    pe = [list(zip(net.length[i], net.gamma[i], net.color[i])) for i in range(net.nnodes)]
    pair = []
    for fixedroot in (False, True):
        sc = P.allocate_scopes(cn, ed, sn, net, 1, fixedroot=fixedroot)
        e = P.ClusterGraphBelief.from_arrays(sc.dims, sc.sepset_clusters, sc.scope_off, sc.scope_idx, None, n_sites=ns)
        e.lg_setup(P.lg_families(sc.clusters, sc.node2cluster, net.node2family, sc.node2fixed, pe, data_row, 1), clean[:, leaves])
        e.set_site_missing_lg(mask[:, leaves])
        pair.append((sc, e))
    tree_sched = P.spanningtree_clusterlist(len(cn), ed, P.default_rootcluster(cn, net.is_leaf))
    ci = next(i for i, c in enumerate(cn) if 1 in c and pair[0][0].dims[i] > 0)
    reml = P.calibrate_exact_sites_(pair[0][1], tree_sched, (ci, int(pair[0][0].dims[ci]) - 1), pair[1][1])
    print(f"BM in closed form on the gappy batch: site 0 observes {int(round(reml['den'][0])) + 1} of {len(leaves)} tips: REML rate "
          f"{reml['R'][0]:.4f}, root mean {reml['mu'][0]:.4f}, log-likelihood {reml['loglik'][0]:.4f}; "
          f"{int((reml['info'] != 0).sum())} sites failed")
    # how the sites evolve TOGETHER: the evolutionary rate matrix between them (evol.vcv), their evolutionary correlations and
    # the phylogenetic principal components (phyl.pca), from one calibration of the univariate engine and one call that forms
    # Y'PY on the matrix cores.  A cross-site estimate needs the same observed tips at every site: the complete table here.
    sc = pair[0][0]
    whole = P.ClusterGraphBelief.from_arrays(sc.dims, sc.sepset_clusters, sc.scope_off, sc.scope_idx, None, n_sites=ns)
    whole.lg_setup(P.lg_families(sc.clusters, sc.node2cluster, net.node2family, sc.node2fixed, pe, data_row, 1),
                   np.ascontiguousarray(X[:, leaves, None]))
    root = (ci, int(sc.dims[ci]) - 1)
    rate = P.calibrate_rate_matrix_sites_(whole, tree_sched, root)
    pca = P.phylo_pca_sites(whole, tree_sched, root, mode="corr", n_components=2)
    print(f"sites 0 and 1 of the complete batch: evolutionary covariance {rate['R'][0, 1]:.4f}, correlation {rate['corr'][0, 1]:.4f}; "
          f"the first two phylogenetic PCs of the {ns} sites carry {pca['values'][0] / ns:.1%} and {pca['values'][1] / ns:.1%} of the "
          f"standardised variance; tip 0 scores {pca['scores'][0, 0]:.3f}, {pca['scores'][0, 1]:.3f} on them")
    # the same components WITHOUT the sites x sites matrix, for batches where it does not fit: subspace iteration on the
    # operator v -> R v, one device pass over the residual rows per iteration (pgbp_bm_rate_apply_sites)
    lead = P.phylo_pca_leading_sites(whole, tree_sched, root, 3, mode="corr")
    print(f"the first three phylogenetic PCs by subspace iteration: {', '.join(f'{x:.1%}' for x in lead['explained'])} of the "
          f"standardised variance after {lead['iterations']} iterations (converged: {lead['converged']}); the first two values "
          f"differ from the dense route by {np.max(np.abs(lead['values'][:2] - pca['values'])) / pca['values'][0]:.1e}")


if __name__ == "__main__":
    main()

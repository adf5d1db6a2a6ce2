// Scan of every edge for a shift of the optimum of its clade under OU, for univariate batches on a thread-per-site engine,
// lanes = sites: pgbp_lg_optimum_scan_sites of include/pgbp.h, in the frame of pgbp_fam_uni.hip -- a workgroup is 256
// consecutive sites, the family table goes through scalar loads, the beliefs are read as whole lines in the layout the pool is
// in (template <bool SM>), nothing is converted.
//
// The log-likelihood is exactly quadratic in an increment delta of the optimum of every edge of clade(v) (the edge above family
// v and all edges below it): with j = 1 / V, kappa = wc j and e = E[r | data] of a family (the offset with the painted optima),
//   score        g_v = sum over f in clade(v) of kappa_f e_f,
//   information  H_v = sum_f wc_f kappa_f - Var(sum_f kappa_f r_f | data),
// and the posterior variance of that functional, which spans the whole clade, follows from one leaves-to-root recursion with
// four numbers per (family, site) (DESIGN.md has the statement).  One launch per height of the family tree from the tips up
// (optscan_level): a thread owns one (family of that height, site), forms the family's closed-form moments and coefficients
// (fam_uni_family), adds its child families' four numbers from [family][4][site] rows in index order (gather form: a row is
// written once, by its owner), and writes what its parent adds in turn:
//   row 0: (kappa + B) rho - kappa qc     row 1: S + (kappa + B)^2 tau     row 2: G + kappa e = g     row 3: K + wc kappa = Kt
// with rho, tau the regression of x_v on x_parent in the family's own cluster.  Then Var_v from the cluster's moments, H_v = Kt_v
// - Var_v, identified iff H_v > min_info Kt_v: delta = g / H, lr = g^2 / H.  The site's (top_lr, top_family) is folded from a row
// of candidates by blocks of 64 families (optscan_top, a strict > in index order) and the blocks in order (optscan_top_fold).
// Failed sites come from the validity pass of pgbp_post_uni_dev.hpp on schedule tree 0 and are NaN throughout.
// No barrier, no atomics, contraction off, every sum in a fixed order, no lane's store depends on another lane: the bytes of a
// site depend neither on the call nor on the site range, the chunks or the layout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "pgbp_devmem.hpp"
#include "pgbp_fam_uni_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"
#include "pgbp_optscan_host.hpp"
#include "pgbp_post_uni_dev.hpp"
#include "pgbp_sample_plan.hpp"
#include "pgbp_shift_dev.hpp"
#include "pgbp_sites_host.hpp"

namespace pgbp {

// fams[q], q < n: the families of this height.  child_off / child_fam: the child families of a family, in index order.
// bad[site] != 0: a failed site, NaN throughout.  state: [n_fam][4][row]; delta, lr, hinf, cand: [n_fam][row] (any may be null);
// cand: lr where the family is identified and lr is finite, NaN elsewhere
// CS: the instance that also reads the per-site clade shifts of the optimum (pgbp_lg_set_clade_shifts_sites); without it the
// kernel is the scan's own, as it was
template <bool SM, bool CS>
__global__ __launch_bounds__(256) void optscan_level(SitesArgs A, LgStatic F, LgParams M, LgShifts Sh, LgOptima Op, LgNoise Nz,
                                                     LgSiteMiss Ms, LgCladeShifts Cs, const int32_t* __restrict__ fams, int n,
                                                     const int32_t* __restrict__ child_off, const int32_t* __restrict__ child_fam,
                                                     const int32_t* __restrict__ bad, double min_info, double* __restrict__ state,
                                                     double* __restrict__ delta, double* __restrict__ lr,
                                                     double* __restrict__ hinf, double* __restrict__ cand) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A.n_sites) return;   // (a lane past the range: no barrier follows, and no other lane's store is its to make)
  const int64_t as = (int64_t)A.site0 + s;
  const LgSite S = lg_site(M, F.n_rates, 1, as);
  const bool nan_site = bad[s] != 0;
  const double zero = 0.0;
  const double* theta = S.theta ? S.theta : &zero;
  for (int q = blockIdx.y; q < n; q += gridDim.y) {
    const int f = fams[q];
    double b_up = 0.0, s_up = 0.0, g_up = 0.0, k_up = 0.0;   // what the parent adds: nothing from a skipped family
    double dv = NAN, lv = NAN, hv = NAN, cv = NAN;
    if (!nan_site) {
      const FamUni X = fam_uni_family<SM>(A.pool, A.stride, A.off, A.bdim, F, M, Sh, Nz, Ms, S, A.fam_cluster, f, A.data_row_len, as);
      if (X.skip) {
        lv = X.np == 0 ? (double)NAN : 0.0;
      } else if (X.np == 0) {
        // a root-prior family has no edge, and nothing gathers from it
      } else if (!(X.q.ok && X.V > 0.0)) {
        b_up = s_up = g_up = k_up = NAN;   // (not reached at a site the validity pass accepts with positive variances)
      } else {
        const FamUniParent P = fam_uni_parent(F, M, S, X.q, f, 0, S.mu[0]);
        const double dopt = Op.regime ? lg_optima_d(Op, theta, S.alpha, F.length, F.gamma, f, F.K, X.np, 0, 1, as, A.data_row_len) : 0.0;
        double e = X.e - dopt;
        if (CS) {   // the offset gains wc_f times this site's deltas that cover f
          bool any;
          e = e - P.wc * lg_clade_sum(Cs, f, as, any);
        }
        const double kap = P.wc * X.j;
        double B = 0.0, Sv = 0.0, G = 0.0, K = 0.0;
        for (int c = child_off[f], c1 = child_off[f + 1]; c < c1; ++c) {
          const double* __restrict__ t = state + (int64_t)child_fam[c] * 4 * A.row + s;
          B = B + t[0];
          Sv = Sv + t[A.row];
          G = G + t[2 * A.row];
          K = K + t[3 * A.row];
        }
        const double g = G + kap * e;
        const double Kt = K + P.wc * kap;
        const double a = kap + B, b = -(kap * P.qc);
        const bool internal = X.cpos >= 0, has_u = P.pk >= 0;
        const double Vu = P.pk == 0 ? X.q.S00 : (P.pk == 1 ? X.q.S11 : 0.0);
        double Var;
        if (internal) {
          const double Vv = X.cpos == 0 ? X.q.S00 : X.q.S11;
          const double Cvu = has_u ? X.q.S01 : 0.0;
          Var = (a * a) * Vv;
          if (has_u) Var = (Var + ((2.0 * a) * b) * Cvu) + (b * b) * Vu;
          Var = Var + Sv;
          const double rho = has_u ? Cvu / Vu : 0.0;
          const double tau = has_u ? Vv - (Cvu * Cvu) / Vu : Vv;
          b_up = a * rho + b;
          s_up = Sv + (a * a) * tau;
        } else {
          Var = has_u ? (b * b) * Vu : 0.0;
          b_up = b;
          s_up = 0.0;
        }
        g_up = g;
        k_up = Kt;
        const double H = Kt - Var;
        if (H > min_info * Kt) {
          dv = g / H;
          lv = (g * g) / H;
          hv = H;
          if (isfinite(lv)) cv = lv;
        } else {
          lv = 0.0;   // not identified
        }
      }
    }
    double* __restrict__ t = state + (int64_t)f * 4 * A.row + s;
    t[0] = b_up;
    t[A.row] = s_up;
    t[2 * A.row] = g_up;
    t[3 * A.row] = k_up;
    const int64_t o = (int64_t)f * A.row + s;
    if (delta) delta[o] = dv;
    if (lr) lr[o] = lv;
    if (hinf) hinf[o] = hv;
    if (cand) cand[o] = cv;
  }
}

// The score at a site's own slots (pgbp_lg_clade_shift_score_sites): thread = (slot, site) picks row family[slot][site] of the
// scan's state (g: row 2, Kt: row 3) and of its information table.  An empty slot and a failed site are NaN; a slot that is not
// identified has NaN information, as in the scan.  g, h, kt: [n_slots][row]
__global__ __launch_bounds__(256) void optscan_gather_slots(LgCladeShifts Cs, int site0, int n_sites, int64_t row,
                                                            const int32_t* __restrict__ bad, const double* __restrict__ state,
                                                            const double* __restrict__ hinf, double* __restrict__ g,
                                                            double* __restrict__ h, double* __restrict__ kt) {
  const int s = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (s >= n_sites) return;
  const int v = Cs.family[(int64_t)j * Cs.row + site0 + s];
  double gv = NAN, hv = NAN, kv = NAN;
  if (v >= 0 && bad[s] == 0) {
    const double* __restrict__ t = state + (int64_t)v * 4 * row + s;
    gv = t[2 * row];
    kv = t[3 * row];
    hv = hinf[(int64_t)v * row + s];
  }
  const int64_t o = (int64_t)j * row + s;
  g[o] = gv;
  h[o] = hv;
  kt[o] = kv;
}

// pbest / pfam: [blocks][row], the largest candidate of the block's families and the first family that has it (-inf, -1: none)
__global__ __launch_bounds__(256) void optscan_top(const double* __restrict__ cand, int n_fam, int n_sites, int64_t row,
                                                   double* __restrict__ pbest, int32_t* __restrict__ pfam) {
  const int s = blockIdx.x * 256 + threadIdx.x, fb = blockIdx.y;
  if (s >= n_sites) return;
  double best = -INFINITY;
  int bf = -1;
  const int f0 = fb * kFamUniBlock, f1 = min(f0 + kFamUniBlock, n_fam);
  for (int f = f0; f < f1; ++f) {
    const double v = cand[(int64_t)f * row + s];
    if (v > best) {   // (false for NaN: not a candidate)
      best = v;
      bf = f;
    }
  }
  pbest[(int64_t)fb * row + s] = best;
  pfam[(int64_t)fb * row + s] = bf;
}

// the blocks in index order with a strict >, so that ties go to the lowest family; NaN and -1 at a failed site
__global__ __launch_bounds__(256) void optscan_top_fold(const double* __restrict__ pbest, const int32_t* __restrict__ pfam, int nb,
                                                        int n_sites, int64_t row, const int32_t* __restrict__ bad,
                                                        double* __restrict__ top_lr, int32_t* __restrict__ top_family, int out0) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_sites) return;
  double best = -INFINITY;
  int bf = -1;
  for (int b = 0; b < nb; ++b) {
    const double v = pbest[(int64_t)b * row + s];
    if (v > best) {
      best = v;
      bf = pfam[(int64_t)b * row + s];
    }
  }
  const bool failed = bad[s] != 0;
  top_lr[out0 + s] = failed ? (double)NAN : best;
  top_family[out0 + s] = failed ? -1 : bf;
}

}  // namespace pgbp

using namespace pgbp;

// ms (pgbp_lg_optimum_scan_sites_timed): the stream is drained after every phase and the wall time of the phase is added to
// ms[0 .. 3] = {validity pass, height launches, top fold, copies}; launches: the number of height launches of the call
static int optimum_scan_sites(pgbp_engine* e, const char* fn, int32_t site_begin, int32_t site_end, double min_info, double* delta,
                              double* lr, double* information, double* top_lr, int32_t* top_family, int32_t* info, double* ms,
                              int32_t* launches, double* slot_g = nullptr, double* slot_h = nullptr, double* slot_kt = nullptr) {
  if (!e) return PGBP_ERR_INVALID;
  SitesCall c{};
  const bool score = slot_g || slot_h || slot_kt;   // pgbp_lg_clade_shift_score_sites: the rows of every site's own slots
  const bool none = !score && !delta && !lr && !information && !top_lr && !top_family;
  int rc = sites_accept(e, fn, "pgbp_lg_set_optima and two pgbp_loglik per clade", site_begin, site_end, none ? "no output buffer" : nullptr, &c);
  if (rc) return rc;
  const LgModel* L = c.L;
  if (L->M.model != PGBP_LG_OU)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": the last pgbp_lg_assignfactors was a Brownian-motion fill, under which "
                                                "wc = 0 and an optimum has no effect (use pgbp_lg_shift_scan_sites for a jump of the mean)");
  if (!L->optscan.built)
    return engine_fail(e, PGBP_ERR_STATE, std::string(fn) + ": no topology (call pgbp_lg_set_topology first)");
  {
    std::string why;
    if (!optscan_plan_single_parents(L->optscan, L->T.n_parents.data(), why)) return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": " + why);
  }
  if (!(min_info >= 0.0 && min_info < 1.0))
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": min_info = " + std::to_string(min_info) + " is not in [0, 1)");
  SampPlan sp;   // the validity pass runs on schedule tree 0 (the clique tree of a tree)
  rc = sample_plan(e, std::string(fn) + ": ", 0, site_begin, site_end, 1, "n_cols", "column", []() { return std::string(); }, sp);
  if (rc) return rc;
  const OptScanPlan& P = L->optscan;
  const int ns = c.ns, nf = L->T.n_families;
  const PostUniPre pre = post_uni_pre(sp);
  const int nfb = std::max(1, (nf + kFamUniBlock - 1) / kFamUniBlock);
  const bool top = top_lr || top_family;
  const LgCladeShifts Cs = L->clade_in_force();
  if (score && !Cs.family)
    return engine_fail(e, PGBP_ERR_STATE, std::string(fn) + ": no clade shifts are in force (call pgbp_lg_set_clade_shifts_sites first)");
  const int n_slots = score ? Cs.n_slots : 0;
  const bool want_h = information || score;
  const int n_tab = (delta ? 1 : 0) + (lr ? 1 : 0) + (want_h ? 1 : 0);
  const int64_t per_site = optscan_per_site(nf, n_tab, top, nfb, pre.nvb) + 3 * (int64_t)n_slots;
  const int64_t limit = g_fam_uni_limit.load();
  if (256 * per_site > limit)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": the state rows and the requested tables of one workgroup of 256 sites take " +
                                                std::to_string(256 * per_site) + " doubles of scratch, above the limit of " +
                                                std::to_string(limit) + " doubles (pgbp_sites_sweep_scratch_limit: " +
                                                std::to_string(256 * per_site) + " suffices)");
  if (launches) *launches = 0;
  if (ns == 0) return PGBP_OK;
  const int chunk = fam_uni_chunk(ns, per_site);
  const LgOptima Op = L->optima_in_force();
  std::vector<int32_t> rank(ns, 0);
  DevBuf<SampItem> d_tab;
  DevBuf<int32_t> d_idx, d_pfirst, d_rank, d_fcl, d_pfam, d_topf;
  DevBuf<double> d_state, d_delta, d_lr, d_hinf, d_cand, d_pbest, d_top, d_sg, d_sh, d_sk;
  const size_t tab = (size_t)std::max(1, nf) * chunk, blk = (size_t)nfb * chunk;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_tab, std::max<size_t>(1, pre.tab.size()));
  S.alloc(d_idx, std::max<size_t>(1, sp.idx.size()));
  S.alloc(d_pfirst, (size_t)std::max(1, pre.nvb) * chunk);
  S.alloc(d_rank, ns);
  S.alloc(d_fcl, std::max(1, nf));
  S.alloc(d_state, 4 * tab);
  S.alloc(d_delta, tab, delta != nullptr);
  S.alloc(d_lr, tab, lr != nullptr);
  S.alloc(d_hinf, tab, want_h);
  S.alloc(d_sg, (size_t)std::max(1, n_slots) * chunk, score);
  S.alloc(d_sh, (size_t)std::max(1, n_slots) * chunk, score);
  S.alloc(d_sk, (size_t)std::max(1, n_slots) * chunk, score);
  S.alloc(d_cand, tab, top);
  S.alloc(d_pbest, blk, top);
  S.alloc(d_pfam, blk, top);
  S.alloc(d_top, ns, top);
  S.alloc(d_topf, ns, top);
  S.upload(d_tab, pre.tab.data(), pre.tab.size());
  S.upload(d_idx, sp.idx.data(), sp.idx.size());
  S.upload(d_fcl, L->T.cluster.data(), nf);
  if ((rc = S.ready())) return rc;
  SitesClock phase(S, ms, 4);
  const int nh = P.n_heights();
  int n_launch = 0;
  for (int s0 = 0; S.ok() && s0 < ns; s0 += chunk) {
    const int n = std::min(chunk, ns - s0);
    const SitesArgs A = sites_args(c, site_begin + s0, n, chunk, d_fcl.get());
    const dim3 gs((n + 255) / 256);
    if (pre.n_pre > 0) {
      post_uni_validity(S, c.U.sm, A, pre, d_tab.get(), d_idx.get(), d_pfirst.get(), d_rank.get(), s0);
    } else if (S.ok()) {
      S.err = hipMemsetAsync(d_rank.get() + s0, 0, sizeof(int32_t) * (size_t)n, S.st);   // no cluster has a variable
    }
    phase(0);
    for (int h = 0; h < nh; ++h) {
      const int nq = P.height_off[h + 1] - P.height_off[h];
      if (nq == 0) continue;
      const dim3 gl(gs.x, std::min(nq, 65535));
#define PGBP_OPTSCAN_LEVEL(SM_, CS_)                                                                                              \
  S.launch(optscan_level<SM_, CS_>, gl, A, L->F, L->M, L->Sh, Op, L->Nz, L->Ms, Cs, L->d_os_height_fam.get() + P.height_off[h], \
           nq, L->d_os_child_off.get(), L->d_os_child_fam.get(), d_rank.get() + s0, min_info, d_state.get(), d_delta.get(),     \
           d_lr.get(), d_hinf.get(), d_cand.get())
      if (Cs.family) {
        if (c.U.sm) PGBP_OPTSCAN_LEVEL(true, true); else PGBP_OPTSCAN_LEVEL(false, true);
      } else {
        if (c.U.sm) PGBP_OPTSCAN_LEVEL(true, false); else PGBP_OPTSCAN_LEVEL(false, false);
      }
#undef PGBP_OPTSCAN_LEVEL
      ++n_launch;
    }
    if (score)
      S.launch(optscan_gather_slots, dim3(gs.x, n_slots), Cs, site_begin + s0, n, (int64_t)chunk, d_rank.get() + s0, d_state.get(),
               d_hinf.get(), d_sg.get(), d_sh.get(), d_sk.get());
    S.check();
    phase(1);
    if (top) {
      S.launch(optscan_top, dim3(gs.x, nfb), d_cand.get(), nf, n, (int64_t)chunk, d_pbest.get(), d_pfam.get());
      S.launch(optscan_top_fold, gs, d_pbest.get(), d_pfam.get(), nfb, n, (int64_t)chunk, d_rank.get() + s0, d_top.get(), d_topf.get(),
               s0);
      S.check();
    }
    phase(2);
    S.rows(delta, ns, s0, d_delta.get(), chunk, n, nf);
    S.rows(lr, ns, s0, d_lr.get(), chunk, n, nf);
    S.rows(information, ns, s0, d_hinf.get(), chunk, n, nf);
    S.rows(slot_g, ns, s0, d_sg.get(), chunk, n, n_slots);
    S.rows(slot_h, ns, s0, d_sh.get(), chunk, n, n_slots);
    S.rows(slot_kt, ns, s0, d_sk.get(), chunk, n, n_slots);
    phase(3);
  }
  S.download(rank.data(), d_rank.get(), ns);
  S.download(top_lr, d_top.get(), ns);
  S.download(top_family, d_topf.get(), ns);
  if ((rc = S.finish())) return rc;
  phase(3);
  post_uni_info(pre, rank, info);
  if (launches) *launches = n_launch;
  return PGBP_OK;
}

extern "C" int pgbp_lg_optimum_scan_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double min_info, double* delta,
                                          double* lr, double* information, double* top_lr, int32_t* top_family, int32_t* info) {
  return optimum_scan_sites(e, "pgbp_lg_optimum_scan_sites", site_begin, site_end, min_info, delta, lr, information, top_lr,
                            top_family, info, nullptr, nullptr);
}

extern "C" int pgbp_lg_optimum_scan_sites_timed(pgbp_engine* e, int32_t site_begin, int32_t site_end, double min_info, double* delta,
                                                double* lr, double* information, double* top_lr, int32_t* top_family,
                                                int32_t* info, double* ms4, int32_t* launches) {
  if (e && !ms4) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_optimum_scan_sites_timed: no buffer for the phase times");
  return optimum_scan_sites(e, "pgbp_lg_optimum_scan_sites_timed", site_begin, site_end, min_info, delta, lr, information, top_lr,
                            top_family, info, ms4, launches);
}

extern "C" int pgbp_lg_clade_shift_score_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double min_info, double* g,
                                               double* information, double* kt, int32_t* info) {
  if (e && (!g || !information || !kt))
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_clade_shift_score_sites: no output buffer");
  return optimum_scan_sites(e, "pgbp_lg_clade_shift_score_sites", site_begin, site_end, min_info, nullptr, nullptr, nullptr, nullptr,
                            nullptr, info, nullptr, nullptr, g, information, kt);
}

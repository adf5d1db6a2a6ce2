// The three per-family sweeps over calibrated beliefs for univariate batches on a thread-per-site engine, lanes = sites:
// pgbp_lg_shift_scan_sites, pgbp_lg_edge_gradient_sites and pgbp_lg_loo_sites of include/pgbp.h -- the p = 1 cases of
// pgbp_scan.hip, pgbp_edge.hip and pgbp_loo.hip in the frame of pgbp_grad_uni.hip: a workgroup is 256 consecutive sites, grid.y
// a block of kFamUniBlock consecutive families (tip families for the leave-one-out sweep), a thread walks its block in index
// order for its one site.  The family table is uniform across a wavefront (scalar loads); the belief entries and the tip data
// are read as whole lines in the layout the pool is in (site-minor from 64 sites on, plain below: template <bool SM>), so the
// calls convert nothing and leave the layout as they found it.
//
// Per (family, site) everything is closed form (pgbp_fam_uni_dev.hpp): with V, j = 1 / V, e = E[r], C = u' Sigma u, g_w = j e
//   scan:  H = j - (j C) j (from C itself, never from M = C + e^2); identified iff H > min_info j; jump = g_w / H, lr = g_w^2 / H;
//   edge:  G_V = (j M j - j) / 2, g_qk = j (e x_k + (Sigma u)[v_k]), dX_k = dvc G_V R[colour_k] + dwc theta g_w + dqc g_qk;
//   loo:   D = V - C, determined iff D > 2^-40 V and V > 0; var = V^2 / D, mean = y - V e / D,
//          lpd = -(log 2pi + 2 log V - log D + e^2 / D) / 2.
// Outputs are site-minor: a row of sites per (family[, entry]), so every store is a whole line and nothing is transposed.  No
// family's output depends on another's; what does reduce across families -- the site's info, the scan's (top_lr, top_family)
// and the leave-one-out total -- is kept per block by the thread and folded by fam_uni_fold in block order.  No barrier, no
// atomics, contraction off, every sum in a fixed order, no lane's store depends on another lane: the bytes of a site depend
// neither on the call nor on the site range or the chunks it came in.  The rows of a chunk of sites at a time go through
// scratch (256 MB at most, whole workgroups: pgbp_sites_sweep_scratch_limit) and are copied into the caller's rows by strided
// copies; one stream synchronisation per call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <vector>

#include "pgbp_devmem.hpp"
#include "pgbp_fam_uni_dev.hpp"
#include "pgbp_sites_host.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"

namespace pgbp {

#define PGBP_FAM_UNI_LOG2PI 1.8378770664093454835606594728112

// jump, lr, hinf: [n_fam][row] (any may be null); pbest / pfam: [blocks][row], the largest lr of the block's families that
// have an edge, are identified and whose lr is finite, and the first family that has it (-inf, -1: none); pinfo: [blocks][row]
template <bool SM>
__global__ __launch_bounds__(256) void fam_uni_scan(SitesArgs A, LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz, LgSiteMiss Ms,
                                                    int n_fam, double min_info, double* __restrict__ jump, double* __restrict__ lr,
                                                    double* __restrict__ hinf, double* __restrict__ pbest,
                                                    int32_t* __restrict__ pfam, int32_t* __restrict__ pinfo) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x, fb = blockIdx.y;
  if (s >= A.n_sites) return;   // (a lane past the range: no barrier follows, and no other lane's store is its to make)
  const int64_t as = (int64_t)A.site0 + s;
  const LgSite S = lg_site(M, F.n_rates, 1, as);
  double best = -INFINITY;
  int bf = -1, bad = kFamUniNoInfo;
  const int f0 = fb * kFamUniBlock, f1 = min(f0 + kFamUniBlock, n_fam);
  for (int f = f0; f < f1; ++f) {
    const FamUni X = fam_uni_family<SM>(A.pool, A.stride, A.off, A.bdim, F, M, Sh, Nz, Ms, S, A.fam_cluster, f, A.data_row_len, as);
    double jv = NAN, lv = NAN, hv = NAN;
    if (X.skip) {
      lv = X.np == 0 ? (double)NAN : 0.0;
    } else if (X.np == 0) {   // a root-prior family has no edge; its cluster's failure is reported
      if (!X.q.ok) bad = min(bad, X.c + 1);
    } else if (!(X.q.ok && X.V > 0.0)) {
      bad = min(bad, X.c + 1);
    } else {
      const double H = X.j - (X.j * X.C) * X.j;
      if (H > min_info * X.j) {
        jv = X.gw / H;
        lv = (X.gw * X.gw) / H;
        hv = H;
        if (isfinite(lv) && lv > best) {
          best = lv;
          bf = f;
        }
      } else {
        lv = 0.0;   // not identified
      }
    }
    const int64_t o = (int64_t)f * A.row + s;
    if (jump) jump[o] = jv;
    if (lr) lr[o] = lv;
    if (hinf) hinf[o] = hv;
  }
  const int64_t o = (int64_t)fb * A.row + s;
  if (pbest) {
    pbest[o] = best;
    pfam[o] = bf;
  }
  pinfo[o] = bad;
}

// dlen, dgam: [n_fam][K][row], dshift: [n_fam][row] (any may be null); pinfo: [blocks][row]
template <bool SM>
__global__ __launch_bounds__(256) void fam_uni_edge(SitesArgs A, LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz, LgSiteMiss Ms, int n_fam,
                                                    double* __restrict__ dlen, double* __restrict__ dgam,
                                                    double* __restrict__ dshift, int32_t* __restrict__ pinfo) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x, fb = blockIdx.y;
  if (s >= A.n_sites) return;
  const int64_t as = (int64_t)A.site0 + s;
  const int K = F.K;
  const LgSite S = lg_site(M, F.n_rates, 1, as);
  const double mu = S.mu[0], theta = S.theta ? S.theta[0] : 0.0;
  int bad = kFamUniNoInfo;
  const int f0 = fb * kFamUniBlock, f1 = min(f0 + kFamUniBlock, n_fam);
  for (int f = f0; f < f1; ++f) {
    const FamUni X = fam_uni_family<SM>(A.pool, A.stride, A.off, A.bdim, F, M, Sh, Nz, Ms, S, A.fam_cluster, f, A.data_row_len, as);
    const int np = X.np;
    const bool fail = !X.skip && !(X.q.ok && X.V > 0.0);
    if (fail) bad = min(bad, X.c + 1);
    const double Mx = X.C + X.e * X.e;
    const double G = 0.5 * ((X.j * Mx) * X.j - X.j);
    if (dshift) dshift[(int64_t)f * A.row + s] = X.skip ? 0.0 : (fail ? (double)NAN : X.gw);
    if (!dlen && !dgam) continue;
    for (int k = 0; k < K; ++k) {
      double dl = NAN, dg = NAN;   // no such edge (every entry of a root-prior family), or a failed site
      if (k < np && X.skip) {
        dl = dg = 0.0;
      } else if (k < np && !fail) {
        const FamUniParent P = fam_uni_parent(F, M, S, X.q, f, k, mu);
        const LgEdgeDerivs d = lg_coefs_dedge(M.model, S.alpha, F.length[(size_t)f * K + k], F.gamma[(size_t)f * K + k]);
        const double su = P.pk == 0 ? X.su0 : (P.pk == 1 ? X.su1 : 0.0);
        const double gq = X.j * (X.e * P.xk + su);
        const double trGR = G * S.R[P.col];
        const double thg = S.theta ? theta * X.gw : 0.0;
        dl = d.v_t * trGR + d.w_t * thg + d.q_t * gq;
        dg = d.v_g * trGR + d.w_g * thg + d.q_g * gq;
        if (Sh.slot && Sh.slot[(size_t)f * K + k] >= 0)   // the shift's coefficient is gamma_k: + s_k g_w
          dg = dg + lg_shift_value(Sh, (int64_t)f * K + k, 0, 1, as) * X.gw;
      }
      const int64_t o = ((int64_t)f * K + k) * A.row + s;
      if (dlen) dlen[o] = dl;
      if (dgam) dgam[o] = dg;
    }
  }
  pinfo[(int64_t)fb * A.row + s] = bad;
}

// tip_fam[ti]: the family of tip ti.  mean, var (either may be null), lpd: [n_tip][row]; info: [n_tip][row] (may be null);
// psum: [blocks][row], the block's lpd added in tip order
template <bool SM>
__global__ __launch_bounds__(256) void fam_uni_loo(SitesArgs A, LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz, LgSiteMiss Ms,
                                                   const int32_t* __restrict__ tip_fam, int n_tip, double* __restrict__ mean,
                                                   double* __restrict__ var, double* __restrict__ lpd,
                                                   int32_t* __restrict__ info, double* __restrict__ psum) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x, tb = blockIdx.y;
  if (s >= A.n_sites) return;
  const int64_t as = (int64_t)A.site0 + s;
  const LgSite S = lg_site(M, F.n_rates, 1, as);
  double acc = 0.0;
  const int t0 = tb * kFamUniBlock, t1 = min(t0 + kFamUniBlock, n_tip);
  for (int ti = t0; ti < t1; ++ti) {
    const int f = tip_fam[ti];
    const FamUni X = fam_uni_family<SM>(A.pool, A.stride, A.off, A.bdim, F, M, Sh, Nz, Ms, S, A.fam_cluster, f, A.data_row_len, as);
    double mv = NAN, vv = NAN, lv = NAN;
    int st = 1;
    if (X.masked) {
      st = PGBP_INFO_NOT_OBSERVED;   // not observed at this site: nothing to leave out, nothing for the total
    } else if (!X.skip && X.q.st != 0) {
      st = X.q.st > 0 ? 1 + X.q.st : 1;   // the cluster is not positive definite; the constant belief: u is undetermined
    } else if (!X.skip) {
      const double D = X.V - X.C;   // S = Var(u) = u' Sigma u over the cluster parents
      if (D > X.V * kLooPivotFloor && X.V > 0.0) {
        st = 0;
        vv = (X.V * X.V) / D;
        mv = X.y - (X.V * X.e) / D;
        lv = -0.5 * (((PGBP_FAM_UNI_LOG2PI + 2.0 * log(X.V)) - log(D)) + (X.e * X.e) / D);
      }
    }
    const int64_t o = (int64_t)ti * A.row + s;
    if (mean) mean[o] = mv;
    if (var) var[o] = vv;
    lpd[o] = lv;
    if (info) info[o] = st;
    if (!X.masked) acc = acc + lv;
  }
  psum[(int64_t)tb * A.row + s] = acc;
}

// Folds the blocks' records of a site in block order; any group of inputs may be null.  info[out0 + site]: the smallest mark
// of a block, 0: none.  (top_lr, top_family): the largest pbest with a strict >, so that ties go to the lowest family; -inf
// and -1 when no block has one, NaN and -1 at a failed site.  total: the psum added in block order.
__global__ __launch_bounds__(256) void fam_uni_fold(const int32_t* __restrict__ pinfo, const double* __restrict__ pbest,
                                                    const int32_t* __restrict__ pfam, const double* __restrict__ psum, int nb,
                                                    int n_sites, int64_t row, int32_t* __restrict__ info,
                                                    double* __restrict__ top_lr, int32_t* __restrict__ top_family,
                                                    double* __restrict__ total, int out0) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_sites) return;
  int bad = kFamUniNoInfo;
  if (pinfo) {
    for (int b = 0; b < nb; ++b) bad = min(bad, pinfo[(int64_t)b * row + s]);
    info[out0 + s] = bad == kFamUniNoInfo ? 0 : bad;
  }
  if (pbest) {
    double best = -INFINITY;
    int bf = -1;
    for (int b = 0; b < nb; ++b) {
      const double v = pbest[(int64_t)b * row + s];
      if (v > best) {
        best = v;
        bf = pfam[(int64_t)b * row + s];
      }
    }
    const bool failed = bad != kFamUniNoInfo;
    top_lr[out0 + s] = failed ? (double)NAN : best;
    top_family[out0 + s] = failed ? -1 : bf;
  }
  if (psum) {
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc = acc + psum[(int64_t)b * row + s];
    total[out0 + s] = acc;
  }
}

// (pgbp_sites_host.hpp: the host frame of every lanes-are-sites call)
std::atomic<int64_t> g_fam_uni_limit{(int64_t)32 << 20};

namespace {

// every row of a failed site: NaN
void fam_uni_nan(double* out, int64_t rows, int ns, int s) {
  if (!out) return;
  for (int64_t r = 0; r < rows; ++r) out[r * ns + s] = NAN;
}

}  // namespace

}  // namespace pgbp

using namespace pgbp;

extern "C" void pgbp_sites_sweep_scratch_limit(int64_t doubles) { g_fam_uni_limit.store(doubles > 0 ? doubles : (int64_t)32 << 20); }

extern "C" int pgbp_lg_shift_scan_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double min_info, double* jump,
                                        double* lr, double* information, double* top_lr, int32_t* top_family, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_lg_shift_scan_sites";
  SitesCall c{};
  const bool none = !jump && !lr && !information && !top_lr && !top_family;
  int rc = sites_accept(e, fn, "pgbp_lg_shift_scan", site_begin, site_end, none ? "no output buffer" : nullptr, &c);
  if (rc) return rc;
  if ((rc = lg_refuse_optima(e, fn, c.L))) return rc;
  if (!(min_info >= 0.0 && min_info < 1.0))
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": min_info = " + std::to_string(min_info) + " is not in [0, 1)");
  const LgModel* L = c.L;
  const int ns = c.ns, nf = L->T.n_families;
  if (ns == 0) return PGBP_OK;
  const int nfb = std::max(1, (nf + kFamUniBlock - 1) / kFamUniBlock);
  const bool top = top_lr || top_family;
  const int n_tab = (jump ? 1 : 0) + (lr ? 1 : 0) + (information ? 1 : 0);
  const int chunk = fam_uni_chunk(ns, (int64_t)nf * n_tab + 3 * (int64_t)nfb);
  std::vector<int32_t> inf(ns, 0);
  DevBuf<int32_t> d_fcl, d_pinfo, d_pfam, d_info, d_topf;
  DevBuf<double> d_jump, d_lr, d_hinf, d_pbest, d_top;
  const size_t tab = (size_t)nf * chunk, blk = (size_t)nfb * chunk;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_fcl, std::max(1, nf));
  S.alloc(d_jump, tab, jump != nullptr);
  S.alloc(d_lr, tab, lr != nullptr);
  S.alloc(d_hinf, tab, information != nullptr);
  S.alloc(d_pinfo, blk);
  S.alloc(d_pbest, blk, top);
  S.alloc(d_pfam, blk, top);
  S.alloc(d_info, ns);
  S.alloc(d_top, ns, top);
  S.alloc(d_topf, ns, top);
  S.upload(d_fcl, L->T.cluster.data(), nf);
  if ((rc = S.ready())) return rc;
  for (int s0 = 0; S.ok() && s0 < ns; s0 += chunk) {
    const int n = std::min(chunk, ns - s0);
    const SitesArgs A = sites_args(c, site_begin + s0, n, chunk, d_fcl.get());
    const dim3 grid((n + 255) / 256, nfb);
    PGBP_SITES_LAUNCH(S, c.U.sm, fam_uni_scan, grid, A, L->F, L->M, L->Sh, L->Nz, L->Ms, nf, min_info, d_jump.get(), d_lr.get(),
                      d_hinf.get(), d_pbest.get(), d_pfam.get(), d_pinfo.get());
    S.launch(fam_uni_fold, dim3(grid.x), d_pinfo.get(), d_pbest.get(), d_pfam.get(), nullptr, nfb, n, (int64_t)chunk, d_info.get(),
             d_top.get(), d_topf.get(), nullptr, s0);
    S.check();
    S.rows(jump, ns, s0, d_jump.get(), chunk, n, nf);
    S.rows(lr, ns, s0, d_lr.get(), chunk, n, nf);
    S.rows(information, ns, s0, d_hinf.get(), chunk, n, nf);
  }
  S.download(inf.data(), d_info.get(), ns);
  S.download(top_lr, d_top.get(), ns);
  S.download(top_family, d_topf.get(), ns);
  if ((rc = S.finish())) return rc;
  for (int s = 0; s < ns; ++s) {
    if (info) info[s] = inf[s];
    if (!inf[s]) continue;   // a site with a cluster that is not positive definite: NaN throughout
    fam_uni_nan(jump, nf, ns, s);
    fam_uni_nan(lr, nf, ns, s);
    fam_uni_nan(information, nf, ns, s);
  }
  return PGBP_OK;
}

extern "C" int pgbp_lg_edge_gradient_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dlength, double* dgamma,
                                           double* dshift, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_lg_edge_gradient_sites";
  SitesCall c{};
  const bool none = !dlength && !dgamma && !dshift;
  int rc = sites_accept(e, fn, "pgbp_lg_edge_gradient", site_begin, site_end, none ? "no output buffer" : nullptr, &c);
  if (rc) return rc;
  if ((rc = lg_refuse_optima(e, fn, c.L))) return rc;
  const LgModel* L = c.L;
  const int ns = c.ns, nf = L->T.n_families, K = L->F.K;
  if (ns == 0) return PGBP_OK;
  const int nfb = std::max(1, (nf + kFamUniBlock - 1) / kFamUniBlock);
  const int chunk = fam_uni_chunk(ns, (int64_t)nf * ((dlength ? K : 0) + (dgamma ? K : 0) + (dshift ? 1 : 0)) + nfb);
  std::vector<int32_t> inf(ns, 0);
  DevBuf<int32_t> d_fcl, d_pinfo, d_info;
  DevBuf<double> d_len, d_gam, d_shift;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_fcl, std::max(1, nf));
  S.alloc(d_len, (size_t)nf * K * chunk, dlength != nullptr);
  S.alloc(d_gam, (size_t)nf * K * chunk, dgamma != nullptr);
  S.alloc(d_shift, (size_t)nf * chunk, dshift != nullptr);
  S.alloc(d_pinfo, (size_t)nfb * chunk);
  S.alloc(d_info, ns);
  S.upload(d_fcl, L->T.cluster.data(), nf);
  if ((rc = S.ready())) return rc;
  for (int s0 = 0; S.ok() && s0 < ns; s0 += chunk) {
    const int n = std::min(chunk, ns - s0);
    const SitesArgs A = sites_args(c, site_begin + s0, n, chunk, d_fcl.get());
    const dim3 grid((n + 255) / 256, nfb);
    PGBP_SITES_LAUNCH(S, c.U.sm, fam_uni_edge, grid, A, L->F, L->M, L->Sh, L->Nz, L->Ms, nf, d_len.get(), d_gam.get(), d_shift.get(),
                      d_pinfo.get());
    S.launch(fam_uni_fold, dim3(grid.x), d_pinfo.get(), nullptr, nullptr, nullptr, nfb, n, (int64_t)chunk, d_info.get(), nullptr,
             nullptr, nullptr, s0);
    S.check();
    S.rows(dlength, ns, s0, d_len.get(), chunk, n, (int64_t)nf * K);
    S.rows(dgamma, ns, s0, d_gam.get(), chunk, n, (int64_t)nf * K);
    S.rows(dshift, ns, s0, d_shift.get(), chunk, n, nf);
  }
  S.download(inf.data(), d_info.get(), ns);
  if ((rc = S.finish())) return rc;
  for (int s = 0; s < ns; ++s) {
    if (info) info[s] = inf[s];
    if (!inf[s]) continue;   // a site with a cluster that is not positive definite: every entry NaN
    fam_uni_nan(dlength, (int64_t)nf * K, ns, s);
    fam_uni_nan(dgamma, (int64_t)nf * K, ns, s);
    fam_uni_nan(dshift, nf, ns, s);
  }
  return PGBP_OK;
}

extern "C" int pgbp_lg_loo_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* mean, double* var, double* lpd,
                                 double* total, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_lg_loo_sites";
  SitesCall c{};
  int rc = sites_accept(e, fn, "pgbp_lg_loo", site_begin, site_end, lpd ? nullptr : "no output buffer (lpd)", &c);
  if (rc) return rc;
  if ((rc = lg_refuse_optima(e, fn, c.L))) return rc;
  const LgModel* L = c.L;
  const std::vector<int32_t> tips = L->T.loo_tips();   // the tip families, in table order
  const int ns = c.ns, nf = L->T.n_families, nt = (int)tips.size();
  if (ns == 0) return PGBP_OK;
  if (nt == 0) {
    if (total) std::fill(total, total + ns, 0.0);
    return PGBP_OK;
  }
  const int ntb = (nt + kFamUniBlock - 1) / kFamUniBlock;
  const int chunk = fam_uni_chunk(ns, (int64_t)nt * (1 + (mean ? 1 : 0) + (var ? 1 : 0) + (info ? 1 : 0)) + ntb);
  DevBuf<int32_t> d_fcl, d_tips, d_info;
  DevBuf<double> d_mean, d_var, d_lpd, d_psum, d_total;
  const size_t tab = (size_t)nt * chunk;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_fcl, std::max(1, nf));
  S.alloc(d_tips, nt);
  S.alloc(d_mean, tab, mean != nullptr);
  S.alloc(d_var, tab, var != nullptr);
  S.alloc(d_lpd, tab);
  S.alloc(d_info, tab, info != nullptr);
  S.alloc(d_psum, (size_t)ntb * chunk);
  S.alloc(d_total, ns);
  S.upload(d_fcl, L->T.cluster.data(), nf);
  S.upload(d_tips, tips.data(), nt);
  if ((rc = S.ready())) return rc;
  for (int s0 = 0; S.ok() && s0 < ns; s0 += chunk) {
    const int n = std::min(chunk, ns - s0);
    const SitesArgs A = sites_args(c, site_begin + s0, n, chunk, d_fcl.get());
    const dim3 grid((n + 255) / 256, ntb);
    PGBP_SITES_LAUNCH(S, c.U.sm, fam_uni_loo, grid, A, L->F, L->M, L->Sh, L->Nz, L->Ms, d_tips.get(), nt, d_mean.get(), d_var.get(),
                      d_lpd.get(), d_info.get(), d_psum.get());
    S.launch(fam_uni_fold, dim3(grid.x), nullptr, nullptr, nullptr, d_psum.get(), ntb, n, (int64_t)chunk, nullptr, nullptr, nullptr,
             d_total.get(), s0);
    S.check();
    S.rows(mean, ns, s0, d_mean.get(), chunk, n, nt);
    S.rows(var, ns, s0, d_var.get(), chunk, n, nt);
    S.rows(lpd, ns, s0, d_lpd.get(), chunk, n, nt);
    S.rows(info, ns, s0, d_info.get(), chunk, n, nt);
  }
  S.download(total, d_total.get(), ns);
  return S.finish();
}

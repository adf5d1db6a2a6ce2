// What a user asks of a fitted univariate batch on a thread-per-site engine, lanes = sites: pgbp_moments_sites,
// pgbp_sample_posterior_sites and pgbp_lg_impute_sites of include/pgbp.h -- the cases of pgbp_moments.hip, pgbp_sample.hip and
// pgbp_impute.hip at p = 1 with every belief of at most 2 variables, in the frame of pgbp_fam_uni.hip: a workgroup is 256
// consecutive sites, a thread holds one site and walks a block of kFamUniBlock wave-uniform table entries (listed beliefs,
// clusters in preorder, listed tip families) along grid.y.  The beliefs are read as whole lines in the layout the pool is in
// (template <bool SM>, engine_uni_view): nothing is converted, pgbp_layout is the same before and after.
//
// Per (entry, site) everything is closed form.  With the record [J | h | g] of a belief of m <= 2 variables:
//   moments: Sigma = J^-1, mu = Sigma h (fam_uni_moments), norm = g + ((m log 2pi - log det J) + h'mu) / 2, log det J = log a
//            (+ log of the Schur complement), the terms in that order;
//   draws:   a cluster with R random and S copied from its parent in the schedule tree (sample_plan's items by level):
//            r = 1: x_R = (a0 - G x_S) + T00 z_R,  a0 = h_R / J_RR, G = J_RS / J_RR, T00 = 1 / sqrt(J_RR);
//            r = 2: x_0 = a0 + (T00 z_0 + T01 z_1), x_1 = a1 + T11 z_1, a = J^-1 h, T = L^-T of J = L L';
//            the (at most five) coefficients are formed in registers by the level launch that uses them, once per (cluster,
//            site) and for all the draws of the launch -- no factor pool;
//   impute:  a listed tip observes nothing at p = 1: mean = E[u] + w, var = u' Sigma u + V over the cluster parents, with the
//            shifts and the tip noise in force (fam_uni_parent's coefficients, pgbp_impute.hip's info codes).
// Outputs are site-minor rows; a chunk of sites at a time goes through scratch bounded by pgbp_sites_sweep_scratch_limit and is
// copied to the caller's rows by strided copies; one stream synchronisation per call.  No barrier, no atomics, contraction off,
// every sum in a fixed order, no lane's store depends on another lane: a site's bytes depend neither on the call nor on the
// site range or the chunks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "pgbp_devmem.hpp"
#include "pgbp_fam_uni_dev.hpp"
#include "pgbp_sites_host.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"
#include "pgbp_philox_dev.hpp"
#include "pgbp_post_uni_dev.hpp"
#include "pgbp_sample_plan.hpp"

namespace pgbp {

#define PGBP_POST_UNI_LOG2PI 1.8378770664093454835606594728112

// ---- moments

// one listed belief: its first row of mean and of cov (the packed upper triangle: S00, S01, S11)
struct PostMomItem {
  int32_t belief, mean_row, cov_row;
};

// mean: [sum of dims][row], cov: [sum of m (m + 1) / 2][row] (may be null), norm: [n][row], info: [n][row] (may be null)
template <bool SM>
__global__ __launch_bounds__(256) void post_uni_moments(SitesArgs A, const PostMomItem* __restrict__ items, int n_items,
                                                        double* __restrict__ mean, double* __restrict__ cov,
                                                        double* __restrict__ norm, int32_t* __restrict__ info) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A.n_sites) return;   // (a lane past the range: no barrier follows, and no other lane's store is its to make)
  const int64_t as = (int64_t)A.site0 + s;
  const int i0 = blockIdx.y * kFamUniBlock, i1 = min(i0 + kFamUniBlock, n_items);
  for (int i = i0; i < i1; ++i) {
    const PostMomItem it = items[i];
    const int m = A.bdim[it.belief];
    const int64_t o = A.off[it.belief];
    const FamUniMom q = fam_uni_moments<SM>(A.pool, A.stride, o, m, as);
    const double g = fam_uni_ld<SM>(A.pool, A.stride, o, m * m + m, as);
    double mu0 = NAN, mu1 = NAN, S00 = NAN, S01 = NAN, S11 = NAN, nv = NAN;
    if (q.st == 0) {
      mu0 = q.m0; mu1 = q.m1; S00 = q.S00; S01 = q.S01; S11 = q.S11;
      double logdet, quad;
      if (m == 1) {
        logdet = log(fam_uni_ld<SM>(A.pool, A.stride, o, 0, as));
        quad = fam_uni_ld<SM>(A.pool, A.stride, o, 1, as) * q.m0;
      } else {
        const double a = fam_uni_ld<SM>(A.pool, A.stride, o, 0, as), b = fam_uni_ld<SM>(A.pool, A.stride, o, 2, as);
        const double sc = fam_uni_ld<SM>(A.pool, A.stride, o, 3, as) - (b / a) * b;
        logdet = log(a) + log(sc);
        quad = fam_uni_ld<SM>(A.pool, A.stride, o, 4, as) * q.m0 + fam_uni_ld<SM>(A.pool, A.stride, o, 5, as) * q.m1;
      }
      nv = g + 0.5 * (((double)m * PGBP_POST_UNI_LOG2PI - logdet) + quad);
    } else if (q.st < 0) {   // the constant belief, and a belief without variables: mu = Inf, norm = g, Sigma NaN
      mu0 = mu1 = INFINITY;
      nv = g;
    }
    if (m >= 1) mean[(int64_t)it.mean_row * A.row + s] = mu0;
    if (m == 2) mean[(int64_t)(it.mean_row + 1) * A.row + s] = mu1;
    if (cov) {
      if (m >= 1) cov[(int64_t)it.cov_row * A.row + s] = S00;
      if (m == 2) {
        cov[(int64_t)(it.cov_row + 1) * A.row + s] = S01;
        cov[(int64_t)(it.cov_row + 2) * A.row + s] = S11;
      }
    }
    norm[(int64_t)i * A.row + s] = nv;
    if (info) info[(int64_t)i * A.row + s] = q.st > 0 ? q.st : 0;
  }
}

// ---- imputation

// fam[ti]: the listed family ti, pred[ti]: its mask of predicted traits, dyn[ti] != 0: listed because the per-site mask hides it
// at some site, and observed (nothing to predict) at every other; mean, var (either may be null), info: [n_list][row]
template <bool SM>
__global__ __launch_bounds__(256) void post_uni_impute(SitesArgs A, LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz, LgSiteMiss Ms,
                                                       const int32_t* __restrict__ fam, const int32_t* __restrict__ fcl,
                                                       const unsigned long long* __restrict__ pred,
                                                       const int32_t* __restrict__ dyn, int n_list,
                                                       double* __restrict__ mean, double* __restrict__ var,
                                                       int32_t* __restrict__ info) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A.n_sites) return;
  const int64_t as = (int64_t)A.site0 + s;
  const int K = F.K;
  const LgSite S = lg_site(M, F.n_rates, 1, as);
  const double mu = S.mu[0], theta = S.theta ? S.theta[0] : 0.0;
  const int t0 = blockIdx.y * kFamUniBlock, t1 = min(t0 + kFamUniBlock, n_list);
  for (int ti = t0; ti < t1; ++ti) {
    const int f = fam[ti];
    double mv = NAN, vv = NAN;
    int st = -1;   // nothing of this tip is predicted: a cluster parent lacks the trait
    if (dyn[ti] && !lg_site_masked_family(Ms, F, f, as)) {
      st = PGBP_INFO_NOT_OBSERVED;   // observed at this site: nothing to impute
    } else if (pred[ti] & 1ull) {
      const int np = F.n_parents[f], c = fcl[ti];
      bool any_scope = false;
      for (int k = 0; k < np; ++k) any_scope |= F.parent_pos[(size_t)f * K + k] >= 0;
      FamUniMom q{0.0, 0.0, 0.0, 0.0, 0.0, 0, true};
      if (any_scope) q = fam_uni_moments<SM>(A.pool, A.stride, A.off[c], A.bdim[c], as);
      if (q.st != 0) {
        st = q.st > 0 ? 1 + q.st : 1;   // the cluster is not positive definite; the constant belief: no moments of the parents
      } else {
        double u0 = 0.0, u1 = 0.0, eu = 0.0, V = 0.0, w = 0.0;
        for (int k = 0; k < np; ++k) {
          const FamUniParent P = fam_uni_parent(F, M, S, q, f, k, mu);
          V = V + P.vc * S.R[P.col];
          if (S.theta) w = w + P.wc * theta;
          eu = eu + P.qc * P.xk;   // (the fixed root: its constant qc mu)
          if (P.pk == 0) u0 = u0 + P.qc;
          else if (P.pk == 1) u1 = u1 + P.qc;
        }
        if (Sh.slot) w = w + lg_shift_d(Sh, F.gamma, f, K, np, 0, 1, as);
        const int sn = lg_noise_slot(Nz, f);
        if (sn >= 0) V = V + lg_noise_E(Nz, sn, 0, 0, 1, as);   // a noisy tip: the observation is predicted
        const double su0 = q.S00 * u0 + q.S01 * u1, su1 = q.S01 * u0 + q.S11 * u1;
        const double C = u0 * su0 + u1 * su1;
        if (V > 0.0) {
          st = 0;
          mv = eu + w;
          vv = V + C;
        } else {
          st = 1;   // the tip's variance is not positive
        }
      }
    }
    const int64_t o = (int64_t)ti * A.row + s;
    if (mean) mean[o] = mv;
    if (var) var[o] = vv;
    if (info) info[o] = st;
  }
}

// ---- joint draws

// (PostUniCond, post_uni_cond and the validity pass post_uni_valid / post_uni_first: pgbp_post_uni_dev.hpp)

// the standard normal of (entry, draw, absolute site): counter (entry, draw, site, 1), the cosine branch of Box-Muller
__device__ __forceinline__ double post_normal(uint32_t entry, uint32_t draw, uint32_t site, uint32_t k0, uint32_t k1) {
#pragma clang fp contract(off)
  uint32_t r[4];
  philox4x32_10(entry, draw, site, 1u, k0, k1, r);
  const double u1 = sim_uniform(r[0], r[1]), u2 = sim_uniform(r[2], r[3]);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// One preorder level: thread = site, the items of the level along grid.y, the nd draws of the launch in a loop.  z (null: the
// generator, draws d0 .. d0 + nd) and x: [nd][size][row] of this chunk; bad[site]: not 0 where the site's draws are NaN
template <bool SM>
__global__ __launch_bounds__(256) void post_uni_apply(SitesArgs A, const SampItem* __restrict__ items, int n_items,
                                                      const int32_t* __restrict__ idx, const int32_t* __restrict__ bad, int d0,
                                                      int nd, int64_t size, const double* __restrict__ z, uint32_t k0, uint32_t k1,
                                                      double* __restrict__ x) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A.n_sites) return;
  const int64_t as = (int64_t)A.site0 + s;
  const bool nan_site = bad[s] != 0;
  for (int q = blockIdx.y; q < n_items; q += gridDim.y) {
    const SampItem it = items[q];
    const int m = it.m, r = it.r;
    const int32_t* __restrict__ perm = idx + it.perm;
    const int32_t* __restrict__ ppos = perm + m;
    const int p0 = perm[0], p1 = m == 2 ? perm[1] : 0;
    PostUniCond c{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, true};
    if (r > 0 && !nan_site) c = post_uni_cond<SM>(A.pool, A.stride, A.off[it.cluster], m, r, p0, as);
    for (int dr = 0; dr < nd; ++dr) {
      const int64_t base = (int64_t)dr * size;
      double* __restrict__ xo = x + (base + it.x_off) * A.row + s;
      const double* __restrict__ xp = x + (base + it.px_off) * A.row + s;
      double v0 = NAN, v1 = NAN;   // the values at perm[0], perm[1]
      if (!nan_site) {
        double z0 = 0.0, z1 = 0.0;
        if (r >= 1) z0 = z ? z[(base + it.x_off + p0) * A.row + s]
                           : post_normal((uint32_t)(it.x_off + p0), (uint32_t)(d0 + dr), (uint32_t)as, k0, k1);
        if (r == 2) z1 = z ? z[(base + it.x_off + p1) * A.row + s]
                           : post_normal((uint32_t)(it.x_off + p1), (uint32_t)(d0 + dr), (uint32_t)as, k0, k1);
        if (r == 2) {
          v0 = c.a0 + (c.T00 * z0 + c.T01 * z1);
          v1 = c.a1 + c.T11 * z1;
        } else if (r == 1) {
          v0 = c.a0 + c.T00 * z0;
          if (m == 2) {
            v1 = xp[(int64_t)ppos[0] * A.row];
            v0 = (c.a0 - c.G * v1) + c.T00 * z0;
          }
        } else {
          v0 = xp[(int64_t)ppos[0] * A.row];
          if (m == 2) v1 = xp[(int64_t)ppos[1] * A.row];
        }
      }
      xo[(int64_t)p0 * A.row] = v0;
      if (m == 2) xo[(int64_t)p1 * A.row] = v1;
    }
  }
}

}  // namespace pgbp

using namespace pgbp;

extern "C" int pgbp_moments_sites(pgbp_engine* e, int32_t n, const int32_t* beliefs, int32_t site_begin, int32_t site_end,
                                  double* mean, double* cov, double* norm, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_moments_sites";
  SitesCall c{};
  int rc = sites_accept(e, fn, "pgbp_moments", site_begin, site_end, (!mean || !norm) ? "no output buffer (mean, norm)" : nullptr, &c);
  if (rc) return rc;
  const Plan& pl = *c.v.plan;
  if (beliefs && n < 0) return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": negative number of beliefs");
  const int nl = beliefs ? n : pl.n_clusters;
  std::vector<PostMomItem> items(nl);
  int32_t nm = 0, nt = 0;
  for (int i = 0; i < nl; ++i) {
    const int32_t b = beliefs ? beliefs[i] : i;
    if (b < 0 || b >= pl.n_beliefs())
      return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": belief index " + std::to_string(b) + " out of range (entry " +
                                                  std::to_string(i) + " of the list)");
    const int m = pl.dims[b];
    items[i] = PostMomItem{b, nm, nt};
    nm += m;
    nt += m * (m + 1) / 2;
  }
  const int ns = c.ns;
  if (ns == 0 || nl == 0) return PGBP_OK;
  const int nb = (nl + kFamUniBlock - 1) / kFamUniBlock;
  const int chunk = fam_uni_chunk(ns, (int64_t)nm + (cov ? nt : 0) + nl + (info ? nl : 0));
  DevBuf<PostMomItem> d_items;
  DevBuf<double> d_mean, d_cov, d_norm;
  DevBuf<int32_t> d_info;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_items, nl);
  S.alloc(d_mean, (size_t)std::max(1, nm) * chunk);
  S.alloc(d_cov, (size_t)std::max(1, nt) * chunk, cov != nullptr);
  S.alloc(d_norm, (size_t)nl * chunk);
  S.alloc(d_info, (size_t)nl * chunk, info != nullptr);
  S.upload(d_items, items.data(), nl);
  if ((rc = S.ready())) return rc;
  for (int s0 = 0; S.ok() && s0 < ns; s0 += chunk) {
    const int nn = std::min(chunk, ns - s0);
    const SitesArgs A = sites_args(c, site_begin + s0, nn, chunk);
    const dim3 grid((nn + 255) / 256, nb);
    PGBP_SITES_LAUNCH(S, c.U.sm, post_uni_moments, grid, A, d_items.get(), nl, d_mean.get(), d_cov.get(), d_norm.get(), d_info.get());
    S.check();
    S.rows(mean, ns, s0, d_mean.get(), chunk, nn, nm);
    S.rows(cov, ns, s0, d_cov.get(), chunk, nn, nt);
    S.rows(norm, ns, s0, d_norm.get(), chunk, nn, nl);
    S.rows(info, ns, s0, d_info.get(), chunk, nn, nl);
  }
  return S.finish();
}

extern "C" int pgbp_lg_impute_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* mean, double* var,
                                    int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_lg_impute_sites";
  SitesCall c{};
  int rc = sites_accept(e, fn, "pgbp_lg_impute", site_begin, site_end,
                          (!mean && !var) ? "no output buffer (mean and var are both NULL)" : nullptr, &c);
  if (rc) return rc;
  if ((rc = lg_refuse_optima(e, fn, c.L))) return rc;
  const LgModel* L = c.L;
  std::vector<int32_t> fams, cls, dyn;
  std::vector<unsigned long long> pred;
  lg_impute_list(*L, fams, pred, &dyn);   // (with the tips the per-site mask hides at some site)
  for (int32_t f : fams) cls.push_back(L->T.cluster[f]);
  const int ns = c.ns, nl = (int)fams.size();
  if (ns == 0 || nl == 0) return PGBP_OK;
  const int nb = (nl + kFamUniBlock - 1) / kFamUniBlock;
  const int chunk = fam_uni_chunk(ns, (int64_t)nl * ((mean ? 1 : 0) + (var ? 1 : 0) + (info ? 1 : 0)));
  DevBuf<int32_t> d_fams, d_cls, d_dyn, d_info;
  DevBuf<unsigned long long> d_pred;
  DevBuf<double> d_mean, d_var;
  const size_t tab = (size_t)nl * chunk;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_fams, nl);
  S.alloc(d_cls, nl);
  S.alloc(d_pred, nl);
  S.alloc(d_dyn, nl);
  S.alloc(d_mean, tab, mean != nullptr);
  S.alloc(d_var, tab, var != nullptr);
  S.alloc(d_info, tab, info != nullptr);
  S.upload(d_fams, fams.data(), nl);
  S.upload(d_cls, cls.data(), nl);
  S.upload(d_pred, pred.data(), nl);
  S.upload(d_dyn, dyn.data(), nl);
  if ((rc = S.ready())) return rc;
  for (int s0 = 0; S.ok() && s0 < ns; s0 += chunk) {
    const int nn = std::min(chunk, ns - s0);
    const SitesArgs A = sites_args(c, site_begin + s0, nn, chunk);
    const dim3 grid((nn + 255) / 256, nb);
    PGBP_SITES_LAUNCH(S, c.U.sm, post_uni_impute, grid, A, L->F, L->M, L->Sh, L->Nz, L->Ms, d_fams.get(), d_cls.get(), d_pred.get(), d_dyn.get(), nl,
                      d_mean.get(), d_var.get(), d_info.get());
    S.check();
    S.rows(mean, ns, s0, d_mean.get(), chunk, nn, nl);
    S.rows(var, ns, s0, d_var.get(), chunk, nn, nl);
    S.rows(info, ns, s0, d_info.get(), chunk, nn, nl);
  }
  return S.finish();
}

// ms (pgbp_sample_posterior_sites_timed): the stream is drained after every phase and the wall time of the phase is added to
// ms[0 .. 3] = {validity pass, copy of z, level launches, copy of x}
static int sample_posterior_sites(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_draws,
                                  const double* z, uint64_t seed, double* x, int32_t* info, double* ms) {
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_sample_posterior_sites";
  SitesCall c{};
  int rc = sites_accept(e, fn, "pgbp_sample_posterior", site_begin, site_end, nullptr, &c);
  if (rc) return rc;
  SampPlan sp;
  rc = sample_plan(e, std::string(fn) + ": ", tree, site_begin, site_end, n_draws, "n_draws", "draw",
                   [&]() { return std::string(!x ? "no output buffer x" : ""); }, sp);
  if (rc) return rc;
  const int ns = c.ns;
  const int64_t size = sp.size;
  if (ns == 0) return PGBP_OK;
  if (size == 0) {
    if (info) std::fill(info, info + ns, 0);
    return PGBP_OK;
  }
  const PostUniPre pre = post_uni_pre(sp);
  // z (when given) and x of a chunk of draws and a chunk of sites: one workgroup's sites at least, so the draws are cut first
  const int64_t per_draw = size * (z ? 2 : 1);
  const int dchunk = (int)std::min<int64_t>(n_draws, std::max<int64_t>(1, g_fam_uni_limit.load() / (256 * per_draw)));
  const int chunk = fam_uni_chunk(ns, per_draw * dchunk + pre.nvb);
  std::vector<int32_t> rank(ns, 0);
  DevBuf<SampItem> d_tab;
  DevBuf<int32_t> d_idx, d_pfirst, d_rank;
  DevBuf<double> d_z, d_x;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_tab, pre.tab.size());
  S.alloc(d_idx, sp.idx.size());
  S.alloc(d_pfirst, (size_t)pre.nvb * chunk);
  S.alloc(d_rank, ns);
  S.alloc(d_z, (size_t)dchunk * size * chunk, z != nullptr);
  S.alloc(d_x, (size_t)dchunk * size * chunk);
  S.upload(d_tab, pre.tab.data(), pre.tab.size());
  S.upload(d_idx, sp.idx.data(), sp.idx.size());
  if ((rc = S.ready())) return rc;
  SitesClock phase(S, ms, 4);
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffull), k1 = (uint32_t)(seed >> 32);
  for (int s0 = 0; S.ok() && s0 < ns; s0 += chunk) {
    const int nn = std::min(chunk, ns - s0);
    const SitesArgs A = sites_args(c, site_begin + s0, nn, chunk);
    post_uni_validity(S, c.U.sm, A, pre, d_tab.get(), d_idx.get(), d_pfirst.get(), d_rank.get(), s0);
    phase(0);
    for (int d0 = 0; S.ok() && d0 < n_draws; d0 += dchunk) {
      const int nd = std::min(dchunk, n_draws - d0);
      const int64_t rows = (int64_t)nd * size;
      if (z)   // rows of the caller's [n_draws][size][ns] into the chunk's [nd][size][chunk]
        S.err = hipMemcpy2DAsync(d_z.get(), sizeof(double) * (size_t)chunk, z + (size_t)d0 * size * ns + s0, sizeof(double) * (size_t)ns,
                                 sizeof(double) * (size_t)nn, (size_t)rows, hipMemcpyHostToDevice, S.st);
      phase(1);
      for (size_t l = 0; l + 1 < sp.level_off.size(); ++l) {
        const int ni = sp.level_off[l + 1] - sp.level_off[l];
        const dim3 grid((nn + 255) / 256, std::min(ni, 65535));
        PGBP_SITES_LAUNCH(S, c.U.sm, post_uni_apply, grid, A, d_tab.get() + sp.level_off[l], ni, d_idx.get(), d_rank.get() + s0, d0,
                          nd, size, d_z.get(), k0, k1, d_x.get());
      }
      S.check();
      phase(2);
      S.rows(x + (size_t)d0 * size * ns, ns, s0, d_x.get(), chunk, nn, rows);
      phase(3);
    }
  }
  S.download(rank.data(), d_rank.get(), ns);
  if ((rc = S.finish())) return rc;
  post_uni_info(pre, rank, info);
  return PGBP_OK;
}

extern "C" int pgbp_sample_posterior_sites(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_draws,
                                           const double* z, uint64_t seed, double* x, int32_t* info) {
  return sample_posterior_sites(e, tree, site_begin, site_end, n_draws, z, seed, x, info, nullptr);
}

extern "C" int pgbp_sample_posterior_sites_timed(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end,
                                                 int32_t n_draws, const double* z, uint64_t seed, double* x, int32_t* info,
                                                 double* ms4) {
  if (e && !ms4) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_sample_posterior_sites_timed: no buffer for the phase times");
  return sample_posterior_sites(e, tree, site_begin, site_end, n_draws, z, seed, x, info, ms4);
}

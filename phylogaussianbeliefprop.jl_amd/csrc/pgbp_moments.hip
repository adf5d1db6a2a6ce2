// Posterior moments of MANY beliefs in one call (pgbp_moments of include/pgbp.h): integratebelief!
// (src/beliefupdates.jl:168-200) with the covariance Sigma = J^-1, over a grid of (belief, site).
//
// Arithmetic contract = integrate_kernel's (pgbp_kernels.hip): the upper triangle is read (PDMat(Symmetric(J))), pivots
// in order, W[i][j] -= (W[i][k] * rd) * W[k][j] with rd the refined reciprocal of the pivot, log det through the
// mantissa / exponent product (renormalised after every sixteenth pivot), sum h~_k^2 rd in pivot order, back substitution
// x_k = h_k / U_kk, h_i -= U_ik x_k.  Every entry sees the same operations in the same order whatever the lane that
// holds it, so mu and norm are bit-identical to pgbp_integrate's in all three classes.
//
// Classes (one launch each):
//   small: at most 16 variables, one belief per ROW OF 16 LANES, four per wavefront, the system [J | h] one row per lane
//          in registers (the frame of bp_level_small4 / the m <= 16 branch of integrate_kernel), no LDS, no barrier;
//   wave : 17 .. 64 variables, one wavefront per belief, the working matrix in LDS (8.4 KB at 32 variables);
//   block: 65 .. kLdsMaxDim variables, a workgroup of 256 threads per belief, the working matrix in up to 133 KB of LDS.
// The inverse is formed IN PLACE from the elimination's factor: J = U~' D U~ (U~ = D^-1 U unit upper triangular), so
// U~ Sigma = D^-1 U~^-T is lower triangular with diagonal D^-1, and row i of Sigma follows from the rows below it:
//   Sigma_ij = -(sum_{l > i} U_il Sigma_lj) / d_i  (j > i),    Sigma_ii = (1 - sum_{l > i} U_il Sigma_li) / d_i,
// i = m - 1 .. 0.  Sigma's lower triangle takes the place of the eliminated entries and the diagonal; the strict upper
// triangle keeps U until its row is done: m x (m + 1) doubles + m reciprocals, where [J | h | I] would need twice that.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pgbp_bs16.hpp"
#include "pgbp_devmem.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"
#include "pgbp_mom_dev.hpp"

namespace pgbp {

#ifndef PGBP_LOG2PI
#define PGBP_LOG2PI 1.8378770664093454835606594728112
#endif

extern __shared__ double mom_lds[];

// one listed belief: where it is and where its outputs go
struct MomItem {
  int32_t belief;
  int32_t slot;      // position in the caller's list (info index)
  int64_t out_off;   // doubles from the start of a site's output
};

// norm = g + (m log 2pi - logdet + h'mu) / 2 with the roundings of integrate_kernel as the compiler builds it: the
// exponent's share of log det is a product of its own, m log 2pi - logdet one fused operation, the halving and g another.
// Contraction is off in this file's arithmetic and every fused operation is written out, so that the bits do not depend on
// what the optimiser finds to fuse in a given context.
__device__ __forceinline__ double mom_norm(double g, int m, double mant, int expo, double quad) {
#pragma clang fp contract(off)
  const double e2 = (double)expo * 0.69314718055994530941723212145818;
  const double logdet = e2 + log(mant);
  const double t = fma((double)m, PGBP_LOG2PI, -logdet);
  return fma(quad + t, 0.5, g);
}

// element (i, j) of the symmetrised precision of a record (either layout)
__device__ __forceinline__ double mom_J(const double* __restrict__ rec, int m, int i, int j, bool packed, int fp) {
  if (packed) return rec[bs16::J_off(m, i, j, fp)];
  return (i <= j) ? rec[i + (int64_t)j * m] : rec[j + (int64_t)i * m];
}

// outputs of a belief without moments: fill = NaN (not positive definite) or Inf (the constant belief: mu only, Sigma NaN)
__device__ __forceinline__ void mom_fill(double* __restrict__ o, int m, bool cov, double mu_fill, double norm, int t, int nt) {
  const int nc = cov ? m * m : 0;
  for (int idx = t; idx < nc; idx += nt) o[idx] = NAN;
  for (int idx = t; idx < m; idx += nt) o[nc + idx] = mu_fill;
  if (t == 0) o[nc + m] = norm;
}

// ---- small class: four beliefs per wavefront, one per row of 16 lanes, in registers
template <bool COV>
__global__ __launch_bounds__(64) void moments_small4(const double* __restrict__ pool, int64_t pool_stride,
                                                     const int64_t* __restrict__ boff, const int32_t* __restrict__ bdim,
                                                     int bs, int fp, const MomItem* __restrict__ items, int n_items,
                                                     int site_begin, int n_sites, int n_list, double* __restrict__ out,
                                                     int64_t out_stride, int32_t* __restrict__ info_out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const int i = lane & 15, r0 = lane & 48;
  const int it = blockIdx.x * 4 + (lane >> 4);
  const bool have = it < n_items;
  MomItem item{0, 0, 0};
  if (have) item = items[it];
  const int m = have ? bdim[item.belief] : 0;
  const bool packed = bs && bs16::applies(m, fp);
  int mmax = m;
#pragma unroll
  for (int o = 32; o >= 16; o >>= 1) mmax = max(mmax, __shfl_xor(mmax, o));
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const double* __restrict__ rec = pool + (int64_t)(site_begin + site) * pool_stride + (have ? boff[item.belief] : 0);
    const bool live = i < m;
    double row[17];
#pragma unroll
    for (int j = 0; j < 16; ++j) row[j] = (live && j < m) ? mom_J(rec, m, i, j, packed, fp) : 0.0;
    row[16] = live ? (packed ? rec[bs16::h_off(m, i, fp)] : rec[(int64_t)m * m + i]) : 0.0;
    bool nzr = live && row[16] != 0.0;
    if (live) {
      if (packed) {
#pragma unroll
        for (int j = 0; j < 16; ++j) nzr |= row[j] != 0.0;
      } else {   // (every stored entry, both triangles: integrate_kernel)
        for (int j = 0; j < m; ++j) nzr |= rec[i + (int64_t)j * m] != 0.0;
      }
    }
    const bool any_nz = ((__ballot(nzr) >> r0) & 0xFFFFull) != 0;
    const double g = have ? (packed ? rec[bs16::g_off(m, fp)] : rec[(int64_t)m * m + m]) : 0.0;
    const int ni = any_nz ? m : 0;
    // elimination: wave-uniform control flow, every row of 16 lanes on its own frame; the updates are predicated
    double mant = 1.0, quad = 0.0;
    int expo = 0, info = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k < mmax) {
        const double d = __shfl(row[k], k, 16);
        const double hk = __shfl(row[16], k, 16);
        const bool act = k < ni && info == 0;
        if (act && !(d > 0.0)) info = k + 1;
        const bool go = act && info == 0;
        const double rd = refined_rcp(d);
        int ex;
        const double fr = frexp(d, &ex);
        if (go) {
          mant *= fr;
          expo += ex;
          quad = fma(rd, hk * hk, quad);
        }
        const double f = row[k] * rd;
#pragma unroll
        for (int j = k + 1; j <= 16; ++j) {
          const double pkj = __shfl(row[j], k, 16);
          const double nv = fma(-f, pkj, row[j]);
          if (go && i > k) row[j] = nv;
        }
      }
    }
    if (m == 16) { int ex; mant = frexp(mant, &ex); expo += ex; }   // (eliminate_leading: after every sixteenth pivot)
    const bool ok = ni > 0 && info == 0;
    const double norm = mom_norm(g, m, ok ? mant : 1.0, expo, quad);
    double S[16];
    if constexpr (COV) {
#pragma unroll
      for (int j = 0; j < 16; ++j) S[j] = 0.0;
#pragma unroll
      for (int ii = 15; ii >= 0; --ii) {
        if (ii < mmax) {
          const bool go = ok && ii < m;
          const double dinv = refined_rcp(__shfl(row[ii], ii, 16));
          double dot = 0.0, dot_d = 0.0;
#pragma unroll
          for (int l = ii + 1; l < 16; ++l) {
            const double u = __shfl(row[l], ii, 16);   // U_il
            dot = fma(u, S[l], dot);                    // lane j: sum_l U_il Sigma_jl
          }
          if (go && i > ii) S[ii] = -(dot * dinv);
#pragma unroll
          for (int l = ii + 1; l < 16; ++l) {
            const double t = __shfl(S[ii], l, 16);     // Sigma_li, to lane i
            if (go && i == ii) S[l] = t;
            dot_d = fma(row[l], t, dot_d);
          }
          if (go && i == ii) S[ii] = fma(-dot_d, dinv, dinv);
        }
      }
    }
    // back substitution on the upper-triangular system left by the elimination
#pragma unroll
    for (int k = 15; k >= 0; --k) {
      if (k < mmax) {
        const double xk = __shfl(row[16] / row[k], k, 16);
        const bool go = ok && k < m;
        const double nv = fma(-row[k], xk, row[16]);
        if (go && i == k) row[16] = xk;
        if (go && i < k) row[16] = nv;
      }
    }
    if (have) {
      double* __restrict__ o = out + (int64_t)site * out_stride + item.out_off;
      const int nc = COV ? m * m : 0;
      if (ok) {
        if constexpr (COV) {
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (live && j < m) o[i + j * m] = S[j];   // (S[j] of lane i = Sigma_ij = Sigma_ji, the same bits)
        }
        if (live) o[nc + i] = row[16];
        if (i == 0) o[nc + m] = norm;
      } else {
        const bool constant = ni == 0;   // J = 0, h = 0: mu = Inf, norm = g (:189-191)
        if constexpr (COV) {
          for (int j = 0; j < m; ++j)
            if (live) o[i + j * m] = NAN;
        }
        if (live) o[nc + i] = constant ? INFINITY : NAN;
        if (i == 0) o[nc + m] = constant ? g : NAN;
      }
      if (i == 0 && info_out) info_out[(int64_t)site * n_list + item.slot] = info;
    }
  }
}


// ---- wave / block class: one workgroup of NT threads per (belief, site), the working matrix in LDS
template <int NT, bool COV>
__global__ __launch_bounds__(NT) void moments_lds(const double* __restrict__ pool, int64_t pool_stride,
                                                  const int64_t* __restrict__ boff, const int32_t* __restrict__ bdim,
                                                  int bs, int fp, const MomItem* __restrict__ items, int site_begin,
                                                  int n_sites, int n_list, double* __restrict__ out, int64_t out_stride,
                                                  int32_t* __restrict__ info_out) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  const MomItem item = items[blockIdx.x];
  const int m = bdim[item.belief];
  const int ld = (m + 1) | 1;
  double* __restrict__ W = mom_lds;
  double* __restrict__ dv = mom_lds + m * ld;   // reciprocals of the pivots
  const bool packed = bs && bs16::applies(m, fp);
  const int nc = COV ? m * m : 0;
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const double* __restrict__ rec = pool + (int64_t)(site_begin + site) * pool_stride + boff[item.belief];
    double* __restrict__ o = out + (int64_t)site * out_stride + item.out_off;
    int32_t* __restrict__ inf = info_out ? info_out + (int64_t)site * n_list + item.slot : nullptr;
    const double g = packed ? rec[bs16::g_off(m, fp)] : rec[(int64_t)m * m + m];
    double mant = 1.0, quad = 0.0;
    int expo = 0;
    const int st = mom_solve<NT, COV>(rec, m, packed, fp, W, dv, t, mant, expo, quad);
    if (st != 0) {   // constant belief: mu = Inf, norm = g (:189-191); not positive definite: NaN
      mom_fill(o, m, COV, st < 0 ? INFINITY : NAN, st < 0 ? g : NAN, t, NT);
      if (t == 0 && inf) *inf = st < 0 ? 0 : st;
      continue;
    }
    for (int i = t; i < m; i += NT) o[nc + i] = W[i * ld + m];
    if (t == 0) {
      o[nc + m] = mom_norm(g, m, mant, expo, quad);
      if (inf) *inf = 0;
    }
    if constexpr (COV) {
      for (int idx = t; idx < m * m; idx += NT) {
        const int j = idx / m, i = idx - j * m;
        o[idx] = (i >= j) ? W[i * ld + j] : W[j * ld + i];
      }
    }
  }
}


// ---- the family sweep of calibrate_exact_cliquetree! (src/calibration.jl:442-499; pgbp_bm_exact_stats) ----------------
// One workgroup per (family, site): the moments of the family's cluster (mom_solve: Sigma never leaves the LDS), then the
// family's diffExp (p), t = sum gamma^2 length and 1 - diffVar / t into the family's slot [d (p) | t | den term]; a family
// the reference skips leaves t = 0.  bm_exact_reduce adds the slots in family order: thread r takes the families r, r + 256,
// ... in order, the 256 partial sums are added by a fixed tree -- no atomics on doubles, the same bytes on every call.
template <int NT>
__global__ __launch_bounds__(NT) void bm_exact_family(const double* __restrict__ pool, int64_t pool_stride,
                                                      const int64_t* __restrict__ boff, const int32_t* __restrict__ bdim,
                                                      int bs, int fp, LgStatic F, const int32_t* __restrict__ fam_cluster,
                                                      int n_fam, int site0, int n_sites, double* __restrict__ slots,
                                                      int32_t* __restrict__ info, int info0) {
#pragma clang fp contract(off)
  const int t = threadIdx.x, f = blockIdx.x;
  const int p = F.p, K = F.K, np = F.n_parents[f];
  const int c = fam_cluster[f], m = bdim[c], ld = (m + 1) | 1;
  const unsigned long long full = p >= 64 ? ~0ull : ((1ull << p) - 1ull);
  const unsigned long long cm = F.child_mask ? F.child_mask[f] : full;
  const unsigned long long pm0 = (np > 0 && F.parent_mask) ? F.parent_mask[(size_t)f * K] : full;
  const int cpos = F.child_pos[f];
  const bool tip = cpos < 0;
  double tt = 0.0;
  for (int k = 0; k < np; ++k) {
    const double gk = F.gamma[(size_t)f * K + k];
    tt = tt + gk * gk * F.length[(size_t)f * K + k];   // (:459)
  }
  // root prior; zero length (:461); nothing in scope at the parent (tip, :469) / the child (:481); a tip without data
  const bool skip = np == 0 || tt == 0.0 || m == 0 || cm == 0 || (tip && pm0 == 0);
  double* __restrict__ W = mom_lds;
  double* __restrict__ dv = mom_lds + m * ld;
  const bool packed = bs && bs16::applies(m, fp);
  const int sl = p + 2;
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    double* __restrict__ o = slots + ((int64_t)site * n_fam + f) * sl;
    if (skip) {
      for (int a = t; a < sl; a += NT) o[a] = 0.0;
      continue;
    }
    const double* __restrict__ rec = pool + (int64_t)(site0 + site) * pool_stride + boff[c];
    double mant, quad;
    int expo;
    const int st = mom_solve<NT, true>(rec, m, packed, fp, W, dv, t, mant, expo, quad);
    if (st != 0) {   // not positive definite (or the constant belief: no moments): the site's sums are NaN
      for (int a = t; a < sl; a += NT) o[a] = NAN;
      if (t == 0 && st > 0) atomicMin(info + info0 + site, c + 1);
      continue;
    }
    if (tip) {
      const int ppos = F.parent_pos[(size_t)f * K];
      const double* __restrict__ y = F.data + ((int64_t)(site0 + site) * F.n_rows + F.data_row[f]) * p;
      for (int a = t; a < p; a += NT) o[a] = W[(ppos + a) * ld + m] - y[a];   // (:475)
      if (t == 0) {
        o[p] = tt;
        o[p + 1] = 1.0 - W[0] / tt;   // vv[1, 1] (:478)
      }
    } else {
      for (int a = t; a < p; a += NT) {
        double d = W[(cpos + a) * ld + m];
        for (int k = 0; k < np; ++k) d = d - F.gamma[(size_t)f * K + k] * W[(F.parent_pos[(size_t)f * K + k] + a) * ld + m];   // (:489)
        o[a] = d;
      }
      if (t == 0) {
        double dvar = W[cpos * ld + cpos];
        for (int k1 = 0; k1 < np; ++k1) {
          const int j1 = F.parent_pos[(size_t)f * K + k1];
          const double g1 = F.gamma[(size_t)f * K + k1];
          dvar = dvar - 2.0 * g1 * (cpos >= j1 ? W[cpos * ld + j1] : W[j1 * ld + cpos]);   // (:490)
          for (int k2 = 0; k2 < np; ++k2) {
            const int j2 = F.parent_pos[(size_t)f * K + k2];
            dvar = dvar + g1 * F.gamma[(size_t)f * K + k2] * (j1 >= j2 ? W[j1 * ld + j2] : W[j2 * ld + j1]);   // (:493)
          }
        }
        o[p] = tt;
        o[p + 1] = 1.0 - dvar / tt;   // (:497)
      }
    }
  }
}

__global__ __launch_bounds__(256) void bm_exact_reduce(const double* __restrict__ slots, int n_fam, int p, int n_sites,
                                                       double* __restrict__ num, double* __restrict__ den, int out0) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int t = threadIdx.x, en = blockIdx.x, sl = p + 2;
  const int a = en % p, b = en / p;   // en == p * p: the denominator
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const double* __restrict__ S = slots + (int64_t)site * n_fam * sl;
    double acc = 0.0;
    for (int f = t; f < n_fam; f += 256) {
      const double* __restrict__ o = S + (int64_t)f * sl;
      if (o[p] != 0.0) acc = acc + (en < p * p ? (o[a] * o[b]) / o[p] : o[p + 1]);   // (:476, :478 / :496, :497)
    }
    __syncthreads();
    part[t] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) part[t] = part[t] + part[t + w];
      __syncthreads();
    }
    if (t == 0) {
      if (en < p * p) num[(int64_t)(out0 + site) * p * p + en] = part[0];
      else den[out0 + site] = part[0];
    }
  }
}

static size_t moments_lds_bytes(int m) { return sizeof(double) * ((size_t)m * ((m + 1) | 1) + (size_t)m); }

template <int NT>
static void launch_moments_lds(bool cov, int n_items, int max_m, int grid_y, const EngineView& v, const MomItem* d_items,
                               int site_begin, int n_sites, int n_list, double* d_out, int64_t out_stride, int32_t* d_info) {
  const size_t bytes = moments_lds_bytes(max_m);
  const Plan& p = *v.plan;
  if (cov) {
    if (bytes > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(moments_lds<NT, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    hipLaunchKernelGGL((moments_lds<NT, true>), dim3(n_items, grid_y), dim3(NT), bytes, v.st, v.pool, p.pool_stride(), v.boff,
                       v.bdim, v.bs16, p.fast_p, d_items, site_begin, n_sites, n_list, d_out, out_stride, d_info);
  } else {
    if (bytes > 64 * 1024)
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(moments_lds<NT, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    hipLaunchKernelGGL((moments_lds<NT, false>), dim3(n_items, grid_y), dim3(NT), bytes, v.st, v.pool, p.pool_stride(), v.boff,
                       v.bdim, v.bs16, p.fast_p, d_items, site_begin, n_sites, n_list, d_out, out_stride, d_info);
  }
}

// the caller's list (NULL: all clusters), checked; false: e's error is set
static bool moments_list(pgbp_engine* e, const Plan& p, int32_t n, const int32_t* beliefs, std::vector<int32_t>& list, int* rc) {
  if (!beliefs) {
    list.resize(p.n_clusters);
    for (int32_t b = 0; b < p.n_clusters; ++b) list[b] = b;
  } else {
    if (n < 0) { *rc = engine_fail(e, PGBP_ERR_INVALID, "pgbp_moments: negative number of beliefs"); return false; }
    list.assign(beliefs, beliefs + n);
  }
  for (size_t i = 0; i < list.size(); ++i) {
    const int32_t b = list[i];
    if (b < 0 || b >= p.n_beliefs()) {
      *rc = engine_fail(e, PGBP_ERR_INVALID, "pgbp_moments: belief index " + std::to_string(b) + " out of range (entry " +
                                                  std::to_string(i) + " of the list)");
      return false;
    }
    if (p.dims[b] > kLdsMaxDim) {
      *rc = engine_fail(e, PGBP_ERR_INVALID, "pgbp_moments: belief " + std::to_string(b) + " has " + std::to_string(p.dims[b]) +
                                                  " variables, more than the " + std::to_string(kLdsMaxDim) +
                                                  " the moments kernels take");
      return false;
    }
  }
  return true;
}

}  // namespace pgbp

using namespace pgbp;

extern "C" int64_t pgbp_moments_size(pgbp_engine* e, int32_t n, const int32_t* beliefs, int32_t want_cov) {
  if (!e) return -1;
  const Plan& p = *engine_plan(e);   // (a function of the plan alone: the engine's state and last error are left as they are)
  if (beliefs && n < 0) return -1;
  const int32_t nl = beliefs ? n : p.n_clusters;
  int64_t at = 0;
  for (int32_t i = 0; i < nl; ++i) {
    const int32_t b = beliefs ? beliefs[i] : i;
    if (b < 0 || b >= p.n_beliefs() || p.dims[b] > kLdsMaxDim) return -1;
    const int64_t m = p.dims[b];
    at += (want_cov ? m * m : 0) + m + 1;
  }
  return at;
}

extern "C" int pgbp_moments(pgbp_engine* e, int32_t n, const int32_t* beliefs, int32_t site_begin, int32_t site_end,
                            int32_t want_cov, double* out, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  EngineView v;
  int rc = engine_view(e, &v);
  if (rc) return rc;
  const Plan& p = *v.plan;
  if (site_begin < 0 || site_end < site_begin || site_end > p.n_sites)
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_moments: site range [" + std::to_string(site_begin) + ", " +
                                                std::to_string(site_end) + ") outside the engine's " + std::to_string(p.n_sites) + " sites");
  std::vector<int32_t> list;
  if (!moments_list(e, p, n, beliefs, list, &rc)) return rc;
  const int nl = (int)list.size(), ns = site_end - site_begin;
  if (nl == 0 || ns == 0) return PGBP_OK;
  if (!out) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_moments: no output buffer");
  // items by class, list order inside a class; outputs in list order
  std::vector<MomItem> items[3];
  int max_m[3] = {0, 0, 0};
  int64_t at = 0;
  for (int i = 0; i < nl; ++i) {
    const int m = p.dims[list[i]];
    const int c = m <= 16 ? 0 : (m <= 64 ? 1 : 2);
    items[c].push_back(MomItem{list[i], i, at});
    max_m[c] = std::max(max_m[c], m);
    at += (int64_t)(want_cov ? m * m : 0) + m + 1;
  }
  const int64_t out_stride = at;
  std::vector<MomItem> all;
  for (int c = 0; c < 3; ++c) all.insert(all.end(), items[c].begin(), items[c].end());
  DevBuf<MomItem> d_items;
  DevBuf<double> d_out;
  DevBuf<int32_t> d_info;
  hipError_t herr = (hipError_t)d_items.alloc(all.size());
  if (herr == hipSuccess) herr = (hipError_t)d_out.alloc((size_t)out_stride * ns);
  if (herr == hipSuccess) herr = (hipError_t)d_info.alloc((size_t)nl * ns);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_items.get(), all.data(), sizeof(MomItem) * all.size(), hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) {
    const int grid_y = std::min(ns, 65535);
    const int n0 = (int)items[0].size(), n1 = (int)items[1].size(), n2 = (int)items[2].size();
    if (n0 > 0) {
      if (want_cov)
        hipLaunchKernelGGL(moments_small4<true>, dim3((n0 + 3) / 4, grid_y), dim3(64), 0, v.st, v.pool, p.pool_stride(), v.boff,
                           v.bdim, v.bs16, p.fast_p, d_items.get(), n0, site_begin, ns, nl, d_out.get(), out_stride, d_info.get());
      else
        hipLaunchKernelGGL(moments_small4<false>, dim3((n0 + 3) / 4, grid_y), dim3(64), 0, v.st, v.pool, p.pool_stride(), v.boff,
                           v.bdim, v.bs16, p.fast_p, d_items.get(), n0, site_begin, ns, nl, d_out.get(), out_stride, d_info.get());
    }
    if (n1 > 0) launch_moments_lds<64>(want_cov != 0, n1, max_m[1], grid_y, v, d_items.get() + n0, site_begin, ns, nl, d_out.get(), out_stride, d_info.get());
    if (n2 > 0) launch_moments_lds<256>(want_cov != 0, n2, max_m[2], grid_y, v, d_items.get() + n0 + n1, site_begin, ns, nl, d_out.get(), out_stride, d_info.get());
    herr = hipGetLastError();
  }
  if (herr == hipSuccess) herr = hipMemcpyAsync(out, d_out.get(), sizeof(double) * (size_t)out_stride * ns, hipMemcpyDeviceToHost, v.st);
  if (herr == hipSuccess && info) herr = hipMemcpyAsync(info, d_info.get(), sizeof(int32_t) * (size_t)nl * ns, hipMemcpyDeviceToHost, v.st);
  const hipError_t serr = hipStreamSynchronize(v.st);   // (also when something failed: `all` is a local the upload reads)
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_moments: ") + hipGetErrorString(herr));
  return PGBP_OK;
}

extern "C" int pgbp_bm_exact_stats(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* num, double* den, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const LgModel* L = engine_lg(e);
  if (!L) return engine_fail(e, PGBP_ERR_STATE, "pgbp_bm_exact_stats: no family table (call pgbp_lg_setup first)");
  if (site_begin < 0 || site_end < site_begin || site_end > engine_n_sites(e))
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_bm_exact_stats: site range outside the engine's sites");
  if (!num || !den) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_bm_exact_stats: no output buffer");
  if (L->Ms.words)
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_bm_exact_stats: a per-site mask of missing tips is in force (pgbp_lg_set_site_missing), "
                                            "which this sweep cannot honour (use pgbp_lg_gradient_sites: fit_sites_lg)");
  EngineView v;
  int rc = engine_view(e, &v);
  if (rc) return rc;
  const Plan& pl = *v.plan;
  const LgStatic& F = L->F;
  const int p = F.p, K = F.K;
  // the host table for the checks of src/calibration.jl:416-421 and of this sweep; the size of a family's cluster is checked
  // below, family by family, behind the reference's own checks
  const LgTable& T = L->T;
  const std::vector<int32_t> &fcl = T.cluster, &npar = T.n_parents, &cpos = T.child_pos, &ppos = T.parent_pos;
  const std::vector<unsigned long long> &cmask = T.child_mask, &pmask = T.parent_mask;
  const int nf = T.n_families;
  hipError_t herr = hipSuccess;
  const unsigned long long full = p >= 64 ? ~0ull : ((1ull << p) - 1ull);
  int max_m = 1;
  for (int f = 0; f < nf; ++f) {
    const std::string where = "pgbp_bm_exact_stats: family " + std::to_string(f) + " (cluster " + std::to_string(fcl[f]) + "): ";
    const unsigned long long cm = cmask.empty() ? full : cmask[f];
    if (cm != 0 && cm != full)
      return engine_fail(e, PGBP_ERR_INVALID, "some leaf must have partial data: cluster " + std::to_string(fcl[f]) +
                                                  " has partial traits in scope");
    for (int k = 0; k < npar[f]; ++k) {
      const unsigned long long pm = pmask.empty() ? full : pmask[(size_t)f * K + k];
      if (pm != 0 && pm != full)
        return engine_fail(e, PGBP_ERR_INVALID, "some leaf must have partial data: cluster " + std::to_string(fcl[f]) +
                                                    " has partial traits in scope");
      if (ppos[(size_t)f * K + k] < 0 && pm != 0)   // (-1 with an empty mask: a parent with nothing in scope)
        return engine_fail(e, PGBP_ERR_INVALID, where + "its parent is the fixed root: the sweep is defined on the engine with "
                                                        "an improper root prior (fixedroot = false)");
    }
    if (npar[f] == 0) continue;
    if (cpos[f] < 0 && cm != 0 && (pmask.empty() || pmask[(size_t)f * K] != 0)) {
      // a tip: the reference reads vv[1, 1], the cluster's first variable (:478) -- in a clique tree the parent's first trait
      if (npar[f] != 1) return engine_fail(e, PGBP_ERR_INVALID, where + "a leaf with more than one parent");
      if (ppos[(size_t)f * K] != 0)
        return engine_fail(e, PGBP_ERR_INVALID, where + "the tip's parent is not the first variable of the cluster (vv[1, 1] of "
                                                        "src/calibration.jl:478 is then not the parent's variance)");
    }
    if (pl.dims[fcl[f]] > kLdsMaxDim)
      return engine_fail(e, PGBP_ERR_INVALID, where + "the cluster has more than " + std::to_string(kLdsMaxDim) + " variables");
    max_m = std::max(max_m, (int)pl.dims[fcl[f]]);
  }
  const int ns = site_end - site_begin;
  if (ns == 0) return PGBP_OK;
  if (nf == 0) {
    std::fill(num, num + (size_t)ns * p * p, 0.0);
    std::fill(den, den + ns, 0.0);
    if (info) std::fill(info, info + ns, 0);
    return PGBP_OK;
  }
  // slots of a chunk of sites at a time (256 MB at most: cfg4's 8 000 sites x 40 000 families would be 7.7 GB at once)
  const int64_t per_site = (int64_t)nf * (p + 2);
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(ns, ((int64_t)32 << 20) / per_site));
  std::vector<int32_t> inf(ns, 0x7fffffff);   // (ahead of the buffers: they are released, which drains the uploads, first)
  DevBuf<int32_t> d_fcl, d_info;
  DevBuf<double> d_slots, d_num, d_den;
  herr = (hipError_t)d_fcl.alloc(nf);
  if (herr == hipSuccess) herr = (hipError_t)d_slots.alloc((size_t)per_site * chunk);
  if (herr == hipSuccess) herr = (hipError_t)d_num.alloc((size_t)ns * p * p);
  if (herr == hipSuccess) herr = (hipError_t)d_den.alloc((size_t)ns);
  if (herr == hipSuccess) herr = (hipError_t)d_info.alloc((size_t)ns);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_fcl.get(), fcl.data(), sizeof(int32_t) * nf, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_info.get(), inf.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) {
    const size_t bytes = moments_lds_bytes(max_m);
    const void* kern = max_m <= 64 ? reinterpret_cast<const void*>(bm_exact_family<64>) : reinterpret_cast<const void*>(bm_exact_family<256>);
    if (bytes > 64 * 1024) (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    for (int s0 = 0; s0 < ns; s0 += chunk) {
      const int n = std::min(chunk, ns - s0), gy = std::min(n, 65535);
      if (max_m <= 64)
        hipLaunchKernelGGL(bm_exact_family<64>, dim3(nf, gy), dim3(64), bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, d_fcl.get(), nf, site_begin + s0, n, d_slots.get(), d_info.get(), s0);
      else
        hipLaunchKernelGGL(bm_exact_family<256>, dim3(nf, gy), dim3(256), bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, d_fcl.get(), nf, site_begin + s0, n, d_slots.get(), d_info.get(), s0);
      hipLaunchKernelGGL(bm_exact_reduce, dim3(p * p + 1, gy), dim3(256), 0, v.st, d_slots.get(), nf, p, n, d_num.get(), d_den.get(), s0);
    }
    herr = hipGetLastError();
  }
  if (herr == hipSuccess) herr = hipMemcpyAsync(num, d_num.get(), sizeof(double) * (size_t)ns * p * p, hipMemcpyDeviceToHost, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(den, d_den.get(), sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(inf.data(), d_info.get(), sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, v.st);
  const hipError_t serr = hipStreamSynchronize(v.st);
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_bm_exact_stats: ") + hipGetErrorString(herr));
  if (info)
    for (int s2 = 0; s2 < ns; ++s2) info[s2] = inf[s2] == 0x7fffffff ? 0 : inf[s2];
  return PGBP_OK;
}

// Leave-one-out predictive moments of every tip from calibrated beliefs (pgbp_lg_loo of include/pgbp.h).
//
// A tip's data enters the model through one factor, N(y_O; u + w, V) in the notation of pgbp_lgfill.hip / pgbp_grad.hip
// (coefficients, block table, Cov(u), the Cholesky and the staging of a packed record: pgbp_fam_dev.hpp):
// u = (sum_k qc_k x_k)_O the parents' contribution (a fixed-root parent: its constant), w = (sum_k wc_k theta)_O,
// V = (sum_k vc_k R[colour_k])_OO, O = child_mask[f] the observed traits, o = |O|.  With m_u = E[u], S = Cov(u) under the
// calibrated belief of the family's cluster and r = y_O - w - m_u, dividing the factor out of the belief leaves the cavity
// distribution of u, and integrating the factor against it gives the predictive distribution of y_O given all OTHER data:
//   D = V - S,   P = V D^-1 V (covariance),   d = V D^-1 r = y_O - mean,
//   lpd = -(o log 2pi + 2 log det V - log det D + r' D^-1 r) / 2          (d' P^-1 d = r' D^-1 r).
// D is positive definite unless the other data leave u undetermined.
// With tip noise set (pgbp_lg_set_tip_noise) the tip's variable is the OBSERVATION y = x + eps: V is V + E_OO for a noisy tip,
// here as in the factor, and the moments are those of the predicted observation.
//
// Stage 1 (loo_family): one workgroup per (tip family, site) solves the family's cluster in LDS (mom_solve: Sigma never leaves
// the LDS), forms V, D = V - S and the right-hand sides [V | r], factorises D = L L' (left-looking Cholesky, the lower
// triangle), Y = L^-1 [V | r] (a thread per column), factorises V for its determinant, and writes mean = y - Y'z,
// P = Y'Y (upper triangle computed, mirrored), lpd and info.  Every sum in index order, no atomics.
// Stage 2 (loo_reduce): the site's total = sum of lpd in tip-family order: thread r adds the tips r, r + 256, ... in order, the
// 256 partial sums are added by a fixed tree (the scheme of bm_exact_reduce): two calls return the same bytes.
// The outputs of a chunk of sites at a time (256 MB at most: pgbp_loo_scratch_limit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <vector>

#include "pgbp_bs16.hpp"
#include "pgbp_devmem.hpp"
#include "pgbp_fam_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"

namespace pgbp {

extern __shared__ double loo_lds[];

#define PGBP_LOO_LOG2PI 1.8378770664093454835606594728112

// LDS of loo_family beyond mom_solve's: doubles, then ints
__host__ __device__ inline size_t loo_extra_doubles(int p, int K) {
  return 3 * (size_t)p * p + 4 * (size_t)p + 3 * (size_t)K + (size_t)K * p;
}
__host__ __device__ inline size_t loo_extra_ints(int p, int K) { return (size_t)K + (size_t)p + (size_t)K * p; }

// tip_fam[ti]: the family of tip ti, tip_cluster[ti]: its cluster.  Outputs of the chunk: mean [n_sites][n_tip][p] and
// cov [n_sites][n_tip][p*p] (either may be null), lpd and info [n_sites][n_tip].
template <int NT>
__global__ __launch_bounds__(NT) void loo_family(const double* __restrict__ pool, int64_t pool_stride,
                                                 const int64_t* __restrict__ boff, const int32_t* __restrict__ bdim, int bs,
                                                 int fp, LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz,
                                                 const int32_t* __restrict__ tip_fam,
                                                 const int32_t* __restrict__ tip_cluster, int n_tip, int site0, int n_sites,
                                                 double* __restrict__ mean, double* __restrict__ cov,
                                                 double* __restrict__ lpd, int32_t* __restrict__ info) {
#pragma clang fp contract(off)
  const int t = threadIdx.x, ti = blockIdx.x;
  const int f = tip_fam[ti];
  const int p = F.p, K = F.K, np = F.n_parents[f], nr = F.n_rates;
  const int c = tip_cluster[ti], m = bdim[c], ld = (m + 1) | 1;
  const unsigned long long full = p >= 64 ? ~0ull : ((1ull << p) - 1ull);
  const unsigned long long O = F.child_mask ? (F.child_mask[f] & full) : full;
  const int mo = __popcll(O), ldy = mo + 1;
  const int row = F.data_row[f];
  const int sn = lg_noise_slot(Nz, f);
  // LDS: [W | dv] of mom_solve, then this kernel's arrays
  double* __restrict__ W = loo_lds;
  double* __restrict__ dv = loo_lds + m * ld;
  double* __restrict__ Vm = loo_lds + mom_lds_doubles(m);   // V_OO (mo x mo), then its factor below the diagonal
  double* __restrict__ Dm = Vm + p * p;                     // D = V - S, then its factor L below the diagonal
  double* __restrict__ Ym = Dm + p * p;                     // [V | r] -> L^-1 [V | r]   (mo x (mo + 1))
  double* __restrict__ dlD = Ym + p * p + p;                // diagonal of D's factor
  double* __restrict__ dlV = dlD + p;                       // diagonal of V's factor
  double* __restrict__ yv = dlV + p;                        // y_O
  double* __restrict__ cf = yv + p;                         // rows of K: qc, vc, wc
  double* __restrict__ xm = cf + 3 * K;                     // [k][i]: posterior mean of parent k (or its constant) at kept trait i
  int* __restrict__ ipos = reinterpret_cast<int*>(loo_lds + mom_lds_doubles(m) + ((loo_extra_doubles(p, K) + 1) & ~(size_t)1));
  int* __restrict__ oidx = ipos + K;
  int* __restrict__ vi = oidx + p;                          // [k][i]: the variable's index in the cluster, -1: a constant
  // a packed (BS16) record is first copied here in the plain layout (fam_stage_plain)
  double* __restrict__ stage = loo_lds + mom_lds_doubles(m) + ((loo_extra_doubles(p, K) + 1) & ~(size_t)1) +
                               ((loo_extra_ints(p, K) + 1) >> 1);
  bool any_scope = false;
  for (int k = 0; k < np; ++k) any_scope |= F.parent_pos[(size_t)f * K + k] >= 0;
  const bool packed = bs && bs16::applies(m, fp);
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const int64_t slot = (int64_t)site * n_tip + ti;
    double* __restrict__ om = mean ? mean + slot * p : nullptr;
    double* __restrict__ oc = cov ? cov + slot * p * p : nullptr;
    const int64_t as = site0 + site;
    const LgSite S = lg_site(M, nr, p, as);
    int st = 0;
    if (any_scope) {
      const double* __restrict__ rec = pool + as * pool_stride + boff[c];
      double mant, quad;
      int expo;
      if (packed) {
        fam_stage_plain<NT>(rec, m, fp, stage, t);
        rec = stage;
      }
      st = mom_solve<NT, true>(rec, m, false, fp, W, dv, t, mant, expo, quad);
    } else {
      __syncthreads();   // (the previous site's arrays have been read)
    }
    if (st != 0) {   // the cluster is not positive definite; the constant belief (J = 0): u is undetermined, as D singular
      if (om) for (int a = t; a < p; a += NT) om[a] = NAN;
      if (oc) for (int a = t; a < p * p; a += NT) oc[a] = NAN;
      if (t == 0) {
        lpd[slot] = NAN;
        info[slot] = st > 0 ? 1 + st : 1;
      }
      continue;
    }
    // coefficients, positions, kept traits
    for (int k = t; k < np; k += NT) {
      lg_coefs<false>(M.model, S.alpha, F.length[(size_t)f * K + k], F.gamma[(size_t)f * K + k], cf[k], cf[K + k], cf[2 * K + k]);
      ipos[k] = F.parent_pos[(size_t)f * K + k];
    }
    for (int tr = t; tr < p; tr += NT)
      if ((O >> tr) & 1ull) oidx[mask_rank(O, tr)] = tr;
    __syncthreads();
    // where each parent's kept traits sit in the cluster, and their posterior mean (or the fixed root's constant)
    fam_blocks<NT>(F, f, as, S.mu, 0, np, O, ipos, oidx, mo, W, ld, m, vi, xm, t);
    for (int i = t; i < mo; i += NT) yv[i] = F.data[(as * F.n_rows + row) * p + oidx[i]];
    // V_OO, twice: the matrix to factorise and the right-hand sides
    for (int idx = t; idx < mo * mo; idx += NT) {
      const int i = idx / mo, j = idx - i * mo;
      const int e = oidx[i] + oidx[j] * p;
      double v = 0.0;
      for (int k = 0; k < np; ++k) v = v + cf[K + k] * S.R[(int64_t)F.color[(size_t)f * K + k] * p * p + e];
      if (sn >= 0) v = v + lg_noise_E(Nz, sn, oidx[i], oidx[j], p, as);   // a noisy tip: the observation's variance V + E
      Vm[i * mo + j] = v;
      Ym[i * ldy + j] = v;
    }
    __syncthreads();
    // r = y_O - w - m_u, the last right-hand side
    for (int i = t; i < mo; i += NT) {
      double mu_u = 0.0;
      for (int k = 0; k < np; ++k) mu_u = mu_u + cf[k] * xm[k * p + i];
      double w = 0.0;
      if (S.theta)
        for (int k = 0; k < np; ++k) w = w + cf[2 * K + k] * S.theta[oidx[i]];
      if (Sh.slot) w = w + lg_shift_d(Sh, F.gamma, f, K, np, oidx[i], p, as);   // a shift of the mean on a parent edge
      Ym[i * ldy + mo] = (yv[i] - w) - mu_u;
    }
    // D = V - S, S = Cov(u): the lower triangle
    for (int idx = t; idx < mo * mo; idx += NT) {
      const int i = idx / mo, j = idx - i * mo;
      if (j > i) continue;
      Dm[i * mo + j] = Vm[i * mo + j] - fam_cov(W, ld, vi, p, [&](int k) -> double { return cf[k]; }, np, i, j);
    }
    __syncthreads();
    bool ok = lds_cholesky<NT>(Dm, mo, mo, dlD, Vm, t);
    if (ok) {
      // Y = L^-1 [V | r]: thread j its own column, rows in order
      for (int j = t; j <= mo; j += NT)
        for (int i = 0; i < mo; ++i) {
          double s = Ym[i * ldy + j];
          for (int k = 0; k < i; ++k) s = fma(-Dm[i * mo + k], Ym[k * ldy + j], s);
          Ym[i * ldy + j] = s / dlD[i];
        }
      ok = lds_cholesky<NT>(Vm, mo, mo, dlV, nullptr, t);   // (its first barrier publishes Y)
    }
    if (!ok) {   // D or V is not positive definite
      if (om) for (int a = t; a < p; a += NT) om[a] = NAN;
      if (oc) for (int a = t; a < p * p; a += NT) oc[a] = NAN;
      if (t == 0) {
        lpd[slot] = NAN;
        info[slot] = 1;
      }
      continue;
    }
    // NaN at the unobserved traits (every entry is written by exactly one thread)
    if (om)
      for (int a = t; a < p; a += NT)
        if (!((O >> a) & 1ull)) om[a] = NAN;
    if (oc)
      for (int a = t; a < p * p; a += NT) {
        const int ja = a / p, ia = a - ja * p;
        if (!((O >> ia) & 1ull) || !((O >> ja) & 1ull)) oc[a] = NAN;
      }
    if (om)
      for (int i = t; i < mo; i += NT) {
        double d = 0.0;
        for (int l = 0; l < mo; ++l) d = fma(Ym[l * ldy + i], Ym[l * ldy + mo], d);
        om[oidx[i]] = yv[i] - d;
      }
    if (oc)
      for (int idx = t; idx < mo * mo; idx += NT) {
        const int i = idx / mo, j = idx - i * mo;
        if (i > j) continue;
        double s = 0.0;
        for (int l = 0; l < mo; ++l) s = fma(Ym[l * ldy + i], Ym[l * ldy + j], s);
        oc[oidx[i] + oidx[j] * p] = s;
        oc[oidx[j] + oidx[i] * p] = s;
      }
    if (t == 0) {
      double quad = 0.0, ldD = 0.0, ldV = 0.0;
      for (int l = 0; l < mo; ++l) {
        quad = fma(Ym[l * ldy + mo], Ym[l * ldy + mo], quad);
        ldD = ldD + log(dlD[l]);
        ldV = ldV + log(dlV[l]);
      }
      // log det = 2 sum log(diagonal of the factor)
      lpd[slot] = -0.5 * ((((double)mo * PGBP_LOO_LOG2PI + 4.0 * ldV) - 2.0 * ldD) + quad);
      info[slot] = 0;
    }
  }
}

__global__ __launch_bounds__(256) void loo_reduce(const double* __restrict__ lpd, int n_tip, int n_sites,
                                                  double* __restrict__ total, int out0) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int t = threadIdx.x;
  for (int site = blockIdx.x; site < n_sites; site += gridDim.x) {
    const double* __restrict__ S = lpd + (int64_t)site * n_tip;
    double acc = 0.0;
    for (int f = t; f < n_tip; f += 256) acc = acc + S[f];
    __syncthreads();
    part[t] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) part[t] = part[t] + part[t + w];
      __syncthreads();
    }
    if (t == 0) total[out0 + site] = part[0];
  }
}

// bound of the call's device outputs, in doubles: those of a chunk of sites (pgbp_loo_scratch_limit)
static std::atomic<int64_t> g_loo_limit{(int64_t)32 << 20};

}  // namespace pgbp

using namespace pgbp;

// the count and the list are the host table's, whatever the clusters' sizes (the sweep is not served above 128 variables)
extern "C" int32_t pgbp_lg_loo_count(pgbp_engine* e) {
  if (!e) return -1;
  const LgModel* L = engine_lg(e);
  if (!L) return engine_fail(e, PGBP_ERR_STATE, "pgbp_lg_loo_count: no family table (call pgbp_lg_setup first)"), -1;
  return (int32_t)L->T.loo_tips().size();
}

extern "C" int pgbp_lg_loo_families(pgbp_engine* e, int32_t* fam) {
  if (!e) return PGBP_ERR_INVALID;
  const LgModel* L = engine_lg(e);
  if (!L) return engine_fail(e, PGBP_ERR_STATE, "pgbp_lg_loo_families: no family table (call pgbp_lg_setup first)");
  const std::vector<int32_t> tips = L->T.loo_tips();
  if (!fam && !tips.empty()) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_loo_families: no output buffer");
  std::copy(tips.begin(), tips.end(), fam);
  return PGBP_OK;
}

extern "C" void pgbp_loo_scratch_limit(int64_t doubles) { g_loo_limit.store(doubles > 0 ? doubles : (int64_t)32 << 20); }

extern "C" int pgbp_lg_loo(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* mean, double* cov, double* lpd,
                           double* total, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const LgModel* L = nullptr;
  int rc = lg_sweep_state(e, "pgbp_lg_loo", site_begin, site_end, &L, "pgbp_lg_loo_sites");
  if (rc) return rc;
  if ((rc = lg_refuse_optima(e, "pgbp_lg_loo", L))) return rc;
  const LgStatic& F = L->F;
  const LgParams& M = L->M;
  const LgShifts& Sh = L->Sh;
  const LgNoise& Nz = L->Nz;
  if (!lpd) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_loo: no output buffer (lpd)");
  EngineView v;
  if ((rc = engine_view(e, &v))) return rc;
  // the limits are pgbp_lg_gradient's, over the clusters of ALL families of the table: an engine either serves both sweeps
  // or neither, and the dimension class of the launch is the gradient's
  int max_m = 0;
  std::string why;
  if (!L->T.cluster_dims("pgbp_lg_loo", kLdsMaxDim, &max_m, why)) return engine_fail(e, PGBP_ERR_INVALID, why);
  const std::vector<int32_t> tips = L->T.loo_tips();   // the tip families, in table order, and the cluster of each
  std::vector<int32_t> tcl;
  for (int32_t f : tips) tcl.push_back(L->T.cluster[f]);
  // (as in pgbp_lg_gradient, what follows runs on the caller's current device)
  const Plan& pl = *v.plan;
  const int p = F.p, K = F.K, nt = (int)tips.size();
  size_t stage = 0;   // a packed record's plain copy
  for (int i = 0; i < nt && v.bs16; ++i) {
    const size_t m = (size_t)pl.dims[tcl[i]];
    if (bs16::applies((int)m, pl.fast_p)) stage = std::max(stage, m * m + m);
  }
  const size_t lds_bytes = sizeof(double) * (mom_lds_doubles(max_m) + ((loo_extra_doubles(p, K) + 1) & ~(size_t)1) +
                                             ((loo_extra_ints(p, K) + 1) >> 1) + stage);
  if (lds_bytes > 160 * 1024)
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_loo: a cluster of " + std::to_string(max_m) + " variables with " +
                                                std::to_string(p) + " traits needs " + std::to_string(lds_bytes) +
                                                " bytes of LDS, more than the 160 KB of a compute unit");
  const int ns = site_end - site_begin;
  if (ns == 0) return PGBP_OK;
  if (nt == 0) {
    if (total)
      for (int s = 0; s < ns; ++s) total[s] = 0.0;
    return PGBP_OK;
  }
  const int pp = p * p;
  const int64_t per_site = (int64_t)nt * (1 + (mean ? p : 0) + (cov ? pp : 0));
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(ns, g_loo_limit.load() / per_site));
  DevBuf<int32_t> d_tips, d_tcl, d_info;
  DevBuf<double> d_mean, d_cov, d_lpd, d_total;
  const size_t cn = (size_t)chunk * nt;
  hipError_t herr = (hipError_t)d_tips.alloc(nt);
  if (herr == hipSuccess) herr = (hipError_t)d_tcl.alloc(nt);
  if (herr == hipSuccess) herr = (hipError_t)d_info.alloc(cn);
  if (herr == hipSuccess && mean) herr = (hipError_t)d_mean.alloc(cn * p);
  if (herr == hipSuccess && cov) herr = (hipError_t)d_cov.alloc(cn * pp);
  if (herr == hipSuccess) herr = (hipError_t)d_lpd.alloc(cn);
  if (herr == hipSuccess) herr = (hipError_t)d_total.alloc((size_t)ns);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_tips.get(), tips.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_tcl.get(), tcl.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice, v.st);
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_loo (scratch): ") + hipGetErrorString(herr));
  (void)hipGetLastError();   // (an error an earlier asynchronous call left behind is that call's to report)
  {
    const void* kern = max_m <= 64 ? reinterpret_cast<const void*>(loo_family<64>) : reinterpret_cast<const void*>(loo_family<256>);
    if (lds_bytes > 64 * 1024) herr = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    for (int s0 = 0; herr == hipSuccess && s0 < ns; s0 += chunk) {
      const int n = std::min(chunk, ns - s0), gy = std::min(n, 65535);
      if (max_m <= 64)
        hipLaunchKernelGGL(loo_family<64>, dim3(nt, gy), dim3(64), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, Nz, d_tips.get(), d_tcl.get(), nt, site_begin + s0, n, d_mean.get(), d_cov.get(), d_lpd.get(), d_info.get());
      else
        hipLaunchKernelGGL(loo_family<256>, dim3(nt, gy), dim3(256), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, Nz, d_tips.get(), d_tcl.get(), nt, site_begin + s0, n, d_mean.get(), d_cov.get(), d_lpd.get(), d_info.get());
      hipLaunchKernelGGL(loo_reduce, dim3(gy), dim3(256), 0, v.st, d_lpd.get(), nt, n, d_total.get(), s0);
      herr = hipGetLastError();
      const size_t o = (size_t)s0 * nt, len = (size_t)n * nt;
      if (herr == hipSuccess) herr = hipMemcpyAsync(lpd + o, d_lpd.get(), sizeof(double) * len, hipMemcpyDeviceToHost, v.st);
      if (herr == hipSuccess && mean) herr = hipMemcpyAsync(mean + o * p, d_mean.get(), sizeof(double) * len * p, hipMemcpyDeviceToHost, v.st);
      if (herr == hipSuccess && cov) herr = hipMemcpyAsync(cov + o * pp, d_cov.get(), sizeof(double) * len * pp, hipMemcpyDeviceToHost, v.st);
      if (herr == hipSuccess && info) herr = hipMemcpyAsync(info + o, d_info.get(), sizeof(int32_t) * len, hipMemcpyDeviceToHost, v.st);
    }
  }
  if (herr == hipSuccess && total) herr = hipMemcpyAsync(total, d_total.get(), sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost, v.st);
  const hipError_t serr = hipStreamSynchronize(v.st);
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_loo: ") + hipGetErrorString(herr));
  return PGBP_OK;
}

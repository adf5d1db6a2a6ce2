// Posterior moments of the MISSING values of every tip from calibrated beliefs (pgbp_lg_impute of include/pgbp.h): the
// complement of pgbp_loo.hip -- there a tip's own data is divided out of its cluster's belief, here nothing is left out.
//
// A tip's factor is N(x; u + w, V) in the notation of pgbp_lgfill.hip / pgbp_loo.hip (coefficients, block table, Cov(u_Z), the
// Cholesky and the staging of a packed record: pgbp_fam_dev.hpp): u = sum_k qc_k x_k the parents'
// contribution (a fixed-root parent: its constant qc_k mu), w = sum_k wc_k theta, V = sum_k vc_k R[colour_k] (p x p).  With
// O = child_mask[f] the observed traits, M its complement, the PREDICTED traits are P = M intersected with the scope of every
// cluster parent (a missing trait a parent does not hold is in no belief of the graph: NaN), Z = O u P.  Given the parents the
// tip's noise eps = x - u - w is independent of every other datum, eps_O is pinned by y_O and eps_P | eps_O is the Gaussian
// conditional, so with m = J^-1 h and S = J^-1 of the family's calibrated cluster (which holds the tip's own data already):
//   B    = V_PO V_OO^-1                                   (empty when O is empty)
//   mean = E[u_P] + w_P + B (y_O - w_O - E[u_O])
//   cov  = [-B  I] Cov(u_Z) [-B  I]' + V_PP - B V_OP
//   E[u_T] = sum_k qc_k m[idx_k(T)] (+ qc_k mu_T of a fixed-root parent),  Cov(u_A, u_B) = sum_{a, b} qc_a qc_b S[idx_a(A), idx_b(B)]
// over the cluster parents, idx_k(t) = parent_pos + popcount(parent_mask below t).
// With tip noise set (pgbp_lg_set_tip_noise) V is V + E for a noisy tip at all of Z (the blocks E_PP and E_PO as well as E_OO):
// the moments are those of the missing entries of the OBSERVATION y = x + eps, not of the trait value under it.
//
// impute_family: one workgroup per (listed family, site) solves the family's cluster in LDS (mom_solve: Sigma never leaves the
// LDS; skipped when no parent is in a cluster: a star tree under a fixed root), forms V_ZZ (Z ordered O first, then P),
// Cov(u_Z) and E[u_Z], factorises V_OO = L L' (left-looking Cholesky, the lower triangle), Y = L^-1 V_OP (a thread per column),
// C = V_PP - Y'Y (factorised once more, on a copy: it must be positive definite), B' = L^-T Y in place, G = [-B I] Cov(u_Z),
// and writes mean and cov = C + G [-B I]' (the lower triangle computed, mirrored) and info.  Every sum in index order, no
// atomics, no reduction: two calls return the same bytes.  The outputs of a chunk of sites at a time
// (pgbp_impute_scratch_limit).
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

extern __shared__ double imp_lds[];

// LDS of impute_family beyond mom_solve's: doubles (five p x p blocks: V_ZZ, Cov(u_Z), Y / B', C, the copy of C / G; six
// p-vectors; qc, vc, wc; the parents' means), then ints
__host__ __device__ inline size_t impute_extra_doubles(int p, int K) {
  return 5 * (size_t)p * p + 6 * (size_t)p + 3 * (size_t)K + (size_t)K * p;
}
__host__ __device__ inline size_t impute_extra_ints(int p, int K) { return (size_t)K + (size_t)p + (size_t)K * p; }
// the whole need, in doubles: mom_solve's matrix for the largest cluster, the blocks above, the plain copy of a packed record
__host__ __device__ inline size_t impute_lds_doubles(int max_m, int p, int K, size_t stage) {
  return mom_lds_doubles(max_m) + ((impute_extra_doubles(p, K) + 1) & ~(size_t)1) + ((impute_extra_ints(p, K) + 1) >> 1) + stage;
}

// fam[ti]: the listed family ti, fcl[ti]: its cluster, pred[ti]: its mask P.  Outputs of the chunk: mean [n_sites][n_fam][p]
// and cov [n_sites][n_fam][p*p] (either may be null), info [n_sites][n_fam].
template <int NT>
__global__ __launch_bounds__(NT) void impute_family(const double* __restrict__ pool, int64_t pool_stride,
                                                    const int64_t* __restrict__ boff, const int32_t* __restrict__ bdim, int bs,
                                                    int fp, LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz,
                                                    const int32_t* __restrict__ fam,
                                                    const int32_t* __restrict__ fcl, const unsigned long long* __restrict__ pred,
                                                    int n_fam, int site0, int n_sites, double* __restrict__ mean,
                                                    double* __restrict__ cov, int32_t* __restrict__ info) {
#pragma clang fp contract(off)
  const int t = threadIdx.x, ti = blockIdx.x;
  const int f = fam[ti];
  const int p = F.p, K = F.K, np = F.n_parents[f], nr = F.n_rates;
  const int c = fcl[ti], m = bdim[c], ld = (m + 1) | 1;
  const unsigned long long full = p >= 64 ? ~0ull : ((1ull << p) - 1ull);
  const unsigned long long O = F.child_mask[f] & full;   // (a listed family has masks)
  const unsigned long long P = pred[ti] & full & ~O;
  const int no = __popcll(O), nq = __popcll(P), nz = no + nq;
  const int row = F.data_row[f];
  const int sn = lg_noise_slot(Nz, f);
  // LDS: [W | dv] of mom_solve, then this kernel's arrays
  double* __restrict__ W = imp_lds;
  double* __restrict__ dv = imp_lds + m * ld;
  double* __restrict__ Vz = imp_lds + mom_lds_doubles(m);   // V_ZZ (nz x nz), then V_OO's factor below its diagonal
  double* __restrict__ Cu = Vz + p * p;                     // Cov(u_Z) (nz x nz), both triangles
  double* __restrict__ Ym = Cu + p * p;                     // V_OP -> Y = L^-1 V_OP -> B' = L^-T Y   (no x nq)
  double* __restrict__ Cm = Ym + p * p;                     // C = V_PP - Y'Y (nq x nq), both triangles
  double* __restrict__ Dm = Cm + p * p;                     // the copy of C that is factorised, then G = [-B I] Cov(u_Z) (nq x nz)
  double* __restrict__ eu = Dm + p * p;                     // E[u_Z]
  double* __restrict__ wv = eu + p;                         // w_Z
  double* __restrict__ yv = wv + p;                         // y_O
  double* __restrict__ rv = yv + p;                         // y_O - w_O - E[u_O]
  double* __restrict__ dlV = rv + p;                        // diagonal of V_OO's factor
  double* __restrict__ dlC = dlV + p;                       // diagonal of C's factor
  double* __restrict__ cf = dlC + p;                        // rows of K: qc, vc, wc
  double* __restrict__ xm = cf + 3 * K;                     // [k][i]: posterior mean of parent k (or its constant) at trait Z_i
  int* __restrict__ ipos = reinterpret_cast<int*>(imp_lds + mom_lds_doubles(m) + ((impute_extra_doubles(p, K) + 1) & ~(size_t)1));
  int* __restrict__ zidx = ipos + K;                        // Z: the observed traits in order, then the predicted ones
  int* __restrict__ vi = zidx + p;                          // [k][i]: the variable's index in the cluster, -1: a constant
  // a packed (BS16) record is first copied here in the plain layout (fam_stage_plain)
  double* __restrict__ stage = imp_lds + mom_lds_doubles(m) + ((impute_extra_doubles(p, K) + 1) & ~(size_t)1) +
                               ((impute_extra_ints(p, K) + 1) >> 1);
  bool any_scope = false;
  for (int k = 0; k < np; ++k) any_scope |= F.parent_pos[(size_t)f * K + k] >= 0;
  const bool packed = bs && bs16::applies(m, fp);
  // (every condition of an early `continue` below is the same in all threads of the workgroup: P and any_scope belong to the
  // family, mom_solve and lds_cholesky return what every thread computed from the same LDS words)
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const int64_t slot = (int64_t)site * n_fam + ti;
    double* __restrict__ om = mean ? mean + slot * p : nullptr;
    double* __restrict__ oc = cov ? cov + slot * p * p : nullptr;
    if (P == 0ull) {   // nothing to predict: no solve
      if (om) for (int a = t; a < p; a += NT) om[a] = NAN;
      if (oc) for (int a = t; a < p * p; a += NT) oc[a] = NAN;
      if (t == 0) info[slot] = -1;
      continue;
    }
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
    if (st != 0) {   // the cluster is not positive definite, or the constant belief (J = 0) while a parent's moments are needed
      if (om) for (int a = t; a < p; a += NT) om[a] = NAN;
      if (oc) for (int a = t; a < p * p; a += NT) oc[a] = NAN;
      if (t == 0) info[slot] = st > 0 ? 1 + st : 1;
      continue;
    }
    // coefficients, positions, the traits of Z
    for (int k = t; k < np; k += NT) {
      lg_coefs<false>(M.model, S.alpha, F.length[(size_t)f * K + k], F.gamma[(size_t)f * K + k], cf[k], cf[K + k], cf[2 * K + k]);
      ipos[k] = F.parent_pos[(size_t)f * K + k];
    }
    for (int tr = t; tr < p; tr += NT) {
      if ((O >> tr) & 1ull) zidx[mask_rank(O, tr)] = tr;
      else if ((P >> tr) & 1ull) zidx[no + mask_rank(P, tr)] = tr;
    }
    __syncthreads();
    // where each cluster parent's traits of Z sit in the cluster, and their posterior mean (or the fixed root's constant)
    // (P is not empty: every cluster parent holds a trait, its parent_pos is not negative; a negative one is the fixed root)
    fam_blocks<NT>(F, f, as, S.mu, 0, np, O, ipos, zidx, nz, W, ld, m, vi, xm, t);
    for (int i = t; i < no; i += NT) yv[i] = F.data[(as * F.n_rows + row) * p + zidx[i]];
    // V_ZZ
    for (int idx = t; idx < nz * nz; idx += NT) {
      const int i = idx / nz, j = idx - i * nz;
      const int e = zidx[i] + zidx[j] * p;
      double v = 0.0;
      for (int k = 0; k < np; ++k) v = v + cf[K + k] * S.R[(int64_t)F.color[(size_t)f * K + k] * p * p + e];
      if (sn >= 0) v = v + lg_noise_E(Nz, sn, zidx[i], zidx[j], p, as);   // a noisy tip: the observation's V + E, blocks E_PP, E_PO included
      Vz[i * nz + j] = v;
    }
    __syncthreads();
    // E[u_Z], w_Z and the residual of the observed traits
    for (int i = t; i < nz; i += NT) {
      double e = 0.0;
      for (int k = 0; k < np; ++k) e = e + cf[k] * xm[k * p + i];
      double w = 0.0;
      if (S.theta)
        for (int k = 0; k < np; ++k) w = w + cf[2 * K + k] * S.theta[zidx[i]];
      if (Sh.slot) w = w + lg_shift_d(Sh, F.gamma, f, K, np, zidx[i], p, as);   // a shift of the mean: the full p-vector of d
      eu[i] = e;
      wv[i] = w;
      if (i < no) rv[i] = (yv[i] - w) - e;
    }
    // Cov(u_Z): the lower triangle, mirrored
    for (int idx = t; idx < nz * nz; idx += NT) {
      const int i = idx / nz, j = idx - i * nz;
      if (j > i) continue;
      const double s = fam_cov(W, ld, vi, p, [&](int k) -> double { return cf[k]; }, np, i, j);
      Cu[i * nz + j] = s;
      Cu[j * nz + i] = s;
    }
    __syncthreads();
    bool ok = lds_cholesky<NT>(Vz, no, nz, dlV, nullptr, t);
    if (ok) {
      // Y = L^-1 V_OP: thread j its own column, rows in order
      for (int j = t; j < nq; j += NT)
        for (int i = 0; i < no; ++i) {
          double s = Vz[i * nz + no + j];
          for (int k = 0; k < i; ++k) s = fma(-Vz[i * nz + k], Ym[k * nq + j], s);
          Ym[i * nq + j] = s / dlV[i];
        }
      __syncthreads();
      // C = V_PP - Y'Y, the conditional variance of the noise: the lower triangle, mirrored; and the copy to factorise
      for (int idx = t; idx < nq * nq; idx += NT) {
        const int a = idx / nq, b = idx - a * nq;
        if (b > a) continue;
        double s = Vz[(no + a) * nz + no + b];
        for (int l = 0; l < no; ++l) s = fma(-Ym[l * nq + a], Ym[l * nq + b], s);
        Cm[a * nq + b] = s;
        Cm[b * nq + a] = s;
        Dm[a * nq + b] = s;
      }
      __syncthreads();
      ok = lds_cholesky<NT>(Dm, nq, nq, dlC, nullptr, t);   // (nq >= 1: it ends behind a barrier)
    }
    if (!ok) {   // V_OO or the conditional variance is not positive definite
      if (om) for (int a = t; a < p; a += NT) om[a] = NAN;
      if (oc) for (int a = t; a < p * p; a += NT) oc[a] = NAN;
      if (t == 0) info[slot] = 1;
      continue;
    }
    // B' = L^-T Y in place: thread j its own column, rows from the last
    for (int j = t; j < nq; j += NT)
      for (int i = no - 1; i >= 0; --i) {
        double s = Ym[i * nq + j];
        for (int k = i + 1; k < no; ++k) s = fma(-Vz[k * nz + i], Ym[k * nq + j], s);
        Ym[i * nq + j] = s / dlV[i];
      }
    __syncthreads();
    // G = [-B I] Cov(u_Z)   (nq x nz; B(a, l) = Ym[l][a])
    for (int idx = t; idx < nq * nz; idx += NT) {
      const int a = idx / nz, j = idx - a * nz;
      double s = 0.0;
      for (int l = 0; l < no; ++l) s = fma(Ym[l * nq + a], Cu[l * nz + j], s);
      Dm[a * nz + j] = Cu[(no + a) * nz + j] - s;
    }
    // NaN outside P (every entry is written by exactly one thread)
    if (om)
      for (int a = t; a < p; a += NT)
        if (!((P >> a) & 1ull)) om[a] = NAN;
    if (oc)
      for (int a = t; a < p * p; a += NT) {
        const int ja = a / p, ia = a - ja * p;
        if (!((P >> ia) & 1ull) || !((P >> ja) & 1ull)) oc[a] = NAN;
      }
    if (om)
      for (int a = t; a < nq; a += NT) {
        double d = 0.0;
        for (int l = 0; l < no; ++l) d = fma(Ym[l * nq + a], rv[l], d);
        om[zidx[no + a]] = (eu[no + a] + wv[no + a]) + d;
      }
    __syncthreads();
    // cov = C + G [-B I]': the lower triangle, mirrored
    if (oc)
      for (int idx = t; idx < nq * nq; idx += NT) {
        const int a = idx / nq, b = idx - a * nq;
        if (b > a) continue;
        double s = 0.0;
        for (int l = 0; l < no; ++l) s = fma(Dm[a * nz + l], Ym[l * nq + b], s);
        const double v = (Cm[a * nq + b] + Dm[a * nz + no + b]) - s;
        oc[zidx[no + a] + zidx[no + b] * p] = v;
        oc[zidx[no + b] + zidx[no + a] * p] = v;
      }
    if (t == 0) info[slot] = 0;
  }
}

// bound of the call's device outputs, in doubles: those of a chunk of sites (pgbp_impute_scratch_limit)
static std::atomic<int64_t> g_impute_limit{(int64_t)32 << 20};

}  // namespace pgbp

using namespace pgbp;

// the count and the list are the host table's, whatever the clusters' sizes (the sweep is not served above 128 variables)
extern "C" int32_t pgbp_lg_impute_count(pgbp_engine* e) {
  if (!e) return -1;
  const LgModel* L = engine_lg(e);
  if (!L) return engine_fail(e, PGBP_ERR_STATE, "pgbp_lg_impute_count: no family table (call pgbp_lg_setup first)"), -1;
  std::vector<int32_t> fams;
  std::vector<unsigned long long> pred;
  lg_impute_list(*L, fams, pred);   // (with the tips a per-site mask hides at some site: pgbp_lg_impute_sites)
  return (int32_t)fams.size();
}

extern "C" int pgbp_lg_impute_families(pgbp_engine* e, int32_t* fam, uint64_t* predicted) {
  if (!e) return PGBP_ERR_INVALID;
  const LgModel* L = engine_lg(e);
  if (!L) return engine_fail(e, PGBP_ERR_STATE, "pgbp_lg_impute_families: no family table (call pgbp_lg_setup first)");
  std::vector<int32_t> fams;
  std::vector<unsigned long long> pred;
  lg_impute_list(*L, fams, pred);
  if (fam) std::copy(fams.begin(), fams.end(), fam);
  if (predicted)
    for (size_t i = 0; i < pred.size(); ++i) predicted[i] = (uint64_t)pred[i];
  return PGBP_OK;
}

extern "C" void pgbp_impute_scratch_limit(int64_t doubles) { g_impute_limit.store(doubles > 0 ? doubles : (int64_t)32 << 20); }

extern "C" int pgbp_lg_impute(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* mean, double* cov, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const LgModel* L = nullptr;
  int rc = lg_sweep_state(e, "pgbp_lg_impute", site_begin, site_end, &L, "pgbp_lg_impute_sites");
  if (rc) return rc;
  if ((rc = lg_refuse_optima(e, "pgbp_lg_impute", L))) return rc;
  const LgStatic& F = L->F;
  const LgParams& M = L->M;
  const LgShifts& Sh = L->Sh;
  const LgNoise& Nz = L->Nz;
  if (!mean && !cov) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_impute: no output buffer (mean and cov are both NULL)");
  EngineView v;
  if ((rc = engine_view(e, &v))) return rc;
  // the limits are pgbp_lg_loo's, over the clusters of ALL families of the table: an engine serves every sweep or none
  int max_m = 0;
  std::string why;
  if (!L->T.cluster_dims("pgbp_lg_impute", kLdsMaxDim, &max_m, why)) return engine_fail(e, PGBP_ERR_INVALID, why);
  // the listed families (tip families with a missing trait), in table order, the cluster of each and its mask P
  std::vector<int32_t> fams, cls;
  std::vector<unsigned long long> pred;
  L->T.impute_list(fams, pred);
  for (int32_t f : fams) cls.push_back(L->T.cluster[f]);
  // (as in pgbp_lg_loo, what follows runs on the caller's current device)
  const Plan& pl = *v.plan;
  const int p = F.p, K = F.K, n = (int)fams.size();
  size_t stage = 0;   // a packed record's plain copy
  for (int i = 0; i < n && v.bs16; ++i) {
    const size_t m = (size_t)pl.dims[cls[i]];
    if (bs16::applies((int)m, pl.fast_p)) stage = std::max(stage, m * m + m);
  }
  const size_t lds_bytes = sizeof(double) * impute_lds_doubles(max_m, p, K, stage);
  if (lds_bytes > 160 * 1024)
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_impute: a cluster of " + std::to_string(max_m) + " variables with " +
                                                std::to_string(p) + " traits needs " + std::to_string(lds_bytes) +
                                                " bytes of LDS, more than the 160 KB of a compute unit");
  const int ns = site_end - site_begin;
  if (ns == 0 || n == 0) return PGBP_OK;
  const int pp = p * p;
  const int64_t per_site = (int64_t)n * (1 + (mean ? p : 0) + (cov ? pp : 0));
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(ns, g_impute_limit.load() / per_site));
  DevBuf<int32_t> d_fams, d_cls, d_info;
  DevBuf<unsigned long long> d_pred;
  DevBuf<double> d_mean, d_cov;
  const size_t cn = (size_t)chunk * n;
  hipError_t herr = (hipError_t)d_fams.alloc(n);
  if (herr == hipSuccess) herr = (hipError_t)d_cls.alloc(n);
  if (herr == hipSuccess) herr = (hipError_t)d_pred.alloc(n);
  if (herr == hipSuccess) herr = (hipError_t)d_info.alloc(cn);
  if (herr == hipSuccess && mean) herr = (hipError_t)d_mean.alloc(cn * p);
  if (herr == hipSuccess && cov) herr = (hipError_t)d_cov.alloc(cn * pp);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_fams.get(), fams.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_cls.get(), cls.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess)
    herr = hipMemcpyAsync(d_pred.get(), pred.data(), sizeof(unsigned long long) * n, hipMemcpyHostToDevice, v.st);
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_impute (scratch): ") + hipGetErrorString(herr));
  (void)hipGetLastError();   // (an error an earlier asynchronous call left behind is that call's to report)
  {
    const void* kern =
        max_m <= 64 ? reinterpret_cast<const void*>(impute_family<64>) : reinterpret_cast<const void*>(impute_family<256>);
    if (lds_bytes > 64 * 1024) herr = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    for (int s0 = 0; herr == hipSuccess && s0 < ns; s0 += chunk) {
      const int nsc = std::min(chunk, ns - s0), gy = std::min(nsc, 65535);
      if (max_m <= 64)
        hipLaunchKernelGGL(impute_family<64>, dim3(n, gy), dim3(64), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, Nz, d_fams.get(), d_cls.get(), d_pred.get(), n, site_begin + s0, nsc,
                           d_mean.get(), d_cov.get(), d_info.get());
      else
        hipLaunchKernelGGL(impute_family<256>, dim3(n, gy), dim3(256), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, Nz, d_fams.get(), d_cls.get(), d_pred.get(), n, site_begin + s0, nsc,
                           d_mean.get(), d_cov.get(), d_info.get());
      herr = hipGetLastError();
      const size_t o = (size_t)s0 * n, len = (size_t)nsc * n;
      if (herr == hipSuccess && mean)
        herr = hipMemcpyAsync(mean + o * p, d_mean.get(), sizeof(double) * len * p, hipMemcpyDeviceToHost, v.st);
      if (herr == hipSuccess && cov)
        herr = hipMemcpyAsync(cov + o * pp, d_cov.get(), sizeof(double) * len * pp, hipMemcpyDeviceToHost, v.st);
      if (herr == hipSuccess && info)
        herr = hipMemcpyAsync(info + o, d_info.get(), sizeof(int32_t) * len, hipMemcpyDeviceToHost, v.st);
    }
  }
  const hipError_t serr = hipStreamSynchronize(v.st);
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_impute: ") + hipGetErrorString(herr));
  return PGBP_OK;
}

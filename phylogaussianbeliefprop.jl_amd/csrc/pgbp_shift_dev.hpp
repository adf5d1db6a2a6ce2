// Mean shifts on edges (pgbp_lg_set_shifts of include/pgbp.h), device side: the displacement d = sum_k gamma_k s_k that a
// family's offset w gains; and painted optima under OU (pgbp_lg_set_optima), which displace w by d_opt (lg_optima_d
// below).  Shared by the correction of the factor fill (pgbp_shift.hip) and by the four post-calibration
// sweeps, which all form w themselves: pgbp_grad.hip and pgbp_edge.hip in their common body (fam_score_T of
// pgbp_fam_dev.hpp), pgbp_loo.hip and pgbp_impute.hip in their own kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "pgbp_kernels.hpp"

namespace pgbp {

// the shift s_k of parent edge k of family f at trait tr for site `site` (absolute), 0 when that edge carries none
__device__ __forceinline__ double lg_shift_value(const LgShifts& S, int64_t edge, int tr, int p, int64_t site) {
  const int s = S.slot[edge];
  if (s < 0) return 0.0;
  return S.value[((S.per_site ? site * S.n : 0) + s) * p + tr];
}

// does family f (np parent edges, row length K) carry a shift on any of its edges?
__device__ __forceinline__ bool lg_shift_any(const LgShifts& S, int64_t f, int K, int np) {
  if (!S.slot) return false;
  for (int k = 0; k < np; ++k)
    if (S.slot[f * K + k] >= 0) return true;
  return false;
}

// d_tr = sum_k gamma_k s_k[tr] over the shifted edges of family f, in the order of k; 0 without shifts
__device__ __forceinline__ double lg_shift_d(const LgShifts& S, const double* __restrict__ gamma, int64_t f, int K, int np,
                                             int tr, int p, int64_t site) {
#pragma clang fp contract(off)
  double d = 0.0;
  if (!S.slot) return d;
  for (int k = 0; k < np; ++k) {
    const int s = S.slot[f * K + k];
    if (s >= 0) d = d + gamma[f * K + k] * S.value[((S.per_site ? site * S.n : 0) + s) * p + tr];
  }
  return d;
}

// Painted optima (pgbp_lg_set_optima): does family f carry a regime on any of its edges?
__device__ __forceinline__ bool lg_optima_any(const LgOptima& Op, int64_t f, int K, int np) {
  if (!Op.regime) return false;
  for (int k = 0; k < np; ++k)
    if (Op.regime[f * K + k] > 0) return true;
  return false;
}

// d_opt at trait tr = sum_k wc_k (theta_r(f,k) - theta) over the painted edges of family f, in the order of k, wc_k =
// gamma_k (1 - exp(-alpha t_k)) as lg_coefs forms it; 0 without optima.  theta: of this site (LgParams), alpha likewise.
// value_sm is read where it exists (p = 1, per-site values: a line per wavefront when lanes are sites).
__device__ __forceinline__ double lg_optima_d(const LgOptima& Op, const double* __restrict__ theta, double alpha,
                                              const double* __restrict__ length, const double* __restrict__ gamma, int64_t f,
                                              int K, int np, int tr, int p, int64_t site, int64_t sm_stride) {
#pragma clang fp contract(off)
  double d = 0.0;
  if (!Op.regime) return d;
  for (int k = 0; k < np; ++k) {
    const int r = Op.regime[f * K + k];
    if (r <= 0) continue;
    const double wc = gamma[f * K + k] * (1.0 - exp(-alpha * length[f * K + k]));
    const double th = Op.value_sm ? Op.value_sm[(int64_t)(r - 1) * sm_stride + site]
                                  : Op.value[((Op.per_site ? site * Op.n : 0) + (r - 1)) * p + tr];
    d = d + wc * (th - theta[tr]);
  }
  return d;
}

// Per-site clade shifts of the optimum (pgbp_lg_set_clade_shifts_sites): the sum of the deltas of this site's slots whose
// clade holds family f -- pre[v_j] <= pre[f] <= last[v_j] -- added in slot order.  any: does a slot cover f at all?
__device__ __forceinline__ double lg_clade_sum(const LgCladeShifts& C, int64_t f, int64_t site, bool& any) {
#pragma clang fp contract(off)
  double s = 0.0;
  bool hit = false;
  if (C.family) {
    const int r = C.pre[f];
    for (int j = 0; j < C.n_slots; ++j) {
      const int v = C.family[(int64_t)j * C.row + site];
      if (v < 0) continue;
      if (C.pre[v] <= r && r <= C.last[v]) {
        s = s + C.delta[(int64_t)j * C.row + site];
        hit = true;
      }
    }
  }
  any = hit;
  return s;
}

// d_clade = sum_k wc_k times that sum over the parent edges of family f (one on a tree), wc_k as lg_coefs forms it: what the
// offset w of family f gains at this site; 0 without a setting
__device__ __forceinline__ double lg_clade_d(const LgCladeShifts& C, double alpha, const double* __restrict__ length,
                                             const double* __restrict__ gamma, int64_t f, int K, int np, int64_t site,
                                             bool& any) {
#pragma clang fp contract(off)
  const double s = lg_clade_sum(C, f, site, any);
  if (!C.family) return 0.0;
  double d = 0.0;
  for (int k = 0; k < np; ++k) {
    const double wc = gamma[f * K + k] * (1.0 - exp(-alpha * length[f * K + k]));
    d = d + wc * s;
  }
  return d;
}

// The displacement of family f at this site and trait: what its offset w gains from the shifts on its edges and from the painted
// optima.  The one statement of it for the correction of the fill (pgbp_shift.hip), the noise correction (pgbp_noise.hip) and
// the per-site mask (pgbp_sitemiss.hip).  alpha, theta: of this site; sm_stride: the row length of value_sm.
__device__ __forceinline__ double lg_disp_d(const LgShifts& S, const LgOptima& Op, const double* __restrict__ theta, double alpha,
                                            const double* __restrict__ length, const double* __restrict__ gamma, int64_t f, int K,
                                            int np, int tr, int p, int64_t site, int64_t sm_stride) {
#pragma clang fp contract(off)
  const double d = lg_shift_d(S, gamma, f, K, np, tr, p, site);
  if (!Op.regime) return d;
  return d + lg_optima_d(Op, theta, alpha, length, gamma, f, K, np, tr, p, site, sm_stride);
}

}  // namespace pgbp

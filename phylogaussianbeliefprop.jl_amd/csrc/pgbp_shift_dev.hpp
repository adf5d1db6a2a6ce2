// Mean shifts on edges (pgbp_lg_set_shifts of include/pgbp.h), device side: the displacement d = sum_k gamma_k s_k that a
// family's offset w gains.  Shared by the correction of the factor fill (pgbp_shift.hip) and by the four post-calibration
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

}  // namespace pgbp

// Measurement error at the tips (pgbp_lg_set_tip_noise of include/pgbp.h), device side: the matrix
// E_f = scale_f Sigma_e + diag(se2_f) that the conditional variance of a noisy tip family gains.  Shared by the correction of
// the factor fill (pgbp_noise.hip) and by the post-calibration sweeps, which all form V_OO themselves: fam_score_T of
// pgbp_fam_dev.hpp (pgbp_grad.hip, pgbp_edge.hip, pgbp_scan.hip), pgbp_loo.hip and pgbp_impute.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "pgbp_kernels.hpp"

namespace pgbp {

// the noise slot of family f, -1: none set or not a noisy family
__device__ __forceinline__ int lg_noise_slot(const LgNoise& N, int64_t f) { return N.slot ? N.slot[f] : -1; }

// E_f(ti, tj) of the family with slot s >= 0 at the traits ti, tj for site `site` (absolute)
__device__ __forceinline__ double lg_noise_E(const LgNoise& N, int s, int ti, int tj, int p, int64_t site) {
#pragma clang fp contract(off)
  const int64_t ps = N.per_site ? site : 0;
  double v = N.scale[s] * N.sigma_e[(ps * p + tj) * p + ti];
  if (ti == tj && N.se2) v = v + N.se2[((ps * N.n) + s) * p + ti];
  return v;
}

}  // namespace pgbp

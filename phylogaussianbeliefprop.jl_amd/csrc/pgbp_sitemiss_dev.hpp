// Per-site missing tips of a univariate batch (pgbp_lg_set_site_missing of include/pgbp.h), device side: the one test the fill
// correction (pgbp_sitemiss.hip) and the lanes-are-sites sweeps (pgbp_fam_uni_dev.hpp, pgbp_grad_uni.hip, pgbp_post_uni.hip)
// make.  The setter accepts bits only at the data rows of tip families, so callers test tip families only.
#pragma once
#include <hip/hip_runtime.h>

#include "pgbp_kernels.hpp"

namespace pgbp {

// is the tip with data row `row` masked at site `as` (absolute)?  A wavefront of 64 consecutive sites reads at most two words.
__device__ __forceinline__ bool lg_site_masked(const LgSiteMiss& Ms, int row, int64_t as) {
  return Ms.words && ((Ms.words[(int64_t)row * Ms.W + (as >> 6)] >> (as & 63)) & 1ull);
}

// the same for family f of the table: false for anything but a tip family (child_pos < 0, a data row, a parent edge)
__device__ __forceinline__ bool lg_site_masked_family(const LgSiteMiss& Ms, const LgStatic& F, int f, int64_t as) {
  if (!Ms.words) return false;
  const int row = F.data_row[f];
  return F.child_pos[f] < 0 && row >= 0 && F.n_parents[f] > 0 && lg_site_masked(Ms, row, as);
}

}  // namespace pgbp

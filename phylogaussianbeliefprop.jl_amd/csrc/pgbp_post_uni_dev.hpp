// Device pieces shared by the lanes-are-sites sweeps over a schedule tree of a univariate batch (pgbp_post_uni.hip: the joint
// draws; pgbp_cov_uni.hip: the posterior covariance): what every kernel takes of the engine and of the call, the closed-form
// conditional of a cluster's R given its S at a site, and the validity pass -- which site has a conditional J_RR that is not
// positive definite, and which cluster in preorder is the first.  Frame and arithmetic contract of pgbp_fam_uni_dev.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "pgbp_fam_uni_dev.hpp"
#include "pgbp_sample_plan.hpp"

namespace pgbp {

// what every kernel takes of the engine and of the call
struct PostUniArgs {
  const double* pool;
  int64_t stride;
  const int64_t* off;
  const int32_t* bdim;
  int site0, n_sites;
  int64_t row;   // the row length of the scratch (the chunk)
};

// The conditional of a cluster's R given its S at a site: x_R = a - G x_S + T z_R (at most five numbers; r = 1: a0, G, T00;
// r = 2: a0, a1, T00, T01, T11).  ok: J_RR is positive definite, pivot by pivot as mom_cond_factor tests it.
struct PostUniCond {
  double a0, a1, G, T00, T01, T11;
  bool ok;
};

// m, r of the cluster; pr: the position of R in a cluster of 2 variables with r = 1
template <bool SM>
__device__ __forceinline__ PostUniCond post_uni_cond(const double* __restrict__ pool, int64_t stride, int64_t o, int m, int r, int pr,
                                                     int64_t as) {
#pragma clang fp contract(off)
  PostUniCond c{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, true};
  if (r == 2) {
    const double a = fam_uni_ld<SM>(pool, stride, o, 0, as), b = fam_uni_ld<SM>(pool, stride, o, 2, as);
    const double d = fam_uni_ld<SM>(pool, stride, o, 3, as);
    const double h0 = fam_uni_ld<SM>(pool, stride, o, 4, as), h1 = fam_uni_ld<SM>(pool, stride, o, 5, as);
    const double ba = b / a, sc = d - ba * b;
    c.ok = a > 0.0 && sc > 0.0;
    c.a1 = (h1 - ba * h0) / sc;
    c.a0 = (h0 - b * c.a1) / a;
    c.T00 = 1.0 / sqrt(a);
    c.T11 = 1.0 / sqrt(sc);
    c.T01 = -(ba * c.T11);
  } else if (r == 1) {
    const int jd = m == 2 ? 3 * pr : 0;   // J[pr][pr] of the column-major record
    const double J = fam_uni_ld<SM>(pool, stride, o, jd, as), h = fam_uni_ld<SM>(pool, stride, o, m * m + pr, as);
    c.ok = J > 0.0;
    c.a0 = h / J;
    if (m == 2) c.G = fam_uni_ld<SM>(pool, stride, o, 2, as) / J;   // the upper triangle: J[0][1]
    c.T00 = 1.0 / sqrt(J);
  }
  return c;
}

// pre[k]: the item of the cluster of preorder rank k (clusters with variables only).  pfirst: [blocks][row], the smallest rank of
// the block whose J_RR is not positive definite, kFamUniNoInfo: none
template <bool SM>
__global__ __launch_bounds__(256) void post_uni_valid(PostUniArgs A, const SampItem* __restrict__ pre, int n_pre,
                                                      const int32_t* __restrict__ idx, int32_t* __restrict__ pfirst) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A.n_sites) return;
  const int64_t as = (int64_t)A.site0 + s;
  int first = kFamUniNoInfo;
  const int k0 = blockIdx.y * kFamUniBlock, k1 = min(k0 + kFamUniBlock, n_pre);
  for (int k = k0; k < k1; ++k) {
    const SampItem it = pre[k];
    if (it.r == 0) continue;
    const PostUniCond c = post_uni_cond<SM>(A.pool, A.stride, A.off[it.cluster], it.m, it.r, idx[it.perm], as);
    if (!c.ok && first == kFamUniNoInfo) first = k;
  }
  pfirst[(int64_t)blockIdx.y * A.row + s] = first;
}

// rank[out0 + site] = 1 + the first preorder rank that failed, the blocks folded in order; 0: none.  (One copy per file that
// includes this header: each object carries its own device code.)
static __global__ __launch_bounds__(256) void post_uni_first(const int32_t* __restrict__ pfirst, int nb, int n_sites, int64_t row,
                                                             int32_t* __restrict__ rank, int out0) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_sites) return;
  int first = kFamUniNoInfo;
  for (int b = 0; b < nb; ++b) {
    const int v = pfirst[(int64_t)b * row + s];
    if (first == kFamUniNoInfo) first = v;
  }
  rank[out0 + s] = first == kFamUniNoInfo ? 0 : first + 1;
}

}  // namespace pgbp

// Device pieces shared by the lanes-are-sites sweeps over a schedule tree of a univariate batch (pgbp_post_uni.hip: the joint
// draws; pgbp_cov_uni.hip: the posterior covariance): the closed-form conditional of a cluster's R given its S at a site, and
// the validity pass -- which site has a conditional J_RR that is not positive definite, and which cluster in preorder is the
// first -- with its host side: its table, its two launches, and the info it gives.  Frame and arithmetic contract of
// pgbp_fam_uni_dev.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "pgbp_fam_uni_dev.hpp"
#include "pgbp_sample_plan.hpp"
#include "pgbp_sites_host.hpp"

namespace pgbp {

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
__global__ __launch_bounds__(256) void post_uni_valid(SitesArgs A, const SampItem* __restrict__ pre, int n_pre,
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

// The table of a sweep: the items by level, and behind them the items of the clusters with variables by preorder rank (the
// validity pass).  at[c]: the item of cluster c among those by level, -1: no variables.
struct PostUniPre {
  std::vector<SampItem> tab;
  std::vector<int32_t> at, pre_cluster;
  int n_items, n_pre, nvb;   // items by level, by preorder rank, and the blocks of the latter
};

inline PostUniPre post_uni_pre(const SampPlan& sp) {
  PostUniPre pre{sp.by_level, std::vector<int32_t>(sp.nc, -1), {}, (int)sp.by_level.size(), 0, 0};
  for (size_t q = 0; q < sp.by_level.size(); ++q) pre.at[sp.by_level[q].cluster] = (int32_t)q;
  for (int32_t cl : sp.order)
    if (pre.at[cl] >= 0) {
      pre.tab.push_back(sp.by_level[pre.at[cl]]);
      pre.pre_cluster.push_back(cl);
    }
  pre.n_pre = (int)pre.pre_cluster.size();
  pre.nvb = (pre.n_pre + kFamUniBlock - 1) / kFamUniBlock;
  return pre;
}

// the pass over the chunk of A: d_rank[s0 + site] for its sites (d_pfirst: [nvb][row] of scratch)
static inline void post_uni_validity(SitesScratch& S, int sm, const SitesArgs& A, const PostUniPre& pre, const SampItem* d_tab,
                                     const int32_t* d_idx, int32_t* d_pfirst, int32_t* d_rank, int s0) {
  const dim3 gs((A.n_sites + 255) / 256);
  PGBP_SITES_LAUNCH(S, sm, post_uni_valid, dim3(gs.x, pre.nvb), A, d_tab + pre.n_items, pre.n_pre, d_idx, d_pfirst);
  S.launch(post_uni_first, gs, d_pfirst, pre.nvb, A.n_sites, A.row, d_rank, s0);
  S.check();
}

// info[s]: the 1-based index of the first cluster in preorder whose J_RR is not positive definite at site s, 0: none
inline void post_uni_info(const PostUniPre& pre, const std::vector<int32_t>& rank, int32_t* info) {
  if (!info) return;
  for (size_t s = 0; s < rank.size(); ++s) info[s] = rank[s] ? pre.pre_cluster[rank[s] - 1] + 1 : 0;
}

}  // namespace pgbp

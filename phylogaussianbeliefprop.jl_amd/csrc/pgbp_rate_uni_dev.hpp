// Phase one of the cross-site calls of a univariate batch (pgbp_rate_uni.hip: the rate matrix between the sites;
// pgbp_rate_apply_uni.hip: the rate matrix applied to a block of vectors), written once: the residual rows
// U[family][site] = e / sqrt(t) of a chunk of families, and the fold of the blocks' den partials and marks across the chunks.
// Frame and arithmetic contract of pgbp_fam_uni_dev.hpp.  (One copy of the device code per file that includes this header.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "pgbp_fam_uni_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"

namespace pgbp {

typedef double rate_v4d __attribute__((ext_vector_type(4)));

// U rows [row][site] of the chunk's families f_begin .. f_begin + rows4 (rows4: a multiple of 4, at most 64 grid.y); pden,
// pinfo: [block][site], the row length is A.row throughout
template <bool SM>
__global__ __launch_bounds__(256) void rate_uni_resid(SitesArgs A, LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz, LgSiteMiss Ms,
                                                      int n_fam, int f_begin, int rows4, double* __restrict__ U,
                                                      double* __restrict__ pden, int32_t* __restrict__ pinfo) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x, fb = blockIdx.y;
  if (s >= A.n_sites) return;   // (a lane past the range: no barrier follows, and no other lane's store is its to make)
  const int64_t as = (int64_t)A.site0 + s;
  const int K = F.K;
  const LgSite S = lg_site(M, F.n_rates, 1, as);
  double den = 0.0;
  int bad = kFamUniNoInfo;
  const int r0 = fb * kFamUniBlock, r1 = min(r0 + kFamUniBlock, rows4);
  for (int r = r0; r < r1; ++r) {
    const int f = f_begin + r;
    double u = 0.0;
    if (f < n_fam) {
      const int np = F.n_parents[f];
      double tt = 0.0;
      for (int k = 0; k < np; ++k) {
        const double gk = F.gamma[(size_t)f * K + k];
        tt = tt + gk * gk * F.length[(size_t)f * K + k];   // (:459)
      }
      // the families exact_uni_family skips, in its order
      bool in = !(np == 0 || tt == 0.0 || A.bdim[A.fam_cluster[f]] == 0);
      if (in && F.child_pos[f] < 0 && F.parent_mask && F.parent_mask[(size_t)f * K] == 0ull) in = false;
      if (in) {
        const FamUni X = fam_uni_family<SM>(A.pool, A.stride, A.off, A.bdim, F, M, Sh, Nz, Ms, S, A.fam_cluster, f, A.data_row_len, as);
        if (!X.skip) {
          if (X.q.st != 0) {
            if (X.q.st > 0) bad = min(bad, X.c + 1);
            u = NAN;
            den = NAN;
          } else {
            u = X.e / sqrt(tt);
            den = den + (1.0 - X.C / tt);
          }
        }
      }
    }
    U[(int64_t)r * A.row + s] = u;
  }
  pden[(int64_t)fb * A.row + s] = den;
  pinfo[(int64_t)fb * A.row + s] = bad;
}

// grid.y = 0: den[out0 + site] = (first ? 0.0 : what the chunks before left) + the chunk's blocks in block order -- over the
// chunks of a call the sum exact_uni_reduce forms; grid.y = 1: the smallest mark so far, and in the last chunk mu (as
// exact_uni_reduce) and info[out0 + site] = the mark or 0
template <bool SM>
__global__ __launch_bounds__(256) void rate_uni_reduce(SitesArgs A, const double* __restrict__ pden, const int32_t* __restrict__ pinfo,
                                                       int nblk, int first, int last, int root_belief, int root_pos,
                                                       double* __restrict__ den, double* __restrict__ mu, int32_t* __restrict__ info,
                                                       int out0) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A.n_sites) return;
  if (blockIdx.y == 0) {
    double acc = first ? 0.0 : den[out0 + s];
    for (int b = 0; b < nblk; ++b) acc = acc + pden[(int64_t)b * A.row + s];
    den[out0 + s] = acc;
  } else {
    int bad = first ? kFamUniNoInfo : info[out0 + s];
    for (int b = 0; b < nblk; ++b) bad = min(bad, pinfo[(int64_t)b * A.row + s]);
    if (last) {
      if (mu) {
        const FamUniMom q = fam_uni_moments<SM>(A.pool, A.stride, A.off[root_belief], A.bdim[root_belief], (int64_t)A.site0 + s);
        if (q.st > 0) bad = min(bad, root_belief + 1);
        mu[out0 + s] = q.st != 0 ? (double)NAN : (root_pos == 0 ? q.m0 : q.m1);
      }
      bad = bad == kFamUniNoInfo ? 0 : bad;
    }
    info[out0 + s] = bad;
  }
}

}  // namespace pgbp

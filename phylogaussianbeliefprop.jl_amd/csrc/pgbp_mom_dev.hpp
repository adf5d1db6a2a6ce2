// Device helpers shared by the kernels that solve a belief's system [J | h] in LDS (pgbp_moments.hip: pgbp_moments,
// pgbp_bm_exact_stats; the family sweeps pgbp_grad.hip, pgbp_edge.hip, pgbp_loo.hip, pgbp_impute.hip; pgbp_sample.hip).  Arithmetic contract: see the head of pgbp_moments.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "pgbp_bs16.hpp"

namespace pgbp {

__device__ __forceinline__ double refined_rcp(double d) {
  double rd = __builtin_amdgcn_rcp(d);
  rd = fma(fma(-d, rd, 1.0), rd, rd);
  rd = fma(fma(-d, rd, 1.0), rd, rd);
  return rd;
}

// The moments of one record by a workgroup of NT threads, in LDS: W (m x ld, ld = (m + 1) | 1) and dv (m).  Returns -1: the
// constant belief (J = 0, h = 0); > 0: PosDefException.info; 0: mu in column m of W and, COV, Sigma(l, j) at W[max(l, j)][min(l, j)].
// mant / expo / quad: the pieces of the normalisation constant (mom_norm).
template <int NT, bool COV>
__device__ __forceinline__ int mom_solve(const double* __restrict__ rec, const int m, const bool packed, const int fp,
                                         double* __restrict__ W, double* __restrict__ dv, const int t, double& mant, int& expo,
                                         double& quad) {
#pragma clang fp contract(off)
  const int ld = (m + 1) | 1;
  __syncthreads();   // (the previous site's matrix has been read)
  bool nz = false;
  for (int idx = t; idx < m * m; idx += NT) {
    const int j = idx / m, i = idx - j * m;
    if (packed) {
      const double v = rec[bs16::J_off(m, i, j, fp)];
      nz |= v != 0.0;
      W[i * ld + j] = v;
    } else {
      const double raw = rec[idx];
      nz |= raw != 0.0;
      W[i * ld + j] = (i <= j) ? raw : rec[j + (int64_t)i * m];   // PDMat(Symmetric(J)): the upper triangle
    }
  }
  for (int i = t; i < m; i += NT) {
    const double hv = packed ? rec[bs16::h_off(m, i, fp)] : rec[(int64_t)m * m + i];
    nz |= hv != 0.0;
    W[i * ld + m] = hv;
  }
  if (!__syncthreads_or(nz ? 1 : 0)) return -1;   // constant belief
  // elimination (eliminate_leading's operations, entry by entry; the lane grid shrinks with the trailing block)
  mant = 1.0;
  quad = 0.0;
  expo = 0;
  int info = 0;
  const int ncol = m + 1;
  for (int k = 0; k < m; ++k) {
    const double d = W[k * ld + k];
    const double hk = W[k * ld + m];
    if (!(d > 0.0)) {
      info = k + 1;
      break;   // (uniform: every thread reads the same pivot)
    }
    const double rd = refined_rcp(d);
    int ex;
    mant *= frexp(d, &ex);
    expo += ex;
    if ((k & 15) == 15) { mant = frexp(mant, &ex); expo += ex; }
    quad = fma(rd, hk * hk, quad);
    const int rem = ncol - k - 1;   // columns k + 1 .. m
    int lg = 0;
    while ((1 << lg) < rem && (1 << lg) < 64) ++lg;
    const int L = 1 << lg, jj = t & (L - 1), i0 = t >> lg, R = NT >> lg;
    for (int j = k + 1 + jj; j < ncol; j += L) {
      const double pkj = W[k * ld + j];
      for (int i = k + 1 + i0; i < m; i += R) W[i * ld + j] = fma(-(W[i * ld + k] * rd), pkj, W[i * ld + j]);
    }
    __syncthreads();
  }
  if (info != 0) return info;
  if constexpr (COV) {
    for (int i = t; i < m; i += NT) dv[i] = refined_rcp(W[i * ld + i]);
  }
  // back substitution on the upper-triangular system left by the elimination
  for (int k = m - 1; k >= 0; --k) {
    if (t == 0) W[k * ld + m] = W[k * ld + m] / W[k * ld + k];
    __syncthreads();
    const double xk = W[k * ld + m];
    for (int i = t; i < k; i += NT) W[i * ld + m] = fma(-W[i * ld + k], xk, W[i * ld + m]);
    __syncthreads();
  }
  if constexpr (COV) {
    // the inverse in place, row i from the rows below it: Sigma(l, j) sits at W[max][min]
    for (int i = m - 1; i >= 0; --i) {
      const double di = dv[i];
      const double* __restrict__ Ui = W + i * ld;
      for (int j = i + 1 + t; j < m; j += NT) {
        double dot = 0.0;
        for (int l = i + 1; l < j; ++l) dot = fma(Ui[l], W[j * ld + l], dot);
        for (int l = j; l < m; ++l) dot = fma(Ui[l], W[l * ld + j], dot);
        W[j * ld + i] = -(dot * di);
      }
      __syncthreads();
      if (t < 64) {   // the diagonal entry: partial sums of the first wavefront, added by a fixed tree
        double dot = 0.0;
        for (int l = i + 1 + t; l < m; l += 64) dot = fma(Ui[l], W[l * ld + i], dot);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
        if (t == 0) W[i * ld + i] = fma(-dot, di, di);
      }
      __syncthreads();
    }
  }
  return 0;
}

// The CONDITIONAL factorisation of one record (pgbp_sample.hip: pgbp_sample_posterior) by a group of GT threads (thread tg of the
// group; several groups may share a workgroup: every barrier below is met by the whole workgroup, `rb` = the largest r among
// its groups bounds the loops that hold one).  perm[0 .. r) = the variables R that stay random, perm[r .. m) = the variables S
// that are conditioned on; the system [J_RR | J_RS | h_R] is gathered through perm into W (r x ld, ld = (m + 1) | 1) and its r
// pivots are eliminated with mom_solve's operations, entry by entry: the upper triangle is read, the pivots in order,
// W[i][j] -= (W[i][k] * rd) * W[k][j] with rd the refined reciprocal of the pivot.  The s + 1 right-hand columns are then back
// substituted (mom_solve's division and update, column by column) and the triangular factor is inverted below the diagonal.
// Returns 0, or k + 1 when pivot k is not positive (W is then unspecified).  On return 0:
//   G = J_RR^-1 J_RS at W[i][r + j],  a = J_RR^-1 h_R at W[i][m],
//   T = L^-T, J_RR = L L' the Cholesky factor (L lower triangular, positive diagonal): T(i, j) at W[j][i] for i < j, T(j, j) in
//   dv[j] (= 1 / sqrt(pivot j)), zero below the diagonal.  The elimination leaves U = D^(1/2) L' (pivots d on its diagonal), so
//   T = U^-1 D^(1/2): column j by T(i, j) = -(sum_{i < l <= j} U(i, l) T(l, j)) / d_i, i = j - 1 .. 0, thread j its own column.
// Needs r <= GT.
template <int GT>
__device__ __forceinline__ int mom_cond_factor(const double* __restrict__ rec, const int m, const int r, const int rb,
                                               const int32_t* __restrict__ perm, const bool packed, const int fp,
                                               double* __restrict__ W, double* __restrict__ dv, const int tg) {
#pragma clang fp contract(off)
  const int ld = (m + 1) | 1;
  const int ncol = m + 1;
  __syncthreads();   // (the previous site's matrix has been read)
  for (int idx = tg; idx < r * m; idx += GT) {
    const int i = idx / m, j = idx - i * m;
    const int vi = perm[i], vj = perm[j];
    const int lo = vi < vj ? vi : vj, hi = vi < vj ? vj : vi;   // PDMat(Symmetric(J)): the upper triangle
    W[i * ld + j] = packed ? rec[bs16::J_off(m, lo, hi, fp)] : rec[lo + (int64_t)hi * m];
  }
  for (int i = tg; i < r; i += GT) W[i * ld + m] = packed ? rec[bs16::h_off(m, perm[i], fp)] : rec[(int64_t)m * m + perm[i]];
  __syncthreads();
  int info = 0;
  for (int k = 0; k < rb; ++k) {
    if (k < r && info == 0) {
      const double d = W[k * ld + k];
      if (!(d > 0.0)) {
        info = k + 1;   // (uniform in the group: every thread reads the same pivot)
      } else {
        const double rd = refined_rcp(d);
        const int rem = ncol - k - 1;   // columns k + 1 .. m
        int lg = 0;
        while ((1 << lg) < rem && (1 << lg) < 64 && (1 << lg) < GT) ++lg;
        const int L = 1 << lg, jj = tg & (L - 1), i0 = tg >> lg, R = GT >> lg;
        for (int j = k + 1 + jj; j < ncol; j += L) {
          const double pkj = W[k * ld + j];
          for (int i = k + 1 + i0; i < r; i += R) W[i * ld + j] = fma(-(W[i * ld + k] * rd), pkj, W[i * ld + j]);
        }
      }
    }
    __syncthreads();
  }
  const bool ok = info == 0;
  if (ok)
    for (int i = tg; i < r; i += GT) { const double d = W[i * ld + i]; dv[i] = sqrt(d) * refined_rcp(d); }
  // back substitution of the columns r .. m on the upper-triangular system left by the elimination
  const int nrhs = ncol - r;
  for (int k = rb - 1; k >= 0; --k) {
    const bool go = ok && k < r;
    if (go)
      for (int c = tg; c < nrhs; c += GT) W[k * ld + r + c] = W[k * ld + r + c] / W[k * ld + k];
    __syncthreads();
    if (go)
      for (int idx = tg; idx < k * nrhs; idx += GT) {
        const int i = idx / nrhs, c = r + (idx - i * nrhs);
        W[i * ld + c] = fma(-W[i * ld + k], W[k * ld + c], W[i * ld + c]);
      }
    __syncthreads();
  }
  // T = U^-1 D^(1/2) below the diagonal: thread j owns column j (row j of W) and reads only U and its own row -- no barrier
  if (ok && tg < r) {
    const int j = tg;
    for (int i = j - 1; i >= 0; --i) {
      const double* __restrict__ Ui = W + i * ld;
      double dot = 0.0;
      for (int l = i + 1; l < j; ++l) dot = fma(Ui[l], W[j * ld + l], dot);
      dot = fma(Ui[j], dv[j], dot);
      W[j * ld + i] = -(dot * refined_rcp(Ui[i]));
    }
  }
  __syncthreads();
  return info;
}

// doubles of LDS mom_solve needs for a record of m variables: W (m x ((m + 1) | 1)) and the m reciprocals of the pivots
__host__ __device__ inline size_t mom_lds_doubles(int m) { return (size_t)m * ((m + 1) | 1) + (size_t)m; }

}  // namespace pgbp

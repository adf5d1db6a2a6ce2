// Device pieces shared by the kernels that sweep the node families of a linear-Gaussian model: the factor fill and its shift
// correction (pgbp_lgfill.hip, pgbp_shift.hip: mask_rank, lg_coefs) and the four sweeps over calibrated beliefs --
// pgbp_grad.hip and pgbp_edge.hip (all of it but lds_cholesky and fam_stage_plain; their common body is fam_score_T +
// fam_score_gv), pgbp_loo.hip and pgbp_impute.hip (mask_rank, lg_coefs, lds_cholesky, LgSite, fam_blocks, fam_cov,
// fam_stage_plain).  Notation of pgbp_lgfill.hip and pgbp_grad.hip.  Arithmetic contract: every sum in a fixed index order,
// contraction off, so that a kernel's bytes do not depend on which of these it inlines.
#pragma once
#include <hip/hip_runtime.h>

#include "pgbp_bs16.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_mom_dev.hpp"
#include "pgbp_noise_dev.hpp"
#include "pgbp_shift_dev.hpp"

namespace pgbp {

// rank of trait t inside a node's block = number of in-scope traits before it
__device__ __forceinline__ int mask_rank(unsigned long long mask, int t) { return __popcll(mask & ((1ull << t) - 1ull)); }

// Edge coefficients of a parent edge (length t, inheritance gam) under the model; a = exp(-alpha t).
// FILL: the factor fill and its shift correction are built with the compiler's contraction, under which 1 - a^2 is ONE fused
// operation wherever this is inlined; the sweeps over calibrated beliefs round a^2 first.  Both are written out here (an ulp
// of vc under the OU model apart), so that every caller keeps the bytes it has always returned.
template <bool FILL>
__device__ __forceinline__ void lg_coefs(int model, double alpha, double t, double gam, double& qc, double& vc, double& wc) {
#pragma clang fp contract(off)
  if (model == PGBP_LG_OU) {
    const double a = exp(-alpha * t);
    qc = gam * a;
    vc = gam * gam * (FILL ? fma(-a, a, 1.0) : 1.0 - a * a);
    wc = gam * (1.0 - a);
  } else {
    qc = gam;
    vc = gam * gam * t;
    wc = 0.0;
  }
}

// their derivatives in alpha
__device__ __forceinline__ void lg_coefs_dalpha(int model, double alpha, double t, double gam, double& dqc, double& dvc,
                                                double& dwc) {
#pragma clang fp contract(off)
  if (model == PGBP_LG_OU) {
    const double a = exp(-alpha * t);
    dqc = -(gam * t) * a;
    dvc = 2.0 * (gam * gam) * t * (a * a);
    dwc = (gam * t) * a;
  } else {
    dqc = dvc = dwc = 0.0;
  }
}

// their partial derivatives in the length (q_t, v_t, w_t) and in the inheritance (q_g, v_g, w_g)
struct LgEdgeDerivs {
  double q_t, v_t, w_t, q_g, v_g, w_g;
};
__device__ __forceinline__ LgEdgeDerivs lg_coefs_dedge(int model, double alpha, double t, double gam) {
#pragma clang fp contract(off)
  LgEdgeDerivs c;
  if (model == PGBP_LG_OU) {
    const double a = exp(-alpha * t);
    c.q_t = -(gam * alpha) * a;
    c.v_t = 2.0 * (gam * gam) * alpha * (a * a);
    c.w_t = (gam * alpha) * a;
    c.q_g = a;
    c.v_g = 2.0 * gam * (1.0 - a * a);
    c.w_g = 1.0 - a;
  } else {
    c.q_t = 0.0;
    c.v_t = gam * gam;
    c.w_t = 0.0;
    c.q_g = 1.0;
    c.v_g = 2.0 * gam * t;
    c.w_g = 0.0;
  }
  return c;
}

// Gauss-Jordan on the mo x 2mo system [V | I] (row stride ld) in LDS by NT threads: the right half becomes V^-1; false when
// a pivot is not positive (uniform: every thread reads the same pivot)
template <int NT>
__device__ __forceinline__ bool spd_invert(double* __restrict__ A, int mo, int ld, int t) {
#pragma clang fp contract(off)
  const int nc = 2 * mo;
  for (int k = 0; k < mo; ++k) {
    __syncthreads();
    const double d = A[k * ld + k];
    if (!(d > 0.0)) return false;
    const double rd = 1.0 / d;
    __syncthreads();
    for (int j = k + 1 + t; j < nc; j += NT) A[k * ld + j] = A[k * ld + j] * rd;
    __syncthreads();
    const int ncol = nc - (k + 1);
    for (int idx = t; idx < (mo - 1) * ncol; idx += NT) {
      int i = idx / ncol;
      const int j = k + 1 + (idx - i * ncol);
      if (i >= k) ++i;
      A[i * ld + j] = A[i * ld + j] - A[i * ld + k] * A[k * ld + j];
    }
  }
  __syncthreads();
  return true;
}

// A matrix formed by cancellation against the beliefs (D = V - S of pgbp_loo.hip) carries an error of about 2^-52 |V| in its
// entries.  A pivot of its factorisation that is not above 2^-40 of V's diagonal entry is rounding noise (the cavity variance
// is more than 2^40 times the tip's own): D is then reported as not positive definite.
constexpr double kLooPivotFloor = 0x1p-40;

// Left-looking Cholesky of the lower triangle of the leading n x n block of A (row stride ld) in LDS by NT threads: L(i, j),
// i > j, in place; the diagonal of L in dl (A's diagonal is left as it was).  floor: null (the pivot must exceed 0), or per
// pivot the value it must exceed (floor[j * (ld + 1)] * kLooPivotFloor).  false when a pivot fails (uniform: every thread
// computes the same pivot).  Every column ends behind a barrier; the caller's barrier stands before the first.
template <int NT>
__device__ __forceinline__ bool lds_cholesky(double* __restrict__ A, int n, int ld, double* __restrict__ dl,
                                             const double* __restrict__ floor, int t) {
#pragma clang fp contract(off)
  for (int j = 0; j < n; ++j) {
    double d = A[j * ld + j];
    for (int k = 0; k < j; ++k) d = fma(-A[j * ld + k], A[j * ld + k], d);
    const double lim = floor ? floor[j * ld + j] * kLooPivotFloor : 0.0;
    if (!(d > lim)) return false;
    const double l = sqrt(d);
    for (int i = j + 1 + t; i < n; i += NT) {
      double s = A[i * ld + j];
      for (int k = 0; k < j; ++k) s = fma(-A[i * ld + k], A[j * ld + k], s);
      A[i * ld + j] = s / l;
    }
    if (t == 0) dl[j] = l;
    __syncthreads();
  }
  return true;
}

// lds_cholesky's arithmetic with a skip (pgbp_scan.hip): index j is KEPT when its pivot, given the kept indices before it,
// exceeds min_info * lim[j * lstride]; otherwise it is dropped from the system -- its row and column take no part in any
// later pivot or column.  L(i, j) in place below the diagonal for every kept j (all i > j, kept or not: a dropped row is
// never read), the diagonal of L in dl at the kept indices; A's diagonal and upper triangle are left as they were.  Returns
// the mask of kept indices (uniform: every thread computes the same pivots; a pivot that is NaN is dropped).  Every kept
// column ends behind a barrier; the caller's barrier stands before the first.
template <int NT>
__device__ __forceinline__ unsigned long long lds_cholesky_skip(double* __restrict__ A, int n, int ld, double* __restrict__ dl,
                                                                const double* __restrict__ lim, int lstride, double min_info,
                                                                int t) {
#pragma clang fp contract(off)
  unsigned long long kept = 0ull;
  for (int j = 0; j < n; ++j) {
    double d = A[j * ld + j];
    for (int k = 0; k < j; ++k)
      if ((kept >> k) & 1ull) d = fma(-A[j * ld + k], A[j * ld + k], d);
    if (!(d > min_info * lim[j * lstride])) continue;
    const double l = sqrt(d);
    for (int i = j + 1 + t; i < n; i += NT) {
      double s = A[i * ld + j];
      for (int k = 0; k < j; ++k)
        if ((kept >> k) & 1ull) s = fma(-A[i * ld + k], A[j * ld + k], s);
      A[i * ld + j] = s / l;
    }
    if (t == 0) dl[j] = l;
    kept |= 1ull << j;
    __syncthreads();
  }
  return kept;
}

// the parameters of site `as` (absolute): theta is null and alpha 0 unless the model is OU
struct LgSite {
  const double *R, *mu, *theta;
  double alpha;
};
__device__ __forceinline__ LgSite lg_site(const LgParams& M, int nr, int p, int64_t as) {
  const bool ou = M.model == PGBP_LG_OU;
  const int64_t ps = M.per_site ? as : 0;
  return LgSite{M.R + ps * nr * p * p, M.mu + ps * p, (ou && M.theta) ? M.theta + ps * p : nullptr, ou ? M.alpha[ps] : 0.0};
}

// A packed (BS16) record copied to `stage` in the plain layout, the upper triangle mirrored (what a plain record gives
// mom_solve: PDMat(Symmetric(J))) -- a packed record keeps both triangles of its diagonal 2 x 2 blocks, equal to the last bit
// only: read this way the two layouts give the same bytes.  (mom_solve's first barrier publishes the copy; its loads end
// behind a barrier as well.)
template <int NT>
__device__ __forceinline__ void fam_stage_plain(const double* __restrict__ rec, int m, int fp, double* __restrict__ stage, int t) {
  for (int idx = t; idx < m * m; idx += NT) {
    const int j = idx / m, i = idx - j * m;
    stage[idx] = rec[bs16::J_off(m, i < j ? i : j, i < j ? j : i, fp)];
  }
  for (int i = t; i < m; i += NT) stage[m * m + i] = rec[bs16::h_off(m, i, fp)];
}

// Where the listed traits tidx[0 .. n) of each block sit in the cluster, vi[a * p + i] (-1: a constant), and their posterior
// mean (column m of mom_solve's W) or constant value, xm[a * p + i].  Blocks a < child are the child (at most one: its mask
// is O, its constant the family's data row), block a >= child is parent a - child (its constant: the fixed root's mu);
// ipos[a]: the block's position in the cluster, negative: a constant.
template <int NT>
__device__ __forceinline__ void fam_blocks(const LgStatic& F, int f, int64_t as, const double* __restrict__ mu, int child,
                                           int n_blocks, unsigned long long O, const int* __restrict__ ipos,
                                           const int* __restrict__ tidx, int n, const double* __restrict__ W, int ld, int m,
                                           int* __restrict__ vi, double* __restrict__ xm, int t) {
  const int p = F.p, K = F.K;
  const unsigned long long full = p >= 64 ? ~0ull : ((1ull << p) - 1ull);
  for (int idx = t; idx < n_blocks * n; idx += NT) {
    const int a = idx / n, i = idx - a * n, tr = tidx[i];
    const int pa = ipos[a];
    if (pa >= 0) {
      const unsigned long long ma = a < child ? O : (F.parent_mask ? F.parent_mask[(size_t)f * K + a - child] : full);
      const int v = pa + mask_rank(ma, tr);
      vi[a * p + i] = v;
      xm[a * p + i] = W[v * ld + m];
    } else {
      vi[a * p + i] = -1;
      xm[a * p + i] = a < child ? F.data[(as * F.n_rows + F.data_row[f]) * p + tr] : mu[tr];   // tip / fixed root
    }
  }
}

// sum_a sum_b c(a) c(b) Sigma(v_a(i), v_b(j)) over the blocks in scope, Sigma as mom_solve leaves it (the lower triangle of W)
template <class C>
__device__ __forceinline__ double fam_cov(const double* __restrict__ W, int ld, const int* __restrict__ vi, int p, C c,
                                          int n_blocks, int i, int j) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int a = 0; a < n_blocks; ++a) {
    const int va = vi[a * p + i];
    if (va < 0) continue;
    for (int b = 0; b < n_blocks; ++b) {
      const int vb = vi[b * p + j];
      if (vb < 0) continue;
      s = s + c(a) * c(b) * (va >= vb ? W[va * ld + vb] : W[vb * ld + va]);
    }
  }
  return s;
}

// ---- the score of a family under its cluster's belief (pgbp_grad.hip, pgbp_edge.hip)
// LDS beyond mom_solve's [W | dv]: the arrays below, `rows` rows of K edge coefficients (rows 0 .. 2: qc, vc, wc; the kernel's
// own derivative rows behind them), `extra` doubles of the kernel's own, then the ints
struct FamLds {
  double *W, *dv;
  double* A;      // [V_OO | I] -> [.. | j], mo x ldv
  double* Mx;     // M = Cov(r) + e e', then G_V  (mo x mo)
  double* Tx;     // j M
  double* ev;     // e
  double* ge;     // g_w = j e
  double* xm;     // [a][i]: posterior mean of block a (or its constant value) at kept trait i
  double* cf;     // [rows][K]
  double* extra;
  int* ipos;      // [K + 1]: the child's position in the cluster, then the parents'
  int* oidx;      // the kept traits
  int* vi;        // [a][i]: the variable's index in the cluster, -1: a constant
};
__host__ __device__ inline int fam_ldv(int p) { return (2 * p) | 1; }
__host__ __device__ inline size_t fam_score_doubles(int p, int K, int rows, size_t extra) {
  const size_t n = (size_t)p * fam_ldv(p) + 2 * (size_t)p * p + 2 * (size_t)p + (size_t)(K + 1) * p + (size_t)rows * K + extra;
  return (n + 1) & ~(size_t)1;
}
__host__ __device__ inline size_t fam_score_lds_bytes(int max_m, int p, int K, int rows, size_t extra) {
  return sizeof(double) * (mom_lds_doubles(max_m) + fam_score_doubles(p, K, rows, extra)) +
         sizeof(int) * ((size_t)(K + 1) + (size_t)p + (size_t)(K + 1) * p);
}
__device__ __forceinline__ FamLds fam_carve(double* lds, int m, int p, int K, int rows, size_t extra) {
  FamLds L;
  L.W = lds;
  L.dv = lds + m * ((m + 1) | 1);
  L.A = lds + mom_lds_doubles(m);
  L.Mx = L.A + p * fam_ldv(p);
  L.Tx = L.Mx + p * p;
  L.ev = L.Tx + p * p;
  L.ge = L.ev + p;
  L.xm = L.ge + p;
  L.cf = L.xm + (K + 1) * p;
  L.extra = L.cf + rows * K;
  L.ipos = reinterpret_cast<int*>(L.A + fam_score_doubles(p, K, rows, extra));
  L.oidx = L.ipos + (K + 1);
  L.vi = L.oidx + p;
  return L;
}

// c_0 = 1 (child), c_k = -qc_k
__device__ __forceinline__ double fam_c(const double* __restrict__ cf, int a) { return a == 0 ? 1.0 : -cf[a - 1]; }
// j(i, k) in the right half of A: the upper triangle mirrored, exactly symmetric (as the fill reads it)
__device__ __forceinline__ double fam_j(const double* __restrict__ A, int ldv, int mo, int i, int k) {
  return i <= k ? A[i * ldv + mo + k] : A[k * ldv + mo + i];
}

// From the moments of the family's cluster (mom_solve has run, or nothing is in scope and a barrier stands behind the previous
// site's reads) to T = j M: fills cf rows 0 .. 2, ipos, oidx, vi, xm, ev = e, Mx = M, the right half of A = j, Tx = j M,
// ge = g_w.  A noisy tip family (Nz: pgbp_lg_set_tip_noise) has V_OO + E_OO in place of V_OO, and so j = (V_OO + E_OO)^-1
// in everything formed from it.  Op: painted optima (pgbp_lg_set_optima; regime null: none), whose d_opt w gains.
// false when that variance is not positive definite.  No barrier stands behind the writes of Tx and ge:
// fam_score_gv begins with it.
template <int NT, bool OPT>
__device__ __forceinline__ bool fam_score_T_opt(const FamLds& L, const LgStatic& F, const LgParams& M, const LgShifts& Sh,
                                                const LgOptima& Op, const LgNoise& Nz, const LgSite& S, int f, int m, unsigned long long O, int64_t as, int t) {
#pragma clang fp contract(off)
  const int p = F.p, K = F.K, np = F.n_parents[f], nn = np + 1, mo = __popcll(O);
  const int ld = (m + 1) | 1, ldv = fam_ldv(p);
  double* __restrict__ W = L.W;
  double* __restrict__ A = L.A;
  double* __restrict__ Mx = L.Mx;
  double* __restrict__ cf = L.cf;
  int* __restrict__ oidx = L.oidx;
  // coefficients, positions, kept traits
  for (int a = t; a <= np; a += NT) {
    if (a == 0) {
      L.ipos[0] = F.child_pos[f];
    } else {
      const int k = a - 1;
      lg_coefs<false>(M.model, S.alpha, F.length[(size_t)f * K + k], F.gamma[(size_t)f * K + k], cf[k], cf[K + k], cf[2 * K + k]);
      L.ipos[a] = F.parent_pos[(size_t)f * K + k];
    }
  }
  for (int tr = t; tr < p; tr += NT)
    if ((O >> tr) & 1ull) oidx[mask_rank(O, tr)] = tr;
  __syncthreads();
  fam_blocks<NT>(F, f, as, S.mu, 1, nn, O, L.ipos, oidx, mo, W, ld, m, L.vi, L.xm, t);
  // V_OO and the identity
  const int sn = lg_noise_slot(Nz, f);
  for (int idx = t; idx < mo * mo; idx += NT) {
    const int j = idx / mo, i = idx - j * mo;
    const int e = oidx[i] + oidx[j] * p;
    double v = 0.0;
    if (np == 0) {
      v = S.R[(int64_t)F.color[(size_t)f * K] * p * p + e];
    } else {
      for (int k = 0; k < np; ++k) v = v + cf[K + k] * S.R[(int64_t)F.color[(size_t)f * K + k] * p * p + e];
    }
    if (sn >= 0) v = v + lg_noise_E(Nz, sn, oidx[i], oidx[j], p, as);   // a noisy tip: V_OO + E_OO
    A[i * ldv + j] = v;
    A[i * ldv + mo + j] = (i == j) ? 1.0 : 0.0;
  }
  __syncthreads();
  // e = E[r]
  for (int i = t; i < mo; i += NT) {
    const int tr = oidx[i];
    double e = 0.0;
    for (int a = 0; a < nn; ++a) e = e + fam_c(cf, a) * L.xm[a * p + i];
    double w = 0.0;
    if (np == 0) {
      w = S.mu[tr];
    } else if (S.theta) {
      for (int k = 0; k < np; ++k) w = w + cf[2 * K + k] * S.theta[tr];
    }
    if (Sh.slot) w = w + lg_shift_d(Sh, F.gamma, f, K, np, tr, p, as);   // a shift of the mean on a parent edge
    if constexpr (OPT) {   // painted optima
      if (Op.regime) w = w + lg_optima_d(Op, S.theta, S.alpha, F.length, F.gamma, f, K, np, tr, p, as, 0);
    }
    L.ev[i] = e - w;
  }
  __syncthreads();
  // M = Cov(r) + e e'
  for (int idx = t; idx < mo * mo; idx += NT) {
    const int j = idx / mo, i = idx - j * mo;
    const double s = fam_cov(W, ld, L.vi, p, [&](int a) -> double { return fam_c(cf, a); }, nn, i, j);
    Mx[i * mo + j] = s + L.ev[i] * L.ev[j];
  }
  if (!spd_invert<NT>(A, mo, ldv, t)) return false;   // (the fill made this cluster's g NaN)
  for (int idx = t; idx < mo * mo; idx += NT) {
    const int k = idx / mo, i = idx - k * mo;
    double s = 0.0;
    for (int l = 0; l < mo; ++l) s = s + fam_j(A, ldv, mo, i, l) * Mx[l * mo + k];
    L.Tx[i * mo + k] = s;
  }
  for (int i = t; i < mo; i += NT) {
    double s = 0.0;
    for (int l = 0; l < mo; ++l) s = s + fam_j(A, ldv, mo, i, l) * L.ev[l];
    L.ge[i] = s;
  }
  return true;
}

// the body without painted optima (pgbp_edge.hip, pgbp_scan.hip: they refuse while optima are in force)
template <int NT>
__device__ __forceinline__ bool fam_score_T(const FamLds& L, const LgStatic& F, const LgParams& M, const LgShifts& Sh,
                                            const LgNoise& Nz, const LgSite& S, int f, int m, unsigned long long O, int64_t as, int t) {
  return fam_score_T_opt<NT, false>(L, F, M, Sh, LgOptima{}, Nz, S, f, m, O, as, t);
}

// G_V = (j M j - j) / 2 (upper triangle computed, mirrored) over M in Mx, which T = j M has consumed; o: null, or the p x p
// block of global memory that receives G_V at the kept traits as well.  Begins with the barrier behind fam_score_T's writes
// (and whatever the caller wrote since), ends without one.
template <int NT>
__device__ __forceinline__ void fam_score_gv(const FamLds& L, int p, int mo, double* __restrict__ o, int t) {
#pragma clang fp contract(off)
  const int ldv = fam_ldv(p);
  __syncthreads();
  for (int idx = t; idx < mo * mo; idx += NT) {
    const int k = idx / mo, i = idx - k * mo;
    if (i > k) continue;
    double s = 0.0;
    for (int l = 0; l < mo; ++l) s = s + L.Tx[i * mo + l] * fam_j(L.A, ldv, mo, l, k);
    const double g = 0.5 * (s - fam_j(L.A, ldv, mo, i, k));
    if (o) {
      o[L.oidx[i] + L.oidx[k] * p] = g;
      o[L.oidx[k] + L.oidx[i] * p] = g;
    }
    L.Mx[i * mo + k] = g;
    L.Mx[k * mo + i] = g;
  }
}

}  // namespace pgbp

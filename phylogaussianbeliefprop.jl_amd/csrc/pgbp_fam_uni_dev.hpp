// Device pieces shared by the three lanes-are-sites family sweeps of a univariate batch (pgbp_fam_uni.hip: the scan, the edge
// derivatives and the leave-one-out predictions of a thread-per-site engine): p = 1, every belief of at most 2 variables.  A
// thread holds one site and walks families; per (family, site) everything is closed form.  Written once here:
//   * the moments of a cluster of 0, 1 or 2 variables, Sigma = J^-1 (PDMat(Symmetric(J)): the upper triangle), m = Sigma h;
//   * the one pass over a family's blocks -- r = sum_a c_a x_a - w with c_0 = 1 (child), c_k = -qc_k, so that
//     r = u_0 x_0 + u_1 x_1 + const - w with u_v the sum of the c_a that sit at variable v -- which gives u, the constant, V
//     (with the tip noise E_f) and w (with the shifts), and per parent the coefficients and the parent's mean;
//   * what all three sweeps form from them: e = E[r], Sigma u, C = u' Sigma u, j = 1 / V, g_w = j e.
// Notation and frame of pgbp_grad_uni.hip, which takes the moments from here and keeps its own pass over the parents: it adds
// the alpha-derivative sums in the same loop, and a second pass would evaluate lg_coefs twice per edge.  Arithmetic contract
// of pgbp_fam_dev.hpp: every sum in a fixed index order, contraction off.
#pragma once
#include <hip/hip_runtime.h>

#include "pgbp_fam_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_sitemiss_dev.hpp"

namespace pgbp {

constexpr int kFamUniBlock = 64;   // families per thread (grid.y = blocks of them)
constexpr int kFamUniNoInfo = 0x7fffffff;

// what every lanes-are-sites kernel takes of the engine and of the call (sites_args of pgbp_sites_host.hpp fills it;
// grad_uni_family takes its members as a flat list)
struct SitesArgs {
  const double* pool;
  int64_t stride;
  const int64_t* off;
  const int32_t* bdim;
  int site0, n_sites;
  int64_t row;                  // the row length of the scratch (the chunk)
  const int32_t* fam_cluster;   // the family sweeps only: the cluster of a family, and the row length of the site-minor data
  int64_t data_row_len;
};

// element t of the belief at offset `off` for site `as`, in the layout the pool is in (UniView of pgbp_kernels.hpp)
template <bool SM>
__device__ __forceinline__ double fam_uni_ld(const double* __restrict__ pool, int64_t stride, int64_t off, int t, int64_t as) {
  return SM ? pool[(off + t) * stride + as] : pool[as * stride + off + t];
}

// Sigma and m of a cluster.  st: 0, or what mom_solve (pgbp_mom_dev.hpp) returns for such a record -- -1: the constant belief
// (J = 0, h = 0, and a cluster without variables), k + 1: pivot k is not positive.  ok = (st == 0).
struct FamUniMom {
  double S00, S01, S11, m0, m1;
  int st;
  bool ok;
};

template <bool SM>
__device__ __forceinline__ FamUniMom fam_uni_moments(const double* __restrict__ pool, int64_t stride, int64_t o, int m,
                                                     int64_t as) {
#pragma clang fp contract(off)
  FamUniMom q{0.0, 0.0, 0.0, 0.0, 0.0, 0, true};
  if (m == 1) {
    const double J = fam_uni_ld<SM>(pool, stride, o, 0, as), h = fam_uni_ld<SM>(pool, stride, o, 1, as);
    q.st = J > 0.0 ? 0 : ((J == 0.0 && h == 0.0) ? -1 : 1);
    q.S00 = 1.0 / J;
    q.m0 = h / J;
  } else if (m == 2) {
    const double a = fam_uni_ld<SM>(pool, stride, o, 0, as), b = fam_uni_ld<SM>(pool, stride, o, 2, as);
    const double d = fam_uni_ld<SM>(pool, stride, o, 3, as);
    const double h0 = fam_uni_ld<SM>(pool, stride, o, 4, as), h1 = fam_uni_ld<SM>(pool, stride, o, 5, as);
    const double ba = b / a, sc = d - ba * b;   // the Schur complement of the first pivot
    if (a > 0.0) q.st = sc > 0.0 ? 0 : 2;
    else q.st = (a == 0.0 && b == 0.0 && d == 0.0 && h0 == 0.0 && h1 == 0.0 && fam_uni_ld<SM>(pool, stride, o, 1, as) == 0.0) ? -1 : 1;
    q.S11 = 1.0 / sc;
    q.S01 = -(ba * q.S11);
    q.S00 = 1.0 / a + ba * ba * q.S11;
    q.m1 = (h1 - ba * h0) / sc;
    q.m0 = (h0 - b * q.m1) / a;
  } else {
    q.st = -1;   // (a variable in scope of a cluster without variables: no moments)
  }
  q.ok = q.st == 0;
  return q;
}

// parent edge k of family f: its coefficients, its colour, where the parent sits (pk: 0 / 1, negative: the fixed root) and the
// parent's mean x_k (mu of the fixed root), and (Sigma u)[v_k] is the caller's to pick by pk
struct FamUniParent {
  double qc, vc, wc, xk;
  int col, pk;
};
__device__ __forceinline__ FamUniParent fam_uni_parent(const LgStatic& F, const LgParams& M, const LgSite& S, const FamUniMom& q,
                                                       int f, int k, double mu) {
  FamUniParent P;
  const size_t i = (size_t)f * F.K + k;
  lg_coefs<false>(M.model, S.alpha, F.length[i], F.gamma[i], P.qc, P.vc, P.wc);
  P.col = F.color[i];
  P.pk = F.parent_pos[i];
  P.xk = P.pk == 0 ? q.m0 : (P.pk == 1 ? q.m1 : mu);
  return P;
}

// A family at a site.  skip: the factor fill skips it (child_mask == 0, or a tip the per-site mask says is not observed at this
// site: masked), or it is the root-prior family of a fixed root, which has no factor -- nothing else is set then.  y: the tip's
// data value (0 when the child is not a tip with data).
struct FamUni {
  int np, cpos, c, sn;
  bool skip, masked;
  FamUniMom q;
  double u0, u1, cst, V, w, y;
  // what the sweeps form from them
  double e, su0, su1, C, j, gw;
};

template <bool SM>
__device__ __forceinline__ FamUni fam_uni_family(const double* __restrict__ pool, int64_t stride, const int64_t* __restrict__ off,
                                                 const int32_t* __restrict__ bdim, const LgStatic& F, const LgParams& M,
                                                 const LgShifts& Sh, const LgNoise& Nz, const LgSiteMiss& Ms, const LgSite& S,
                                                 const int32_t* __restrict__ fam_cluster, int f, int64_t data_row_len, int64_t as) {
#pragma clang fp contract(off)
  FamUni A;
  const int K = F.K;
  const int np = F.n_parents[f], cpos = F.child_pos[f];
  A.np = np;
  A.cpos = cpos;
  A.c = fam_cluster[f];
  A.sn = -1;
  A.masked = lg_site_masked_family(Ms, F, f, as);
  A.skip = (F.child_mask && !(F.child_mask[f] & 1ull)) || (np == 0 && cpos < 0) || A.masked;
  A.q = FamUniMom{0.0, 0.0, 0.0, 0.0, 0.0, 0, true};
  A.u0 = A.u1 = A.cst = A.V = A.w = A.y = 0.0;
  A.e = A.su0 = A.su1 = A.C = A.j = A.gw = 0.0;
  if (A.skip) return A;
  bool any_scope = cpos >= 0;
  for (int k = 0; k < np; ++k) any_scope |= F.parent_pos[(size_t)f * K + k] >= 0;
  if (any_scope) A.q = fam_uni_moments<SM>(pool, stride, off[A.c], bdim[A.c], as);
  const double mu = S.mu[0], theta = S.theta ? S.theta[0] : 0.0;
  double u0 = 0.0, u1 = 0.0, cst = 0.0, V = 0.0, w = 0.0;
  if (cpos == 0) u0 = 1.0;
  else if (cpos == 1) u1 = 1.0;
  else if (F.data_row[f] >= 0) {   // a tip: its data row, [row][site] where the engine keeps that copy
    A.y = F.data_sm ? F.data_sm[(int64_t)F.data_row[f] * data_row_len + as] : F.data[as * F.n_rows + F.data_row[f]];
    cst = A.y;
  }
  if (np == 0) {
    V = S.R[F.color[(size_t)f * K]];
    w = mu;
  } else {
    for (int k = 0; k < np; ++k) {
      const FamUniParent P = fam_uni_parent(F, M, S, A.q, f, k, mu);
      V = V + P.vc * S.R[P.col];
      if (S.theta) w = w + P.wc * theta;
      if (P.pk == 0) u0 = u0 - P.qc;
      else if (P.pk == 1) u1 = u1 - P.qc;
      else cst = cst - P.qc * mu;   // the fixed root
    }
    if (Sh.slot) w = w + lg_shift_d(Sh, F.gamma, f, K, np, 0, 1, as);   // a shift of the mean on a parent edge
  }
  A.sn = lg_noise_slot(Nz, f);
  if (A.sn >= 0) V = V + lg_noise_E(Nz, A.sn, 0, 0, 1, as);   // a noisy tip: V + E
  A.u0 = u0;
  A.u1 = u1;
  A.cst = cst;
  A.V = V;
  A.w = w;
  A.e = (u0 * A.q.m0 + u1 * A.q.m1 + cst) - w;
  A.su0 = A.q.S00 * u0 + A.q.S01 * u1;   // Sigma u
  A.su1 = A.q.S01 * u0 + A.q.S11 * u1;
  A.C = u0 * A.su0 + u1 * A.su1;         // Cov(r | data) = u' Sigma u
  A.j = 1.0 / V;
  A.gw = A.j * A.e;
  return A;
}

}  // namespace pgbp

// Per-site missing tips of a univariate batch in the factor fill (pgbp_lg_set_site_missing of include/pgbp.h).
//
// At p = 1 a tip that is not observed at a site is a family the fill skips there -- its factor is 1 -- with no change of scopes
// or of the cluster graph.  The fill kernels, the shift and the noise corrections are left alone and write every record as if
// every tip were observed (reading the 0.0 the setter stored at the masked entries); this kernel runs after them whenever a
// mask is set.  Lanes are sites: a workgroup is 256 consecutive sites, grid.y runs over the clusters that hold a tip family
// masked at some site (the setter's list).  A thread whose site masks no family of its cluster stores nothing: that record
// keeps the fill's bytes.  A thread whose site does mask one RECOMPUTES the record from the family table without the masked
// families -- the closed forms of lg_fill_uni_sm_kernel with the shifts and the tip noise in force,
//     V = sum_k vc_k R[colour_k] (+ E_f),  z = w + d - sum over the fixed nodes of c_a y_a,  j = 1 / V,
//     J_ab += c_a c_b j,  h_a += c_a j z,  g += -(log 2pi + log V + z j z) / 2
// -- and writes it to the pool and, when given, to the factor pool.  Recomputed, not subtracted: a cluster whose only family is
// the masked tip holds exactly +0.0 in every entry (sums that start from 0.0 and gain nothing), nothing depends on the stored
// placeholder, and there is no cancellation error in proportion to the removed precision.  One writer per record, no atomics,
// no barrier, contraction off, every sum in table order: the same bytes on every call, whatever other sites are in the launch.
#include <hip/hip_runtime.h>

#include "pgbp_fam_dev.hpp"
#include "pgbp_internal.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_noise_dev.hpp"
#include "pgbp_shift_dev.hpp"
#include "pgbp_sitemiss_dev.hpp"

namespace pgbp {

#define PGBP_SITEMISS_LOG2PI 1.8378770664093454835606594728112

template <bool SM>
__global__ __launch_bounds__(256) void sitemiss_fill_kernel(LgStatic F, LgParams M, LgShifts Sh, LgOptima Op, LgNoise Nz, LgSiteMiss Ms, LgCladeShifts Cs,
                                                            const int32_t* __restrict__ mcl, double* __restrict__ pool,
                                                            int64_t stride, double* __restrict__ fpool, int64_t fstride,
                                                            const int64_t* __restrict__ off, const int32_t* __restrict__ dim,
                                                            int n_sites) {
#pragma clang fp contract(off)
  const int site = blockIdx.x * 256 + threadIdx.x;
  if (site >= n_sites) return;   // (no barrier follows, and no other lane's store is this lane's to make)
  const int c = mcl[blockIdx.y];
  const int K = F.K;
  const int f_begin = F.cl_off[c], f_end = F.cl_off[c + 1];
  bool any = false;
  for (int fi = f_begin; fi < f_end; ++fi) any |= lg_site_masked_family(Ms, F, F.cl_fam[fi], site);
  if (!any) return;              // this (cluster, site) keeps the fill's bytes
  const LgSite S = lg_site(M, F.n_rates, 1, site);
  const double mu = S.mu[0], theta = S.theta ? S.theta[0] : 0.0;
  const int64_t drow = sm_row(n_sites);
  const int m = dim[c];
  double J00 = 0.0, J10 = 0.0, J01 = 0.0, J11 = 0.0, h0 = 0.0, h1 = 0.0, g = 0.0;
  for (int fi = f_begin; fi < f_end; ++fi) {
    const int f = F.cl_fam[fi];
    const int np = F.n_parents[f], cpos = F.child_pos[f];
    if (F.child_mask && !(F.child_mask[f] & 1ull)) continue;   // missing / out of scope below at every site: factor = 1
    if (lg_site_masked_family(Ms, F, f, site)) continue;       // not observed at this site: factor = 1
    double V = 0.0, z = 0.0;
    if (np == 0) {
      V = S.R[F.color[(int64_t)f * K]];
      z = mu;
    } else {
      for (int k = 0; k < np; ++k) {
        double qc, vc, wc;
        lg_coefs<true>(M.model, S.alpha, F.length[(int64_t)f * K + k], F.gamma[(int64_t)f * K + k], qc, vc, wc);
        V = V + vc * S.R[F.color[(int64_t)f * K + k]];
        z = z + wc * theta;
        if (F.parent_pos[(int64_t)f * K + k] < 0) z = z + qc * mu;   // the fixed root
      }
      // a shift of the mean on a parent edge, a painted optimum
      z = z + lg_disp_d(Sh, Op, &theta, S.alpha, F.length, F.gamma, f, K, np, 0, 1, site, drow);
      if (Cs.family) {   // this site's clade shifts of the optimum
        bool any;
        z = z + lg_clade_d(Cs, S.alpha, F.length, F.gamma, f, K, np, site, any);
      }
      if (cpos < 0) z = z - F.data_sm[(int64_t)F.data_row[f] * drow + site];   // a tip: its value
      const int sn = lg_noise_slot(Nz, f);
      if (sn >= 0) V = V + lg_noise_E(Nz, sn, 0, 0, 1, site);        // a noisy tip: V + E
    }
    const double j = 1.0 / V;
    g = g + -0.5 * ((PGBP_SITEMISS_LOG2PI + log(V)) + (z * j) * z);
    if (!(V > 0.0)) g = NAN;
    for (int a = 0; a <= np; ++a) {   // in-scope nodes: at most two
      const int pa = a == 0 ? cpos : F.parent_pos[(int64_t)f * K + a - 1];
      if (pa < 0) continue;
      double ca = 1.0, vc, wc;
      if (a > 0) {
        lg_coefs<true>(M.model, S.alpha, F.length[(int64_t)f * K + a - 1], F.gamma[(int64_t)f * K + a - 1], ca, vc, wc);
        ca = -ca;
      }
      if (pa == 0) h0 = h0 + (ca * j) * z;
      else h1 = h1 + (ca * j) * z;
      for (int b = 0; b <= np; ++b) {
        const int pb = b == 0 ? cpos : F.parent_pos[(int64_t)f * K + b - 1];
        if (pb < 0) continue;
        double cb = 1.0;
        if (b > 0) {
          lg_coefs<true>(M.model, S.alpha, F.length[(int64_t)f * K + b - 1], F.gamma[(int64_t)f * K + b - 1], cb, vc, wc);
          cb = -cb;
        }
        const double v = (ca * cb) * j;
        if (pa == 0 && pb == 0) J00 = J00 + v;
        else if (pa == 1 && pb == 0) J10 = J10 + v;
        else if (pa == 0 && pb == 1) J01 = J01 + v;
        else J11 = J11 + v;
      }
    }
  }
  // [J (m*m) | h (m) | g] of the cluster: element t of site s at (off + t) * stride + s, or at s * stride + off + t
  double v[7];
  int len;
  if (m == 2) { v[0] = J00; v[1] = J10; v[2] = J01; v[3] = J11; v[4] = h0; v[5] = h1; v[6] = g; len = 7; }
  else if (m == 1) { v[0] = J00; v[1] = h0; v[2] = g; len = 3; }
  else { v[0] = g; len = 1; }
  const int64_t o = off[c];
  for (int t = 0; t < len; ++t) {
    if (SM) {
      pool[(o + t) * stride + site] = v[t];
      if (fpool) fpool[(o + t) * fstride + site] = v[t];
    } else {
      pool[(int64_t)site * stride + o + t] = v[t];
      if (fpool) fpool[(int64_t)site * fstride + o + t] = v[t];
    }
  }
}

// thread = (row, site): 0.0 at the masked entries of both copies of the tip data
__global__ __launch_bounds__(256) void sitemiss_zero_kernel(LgSiteMiss Ms, double* __restrict__ data, double* __restrict__ data_sm,
                                                            int n_rows, int n_sites, int64_t drow, int row0) {
  const int site = blockIdx.x * 256 + threadIdx.x, row = row0 + blockIdx.y;
  if (site >= n_sites || row >= n_rows) return;
  if (!lg_site_masked(Ms, row, site)) return;
  data[(int64_t)site * n_rows + row] = 0.0;
  if (data_sm) data_sm[(int64_t)row * drow + site] = 0.0;
}

void launch_lg_sitemiss(const LgStatic& F, const LgParams& M, const LgShifts& S, const LgOptima& Op, const LgNoise& Nz,
                        const LgSiteMiss& Ms, const LgCladeShifts& Cs,
                        const int32_t* d_mcl, int n_mcl, int sm, double* pool, int64_t stride, double* fpool, int64_t fstride,
                        const int64_t* d_off, const int32_t* d_dim, int n_sites, hipStream_t st) {
  if (n_mcl <= 0 || !Ms.words) return;
  const int gx = (n_sites + 255) / 256;
  for (int c0 = 0; c0 < n_mcl; c0 += 65535) {   // (grid.y is 16 bits wide)
    const dim3 grid(gx, n_mcl - c0 < 65535 ? n_mcl - c0 : 65535);
    if (sm)
      hipLaunchKernelGGL(sitemiss_fill_kernel<true>, grid, dim3(256), 0, st, F, M, S, Op, Nz, Ms, Cs, d_mcl + c0, pool, stride, fpool,
                         fstride, d_off, d_dim, n_sites);
    else
      hipLaunchKernelGGL(sitemiss_fill_kernel<false>, grid, dim3(256), 0, st, F, M, S, Op, Nz, Ms, Cs, d_mcl + c0, pool, stride, fpool,
                         fstride, d_off, d_dim, n_sites);
  }
}

void launch_lg_sitemiss_zero(const LgSiteMiss& Ms, double* data, double* data_sm, int n_rows, int n_sites, hipStream_t st) {
  if (!Ms.words || n_rows <= 0 || n_sites <= 0) return;
  const int gx = (n_sites + 255) / 256;
  for (int r0 = 0; r0 < n_rows; r0 += 65535) {
    const int nr = n_rows - r0 < 65535 ? n_rows - r0 : 65535;   // (grid.y is 16 bits wide)
    hipLaunchKernelGGL(sitemiss_zero_kernel, dim3(gx, nr), dim3(256), 0, st, Ms, data, data_sm, n_rows, n_sites, sm_row(n_sites), r0);
  }
}

}  // namespace pgbp

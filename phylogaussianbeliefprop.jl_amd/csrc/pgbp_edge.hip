// Derivatives of the log-likelihood in every edge length, every inheritance and a mean shift on every edge, from calibrated
// beliefs (pgbp_lg_edge_gradient of include/pgbp.h).
//
// Fisher's identity as in pgbp_grad.hip, without the sum over the families: the length t_k and the inheritance gamma_k of
// parent edge k enter the likelihood through the factor of their own family only, and there through the edge coefficients
// (qc_k, vc_k, wc_k) of lg_coefs (pgbp_lgfill.hip).  With the family quantities of pgbp_grad.hip -- O = child_mask[f],
// j = (V_OO)^-1, r = x_child - sum_k qc_k x_k - w, e = E[r], M = Cov(r) + e e', G_V = (j M j - j) / 2, g_w = j e,
// g_qk = E[r' j x_k] under the belief of the family's cluster --
//   dX_k = dvc_k/dX tr(G_V R[colour_k]_OO) + dwc_k/dX theta_O' g_w + dqc_k/dX g_qk,    X in {t, gamma},
//   BM:  dqc/dt = 0,            dvc/dt = gamma^2,               dwc/dt = 0;
//        dqc/dgamma = 1,        dvc/dgamma = 2 gamma t,         dwc/dgamma = 0;
//   OU (a = exp(-alpha t)):
//        dqc/dt = -gamma alpha a,  dvc/dt = 2 gamma^2 alpha a^2,  dwc/dt = gamma alpha a;
//        dqc/dgamma = a,           dvc/dgamma = 2 gamma (1 - a^2), dwc/dgamma = 1 - a,
// and the score of an additive displacement s of the child's conditional mean (r = ... - w - s) is g_w.
//
// One workgroup per (family, site) solves the family's cluster in LDS (mom_solve) and writes the family's own K + K + p
// numbers: no slot pool, no reduction, no floating-point atomics.  What a (family, site) writes depends on nothing else in
// the call, and every sum below is taken in a fixed index order: two calls return the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "pgbp_bs16.hpp"
#include "pgbp_devmem.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_mom_dev.hpp"
#include "pgbp_shift_dev.hpp"

namespace pgbp {

extern __shared__ double edge_lds[];

// edge coefficients of a parent edge (lg_coefs of pgbp_lgfill.hip; a = exp(-alpha t)) and their partial derivatives in the
// length (q_t, v_t, w_t) and in the inheritance (q_g, v_g, w_g)
struct EdgeCoefs {
  double qc, vc, wc, q_t, v_t, w_t, q_g, v_g, w_g;
};
__device__ __forceinline__ EdgeCoefs edge_coefs(int model, double alpha, double t, double gam) {
#pragma clang fp contract(off)
  EdgeCoefs c;
  if (model == PGBP_LG_OU) {
    const double a = exp(-alpha * t);
    c.qc = gam * a;
    c.vc = gam * gam * (1.0 - a * a);
    c.wc = gam * (1.0 - a);
    c.q_t = -(gam * alpha) * a;
    c.v_t = 2.0 * (gam * gam) * alpha * (a * a);
    c.w_t = (gam * alpha) * a;
    c.q_g = a;
    c.v_g = 2.0 * gam * (1.0 - a * a);
    c.w_g = 1.0 - a;
  } else {
    c.qc = gam;
    c.vc = gam * gam * t;
    c.wc = 0.0;
    c.q_t = 0.0;
    c.v_t = gam * gam;
    c.w_t = 0.0;
    c.q_g = 1.0;
    c.v_g = 2.0 * gam * t;
    c.w_g = 0.0;
  }
  return c;
}

__device__ __forceinline__ int edge_rank(unsigned long long mask, int t) { return __popcll(mask & ((1ull << t) - 1ull)); }

// Gauss-Jordan on the mo x 2mo system [V | I] (row stride ld) in LDS by NT threads: the right half becomes V^-1; false when
// a pivot is not positive (uniform: every thread reads the same pivot)
template <int NT>
__device__ __forceinline__ bool edge_invert(double* __restrict__ A, int mo, int ld, int t) {
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

// LDS of edge_family beyond mom_solve's: doubles, then ints
constexpr int kEdgeCoefs = 9;   // the members of EdgeCoefs, K of each
__host__ __device__ inline int edge_ldv(int p) { return (2 * p) | 1; }
__host__ __device__ inline size_t edge_extra_doubles(int p, int K) {
  return (size_t)p * edge_ldv(p) + 3 * (size_t)p * p + 4 * (size_t)p + (size_t)(K + 1) * p + (size_t)kEdgeCoefs * K;
}
__host__ __device__ inline size_t edge_extra_ints(int p, int K) { return (size_t)(K + 1) + (size_t)p + (size_t)(K + 1) * p; }

// dlen / dgam [n_sites][n_fam][K], dshift [n_sites][n_fam][p] of the sites site0 .. site0 + n_sites (any may be null)
template <int NT>
__global__ __launch_bounds__(NT) void edge_family(const double* __restrict__ pool, int64_t pool_stride,
                                                  const int64_t* __restrict__ boff, const int32_t* __restrict__ bdim, int bs,
                                                  int fp, LgStatic F, LgParams M, LgShifts Sh, const int32_t* __restrict__ fam_cluster,
                                                  int n_fam, int site0, int n_sites, double* __restrict__ dlen,
                                                  double* __restrict__ dgam, double* __restrict__ dshift,
                                                  int32_t* __restrict__ info, int info0) {
#pragma clang fp contract(off)
  const int t = threadIdx.x, f = blockIdx.x;
  const int p = F.p, K = F.K, np = F.n_parents[f], nn = np + 1;
  const int c = fam_cluster[f], m = bdim[c], ld = (m + 1) | 1;
  const unsigned long long full = p >= 64 ? ~0ull : ((1ull << p) - 1ull);
  const unsigned long long O = F.child_mask ? (F.child_mask[f] & full) : full;
  const int mo = __popcll(O);
  const int cpos = F.child_pos[f];
  // LDS: [W | dv] of mom_solve, then this kernel's arrays
  double* __restrict__ W = edge_lds;
  double* __restrict__ dv = edge_lds + m * ld;
  double* __restrict__ A = edge_lds + mom_lds_doubles(m);   // [V_OO | I] -> [.. | j], mo x ldv
  const int ldv = edge_ldv(p);
  double* __restrict__ Mx = A + p * ldv;        // M = Cov(r) + e e', then G_V  (mo x mo)
  double* __restrict__ Tx = Mx + p * p;         // j M, then the terms of tr(G_V R[colour_k])
  double* __restrict__ Px = Tx + p * p;         // the terms of g_qk = sum_il j(l, i) E[r x_k'](i, l)
  double* __restrict__ ev = Px + p * p;         // e
  double* __restrict__ ge = ev + p;             // j e
  double* __restrict__ rq = ge + p;             // row sums of Px, of Tx
  double* __restrict__ rr = rq + p;
  double* __restrict__ xm = rr + p;             // [a][i]: posterior mean of block a (or its constant value) at kept trait i
  double* __restrict__ cf = xm + (K + 1) * p;   // [kEdgeCoefs][K]
  int* __restrict__ ipos = reinterpret_cast<int*>(edge_lds + mom_lds_doubles(m) + ((edge_extra_doubles(p, K) + 1) & ~(size_t)1));
  int* __restrict__ oidx = ipos + (K + 1);
  int* __restrict__ vi = oidx + p;              // [a][i]: the variable's index in the cluster, -1: a constant
  bool any_scope = cpos >= 0;
  for (int k = 0; k < np; ++k) any_scope |= F.parent_pos[(size_t)f * K + k] >= 0;
  // families the factor fill skips (and a root-prior family of a fixed root, which has no factor)
  const bool skip = mo == 0 || (np == 0 && cpos < 0);
  const bool packed = bs && bs16::applies(m, fp);
  const bool ou = M.model == PGBP_LG_OU;
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const int64_t fo = (int64_t)site * n_fam + f;
    // every entry of the family: `edge` at its real edges, NaN where there is no edge, `shift` at the p traits
    auto write_all = [&](double edge, double shift) {
      for (int k = t; k < K; k += NT) {
        if (dlen) dlen[fo * K + k] = k < np ? edge : NAN;
        if (dgam) dgam[fo * K + k] = k < np ? edge : NAN;
      }
      if (dshift)
        for (int a = t; a < p; a += NT) dshift[fo * p + a] = shift;
    };
    if (skip) {
      write_all(0.0, 0.0);
      continue;
    }
    const int64_t as = site0 + site, ps = M.per_site ? as : 0;
    const double* __restrict__ R = M.R + ps * F.n_rates * p * p;
    const double* __restrict__ mu = M.mu + ps * p;
    const double* __restrict__ theta = (ou && M.theta) ? M.theta + ps * p : nullptr;
    const double alpha = ou ? M.alpha[ps] : 0.0;
    int st = 0;
    if (any_scope) {
      const double* __restrict__ rec = pool + as * pool_stride + boff[c];
      double mant, quad;
      int expo;
      st = mom_solve<NT, true>(rec, m, packed, fp, W, dv, t, mant, expo, quad);
    } else {
      __syncthreads();   // (the previous site's arrays have been read)
    }
    if (st != 0) {   // not positive definite (the constant belief J = 0 included: no moments)
      write_all(NAN, NAN);
      if (t == 0) atomicMin(info + info0 + site, c + 1);
      continue;
    }
    // coefficients, positions, kept traits
    for (int a = t; a <= np; a += NT) {
      if (a == 0) {
        ipos[0] = cpos;
      } else {
        const int k = a - 1;
        const EdgeCoefs e = edge_coefs(M.model, alpha, F.length[(size_t)f * K + k], F.gamma[(size_t)f * K + k]);
        cf[0 * K + k] = e.qc; cf[1 * K + k] = e.vc; cf[2 * K + k] = e.wc;
        cf[3 * K + k] = e.q_t; cf[4 * K + k] = e.v_t; cf[5 * K + k] = e.w_t;
        cf[6 * K + k] = e.q_g; cf[7 * K + k] = e.v_g; cf[8 * K + k] = e.w_g;
        ipos[a] = F.parent_pos[(size_t)f * K + k];
      }
    }
    for (int tr = t; tr < p; tr += NT)
      if ((O >> tr) & 1ull) oidx[edge_rank(O, tr)] = tr;
    __syncthreads();
    auto cz = [&](int a) -> double { return a == 0 ? 1.0 : -cf[a - 1]; };   // c_0 = 1, c_k = -qc_k
    // where each block's kept traits sit in the cluster, and their posterior mean (or constant value)
    for (int idx = t; idx < nn * mo; idx += NT) {
      const int a = idx / mo, i = idx - a * mo, tr = oidx[i];
      const int pa = ipos[a];
      if (pa >= 0) {
        const unsigned long long ma = a == 0 ? O : (F.parent_mask ? F.parent_mask[(size_t)f * K + a - 1] : full);
        const int v = pa + edge_rank(ma, tr);
        vi[a * p + i] = v;
        xm[a * p + i] = W[v * ld + m];
      } else {
        vi[a * p + i] = -1;
        xm[a * p + i] = a == 0 ? F.data[(as * F.n_rows + F.data_row[f]) * p + tr] : mu[tr];   // tip / fixed root
      }
    }
    // V_OO and the identity
    for (int idx = t; idx < mo * mo; idx += NT) {
      const int j = idx / mo, i = idx - j * mo;
      const int e = oidx[i] + oidx[j] * p;
      double v = 0.0;
      if (np == 0) {
        v = R[(int64_t)F.color[(size_t)f * K] * p * p + e];
      } else {
        for (int k = 0; k < np; ++k) v = v + cf[1 * K + k] * R[(int64_t)F.color[(size_t)f * K + k] * p * p + e];
      }
      A[i * ldv + j] = v;
      A[i * ldv + mo + j] = (i == j) ? 1.0 : 0.0;
    }
    __syncthreads();
    // e = E[r]
    for (int i = t; i < mo; i += NT) {
      const int tr = oidx[i];
      double e = 0.0;
      for (int a = 0; a < nn; ++a) e = e + cz(a) * xm[a * p + i];
      double w = 0.0;
      if (np == 0) {
        w = mu[tr];
      } else if (theta) {
        for (int k = 0; k < np; ++k) w = w + cf[2 * K + k] * theta[tr];
      }
      if (Sh.slot) w = w + lg_shift_d(Sh, F.gamma, f, K, np, tr, p, as);   // a shift of the mean on a parent edge
      ev[i] = e - w;
    }
    __syncthreads();
    // M = Cov(r) + e e'
    for (int idx = t; idx < mo * mo; idx += NT) {
      const int j = idx / mo, i = idx - j * mo;
      double s = 0.0;
      for (int a = 0; a < nn; ++a) {
        const int va = vi[a * p + i];
        if (va < 0) continue;
        for (int b = 0; b < nn; ++b) {
          const int vb = vi[b * p + j];
          if (vb < 0) continue;
          s = s + cz(a) * cz(b) * (va >= vb ? W[va * ld + vb] : W[vb * ld + va]);
        }
      }
      Mx[i * mo + j] = s + ev[i] * ev[j];
    }
    if (!edge_invert<NT>(A, mo, ldv, t)) {   // a variance that is not positive definite: the fill made this cluster's g NaN
      write_all(NAN, NAN);
      if (t == 0) atomicMin(info + info0 + site, c + 1);
      continue;
    }
    // j(i, k): the upper triangle mirrored, exactly symmetric (as the fill reads it)
    auto jj = [&](int i, int k) -> double { return i <= k ? A[i * ldv + mo + k] : A[k * ldv + mo + i]; };
    for (int idx = t; idx < mo * mo; idx += NT) {
      const int k = idx / mo, i = idx - k * mo;
      double s = 0.0;
      for (int l = 0; l < mo; ++l) s = s + jj(i, l) * Mx[l * mo + k];
      Tx[i * mo + k] = s;
    }
    for (int i = t; i < mo; i += NT) {
      double s = 0.0;
      for (int l = 0; l < mo; ++l) s = s + jj(i, l) * ev[l];
      ge[i] = s;
    }
    __syncthreads();
    // G_V = (j M j - j) / 2 (upper triangle computed, mirrored) over M, which T = j M has consumed
    for (int idx = t; idx < mo * mo; idx += NT) {
      const int k = idx / mo, i = idx - k * mo;
      if (i > k) continue;
      double s = 0.0;
      for (int l = 0; l < mo; ++l) s = s + Tx[i * mo + l] * jj(l, k);
      const double g = 0.5 * (s - jj(i, k));
      Mx[i * mo + k] = g;
      Mx[k * mo + i] = g;
    }
    // the shift: g_w embedded into the p traits
    if (dshift)
      for (int tr = t; tr < p; tr += NT) dshift[fo * p + tr] = ((O >> tr) & 1ull) ? ge[edge_rank(O, tr)] : 0.0;
    for (int k = np + t; k < K; k += NT) {   // no such edge (every entry of a root-prior family)
      if (dlen) dlen[fo * K + k] = NAN;
      if (dgam) dgam[fo * K + k] = NAN;
    }
    if (!dlen && !dgam) continue;
    for (int k = 0; k < np; ++k) {
      __syncthreads();   // (G_V is complete and T read; the previous edge's row sums have been read)
      const double* __restrict__ Rk = R + (int64_t)F.color[(size_t)f * K + k] * p * p;
      for (int idx = t; idx < mo * mo; idx += NT) {
        const int i = idx / mo, l = idx - i * mo;
        // E[r x_k'](i, l) = sum_a c_a Sigma(a_i, k_l) + e_i m_k(l)
        double ex = ev[i] * xm[(k + 1) * p + l];
        const int vk = vi[(k + 1) * p + l];
        if (vk >= 0) {
          for (int a = 0; a < nn; ++a) {
            const int va = vi[a * p + i];
            if (va >= 0) ex = ex + cz(a) * (va >= vk ? W[va * ld + vk] : W[vk * ld + va]);
          }
        }
        Px[idx] = jj(l, i) * ex;
        Tx[idx] = Mx[idx] * Rk[oidx[l] + oidx[i] * p];
      }
      __syncthreads();
      for (int i = t; i < mo; i += NT) {   // row i in column order
        double sq = 0.0, sr = 0.0;
        for (int l = 0; l < mo; ++l) {
          sq = sq + Px[i * mo + l];
          sr = sr + Tx[i * mo + l];
        }
        rq[i] = sq;
        rr[i] = sr;
      }
      __syncthreads();
      if (t == 0) {   // the rows in row order
        double gq = 0.0, trGR = 0.0, thg = 0.0;
        for (int i = 0; i < mo; ++i) {
          gq = gq + rq[i];
          trGR = trGR + rr[i];
          if (theta) thg = thg + theta[oidx[i]] * ge[i];
        }
        if (dlen) dlen[fo * K + k] = cf[4 * K + k] * trGR + cf[5 * K + k] * thg + cf[3 * K + k] * gq;
        if (dgam) {
          double dg = cf[7 * K + k] * trGR + cf[8 * K + k] * thg + cf[6 * K + k] * gq;
          if (Sh.slot && Sh.slot[(size_t)f * K + k] >= 0) {   // the shift's coefficient is gamma_k: + s_k,O' g_w
            double sg = 0.0;
            for (int i = 0; i < mo; ++i) sg = sg + lg_shift_value(Sh, (int64_t)f * K + k, oidx[i], p, as) * ge[i];
            dg = dg + sg;
          }
          dgam[fo * K + k] = dg;
        }
      }
    }
  }
}

}  // namespace pgbp

using namespace pgbp;

extern "C" int pgbp_lg_edge_gradient(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dlength, double* dgamma,
                                     double* dshift, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  LgParams M{};
  {
    const EngineView v0 = engine_peek(e);
    if (!v0.lg_ready)
      return engine_fail(e, PGBP_ERR_STATE, "pgbp_lg_edge_gradient: no family table (call pgbp_lg_setup first)");
    if (!engine_lg_params(e, &M))
      return engine_fail(e, PGBP_ERR_STATE, "pgbp_lg_edge_gradient: no parameters yet (call pgbp_lg_assignfactors first)");
    if (site_begin < 0 || site_end < site_begin || site_end > v0.plan->n_sites)
      return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_edge_gradient: site range outside the engine's sites");
    if (!dlength && !dgamma && !dshift) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_edge_gradient: no output buffer");
  }
  EngineView v;
  int rc = engine_view(e, &v);
  if (rc) return rc;
  // (as in pgbp_lg_gradient, what follows runs on the caller's current device)
  const Plan& pl = *v.plan;
  const LgStatic& F = *v.lg;
  const LgShifts Sh = engine_lg_shifts(e);
  const int nc = pl.n_clusters, p = F.p, K = F.K;
  // which cluster each family sits in (the CSR of pgbp_lg_setup back from the device: a word per family)
  std::vector<int32_t> off(nc + 1);
  hipError_t herr = hipMemcpy(off.data(), F.cl_off, sizeof(int32_t) * (nc + 1), hipMemcpyDeviceToHost);
  const int nf = herr == hipSuccess ? off[nc] : 0;
  std::vector<int32_t> cfam(std::max(nf, 1));
  if (herr == hipSuccess && nf > 0) herr = hipMemcpy(cfam.data(), F.cl_fam, sizeof(int32_t) * nf, hipMemcpyDeviceToHost);
  if (herr != hipSuccess)
    return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_edge_gradient (family table): ") + hipGetErrorString(herr));
  std::vector<int32_t> fcl(std::max(nf, 1), 0);
  int max_m = 1;
  for (int c = 0; c < nc; ++c)
    for (int q = off[c]; q < off[c + 1]; ++q) {
      fcl[cfam[q]] = c;
      if (pl.dims[c] > kLdsMaxDim)
        return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_edge_gradient: family " + std::to_string(cfam[q]) + " (cluster " +
                                                    std::to_string(c) + "): the cluster has more than " +
                                                    std::to_string(kLdsMaxDim) + " variables");
      max_m = std::max(max_m, (int)pl.dims[c]);
    }
  const size_t lds_bytes = sizeof(double) * (mom_lds_doubles(max_m) + ((edge_extra_doubles(p, K) + 1) & ~(size_t)1)) +
                           sizeof(int) * edge_extra_ints(p, K);
  if (lds_bytes > 160 * 1024)
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_edge_gradient: a cluster of " + std::to_string(max_m) + " variables with " +
                                                std::to_string(p) + " traits needs " + std::to_string(lds_bytes) +
                                                " bytes of LDS, more than the 160 KB of a compute unit");
  const int ns = site_end - site_begin;
  if (ns == 0) return PGBP_OK;
  if (nf == 0) {
    if (info) std::fill(info, info + ns, 0);
    return PGBP_OK;
  }
  // device copies of the requested outputs for a chunk of sites (256 MB at most), copied out chunk by chunk in stream order
  const int64_t per_site = (int64_t)nf * ((dlength ? K : 0) + (dgamma ? K : 0) + (dshift ? p : 0));
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(ns, ((int64_t)32 << 20) / per_site));
  std::vector<int32_t> inf(ns, 0x7fffffff);   // (ahead of the buffers: they are released, which drains the uploads, first)
  DevBuf<int32_t> d_fcl, d_info;
  DevBuf<double> d_len, d_gam, d_shift;
  herr = (hipError_t)d_fcl.alloc(nf);
  if (herr == hipSuccess && dlength) herr = (hipError_t)d_len.alloc((size_t)chunk * nf * K);
  if (herr == hipSuccess && dgamma) herr = (hipError_t)d_gam.alloc((size_t)chunk * nf * K);
  if (herr == hipSuccess && dshift) herr = (hipError_t)d_shift.alloc((size_t)chunk * nf * p);
  if (herr == hipSuccess) herr = (hipError_t)d_info.alloc((size_t)ns);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_fcl.get(), fcl.data(), sizeof(int32_t) * nf, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_info.get(), inf.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice, v.st);
  if (herr != hipSuccess)
    return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_edge_gradient (scratch): ") + hipGetErrorString(herr));
  (void)hipGetLastError();   // (an error an earlier asynchronous call left behind is that call's to report)
  {
    const void* kern = max_m <= 64 ? reinterpret_cast<const void*>(edge_family<64>) : reinterpret_cast<const void*>(edge_family<256>);
    if (lds_bytes > 64 * 1024) herr = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    for (int s0 = 0; herr == hipSuccess && s0 < ns; s0 += chunk) {
      const int n = std::min(chunk, ns - s0), gy = std::min(n, 65535);
      if (max_m <= 64)
        hipLaunchKernelGGL(edge_family<64>, dim3(nf, gy), dim3(64), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, d_fcl.get(), nf, site_begin + s0, n, d_len.get(), d_gam.get(), d_shift.get(),
                           d_info.get(), s0);
      else
        hipLaunchKernelGGL(edge_family<256>, dim3(nf, gy), dim3(256), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, d_fcl.get(), nf, site_begin + s0, n, d_len.get(), d_gam.get(), d_shift.get(),
                           d_info.get(), s0);
      herr = hipGetLastError();
      const size_t nk = (size_t)n * nf * K, np_ = (size_t)n * nf * p, ok = (size_t)s0 * nf * K, op = (size_t)s0 * nf * p;
      if (herr == hipSuccess && dlength)
        herr = hipMemcpyAsync(dlength + ok, d_len.get(), sizeof(double) * nk, hipMemcpyDeviceToHost, v.st);
      if (herr == hipSuccess && dgamma)
        herr = hipMemcpyAsync(dgamma + ok, d_gam.get(), sizeof(double) * nk, hipMemcpyDeviceToHost, v.st);
      if (herr == hipSuccess && dshift)
        herr = hipMemcpyAsync(dshift + op, d_shift.get(), sizeof(double) * np_, hipMemcpyDeviceToHost, v.st);
    }
  }
  if (herr == hipSuccess) herr = hipMemcpyAsync(inf.data(), d_info.get(), sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, v.st);
  const hipError_t serr = hipStreamSynchronize(v.st);
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_edge_gradient: ") + hipGetErrorString(herr));
  for (int s = 0; s < ns; ++s) {
    const int32_t bad = inf[s] == 0x7fffffff ? 0 : inf[s];
    if (info) info[s] = bad;
    if (!bad) continue;   // a site with a cluster that is not positive definite: every entry NaN
    if (dlength) std::fill(dlength + (size_t)s * nf * K, dlength + (size_t)(s + 1) * nf * K, NAN);
    if (dgamma) std::fill(dgamma + (size_t)s * nf * K, dgamma + (size_t)(s + 1) * nf * K, NAN);
    if (dshift) std::fill(dshift + (size_t)s * nf * p, dshift + (size_t)(s + 1) * nf * p, NAN);
  }
  return PGBP_OK;
}

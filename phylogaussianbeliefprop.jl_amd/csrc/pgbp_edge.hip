// Derivatives of the log-likelihood in every edge length, every inheritance and a mean shift on every edge, from calibrated
// beliefs (pgbp_lg_edge_gradient of include/pgbp.h).
//
// Fisher's identity as in pgbp_grad.hip, without the sum over the families: the length t_k and the inheritance gamma_k of
// parent edge k enter the likelihood through the factor of their own family only, and there through the edge coefficients
// (qc_k, vc_k, wc_k) of lg_coefs (pgbp_fam_dev.hpp; their derivatives: lg_coefs_dedge).  With the family quantities that
// fam_score_T and fam_score_gv of that header form for this kernel and grad_family alike -- O = child_mask[f],
// j = (V_OO)^-1, r = x_child - sum_k qc_k x_k - w, e = E[r], M = Cov(r) + e e', G_V = (j M j - j) / 2, g_w = j e,
// g_qk = E[r' j x_k] under the belief of the family's cluster --
//   dX_k = dvc_k/dX tr(G_V R[colour_k]_OO) + dwc_k/dX theta_O' g_w + dqc_k/dX g_qk,    X in {t, gamma},
//   BM:  dqc/dt = 0,            dvc/dt = gamma^2,               dwc/dt = 0;
//        dqc/dgamma = 1,        dvc/dgamma = 2 gamma t,         dwc/dgamma = 0;
//   OU (a = e^(-alpha t)):
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
#include "pgbp_fam_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"

namespace pgbp {

extern __shared__ double edge_lds[];

// LDS of edge_family: fam_score's arrays with six more rows of coefficients (LgEdgeDerivs: q_t, v_t, w_t, q_g, v_g, w_g), and
// of its own Px (p x p) and the row sums rq, rr (p each)
constexpr int kEdgeRows = 9;
__host__ __device__ inline size_t edge_extra_doubles(int p) { return (size_t)p * p + 2 * (size_t)p; }

// dlen / dgam [n_sites][n_fam][K], dshift [n_sites][n_fam][p] of the sites site0 .. site0 + n_sites (any may be null)
template <int NT>
__global__ __launch_bounds__(NT) void edge_family(const double* __restrict__ pool, int64_t pool_stride,
                                                  const int64_t* __restrict__ boff, const int32_t* __restrict__ bdim, int bs,
                                                  int fp, LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz,
                                                  const int32_t* __restrict__ fam_cluster,
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
  const FamLds L = fam_carve(edge_lds, m, p, K, kEdgeRows, edge_extra_doubles(p));
  const int ldv = fam_ldv(p);
  double* cf = L.cf;                            // rows of K: qc, vc, wc, then LgEdgeDerivs
  double* __restrict__ Tx = L.Tx;               // j M, then the terms of tr(G_V R[colour_k])
  double* __restrict__ Px = L.extra;            // the terms of g_qk = sum_il j(l, i) E[r x_k'](i, l)
  double* __restrict__ rq = Px + p * p;         // row sums of Px, of Tx
  double* __restrict__ rr = rq + p;
  bool any_scope = cpos >= 0;
  for (int k = 0; k < np; ++k) any_scope |= F.parent_pos[(size_t)f * K + k] >= 0;
  // families the factor fill skips (and a root-prior family of a fixed root, which has no factor)
  const bool skip = mo == 0 || (np == 0 && cpos < 0);
  const bool packed = bs && bs16::applies(m, fp);
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
    const int64_t as = site0 + site;
    const LgSite S = lg_site(M, F.n_rates, p, as);
    int st = 0;
    if (any_scope) {
      const double* __restrict__ rec = pool + as * pool_stride + boff[c];
      double mant, quad;
      int expo;
      st = mom_solve<NT, true>(rec, m, packed, fp, L.W, L.dv, t, mant, expo, quad);
    } else {
      __syncthreads();   // (the previous site's arrays have been read)
    }
    // the cluster is not positive definite (the constant belief J = 0 included: no moments), or the family's variance is not
    // (the fill made this cluster's g NaN)
    if (st == 0) {
      for (int k = t; k < np; k += NT) {
        const LgEdgeDerivs d = lg_coefs_dedge(M.model, S.alpha, F.length[(size_t)f * K + k], F.gamma[(size_t)f * K + k]);
        cf[3 * K + k] = d.q_t; cf[4 * K + k] = d.v_t; cf[5 * K + k] = d.w_t;
        cf[6 * K + k] = d.q_g; cf[7 * K + k] = d.v_g; cf[8 * K + k] = d.w_g;
      }
      if (!fam_score_T<NT>(L, F, M, Sh, Nz, S, f, m, O, as, t)) st = 1;
    }
    if (st != 0) {
      write_all(NAN, NAN);
      if (t == 0) atomicMin(info + info0 + site, c + 1);
      continue;
    }
    fam_score_gv<NT>(L, p, mo, nullptr, t);   // G_V over M
    // the shift: g_w embedded into the p traits
    if (dshift)
      for (int tr = t; tr < p; tr += NT) dshift[fo * p + tr] = ((O >> tr) & 1ull) ? L.ge[mask_rank(O, tr)] : 0.0;
    for (int k = np + t; k < K; k += NT) {   // no such edge (every entry of a root-prior family)
      if (dlen) dlen[fo * K + k] = NAN;
      if (dgam) dgam[fo * K + k] = NAN;
    }
    if (!dlen && !dgam) continue;
    for (int k = 0; k < np; ++k) {
      __syncthreads();   // (G_V is complete and T read; the previous edge's row sums have been read)
      const double* __restrict__ Rk = S.R + (int64_t)F.color[(size_t)f * K + k] * p * p;
      for (int idx = t; idx < mo * mo; idx += NT) {
        const int i = idx / mo, l = idx - i * mo;
        // E[r x_k'](i, l) = sum_a c_a Sigma(a_i, k_l) + e_i m_k(l)
        double ex = L.ev[i] * L.xm[(k + 1) * p + l];
        const int vk = L.vi[(k + 1) * p + l];
        if (vk >= 0) {
          for (int a = 0; a < nn; ++a) {
            const int va = L.vi[a * p + i];
            if (va >= 0) ex = ex + fam_c(cf, a) * (va >= vk ? L.W[va * ld + vk] : L.W[vk * ld + va]);
          }
        }
        Px[idx] = fam_j(L.A, ldv, mo, l, i) * ex;
        Tx[idx] = L.Mx[idx] * Rk[L.oidx[l] + L.oidx[i] * p];
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
          if (S.theta) thg = thg + S.theta[L.oidx[i]] * L.ge[i];
        }
        if (dlen) dlen[fo * K + k] = cf[4 * K + k] * trGR + cf[5 * K + k] * thg + cf[3 * K + k] * gq;
        if (dgam) {
          double dg = cf[7 * K + k] * trGR + cf[8 * K + k] * thg + cf[6 * K + k] * gq;
          if (Sh.slot && Sh.slot[(size_t)f * K + k] >= 0) {   // the shift's coefficient is gamma_k: + s_k,O' g_w
            double sg = 0.0;
            for (int i = 0; i < mo; ++i) sg = sg + lg_shift_value(Sh, (int64_t)f * K + k, L.oidx[i], p, as) * L.ge[i];
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
  const LgModel* L = nullptr;
  int rc = lg_sweep_state(e, "pgbp_lg_edge_gradient", site_begin, site_end, &L, "pgbp_lg_edge_gradient_sites");
  if (rc) return rc;
  if ((rc = lg_refuse_optima(e, "pgbp_lg_edge_gradient", L))) return rc;
  const LgStatic& F = L->F;
  const LgParams& M = L->M;
  const LgShifts& Sh = L->Sh;
  const LgNoise& Nz = L->Nz;
  if (!dlength && !dgamma && !dshift) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_edge_gradient: no output buffer");
  EngineView v;
  if ((rc = engine_view(e, &v))) return rc;
  // (as in pgbp_lg_gradient, what follows runs on the caller's current device)
  const Plan& pl = *v.plan;
  const int p = F.p, K = F.K;
  const std::vector<int32_t>& fcl = L->T.cluster;   // which cluster each family sits in
  int max_m = 0;
  std::string why;
  if (!L->T.cluster_dims("pgbp_lg_edge_gradient", kLdsMaxDim, &max_m, why)) return engine_fail(e, PGBP_ERR_INVALID, why);
  const int nf = L->T.n_families;
  const size_t lds_bytes = fam_score_lds_bytes(max_m, p, K, kEdgeRows, edge_extra_doubles(p));
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
  hipError_t herr = (hipError_t)d_fcl.alloc(nf);
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
                           v.bs16, pl.fast_p, F, M, Sh, Nz, d_fcl.get(), nf, site_begin + s0, n, d_len.get(), d_gam.get(), d_shift.get(),
                           d_info.get(), s0);
      else
        hipLaunchKernelGGL(edge_family<256>, dim3(nf, gy), dim3(256), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, Nz, d_fcl.get(), nf, site_begin + s0, n, d_len.get(), d_gam.get(), d_shift.get(),
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

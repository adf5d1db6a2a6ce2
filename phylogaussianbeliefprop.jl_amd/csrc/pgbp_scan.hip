// A scan of every edge for a mean shift, from calibrated beliefs (pgbp_lg_shift_scan of include/pgbp.h): the maximum-
// likelihood displacement of every family's conditional mean, its observed information and the likelihood-ratio statistic.
//
// The log-likelihood is quadratic in a displacement d of the child's conditional mean (r = x_child - sum_k qc_k x_k - w - d).
// With the family quantities of pgbp_fam_dev.hpp -- O = child_mask[f], j = (V_OO)^-1, e = E[r], g_w = j e -- and
// C = Cov(r | data) (the double sum of fam_cov, WITHOUT the e e' term):
//   score at d = 0:            g_w
//   observed information:      H_f = j - j C j      (mo x mo; no data value enters it)
//   ML displacement:           dhat = H_f^-1 g_w
//   gain 2 (ll(dhat) - ll(0)): lr = g_w' H_f^-1 g_w
// A shift s_k on parent edge k enters as gamma_k s_k: shat_k = dhat / gamma_k, information gamma_k^2 H_f, the same lr.
//
// H_f is formed from C itself.  j M j - j with M = C + e e' (what fam_score_T and fam_score_gv form for the gradients) holds
// H_f as well, minus g_w g_w': at the edges the scan is run for |e| is large, and taking g_w g_w' back out would cost H_f the
// digits of that product.  Formed directly, H_f of a site is the same bytes whatever its data.
//
// The traits of O are taken in index order by a left-looking Cholesky with a skip (lds_cholesky_skip): a trait whose pivot,
// given the kept traits before it, is not above min_info * j_ii is not identified (no tip below observes it, or the data leave
// the prior untouched) and is dropped, row and column; the solve is the ML displacement restricted to the kept traits.
//
// One workgroup per (family, site), the frame of edge_family: the cluster solved in LDS (mom_solve), every sum in a fixed index
// order, contraction off, each workgroup writing its own outputs only -- no reduction, no atomics on doubles, the same bytes
// on every call and for every chunking of the sites.
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

extern __shared__ double scan_lds[];

// LDS of scan_family: fam_score's arrays with the three rows of coefficients, and of its own C (p x p), the diagonal of the
// factor, the right-hand side and the solution (p each).  H_f takes Mx and j C takes Tx, which fam_score_T has finished with.
constexpr int kScanRows = 3;
__host__ __device__ inline size_t scan_extra_doubles(int p) { return (size_t)p * p + 3 * (size_t)p; }
// ... and, behind the ints, the plain copy of a packed (BS16) record (fam_stage_plain): the solve then reads a packed record
// through its upper triangle, as it reads a plain one, and the two layouts give the same bytes
__host__ __device__ inline size_t scan_stage_offset(int m, int p, int K) {
  return (fam_score_lds_bytes(m, p, K, kScanRows, scan_extra_doubles(p)) + sizeof(double) - 1) / sizeof(double);
}

// jump [n_sites][n_fam][p], lr [n_sites][n_fam], ident [n_sites][n_fam], hinf [n_sites][n_fam][p][p] of the sites
// site0 .. site0 + n_sites (any may be null)
template <int NT>
__global__ __launch_bounds__(NT) void scan_family(const double* __restrict__ pool, int64_t pool_stride,
                                                  const int64_t* __restrict__ boff, const int32_t* __restrict__ bdim, int bs,
                                                  int fp, LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz,
                                                  const int32_t* __restrict__ fam_cluster,
                                                  int n_fam, int site0, int n_sites, double min_info, double* __restrict__ jump,
                                                  double* __restrict__ lr, unsigned long long* __restrict__ ident,
                                                  double* __restrict__ hinf, int32_t* __restrict__ info, int info0) {
#pragma clang fp contract(off)
  const int t = threadIdx.x, f = blockIdx.x;
  const int p = F.p, K = F.K, np = F.n_parents[f], nn = np + 1;
  const int c = fam_cluster[f], m = bdim[c], ld = (m + 1) | 1;
  const unsigned long long full = p >= 64 ? ~0ull : ((1ull << p) - 1ull);
  const unsigned long long O = F.child_mask ? (F.child_mask[f] & full) : full;
  const int mo = __popcll(O);
  const int cpos = F.child_pos[f];
  const FamLds L = fam_carve(scan_lds, m, p, K, kScanRows, scan_extra_doubles(p));
  const int ldv = fam_ldv(p);
  double* __restrict__ Cx = L.extra;       // C = Cov(r | data)
  double* __restrict__ dl = Cx + p * p;    // the diagonal of H_f's factor at the kept traits
  double* __restrict__ yv = dl + p;        // g_w, then the forward solve's y, then the back solve's right-hand side
  double* __restrict__ xv = yv + p;        // dhat
  double* __restrict__ Hx = L.Mx;          // H_f; below the diagonal its factor
  double* __restrict__ JC = L.Tx;          // j C
  double* __restrict__ stage = scan_lds + scan_stage_offset(m, p, K);
  bool any_scope = cpos >= 0;
  for (int k = 0; k < np; ++k) any_scope |= F.parent_pos[(size_t)f * K + k] >= 0;
  const bool packed = bs && bs16::applies(m, fp);
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const int64_t fo = (int64_t)site * n_fam + f;
    // every entry of the family: NaN jump and information, `gain`, no trait identified
    auto write_none = [&](double gain) {
      if (jump)
        for (int a = t; a < p; a += NT) jump[fo * p + a] = NAN;
      if (hinf)
        for (int a = t; a < p * p; a += NT) hinf[fo * p * p + a] = NAN;
      if (t == 0) {
        if (lr) lr[fo] = gain;
        if (ident) ident[fo] = 0ull;
      }
    };
    // a family the factor fill skips
    if (mo == 0 || (np == 0 && cpos < 0)) {
      write_none(np == 0 ? NAN : 0.0);
      continue;
    }
    const int64_t as = site0 + site;
    const LgSite S = lg_site(M, F.n_rates, p, as);
    int st = 0;
    if (any_scope) {
      const double* __restrict__ rec = pool + as * pool_stride + boff[c];
      double mant, quad;
      int expo;
      if (packed) {   // (the previous site's solve read its copy ahead of its first barrier)
        fam_stage_plain<NT>(rec, m, fp, stage, t);
        rec = stage;
      }
      st = mom_solve<NT, true>(rec, m, false, fp, L.W, L.dv, t, mant, expo, quad);
    } else {
      __syncthreads();   // (the previous site's arrays have been read)
    }
    // a root-prior family has no edge; its cluster's failure is reported as the edge sweep reports it
    if (st == 0 && np > 0 && !fam_score_T<NT>(L, F, M, Sh, Nz, S, f, m, O, as, t)) st = 1;
    if (st != 0) {
      write_none(NAN);
      if (t == 0) atomicMin(info + info0 + site, c + 1);
      continue;
    }
    if (np == 0) {
      write_none(NAN);
      continue;
    }
    __syncthreads();   // (fam_score_T's Tx and ge are written; Mx and Tx are free from here)
    // C: the upper triangle in fam_cov's order, mirrored
    for (int idx = t; idx < mo * mo; idx += NT) {
      const int i = idx / mo, k = idx - i * mo;
      if (i > k) continue;
      const double s = fam_cov(L.W, ld, L.vi, p, [&](int a) -> double { return fam_c(L.cf, a); }, nn, i, k);
      Cx[i * mo + k] = s;
      Cx[k * mo + i] = s;
    }
    for (int i = t; i < mo; i += NT) yv[i] = L.ge[i];
    __syncthreads();
    for (int idx = t; idx < mo * mo; idx += NT) {
      const int i = idx / mo, k = idx - i * mo;
      double s = 0.0;
      for (int l = 0; l < mo; ++l) s = s + fam_j(L.A, ldv, mo, i, l) * Cx[l * mo + k];
      JC[i * mo + k] = s;
    }
    __syncthreads();
    // H_f = j - (j C) j: the upper triangle, mirrored
    for (int idx = t; idx < mo * mo; idx += NT) {
      const int i = idx / mo, k = idx - i * mo;
      if (i > k) continue;
      double s = 0.0;
      for (int l = 0; l < mo; ++l) s = s + JC[i * mo + l] * fam_j(L.A, ldv, mo, l, k);
      const double h = fam_j(L.A, ldv, mo, i, k) - s;
      Hx[i * mo + k] = h;
      Hx[k * mo + i] = h;
    }
    __syncthreads();
    // the kept traits: pivot_i > min_info * j_ii (j's diagonal sits at A[i * ldv + mo + i])
    const unsigned long long kept = lds_cholesky_skip<NT>(Hx, mo, mo, dl, L.A + mo, ldv + 1, min_info, t);
    // forward: L y = g_w on the kept traits, column by column (row i gathers its terms in the order of the columns)
    for (int k = 0; k < mo; ++k) {
      if (!((kept >> k) & 1ull)) continue;
      const double yk = yv[k] / dl[k];
      for (int i = k + 1 + t; i < mo; i += NT)
        if ((kept >> i) & 1ull) yv[i] = fma(-Hx[i * mo + k], yk, yv[i]);
      __syncthreads();
    }
    for (int i = t; i < mo; i += NT)
      if ((kept >> i) & 1ull) yv[i] = yv[i] / dl[i];
    __syncthreads();
    if (t == 0 && lr) {   // the gain: sum of y_i^2 in index order
      double s = 0.0;
      for (int i = 0; i < mo; ++i)
        if ((kept >> i) & 1ull) s = s + yv[i] * yv[i];
      lr[fo] = s;
    }
    // back: L' dhat = y, from the last kept trait down
    for (int k = mo - 1; k >= 0; --k) {
      if (!((kept >> k) & 1ull)) continue;
      const double xk = yv[k] / dl[k];
      if (t == 0) xv[k] = xk;
      for (int i = t; i < k; i += NT)
        if ((kept >> i) & 1ull) yv[i] = fma(-Hx[k * mo + i], xk, yv[i]);
      __syncthreads();
    }
    // outputs, embedded into the p traits (H_f from its upper triangle, which the factorisation left as it was)
    if (jump)
      for (int tr = t; tr < p; tr += NT) {
        const int i = mask_rank(O, tr);
        jump[fo * p + tr] = (((O >> tr) & 1ull) && ((kept >> i) & 1ull)) ? xv[i] : NAN;
      }
    if (hinf)
      for (int idx = t; idx < p * p; idx += NT) {
        const int a = idx / p, b = idx - a * p;
        double h = NAN;
        if (((O >> a) & 1ull) && ((O >> b) & 1ull)) {
          const int i = mask_rank(O, a), k = mask_rank(O, b);
          if (((kept >> i) & 1ull) && ((kept >> k) & 1ull)) h = i <= k ? Hx[i * mo + k] : Hx[k * mo + i];
        }
        hinf[fo * p * p + idx] = h;
      }
    if (t == 0 && ident) {
      unsigned long long id = 0ull;
      for (int i = 0; i < mo; ++i)
        if ((kept >> i) & 1ull) id |= 1ull << L.oidx[i];
      ident[fo] = id;
    }
  }
}

}  // namespace pgbp

using namespace pgbp;

extern "C" int pgbp_lg_shift_scan(pgbp_engine* e, int32_t site_begin, int32_t site_end, double min_info, double* jump, double* lr,
                                  uint64_t* identified, double* information, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const LgModel* L = engine_lg(e);
  if (!L) return engine_fail(e, PGBP_ERR_STATE, "pgbp_lg_shift_scan: no family table (call pgbp_lg_setup first)");
  if (L->T.p > 64)   // (a table the scan cannot serve, whatever its parameters)
    return engine_fail(e, PGBP_ERR_INVALID,
                       "pgbp_lg_shift_scan: p = " + std::to_string(L->T.p) + " traits, more than the 64 of a trait mask");
  int rc = lg_sweep_state(e, "pgbp_lg_shift_scan", site_begin, site_end, &L, "pgbp_lg_shift_scan_sites");
  if (rc) return rc;
  if ((rc = lg_refuse_optima(e, "pgbp_lg_shift_scan", L))) return rc;
  const LgStatic& F = L->F;
  const LgParams& M = L->M;
  const LgShifts& Sh = L->Sh;
  const LgNoise& Nz = L->Nz;
  if (!jump && !lr && !identified && !information)
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_shift_scan: no output buffer");
  if (!(min_info >= 0.0 && min_info < 1.0))
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_shift_scan: min_info = " + std::to_string(min_info) + " is not in [0, 1)");
  EngineView v;
  if ((rc = engine_view(e, &v))) return rc;
  // (as in pgbp_lg_edge_gradient, what follows runs on the caller's current device)
  const Plan& pl = *v.plan;
  const int p = F.p, K = F.K;
  const std::vector<int32_t>& fcl = L->T.cluster;   // which cluster each family sits in
  int max_m = 0;
  std::string why;
  if (!L->T.cluster_dims("pgbp_lg_shift_scan", kLdsMaxDim, &max_m, why)) return engine_fail(e, PGBP_ERR_INVALID, why);
  const int nf = L->T.n_families;
  size_t stage = 0;   // a packed record's plain copy
  for (int f = 0; f < nf && v.bs16; ++f) {
    const size_t m = (size_t)pl.dims[fcl[f]];
    if (bs16::applies((int)m, pl.fast_p)) stage = std::max(stage, m * m + m);
  }
  const size_t lds_bytes = sizeof(double) * (scan_stage_offset(max_m, p, K) + stage);
  if (lds_bytes > 160 * 1024)
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_shift_scan: a cluster of " + std::to_string(max_m) + " variables with " +
                                                std::to_string(p) + " traits needs " + std::to_string(lds_bytes) +
                                                " bytes of LDS, more than the 160 KB of a compute unit");
  const int ns = site_end - site_begin;
  if (ns == 0) return PGBP_OK;
  if (nf == 0) {
    if (info) std::fill(info, info + ns, 0);
    return PGBP_OK;
  }
  // device copies of the requested outputs for a chunk of sites (256 MB at most), copied out chunk by chunk in stream order
  const int64_t per_site =
      (int64_t)nf * ((jump ? p : 0) + (lr ? 1 : 0) + (identified ? 1 : 0) + (information ? (int64_t)p * p : 0));
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(ns, ((int64_t)32 << 20) / per_site));
  std::vector<int32_t> inf(ns, 0x7fffffff);   // (ahead of the buffers: they are released, which drains the uploads, first)
  DevBuf<int32_t> d_fcl, d_info;
  DevBuf<double> d_jump, d_lr, d_hinf;
  DevBuf<unsigned long long> d_id;
  hipError_t herr = (hipError_t)d_fcl.alloc(nf);
  if (herr == hipSuccess && jump) herr = (hipError_t)d_jump.alloc((size_t)chunk * nf * p);
  if (herr == hipSuccess && lr) herr = (hipError_t)d_lr.alloc((size_t)chunk * nf);
  if (herr == hipSuccess && identified) herr = (hipError_t)d_id.alloc((size_t)chunk * nf);
  if (herr == hipSuccess && information) herr = (hipError_t)d_hinf.alloc((size_t)chunk * nf * p * p);
  if (herr == hipSuccess) herr = (hipError_t)d_info.alloc((size_t)ns);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_fcl.get(), fcl.data(), sizeof(int32_t) * nf, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_info.get(), inf.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice, v.st);
  if (herr != hipSuccess)
    return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_shift_scan (scratch): ") + hipGetErrorString(herr));
  (void)hipGetLastError();   // (an error an earlier asynchronous call left behind is that call's to report)
  {
    const void* kern = max_m <= 64 ? reinterpret_cast<const void*>(scan_family<64>) : reinterpret_cast<const void*>(scan_family<256>);
    if (lds_bytes > 64 * 1024) herr = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    for (int s0 = 0; herr == hipSuccess && s0 < ns; s0 += chunk) {
      const int n = std::min(chunk, ns - s0), gy = std::min(n, 65535);
      if (max_m <= 64)
        hipLaunchKernelGGL(scan_family<64>, dim3(nf, gy), dim3(64), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, Nz, d_fcl.get(), nf, site_begin + s0, n, min_info, d_jump.get(), d_lr.get(),
                           d_id.get(), d_hinf.get(), d_info.get(), s0);
      else
        hipLaunchKernelGGL(scan_family<256>, dim3(nf, gy), dim3(256), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, Nz, d_fcl.get(), nf, site_begin + s0, n, min_info, d_jump.get(), d_lr.get(),
                           d_id.get(), d_hinf.get(), d_info.get(), s0);
      herr = hipGetLastError();
      const size_t n1 = (size_t)n * nf, o1 = (size_t)s0 * nf;
      if (herr == hipSuccess && jump)
        herr = hipMemcpyAsync(jump + o1 * p, d_jump.get(), sizeof(double) * n1 * p, hipMemcpyDeviceToHost, v.st);
      if (herr == hipSuccess && lr) herr = hipMemcpyAsync(lr + o1, d_lr.get(), sizeof(double) * n1, hipMemcpyDeviceToHost, v.st);
      if (herr == hipSuccess && identified)
        herr = hipMemcpyAsync(identified + o1, d_id.get(), sizeof(uint64_t) * n1, hipMemcpyDeviceToHost, v.st);
      if (herr == hipSuccess && information)
        herr = hipMemcpyAsync(information + o1 * p * p, d_hinf.get(), sizeof(double) * n1 * p * p, hipMemcpyDeviceToHost, v.st);
    }
  }
  if (herr == hipSuccess) herr = hipMemcpyAsync(inf.data(), d_info.get(), sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, v.st);
  const hipError_t serr = hipStreamSynchronize(v.st);
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_shift_scan: ") + hipGetErrorString(herr));
  for (int s = 0; s < ns; ++s) {
    const int32_t bad = inf[s] == 0x7fffffff ? 0 : inf[s];
    if (info) info[s] = bad;
    if (!bad) continue;   // a site with a cluster that is not positive definite: NaN throughout, no trait identified
    const size_t a = (size_t)s * nf, b = (size_t)(s + 1) * nf;
    if (jump) std::fill(jump + a * p, jump + b * p, NAN);
    if (lr) std::fill(lr + a, lr + b, NAN);
    if (identified) std::fill(identified + a, identified + b, (uint64_t)0);
    if (information) std::fill(information + a * p * p, information + b * p * p, NAN);
  }
  return PGBP_OK;
}

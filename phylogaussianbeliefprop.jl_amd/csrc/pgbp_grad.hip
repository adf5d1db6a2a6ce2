// Exact gradient of the log-likelihood from calibrated beliefs (pgbp_lg_gradient of include/pgbp.h).
//
// Fisher's identity: d loglik / d theta = sum_f E[ d log phi_f / d theta | data ], a sum over the node families given to
// pgbp_lg_setup of an expectation under the posterior of the family's variables -- the calibrated belief of the family's
// cluster.  Notation of pgbp_lgfill.hip: child coefficient c_0 = 1, parent k c_k = -qc_k, V = sum_k vc_k R[colour_k],
// w = sum_k wc_k theta (root-prior family: r = x_root - mu, V = R[colour]); O = child_mask[f] the components the factor
// keeps, j = (V_OO)^-1.  With r = sum_a c_a x_a - w, a block in scope random with the posterior moments (m_a, Sigma_ab) of
// the cluster's J^-1 h and J^-1, a tip's data row and the fixed root's mean constants:
//   e = E[r],  M = Cov(r) + e e',   G_V = (j M j - j) / 2   (d loglik = tr(G_V dV)),   g_w = j e   (d loglik = g_w' dw),
//   g_qk = E[r' j x_k] = tr(j (sum_a c_a Sigma_ak + e m_k'))                          (d loglik = g_qk dqc_k),
// and the chain rule through the edge coefficients (lg_coefs, lg_coefs_dalpha of pgbp_fam_dev.hpp) gives dR[colour], dmu,
// dtheta and dalpha.  e, M, j, G_V and g_w are formed by fam_score_T and fam_score_gv of that header, the body this kernel
// shares with edge_family (pgbp_edge.hip); the slot, the alpha term and the chain-rule coefficients are this kernel's own.
//
// Stage 1 (grad_family): one workgroup per (family, site) solves the family's cluster in LDS (mom_solve: Sigma never leaves
// the LDS) and writes the family's slot [G_V (p*p) | g_w (p) | dalpha term | c_mu | c_theta | c_R[n_rates]]: the matrices once
// and the scalar chain-rule coefficients beside them, so that the slot does not grow with the number of rates.  With tip noise
// set (pgbp_lg_set_tip_noise) the slot carries one more coefficient behind c_R: scale_f of a noisy tip family (else 0), and the
// reduction one more p x p block, dsigma_e = sum_f scale_f G_V(f) (pgbp_lg_gradient_noise): Sigma_e is reduced as one more rate.
// With painted optima in force under OU (pgbp_lg_set_optima) w is sum_k wc_k theta_{r(f,k)} (fam_score_T), the dalpha term of
// edge k uses theta_{r(f,k)}, c_theta sums wc_k over the unpainted edges only, and the slot carries one coefficient per regime
// behind the others: doptima[r] = sum_f (sum over the edges of regime r of wc_k) g_w(f), one more block of the reduction
// (pgbp_lg_gradient_optima).
// Stage 2 (grad_reduce_blocks, grad_reduce_final): the slots are added in a FIXED order -- 256 consecutive families per
// workgroup, four lanes of 64 families each in family order, the four lanes added in lane order, then the block partials by a
// fixed tree -- no floating-point atomics: two calls return the same bytes.  The slots of a chunk of sites at a time
// (256 MB at most), as pgbp_bm_exact_stats bounds its scratch.
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

extern __shared__ double grad_lds[];

constexpr int kGradFamBlock = 256;   // families per workgroup of the first reduction

// LDS of grad_family: fam_score's arrays with three more rows of coefficients, the alpha-derivatives dqc, dvc, dwc
constexpr int kGradRows = 6;

template <int NT>
__global__ __launch_bounds__(NT) void grad_family(const double* __restrict__ pool, int64_t pool_stride,
                                                  const int64_t* __restrict__ boff, const int32_t* __restrict__ bdim, int bs,
                                                  int fp, LgStatic F, LgParams M, LgShifts Sh, LgOptima Op, LgNoise Nz,
                                                  const int32_t* __restrict__ fam_cluster,
                                                  int n_fam, int site0, int n_sites, double* __restrict__ slots,
                                                  int32_t* __restrict__ info, int info0) {
#pragma clang fp contract(off)
  const int t = threadIdx.x, f = blockIdx.x;
  const int p = F.p, K = F.K, np = F.n_parents[f], nn = np + 1, nr = F.n_rates;
  const int c = fam_cluster[f], m = bdim[c], ld = (m + 1) | 1;
  const unsigned long long full = p >= 64 ? ~0ull : ((1ull << p) - 1ull);
  const unsigned long long O = F.child_mask ? (F.child_mask[f] & full) : full;
  const int mo = __popcll(O);
  const int cpos = F.child_pos[f];
  // with tip noise set the slot carries one more coefficient behind those of the rates: scale_f of a noisy tip family (else
  // 0), the weight of G_V in dsigma_e -- Sigma_e is reduced as one more rate
  const int nrs = nr + (Nz.slot ? 1 : 0);
  // with painted optima in force (pgbp_lg_set_optima) one more coefficient per regime behind those: the sum of wc_k over the
  // family's edges of that regime, the weight of g_w in doptima[regime]
  const int nopt = Op.regime ? Op.n : 0;
  const int sl = p * p + p + 3 + nrs + nopt;
  const int DA = p * p + p, CMU = DA + 1, CTH = DA + 2, CR = DA + 3;
  const FamLds L = fam_carve(grad_lds, m, p, K, kGradRows, 0);
  const int ldv = fam_ldv(p);
  double* cf = L.cf;   // rows of K: qc, vc, wc, dqc, dvc, dwc
  bool any_scope = cpos >= 0;
  for (int k = 0; k < np; ++k) any_scope |= F.parent_pos[(size_t)f * K + k] >= 0;
  // families the factor fill skips contribute nothing (and a root-prior family of a fixed root, which has no factor)
  const bool skip = mo == 0 || (np == 0 && cpos < 0);
  const bool packed = bs && bs16::applies(m, fp);
  const bool ou = M.model == PGBP_LG_OU;
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    double* __restrict__ o = slots + ((int64_t)site * n_fam + f) * sl;
    if (skip) {
      for (int a = t; a < sl; a += NT) o[a] = 0.0;
      continue;
    }
    const int64_t as = site0 + site;
    const LgSite S = lg_site(M, nr, p, as);
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
    // (the fill made this cluster's g NaN): the site's sums are NaN
    if (st == 0) {
      for (int k = t; k < np; k += NT)
        lg_coefs_dalpha(M.model, S.alpha, F.length[(size_t)f * K + k], F.gamma[(size_t)f * K + k], cf[3 * K + k], cf[4 * K + k],
                        cf[5 * K + k]);
      if (!fam_score_T_opt<NT, true>(L, F, M, Sh, Op, Nz, S, f, m, O, as, t)) st = 1;
    }
    if (st != 0) {
      for (int a = t; a < sl; a += NT) o[a] = NAN;
      if (t == 0) atomicMin(info + info0 + site, c + 1);
      continue;
    }
    for (int a = t; a < DA; a += NT) o[a] = 0.0;   // (the entries outside O)
    // G_V embedded into p x p, and kept in Mx for the alpha term; g_w = j e
    fam_score_gv<NT>(L, p, mo, o, t);
    for (int i = t; i < mo; i += NT) o[p * p + L.oidx[i]] = L.ge[i];
    __syncthreads();
    if (t == 0) {
      double cmu = 0.0, cth = 0.0, da = 0.0;
      if (np == 0) {
        cmu = 1.0;
      } else {
        for (int k = 0; k < np; ++k) {
          if (L.ipos[k + 1] < 0) cmu = cmu - fam_c(cf, k + 1);   // qc_k: the parent is the fixed root
          if (!Op.regime || Op.regime[(size_t)f * K + k] <= 0) cth = cth + cf[2 * K + k];   // theta: the unpainted edges
        }
        if (ou) {
          for (int k = 0; k < np; ++k) {
            const double* __restrict__ Rk = S.R + (int64_t)F.color[(size_t)f * K + k] * p * p;
            // the optimum of this edge: theta, or the value of its regime
            const int rk = Op.regime ? Op.regime[(size_t)f * K + k] : 0;
            const double* __restrict__ thk = rk > 0 ? Op.value + ((Op.per_site ? as * Op.n : 0) + (rk - 1)) * p : S.theta;
            double trGR = 0.0, thg = 0.0, gq = 0.0;
            for (int i = 0; i < mo; ++i) {
              for (int l = 0; l < mo; ++l) {
                trGR = trGR + L.Mx[i * mo + l] * Rk[L.oidx[l] + L.oidx[i] * p];
                // E[r x_k'](i, l) = sum_a c_a Sigma(a_i, k_l) + e_i m_k(l)
                double ex = L.ev[i] * L.xm[(k + 1) * p + l];
                const int vk = L.vi[(k + 1) * p + l];
                if (vk >= 0) {
                  for (int a = 0; a < nn; ++a) {
                    const int va = L.vi[a * p + i];
                    if (va >= 0) ex = ex + fam_c(cf, a) * (va >= vk ? L.W[va * ld + vk] : L.W[vk * ld + va]);
                  }
                }
                gq = gq + fam_j(L.A, ldv, mo, l, i) * ex;
              }
              if (thk) thg = thg + thk[L.oidx[i]] * L.ge[i];
            }
            da = da + cf[4 * K + k] * trGR + cf[5 * K + k] * thg + cf[3 * K + k] * gq;
          }
        }
      }
      o[DA] = da;
      o[CMU] = cmu;
      o[CTH] = cth;
    }
    for (int r = t; r < nrs; r += NT) {
      double cr = 0.0;
      if (r == nr) {
        const int sn = Nz.slot[f];
        cr = sn >= 0 ? Nz.scale[sn] : 0.0;
      } else if (np == 0) {
        cr = F.color[(size_t)f * K] == r ? 1.0 : 0.0;
      } else {
        for (int k = 0; k < np; ++k)
          if (F.color[(size_t)f * K + k] == r) cr = cr + cf[K + k];
      }
      o[CR + r] = cr;
    }
    for (int r = t; r < nopt; r += NT) {
      double co = 0.0;
      for (int k = 0; k < np; ++k)
        if (Op.regime[(size_t)f * K + k] == r + 1) co = co + cf[2 * K + k];
      o[CR + nrs + r] = co;
    }
  }
}

// entry en of a site's gradient [dR (n_rates * p*p) | dmu (p) | dtheta (p) | dalpha | doptima (n_regimes * p)] as this
// family's slot gives it
__device__ __forceinline__ double grad_entry(const double* __restrict__ o, int en, int p, int nr) {
#pragma clang fp contract(off)
  const int pp = p * p, DA = pp + p;
  if (en < nr * pp) {
    const int r = en / pp;
    return o[en - r * pp] * o[DA + 3 + r];
  }
  en -= nr * pp;
  if (en < p) return o[pp + en] * o[DA + 1];
  en -= p;
  if (en < p) return o[pp + en] * o[DA + 2];
  if (en == p) return o[DA];
  en -= p + 1;   // doptima[r][trait] = g_w[trait] * (the slot's coefficient of regime r)
  const int r = en / p;
  return o[pp + en - r * p] * o[DA + 3 + nr + r];
}

// partial[site][block][entry]: kGradFamBlock consecutive families, lane q = t / 64 adds its 64 families in family order,
// the four lanes are added in lane order
__global__ __launch_bounds__(256) void grad_reduce_blocks(const double* __restrict__ slots, int n_fam, int p, int nr, int nopt,
                                                          int n_ent, int n_sites, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int t = threadIdx.x, el = t & 63, q = t >> 6;
  const int en = blockIdx.x * 64 + el, fb = blockIdx.y, nfb = gridDim.y;
  const int sl = p * p + p + 3 + nr + nopt;
  for (int site = blockIdx.z; site < n_sites; site += gridDim.z) {
    double acc = 0.0;
    if (en < n_ent) {
      const int f0 = fb * kGradFamBlock + q * 64;
      const int f1 = min(f0 + 64, n_fam);
      for (int f = f0; f < f1; ++f) acc = acc + grad_entry(slots + ((int64_t)site * n_fam + f) * sl, en, p, nr);
    }
    __syncthreads();
    part[t] = acc;
    __syncthreads();
    if (q == 0 && en < n_ent)
      partial[((int64_t)site * nfb + fb) * n_ent + en] = ((part[el] + part[64 + el]) + part[128 + el]) + part[192 + el];
  }
}

__global__ __launch_bounds__(256) void grad_reduce_final(const double* __restrict__ partial, int nfb, int n_ent, int n_sites,
                                                         double* __restrict__ out, int out0) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const int t = threadIdx.x, en = blockIdx.x;
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    double acc = 0.0;
    for (int b = t; b < nfb; b += 256) acc = acc + partial[((int64_t)site * nfb + b) * n_ent + en];
    __syncthreads();
    part[t] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) part[t] = part[t] + part[t + w];
      __syncthreads();
    }
    if (t == 0) out[(int64_t)(out0 + site) * n_ent + en] = part[0];
  }
}

}  // namespace pgbp

using namespace pgbp;

static int lg_gradient(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu, double* dalpha,
                       double* dtheta, double* dsigma_e, double* doptima, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const LgModel* L = nullptr;
  int rc = lg_sweep_state(e, "pgbp_lg_gradient", site_begin, site_end, &L, "pgbp_lg_gradient_sites");
  if (rc) return rc;
  if ((rc = lg_refuse_clade_shifts(e, "pgbp_lg_gradient", L))) return rc;
  const LgStatic& F = L->F;
  const LgParams& M = L->M;
  const LgShifts& Sh = L->Sh;
  const LgNoise& Nz = L->Nz;
  LgOptima Op = L->optima_in_force();
  Op.value_sm = nullptr;   // (the [regime][site] rows are for lanes = sites)
  const int nopt = Op.regime ? Op.n : 0, nopt_out = L->Op.regime ? L->Op.n : 0;
  // painted optima change dtheta and dalpha: a caller that cannot take doptima would read them as the unpainted model's
  if (nopt > 0 && !doptima)
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_gradient: painted optima are in force (pgbp_lg_set_optima): use "
                                            "pgbp_lg_gradient_optima, which returns doptima");
  if (!dR || !dmu) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_gradient: no output buffer");
  if (M.model == PGBP_LG_OU && (!dalpha || !dtheta))
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_gradient: the OU model needs dalpha and dtheta");
  EngineView v;
  if ((rc = engine_view(e, &v))) return rc;
  // (as in pgbp_bm_exact_stats, what follows runs on the caller's current device: an engine of a multi-device group is
  // swept from the thread that has its device current)
  const Plan& pl = *v.plan;
  const int p = F.p, K = F.K, nr0 = F.n_rates;
  const int nr = nr0 + (Nz.slot ? 1 : 0);   // the slots and the reduction carry Sigma_e as one more rate (grad_family)
  const std::vector<int32_t>& fcl = L->T.cluster;   // which cluster each family sits in
  int max_m = 0;
  std::string why;
  if (!L->T.cluster_dims("pgbp_lg_gradient", kLdsMaxDim, &max_m, why)) return engine_fail(e, PGBP_ERR_INVALID, why);
  const int nf = L->T.n_families;
  const size_t lds_bytes = fam_score_lds_bytes(max_m, p, K, kGradRows, 0);
  if (lds_bytes > 160 * 1024)
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_gradient: a cluster of " + std::to_string(max_m) + " variables with " +
                                                std::to_string(p) + " traits needs " + std::to_string(lds_bytes) +
                                                " bytes of LDS, more than the 160 KB of a compute unit");
  const int ns = site_end - site_begin;
  if (ns == 0) return PGBP_OK;
  const bool ou = M.model == PGBP_LG_OU;
  const int pp = p * p, n_ent = nr * pp + 2 * p + 1 + nopt * p;
  auto scatter = [&](const double* src, const int32_t* inf) {   // a site's [dR | dmu | dtheta | dalpha] to the caller's arrays
    for (int s = 0; s < ns; ++s) {
      const bool bad = inf && inf[s] != 0;
      const double* g = src ? src + (size_t)s * n_ent : nullptr;
      for (int a = 0; a < nr0 * pp; ++a) dR[(size_t)s * nr0 * pp + a] = bad ? NAN : (g ? g[a] : 0.0);
      if (dsigma_e)
        for (int a = 0; a < pp; ++a) dsigma_e[(size_t)s * pp + a] = bad ? NAN : ((g && nr > nr0) ? g[nr0 * pp + a] : 0.0);
      for (int a = 0; a < p; ++a) dmu[(size_t)s * p + a] = bad ? NAN : (g ? g[nr * pp + a] : 0.0);
      if (dtheta)
        for (int a = 0; a < p; ++a) dtheta[(size_t)s * p + a] = bad ? NAN : ((g && ou) ? g[nr * pp + p + a] : 0.0);
      if (dalpha) dalpha[s] = bad ? NAN : ((g && ou) ? g[nr * pp + 2 * p] : 0.0);
      if (doptima)   // (set under BM: the optima have no effect, their derivative is 0)
        for (int a = 0; a < nopt_out * p; ++a)
          doptima[(size_t)s * nopt_out * p + a] = bad ? NAN : ((g && nopt > 0) ? g[nr * pp + 2 * p + 1 + a] : 0.0);
      if (info) info[s] = inf ? inf[s] : 0;
    }
  };
  if (nf == 0) {
    scatter(nullptr, nullptr);
    return PGBP_OK;
  }
  const int sl = pp + p + 3 + nr + nopt;
  const int64_t per_site = (int64_t)nf * sl;
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(ns, ((int64_t)32 << 20) / per_site));
  const int nfb = (nf + kGradFamBlock - 1) / kGradFamBlock;
  std::vector<int32_t> inf(ns, 0x7fffffff);   // (ahead of the buffers: they are released, which drains the uploads, first)
  std::vector<double> out((size_t)ns * n_ent);
  DevBuf<int32_t> d_fcl, d_info;
  DevBuf<double> d_slots, d_part, d_out;
  hipError_t herr = (hipError_t)d_fcl.alloc(nf);
  if (herr == hipSuccess) herr = (hipError_t)d_slots.alloc((size_t)per_site * chunk);
  if (herr == hipSuccess) herr = (hipError_t)d_part.alloc((size_t)chunk * nfb * n_ent);
  if (herr == hipSuccess) herr = (hipError_t)d_out.alloc((size_t)ns * n_ent);
  if (herr == hipSuccess) herr = (hipError_t)d_info.alloc((size_t)ns);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_fcl.get(), fcl.data(), sizeof(int32_t) * nf, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_info.get(), inf.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice, v.st);
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_gradient (scratch): ") + hipGetErrorString(herr));
  (void)hipGetLastError();   // (an error an earlier asynchronous call left behind is that call's to report)
  {
    const void* kern = max_m <= 64 ? reinterpret_cast<const void*>(grad_family<64>) : reinterpret_cast<const void*>(grad_family<256>);
    if (lds_bytes > 64 * 1024) herr = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    for (int s0 = 0; herr == hipSuccess && s0 < ns; s0 += chunk) {
      const int n = std::min(chunk, ns - s0), gy = std::min(n, 65535);
      if (max_m <= 64)
        hipLaunchKernelGGL(grad_family<64>, dim3(nf, gy), dim3(64), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, Op, Nz, d_fcl.get(), nf, site_begin + s0, n, d_slots.get(), d_info.get(), s0);
      else
        hipLaunchKernelGGL(grad_family<256>, dim3(nf, gy), dim3(256), lds_bytes, v.st, v.pool, pl.pool_stride(), v.boff, v.bdim,
                           v.bs16, pl.fast_p, F, M, Sh, Op, Nz, d_fcl.get(), nf, site_begin + s0, n, d_slots.get(), d_info.get(), s0);
      hipLaunchKernelGGL(grad_reduce_blocks, dim3((n_ent + 63) / 64, nfb, gy), dim3(256), 0, v.st, d_slots.get(), nf, p, nr, nopt, n_ent, n,
                         d_part.get());
      hipLaunchKernelGGL(grad_reduce_final, dim3(n_ent, gy), dim3(256), 0, v.st, d_part.get(), nfb, n_ent, n, d_out.get(), s0);
    }
    if (herr == hipSuccess) herr = hipGetLastError();
  }
  if (herr == hipSuccess) herr = hipMemcpyAsync(out.data(), d_out.get(), sizeof(double) * out.size(), hipMemcpyDeviceToHost, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(inf.data(), d_info.get(), sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, v.st);
  const hipError_t serr = hipStreamSynchronize(v.st);
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, std::string("pgbp_lg_gradient: ") + hipGetErrorString(herr));
  for (int s = 0; s < ns; ++s) inf[s] = inf[s] == 0x7fffffff ? 0 : inf[s];
  scatter(out.data(), inf.data());
  return PGBP_OK;
}

extern "C" int pgbp_lg_gradient(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu, double* dalpha,
                                double* dtheta, int32_t* info) {
  return lg_gradient(e, site_begin, site_end, dR, dmu, dalpha, dtheta, nullptr, nullptr, info);
}

extern "C" int pgbp_lg_gradient_noise(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu,
                                      double* dalpha, double* dtheta, double* dsigma_e, int32_t* info) {
  return lg_gradient(e, site_begin, site_end, dR, dmu, dalpha, dtheta, dsigma_e, nullptr, info);
}

extern "C" int pgbp_lg_gradient_optima(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu,
                                       double* dalpha, double* dtheta, double* dsigma_e, double* doptima, int32_t* info) {
  if (e && !doptima && pgbp_lg_optima_count(e) > 0)
    return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_gradient_optima: no output buffer (doptima)");
  return lg_gradient(e, site_begin, site_end, dR, dmu, dalpha, dtheta, dsigma_e, doptima, info);
}

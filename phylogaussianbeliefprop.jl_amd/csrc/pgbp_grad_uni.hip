// The gradient sweep of pgbp_grad.hip for univariate batches on a thread-per-site engine (pgbp_lg_gradient_sites of
// include/pgbp.h): p = 1, every belief of at most 2 variables, at least 8 sites.  Lanes are sites: a workgroup is 256
// consecutive sites, grid.y a block of kFamUniBlock consecutive families, a thread walks its block's families in index
// order for its one site.  The family table is uniform across a wavefront (scalar loads); the belief entries and the tip data
// are read as whole lines in the layout the pool is in (site-minor from 64 sites on, plain below: grad_uni_family<SM>), so the
// call converts nothing and leaves the layout as it found it.
//
// Per (family, site) everything is closed form.  Notation of pgbp_grad.hip: r = sum_a c_a x_a - w with c_0 = 1 (child),
// c_k = -qc_k.  The blocks in scope are variables of a cluster of at most 2, so r = u_0 x_0 + u_1 x_1 + const - w with u_v the
// sum of the c_a that sit at variable v, and with Sigma = J^-1, m = Sigma h of the cluster:
//   e = u'm + const - w,  Cov(r) = u' Sigma u,  M = Cov(r) + e^2,  V = sum_k vc_k R[colour_k] (+ E_f),  j = 1 / V,
//   G_V = (j M j - j) / 2,  g_w = j e,  g_qk = j (e x_k + (Sigma u)[v_k])   (x_k: the parent's mean, or mu of the fixed root).
// The alpha term sum_k (dvc_k R_k G_V + dwc_k theta g_w + dqc_k g_qk) is linear in per-parent sums, so one pass over the
// parents is enough.  Coefficients, shift and noise from lg_coefs<false>, lg_coefs_dalpha, lg_shift_d and lg_noise_E.
//
// Reduction: each thread writes its block's partial sums to partial[family block][entry][site]; grad_uni_reduce adds the
// blocks in index order.  No atomics, contraction off, every sum in a fixed order: the bytes of a site depend neither on the
// call nor on the site range it came in.  A launch carries kGradUniRates rates in registers; a model with more rates is swept
// once per group of rates (the scalar entries with the first).  The partials of a chunk of sites at a time (256 MB at most,
// whole workgroups: pgbp_sites_sweep_scratch_limit).  Host frame of pgbp_sites_host.hpp, moments of pgbp_fam_uni_dev.hpp.
// A lane whose cluster or variance is not positive definite records the 1-based cluster index and adds nothing; there is no
// barrier in either kernel, and no lane's store depends on another lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "pgbp_devmem.hpp"
#include "pgbp_fam_uni_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"
#include "pgbp_sites_host.hpp"

namespace pgbp {

constexpr int kGradUniRates = 4;    // rates a launch accumulates in registers
constexpr int kGradUniOptima = 4;   // regimes a launch of the painted instance accumulates in registers

// entries of a site's gradient: [dR (n_rates) | dsigma_e | dmu | dtheta | dalpha | doptima (n_regimes)]
__host__ __device__ inline int grad_uni_entries(int nr, int nopt = 0) { return nr + 4 + nopt; }

// partial: [blocks][entries][part_row], pinfo: [blocks][part_row] (written by the launch of the first rates, r0 == 0).  The
// members of SitesArgs as a flat list: with the struct the kernel keeps its 129 VGPRs but spills 24 more SGPRs into them.
//
// OPT: the instance for painted optima under OU (pgbp_lg_set_optima; pgbp_lg_gradient_sites_optima).  The regime of an edge is
// uniform across the wavefront (scalar loads); its optimum theta_r is a whole line of the [regime][site] rows, or one scalar
// when the values are shared.  w = sum_k wc_k theta_{r(f,k)}, the dwc term of dalpha uses theta_{r(f,k)}, dtheta sums wc_k
// over the unpainted edges, and doptima[r] = sum over the edges of regime r of wc_k g_w: kGradUniOptima regimes from g0 on in
// registers per launch, entries [nr + 4 + r] of the partial sums.  The instance without optima is the kernel as it was: every
// painted statement is under `if constexpr (OPT)`.
template <bool SM, bool OPT>
__device__ __forceinline__ void grad_uni_family_body(const double* __restrict__ pool, int64_t stride,
                                                     const int64_t* __restrict__ off, const int32_t* __restrict__ bdim,
                                                     const LgStatic& F, const LgParams& M, const LgShifts& Sh, const LgNoise& Nz,
                                                     const LgSiteMiss& Ms, const LgOptima& Op,
                                                     const int32_t* __restrict__ fam_cluster, int n_fam, int64_t data_row_len,
                                                     int site0, int n_sites, int r0, int g0, int64_t part_row,
                                                     double* __restrict__ partial, int32_t* __restrict__ pinfo) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x, fb = blockIdx.y;
  if (s >= n_sites) return;   // (a lane past the range: no barrier follows, and no other lane's store is its to make)
  const int64_t as = (int64_t)site0 + s;
  const int K = F.K, nr = F.n_rates;
  const bool ou = M.model == PGBP_LG_OU;
  const LgSite S = lg_site(M, nr, 1, as);
  const double mu = S.mu[0], theta = S.theta ? S.theta[0] : 0.0;
  double accR[kGradUniRates];
#pragma unroll
  for (int i = 0; i < kGradUniRates; ++i) accR[i] = 0.0;
  double dsig = 0.0, dmu = 0.0, dth = 0.0, da = 0.0;
  double accO[OPT ? kGradUniOptima : 1];
#pragma unroll
  for (int i = 0; i < (OPT ? kGradUniOptima : 1); ++i) accO[i] = 0.0;
  const int nopt = OPT ? Op.n : 0;
  int bad = kFamUniNoInfo;
  const int f0 = fb * kFamUniBlock, f1 = min(f0 + kFamUniBlock, n_fam);
  for (int f = f0; f < f1; ++f) {
    const int np = F.n_parents[f], cpos = F.child_pos[f];
    // families the factor fill skips contribute nothing (and a root-prior family of a fixed root, which has no factor)
    if (F.child_mask && !(F.child_mask[f] & 1ull)) continue;
    if (np == 0 && cpos < 0) continue;
    // u and the constant part of the child; a tip the per-site mask says is not observed at this site is skipped as above
    double u0 = 0.0, u1 = 0.0, cst = 0.0;
    if (cpos == 0) u0 = 1.0;
    else if (cpos == 1) u1 = 1.0;
    else if (F.data_row[f] >= 0) {   // a tip: its data row, [row][site] where the engine keeps that copy
      const int row = F.data_row[f];
      if (np > 0 && lg_site_masked(Ms, row, as)) continue;
      cst = F.data_sm ? F.data_sm[(int64_t)row * data_row_len + as] : F.data[as * F.n_rows + row];
    }
    const int c = fam_cluster[f];
    bool any_scope = cpos >= 0;
    for (int k = 0; k < np; ++k) any_scope |= F.parent_pos[(size_t)f * K + k] >= 0;
    // moments of the cluster (no variable in scope: none are needed)
    FamUniMom q{0.0, 0.0, 0.0, 0.0, 0.0, 0, true};
    if (any_scope) q = fam_uni_moments<SM>(pool, stride, off[c], bdim[c], as);
    const double S00 = q.S00, S01 = q.S01, S11 = q.S11, m0 = q.m0, m1 = q.m1;
    bool ok = q.ok;
    // one pass over the blocks: V, w, the rest of u and of the constant part, the chain-rule coefficients and the sums of
    // the alpha term
    double V = 0.0, w = 0.0, cmu = 0.0, cth = 0.0;
    double A1 = 0.0, A2 = 0.0, A3 = 0.0, D0 = 0.0, D1 = 0.0;   // sum dvc R_k, sum dwc, sum dqc x_k, sum dqc at variable 0 / 1
    double cr[kGradUniRates];
#pragma unroll
    for (int i = 0; i < kGradUniRates; ++i) cr[i] = 0.0;
    double co[OPT ? kGradUniOptima : 1];   // sum of wc_k over the edges of regime g0 + 1 + i
#pragma unroll
    for (int i = 0; i < (OPT ? kGradUniOptima : 1); ++i) co[i] = 0.0;
    if (np == 0) {
      const int col = F.color[(size_t)f * K];
      V = S.R[col];
      w = mu;
      cmu = 1.0;
#pragma unroll
      for (int i = 0; i < kGradUniRates; ++i)
        if (col == r0 + i) cr[i] = 1.0;
    } else {
      for (int k = 0; k < np; ++k) {
        const double len = F.length[(size_t)f * K + k], gam = F.gamma[(size_t)f * K + k];
        const int col = F.color[(size_t)f * K + k], pk = F.parent_pos[(size_t)f * K + k];
        double qc, vc, wc, dqc, dvc, dwc;
        lg_coefs<false>(M.model, S.alpha, len, gam, qc, vc, wc);
        lg_coefs_dalpha(M.model, S.alpha, len, gam, dqc, dvc, dwc);
        const double Rk = S.R[col];
        V = V + vc * Rk;
        A1 = A1 + dvc * Rk;
        if constexpr (OPT) {
          const int rk = Op.regime[(size_t)f * K + k];   // (uniform across the wavefront)
          double thk = theta;
          if (rk > 0) thk = Op.value_sm ? Op.value_sm[(int64_t)(rk - 1) * data_row_len + as] : Op.value[rk - 1];
          else cth = cth + wc;
          w = w + wc * thk;
          A2 = A2 + dwc * thk;   // (the optimum inside the sum: it differs by edge)
#pragma unroll
          for (int i = 0; i < kGradUniOptima; ++i)
            if (rk == g0 + 1 + i) co[i] = co[i] + wc;
        } else {
          cth = cth + wc;
          if (S.theta) w = w + wc * theta;
          A2 = A2 + dwc;
        }
        if (pk == 0) {
          u0 = u0 - qc;
          D0 = D0 + dqc;
          A3 = A3 + dqc * m0;
        } else if (pk == 1) {
          u1 = u1 - qc;
          D1 = D1 + dqc;
          A3 = A3 + dqc * m1;
        } else {   // the fixed root
          cst = cst - qc * mu;
          cmu = cmu + qc;
          A3 = A3 + dqc * mu;
        }
#pragma unroll
        for (int i = 0; i < kGradUniRates; ++i)
          if (col == r0 + i) cr[i] = cr[i] + vc;
      }
      if (Sh.slot) w = w + lg_shift_d(Sh, F.gamma, f, K, np, 0, 1, as);   // a shift of the mean on a parent edge
    }
    const int sn = lg_noise_slot(Nz, f);
    if (sn >= 0) V = V + lg_noise_E(Nz, sn, 0, 0, 1, as);   // a noisy tip: V + E
    ok = ok && V > 0.0;
    const double e = (u0 * m0 + u1 * m1 + cst) - w;
    const double su0 = S00 * u0 + S01 * u1, su1 = S01 * u0 + S11 * u1;   // Sigma u
    const double Mx = (u0 * su0 + u1 * su1) + e * e;
    const double j = 1.0 / V;
    const double ge = j * e;
    const double G = 0.5 * ((j * Mx) * j - j);
    if (ok) {
#pragma unroll
      for (int i = 0; i < kGradUniRates; ++i) accR[i] = accR[i] + G * cr[i];
      if (sn >= 0) dsig = dsig + G * Nz.scale[sn];
      dmu = dmu + ge * cmu;
      dth = dth + ge * cth;
      if constexpr (OPT) {
#pragma unroll
        for (int i = 0; i < kGradUniOptima; ++i) accO[i] = accO[i] + ge * co[i];
        da = da + ((A1 * G + A2 * ge) + j * (e * A3 + (D0 * su0 + D1 * su1)));
      } else {
        if (ou) da = da + ((A1 * G + A2 * (theta * ge)) + j * (e * A3 + (D0 * su0 + D1 * su1)));
      }
    } else {
      bad = min(bad, c + 1);
    }
  }
  const int n_ent = grad_uni_entries(nr, nopt);
  double* __restrict__ o = partial + (int64_t)fb * n_ent * part_row + s;
#pragma unroll
  for (int i = 0; i < kGradUniRates; ++i)
    if (r0 + i < nr) o[(int64_t)(r0 + i) * part_row] = accR[i];
  if (r0 == 0) {
    o[(int64_t)nr * part_row] = dsig;
    o[(int64_t)(nr + 1) * part_row] = dmu;
    o[(int64_t)(nr + 2) * part_row] = dth;
    o[(int64_t)(nr + 3) * part_row] = da;
    pinfo[(int64_t)fb * part_row + s] = bad;
  }
  if constexpr (OPT) {
#pragma unroll
    for (int i = 0; i < kGradUniOptima; ++i)
      if (g0 + i < nopt) o[(int64_t)(nr + 4 + g0 + i) * part_row] = accO[i];
  }
}

template <bool SM>
__global__ __launch_bounds__(256) void grad_uni_family(const double* __restrict__ pool, int64_t stride,
                                                       const int64_t* __restrict__ off, const int32_t* __restrict__ bdim,
                                                       LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz, LgSiteMiss Ms,
                                                       const int32_t* __restrict__ fam_cluster, int n_fam, int64_t data_row_len,
                                                       int site0, int n_sites, int r0, int64_t part_row,
                                                       double* __restrict__ partial, int32_t* __restrict__ pinfo) {
  grad_uni_family_body<SM, false>(pool, stride, off, bdim, F, M, Sh, Nz, Ms, LgOptima{}, fam_cluster, n_fam, data_row_len, site0,
                                  n_sites, r0, 0, part_row, partial, pinfo);
}

// the painted instance: launch l carries the rates from l * kGradUniRates and the regimes from l * kGradUniOptima on
template <bool SM>
__global__ __launch_bounds__(256) void grad_uni_family_optima(const double* __restrict__ pool, int64_t stride,
                                                              const int64_t* __restrict__ off, const int32_t* __restrict__ bdim,
                                                              LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz, LgSiteMiss Ms,
                                                              LgOptima Op, const int32_t* __restrict__ fam_cluster, int n_fam,
                                                              int64_t data_row_len, int site0, int n_sites, int r0, int g0,
                                                              int64_t part_row, double* __restrict__ partial,
                                                              int32_t* __restrict__ pinfo) {
  grad_uni_family_body<SM, true>(pool, stride, off, bdim, F, M, Sh, Nz, Ms, Op, fam_cluster, n_fam, data_row_len, site0, n_sites, r0,
                                 g0, part_row, partial, pinfo);
}

// out[entry][out0 + site] = the blocks' partials added in index order; info[out0 + site] = the smallest mark of a block, 0: none
__global__ __launch_bounds__(256) void grad_uni_reduce(const double* __restrict__ partial, const int32_t* __restrict__ pinfo,
                                                       int nfb, int n_ent, int n_sites, int64_t part_row,
                                                       double* __restrict__ out, int32_t* __restrict__ info, int out0,
                                                       int64_t out_row) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x, en = blockIdx.y;
  if (s >= n_sites) return;
  if (en < n_ent) {
    double acc = 0.0;
    for (int b = 0; b < nfb; ++b) acc = acc + partial[((int64_t)b * n_ent + en) * part_row + s];
    out[(int64_t)en * out_row + out0 + s] = acc;
  } else {
    int bad = kFamUniNoInfo;
    for (int b = 0; b < nfb; ++b) bad = min(bad, pinfo[(int64_t)b * part_row + s]);
    info[out0 + s] = bad == kFamUniNoInfo ? 0 : bad;
  }
}

}  // namespace pgbp

using namespace pgbp;

static int lg_gradient_sites(pgbp_engine* e, const char* fn, int32_t site_begin, int32_t site_end, double* dR, double* dmu,
                             double* dalpha, double* dtheta, double* dsigma_e, double* doptima, bool takes_optima, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  SitesCall c{};
  int rc = sites_accept_state(e, fn, site_begin, site_end, &c);
  if (rc) return rc;
  const LgModel* L = c.L;
  if ((rc = lg_refuse_clade_shifts(e, fn, L))) return rc;   // (grad_uni_family does not know the per-site membership)
  const LgOptima Op = L->optima_in_force();
  const int nopt = Op.regime ? Op.n : 0, nopt_out = L->Op.regime ? L->Op.n : 0;
  // painted optima change dtheta and dalpha: a caller that cannot take doptima would read them as the unpainted model's
  if (nopt > 0 && !takes_optima)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": painted optima are in force (pgbp_lg_set_optima): use "
                                                "pgbp_lg_gradient_sites_optima, which returns doptima");
  if (nopt_out > 0 && takes_optima && !doptima) return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": no output buffer (doptima)");
  if (!dR || !dmu) return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": no output buffer");
  const bool ou = L->M.model == PGBP_LG_OU;
  if (ou && (!dalpha || !dtheta)) return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": the OU model needs dalpha and dtheta");
  if ((rc = sites_accept_engine(e, fn, "pgbp_lg_gradient", c))) return rc;
  const int ns = c.ns;
  if (ns == 0) return PGBP_OK;
  const int nr = L->F.n_rates, nf = L->T.n_families;
  const int n_ent = grad_uni_entries(nr, nopt);
  const int nfb = std::max(1, (nf + kFamUniBlock - 1) / kFamUniBlock);
  const int chunk = fam_uni_chunk(ns, (int64_t)nfb * n_ent);   // the partials of a chunk of sites at a time
  std::vector<double> out((size_t)n_ent * ns);
  std::vector<int32_t> inf(ns, 0);
  DevBuf<int32_t> d_fcl, d_pinfo, d_info;
  DevBuf<double> d_part, d_out;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_fcl, std::max(1, nf));
  S.alloc(d_part, (size_t)nfb * n_ent * chunk);
  S.alloc(d_pinfo, (size_t)nfb * chunk);
  S.alloc(d_out, (size_t)n_ent * ns);
  S.alloc(d_info, ns);
  S.upload(d_fcl, L->T.cluster.data(), nf);
  if ((rc = S.ready())) return rc;
  for (int s0 = 0; S.ok() && s0 < ns; s0 += chunk) {
    const int n = std::min(chunk, ns - s0);
    const SitesArgs A = sites_args(c, site_begin + s0, n, chunk, d_fcl.get());
    const dim3 grid((n + 255) / 256, nfb);
    if (nopt == 0) {
      for (int r0 = 0; r0 == 0 || r0 < nr; r0 += kGradUniRates)
        PGBP_SITES_LAUNCH(S, c.U.sm, grad_uni_family, grid, A.pool, A.stride, A.off, A.bdim, L->F, L->M, L->Sh, L->Nz, L->Ms, A.fam_cluster, nf,
                          A.data_row_len, A.site0, A.n_sites, r0, A.row, d_part.get(), d_pinfo.get());
    } else {   // the painted instance: rates and regimes in groups, side by side
      for (int r0 = 0, g0 = 0; r0 == 0 || r0 < nr || g0 < nopt; r0 += kGradUniRates, g0 += kGradUniOptima)
        PGBP_SITES_LAUNCH(S, c.U.sm, grad_uni_family_optima, grid, A.pool, A.stride, A.off, A.bdim, L->F, L->M, L->Sh, L->Nz, L->Ms, Op,
                          A.fam_cluster, nf, A.data_row_len, A.site0, A.n_sites, r0, g0, A.row, d_part.get(), d_pinfo.get());
    }
    S.launch(grad_uni_reduce, dim3(grid.x, n_ent + 1), d_part.get(), d_pinfo.get(), nfb, n_ent, n, (int64_t)chunk, d_out.get(),
             d_info.get(), s0, (int64_t)ns);
    S.check();
  }
  S.download(out.data(), d_out.get(), out.size());
  S.download(inf.data(), d_info.get(), ns);
  if ((rc = S.finish())) return rc;
  // [entry][site] to the caller's arrays (the layout of pgbp_lg_gradient_noise at p = 1); a failed site holds NaN
  for (int s = 0; s < ns; ++s) {
    const bool bad = inf[s] != 0;
    auto ent = [&](int en) { return bad ? (double)NAN : out[(size_t)en * ns + s]; };
    for (int r = 0; r < nr; ++r) dR[(size_t)s * nr + r] = ent(r);
    if (dsigma_e) dsigma_e[s] = ent(nr);
    dmu[s] = ent(nr + 1);
    if (dtheta) dtheta[s] = bad ? (double)NAN : (ou ? out[(size_t)(nr + 2) * ns + s] : 0.0);
    if (dalpha) dalpha[s] = bad ? (double)NAN : (ou ? out[(size_t)(nr + 3) * ns + s] : 0.0);
    if (doptima)   // (set under BM: the optima have no effect, their derivative is 0)
      for (int r = 0; r < nopt_out; ++r)
        doptima[(size_t)s * nopt_out + r] = bad ? (double)NAN : (nopt > 0 ? out[(size_t)(nr + 4 + r) * ns + s] : 0.0);
    if (info) info[s] = inf[s];
  }
  return PGBP_OK;
}

extern "C" int pgbp_lg_gradient_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu,
                                      double* dalpha, double* dtheta, double* dsigma_e, int32_t* info) {
  return lg_gradient_sites(e, "pgbp_lg_gradient_sites", site_begin, site_end, dR, dmu, dalpha, dtheta, dsigma_e, nullptr, false, info);
}

extern "C" int pgbp_lg_gradient_sites_optima(pgbp_engine* e, int32_t site_begin, int32_t site_end, double* dR, double* dmu,
                                             double* dalpha, double* dtheta, double* dsigma_e, double* doptima, int32_t* info) {
  return lg_gradient_sites(e, "pgbp_lg_gradient_sites_optima", site_begin, site_end, dR, dmu, dalpha, dtheta, dsigma_e, doptima, true,
                           info);
}

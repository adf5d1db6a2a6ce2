// The family sweep of calibrate_exact_cliquetree! (src/calibration.jl:440-499; pgbp_bm_exact_stats of pgbp_moments.hip) for
// univariate batches on a thread-per-site engine, lanes = sites: pgbp_bm_exact_stats_sites of include/pgbp.h, in the frame of
// pgbp_grad_uni.hip -- a workgroup is 256 consecutive sites, grid.y a block of kFamUniBlock consecutive families, a thread walks
// its block's families in index order for its one site.  The family table is uniform across a wavefront (scalar loads); the
// belief entries, the tip data and the per-site mask are read with lanes = sites in the layout the pool is in (site-minor from
// 64 sites on, plain below: template <bool SM>), so the call converts nothing and leaves the layout as it found it.
//
// Per (family, site) that is not skipped, with t = sum_k gamma_k^2 length_k (:459) and the residual of the family
// r = x_child - sum_k gamma_k x_k - d (d: the displacement of the shifts on its parent edges): e = E[r | data] and
// C = Var(r | data) from the calibrated belief of the family's cluster (FamUni::e, FamUni::C of pgbp_fam_uni_dev.hpp: under
// BM qc_k = gamma_k, and w is the shifts' displacement alone), and the terms e^2 / t into num, 1 - C / t into den (:476, :478 /
// :496, :497).  Skipped, as the reference and the general call skip them: a root-prior family, t == 0, child_mask == 0, a tip
// whose parent holds nothing in scope, a cluster without variables -- and a tip the per-site mask says is not observed at this
// site.  An internal family whose whole clade is masked stays in scope: its cluster holds the prior of r alone there, e = 0 and
// C = t, and it adds 0 to both sums; den is the number of observed tips less one.
//
// Reduction: each thread writes its block's two sums, each started from 0.0, to partial[block][2][site]; exact_uni_reduce adds
// the blocks in block order, and forms the posterior mean of the root variable (mu_hat of :435-437) by fam_uni_moments when it
// is asked for.  No atomics, no LDS, no barrier, contraction off, every sum in a fixed order, no lane's store depends on
// another lane: the bytes of a site depend neither on the call nor on the site range or the chunks it came in.  The partials of
// a chunk of sites at a time (whole workgroups: pgbp_sites_sweep_scratch_limit).  Host frame of pgbp_sites_host.hpp.
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

// partial: [blocks][2][row] (num, den), pinfo: [blocks][row].  A needed cluster that is not positive definite marks the site
// (the 1-based cluster index) and, like the constant belief (no mark), makes the block's sums NaN.
template <bool SM>
__global__ __launch_bounds__(256) void exact_uni_family(SitesArgs A, LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz, LgSiteMiss Ms,
                                                        int n_fam, double* __restrict__ partial, int32_t* __restrict__ pinfo) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x, fb = blockIdx.y;
  if (s >= A.n_sites) return;   // (a lane past the range: no barrier follows, and no other lane's store is its to make)
  const int64_t as = (int64_t)A.site0 + s;
  const int K = F.K;
  const LgSite S = lg_site(M, F.n_rates, 1, as);
  double num = 0.0, den = 0.0;
  int bad = kFamUniNoInfo;
  const int f0 = fb * kFamUniBlock, f1 = min(f0 + kFamUniBlock, n_fam);
  for (int f = f0; f < f1; ++f) {
    const int np = F.n_parents[f];
    double tt = 0.0;
    for (int k = 0; k < np; ++k) {
      const double gk = F.gamma[(size_t)f * K + k];
      tt = tt + gk * gk * F.length[(size_t)f * K + k];   // (:459)
    }
    // root prior; zero length (:461); a tip whose parent holds nothing in scope (:469); a cluster without variables
    if (np == 0 || tt == 0.0 || A.bdim[A.fam_cluster[f]] == 0) continue;
    if (F.child_pos[f] < 0 && F.parent_mask && F.parent_mask[(size_t)f * K] == 0ull) continue;
    // child_mask == 0 (:481, and a tip without data), a tip not observed at this site
    const FamUni X = fam_uni_family<SM>(A.pool, A.stride, A.off, A.bdim, F, M, Sh, Nz, Ms, S, A.fam_cluster, f, A.data_row_len, as);
    if (X.skip) continue;
    if (X.q.st != 0) {
      if (X.q.st > 0) bad = min(bad, X.c + 1);
      num = NAN;
      den = NAN;
      continue;
    }
    num = num + (X.e * X.e) / tt;
    den = den + (1.0 - X.C / tt);
  }
  double* __restrict__ o = partial + (int64_t)fb * 2 * A.row + s;
  o[0] = num;
  o[A.row] = den;
  pinfo[(int64_t)fb * A.row + s] = bad;
}

// grid.y = 0 / 1: num / den[out0 + site] = the blocks' partials added in block order; grid.y = 2: info[out0 + site] = the
// smallest mark of a block and of the root belief, 0: none, and, when mu is not null, mu[out0 + site] = the posterior mean of
// variable root_pos of belief root_belief (NaN unless its status is 0)
template <bool SM>
__global__ __launch_bounds__(256) void exact_uni_reduce(SitesArgs A, const double* __restrict__ partial,
                                                        const int32_t* __restrict__ pinfo, int nfb, int root_belief, int root_pos,
                                                        double* __restrict__ num, double* __restrict__ den, double* __restrict__ mu,
                                                        int32_t* __restrict__ info, int out0) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x, en = blockIdx.y;
  if (s >= A.n_sites) return;
  if (en < 2) {
    double acc = 0.0;
    for (int b = 0; b < nfb; ++b) acc = acc + partial[((int64_t)b * 2 + en) * A.row + s];
    (en == 0 ? num : den)[out0 + s] = acc;
  } else {
    int bad = kFamUniNoInfo;
    for (int b = 0; b < nfb; ++b) bad = min(bad, pinfo[(int64_t)b * A.row + s]);
    if (mu) {
      const FamUniMom q = fam_uni_moments<SM>(A.pool, A.stride, A.off[root_belief], A.bdim[root_belief], (int64_t)A.site0 + s);
      if (q.st > 0) bad = min(bad, root_belief + 1);
      mu[out0 + s] = q.st != 0 ? (double)NAN : (root_pos == 0 ? q.m0 : q.m1);
    }
    info[out0 + s] = bad == kFamUniNoInfo ? 0 : bad;
  }
}

}  // namespace pgbp

using namespace pgbp;

extern "C" int pgbp_bm_exact_stats_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, int32_t root_belief,
                                         int32_t root_pos, double* num, double* den, double* mu, int32_t* info) {
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_bm_exact_stats_sites";
  SitesCall c{};
  int rc = sites_accept(e, fn, "pgbp_bm_exact_stats", site_begin, site_end, (!num || !den) ? "no output buffer" : nullptr, &c);
  if (rc) return rc;
  const LgModel* L = c.L;
  const Plan& pl = *c.v.plan;
  // the model and the family table (shared with pgbp_bm_rate_matrix_sites), then the root
  if ((rc = sites_bm_closed_form_checks(e, fn, L))) return rc;
  if (mu && (rc = sites_root_check(e, fn, pl, root_belief, root_pos))) return rc;
  const LgTable& T = L->T;
  const int nf = T.n_families;
  const int ns = c.ns;
  if (ns == 0) return PGBP_OK;
  const int nfb = std::max(1, (nf + kFamUniBlock - 1) / kFamUniBlock);
  const int chunk = fam_uni_chunk(ns, 3 * (int64_t)nfb);   // the partials of a chunk of sites at a time
  std::vector<int32_t> inf(ns, 0);
  DevBuf<int32_t> d_fcl, d_pinfo, d_info;
  DevBuf<double> d_part, d_num, d_den, d_mu;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_fcl, std::max(1, nf));
  S.alloc(d_part, (size_t)nfb * 2 * chunk);
  S.alloc(d_pinfo, (size_t)nfb * chunk);
  S.alloc(d_num, ns);
  S.alloc(d_den, ns);
  S.alloc(d_mu, ns, mu != nullptr);
  S.alloc(d_info, ns);
  S.upload(d_fcl, T.cluster.data(), nf);
  if ((rc = S.ready())) return rc;
  for (int s0 = 0; S.ok() && s0 < ns; s0 += chunk) {
    const int n = std::min(chunk, ns - s0);
    const SitesArgs A = sites_args(c, site_begin + s0, n, chunk, d_fcl.get());
    const dim3 grid((n + 255) / 256, nfb);
    PGBP_SITES_LAUNCH(S, c.U.sm, exact_uni_family, grid, A, L->F, L->M, L->Sh, L->Nz, L->Ms, nf, d_part.get(), d_pinfo.get());
    PGBP_SITES_LAUNCH(S, c.U.sm, exact_uni_reduce, dim3(grid.x, 3), A, d_part.get(), d_pinfo.get(), nfb, (int)root_belief,
                      (int)root_pos, d_num.get(), d_den.get(), d_mu.get(), d_info.get(), s0);
    S.check();
  }
  S.download(num, d_num.get(), ns);
  S.download(den, d_den.get(), ns);
  S.download(mu, d_mu.get(), ns);
  S.download(inf.data(), d_info.get(), ns);
  if ((rc = S.finish())) return rc;
  for (int s = 0; s < ns; ++s) {
    if (info) info[s] = inf[s];
    if (!inf[s]) continue;   // a site with a cluster that is not positive definite: NaN throughout
    num[s] = den[s] = NAN;
    if (mu) mu[s] = NAN;
  }
  return PGBP_OK;
}

// Exact posterior covariances of linear functionals of a fitted univariate batch on a thread-per-site engine, lanes = sites:
// pgbp_posterior_cov_sites of include/pgbp.h -- pgbp_posterior_cov (pgbp_sample.hip) at p = 1 with every belief of at most 2
// variables, in the frame of pgbp_post_uni.hip: a workgroup is 256 consecutive sites, a thread holds one site, the clusters of a
// level of the schedule tree along grid.y, the resident columns in a loop.  The beliefs are read as whole lines in the layout the
// pool is in (template <bool SM>, engine_uni_view): nothing is converted, pgbp_layout is the same before and after.
//
// At one site the sampler of pgbp_sample_posterior_sites is x = m + A z.  For a functional c (wave-uniform: scalar loads):
//   validity: post_uni_valid / post_uni_first, the sampler's pass;
//   adjoint  (cov_uni_adjoint), one launch per level from the deepest, in gather form and IN PLACE in one table of
//            [columns][size][sites]: a cluster C, its children done, forms xbar_C[v] = c[v] + the t of the children whose sepsets
//            map to v (children in index order, then their S positions in order: the list of the general call), leaving +0.0
//            where it took a t; then its coefficients once, in registers (post_uni_cond: T00, T01, T11, G), and writes
//              w_C[R_l] = sum_{i <= l} T_il xbar_C[R_i]  at its R entries,  t_C[S_j] = xbar_C[S_j] - sum_i G_ij xbar_C[R_i]  at its
//            S entries, for its parent to take.  After the root's launch the table is w, +0.0 at every S position.
//   gram     (cov_uni_gram, cov_uni_fold): a thread walks a block of kFamUniBlock entries for all pairs of columns and writes
//            partial[block][pair][site]; the blocks are added in block order.  G_ab = w_a . w_b.
//   forward  (cov_uni_forward), one launch per preorder level: the sampler's apply without its offset and with w for z.
// No factor pool: a cluster's coefficients are formed once per (cluster, site, phase) by the launch that uses them.  Outputs are
// site-minor rows; a chunk of sites at a time goes through scratch bounded by pgbp_sites_sweep_scratch_limit.  No barrier, no
// atomics, contraction off, every sum in a fixed order, no lane's store depends on another lane: a site's bytes depend neither
// on the call nor on the site range, the chunks or the other columns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "pgbp_devmem.hpp"
#include "pgbp_fam_uni_dev.hpp"
#include "pgbp_sites_host.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_post_uni_dev.hpp"
#include "pgbp_sample_plan.hpp"

namespace pgbp {

// xbar of entry e of column `base / size`: c[e], then the t of the listed entries in order; what is taken is left +0.0
__device__ __forceinline__ double cov_uni_gather(const double* __restrict__ c, const int32_t* __restrict__ start,
                                                 const int32_t* __restrict__ src, int64_t base, int64_t e, int64_t row, int s,
                                                 double* __restrict__ x) {
#pragma clang fp contract(off)
  double acc = c[base + e];
  for (int g = start[e], g1 = start[e + 1]; g < g1; ++g) {
    double* __restrict__ t = x + (base + src[g]) * row + s;
    acc = acc + *t;
    *t = 0.0;
  }
  return acc;
}

// One level of the adjoint: thread = site, the items of the level along grid.y, the nc columns of the launch in a loop.
// c: [nc][size]; x: [nc][size][row] of this chunk; start[e] .. start[e + 1]: the entries in `src` whose t entry e gathers;
// bad[site]: not 0 where the site is NaN
template <bool SM>
__global__ __launch_bounds__(256) void cov_uni_adjoint(SitesArgs A, const SampItem* __restrict__ items, int n_items,
                                                       const int32_t* __restrict__ idx, const int32_t* __restrict__ start,
                                                       const int32_t* __restrict__ src, const int32_t* __restrict__ bad, int nc,
                                                       int64_t size, const double* __restrict__ c, double* __restrict__ x) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A.n_sites) return;
  const int64_t as = (int64_t)A.site0 + s;
  const bool nan_site = bad[s] != 0;
  for (int q = blockIdx.y; q < n_items; q += gridDim.y) {
    const SampItem it = items[q];
    const int m = it.m, r = it.r;
    const int32_t* __restrict__ perm = idx + it.perm;
    const int p0 = perm[0], p1 = m == 2 ? perm[1] : 0;
    const int64_t e0 = it.x_off + p0, e1 = it.x_off + p1;
    PostUniCond f{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, true};
    if (r > 0 && !nan_site) f = post_uni_cond<SM>(A.pool, A.stride, A.off[it.cluster], m, r, p0, as);
    for (int col = 0; col < nc; ++col) {
      const int64_t base = (int64_t)col * size;
      double v0 = NAN, v1 = NAN;   // what is left at perm[0], perm[1]
      if (!nan_site) {
        const double xb0 = cov_uni_gather(c, start, src, base, e0, A.row, s, x);
        const double xb1 = m == 2 ? cov_uni_gather(c, start, src, base, e1, A.row, s, x) : 0.0;
        if (r == 2) {
          v0 = f.T00 * xb0;
          v1 = f.T01 * xb0 + f.T11 * xb1;
        } else if (r == 1) {
          v0 = f.T00 * xb0;
          v1 = xb1 - f.G * xb0;
        } else {
          v0 = xb0;
          v1 = xb1;
        }
      }
      x[(base + e0) * A.row + s] = v0;
      if (m == 2) x[(base + e1) * A.row + s] = v1;
    }
  }
}

// One preorder level of k = A w: post_uni_apply without its offset and with w for z.  w, k: [nc][size][row] of this chunk
template <bool SM>
__global__ __launch_bounds__(256) void cov_uni_forward(SitesArgs A, const SampItem* __restrict__ items, int n_items,
                                                       const int32_t* __restrict__ idx, const int32_t* __restrict__ bad, int nc,
                                                       int64_t size, const double* __restrict__ w, double* __restrict__ k) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A.n_sites) return;
  const int64_t as = (int64_t)A.site0 + s;
  const bool nan_site = bad[s] != 0;
  for (int q = blockIdx.y; q < n_items; q += gridDim.y) {
    const SampItem it = items[q];
    const int m = it.m, r = it.r;
    const int32_t* __restrict__ perm = idx + it.perm;
    const int32_t* __restrict__ ppos = perm + m;
    const int p0 = perm[0], p1 = m == 2 ? perm[1] : 0;
    PostUniCond f{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, true};
    if (r > 0 && !nan_site) f = post_uni_cond<SM>(A.pool, A.stride, A.off[it.cluster], m, r, p0, as);
    for (int col = 0; col < nc; ++col) {
      const int64_t base = (int64_t)col * size;
      const double* __restrict__ wi = w + (base + it.x_off) * A.row + s;
      const double* __restrict__ kp = k + (base + it.px_off) * A.row + s;
      double* __restrict__ ko = k + (base + it.x_off) * A.row + s;
      double v0 = NAN, v1 = NAN;   // the values at perm[0], perm[1]
      if (!nan_site) {
        if (r == 2) {
          const double w0 = wi[(int64_t)p0 * A.row], w1 = wi[(int64_t)p1 * A.row];
          v0 = f.T00 * w0 + f.T01 * w1;
          v1 = f.T11 * w1;
        } else if (r == 1) {
          const double w0 = wi[(int64_t)p0 * A.row];
          v0 = f.T00 * w0;
          if (m == 2) {
            v1 = kp[(int64_t)ppos[0] * A.row];
            v0 = -(f.G * v1) + f.T00 * w0;
          }
        } else {
          v0 = kp[(int64_t)ppos[0] * A.row];
          if (m == 2) v1 = kp[(int64_t)ppos[1] * A.row];
        }
      }
      ko[(int64_t)p0 * A.row] = v0;
      if (m == 2) ko[(int64_t)p1 * A.row] = v1;
    }
  }
}

// partial[block][pair][row]: the entries of block blockIdx.y in index order, pair (a <= b) at b (b + 1) / 2 + a
__global__ __launch_bounds__(256) void cov_uni_gram(const double* __restrict__ w, int nc, int64_t size, int n_sites, int64_t row,
                                                    double* __restrict__ partial) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_sites) return;
  const int64_t e0 = (int64_t)blockIdx.y * kFamUniBlock, e1 = min(e0 + (int64_t)kFamUniBlock, size);
  const int np = nc * (nc + 1) / 2;
  double* __restrict__ o = partial + (int64_t)blockIdx.y * np * row + s;
  for (int b = 0; b < nc; ++b)
    for (int a = 0; a <= b; ++a) {
      const double* __restrict__ wa = w + (int64_t)a * size * row + s;
      const double* __restrict__ wb = w + (int64_t)b * size * row + s;
      double acc = 0.0;
      for (int64_t e = e0; e < e1; ++e) acc = acc + wa[e * row] * wb[e * row];
      o[(int64_t)(b * (b + 1) / 2 + a) * row] = acc;
    }
}

// gram[pair][row] = the blocks' partials added in block order; the pairs along grid.y
__global__ __launch_bounds__(256) void cov_uni_fold(const double* __restrict__ partial, int nb, int np, int n_sites, int64_t row,
                                                    double* __restrict__ gram) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_sites) return;
  for (int p = blockIdx.y; p < np; p += gridDim.y) {
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc = acc + partial[((int64_t)b * np + p) * row + s];
    gram[(int64_t)p * row + s] = acc;
  }
}

}  // namespace pgbp

using namespace pgbp;

namespace {

// doubles of scratch a site takes with n columns resident: the table of xbar / w (and k's), the partials of gram, the marks
// of the validity pass
int64_t cov_uni_per_site(int64_t n, int64_t size, bool want_k, bool want_gram, int nvb) {
  const int64_t ngb = (size + kFamUniBlock - 1) / kFamUniBlock;
  return n * size * (want_k ? 2 : 1) + (want_gram ? (ngb + 1) * (n * (n + 1) / 2) : 0) + nvb;
}

}  // namespace

// ms (pgbp_posterior_cov_sites_timed): the stream is drained after every phase and the wall time of the phase is added to
// ms[0 .. 4] = {validity pass (with the upload of c and of the lists), adjoint, gram, forward, copies of w, k and gram}
static int posterior_cov_sites(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_cols, const double* c,
                               double* w, double* k, double* gram, int32_t* info, double* ms) {
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_posterior_cov_sites";
  SitesCall fc{};
  int rc = sites_accept(e, fn, "pgbp_posterior_cov", site_begin, site_end, nullptr, &fc);
  if (rc) return rc;
  SampPlan sp;
  rc = sample_plan(e, std::string(fn) + ": ", tree, site_begin, site_end, n_cols, "n_cols", "column",
                   [&]() { return std::string(!c ? "no input buffer c" : (!w && !k && !gram ? "no output buffer: w, k and gram are all NULL" : "")); },
                   sp);
  if (rc) return rc;
  const int ns = fc.ns;
  const int64_t size = sp.size;
  const PostUniPre pre = post_uni_pre(sp);
  const int nvb = pre.nvb;
  const int ngb = (int)((size + kFamUniBlock - 1) / kFamUniBlock);
  const int np = n_cols * (n_cols + 1) / 2;
  // the columns of a chunk: with gram all of them are resident together (refused when one workgroup's sites do not fit); without,
  // they are cut as the draws of pgbp_sample_posterior_sites are
  const int64_t limit = g_fam_uni_limit.load();
  int cchunk = n_cols;
  if (gram) {
    if (size > 0 && 256 * cov_uni_per_site(n_cols, size, k != nullptr, true, nvb) > limit) {
      int fit = 0;
      while (fit < n_cols && 256 * cov_uni_per_site(fit + 1, size, k != nullptr, true, nvb) <= limit) ++fit;
      return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": gram needs the " + std::to_string(n_cols) +
                                                  " columns of a workgroup of 256 sites resident together; " + std::to_string(fit) +
                                                  " columns fit the scratch limit of " + std::to_string(limit) +
                                                  " doubles (pgbp_sites_sweep_scratch_limit)");
    }
  } else {
    const int64_t per_col = size * (k ? 2 : 1);
    cchunk = (int)std::min<int64_t>(n_cols, std::max<int64_t>(1, limit / std::max<int64_t>(1, 256 * per_col)));
  }
  if (ns == 0) return PGBP_OK;
  if (size == 0) {   // no cluster has a variable: nothing to weigh
    if (info) std::fill(info, info + ns, 0);
    if (gram) std::fill(gram, gram + (size_t)np * ns, 0.0);
    return PGBP_OK;
  }
  const int chunk = fam_uni_chunk(ns, cov_uni_per_site(cchunk, size, k != nullptr, gram != nullptr, nvb));
  // the gather lists of the adjoint, behind the index pool: one offset per entry of the layout (and the end), then the entries
  // whose t the entry takes -- a counting sort, so the list of one entry keeps the order it is met in: the children in index
  // order, a child's S positions in order (pgbp_posterior_cov's)
  const size_t start0 = sp.idx.size();
  {
    size_t n_src = 0;
    for (const SampItem& it : sp.by_level) n_src += (size_t)(it.m - it.r);
    sp.idx.resize(start0 + (size_t)size + 1 + n_src, 0);
    int32_t* start = sp.idx.data() + start0;
    int32_t* src = start + size + 1;
    auto each = [&](auto&& f) {
      for (int ch = 0; ch < sp.nc; ++ch) {
        if (pre.at[ch] < 0) continue;
        const SampItem& it = sp.by_level[pre.at[ch]];   // (the root has no S)
        for (int j = 0; j < it.m - it.r; ++j)
          f(it.px_off + sp.idx[it.perm + it.m + j], it.x_off + sp.idx[it.perm + it.r + j]);
      }
    };
    each([&](int64_t entry, int64_t) { ++start[entry + 1]; });
    for (int64_t q = 0; q < size; ++q) start[q + 1] += start[q];
    each([&](int64_t entry, int64_t from) { src[start[entry]++] = (int32_t)from; });   // (start[entry] walks to the end of its list ...)
    for (int64_t q = size; q > 0; --q) start[q] = start[q - 1];                         // (... which is where the next one begins)
    start[0] = 0;
  }
  std::vector<int32_t> rank(ns, 0);
  DevBuf<SampItem> d_tab;
  DevBuf<int32_t> d_idx, d_pfirst, d_rank;
  DevBuf<double> d_c, d_x, d_k, d_part, d_gram;
  const size_t table = (size_t)cchunk * size * chunk;
  SitesScratch S(e, fn, fc.v.st);
  S.alloc(d_tab, pre.tab.size());
  S.alloc(d_idx, sp.idx.size());
  S.alloc(d_pfirst, (size_t)nvb * chunk);
  S.alloc(d_rank, ns);
  S.alloc(d_c, (size_t)n_cols * size);
  S.alloc(d_x, table);
  S.alloc(d_k, table, k != nullptr);
  S.alloc(d_part, (size_t)ngb * np * chunk, gram != nullptr);
  S.alloc(d_gram, (size_t)np * chunk, gram != nullptr);
  S.upload(d_tab, pre.tab.data(), pre.tab.size());
  S.upload(d_idx, sp.idx.data(), sp.idx.size());
  S.upload(d_c, c, (size_t)n_cols * size);
  if ((rc = S.ready())) return rc;
  SitesClock phase(S, ms, 5);
  const int32_t* d_start = d_idx.get() + start0;
  const int32_t* d_src = d_start + size + 1;
  const int n_levels = (int)sp.level_off.size() - 1;
  for (int s0 = 0; S.ok() && s0 < ns; s0 += chunk) {
    const int nn = std::min(chunk, ns - s0);
    const SitesArgs A = sites_args(fc, site_begin + s0, nn, chunk);
    const dim3 gs((nn + 255) / 256);
    post_uni_validity(S, fc.U.sm, A, pre, d_tab.get(), d_idx.get(), d_pfirst.get(), d_rank.get(), s0);
    phase(0);
    for (int c0 = 0; S.ok() && c0 < n_cols; c0 += cchunk) {
      const int ncol = std::min(cchunk, n_cols - c0);
      const int64_t rows = (int64_t)ncol * size;
      const double* cc = d_c.get() + (size_t)c0 * size;
      for (int l = n_levels - 1; l >= 0; --l) {
        const int ni = sp.level_off[l + 1] - sp.level_off[l];
        PGBP_SITES_LAUNCH(S, fc.U.sm, cov_uni_adjoint, dim3(gs.x, std::min(ni, 65535)), A, d_tab.get() + sp.level_off[l], ni,
                          d_idx.get(), d_start, d_src, d_rank.get() + s0, ncol, size, cc, d_x.get());
      }
      S.check();
      phase(1);
      if (gram) {
        S.launch(cov_uni_gram, dim3(gs.x, ngb), d_x.get(), ncol, size, nn, (int64_t)chunk, d_part.get());
        S.launch(cov_uni_fold, dim3(gs.x, std::min(np, 65535)), d_part.get(), ngb, np, nn, (int64_t)chunk, d_gram.get());
        S.check();
      }
      phase(2);
      for (int l = 0; k && l < n_levels; ++l) {
        const int ni = sp.level_off[l + 1] - sp.level_off[l];
        PGBP_SITES_LAUNCH(S, fc.U.sm, cov_uni_forward, dim3(gs.x, std::min(ni, 65535)), A, d_tab.get() + sp.level_off[l], ni,
                          d_idx.get(), d_rank.get() + s0, ncol, size, d_x.get(), d_k.get());
      }
      S.check();
      phase(3);
      S.rows(w ? w + (size_t)c0 * size * ns : nullptr, ns, s0, d_x.get(), chunk, nn, rows);
      S.rows(k ? k + (size_t)c0 * size * ns : nullptr, ns, s0, d_k.get(), chunk, nn, rows);
      S.rows(gram, ns, s0, d_gram.get(), chunk, nn, np);
      phase(4);
    }
  }
  S.download(rank.data(), d_rank.get(), ns);
  if ((rc = S.finish())) return rc;
  post_uni_info(pre, rank, info);
  return PGBP_OK;
}

extern "C" int pgbp_posterior_cov_sites(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_cols,
                                        const double* c, double* w, double* k, double* gram, int32_t* info) {
  return posterior_cov_sites(e, tree, site_begin, site_end, n_cols, c, w, k, gram, info, nullptr);
}

extern "C" int pgbp_posterior_cov_sites_timed(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_cols,
                                              const double* c, double* w, double* k, double* gram, int32_t* info, double* ms5) {
  if (e && !ms5) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_posterior_cov_sites_timed: no buffer for the phase times");
  return posterior_cov_sites(e, tree, site_begin, site_end, n_cols, c, w, k, gram, info, ms5);
}

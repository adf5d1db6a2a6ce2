// The evolutionary rate matrix between the sites of a univariate batch APPLIED TO A BLOCK OF VECTORS, without the sites x sites
// matrix: pgbp_bm_rate_apply_sites of include/pgbp.h, the operator of an iterative consumer (the leading phylogenetic principal
// components: exact.py, phylo_pca_leading_sites).  gram = U'U with U[f][s] = e_fs / sqrt(t_f) (pgbp_rate_uni.hip), so
//   gv[j][a] = sum_f U[f][a] * (sum_b U[f][b] v[j][b])
// is two skinny products with U.  Three phases per chunk of whole 64-family blocks:
//   rate_uni_resid<SM>, rate_uni_reduce<SM>   phase one of the rate matrix (pgbp_rate_uni_dev.hpp): the chunk's U rows, den,
//                        mu and info;
//   rate_apply_uv<NT>    W[f][j] = sum_b U[f][b] v[j][b] on the matrix cores (v_mfma_f64_16x16x4_f64).  A wavefront owns 16 families
//                        and all the vectors (NT accumulator tiles of 16 x 16), a workgroup of four wavefronts 64 families.  The
//                        site axis is walked in index order, 4 sites per MFMA, in slabs of 32 sites: a wavefront reads its 16 rows
//                        of the slab along the rows (a load is two segments of 256 contiguous bytes) into registers a slab ahead
//                        and turns them through its own LDS tile, since the MFMA wants the contracted axis across lane groups;
//                        v travels as its transpose [site][vector], whose slab is contiguous, through LDS for the four wavefronts.
//   rate_apply_utw<NT>   Z[a][j] += sum_f U[f][a] W[f][j].  A wavefront owns 16 sites and all the vectors, a workgroup 64 sites.
//                        The family axis is walked in index order, 4 families per MFMA, on top of what the chunks before left, in
//                        slabs of 32 families: U straight from global memory in the operand's own layout (a load is four rows of
//                        128 contiguous bytes), a slab ahead; the slab of W shared by the four wavefronts through two LDS buffers,
//                        one barrier per slab.  U is the A operand and W the B operand, as the two factors of rate_uni_syrk are:
//                        with v a unit vector W is a column of U and the MFMA sequence is that of the gram column.
// One owner per tile of W and of Z, no split of a contracted axis, no atomics, contraction off: gv has the same bytes on every
// call, for every chunking (chunk boundaries are multiples of 64 families, so step i of an entry is families 4 i .. 4 i + 3) and
// for every number of vectors a vector travels with (an entry of an MFMA result depends on its own row and column only).
// Host frame of pgbp_sites_host.hpp; U, W, Z and the transposed v are bounded by pgbp_sites_sweep_scratch_limit (a chunk is one
// block at least).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "pgbp_devmem.hpp"
#include "pgbp_fam_uni_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"
#include "pgbp_rate_uni_dev.hpp"
#include "pgbp_sites_host.hpp"

namespace pgbp {

constexpr int kApplyMaxVec = 64;   // vectors per call: four accumulator tiles per wavefront
constexpr int kApplySlab = 32;     // sites (rate_apply_uv) or families (rate_apply_utw) per slab: eight MFMA steps
constexpr int kApplyLdsU = 34;     // doubles per row of a wavefront's U tile in LDS: 32 and a pad of 2, so that the 32 lanes of
                                   // a half wavefront (16 rows x 2 columns) read 32 different pairs of banks

// the 8 doubles a lane fetches of its wavefront's 16 x 32 piece of U: element i is row (lane + 64 i) / 32, column
// (lane + 64 i) % 32 -- a wavefront reads two rows of 32 contiguous doubles -- and +0.0 past the chunk's rows or the sites
__device__ __forceinline__ void rate_apply_fetch(const double* __restrict__ U, int64_t ld, int f0, int rows4, int b0, int n, int lane,
                                                 double (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = lane + 64 * i, r = f0 + (idx >> 5), c = b0 + (idx & 31);
    v[i] = (r < rows4 && c < n) ? U[(int64_t)r * ld + c] : 0.0;
  }
}

// W[r][j] = sum_b U[r][b] Vt[b][j] for the chunk's rows4 rows, b in index order 4 per step; U: [rows][ld], n sites of which
// np = n padded to 16 take part (the sites past n as +0.0); Vt: [np][16 NT], +0.0 in the padding; W: [rows][16 NT].
// Per slab of 32 sites: the next slab -- the wavefront's 16 x 32 piece of U and the workgroup's 32 x 16 NT piece of Vt, which is
// contiguous -- is fetched into registers, the current one is multiplied out of LDS (no global load between the fetch and the
// MFMAs: the memory counter is in order, a load there would wait for the fetch), then a barrier, the stores, a barrier.
template <int NT>
__global__ __launch_bounds__(256) void rate_apply_uv(const double* __restrict__ U, int64_t ld, int rows4, int n, int np,
                                                     const double* __restrict__ Vt, double* __restrict__ W) {
#pragma clang fp contract(off)
  constexpr int nvp = 16 * NT, ldv = nvp + 16;   // (a pad of 16: the two rows a half wavefront reads fall on different banks)
  __shared__ double Us[4][16 * kApplyLdsU];
  __shared__ double Vs[kApplySlab * ldv];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int lr = lane >> 4, lc = lane & 15;   // A: row lc, k = lr; B: k = lr, column lc; C/D: column lc, rows lr + 4 reg
  const int f0 = blockIdx.x * 64 + w * 16;
  const bool active = f0 < rows4;             // (wave-uniform; a wavefront past the rows still meets the barriers)
  rate_v4d acc[NT];
#pragma unroll
  for (int jt = 0; jt < NT; ++jt) acc[jt] = rate_v4d{0.0, 0.0, 0.0, 0.0};
  double pu[8], pv[2 * NT];
  rate_apply_fetch(U, ld, f0, rows4, 0, n, lane, pu);
#pragma unroll
  for (int i = 0; i < 2 * NT; ++i) {
    const int idx = t + 256 * i, r = idx / nvp;
    pv[i] = r < np ? Vt[(int64_t)r * nvp + idx % nvp] : 0.0;
  }
  for (int b0 = 0; b0 < np; b0 += kApplySlab) {
    // (the first slab: nothing is read yet; later ones: every wavefront left the slab before at the barrier below)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = lane + 64 * i;
      Us[w][(idx >> 5) * kApplyLdsU + (idx & 31)] = pu[i];
    }
#pragma unroll
    for (int i = 0; i < 2 * NT; ++i) {
      const int idx = t + 256 * i;
      Vs[(idx / nvp) * ldv + idx % nvp] = pv[i];
    }
    __syncthreads();
    if (b0 + kApplySlab < np) {   // the next slab, in flight while this one is multiplied
      rate_apply_fetch(U, ld, f0, rows4, b0 + kApplySlab, n, lane, pu);
#pragma unroll
      for (int i = 0; i < 2 * NT; ++i) {
        const int idx = t + 256 * i, r = b0 + kApplySlab + idx / nvp;
        pv[i] = r < np ? Vt[(int64_t)r * nvp + idx % nvp] : 0.0;
      }
    }
    if (active) {
      const int steps = min(kApplySlab / 4, (np - b0) / 4);   // no step past the padded sites
#pragma unroll
      for (int kk = 0; kk < kApplySlab / 4; ++kk) {
        if (kk < steps) {
          const double a = Us[w][lc * kApplyLdsU + kk * 4 + lr];
          double b[NT];
#pragma unroll
          for (int jt = 0; jt < NT; ++jt) b[jt] = Vs[(kk * 4 + lr) * ldv + jt * 16 + lc];
#pragma unroll
          for (int jt = 0; jt < NT; ++jt) acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[jt], acc[jt], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  if (active) {
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int r = f0 + lr + 4 * g;
        if (r < rows4) W[(int64_t)r * nvp + jt * 16 + lc] = acc[jt][g];
      }
  }
}

// Zt[a][j] += sum_r U[r][a] W[r][j] over the chunk's rows4 rows (a multiple of 4), r in index order 4 per step; Zt: [np][16 NT],
// read and written in the rows of the 16-site tiles that hold a site below n
template <int NT>
__global__ __launch_bounds__(256) void rate_apply_utw(const double* __restrict__ U, int64_t ld, int rows4, int n,
                                                      const double* __restrict__ W, double* __restrict__ Zt) {
#pragma clang fp contract(off)
  constexpr int nvp = 16 * NT, lds = nvp + 16;   // (a pad of 16: the two rows a half wavefront reads fall on different banks)
  __shared__ double Ws[2][kApplySlab * lds];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int lr = lane >> 4, lc = lane & 15;
  const int a0 = blockIdx.x * 64 + w * 16;
  const bool active = a0 < n;                    // (wave-uniform; n padded to 16 covers the tile)
  const bool col = a0 + lc < n;
  rate_v4d acc[NT];
#pragma unroll
  for (int jt = 0; jt < NT; ++jt)
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[jt][g] = active ? Zt[(int64_t)(a0 + lr + 4 * g) * nvp + jt * 16 + lc] : 0.0;
  double cu[8], pu[8], pw[2 * NT];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    const int r = kk * 4 + lr;
    cu[kk] = (col && r < rows4) ? U[(int64_t)r * ld + a0 + lc] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < 2 * NT; ++i) {
    const int idx = t + 256 * i, r = idx / nvp, c = idx % nvp;
    Ws[0][r * lds + c] = r < rows4 ? W[(int64_t)r * nvp + c] : 0.0;
  }
  __syncthreads();
  for (int k0 = 0, cur = 0; k0 < rows4; k0 += kApplySlab, cur ^= 1) {
    const bool more = k0 + kApplySlab < rows4;
    if (more) {   // the next slab, in flight while this one is multiplied
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const int r = k0 + kApplySlab + kk * 4 + lr;
        pu[kk] = (col && r < rows4) ? U[(int64_t)r * ld + a0 + lc] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < 2 * NT; ++i) {
        const int idx = t + 256 * i, r = k0 + kApplySlab + idx / nvp;
        pw[i] = r < rows4 ? W[(int64_t)r * nvp + idx % nvp] : 0.0;
      }
    }
    if (active) {
      const int steps = min(kApplySlab / 4, (rows4 - k0) / 4);   // no step past the chunk's rows
#pragma unroll
      for (int kk = 0; kk < kApplySlab / 4; ++kk) {
        if (kk < steps) {
          double b[NT];
#pragma unroll
          for (int jt = 0; jt < NT; ++jt) b[jt] = Ws[cur][(kk * 4 + lr) * lds + jt * 16 + lc];
#pragma unroll
          for (int jt = 0; jt < NT; ++jt) acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(cu[kk], b[jt], acc[jt], 0, 0, 0);
        }
      }
    }
    // into the other buffer, which every wavefront left at the barrier that ended the slab before
    if (more) {
#pragma unroll
      for (int i = 0; i < 2 * NT; ++i) {
        const int idx = t + 256 * i;
        Ws[cur ^ 1][(idx / nvp) * lds + idx % nvp] = pw[i];
      }
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) cu[kk] = pu[kk];
    }
    __syncthreads();
  }
  if (active) {
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int g = 0; g < 4; ++g) Zt[(int64_t)(a0 + lr + 4 * g) * nvp + jt * 16 + lc] = acc[jt][g];
  }
}

}  // namespace pgbp

using namespace pgbp;

// kernel<NT> for nt = 1 .. 4 tiles of 16 vectors
#define PGBP_APPLY_LAUNCH(S, nt, kernel, grid, ...)                \
  do {                                                             \
    if ((nt) == 1) (S).launch(kernel<1>, grid, __VA_ARGS__);        \
    else if ((nt) == 2) (S).launch(kernel<2>, grid, __VA_ARGS__);   \
    else if ((nt) == 3) (S).launch(kernel<3>, grid, __VA_ARGS__);   \
    else (S).launch(kernel<4>, grid, __VA_ARGS__);                  \
  } while (0)

// ms (pgbp_bm_rate_apply_sites_timed): the stream is drained after every phase and the wall time of the phase is added to
// ms[0 .. 3] = {residual rows (with the uploads and the reduce), U v, U' W, copies}
static int rate_apply_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, int32_t n_vec, const double* v, int32_t root_belief,
                            int32_t root_pos, double* gv, double* den, double* mu, int32_t* info, double* ms) {
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_bm_rate_apply_sites";
  SitesCall c{};
  int rc = sites_accept_state(e, fn, site_begin, site_end, &c);
  if (rc) return rc;
  if (n_vec < 1 || n_vec > kApplyMaxVec)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": " + std::to_string(n_vec) + " vectors; a call takes 1 to " +
                                                std::to_string(kApplyMaxVec) + " (block a wider set over several calls)");
  if (!v) return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": no input vectors");
  if (!gv) return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": no output buffer");
  if ((rc = sites_accept_engine(e, fn, "pgbp_bm_exact_stats", c))) return rc;
  const LgModel* L = c.L;
  const Plan& pl = *c.v.plan;
  if (L->Ms.words)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": a per-site mask of missing tips is in force (pgbp_lg_set_site_missing): "
                                                "an estimate across two sites needs the same observed tips at both (a shared "
                                                "child_mask is fine)");
  if ((rc = sites_bm_closed_form_checks(e, fn, L))) return rc;
  if (mu && (rc = sites_root_check(e, fn, pl, root_belief, root_pos))) return rc;
  const LgTable& T = L->T;
  const int nf = T.n_families;
  const int n = c.ns;
  if (n == 0) return PGBP_OK;
  const int np = (n + 15) / 16 * 16, nt = (n_vec + 15) / 16, nvp = 16 * nt;   // sites and vectors padded to 16
  const int64_t ld = np;
  const int nfb = std::max(1, (nf + kFamUniBlock - 1) / kFamUniBlock);
  // a chunk: whole blocks of 64 families -- 64 U rows, a den partial and a mark per block and site, 64 W rows -- beside Z and
  // the transposed v
  const int64_t per_block = (int64_t)(kFamUniBlock + 2) * ld + (int64_t)kFamUniBlock * nvp;
  const int64_t left = g_fam_uni_limit.load() - 2 * (int64_t)np * nvp;
  const int bchunk = (int)std::min<int64_t>(nfb, std::max<int64_t>(1, left / per_block));
  std::vector<double> vt((size_t)np * nvp, 0.0), zt((size_t)np * nvp, 0.0);
  for (int j = 0; j < n_vec; ++j)
    for (int b = 0; b < n; ++b) vt[(size_t)b * nvp + j] = v[(size_t)j * n + b];
  std::vector<int32_t> inf(n, 0);
  std::vector<double> dn(n, 0.0), mh(mu ? n : 0, 0.0);
  DevBuf<int32_t> d_fcl, d_pinfo, d_info;
  DevBuf<double> d_U, d_W, d_Z, d_V, d_pden, d_den, d_mu;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_fcl, std::max(1, nf));
  S.alloc(d_U, (size_t)bchunk * kFamUniBlock * ld);
  S.alloc(d_W, (size_t)bchunk * kFamUniBlock * nvp);
  S.alloc(d_Z, (size_t)np * nvp);
  S.alloc(d_V, (size_t)np * nvp);
  S.alloc(d_pden, (size_t)bchunk * ld);
  S.alloc(d_pinfo, (size_t)bchunk * ld);
  S.alloc(d_den, n);
  S.alloc(d_mu, n, mu != nullptr);
  S.alloc(d_info, n);
  S.upload(d_fcl, T.cluster.data(), nf);
  S.upload(d_V, vt.data(), vt.size());
  if (S.ok()) S.err = hipMemsetAsync(d_Z.get(), 0, sizeof(double) * (size_t)np * nvp, c.v.st);
  if ((rc = S.ready())) return rc;
  SitesClock clk(S, ms, 4);
  for (int b0 = 0; S.ok() && b0 < nfb; b0 += bchunk) {
    const int nb = std::min(bchunk, nfb - b0), f_begin = b0 * kFamUniBlock;
    const int rows4 = std::max(0, (std::min(nf, f_begin + nb * kFamUniBlock) - f_begin + 3) / 4 * 4);
    const int first = b0 == 0, last = b0 + nb >= nfb;
    const SitesArgs A = sites_args(c, site_begin, n, (int)ld, d_fcl.get());
    const dim3 grid((n + 255) / 256, nb);
    PGBP_SITES_LAUNCH(S, c.U.sm, rate_uni_resid, grid, A, L->F, L->M, L->Sh, L->Nz, L->Ms, nf, f_begin, rows4, d_U.get(), d_pden.get(),
                      d_pinfo.get());
    PGBP_SITES_LAUNCH(S, c.U.sm, rate_uni_reduce, dim3(grid.x, 2), A, d_pden.get(), d_pinfo.get(), nb, first, last, (int)root_belief,
                      (int)root_pos, d_den.get(), d_mu.get(), d_info.get(), 0);
    clk(0);
    if (rows4)
      PGBP_APPLY_LAUNCH(S, nt, rate_apply_uv, dim3((rows4 + 63) / 64), (const double*)d_U.get(), ld, rows4, n, np,
                        (const double*)d_V.get(), d_W.get());
    clk(1);
    if (rows4)
      PGBP_APPLY_LAUNCH(S, nt, rate_apply_utw, dim3((np + 63) / 64), (const double*)d_U.get(), ld, rows4, n, (const double*)d_W.get(),
                        d_Z.get());
    S.check();
    clk(2);
  }
  S.download(dn.data(), d_den.get(), n);
  if (mu) S.download(mh.data(), d_mu.get(), n);
  S.download(inf.data(), d_info.get(), n);
  S.download(zt.data(), d_Z.get(), zt.size());
  clk(3);
  if ((rc = S.finish())) return rc;
  bool bad = false;
  for (int s = 0; s < n; ++s) {
    if (inf[s]) {   // a site with a cluster that is not positive definite: NaN in its den and its mu, and no column of U
      bad = true;
      dn[s] = NAN;
      if (mu) mh[s] = NAN;
    }
    if (den) den[s] = dn[s];
    if (mu) mu[s] = mh[s];
    if (info) info[s] = inf[s];
  }
  for (int j = 0; j < n_vec; ++j)
    for (int a = 0; a < n; ++a) gv[(size_t)j * n + a] = bad ? (double)NAN : zt[(size_t)a * nvp + j];
  return PGBP_OK;
}

extern "C" int pgbp_bm_rate_apply_sites(pgbp_engine* e, int32_t site_begin, int32_t site_end, int32_t n_vec, const double* v,
                                        int32_t root_belief, int32_t root_pos, double* gv, double* den, double* mu, int32_t* info) {
  return rate_apply_sites(e, site_begin, site_end, n_vec, v, root_belief, root_pos, gv, den, mu, info, nullptr);
}

extern "C" int pgbp_bm_rate_apply_sites_timed(pgbp_engine* e, int32_t site_begin, int32_t site_end, int32_t n_vec, const double* v,
                                              int32_t root_belief, int32_t root_pos, double* gv, double* den, double* mu,
                                              int32_t* info, double* ms4) {
  if (e && !ms4) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_bm_rate_apply_sites_timed: no buffer for the phase times");
  return rate_apply_sites(e, site_begin, site_end, n_vec, v, root_belief, root_pos, gv, den, mu, info, ms4);
}

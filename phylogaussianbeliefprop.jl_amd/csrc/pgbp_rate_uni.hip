// The evolutionary rate matrix between the sites of a univariate batch on a thread-per-site engine (evol.vcv / ratematrix,
// phyl.pca): pgbp_bm_rate_matrix_sites of include/pgbp.h.  Under a Brownian motion with an improper root and the same observed
// tips at every site, (Y'PY)_ab = sum_f e_fa e_fb / t_f with e_fs = E[r_f | data of site s] and t_f = sum_k gamma_k^2 length_k:
// the bilinear form of what pgbp_bm_exact_stats_sites (pgbp_exact_uni.hip) sums on the diagonal.  Two phases per chunk of
// families:
//   rate_uni_resid<SM>  (pgbp_rate_uni_dev.hpp: shared with pgbp_rate_apply_uni.hip, as rate_uni_reduce is)
//                       the frame of exact_uni_family -- a workgroup is 256 consecutive sites, grid.y a block of kFamUniBlock
//                       consecutive families, a thread walks its block for its one site, the beliefs read in the layout the
//                       pool is in -- and stores U[family][site] = e / sqrt(t) (+0.0 for a skipped family and for the rows
//                       that pad the last family up to a multiple of 4); it keeps the block's sum of 1 - C / t and its mark,
//                       which rate_uni_reduce folds in block order across the chunks (den, mu and info of the exact sweep);
//   rate_uni_syrk       gram[a][b] += sum_f U[f][a] U[f][b] on the matrix cores (v_mfma_f64_16x16x4_f64).  A workgroup of four
//                       wavefronts owns a 128 x 128 tile, a wavefront a 64 x 64 quarter of it: 4 x 4 accumulator tiles of
//                       16 x 16 in registers, read from the device-resident gram block at the start and written back at the
//                       end.  The family axis is walked in index order, 4 families per MFMA, in slabs of 16 families staged
//                       through two LDS buffers (each global read is a whole row segment of 128 contiguous doubles; the next
//                       slab is fetched into registers while the current one is multiplied, and stored into the other
//                       buffer before the one barrier of the slab).
// No atomics, no split over the family axis inside a launch, contraction off.  An entry (a, b) sees the same sequence of MFMA
// steps -- families 4 i .. 4 i + 3 at step i, on top of what the chunks before left -- whatever the tile it falls in, the site
// ranges of the query and the chunking: chunk boundaries are multiples of 64 families.  The product of two doubles commutes, so
// entry (b, a) of the transposed query has the same bytes; the tiles wholly below the diagonal of a square query are therefore
// not computed but copied from their mirror images once the last chunk is in (rate_uni_mirror).
// Host frame of pgbp_sites_host.hpp; the U rows of a chunk are bounded by pgbp_sites_sweep_scratch_limit, the gram block is not.
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

constexpr int kRateTile = 128;   // sites per side of a workgroup's tile (four wavefronts, 64 x 64 each)
constexpr int kRateSlab = 16;    // families per LDS slab (four MFMA steps)
constexpr int kRateLds = 144;    // doubles per slab row in LDS: 128 and a pad of 16, so that the rows a half wavefront reads
                                 // (two rows of 16 doubles, 1152 bytes apart) fall on different banks

// the 16 doubles a thread fetches of a slab: element i of the thread is row (t + 256 i) / 128, column (t + 256 i) % 128 of
// the slab -- a wavefront reads 64 contiguous doubles, four whole lines -- and +0.0 past the chunk's rows or the range's sites
__device__ __forceinline__ void rate_uni_fetch(const double* __restrict__ U, int64_t ld, int k0, int rows4, int c0, int n, int t,
                                               double (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = t + 256 * i, r = k0 + (idx >> 7), c = c0 + (idx & 127);
    v[i] = (r < rows4 && c < n) ? U[(int64_t)r * ld + c] : 0.0;
  }
}

// G[a][b] += sum_r UA[r][a] UB[r][b] over the chunk's rows4 rows (a multiple of 4), r in index order.  A workgroup takes one
// tile of kRateTile x kRateTile sites from the host's list (tiles[i] = row tile << 16 | column tile: rate_uni_tiles); the
// workgroups that share an XCD (blockIdx.x % 8) take a contiguous eighth of the list, so that the tiles resident on an XCD
// together are neighbours and share their slabs in its L2.  G: [nr][ldg], read and written only inside nr x nc.
__global__ __launch_bounds__(256) void rate_uni_syrk(const double* __restrict__ UA, const double* __restrict__ UB, int64_t ld,
                                                     int rows4, int nr, int nc, double* __restrict__ G, int64_t ldg,
                                                     const int32_t* __restrict__ tiles, int n_tiles) {
#pragma clang fp contract(off)
  const int xcd = blockIdx.x % 8, q = n_tiles / 8, rm = n_tiles % 8;   // (a bijection of 0 .. n_tiles - 1 for any n_tiles)
  const int tile = tiles[(xcd < rm ? xcd * (q + 1) : rm * (q + 1) + (xcd - rm) * q) + blockIdx.x / 8];
  __shared__ double As[2][kRateSlab * kRateLds], Bs[2][kRateSlab * kRateLds];   // two slabs each: one barrier per slab
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int a0 = (tile >> 16) * kRateTile, b0 = (tile & 0xffff) * kRateTile;
  const int qa = (w >> 1) * 64, qb = (w & 1) * 64;           // the wavefront's quarter of the tile
  const bool active = a0 + qa < nr && b0 + qb < nc;          // (wave-uniform: a quarter wholly past the ranges multiplies nothing)
  const int lr = lane >> 4, lc = lane & 15;                  // C/D: column lc, rows lr + 4 reg; A/B: k = lr, row / column lc
  rate_v4d acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int a = a0 + qa + mi * 16 + lr + 4 * g, b = b0 + qb + ni * 16 + lc;
        acc[mi][ni][g] = (a < nr && b < nc) ? G[(int64_t)a * ldg + b] : 0.0;
      }
  double pa[8], pb[8];
  rate_uni_fetch(UA, ld, 0, rows4, a0, nr, t, pa);
  rate_uni_fetch(UB, ld, 0, rows4, b0, nc, t, pb);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = t + 256 * i, o = (idx >> 7) * kRateLds + (idx & 127);
    As[0][o] = pa[i];
    Bs[0][o] = pb[i];
  }
  __syncthreads();
  for (int k0 = 0, cur = 0; k0 < rows4; k0 += kRateSlab, cur ^= 1) {
    const bool more = k0 + kRateSlab < rows4;
    if (more) {   // the next slab, in flight while this one is multiplied
      rate_uni_fetch(UA, ld, k0 + kRateSlab, rows4, a0, nr, t, pa);
      rate_uni_fetch(UB, ld, k0 + kRateSlab, rows4, b0, nc, t, pb);
    }
    if (active) {
      const int steps = min(kRateSlab / 4, (rows4 - k0) / 4);   // no step past the chunk's rows: an entry sees only its families
#pragma unroll
      for (int kk = 0; kk < kRateSlab / 4; ++kk) {
        if (kk < steps) {
          double fa[4], fb[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            fa[i] = As[cur][(kk * 4 + lr) * kRateLds + qa + i * 16 + lc];
            fb[i] = Bs[cur][(kk * 4 + lr) * kRateLds + qb + i * 16 + lc];
          }
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
        }
      }
    }
    // into the other buffer, which every wavefront left at the barrier that ended the slab before; it is read after this one
    if (more) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int idx = t + 256 * i, o = (idx >> 7) * kRateLds + (idx & 127);
        As[cur ^ 1][o] = pa[i];
        Bs[cur ^ 1][o] = pb[i];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int a = a0 + qa + mi * 16 + lr + 4 * g, b = b0 + qb + ni * 16 + lc;
        if (a < nr && b < nc) G[(int64_t)a * ldg + b] = acc[mi][ni][g];
      }
}

// The tiles wholly below the diagonal of a square query, once the last chunk is in: G[a][b] = G[b][a] for a / kRateTile >
// b / kRateTile, in pieces of 32 x 32 through LDS so that reads and writes are both along rows.  The entry copied is the one
// the update would have formed: the same products in the same order, since a product of two doubles commutes (asserted by
// tests/test_gpu_rate_uni.py against queries that compute those entries).
__global__ __launch_bounds__(256) void rate_uni_mirror(double* __restrict__ G, int n, int64_t ldg) {
  __shared__ double T[32][33];
  const int a0 = blockIdx.y * 32, b0 = blockIdx.x * 32;
  if (a0 / kRateTile <= b0 / kRateTile) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = b0 + ty + 8 * i, c = a0 + tx;   // the source piece: rows b0 .., columns a0 ..
    T[ty + 8 * i][tx] = (r < n && c < n) ? G[(int64_t)r * ldg + c] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int a = a0 + ty + 8 * i, b = b0 + tx;
    if (a < n && b < n) G[(int64_t)a * ldg + b] = T[tx][ty + 8 * i];
  }
}

}  // namespace pgbp

using namespace pgbp;

// The tiles rate_uni_syrk computes, in the order it hands them out: bands of 4 tile rows, in a band groups of 8 tile columns,
// in a group row by row -- 32 consecutive tiles are a 4 x 8 block that reads 12 slab strips, not 33.  upper: a square query,
// whose tiles wholly below the diagonal are mirrored instead.
static std::vector<int32_t> rate_uni_tiles(int nr, int nc, bool upper) {
  const int ty_n = (nr + kRateTile - 1) / kRateTile, tx_n = (nc + kRateTile - 1) / kRateTile;
  std::vector<int32_t> t;
  for (int y0 = 0; y0 < ty_n; y0 += 4)
    for (int x0 = 0; x0 < tx_n; x0 += 8)
      for (int y = y0; y < std::min(y0 + 4, ty_n); ++y)
        for (int x = x0; x < std::min(x0 + 8, tx_n); ++x)
          if (!upper || x >= y) t.push_back((int32_t)((y << 16) | x));
  return t;
}

// ms (pgbp_bm_rate_matrix_sites_timed): the stream is drained after every phase and the wall time of the phase is added to
// ms[0 .. 2] = {residual rows (with the uploads and the reduce), rank-k update, copies}
static int rate_matrix_sites(pgbp_engine* e, int32_t row_begin, int32_t row_end, int32_t col_begin, int32_t col_end,
                             int32_t root_belief, int32_t root_pos, double* gram, double* den, double* mu, int32_t* info, double* ms) {
  if (!e) return PGBP_ERR_INVALID;
  const char* fn = "pgbp_bm_rate_matrix_sites";
  SitesCall c{};
  int rc = sites_accept_state(e, fn, row_begin, row_end, &c);
  if (rc) return rc;
  if (col_begin < 0 || col_end < col_begin || col_end > engine_n_sites(e))
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": site range outside the engine's sites");
  if (!gram) return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": no output buffer");
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
  const int nr = row_end - row_begin, nc = col_end - col_begin, no = nr + nc;
  if (no == 0) return PGBP_OK;
  // the U rows hold the row sites, then the column sites unless they are the row sites; each range padded to 16 sites, so that a
  // range starts on a line
  const bool same = row_begin == col_begin && row_end == col_end;
  const int nrp = (nr + 15) / 16 * 16, ncp = (nc + 15) / 16 * 16;
  const int64_t ld = (int64_t)nrp + (same ? 0 : ncp), colU = same ? 0 : nrp;
  const int nfb = std::max(1, (nf + kFamUniBlock - 1) / kFamUniBlock);
  // a chunk: whole blocks of 64 families over all the sites of the call -- 64 U rows, a den partial and a mark per block and site
  const int64_t per_block = (int64_t)(kFamUniBlock + 2) * std::max<int64_t>(1, ld);
  const int bchunk = (int)std::min<int64_t>(nfb, std::max<int64_t>(1, g_fam_uni_limit.load() / per_block));
  std::vector<int32_t> inf(no, 0);
  std::vector<double> dn(no, 0.0), mh(mu ? no : 0, 0.0);
  const std::vector<int32_t> tiles = rate_uni_tiles(nr, nc, same);
  DevBuf<int32_t> d_fcl, d_pinfo, d_info, d_tiles;
  DevBuf<double> d_gram, d_U, d_pden, d_den, d_mu;
  SitesScratch S(e, fn, c.v.st);
  S.alloc(d_gram, (size_t)nr * ncp);   // the output block: outside the scratch limit
  S.alloc(d_fcl, std::max(1, nf));
  S.alloc(d_U, (size_t)bchunk * kFamUniBlock * ld);
  S.alloc(d_pden, (size_t)bchunk * ld);
  S.alloc(d_pinfo, (size_t)bchunk * ld);
  S.alloc(d_den, no);
  S.alloc(d_mu, no, mu != nullptr);
  S.alloc(d_info, no);
  S.alloc(d_tiles, tiles.size());
  S.upload(d_fcl, T.cluster.data(), nf);
  S.upload(d_tiles, tiles.data(), tiles.size());
  if (S.ok() && nr && nc) S.err = hipMemsetAsync(d_gram.get(), 0, sizeof(double) * (size_t)nr * ncp, c.v.st);
  if ((rc = S.ready())) return rc;
  SitesClock clk(S, ms, 3);
  const int n_ranges = same ? 1 : 2;
  for (int b0 = 0; S.ok() && b0 < nfb; b0 += bchunk) {
    const int nb = std::min(bchunk, nfb - b0), f_begin = b0 * kFamUniBlock;
    const int rows4 = std::max(0, (std::min(nf, f_begin + nb * kFamUniBlock) - f_begin + 3) / 4 * 4);
    const int first = b0 == 0, last = b0 + nb >= nfb;
    for (int k = 0; k < n_ranges; ++k) {
      const int n = k ? nc : nr, site0 = k ? col_begin : row_begin, out0 = k ? nr : 0;
      const int64_t u0 = k ? colU : 0;
      if (n == 0) continue;
      const SitesArgs A = sites_args(c, site0, n, (int)ld, d_fcl.get());
      const dim3 grid((n + 255) / 256, nb);
      PGBP_SITES_LAUNCH(S, c.U.sm, rate_uni_resid, grid, A, L->F, L->M, L->Sh, L->Nz, L->Ms, nf, f_begin, rows4, d_U.get() + u0,
                        d_pden.get() + u0, d_pinfo.get() + u0);
      PGBP_SITES_LAUNCH(S, c.U.sm, rate_uni_reduce, dim3(grid.x, 2), A, d_pden.get() + u0, d_pinfo.get() + u0, nb, first, last,
                        (int)root_belief, (int)root_pos, d_den.get(), d_mu.get(), d_info.get(), out0);
    }
    clk(0);
    if (nr && nc && rows4)
      S.launch(rate_uni_syrk, dim3((unsigned)tiles.size()), d_U.get(), d_U.get() + colU, ld, rows4, nr, nc, d_gram.get(), (int64_t)ncp,
               d_tiles.get(), (int)tiles.size());
    if (same && last && nr > kRateTile) S.launch(rate_uni_mirror, dim3((nr + 31) / 32, (nr + 31) / 32), d_gram.get(), nr, (int64_t)ncp);
    S.check();
    clk(1);
  }
  const int nfirst = same ? nr : no;   // what the device formed: both ranges, or the one they share
  S.download(dn.data(), d_den.get(), nfirst);
  if (mu) S.download(mh.data(), d_mu.get(), nfirst);
  S.download(inf.data(), d_info.get(), nfirst);
  if (nr && nc) S.rows(gram, nc, 0, d_gram.get(), ncp, nc, nr);
  clk(2);
  if ((rc = S.finish())) return rc;
  if (same)
    for (int s = 0; s < nr; ++s) {
      dn[nr + s] = dn[s];
      inf[nr + s] = inf[s];
      if (mu) mh[nr + s] = mh[s];
    }
  for (int s = 0; s < no; ++s) {
    if (inf[s]) {   // a site with a cluster that is not positive definite: NaN in its row or column, its den and its mu
      dn[s] = NAN;
      if (mu) mh[s] = NAN;
      if (s < nr)
        for (int b = 0; b < nc; ++b) gram[(size_t)s * nc + b] = NAN;
      else
        for (int a = 0; a < nr; ++a) gram[(size_t)a * nc + (s - nr)] = NAN;
    }
    if (den) den[s] = dn[s];
    if (mu) mu[s] = mh[s];
    if (info) info[s] = inf[s];
  }
  return PGBP_OK;
}

extern "C" int pgbp_bm_rate_matrix_sites(pgbp_engine* e, int32_t row_begin, int32_t row_end, int32_t col_begin, int32_t col_end,
                                         int32_t root_belief, int32_t root_pos, double* gram, double* den, double* mu, int32_t* info) {
  return rate_matrix_sites(e, row_begin, row_end, col_begin, col_end, root_belief, root_pos, gram, den, mu, info, nullptr);
}

extern "C" int pgbp_bm_rate_matrix_sites_timed(pgbp_engine* e, int32_t row_begin, int32_t row_end, int32_t col_begin, int32_t col_end,
                                               int32_t root_belief, int32_t root_pos, double* gram, double* den, double* mu,
                                               int32_t* info, double* ms3) {
  if (e && !ms3) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_bm_rate_matrix_sites_timed: no buffer for the phase times");
  return rate_matrix_sites(e, row_begin, row_end, col_begin, col_end, root_belief, root_pos, gram, den, mu, info, ms3);
}

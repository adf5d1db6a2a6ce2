// Joint posterior draws of every cluster variable from a calibrated clique tree (pgbp_sample_posterior of include/pgbp.h).
//
// A calibrated clique tree holds the joint: prod clusters / prod sepsets.  Along a preorder of the schedule tree every
// cluster is conditioned on the sepset to its parent: with S the cluster's variables in that sepset and R the rest,
//   x_S = the parent's values,   x_R = J_RR^-1 (h_R - J_RS x_S) + L^-T z_R,   J_RR = L L'.
// Only the copy of x_S depends on the parent, so the work has two phases:
//   factor (sample_factor): one grid over (cluster, site), no dependencies.  [J_RR | J_RS | h_R] is gathered through the
//          scope index into LDS and eliminated with mom_solve's arithmetic (mom_cond_factor, pgbp_mom_dev.hpp); what leaves
//          the LDS is a = J_RR^-1 h_R, G = J_RR^-1 J_RS and T = L^-T: r (m + 1) doubles per (cluster, site), less than the
//          belief's record.  Task shapes by dimension class as in pgbp_moments.hip: up to 16 variables four clusters per
//          wavefront, one per row of 16 lanes (4 x 288 doubles of LDS); up to 64 a wavefront (at most 33 KB: four workgroups
//          per CU); up to 128 a workgroup of 256 threads (up to 133 KB: one workgroup per CU, as the moments kernel).
//   apply  (sample_apply): one launch per preorder level over (cluster of the level, draw, variable) x site:
//          x_R[i] = a_i - sum_j G_ij x_S[j] + sum_{l >= i} T_il z_R[l], every sum in index order by one thread (no atomics),
//          and the copy of x_S.  The factor is computed once however many draws are asked for.
// The factors of a chunk of sites at a time (256 MB at most), z up and x down as one (strided) copy each per chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "pgbp_bs16.hpp"
#include "pgbp_devmem.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_mom_dev.hpp"

namespace pgbp {

extern __shared__ double samp_lds[];

// one cluster of the sweep
struct SampItem {
  int64_t rec_off;   // its record inside a site's belief pool
  int64_t f_off;     // its factor inside a site's factor pool: T' (r x r: T(i, l) at l * r + i), G' (s x r), a (r)
  int64_t x_off;     // its variables inside a (draw, site) of x
  int64_t px_off;    // its parent's
  int32_t cluster, m, r;
  int32_t perm;      // into the index pool: perm[0 .. r) = R, perm[r .. m) = S (positions in the cluster), then the s
                     // positions of S in the parent
};

constexpr int kSampSmallRegion = 16 * 17 + 16;   // doubles of LDS of one row of 16 lanes (m <= 16: ld <= 17)

// NT threads per workgroup, GT per cluster
template <int NT, int GT>
__global__ __launch_bounds__(NT) void sample_factor(const double* __restrict__ pool, int64_t pool_stride, int bs, int fp,
                                                    const SampItem* __restrict__ items, int n_items,
                                                    const int32_t* __restrict__ idx, int region, int site0, int n_sites,
                                                    double* __restrict__ fpool, int64_t f_stride, int32_t* __restrict__ stat,
                                                    int n_clusters) {
#pragma clang fp contract(off)
  constexpr int NG = NT / GT;
  const int t = threadIdx.x, g = t / GT, tg = t - g * GT;
  const int it = blockIdx.x * NG + g;
  const bool have = it < n_items;
  SampItem item{0, 0, 0, 0, 0, 0, 0, 0};
  if (have) item = items[it];
  const int m = item.m, r = item.r, s = m - r, ld = (m + 1) | 1;
  int rb = r;
  if constexpr (NG > 1) {
    rb = 0;
    for (int q = 0; q < NG; ++q) {
      const int o = blockIdx.x * NG + q;
      if (o < n_items) rb = max(rb, items[o].r);
    }
  }
  double* __restrict__ W = samp_lds + (size_t)g * region;
  double* __restrict__ dv = W + r * ld;
  const int32_t* __restrict__ perm = idx + item.perm;
  const bool packed = bs && bs16::applies(m, fp);
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const double* __restrict__ rec = pool + (int64_t)(site0 + site) * pool_stride + item.rec_off;
    const int st = mom_cond_factor<GT>(rec, m, r, rb, perm, packed, fp, W, dv, tg);
    if (!have) continue;
    if (tg == 0) stat[(int64_t)site * n_clusters + item.cluster] = st != 0 ? 1 : 0;
    if (st != 0) continue;   // (sample_apply writes NaN for the whole site and reads no factor of it)
    double* __restrict__ F = fpool + (int64_t)site * f_stride + item.f_off;
    for (int q = tg; q < r * r; q += GT) {
      const int l = q / r, i = q - l * r;
      if (i <= l) F[q] = i == l ? dv[i] : W[l * ld + i];
    }
    double* __restrict__ Gt = F + r * r;
    for (int q = tg; q < s * r; q += GT) {
      const int j = q / r, i = q - j * r;
      Gt[q] = W[i * ld + r + j];
    }
    double* __restrict__ a = Gt + s * r;
    for (int i = tg; i < r; i += GT) a[i] = W[i * ld + m];
  }
}

// info[site] = 1 + the first cluster in preorder whose factorisation failed, or 0: thread t scans the positions t, t + 256, ...
// and keeps its first hit, the 256 candidates are reduced by a fixed tree (integers: any order gives the same minimum)
__global__ __launch_bounds__(256) void sample_info(const int32_t* __restrict__ stat, const int32_t* __restrict__ order,
                                                   int n_clusters, int n_sites, int32_t* __restrict__ info) {
  __shared__ int part[256];
  const int t = threadIdx.x;
  for (int site = blockIdx.x; site < n_sites; site += gridDim.x) {
    int first = 0x7fffffff;
    for (int pos = t; pos < n_clusters; pos += 256)
      if (stat[(int64_t)site * n_clusters + order[pos]] != 0) { first = pos; break; }
    __syncthreads();
    part[t] = first;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) part[t] = min(part[t], part[t + w]);
      __syncthreads();
    }
    if (t == 0) info[site] = part[0] == 0x7fffffff ? 0 : order[part[0]] + 1;
  }
}

// one preorder level: thread = (cluster of the level, draw, variable i < mpad), the sites along blockIdx.y.
// z, x: [n_draws][n_sites][size] of this chunk
__global__ __launch_bounds__(256) void sample_apply(const SampItem* __restrict__ items, int n_items, int mpad, int n_draws,
                                                    int n_sites, const int32_t* __restrict__ idx,
                                                    const double* __restrict__ fpool, int64_t f_stride,
                                                    const int32_t* __restrict__ info, const double* __restrict__ z,
                                                    double* __restrict__ x, int64_t size) {
#pragma clang fp contract(off)
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_items * n_draws * mpad) return;
  const int i = (int)(gid % mpad);
  const int64_t q = gid / mpad;
  const int dr = (int)(q % n_draws);
  const SampItem item = items[q / n_draws];
  const int m = item.m, r = item.r, s = m - r;
  if (i >= m) return;
  const int32_t* __restrict__ perm = idx + item.perm;
  const int32_t* __restrict__ ppos = perm + m;
  const int pos = perm[i];
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const int64_t base = ((int64_t)dr * n_sites + site) * size;
    double* __restrict__ xo = x + base + item.x_off;
    if (info[site] != 0) {
      xo[pos] = NAN;
      continue;
    }
    const double* __restrict__ xp = x + base + item.px_off;
    if (i >= r) {
      xo[pos] = xp[ppos[i - r]];
      continue;
    }
    const double* __restrict__ F = fpool + (int64_t)site * f_stride + item.f_off;
    const double* __restrict__ Gt = F + r * r;
    double acc = Gt[s * r + i];   // a_i
    for (int j = 0; j < s; ++j) acc = fma(-Gt[j * r + i], xp[ppos[j]], acc);
    const double* __restrict__ zi = z + base + item.x_off;
    double nz = 0.0;
    for (int l = i; l < r; ++l) nz = fma(F[l * r + i], zi[perm[l]], nz);
    xo[pos] = acc + nz;
  }
}

// bounds of the call's scratch, in doubles: the factors of a chunk of sites, z (and x) of a chunk of draws (pgbp_sample_scratch_limits)
static std::atomic<int64_t> g_factor_limit{(int64_t)32 << 20}, g_draw_limit{(int64_t)128 << 20};

static size_t sample_lds_bytes(int m) { return sizeof(double) * ((size_t)m * ((m + 1) | 1) + (size_t)m); }

}  // namespace pgbp

using namespace pgbp;

extern "C" int64_t pgbp_sample_size(pgbp_engine* e) {
  if (!e) return -1;
  const Plan& p = *engine_plan(e);
  int64_t n = 0;
  for (int32_t c = 0; c < p.n_clusters; ++c) n += p.dims[c];
  return n;
}

// ms (pgbp_sample_posterior_timed): the stream is drained after every phase and the wall time of the phase is added to
// ms[0 .. 3] = {factor, copy of z, apply, copy of x}
static int sample_posterior(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_draws,
                            const double* z, double* x, int32_t* info, double* ms) {
  if (!e) return PGBP_ERR_INVALID;
  const std::string fn = "pgbp_sample_posterior: ";
  std::vector<SampItem> by_class, by_level;
  std::vector<int32_t> idx, order, level_off, level_mpad;
  int n_class[3] = {0, 0, 0}, max_m[3] = {0, 0, 0};
  int64_t size = 0, f_stride = 0;
  int nc = 0;
  {
    const Plan& p = *engine_peek(e).plan;
    nc = p.n_clusters;
    if (p.trees.empty()) return engine_fail(e, PGBP_ERR_STATE, fn + "no schedule: call pgbp_set_schedule first");
    if (tree < 0 || tree >= (int)p.trees.size())
      return engine_fail(e, PGBP_ERR_INVALID, fn + "schedule tree " + std::to_string(tree) + " out of range (the schedule has " +
                                                  std::to_string(p.trees.size()) + " trees)");
    const Tree& T = p.trees[tree];
    const int ne = (int)T.pa.size();
    // the sweep is the chain rule of a tree-structured joint: every sepset must be an edge of the tree, every cluster on it
    std::vector<int32_t> depth(nc, -1), par_edge(nc, -1);
    bool spans = p.n_sepsets == nc - 1 && ne == nc - 1;
    if (spans) {
      const int root = ne > 0 ? T.pa[0] : 0;
      depth[root] = 0;
      order.push_back(root);
      for (int j = 0; j < ne && spans; ++j) {
        const int pa = T.pa[j], ch = T.ch[j];
        if (depth[pa] < 0 || depth[ch] >= 0) { spans = false; break; }
        depth[ch] = depth[pa] + 1;
        par_edge[ch] = j;
        order.push_back(ch);
      }
    }
    if (!spans)
      return engine_fail(e, PGBP_ERR_INVALID, fn + "schedule tree " + std::to_string(tree) + " (" + std::to_string(ne) +
                                                  " edges) does not span the " + std::to_string(nc) + " clusters, or the graph has a cycle (" +
                                                  std::to_string(p.n_sepsets) + " sepsets): the sweep is exact on a clique tree only");
    for (int c = 0; c < nc; ++c)
      if (p.dims[c] > kLdsMaxDim)
        return engine_fail(e, PGBP_ERR_INVALID, fn + "belief " + std::to_string(c) + " has " + std::to_string(p.dims[c]) +
                                                    " variables, more than the " + std::to_string(kLdsMaxDim) +
                                                    " the moments kernels take");
    if (n_draws < 1) return engine_fail(e, PGBP_ERR_INVALID, fn + "n_draws = " + std::to_string(n_draws) + ", at least one draw is needed");
    if (site_begin < 0 || site_end < site_begin || site_end > p.n_sites)
      return engine_fail(e, PGBP_ERR_INVALID, fn + "site range [" + std::to_string(site_begin) + ", " + std::to_string(site_end) +
                                                  ") outside the engine's " + std::to_string(p.n_sites) + " sites");
    if (!z) return engine_fail(e, PGBP_ERR_INVALID, fn + "no input buffer z");
    if (!x) return engine_fail(e, PGBP_ERR_INVALID, fn + "no output buffer x");
    // items: where every cluster's variables sit in x, its split into R and S, its factor
    std::vector<int64_t> x_off(nc + 1, 0);
    for (int c = 0; c < nc; ++c) x_off[c + 1] = x_off[c] + p.dims[c];
    size = x_off[nc];
    std::vector<SampItem> all(nc);
    int max_depth = 0;
    for (int c = 0; c < nc; ++c) {
      const int m = p.dims[c];
      SampItem it{p.boff[c], f_stride, x_off[c], 0, c, m, m, (int32_t)idx.size()};
      std::vector<char> in_s(m, 0);
      const int32_t *cs = nullptr, *ps = nullptr;
      int s = 0;
      if (par_edge[c] >= 0) {
        const int k = T.sep[par_edge[c]], pa = T.pa[par_edge[c]];
        const int side = p.sepset_clusters[2 * k] == c ? 0 : 1;
        if (p.sepset_clusters[2 * k + side] != c || p.sepset_clusters[2 * k + 1 - side] != pa)
          return engine_fail(e, PGBP_ERR_INVALID, fn + "edge " + std::to_string(par_edge[c]) + " of schedule tree " +
                                                      std::to_string(tree) + " is not sepset " + std::to_string(k));
        cs = p.scope_idx.data() + p.scope_off[2 * k + side];
        ps = p.scope_idx.data() + p.scope_off[2 * k + 1 - side];
        s = (int)(p.scope_off[2 * k + side + 1] - p.scope_off[2 * k + side]);
        it.px_off = x_off[pa];
      }
      for (int j = 0; j < s; ++j) in_s[cs[j]] = 1;
      for (int v = 0; v < m; ++v)
        if (!in_s[v]) idx.push_back(v);
      for (int j = 0; j < s; ++j) idx.push_back(cs[j]);
      for (int j = 0; j < s; ++j) idx.push_back(ps[j]);
      it.r = m - s;
      f_stride += (int64_t)it.r * (m + 1);
      all[c] = it;
      max_depth = std::max(max_depth, depth[c]);
    }
    for (int cl = 0; cl < 3; ++cl)
      for (int c = 0; c < nc; ++c) {
        const int m = all[c].m;
        if (m == 0 || (m <= 16 ? 0 : (m <= 64 ? 1 : 2)) != cl) continue;
        by_class.push_back(all[c]);
        ++n_class[cl];
        max_m[cl] = std::max(max_m[cl], m);
      }
    // the preorder by levels (a cluster's level = its depth in the schedule tree: the level of the preorder message into it)
    std::vector<std::vector<int32_t>> lv(max_depth + 1);
    for (int c : order)
      if (all[c].m > 0) lv[depth[c]].push_back(c);
    level_off.push_back(0);
    for (auto& l : lv) {
      if (l.empty()) continue;
      int mp = 0;
      for (int c : l) { by_level.push_back(all[c]); mp = std::max(mp, all[c].m); }
      level_off.push_back((int32_t)by_level.size());
      level_mpad.push_back(mp);
    }
  }
  const int ns = site_end - site_begin;
  if (ns == 0) return PGBP_OK;
  if (size == 0) {
    if (info) std::fill(info, info + ns, 0);
    return PGBP_OK;
  }
  EngineView v;
  int rc = engine_view(e, &v);
  if (rc) return rc;
  const Plan& p = *v.plan;
  // the factors of a chunk of sites at a time (256 MB at most); z and x of a chunk of draws (1 GB each at most)
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(ns, g_factor_limit.load() / std::max<int64_t>(1, f_stride)));
  const int dchunk = (int)std::max<int64_t>(1, std::min<int64_t>(n_draws, g_draw_limit.load() / ((int64_t)chunk * size)));
  const size_t n_items = by_class.size();
  DevBuf<SampItem> d_items;   // by class, then by level
  DevBuf<int32_t> d_idx, d_order, d_stat, d_info;
  DevBuf<double> d_f, d_z, d_x;
  if (idx.empty()) idx.push_back(0);
  hipError_t herr = (hipError_t)d_items.alloc(2 * n_items);
  if (herr == hipSuccess) herr = (hipError_t)d_idx.alloc(idx.size());
  if (herr == hipSuccess) herr = (hipError_t)d_order.alloc(nc);
  if (herr == hipSuccess) herr = (hipError_t)d_stat.alloc((size_t)chunk * nc);
  if (herr == hipSuccess) herr = (hipError_t)d_info.alloc((size_t)ns);
  if (herr == hipSuccess) herr = (hipError_t)d_f.alloc((size_t)std::max<int64_t>(1, f_stride) * chunk);
  if (herr == hipSuccess) herr = (hipError_t)d_z.alloc((size_t)dchunk * chunk * size);
  if (herr == hipSuccess) herr = (hipError_t)d_x.alloc((size_t)dchunk * chunk * size);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_items.get(), by_class.data(), sizeof(SampItem) * n_items, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_items.get() + n_items, by_level.data(), sizeof(SampItem) * n_items, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_idx.get(), idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) herr = hipMemcpyAsync(d_order.get(), order.data(), sizeof(int32_t) * nc, hipMemcpyHostToDevice, v.st);
  if (herr == hipSuccess) herr = hipMemsetAsync(d_stat.get(), 0, sizeof(int32_t) * (size_t)chunk * nc, v.st);   // (clusters without variables)
  auto t_last = std::chrono::steady_clock::now();
  auto phase = [&](int k) {   // timed variant only
    if (!ms) return;
    const hipError_t perr = hipStreamSynchronize(v.st);
    if (herr == hipSuccess) herr = perr;
    const auto now = std::chrono::steady_clock::now();
    if (k >= 0) ms[k] += std::chrono::duration<double, std::milli>(now - t_last).count();
    t_last = now;
  };
  if (ms) ms[0] = ms[1] = ms[2] = ms[3] = 0.0;
  if (herr == hipSuccess) {
    (void)hipGetLastError();   // (an error an earlier asynchronous call left behind is that call's to report)
    phase(-1);
    const size_t b1 = sample_lds_bytes(max_m[1]), b2 = sample_lds_bytes(max_m[2]);
    if (b2 > 64 * 1024)
      herr = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_factor<256, 256>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)b2);
    const size_t row = sizeof(double) * size;
    for (int s0 = 0; herr == hipSuccess && s0 < ns; s0 += chunk) {
      const int n = std::min(chunk, ns - s0), gy = std::min(n, 65535);
      const SampItem* it = d_items.get();
      if (n_class[0] > 0)
        hipLaunchKernelGGL((sample_factor<64, 16>), dim3((n_class[0] + 3) / 4, gy), dim3(64), sizeof(double) * 4 * kSampSmallRegion,
                           v.st, v.pool, p.pool_stride(), v.bs16, p.fast_p, it, n_class[0], d_idx.get(), kSampSmallRegion,
                           site_begin + s0, n, d_f.get(), f_stride, d_stat.get(), nc);
      it += n_class[0];
      if (n_class[1] > 0)
        hipLaunchKernelGGL((sample_factor<64, 64>), dim3(n_class[1], gy), dim3(64), b1, v.st, v.pool, p.pool_stride(), v.bs16,
                           p.fast_p, it, n_class[1], d_idx.get(), 0, site_begin + s0, n, d_f.get(), f_stride, d_stat.get(), nc);
      it += n_class[1];
      if (n_class[2] > 0)
        hipLaunchKernelGGL((sample_factor<256, 256>), dim3(n_class[2], gy), dim3(256), b2, v.st, v.pool, p.pool_stride(), v.bs16,
                           p.fast_p, it, n_class[2], d_idx.get(), 0, site_begin + s0, n, d_f.get(), f_stride, d_stat.get(), nc);
      hipLaunchKernelGGL(sample_info, dim3(gy), dim3(256), 0, v.st, d_stat.get(), d_order.get(), nc, n, d_info.get() + s0);
      phase(0);
      for (int d0 = 0; herr == hipSuccess && d0 < n_draws; d0 += dchunk) {
        const int nd = std::min(dchunk, n_draws - d0);
        // rows = draws: [nd][n][size] on the device, [n_draws][ns][size] on the host
        if (n == ns)
          herr = hipMemcpyAsync(d_z.get(), z + (size_t)d0 * ns * size, row * n * nd, hipMemcpyHostToDevice, v.st);
        else
          herr = hipMemcpy2DAsync(d_z.get(), row * n, z + ((size_t)d0 * ns + s0) * size, row * ns, row * n, nd, hipMemcpyHostToDevice, v.st);
        phase(1);
        for (size_t l = 0; herr == hipSuccess && l + 1 < level_off.size(); ++l) {
          const int ni = level_off[l + 1] - level_off[l], mp = level_mpad[l];
          const int64_t threads = (int64_t)ni * nd * mp;
          hipLaunchKernelGGL(sample_apply, dim3((unsigned)((threads + 255) / 256), gy), dim3(256), 0, v.st,
                             d_items.get() + n_items + level_off[l], ni, mp, nd, n, d_idx.get(), d_f.get(), f_stride, d_info.get() + s0, d_z.get(), d_x.get(), size);
        }
        if (herr == hipSuccess) herr = hipGetLastError();
        phase(2);
        if (herr == hipSuccess && n == ns)
          herr = hipMemcpyAsync(x + (size_t)d0 * ns * size, d_x.get(), row * n * nd, hipMemcpyDeviceToHost, v.st);
        else if (herr == hipSuccess)
          herr = hipMemcpy2DAsync(x + ((size_t)d0 * ns + s0) * size, row * ns, d_x.get(), row * n, row * n, nd, hipMemcpyDeviceToHost, v.st);
        phase(3);
      }
    }
  }
  if (herr == hipSuccess && info) herr = hipMemcpyAsync(info, d_info.get(), sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, v.st);
  const hipError_t serr = hipStreamSynchronize(v.st);   // (also when something failed: the uploads read this call's locals)
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, fn + hipGetErrorString(herr));
  return PGBP_OK;
}

extern "C" int pgbp_sample_posterior(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_draws,
                                     const double* z, double* x, int32_t* info) {
  return sample_posterior(e, tree, site_begin, site_end, n_draws, z, x, info, nullptr);
}

extern "C" int pgbp_sample_posterior_timed(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_draws,
                                           const double* z, double* x, int32_t* info, double* ms4) {
  if (e && !ms4) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_sample_posterior_timed: no buffer for the phase times");
  return sample_posterior(e, tree, site_begin, site_end, n_draws, z, x, info, ms4);
}

extern "C" void pgbp_sample_scratch_limits(int64_t factor_doubles, int64_t draw_doubles) {
  g_factor_limit.store(factor_doubles > 0 ? factor_doubles : (int64_t)32 << 20);
  g_draw_limit.store(draw_doubles > 0 ? draw_doubles : (int64_t)128 << 20);
}

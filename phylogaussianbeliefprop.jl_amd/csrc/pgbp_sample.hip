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
//
// The same factors give the exact posterior covariance of any two entries (pgbp_posterior_cov): at one site the sweep is linear,
// x = m + A z, and the adjoint sweep w = A'c runs the levels from the deepest to the root (cov_adjoint, cov_w), k = A w the apply
// without its offset (cov_forward).  Both entry points share the host-side plan (sample_plan) and the factor phase (SampDev).
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
#include "pgbp_sample_plan.hpp"

namespace pgbp {

extern __shared__ double samp_lds[];

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

// ---- pgbp_posterior_cov: the adjoint of the sweep above.  At one site the sampler is x = m + A z; for a functional c the call
// returns w = A'c (cov_adjoint level by level from the deepest, then cov_w) and k = A w (cov_forward, sample_apply without the
// offset).  c: [n_cols][size], shared by the sites; xb, w: [n_cols][n_sites][size] of this chunk, k is written over xb.

// one level of the adjoint, in gather form: thread = (cluster P of the level, column, variable v < mpad) forms
//   xbar_P[v] = c_P[v] + sum over P's children in index order, then over their S positions j that map to v, of
//               (xbar_C[S_j] - sum_i G_ij xbar_C[R_i]),
// every child's xbar being final (the level below ran before).  start[e] .. start[e + 1]: the (child among `items`, j) pairs of
// entry e of the layout in `pairs`.  `items`: all of them by level, P = first + ...
__global__ __launch_bounds__(256) void cov_adjoint(const SampItem* __restrict__ items, int first, int n_items, int mpad, int n_cols,
                                                   int n_sites, const int32_t* __restrict__ idx, const int32_t* __restrict__ start,
                                                   const int32_t* __restrict__ pairs, const double* __restrict__ fpool, int64_t f_stride,
                                                   const int32_t* __restrict__ info, const double* __restrict__ c,
                                                   double* __restrict__ xb, int64_t size) {
#pragma clang fp contract(off)
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_items * n_cols * mpad) return;
  const int vv = (int)(gid % mpad);
  const int64_t q = gid / mpad;
  const int col = (int)(q % n_cols);
  const int P = first + (int)(q / n_cols);
  const SampItem item = items[P];
  if (vv >= item.m) return;
  const int e0 = start[item.x_off + vv], e1 = start[item.x_off + vv + 1];
  const double cv = c[(int64_t)col * size + item.x_off + vv];
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    if (info[site] != 0) continue;   // (cov_w and cov_forward write the NaN; no factor of the site is read)
    const int64_t base = ((int64_t)col * n_sites + site) * size;
    double acc = cv;
    for (int e = e0; e < e1; ++e) {
      const SampItem ch = items[pairs[2 * e]];
      const int j = pairs[2 * e + 1], r = ch.r;
      const int32_t* __restrict__ cperm = idx + ch.perm;
      const double* __restrict__ xc = xb + base + ch.x_off;
      const double* __restrict__ Gj = fpool + (int64_t)site * f_stride + ch.f_off + (int64_t)r * r + (int64_t)j * r;
      double t = xc[cperm[r + j]];
      for (int i = 0; i < r; ++i) t = fma(-Gj[i], xc[cperm[i]], t);
      acc += t;
    }
    xb[base + item.x_off + vv] = acc;
  }
}

// w_C[R_l] = sum_{i <= l} T_il xbar_C[R_i], +0.0 at the S positions: one flat launch over (cluster, column, variable l < mpad)
__global__ __launch_bounds__(256) void cov_w(const SampItem* __restrict__ items, int n_items, int mpad, int n_cols, int n_sites,
                                             const int32_t* __restrict__ idx, const double* __restrict__ fpool, int64_t f_stride,
                                             const int32_t* __restrict__ info, const double* __restrict__ xb,
                                             double* __restrict__ w, int64_t size) {
#pragma clang fp contract(off)
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_items * n_cols * mpad) return;
  const int l = (int)(gid % mpad);
  const int64_t q = gid / mpad;
  const int col = (int)(q % n_cols);
  const SampItem item = items[q / n_cols];
  const int m = item.m, r = item.r;
  if (l >= m) return;
  const int32_t* __restrict__ perm = idx + item.perm;
  const int pos = perm[l];
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const int64_t base = ((int64_t)col * n_sites + site) * size + item.x_off;
    if (info[site] != 0) {
      w[base + pos] = NAN;
      continue;
    }
    double acc = 0.0;
    if (l < r) {
      const double* __restrict__ Tl = fpool + (int64_t)site * f_stride + item.f_off + (int64_t)l * r;
      for (int i = 0; i <= l; ++i) acc = fma(Tl[i], xb[base + perm[i]], acc);
    }
    w[base + pos] = acc;
  }
}

// one preorder level of k = A w: sample_apply with w for z and without the offset a
__global__ __launch_bounds__(256) void cov_forward(const SampItem* __restrict__ items, int n_items, int mpad, int n_cols,
                                                   int n_sites, const int32_t* __restrict__ idx,
                                                   const double* __restrict__ fpool, int64_t f_stride,
                                                   const int32_t* __restrict__ info, const double* __restrict__ w,
                                                   double* __restrict__ k, int64_t size) {
#pragma clang fp contract(off)
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_items * n_cols * mpad) return;
  const int i = (int)(gid % mpad);
  const int64_t q = gid / mpad;
  const int col = (int)(q % n_cols);
  const SampItem item = items[q / n_cols];
  const int m = item.m, r = item.r, s = m - r;
  if (i >= m) return;
  const int32_t* __restrict__ perm = idx + item.perm;
  const int32_t* __restrict__ ppos = perm + m;
  const int pos = perm[i];
  for (int site = blockIdx.y; site < n_sites; site += gridDim.y) {
    const int64_t base = ((int64_t)col * n_sites + site) * size;
    double* __restrict__ ko = k + base + item.x_off;
    if (info[site] != 0) {
      ko[pos] = NAN;
      continue;
    }
    const double* __restrict__ kp = k + base + item.px_off;
    if (i >= r) {
      ko[pos] = kp[ppos[i - r]];
      continue;
    }
    const double* __restrict__ F = fpool + (int64_t)site * f_stride + item.f_off;
    const double* __restrict__ Gt = F + r * r;
    double acc = 0.0;
    for (int j = 0; j < s; ++j) acc = fma(-Gt[j * r + i], kp[ppos[j]], acc);
    const double* __restrict__ wi = w + base + item.x_off;
    double nz = 0.0;
    for (int l = i; l < r; ++l) nz = fma(F[l * r + i], wi[perm[l]], nz);
    ko[pos] = acc + nz;
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

// the sites whose factors are held at a time
static int sample_site_chunk(const SampPlan& sp, int ns) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(ns, g_factor_limit.load() / std::max<int64_t>(1, sp.f_stride)));
}

// What both sweeps keep on the device, and the factor phase of a chunk of sites.
struct SampDev {
  DevBuf<SampItem> items;   // by class, then by level
  DevBuf<int32_t> idx, order, stat, info;
  DevBuf<double> f;
  size_t n_items = 0, b1 = 0, b2 = 0;

  const SampItem* by_level() const { return items.get() + n_items; }

  hipError_t upload(const EngineView& v, SampPlan& sp, int chunk, int ns) {
    n_items = sp.by_class.size();
    const int nc = sp.nc;
    if (sp.idx.empty()) sp.idx.push_back(0);
    hipError_t herr = (hipError_t)items.alloc(2 * n_items);
    if (herr == hipSuccess) herr = (hipError_t)idx.alloc(sp.idx.size());
    if (herr == hipSuccess) herr = (hipError_t)order.alloc(nc);
    if (herr == hipSuccess) herr = (hipError_t)stat.alloc((size_t)chunk * nc);
    if (herr == hipSuccess) herr = (hipError_t)info.alloc((size_t)ns);
    if (herr == hipSuccess) herr = (hipError_t)f.alloc((size_t)std::max<int64_t>(1, sp.f_stride) * chunk);
    if (herr == hipSuccess) herr = hipMemcpyAsync(items.get(), sp.by_class.data(), sizeof(SampItem) * n_items, hipMemcpyHostToDevice, v.st);
    if (herr == hipSuccess) herr = hipMemcpyAsync(items.get() + n_items, sp.by_level.data(), sizeof(SampItem) * n_items, hipMemcpyHostToDevice, v.st);
    if (herr == hipSuccess) herr = hipMemcpyAsync(idx.get(), sp.idx.data(), sizeof(int32_t) * sp.idx.size(), hipMemcpyHostToDevice, v.st);
    if (herr == hipSuccess) herr = hipMemcpyAsync(order.get(), sp.order.data(), sizeof(int32_t) * nc, hipMemcpyHostToDevice, v.st);
    if (herr == hipSuccess) herr = hipMemsetAsync(stat.get(), 0, sizeof(int32_t) * (size_t)chunk * nc, v.st);   // (clusters without variables)
    return herr;
  }

  hipError_t prepare(const SampPlan& sp) {
    b1 = sample_lds_bytes(sp.max_m[1]);
    b2 = sample_lds_bytes(sp.max_m[2]);
    if (b2 > 64 * 1024)
      return hipFuncSetAttribute(reinterpret_cast<const void*>(sample_factor<256, 256>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)b2);
    return hipSuccess;
  }

  // the factors and info of the n sites from site_begin + s0 (info at s0 of the call's)
  void factor(const EngineView& v, const SampPlan& sp, int site_begin, int s0, int n) {
    const Plan& p = *v.plan;
    const int gy = std::min(n, 65535), nc = sp.nc;
    const int* n_class = sp.n_class;
    const int64_t f_stride = sp.f_stride;
    const SampItem* it = items.get();
    if (n_class[0] > 0)
      hipLaunchKernelGGL((sample_factor<64, 16>), dim3((n_class[0] + 3) / 4, gy), dim3(64), sizeof(double) * 4 * kSampSmallRegion,
                         v.st, v.pool, p.pool_stride(), v.bs16, p.fast_p, it, n_class[0], idx.get(), kSampSmallRegion,
                         site_begin + s0, n, f.get(), f_stride, stat.get(), nc);
    it += n_class[0];
    if (n_class[1] > 0)
      hipLaunchKernelGGL((sample_factor<64, 64>), dim3(n_class[1], gy), dim3(64), b1, v.st, v.pool, p.pool_stride(), v.bs16,
                         p.fast_p, it, n_class[1], idx.get(), 0, site_begin + s0, n, f.get(), f_stride, stat.get(), nc);
    it += n_class[1];
    if (n_class[2] > 0)
      hipLaunchKernelGGL((sample_factor<256, 256>), dim3(n_class[2], gy), dim3(256), b2, v.st, v.pool, p.pool_stride(), v.bs16,
                         p.fast_p, it, n_class[2], idx.get(), 0, site_begin + s0, n, f.get(), f_stride, stat.get(), nc);
    hipLaunchKernelGGL(sample_info, dim3(gy), dim3(256), 0, v.st, stat.get(), order.get(), nc, n, info.get() + s0);
  }
};

// ms (pgbp_sample_posterior_timed): the stream is drained after every phase and the wall time of the phase is added to
// ms[0 .. 3] = {factor, copy of z, apply, copy of x}
static int sample_posterior(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_draws,
                            const double* z, double* x, int32_t* info, double* ms) {
  if (!e) return PGBP_ERR_INVALID;
  const std::string fn = "pgbp_sample_posterior: ";
  SampPlan sp;
  const int prc = sample_plan(e, fn, tree, site_begin, site_end, n_draws, "n_draws", "draw",
                              [&]() { return std::string(!z ? "no input buffer z" : (!x ? "no output buffer x" : "")); }, sp);
  if (prc) return prc;
  const std::vector<int32_t>&level_off = sp.level_off, &level_mpad = sp.level_mpad;
  const int64_t size = sp.size, f_stride = sp.f_stride;
  const int ns = site_end - site_begin;
  if (ns == 0) return PGBP_OK;
  if (size == 0) {
    if (info) std::fill(info, info + ns, 0);
    return PGBP_OK;
  }
  EngineView v;
  int rc = engine_view(e, &v);
  if (rc) return rc;
  // the factors of a chunk of sites at a time (256 MB at most); z and x of a chunk of draws (1 GB each at most)
  const int chunk = sample_site_chunk(sp, ns);
  const int dchunk = (int)std::max<int64_t>(1, std::min<int64_t>(n_draws, g_draw_limit.load() / ((int64_t)chunk * size)));
  SampDev d;
  DevBuf<double> d_z, d_x;
  hipError_t herr = d.upload(v, sp, chunk, ns);
  if (herr == hipSuccess) herr = (hipError_t)d_z.alloc((size_t)dchunk * chunk * size);
  if (herr == hipSuccess) herr = (hipError_t)d_x.alloc((size_t)dchunk * chunk * size);
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
    herr = d.prepare(sp);
    const size_t row = sizeof(double) * size;
    for (int s0 = 0; herr == hipSuccess && s0 < ns; s0 += chunk) {
      const int n = std::min(chunk, ns - s0), gy = std::min(n, 65535);
      d.factor(v, sp, site_begin, s0, n);
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
                             d.by_level() + level_off[l], ni, mp, nd, n, d.idx.get(), d.f.get(), f_stride, d.info.get() + s0, d_z.get(), d_x.get(), size);
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
  if (herr == hipSuccess && info) herr = hipMemcpyAsync(info, d.info.get(), sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, v.st);
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

// ms (pgbp_posterior_cov_timed): as sample_posterior's, ms[0 .. 4] = {factor, copy of c, adjoint (with w), forward, copies of w and k}
static int posterior_cov(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_cols, const double* c,
                         double* w, double* k, int32_t* info, double* ms) {
  if (!e) return PGBP_ERR_INVALID;
  const std::string fn = "pgbp_posterior_cov: ";
  SampPlan sp;
  const int prc = sample_plan(e, fn, tree, site_begin, site_end, n_cols, "n_cols", "column",
                              [&]() { return std::string(!c ? "no input buffer c" : (!w && !k ? "no output buffer: w and k are both NULL" : "")); }, sp);
  if (prc) return prc;
  const std::vector<int32_t>&level_off = sp.level_off, &level_mpad = sp.level_mpad;
  const int64_t size = sp.size, f_stride = sp.f_stride;
  const int ns = site_end - site_begin;
  if (ns == 0) return PGBP_OK;
  if (size == 0) {
    if (info) std::fill(info, info + ns, 0);
    return PGBP_OK;
  }
  // the gather lists of the adjoint, behind the index pool: one offset per entry of the layout (and the end), then the
  // (child among the items by level, j) pairs, sorted by the parent's entry -- a counting sort, so the pairs of one entry keep
  // the order they are met in: the children in index order, a child's S positions in order
  const int n_items = (int)sp.by_level.size();
  const size_t start0 = sp.idx.size();
  int mpad_all = 0;
  {
    std::vector<int32_t> at(sp.nc, -1);
    size_t n_pairs = 0;
    for (int q = 0; q < n_items; ++q) {
      const SampItem& it = sp.by_level[q];
      at[it.cluster] = q;
      mpad_all = std::max(mpad_all, (int)it.m);
      n_pairs += (size_t)(it.m - it.r);
    }
    sp.idx.resize(start0 + (size_t)size + 1 + 2 * n_pairs, 0);
    int32_t* start = sp.idx.data() + start0;
    int32_t* pairs = start + size + 1;
    auto each_pair = [&](auto&& f) {
      for (int ch = 0; ch < sp.nc; ++ch) {
        if (at[ch] < 0) continue;
        const SampItem& it = sp.by_level[at[ch]];   // (the root has no S)
        for (int j = 0; j < it.m - it.r; ++j) f(it.px_off + sp.idx[it.perm + it.m + j], at[ch], j);
      }
    };
    each_pair([&](int64_t entry, int, int) { ++start[entry + 1]; });
    for (int64_t q = 0; q < size; ++q) start[q + 1] += start[q];
    each_pair([&](int64_t entry, int child, int j) {   // (start[entry] walks to the end of its list ...)
      const size_t o = 2 * (size_t)start[entry]++;
      pairs[o] = child;
      pairs[o + 1] = j;
    });
    for (int64_t q = size; q > 0; --q) start[q] = start[q - 1];   // (... which is where the next one begins)
    start[0] = 0;
  }
  EngineView v;
  int rc = engine_view(e, &v);
  if (rc) return rc;
  // the factors of a chunk of sites at a time; xbar (then k) and w of a chunk of columns, by the sampler's draw limit
  const int chunk = sample_site_chunk(sp, ns);
  const int cchunk = (int)std::max<int64_t>(1, std::min<int64_t>(n_cols, g_draw_limit.load() / ((int64_t)chunk * size)));
  SampDev d;
  DevBuf<double> d_c, d_w, d_k;
  hipError_t herr = d.upload(v, sp, chunk, ns);
  if (herr == hipSuccess) herr = (hipError_t)d_c.alloc((size_t)cchunk * size);
  if (herr == hipSuccess) herr = (hipError_t)d_w.alloc((size_t)cchunk * chunk * size);
  if (herr == hipSuccess) herr = (hipError_t)d_k.alloc((size_t)cchunk * chunk * size);
  auto t_last = std::chrono::steady_clock::now();
  auto phase = [&](int q) {   // timed variant only
    if (!ms) return;
    const hipError_t perr = hipStreamSynchronize(v.st);
    if (herr == hipSuccess) herr = perr;
    const auto now = std::chrono::steady_clock::now();
    if (q >= 0) ms[q] += std::chrono::duration<double, std::milli>(now - t_last).count();
    t_last = now;
  };
  if (ms) std::fill(ms, ms + 5, 0.0);
  if (herr == hipSuccess) {
    (void)hipGetLastError();   // (an error an earlier asynchronous call left behind is that call's to report)
    phase(-1);
    herr = d.prepare(sp);
    const size_t row = sizeof(double) * size;
    const int32_t* start = d.idx.get() + start0;
    const int32_t* pairs = start + size + 1;
    const int n_levels = (int)level_off.size() - 1;
    auto down = [&](double* host, const double* dev, int s0, int n, int c0, int ncol) {   // [ncol][n][size] -> [n_cols][ns][size]
      if (n == ns) return hipMemcpyAsync(host + (size_t)c0 * ns * size, dev, row * n * ncol, hipMemcpyDeviceToHost, v.st);
      return hipMemcpy2DAsync(host + ((size_t)c0 * ns + s0) * size, row * ns, dev, row * n, row * n, ncol, hipMemcpyDeviceToHost, v.st);
    };
    for (int s0 = 0; herr == hipSuccess && s0 < ns; s0 += chunk) {
      const int n = std::min(chunk, ns - s0), gy = std::min(n, 65535);
      d.factor(v, sp, site_begin, s0, n);
      phase(0);
      for (int c0 = 0; herr == hipSuccess && c0 < n_cols; c0 += cchunk) {
        const int ncol = std::min(cchunk, n_cols - c0);
        herr = hipMemcpyAsync(d_c.get(), c + (size_t)c0 * size, row * ncol, hipMemcpyHostToDevice, v.st);
        phase(1);
        for (int l = n_levels - 1; herr == hipSuccess && l >= 0; --l) {
          const int ni = level_off[l + 1] - level_off[l], mp = level_mpad[l];
          const int64_t threads = (int64_t)ni * ncol * mp;
          hipLaunchKernelGGL(cov_adjoint, dim3((unsigned)((threads + 255) / 256), gy), dim3(256), 0, v.st, d.by_level(), level_off[l],
                             ni, mp, ncol, n, d.idx.get(), start, pairs, d.f.get(), f_stride, d.info.get() + s0, d_c.get(), d_k.get(), size);
        }
        if (herr == hipSuccess) {
          const int64_t threads = (int64_t)n_items * ncol * mpad_all;
          hipLaunchKernelGGL(cov_w, dim3((unsigned)((threads + 255) / 256), gy), dim3(256), 0, v.st, d.by_level(), n_items, mpad_all,
                             ncol, n, d.idx.get(), d.f.get(), f_stride, d.info.get() + s0, d_k.get(), d_w.get(), size);
          herr = hipGetLastError();
        }
        phase(2);
        for (int l = 0; k && herr == hipSuccess && l < n_levels; ++l) {
          const int ni = level_off[l + 1] - level_off[l], mp = level_mpad[l];
          const int64_t threads = (int64_t)ni * ncol * mp;
          hipLaunchKernelGGL(cov_forward, dim3((unsigned)((threads + 255) / 256), gy), dim3(256), 0, v.st, d.by_level() + level_off[l],
                             ni, mp, ncol, n, d.idx.get(), d.f.get(), f_stride, d.info.get() + s0, d_w.get(), d_k.get(), size);
        }
        if (herr == hipSuccess) herr = hipGetLastError();
        phase(3);
        if (herr == hipSuccess && w) herr = down(w, d_w.get(), s0, n, c0, ncol);
        if (herr == hipSuccess && k) herr = down(k, d_k.get(), s0, n, c0, ncol);
        phase(4);
      }
    }
  }
  if (herr == hipSuccess && info) herr = hipMemcpyAsync(info, d.info.get(), sizeof(int32_t) * (size_t)ns, hipMemcpyDeviceToHost, v.st);
  const hipError_t serr = hipStreamSynchronize(v.st);   // (also when something failed: the uploads read this call's locals)
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, fn + hipGetErrorString(herr));
  return PGBP_OK;
}

extern "C" int pgbp_posterior_cov(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_cols,
                                  const double* c, double* w, double* k, int32_t* info) {
  return posterior_cov(e, tree, site_begin, site_end, n_cols, c, w, k, info, nullptr);
}

extern "C" int pgbp_posterior_cov_timed(pgbp_engine* e, int32_t tree, int32_t site_begin, int32_t site_end, int32_t n_cols,
                                        const double* c, double* w, double* k, int32_t* info, double* ms5) {
  if (e && !ms5) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_posterior_cov_timed: no buffer for the phase times");
  return posterior_cov(e, tree, site_begin, site_end, n_cols, c, w, k, info, ms5);
}

extern "C" void pgbp_sample_scratch_limits(int64_t factor_doubles, int64_t draw_doubles) {
  g_factor_limit.store(factor_doubles > 0 ? factor_doubles : (int64_t)32 << 20);
  g_draw_limit.store(draw_doubles > 0 ? draw_doubles : (int64_t)128 << 20);
}

// Draws of every node of the network from the CURRENT linear-Gaussian model (pgbp_lg_simulate of include/pgbp.h): the model
// run forwards.  Sites are replicates.  Family f (child x_f, parents pf(k) by pgbp_lg_set_topology) has
//   x_f = sum_k qc_k x_pf(k) + off_f + L_f z_f,      V_f = sum_k vc_k R[colour_k] (+ E_f) = L_f L_f',
//   off_f = (sum_k wc_k) theta + sum_k gamma_k s_k + sum over the parents that are the fixed root of qc_k mu
// (a root-prior family: x = mu + chol(R[colour]) z).  Only the sum over the parents depends on other families, so the work has
// two phases, as in pgbp_sample.hip:
//   factor (sim_factor): one grid over (family, parameter set), no dependencies.  The parameter set is ONE when parameters,
//          shifts and noise are all shared -- the phase then runs once however many sites -- and one per site of the chunk
//          otherwise.  V_f is formed in LDS from lg_coefs<false>, the noise and the shifts of pgbp_fam_dev.hpp and factored by
//          lds_cholesky; what leaves the LDS is the record [L_f packed by rows (p (p + 1) / 2) | qc (K) | off (p)].  Up to 16
//          traits four families per wavefront, one per row of 16 lanes; up to 64 a wavefront per family (33 KB of LDS).
//          p = 1 (sim_factor_uni): a thread per (family, set) and scalars only -- a univariate batch with its own parameters
//          per site has as many records as states.
//   apply  (sim_apply): one launch per topology level over (family of the level, site, trait): the parents' states from the
//          state buffer, the family's own row of L_f against z, every sum in index order by one thread (no atomics); tips
//          write the engine's data buffers as well.  Multivariate engines: state [site][family][trait], (family, trait) the
//          minor thread index.  Univariate batches that keep the [row][site] copy of the data: state [family][site] (rows
//          padded: sm_row), adjacent lanes = adjacent sites, so that states, normals and data_sm rows move as whole lines.
// The normals come from the host (z) or from sim_normals: Philox4x32-10 keyed by the seed, counter (family, trait pair,
// absolute site, 0), one Box-Muller pair per counter -- stateless, so a value does not depend on the chunking.
// Scratch: the factor pool and the state / normal buffers of a chunk of sites (pgbp_simulate_scratch_limits).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "pgbp_devmem.hpp"
#include "pgbp_fam_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"
#include "pgbp_philox_dev.hpp"
#include "pgbp_topology.hpp"

namespace pgbp {

extern __shared__ double sim_lds[];

// doubles of one family's record in the factor pool: L(i, j), j <= i, at i (i + 1) / 2 + j; then qc[K]; then off[p]
__host__ __device__ inline int64_t sim_rec(int p, int K) { return (int64_t)p * (p + 1) / 2 + K + p; }
// doubles of LDS of one family: V (p x ld, ld odd), the diagonal of L, the coefficient rows qc, vc, wc
__host__ __device__ inline int sim_ld(int p) { return p | 1; }
__host__ __device__ inline int sim_region(int p, int K) { return (p * sim_ld(p) + p + 3 * K + 1) & ~1; }

// a tip family with a data row: its state is what the engine's data hold
__device__ __forceinline__ bool sim_is_tip(const LgStatic& F, int f) {
  return F.child_pos[f] < 0 && F.data_row[f] >= 0 && F.n_parents[f] >= 1;
}

// GT threads per family, 64 / GT families per workgroup (one wavefront: its barriers are the wavefront's own, so the rows may
// leave lds_cholesky at different pivots).  set s of the chunk: absolute site site0 + s when per_set, the shared set otherwise
template <int GT>
__global__ __launch_bounds__(64) void sim_factor(LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz,
                                                 const int32_t* __restrict__ pf, int nf, int site0, int n_sets, int per_set,
                                                 double* __restrict__ fpool, int64_t f_stride, int32_t* __restrict__ stat) {
#pragma clang fp contract(off)
  constexpr int NG = kWave / GT;
  const int t = threadIdx.x, g = t / GT, tg = t - g * GT;
  const int f = blockIdx.x * NG + g;
  if (f >= nf) return;
  const int p = F.p, K = F.K, ld = sim_ld(p), np = F.n_parents[f];
  double* __restrict__ A = sim_lds + (size_t)g * sim_region(p, K);
  double* __restrict__ dl = A + p * ld;
  double* __restrict__ cf = dl + p;   // [3][K]: qc, vc, wc
  const int64_t rec = sim_rec(p, K);
  const int sn = lg_noise_slot(Nz, f);
  for (int s = blockIdx.y; s < n_sets; s += gridDim.y) {
    const int64_t as = per_set ? (int64_t)site0 + s : 0;
    const LgSite S = lg_site(M, F.n_rates, p, as);
    __syncthreads();   // (the previous set's reads)
    for (int k = tg; k < np; k += GT)
      lg_coefs<false>(M.model, S.alpha, F.length[(size_t)f * K + k], F.gamma[(size_t)f * K + k], cf[k], cf[K + k], cf[2 * K + k]);
    __syncthreads();
    // the lower triangle of V_f, all p traits
    for (int idx = tg; idx < p * p; idx += GT) {
      const int j = idx / p, i = idx - j * p;
      if (i < j) continue;
      const int e = i + j * p;
      double v = 0.0;
      if (np == 0) {
        v = S.R[(int64_t)F.color[(size_t)f * K] * p * p + e];
      } else {
        for (int k = 0; k < np; ++k) v = v + cf[K + k] * S.R[(int64_t)F.color[(size_t)f * K + k] * p * p + e];
      }
      if (sn >= 0) v = v + lg_noise_E(Nz, sn, i, j, p, as);   // a noisy tip: the observation
      A[i * ld + j] = v;
    }
    __syncthreads();
    const bool ok = lds_cholesky<GT>(A, p, ld, dl, nullptr, tg);
    if (tg == 0) stat[(int64_t)s * nf + f] = ok ? 0 : 1;
    if (!ok) continue;   // (sim_apply writes NaN for the whole site and reads no record of it)
    double* __restrict__ o = fpool + (int64_t)s * f_stride + (int64_t)f * rec;
    for (int idx = tg; idx < p * p; idx += GT) {
      const int i = idx / p, j = idx - i * p;
      if (j <= i) o[i * (i + 1) / 2 + j] = i == j ? dl[i] : A[i * ld + j];
    }
    double* __restrict__ oq = o + p * (p + 1) / 2;
    for (int k = tg; k < K; k += GT) oq[k] = (k < np && pf[(size_t)f * K + k] >= 0) ? cf[k] : 0.0;
    double* __restrict__ oo = oq + K;
    for (int tr = tg; tr < p; tr += GT) {
      double w = 0.0;
      if (np == 0) {
        w = S.mu[tr];
      } else {
        if (S.theta) {
          double c = 0.0;
          for (int k = 0; k < np; ++k) c = c + cf[2 * K + k];
          w = c * S.theta[tr];
        }
        w = w + lg_shift_d(Sh, F.gamma, f, K, np, tr, p, as);
        for (int k = 0; k < np; ++k)
          if (pf[(size_t)f * K + k] == kTopoFixedRoot) w = w + cf[k] * S.mu[tr];
      }
      oo[tr] = w;
    }
  }
}

// p = 1: a thread per (family, set), everything a scalar: L = sqrt(V), the record [L | qc (K) | off].  SM: thread = set, the
// families along blockIdx.y, and the records in the [family][entry][set] order (pss = 1, pfs = the padded row), so that
// adjacent lanes write adjacent doubles here and read them in sim_apply<true>; else thread = family, the sets along
// blockIdx.y, records as sim_factor leaves them.  stat (zeroed by the caller) is written for a failed family only.
template <bool SM>
__global__ __launch_bounds__(256) void sim_factor_uni(LgStatic F, LgParams M, LgShifts Sh, LgNoise Nz,
                                                      const int32_t* __restrict__ pf, int nf, int site0, int n_sets, int per_set,
                                                      double* __restrict__ fpool, int64_t pss, int64_t pfs,
                                                      int32_t* __restrict__ stat) {
#pragma clang fp contract(off)
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (SM ? (int64_t)n_sets : (int64_t)nf)) return;
  const int K = F.K, n_outer = SM ? nf : n_sets;
  const int64_t rec = sim_rec(1, K);
  for (int o = blockIdx.y; o < n_outer; o += gridDim.y) {
    const int s = SM ? (int)gid : o, f = SM ? o : (int)gid;
    const int64_t as = per_set ? (int64_t)site0 + s : 0;
    const LgSite S = lg_site(M, F.n_rates, 1, as);
    const int np = F.n_parents[f];
    double* __restrict__ r = fpool + (int64_t)s * pss + (int64_t)f * rec * pfs;
    double V = 0.0, w = 0.0;
    if (np == 0) {
      V = S.R[F.color[(size_t)f * K]];
      w = S.mu[0];
      for (int k = 0; k < K; ++k) r[(1 + k) * pfs] = 0.0;
    } else {
      double c = 0.0;
      for (int k = 0; k < K; ++k) {
        double qc = 0.0, vc, wc;
        if (k < np) {
          lg_coefs<false>(M.model, S.alpha, F.length[(size_t)f * K + k], F.gamma[(size_t)f * K + k], qc, vc, wc);
          V = V + vc * S.R[F.color[(size_t)f * K + k]];
          c = c + wc;
          if (pf[(size_t)f * K + k] < 0) qc = 0.0;
        }
        r[(1 + k) * pfs] = qc;
      }
      if (S.theta) w = c * S.theta[0];
      w = w + lg_shift_d(Sh, F.gamma, f, K, np, 0, 1, as);
      for (int k = 0; k < np; ++k)
        if (pf[(size_t)f * K + k] == kTopoFixedRoot) {
          double qc, vc, wc;
          lg_coefs<false>(M.model, S.alpha, F.length[(size_t)f * K + k], F.gamma[(size_t)f * K + k], qc, vc, wc);
          w = w + qc * S.mu[0];
        }
    }
    const int sn = lg_noise_slot(Nz, f);
    if (sn >= 0) V = V + lg_noise_E(Nz, sn, 0, 0, 1, as);
    if (!(V > 0.0)) stat[(int64_t)s * nf + f] = 1;
    r[0] = sqrt(V);
    r[(1 + K) * pfs] = w;
  }
}

// info[set] = 1 + the first family whose V_f is not positive definite, or 0 (sample_info of pgbp_sample.hip, in index order)
__global__ __launch_bounds__(256) void sim_info(const int32_t* __restrict__ stat, int nf, int n_sets, int32_t* __restrict__ info) {
  __shared__ int part[256];
  const int t = threadIdx.x;
  for (int s = blockIdx.x; s < n_sets; s += gridDim.x) {
    int first = 0x7fffffff;
    for (int f = t; f < nf; f += 256)
      if (stat[(int64_t)s * nf + f] != 0) { first = f; break; }
    __syncthreads();
    part[t] = first;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) part[t] = min(part[t], part[t + w]);
      __syncthreads();
    }
    if (t == 0) info[s] = part[0] == 0x7fffffff ? 0 : part[0] + 1;
  }
}

// thread = (site, family, trait pair); z at s * ss + (f * p + t) * fs.  sm: the sites are the minor thread index
__global__ __launch_bounds__(256) void sim_normals(int nf, int p, int site0, int n_sites, uint32_t k0, uint32_t k1,
                                                   double* __restrict__ z, int64_t ss, int64_t fs, int sm) {
#pragma clang fp contract(off)
  const int npair = (p + 1) / 2;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, per = (int64_t)nf * npair;
  if (gid >= per * n_sites) return;
  const int s = (int)(sm ? gid % n_sites : gid / per);
  const int64_t rest = sm ? gid / n_sites : gid % per;
  const int f = (int)(rest / npair), q = (int)(rest - (int64_t)f * npair);
  uint32_t r[4];
  philox4x32_10((uint32_t)f, (uint32_t)q, (uint32_t)(site0 + s), 0u, k0, k1, r);
  const double u1 = sim_uniform(r[0], r[1]), u2 = sim_uniform(r[2], r[3]);
  const double rad = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincos(6.283185307179586 * u2, &sn, &cs);
  double* __restrict__ o = z + (int64_t)s * ss + ((int64_t)f * p + 2 * q) * fs;
  o[0] = rad * cs;
  if (2 * q + 1 < p) o[fs] = rad * sn;
}

// One topology level.  SM == false: thread = (family of the level, trait), the sites along blockIdx.y; SM (p = 1): thread =
// site, the families of the level along blockIdx.y.  z, x of this chunk at s * ss + (f * p + t) * fs; entry j of the record of
// (set, family f) at set * pss + (f * rec + j) * pfs.
template <bool SM>
__global__ __launch_bounds__(256) void sim_apply(LgStatic F, const int32_t* __restrict__ pf, const int32_t* __restrict__ lfam,
                                                 int n_lf, int site0, int n_sites, int per_set,
                                                 const double* __restrict__ fpool, int64_t pss, int64_t pfs,
                                                 const int32_t* __restrict__ info, const double* __restrict__ z, double* x,
                                                 int64_t ss, int64_t fs, int write_data, double* __restrict__ data,
                                                 double* __restrict__ data_sm, int64_t sm_stride) {
#pragma clang fp contract(off)
  const int p = F.p, K = F.K;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (SM ? (int64_t)n_sites : (int64_t)n_lf * p)) return;
  const int64_t rec = sim_rec(p, K);
  const int n_outer = SM ? n_lf : n_sites;
  for (int o = blockIdx.y; o < n_outer; o += gridDim.y) {
    const int s = SM ? (int)gid : o;
    const int t = SM ? 0 : (int)(gid % p);
    const int f = lfam[SM ? o : (int)(gid / p)];
    const int set = per_set ? s : 0;
    double* xo = x + (int64_t)s * ss + ((int64_t)f * p + t) * fs;
    if (info[set] != 0) {
      *xo = NAN;
      continue;
    }
    // entry j of the family's record at r[j * pfs]: L's row t, then qc, then off
    const double* __restrict__ r = fpool + (int64_t)set * pss + (int64_t)f * rec * pfs;
    const double* __restrict__ Lr = r + (int64_t)(t * (t + 1) / 2) * pfs;
    const double* __restrict__ qc = r + (int64_t)(p * (p + 1) / 2) * pfs;
    const int np = F.n_parents[f];
    double m = 0.0;
    for (int k = 0; k < np; ++k) {
      const int pk = pf[(size_t)f * K + k];
      if (pk >= 0) m = m + qc[k * pfs] * x[(int64_t)s * ss + ((int64_t)pk * p + t) * fs];
    }
    m = m + qc[(K + t) * pfs];
    const double* __restrict__ zf = z + (int64_t)s * ss + (int64_t)f * p * fs;
    double nz = 0.0;
    for (int j = 0; j <= t; ++j) nz = nz + Lr[j * pfs] * zf[j * fs];
    const double v = m + nz;
    *xo = v;
    if (write_data && sim_is_tip(F, f) && (!F.child_mask || ((F.child_mask[f] >> t) & 1ull))) {
      const int64_t as = (int64_t)site0 + s;
      data[(as * F.n_rows + F.data_row[f]) * p + t] = v;
      if (data_sm) data_sm[(int64_t)F.data_row[f] * sm_stride + as] = v;
    }
  }
}

// bounds of the call's scratch, in doubles: the factor records of a chunk of sites, the states (and the normals) of a chunk
static std::atomic<int64_t> g_sim_factor_limit{(int64_t)32 << 20}, g_sim_state_limit{(int64_t)128 << 20};

}  // namespace pgbp

using namespace pgbp;

// ms (pgbp_lg_simulate_timed): the stream is drained after every phase and the wall time of the phase is added to
// ms[0 .. 3] = {factor, normals (generated or copied up), apply, copies down}
static int lg_simulate(pgbp_engine* e, int32_t site_begin, int32_t site_end, const double* z, uint64_t seed, double* x,
                       double* z_out, int32_t write_data, int32_t* info, double* ms) {
  if (!e) return PGBP_ERR_INVALID;
  const std::string fn = "pgbp_lg_simulate: ";
  const EngineView v = engine_peek(e);
  (void)hipSetDevice(engine_device(e));
  const LgModel* L = engine_lg(e);
  if (!L) return engine_fail(e, PGBP_ERR_STATE, fn + "no family table (call pgbp_lg_setup first)");
  if (!L->d_pf) return engine_fail(e, PGBP_ERR_STATE, fn + "no topology (call pgbp_lg_set_topology first)");
  if (!L->have_params) return engine_fail(e, PGBP_ERR_STATE, fn + "no parameters yet (call pgbp_lg_assignfactors first)");
  if (const int orc = lg_refuse_optima(e, "pgbp_lg_simulate", L)) return orc;
  const LgStatic& F = L->F;
  const LgParams& M = L->M;
  const LgShifts& Sh = L->Sh;
  const LgNoise& Nz = L->Nz;
  // the node topology (parents by family on the device, the families grouped by level) and the tip data as the one writer
  // besides the set-up sees them (data_sm: null unless the table keeps the [row][site] copy)
  const int32_t *parent_family = L->d_pf.get(), *level_fam = L->d_level_fam.get();
  double *data = L->bufs.data.get(), *data_sm = L->bufs.data_sm.get();
  const int p = F.p, K = F.K, nf = L->T.n_families;
  if (L->improper >= 0)
    return engine_fail(e, PGBP_ERR_INVALID, fn + "family " + std::to_string(L->improper / K) + ", parent " + std::to_string(L->improper % K) +
                                                " is a root without a proper prior: the model has no joint distribution to draw from");
  if (site_begin < 0 || site_end < site_begin || site_end > v.plan->n_sites)
    return engine_fail(e, PGBP_ERR_INVALID, fn + "site range [" + std::to_string(site_begin) + ", " + std::to_string(site_end) +
                                                ") outside the engine's " + std::to_string(v.plan->n_sites) + " sites");
  if (!x && !z_out && !write_data)
    return engine_fail(e, PGBP_ERR_INVALID, fn + "nothing to do (x and z_out are NULL and write_data is 0)");
  if (p > 64) return engine_fail(e, PGBP_ERR_INVALID, fn + std::to_string(p) + " traits, more than the 64 the sweep takes");
  const int ns = site_end - site_begin;
  if (ns == 0 || nf == 0) {
    if (info) std::fill(info, info + ns, 0);
    return PGBP_OK;
  }
  const int per_set = (M.per_site || (Sh.slot && Sh.per_site) || (Nz.slot && Nz.per_site)) ? 1 : 0;
  const bool sm = p == 1 && data_sm != nullptr;
  const int64_t rec = sim_rec(p, K), f_stride = (int64_t)nf * rec, size = (int64_t)nf * p;
  int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(ns, g_sim_state_limit.load() / size));
  if (per_set) chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, g_sim_factor_limit.load() / f_stride));
  const int64_t row = sm ? sm_row(chunk) : chunk;              // the states of a chunk: [family][row] or [chunk][family][trait]
  const int n_sets_max = per_set ? (int)chunk : 1;
  const bool pool_sm = sm && per_set;                          // the factor records of a site-minor batch: [family][entry][set]
  const bool stage = sm && (z || x || z_out);                  // the host's [site][family] order on the device
  DevBuf<double> d_f, d_x, d_z, d_stage;
  DevBuf<int32_t> d_stat, d_info;
  hipError_t herr = (hipError_t)d_f.alloc((size_t)(pool_sm ? sm_row(n_sets_max) : n_sets_max) * f_stride);
  if (herr == hipSuccess) herr = (hipError_t)d_stat.alloc((size_t)n_sets_max * nf);
  if (herr == hipSuccess) herr = (hipError_t)d_info.alloc((size_t)n_sets_max);
  if (herr == hipSuccess) herr = (hipError_t)d_x.alloc((size_t)row * size);
  if (herr == hipSuccess) herr = (hipError_t)d_z.alloc((size_t)row * size);
  if (herr == hipSuccess && stage) herr = (hipError_t)d_stage.alloc((size_t)chunk * size);
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, fn + "(scratch) " + hipGetErrorString(herr));
  std::vector<int32_t> h_info((size_t)(per_set ? ns : 1), 0);
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
  (void)hipGetLastError();   // (an error an earlier asynchronous call left behind is that call's to report)
  phase(-1);
  const std::vector<int32_t>& lo = L->level_off;
  const size_t lds = sizeof(double) * (size_t)sim_region(p, K) * (p <= 16 ? 4 : 1);   // (p = 1: sim_factor_uni uses none)
  const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
  for (int64_t s0 = 0; herr == hipSuccess && s0 < ns; s0 += chunk) {
    const int n = (int)std::min<int64_t>(chunk, ns - s0), site0 = site_begin + (int)s0;
    const int n_sets = per_set ? n : 1, gy = std::min(n_sets, 65535);
    // (a short last chunk of a site-minor batch has rows of its own length)
    const int64_t ss = sm ? 1 : size, fs = sm ? sm_row(n) : 1;
    const int64_t pss = pool_sm ? 1 : f_stride, pfs = pool_sm ? sm_row(n_sets) : 1;
    if (per_set || s0 == 0) {
      if (p == 1) {
        herr = hipMemsetAsync(d_stat.get(), 0, sizeof(int32_t) * (size_t)n_sets * nf, v.st);
        if (pool_sm)
          hipLaunchKernelGGL(sim_factor_uni<true>, dim3((n_sets + 255) / 256, std::min(nf, 65535)), dim3(256), 0, v.st, F, M, Sh, Nz,
                             parent_family, nf, site0, n_sets, per_set, d_f.get(), pss, pfs, d_stat.get());
        else
          hipLaunchKernelGGL(sim_factor_uni<false>, dim3((nf + 255) / 256, gy), dim3(256), 0, v.st, F, M, Sh, Nz, parent_family, nf,
                             site0, n_sets, per_set, d_f.get(), pss, pfs, d_stat.get());
      } else if (p <= 16)
        hipLaunchKernelGGL(sim_factor<16>, dim3((nf + 3) / 4, gy), dim3(kWave), lds, v.st, F, M, Sh, Nz, parent_family, nf, site0,
                           n_sets, per_set, d_f.get(), f_stride, d_stat.get());
      else
        hipLaunchKernelGGL(sim_factor<64>, dim3(nf, gy), dim3(kWave), lds, v.st, F, M, Sh, Nz, parent_family, nf, site0, n_sets,
                           per_set, d_f.get(), f_stride, d_stat.get());
      hipLaunchKernelGGL(sim_info, dim3(gy), dim3(256), 0, v.st, d_stat.get(), nf, n_sets, d_info.get());
      if (herr == hipSuccess) herr = hipGetLastError();
      if (herr == hipSuccess)
        herr = hipMemcpyAsync(h_info.data() + (per_set ? s0 : 0), d_info.get(), sizeof(int32_t) * (size_t)n_sets, hipMemcpyDeviceToHost, v.st);
    }
    phase(0);
    const size_t bytes = sizeof(double) * (size_t)n * size;
    if (herr == hipSuccess && z) {
      herr = hipMemcpyAsync(stage ? d_stage.get() : d_z.get(), z + (size_t)s0 * size, bytes, hipMemcpyHostToDevice, v.st);
      if (herr == hipSuccess && sm) launch_transpose_words_f64(d_stage.get(), d_z.get(), nf, n, 1, v.st);
    } else if (herr == hipSuccess) {
      const int64_t threads = (int64_t)n * nf * ((p + 1) / 2);
      hipLaunchKernelGGL(sim_normals, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, v.st, nf, p, site0, n, k0, k1,
                         d_z.get(), ss, fs, sm ? 1 : 0);
    }
    phase(1);
    for (size_t l = 0; herr == hipSuccess && l + 1 < lo.size(); ++l) {
      const int n_lf = lo[l + 1] - lo[l];
      if (n_lf == 0) continue;
      if (sm)
        hipLaunchKernelGGL(sim_apply<true>, dim3((n + 255) / 256, std::min(n_lf, 65535)), dim3(256), 0, v.st, F, parent_family,
                           level_fam + lo[l], n_lf, site0, n, per_set, d_f.get(), pss, pfs, d_info.get(), d_z.get(), d_x.get(), ss,
                           fs, write_data, data, data_sm, sm_row(v.plan->n_sites));
      else
        hipLaunchKernelGGL(sim_apply<false>, dim3((unsigned)(((int64_t)n_lf * p + 255) / 256), std::min(n, 65535)), dim3(256), 0, v.st,
                           F, parent_family, level_fam + lo[l], n_lf, site0, n, per_set, d_f.get(), pss, pfs, d_info.get(),
                           d_z.get(), d_x.get(), ss, fs, write_data, data, data_sm, sm_row(v.plan->n_sites));
    }
    if (herr == hipSuccess) herr = hipGetLastError();
    phase(2);
    for (int which = 0; which < 2 && herr == hipSuccess; ++which) {
      double* host = which == 0 ? x : z_out;
      const double* dev = which == 0 ? d_x.get() : d_z.get();
      if (!host) continue;
      if (sm) {
        launch_transpose_words_f64(dev, d_stage.get(), nf, n, 0, v.st);
        dev = d_stage.get();
      }
      herr = hipMemcpyAsync(host + (size_t)s0 * size, dev, bytes, hipMemcpyDeviceToHost, v.st);
    }
    phase(3);
  }
  const hipError_t serr = hipStreamSynchronize(v.st);   // (also when something failed: the copies use this call's locals)
  if (herr == hipSuccess) herr = serr;
  if (herr != hipSuccess) return engine_fail(e, PGBP_ERR_HIP, fn + hipGetErrorString(herr));
  if (info)
    for (int s = 0; s < ns; ++s) info[s] = h_info[per_set ? s : 0];
  return PGBP_OK;
}

extern "C" int pgbp_lg_simulate(pgbp_engine* e, int32_t site_begin, int32_t site_end, const double* z, uint64_t seed, double* x,
                                double* z_out, int32_t write_data, int32_t* info) {
  return lg_simulate(e, site_begin, site_end, z, seed, x, z_out, write_data, info, nullptr);
}

extern "C" int pgbp_lg_simulate_timed(pgbp_engine* e, int32_t site_begin, int32_t site_end, const double* z, uint64_t seed,
                                      double* x, double* z_out, int32_t write_data, int32_t* info, double* ms4) {
  if (e && !ms4) return engine_fail(e, PGBP_ERR_INVALID, "pgbp_lg_simulate_timed: no buffer for the phase times");
  return lg_simulate(e, site_begin, site_end, z, seed, x, z_out, write_data, info, ms4);
}

extern "C" void pgbp_simulate_scratch_limits(int64_t factor_doubles, int64_t state_doubles) {
  g_sim_factor_limit.store(factor_doubles > 0 ? factor_doubles : (int64_t)32 << 20);
  g_sim_state_limit.store(state_doubles > 0 ? state_doubles : (int64_t)128 << 20);
}

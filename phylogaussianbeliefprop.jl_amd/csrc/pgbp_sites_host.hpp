// Host side of the lanes-are-sites calls of a univariate batch (pgbp_grad_uni.hip, pgbp_fam_uni.hip, pgbp_post_uni.hip,
// pgbp_cov_uni.hip, pgbp_exact_uni.hip), written once: what a call checks before it is accepted, the chunk of sites whose rows fit the scratch, the
// kernel arguments of a chunk, the scratch of a call with its one sticky error, the launch of a kernel in the layout the pool is
// in, and the clock of the timed variants.  Plain helpers: every entry point still reads top to bottom in its own file --
// accept, sizes, scratch, the chunk loop with its launches, copies, finish.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>

#include "pgbp_devmem.hpp"
#include "pgbp_fam_uni_dev.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"

namespace pgbp {

// bound of a call's scratch, in doubles: the rows of a chunk of sites (pgbp_sites_sweep_scratch_limit; pgbp_fam_uni.hip)
extern std::atomic<int64_t> g_fam_uni_limit;

// what a call holds once it is accepted
struct SitesCall {
  const LgModel* L;
  EngineView v;
  UniView U;
  int ns;
};

// The two halves of the checks, in the order and wording of pgbp_lg_gradient_sites.  First the state and the range
// (lg_sweep_state), which fills c (the layout is not touched) ...
inline int sites_accept_state(pgbp_engine* e, const char* fn, int32_t site_begin, int32_t site_end, SitesCall* c) {
  const int rc = lg_sweep_state(e, fn, site_begin, site_end, &c->L);
  if (rc) return rc;
  c->v = engine_peek(e);
  c->U = engine_uni_view(e);
  c->ns = site_end - site_begin;
  return PGBP_OK;
}

// ... then the thread-per-site engine as the plan defines it; `general`: the call to use instead.
inline int sites_accept_engine(pgbp_engine* e, const char* fn, const char* general, const SitesCall& c) {
  const Plan& pl = *c.v.plan;
  const std::string use = std::string(" (use ") + general + ")";
  if (c.L->F.p != 1)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": " + std::to_string(c.L->F.p) + " traits; the thread-per-site sweep is univariate" + use);
  if (pl.max_dim > 2)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": a belief of " + std::to_string(pl.max_dim) +
                                                " variables; the thread-per-site sweep needs every belief at 2 variables or fewer" + use);
  if (pl.n_sites < 8)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": " + std::to_string(pl.n_sites) +
                                                " sites; the thread-per-site kernels run from 8 sites on" + use);
  if (!c.U.tps || c.U.bs16)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": the engine is not on the thread-per-site kernels" + use);
  return PGBP_OK;
}

// Both, with the test of a call's own pointers between them: `missing` is null when the outputs are fine.
inline int sites_accept(pgbp_engine* e, const char* fn, const char* general, int32_t site_begin, int32_t site_end,
                        const char* missing, SitesCall* c) {
  const int rc = sites_accept_state(e, fn, site_begin, site_end, c);
  if (rc) return rc;
  if (missing) return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": " + missing);
  return sites_accept_engine(e, fn, general, *c);
}

// What the closed forms of a Brownian motion with R = 1 (pgbp_bm_exact_stats_sites, pgbp_bm_rate_matrix_sites) check of the
// model and of the family table once the call is accepted: no Ornstein-Uhlenbeck fill, no tip noise, and the checks of the
// general call that can fail at p = 1 (src/calibration.jl:416-421 and the sweep's own).  PGBP_OK, or engine_fail's code.
inline int sites_bm_closed_form_checks(pgbp_engine* e, const char* fn, const LgModel* L) {
  if (L->M.model == PGBP_LG_OU)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": the last pgbp_lg_assignfactors was an Ornstein-Uhlenbeck fill; the "
                                                "closed form is that of a Brownian motion with R = 1 (use fit_sites_lg)");
  if (L->Nz.slot)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": tip noise is in force (pgbp_lg_set_tip_noise): the variance is then "
                                                "not proportional to the rate and the fit has no closed form (use fit_sites_lg)");
  const LgTable& T = L->T;
  const int nf = T.n_families, K = L->F.K;
  for (int f = 0; f < nf; ++f) {
    const std::string where = std::string(fn) + ": family " + std::to_string(f) + " (cluster " + std::to_string(T.cluster[f]) + "): ";
    const unsigned long long cm = T.child_mask.empty() ? 1ull : T.child_mask[f];
    bool pm0 = true;
    for (int k = 0; k < T.n_parents[f]; ++k) {
      const unsigned long long pm = T.parent_mask.empty() ? 1ull : T.parent_mask[(size_t)f * K + k];
      if (k == 0) pm0 = pm != 0;
      if (T.parent_pos[(size_t)f * K + k] < 0 && pm != 0)   // (-1 with an empty mask: a parent with nothing in scope)
        return engine_fail(e, PGBP_ERR_INVALID, where + "its parent is the fixed root: the sweep is defined on the engine with "
                                                        "an improper root prior (fixedroot = false)");
    }
    if (T.n_parents[f] > 1 && T.child_pos[f] < 0 && cm != 0 && pm0)
      return engine_fail(e, PGBP_ERR_INVALID, where + "a leaf with more than one parent");
  }
  return PGBP_OK;
}

// the root (belief, position) a call forms mu from, when it is asked for
inline int sites_root_check(pgbp_engine* e, const char* fn, const Plan& pl, int32_t root_belief, int32_t root_pos) {
  if (root_belief < 0 || root_belief >= pl.n_beliefs())
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": root belief " + std::to_string(root_belief) + " out of range");
  if (root_pos < 0 || root_pos >= pl.dims[root_belief])
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": root position " + std::to_string(root_pos) + " out of range: belief " +
                                                std::to_string(root_belief) + " has " + std::to_string(pl.dims[root_belief]) + " variables");
  return PGBP_OK;
}

// sites per chunk when a site takes per_site doubles of scratch: whole workgroups, one workgroup's sites at least
inline int fam_uni_chunk(int ns, int64_t per_site) {
  const int64_t fit = (g_fam_uni_limit.load() / std::max<int64_t>(1, per_site)) / 256 * 256;
  return (int)std::min<int64_t>(ns, std::max<int64_t>(256, fit));
}

// the kernel arguments of the n sites from site0 on, in scratch rows of `chunk` sites; d_fcl: the family sweeps' table
inline SitesArgs sites_args(const SitesCall& c, int site0, int n, int chunk, const int32_t* d_fcl = nullptr) {
  return SitesArgs{c.U.pool, c.U.stride, c.U.off, c.U.bdim, site0, n, (int64_t)chunk, d_fcl, sm_row(c.v.plan->n_sites)};
}

// The scratch of one call and its one error.  Nothing runs after the first error; the stream is drained before every error
// return (the uploads read the call's locals); a failure of the setup is reported as "fn (scratch): ...", a later one as
// "fn: ..."; the final synchronisation always happens and the first error wins.
struct SitesScratch {
  pgbp_engine* e;
  const char* fn;
  hipStream_t st;
  hipError_t err = hipSuccess;   // (an entry point with a step of its own sets it where ok())

  SitesScratch(pgbp_engine* e_, const char* fn_, hipStream_t st_) : e(e_), fn(fn_), st(st_) {}
  bool ok() const { return err == hipSuccess; }

  // n elements for b, when the call wants it
  template <class T>
  void alloc(DevBuf<T>& b, size_t n, bool wanted = true) {
    if (ok() && wanted) err = (hipError_t)b.alloc(n);
  }
  // n elements of a host array into b
  template <class T>
  void upload(const DevBuf<T>& b, const T* src, size_t n) {
    if (ok() && n) err = hipMemcpyAsync(b.get(), src, sizeof(T) * n, hipMemcpyHostToDevice, st);
  }
  // the end of the setup: 0, or the call's return value
  int ready() {
    if (!ok()) {
      (void)hipStreamSynchronize(st);
      return engine_fail(e, PGBP_ERR_HIP, std::string(fn) + " (scratch): " + hipGetErrorString(err));
    }
    (void)hipGetLastError();   // (an error an earlier asynchronous call left behind is that call's to report)
    return PGBP_OK;
  }
  // a kernel of 256 threads per workgroup on the call's stream
  template <class... P, class... A>
  void launch(void (*kernel)(P...), dim3 grid, A... a) {
    if (ok()) hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, a...);
  }
  // after a chunk's launches
  void check() {
    if (ok()) err = hipGetLastError();
  }
  // `rows` rows of n sites of the scratch (row length chunk) into the caller's rows of ns sites, from site s0 on (dst may be null)
  template <class T>
  void rows(T* dst, int ns, int s0, const T* src, int chunk, int n, int64_t rows) {
    if (ok() && dst && rows)
      err = hipMemcpy2DAsync(dst + s0, sizeof(T) * (size_t)ns, src, sizeof(T) * (size_t)chunk, sizeof(T) * (size_t)n, (size_t)rows,
                             hipMemcpyDeviceToHost, st);
  }
  // n elements to the host (dst may be null)
  template <class T>
  void download(T* dst, const T* src, size_t n) {
    if (ok() && dst) err = hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost, st);
  }
  // the one synchronisation of the call, and its return value
  int finish() {
    const hipError_t serr = hipStreamSynchronize(st);
    if (ok()) err = serr;
    if (!ok()) return engine_fail(e, PGBP_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(err));
    return PGBP_OK;
  }
};

// kernel<SM> in the layout the pool is in (sm: UniView::sm), the kernel named and its arguments written once
#define PGBP_SITES_LAUNCH(S, sm, kernel, grid, ...)     \
  do {                                                  \
    if (sm) (S).launch(kernel<true>, grid, __VA_ARGS__); \
    else (S).launch(kernel<false>, grid, __VA_ARGS__);   \
  } while (0)

// The clock of a timed variant (ms null: the plain call, nothing happens): the stream is drained after every phase and the wall
// time since the last one is added to ms[k]; k < 0 starts the clock.
struct SitesClock {
  SitesScratch& S;
  double* ms;
  std::chrono::steady_clock::time_point t_last;

  SitesClock(SitesScratch& S_, double* ms_, int n) : S(S_), ms(ms_), t_last(std::chrono::steady_clock::now()) {
    if (ms) std::fill(ms, ms + n, 0.0);
    (*this)(-1);
  }
  void operator()(int k) {
    if (!ms) return;
    const hipError_t perr = hipStreamSynchronize(S.st);
    if (S.ok()) S.err = perr;
    const auto now = std::chrono::steady_clock::now();
    if (k >= 0) ms[k] += std::chrono::duration<double, std::milli>(now - t_last).count();
    t_last = now;
  }
};

}  // namespace pgbp

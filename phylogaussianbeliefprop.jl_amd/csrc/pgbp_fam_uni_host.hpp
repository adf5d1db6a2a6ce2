// Host side of the lanes-are-sites sweeps of a univariate batch (pgbp_fam_uni.hip, pgbp_post_uni.hip), written once: what a
// call checks before it is accepted, the chunk of sites whose rows fit the scratch, and the strided copy of a chunk's rows
// into the caller's site-minor rows.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <string>

#include "pgbp_kernels.hpp"
#include "pgbp_lgmodel.hpp"

namespace pgbp {

// bound of a call's scratch, in doubles: the rows of a chunk of sites (pgbp_sites_sweep_scratch_limit; pgbp_fam_uni.hip)
extern std::atomic<int64_t> g_fam_uni_limit;

// what a call holds once it is accepted
struct FamUniCall {
  const LgModel* L;
  EngineView v;
  UniView U;
  int ns;
};

// The checks of pgbp_lg_gradient_sites, in its order and wording: state and range (lg_sweep_state), `missing` (null: the
// outputs are fine), then the thread-per-site engine as the plan defines it; `general`: the call to use instead.
inline int fam_uni_accept(pgbp_engine* e, const char* fn, const char* general, int32_t site_begin, int32_t site_end,
                          const char* missing, FamUniCall* c) {
  const int rc = lg_sweep_state(e, fn, site_begin, site_end, &c->L);
  if (rc) return rc;
  if (missing) return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": " + missing);
  c->v = engine_peek(e);   // (the layout is not touched)
  const Plan& pl = *c->v.plan;
  c->U = engine_uni_view(e);
  const std::string use = std::string(" (use ") + general + ")";
  if (c->L->F.p != 1)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": " + std::to_string(c->L->F.p) + " traits; the thread-per-site sweep is univariate" + use);
  if (pl.max_dim > 2)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": a belief of " + std::to_string(pl.max_dim) +
                                                " variables; the thread-per-site sweep needs every belief at 2 variables or fewer" + use);
  if (pl.n_sites < 8)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": " + std::to_string(pl.n_sites) +
                                                " sites; the thread-per-site kernels run from 8 sites on" + use);
  if (!c->U.tps || c->U.bs16)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": the engine is not on the thread-per-site kernels" + use);
  c->ns = site_end - site_begin;
  return PGBP_OK;
}

// sites per chunk when a site takes per_site doubles of scratch: whole workgroups, one workgroup's sites at least
inline int fam_uni_chunk(int ns, int64_t per_site) {
  const int64_t fit = (g_fam_uni_limit.load() / std::max<int64_t>(1, per_site)) / 256 * 256;
  return (int)std::min<int64_t>(ns, std::max<int64_t>(256, fit));
}

// `rows` rows of n sites of the scratch (row length chunk) into the caller's rows of ns sites, from site s0 on
template <class T>
inline hipError_t fam_uni_copy(T* dst, int ns, int s0, const T* src, int chunk, int n, int64_t rows, hipStream_t st) {
  if (!dst || rows == 0) return hipSuccess;
  return hipMemcpy2DAsync(dst + s0, sizeof(T) * (size_t)ns, src, sizeof(T) * (size_t)chunk, sizeof(T) * (size_t)n, (size_t)rows,
                          hipMemcpyDeviceToHost, st);
}

}  // namespace pgbp

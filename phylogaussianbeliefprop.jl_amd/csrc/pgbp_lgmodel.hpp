// The one owner of everything behind a family table: the table on the host, the device buffers, the
// kernel-argument structs that borrow from them, and what the setters added.  pgbp_lg_setup builds a whole one and the
// engine takes it; an engine without a table holds none.
#pragma once
#include <memory>
#include <vector>

#include "pgbp_devmem.hpp"
#include "pgbp_kernels.hpp"
#include "pgbp_lgtable.hpp"
#include "pgbp_cladeshift_host.hpp"
#include "pgbp_optscan_host.hpp"
#include "pgbp_sitemiss_host.hpp"

namespace pgbp {

// what LgStatic points at: the family table of pgbp_lg_setup and the parameter slots pgbp_lg_assignfactors fills
struct LgBufs {
  DevBuf<int32_t> off, fam, np, cp, row, pp, col;
  DevBuf<double> len, gam, data, data_sm;
  DevBuf<unsigned long long> cm, pm;
  DevBuf<LgSimpleFam> simple;
  DevBuf<double> R, alpha, theta, mu;
};
// what LgShifts points at (pgbp_lg_set_shifts), and the clusters the correction kernel visits
struct LgShiftBufs {
  DevBuf<int32_t> slot, cl;
  DevBuf<double> value, value_sm;
};
// what LgOptima points at (pgbp_lg_set_optima)
struct LgOptimaBufs {
  DevBuf<int32_t> regime;
  DevBuf<double> value, value_sm;
};
// what LgNoise points at (pgbp_lg_set_tip_noise), and the clusters the correction kernel visits
struct LgNoiseBufs {
  DevBuf<int32_t> slot, cl;
  DevBuf<double> scale, sigma_e, se2, se2_sm;
};

// what LgSiteMiss points at (pgbp_lg_set_site_missing), and the clusters the correction kernel visits
struct LgSiteMissBufs {
  DevBuf<unsigned long long> words;
  DevBuf<int32_t> cl;
};

// what LgCladeShifts points at (pgbp_lg_set_clade_shifts_sites), and the clusters the correction kernel visits
struct LgCladeBufs {
  DevBuf<int32_t> family, cl;
  DevBuf<double> delta;
};

struct LgModel {
  LgTable T;
  LgBufs bufs;
  LgStatic F{};             // device pointers into bufs
  LgParams M{};             // the last pgbp_lg_assignfactors (have_params), into bufs
  bool have_params = false;
  // pgbp_lg_set_shifts: Sh.slot == null: none; the number of clusters that hold a shifted family (shift_bufs.cl)
  LgShiftBufs shift_bufs;
  LgShifts Sh{};
  int32_t n_shift_cl = 0;
  // pgbp_lg_set_optima: Op.regime == null: none.  The clusters that hold a shifted (shift_cl) and a painted (opt_cl) family on
  // the host, and their union on the device (disp_cl, n_disp_cl): what the displacement correction visits while optima are set
  LgOptimaBufs opt_bufs;
  LgOptima Op{};
  std::vector<int32_t> shift_cl, opt_cl;
  DevBuf<int32_t> disp_cl;
  int32_t n_disp_cl = 0;
  // the optima as the kernels take them: none under BM, where wc = 0 and they have no effect
  LgOptima optima_in_force() const { return (Op.regime && M.model == PGBP_LG_OU) ? Op : LgOptima{}; }
  // pgbp_lg_set_tip_noise: Nz.slot == null: none; the clusters that hold a noisy tip family and the largest of them
  LgNoiseBufs noise_bufs;
  LgNoise Nz{};
  int32_t n_noise_cl = 0, noise_max_dim = 0;
  // pgbp_lg_set_site_missing: Ms.words == null: none; the mask on the host (words, the masked tip families, their clusters)
  LgSiteMissBufs miss_bufs;
  LgSiteMiss Ms{};
  SiteMissPack miss;
  // pgbp_lg_set_topology (d_pf null: none): parents by family [n_families * K] and the families grouped by level
  // (pgbp_topology.hpp); improper: the first entry f * K + k that is an improper root, -1: none
  DevBuf<int32_t> d_pf, d_level_fam;
  std::vector<int32_t> level_off;
  int32_t improper = -1;
  // the plan of pgbp_lg_optimum_scan_sites, built with the topology (pgbp_optscan_host.hpp; built == false: no topology): the
  // child lists and the families by height, on the host and on the device
  OptScanPlan optscan;
  DevBuf<int32_t> d_os_child_off, d_os_child_fam, d_os_height_fam;
  // the preorder ranks of the family tree, built and uploaded with the topology (pgbp_cladeshift_host.hpp), and
  // pgbp_lg_set_clade_shifts_sites: Cs.family == null: none; the setting on the host as [slot][site] (clade_family, clade_delta)
  // and the number of clusters that hold a family inside some site's clade (clade_bufs.cl)
  CladePlan clade;
  DevBuf<int32_t> d_clade_pre, d_clade_last;
  LgCladeBufs clade_bufs;
  LgCladeShifts Cs{};
  std::vector<int32_t> clade_family;
  std::vector<double> clade_delta;
  int32_t n_clade_cl = 0;
  // the clade shifts as the kernels take them: none under BM, where wc = 0 and they have no effect
  LgCladeShifts clade_in_force() const { return (Cs.family && M.model == PGBP_LG_OU) ? Cs : LgCladeShifts{}; }
};

// the model of the engine's family table, null when there is none (defined in pgbp_engine.hip)
const LgModel* engine_lg(const pgbp_engine* e);

// What a sweep `fn` checks of the engine's state before anything else, in this order: a table, parameters, the site range.
// PGBP_OK with *out, or engine_fail's code.  sites_call: for a general sweep, whose kernels cannot honour a per-site mask, the
// lanes-are-sites call to use while one is in force (pgbp_lg_set_site_missing); null: the call reads the mask itself.
inline int lg_sweep_state(pgbp_engine* e, const char* fn, int32_t site_begin, int32_t site_end, const LgModel** out,
                          const char* sites_call = nullptr) {
  const LgModel* L = engine_lg(e);
  if (!L) return engine_fail(e, PGBP_ERR_STATE, std::string(fn) + ": no family table (call pgbp_lg_setup first)");
  if (sites_call && L->Ms.words)
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": a per-site mask of missing tips is in force (pgbp_lg_set_site_missing), "
                                                "which this sweep cannot honour (use " + sites_call + ")");
  if (!L->have_params)
    return engine_fail(e, PGBP_ERR_STATE, std::string(fn) + ": no parameters yet (call pgbp_lg_assignfactors first)");
  if (site_begin < 0 || site_end < site_begin || site_end > engine_n_sites(e))
    return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": site range outside the engine's sites");
  *out = L;
  return PGBP_OK;
}

// A sweep `fn` that forms the families' offsets itself and does not know painted optima (pgbp_lg_set_optima): refused while
// they are in force under OU, before any launch; PGBP_OK otherwise (under BM the optima have no effect).
// The same for a sweep that does not know the per-site clade shifts of the optimum (pgbp_lg_set_clade_shifts_sites)
inline int lg_refuse_clade_shifts(pgbp_engine* e, const char* fn, const LgModel* L) {
  if (!L || !L->clade_in_force().family) return PGBP_OK;
  return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": per-site clade shifts of the optimum are in force (pgbp_lg_set_clade_shifts_sites: " +
                                              std::to_string(L->Cs.n_slots) + " slots), which this sweep does not honour; it would "
                                              "return the answer without them");
}
inline int lg_refuse_optima(pgbp_engine* e, const char* fn, const LgModel* L) {
  if (const int rc = lg_refuse_clade_shifts(e, fn, L)) return rc;
  if (!L || !L->optima_in_force().regime) return PGBP_OK;
  return engine_fail(e, PGBP_ERR_INVALID, std::string(fn) + ": painted optima are in force (pgbp_lg_set_optima: " + std::to_string(L->Op.n) +
                                              " regimes), which this sweep does not honour yet; it would return the unpainted answer");
}

// The families pgbp_lg_impute_count / _families / _sites list: the statically missing tips of the table (impute_list) and, with
// a per-site mask in force, every tip masked at some site, merged in family order.  dyn[i] != 0: family i of the list is
// observed wherever the mask does not say otherwise (its predicted mask is then 1: p = 1, every parent in scope).
inline void lg_impute_list(const LgModel& L, std::vector<int32_t>& fams, std::vector<unsigned long long>& pred,
                           std::vector<int32_t>* dyn = nullptr) {
  std::vector<int32_t> f0;
  std::vector<unsigned long long> p0;
  L.T.impute_list(f0, p0);
  fams.clear();
  pred.clear();
  if (dyn) dyn->clear();
  const std::vector<int32_t>& f1 = L.Ms.words ? L.miss.fams : std::vector<int32_t>();
  size_t a = 0, b = 0;
  while (a < f0.size() || b < f1.size()) {
    const bool take0 = b >= f1.size() || (a < f0.size() && f0[a] <= f1[b]);
    if (take0 && b < f1.size() && f0[a] == f1[b]) ++b;   // (the setter refuses a statically missing tip: not reached)
    fams.push_back(take0 ? f0[a] : f1[b]);
    pred.push_back(take0 ? p0[a] : 1ull);
    if (dyn) dyn->push_back(take0 ? 0 : 1);
    if (take0) ++a; else ++b;
  }
}

}  // namespace pgbp

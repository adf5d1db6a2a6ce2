// The family table of pgbp_lg_setup (pgbp_lg_families of include/pgbp.h) on the host, validated, once: every check of the
// table and of what the setters are given against it, and every list the sweeps derive from it.
// Plain C++ without the runtime, so that a stand-alone program can run it under a host sanitizer (tests/lgtable_check.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pgbp.h"
#include "pgbp_sitemiss_host.hpp"

namespace pgbp {

// the one family of a cluster as the thread-per-site fill reads it (LgStatic::simple)
struct LgSimpleFam {
  int32_t np, cpos, ppos, row, color, pad;   // parents (0: a root prior), positions of child / parent in the cluster (-1: fixed), data row, rate
  double length, gamma;
  double pad2[2];
};
static_assert(sizeof(LgSimpleFam) == 56 || sizeof(LgSimpleFam) == 64, "LgSimpleFam");

struct LgTable {
  int32_t p = 0, K = 1, n_rates = 0, n_rows = 0, n_families = 0;
  int32_t n_sites = 1;         // of the engine
  std::vector<int32_t> dims;   // [n_clusters] of the plan
  std::vector<int32_t> cluster, n_parents, child_pos, data_row;   // [n_families]
  std::vector<int32_t> parent_pos, color;                         // [n_families * K]
  std::vector<double> length, gamma;                              // [n_families * K]
  std::vector<unsigned long long> child_mask, parent_mask;        // and-ed with full_mask(); empty: the caller gave none
  std::vector<int32_t> cl_off, cl_fam;   // CSR cluster -> its families, stable: the reference's loop order (cl_fam: one word at least)
  std::vector<char> tip;                 // [n_families] child_pos < 0, a data row and a parent edge
  bool uni_ok = false;                   // every belief <= 2 variables and p = 1: the thread-per-site fill applies
  // one record per cluster where every cluster holds exactly one family with at most one parent and there are no scope masks
  // (else empty), and the family each was made from
  std::vector<LgSimpleFam> simple;
  std::vector<int32_t> simple_fam;

  unsigned long long full_mask() const { return p >= 64 ? ~0ull : ((1ull << p) - 1ull); }

  // The checks below return false with the message in `why`; nothing has changed then.

  // pgbp_lg_set_edges: lengths of real edges positive and finite, inheritances finite (either array may be null: left as it is)
  bool check_edges(const double* new_length, const double* new_gamma, std::string& why) const;
  // ... and, after the check: the table's copies and those of the simple records
  void set_edges(const double* new_length, const double* new_gamma);
  // pgbp_lg_set_data / pgbp_lg_get_data (`fn`): the site range, the buffer and -- values -- finite where the table says observed
  // (miss: the per-site mask in force, null: none -- an entry it masks is not observed and may hold anything)
  bool check_data(const char* fn, int32_t site_begin, int32_t site_end, const double* data, bool values, std::string& why,
                  const SiteMissPack* miss = nullptr) const;
  // pgbp_lg_set_shifts: slot [max(1, n_families * K)] = index into the list of the shift on that edge, -1: none; cl = the
  // clusters that hold a shifted family, sorted, each once
  bool shift_list(int32_t n_shifts, const int32_t* edge, const double* value, int32_t per_site, std::vector<int32_t>& slot,
                  std::vector<int32_t>& cl, std::string& why) const;
  // pgbp_lg_set_optima: map [max(1, n_families * K)] = the regime of that edge, 0 where the edge keeps theta and at every entry
  // the call ignores (root priors, k >= n_parents[f]); cl = the clusters that hold a family with a painted edge, sorted, each once
  bool optima_list(int32_t n_regimes, const int32_t* regime, const double* value, int32_t per_site, std::vector<int32_t>& map,
                   std::vector<int32_t>& cl, std::string& why) const;
  // pgbp_lg_set_tip_noise, host part: slot [max(1, n_families)]; sig = sigma_e with the two triangles averaged; cl = the clusters
  // that hold a noisy tip family, sorted, each once, and the largest dimension among them
  bool noise_list(int32_t n, const int32_t* family, const double* scale, const double* sigma_e, const double* se2,
                  int32_t per_site, std::vector<int32_t>& slot, std::vector<double>& sig, std::vector<int32_t>& cl,
                  int32_t* max_dim, std::string& why) const;

  // Which cluster a family sits in is `cluster`.  max_m (may be null): the largest dimension among the clusters that hold a
  // family, 0 without families.  limit > 0: a family in a cluster of more than `limit` variables is refused,
  // "<fn>: family F (cluster C): the cluster has more than <limit> variables" (the first in CSR order).
  bool cluster_dims(const char* fn, int limit, int* max_m, std::string& why) const;
  // pgbp_lg_loo: the tip families with an observed trait, in table order
  std::vector<int32_t> loo_tips() const;
  // pgbp_lg_impute: the tip families with a missing trait, in table order, and the traits predicted for each (missing, and in
  // the scope of every cluster parent); nothing without both masks
  void impute_list(std::vector<int32_t>& fams, std::vector<unsigned long long>& predicted) const;
};

// Every check of pgbp_lg_setup, in its order: false with the message in `why` (empty: an argument that is refused without
// one), `out` untouched.  dims [n_clusters], n_sites, max_dim: of the engine's plan.
bool lg_table_build(const pgbp_lg_families* f, const int32_t* dims, int32_t n_clusters, int32_t n_sites, int32_t max_dim,
                    LgTable& out, std::string& why);

}  // namespace pgbp

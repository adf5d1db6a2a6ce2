// Per-site clade shifts of the OU optimum (pgbp_lg_set_clade_shifts_sites of include/pgbp.h), host side: the preorder numbering
// of the family tree that turns "family f lies in clade(v)" into two integer comparisons, the checks of a setting, and the
// clusters the fill correction visits.  Plain C++ without the runtime, so that a stand-alone program can run it under a host
// sanitizer (tests/clade_shift_check.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace pgbp {

// pre[f]: the preorder rank of family f in the family tree (the roots in index order, the children of a family in index order);
// last[f]: the largest rank inside clade(f), so that g lies in clade(f) iff pre[f] <= pre[g] <= last[f].
struct CladePlan {
  std::vector<int32_t> pre, last;
  bool built = false;

  void clear() { *this = CladePlan{}; }
};

// parent_family[f * K + k], k < n_parents[f], as lg_topology_levels (pgbp_topology.hpp) has checked it: every entry < f, or
// negative (a root).  Only the first parent is read (a network is refused by the setter, not here).  false with `err` (out
// cleared) when an entry is not: the plan never indexes outside.
bool clade_plan_build(int32_t n_families, int32_t K, const int32_t* n_parents, const int32_t* parent_family, CladePlan& out,
                      std::string& err);

// The checks of a setting family / delta [n_slots][n_sites] (-1: an empty slot, whose delta is not read): every family in range,
// with a parent edge (a root-prior family is refused), at most once per site; every delta of a used slot finite.  false with
// `err` naming slot, site and family.
bool clade_setting_check(const CladePlan& plan, const int32_t* n_parents, int32_t n_slots, int32_t n_sites, const int32_t* family,
                         const double* delta, std::string& err);
// the values alone, against the families in force
bool clade_values_check(int32_t n_slots, int32_t n_sites, const int32_t* family, const double* delta, std::string& err);

// The clusters (sorted, each once) that hold a family inside at least one site's clade: the union of the rank intervals
// [pre[v], last[v]] over the used slots of all sites by a difference array, then the clusters of the covered families.
// cluster[f]: the cluster of family f.  The setting has passed clade_setting_check.
void clade_clusters(const CladePlan& plan, const int32_t* cluster, int32_t n_slots, int32_t n_sites, const int32_t* family,
                    std::vector<int32_t>& out);

}  // namespace pgbp

// The plan of the optimum-shift scan (pgbp_lg_optimum_scan_sites of include/pgbp.h), host side: from the node topology of a
// family table (pgbp_lg_set_topology) the child families of every family, the heights and the families grouped by height.
// Plain C++ without the runtime, so that a stand-alone program can run it under a host sanitizer
// (tests/optimum_scan_check.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace pgbp {

// child_off [n_families + 1] -> child_fam: the families whose (first) parent is the child of family f, in index order.
// height[f]: 0 for a family without child families (a tip), else 1 + the largest height of its child families.
// height_off [n_heights + 1] -> height_fam [n_families]: the families of a height in index order.
// multi: the first family with two or more parents, -1: none (the scan is defined on trees; its lists then hold the first
// parent only and are not used).
struct OptScanPlan {
  std::vector<int32_t> child_off, child_fam, height, height_off, height_fam;
  int32_t multi = -1;
  bool built = false;

  void clear() { *this = OptScanPlan{}; }
  int32_t n_heights() const { return height_off.empty() ? 0 : (int32_t)height_off.size() - 1; }
};

// parent_family[f * K + k], k < n_parents[f]: as lg_topology_levels (pgbp_topology.hpp) takes and has checked it -- every
// entry < f, or negative (a root).  false with `err` (out cleared) when an entry is not: the plan never indexes outside.
bool optscan_plan_build(int32_t n_families, int32_t K, const int32_t* n_parents, const int32_t* parent_family, OptScanPlan& out,
                        std::string& err);

// the single-parent check of the scan: true on a tree; false with `err` naming the family otherwise
bool optscan_plan_single_parents(const OptScanPlan& plan, const int32_t* n_parents, std::string& err);

// doubles of scratch a site takes: four state rows per family, the requested tables, the candidates of the top fold, and per
// block of 64 families the fold's record (best, family) with the marks of the validity pass (nvb blocks)
int64_t optscan_per_site(int64_t n_families, int n_tables, bool top, int64_t n_blocks, int64_t nvb);

}  // namespace pgbp

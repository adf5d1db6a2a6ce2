// Node topology of a family table (pgbp_lg_set_topology of include/pgbp.h), host side: validation and levelling.
// Plain C++ without the runtime, so that a stand-alone program can run it under a host sanitizer
// (tests/host/topology_check.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace pgbp {

constexpr int32_t kTopoFixedRoot = -1;   // the parent is the fixed root: its value is mu
constexpr int32_t kTopoImproper = -2;    // the parent is a root without a proper prior: nothing can be simulated

// parent_family[f * K + k], k < n_parents[f]: the family whose child is parent k of family f, kTopoFixedRoot or kTopoImproper
// (entries with k >= n_parents[f] are not read).  Checks every entry (in range, and < f: families are in preorder) and levels
// the table: the root (fixed or improper) and a root-prior family have level 0, every other family 1 + the largest level of
// its parents.  level_off [n_levels + 1] -> level_fam [n_families], the families of a level in index order (level 0 is empty
// under a fixed root).  improper: the first entry f * K + k that is kTopoImproper, -1 when there is none.
// false with `err` naming the entry ("family F, parent K: ..."), the outputs untouched, when the table is not valid.
bool lg_topology_levels(int32_t n_families, int32_t K, const int32_t* n_parents, const int32_t* parent_family,
                        std::vector<int32_t>& level_off, std::vector<int32_t>& level_fam, int32_t* improper, std::string& err);

}  // namespace pgbp

// Validation and levelling of the node topology of a family table (pgbp_topology.hpp).
#include "pgbp_topology.hpp"

#include <algorithm>

namespace pgbp {

bool lg_topology_levels(int32_t n_families, int32_t K, const int32_t* n_parents, const int32_t* parent_family,
                        std::vector<int32_t>& level_off, std::vector<int32_t>& level_fam, int32_t* improper, std::string& err) {
  if (n_families < 0 || K < 1 || (n_families > 0 && (!n_parents || !parent_family))) {
    err = "no table";
    return false;
  }
  std::vector<int32_t> level((size_t)n_families, 0);
  int32_t first_improper = -1, n_levels = n_families > 0 ? 1 : 0;
  for (int32_t f = 0; f < n_families; ++f) {
    const int32_t np = n_parents[f];
    if (np < 0 || np > K) {
      err = "family " + std::to_string(f) + ": number of parents out of range";
      return false;
    }
    int32_t lv = 0;
    for (int32_t k = 0; k < np; ++k) {
      const int32_t pf = parent_family[(size_t)f * K + k];
      const std::string where = "family " + std::to_string(f) + ", parent " + std::to_string(k) + ": ";
      if (pf < kTopoImproper || pf >= n_families) {
        err = where + "parent family " + std::to_string(pf) + " out of range (" + std::to_string(n_families) + " families, -1: the fixed root, -2: an improper root)";
        return false;
      }
      if (pf >= f) {
        err = where + "parent family " + std::to_string(pf) + " does not come before its child (families are in preorder)";
        return false;
      }
      if (pf == kTopoImproper && first_improper < 0) first_improper = f * K + k;
      lv = std::max(lv, 1 + (pf >= 0 ? level[pf] : 0));
    }
    level[f] = lv;
    n_levels = std::max(n_levels, lv + 1);
  }
  std::vector<int32_t> off((size_t)n_levels + 1, 0), fam((size_t)n_families);
  for (int32_t f = 0; f < n_families; ++f) ++off[level[f] + 1];
  for (int32_t l = 0; l < n_levels; ++l) off[l + 1] += off[l];
  std::vector<int32_t> at(off.begin(), off.end() - 1);
  for (int32_t f = 0; f < n_families; ++f) fam[at[level[f]]++] = f;
  level_off = std::move(off);
  level_fam = std::move(fam);
  if (improper) *improper = first_improper;
  return true;
}

}  // namespace pgbp

// Child lists, heights and the families by height of a family table's node topology (pgbp_optscan_host.hpp).
#include "pgbp_optscan_host.hpp"

#include <algorithm>

namespace pgbp {

bool optscan_plan_build(int32_t n_families, int32_t K, const int32_t* n_parents, const int32_t* parent_family, OptScanPlan& out,
                        std::string& err) {
  out.clear();
  if (n_families < 0 || K < 1 || (n_families > 0 && (!n_parents || !parent_family))) {
    err = "no table";
    return false;
  }
  const size_t nf = (size_t)n_families;
  OptScanPlan P;
  // the first parent of every family (-1: none, or a root), checked
  std::vector<int32_t> pa(nf, -1);
  for (int32_t f = 0; f < n_families; ++f) {
    const int32_t np = n_parents[f];
    if (np < 0 || np > K) {
      err = "family " + std::to_string(f) + ": number of parents out of range";
      return false;
    }
    if (np >= 2 && P.multi < 0) P.multi = f;
    if (np == 0) continue;
    const int32_t pf = parent_family[(size_t)f * K];
    if (pf >= f) {
      err = "family " + std::to_string(f) + ", parent 0: parent family " + std::to_string(pf) +
            " does not come before its child (families are in preorder)";
      return false;
    }
    pa[f] = pf < 0 ? -1 : pf;
  }
  // the child lists by a counting sort: a list keeps index order
  P.child_off.assign(nf + 1, 0);
  for (size_t f = 0; f < nf; ++f)
    if (pa[f] >= 0) ++P.child_off[(size_t)pa[f] + 1];
  for (size_t f = 0; f < nf; ++f) P.child_off[f + 1] += P.child_off[f];
  P.child_fam.assign((size_t)P.child_off[nf], 0);
  {
    std::vector<int32_t> at(P.child_off.begin(), P.child_off.end() - 1);
    for (size_t f = 0; f < nf; ++f)
      if (pa[f] >= 0) P.child_fam[(size_t)at[(size_t)pa[f]]++] = (int32_t)f;
  }
  // heights: a parent comes before its children, so one pass from the last family down sees every child first
  P.height.assign(nf, 0);
  int32_t n_heights = n_families > 0 ? 1 : 0;
  for (size_t f = nf; f-- > 0;) {
    n_heights = std::max(n_heights, P.height[f] + 1);
    if (pa[f] >= 0) P.height[(size_t)pa[f]] = std::max(P.height[(size_t)pa[f]], P.height[f] + 1);
  }
  P.height_off.assign((size_t)n_heights + 1, 0);
  for (size_t f = 0; f < nf; ++f) ++P.height_off[(size_t)P.height[f] + 1];
  for (int32_t h = 0; h < n_heights; ++h) P.height_off[(size_t)h + 1] += P.height_off[(size_t)h];
  P.height_fam.assign(nf, 0);
  {
    std::vector<int32_t> at(P.height_off.begin(), P.height_off.end() - 1);
    for (size_t f = 0; f < nf; ++f) P.height_fam[(size_t)at[(size_t)P.height[f]]++] = (int32_t)f;
  }
  P.built = true;
  out = std::move(P);
  return true;
}

bool optscan_plan_single_parents(const OptScanPlan& plan, const int32_t* n_parents, std::string& err) {
  if (plan.multi < 0) return true;
  err = "family " + std::to_string(plan.multi) + " has " + std::to_string(n_parents ? n_parents[plan.multi] : 2) +
        " parents: the scan of a clade's optimum is defined on a tree, where every family has one parent";
  return false;
}

int64_t optscan_per_site(int64_t n_families, int n_tables, bool top, int64_t n_blocks, int64_t nvb) {
  return n_families * (4 + (int64_t)n_tables + (top ? 1 : 0)) + (top ? 2 * n_blocks : 0) + nvb;
}

}  // namespace pgbp

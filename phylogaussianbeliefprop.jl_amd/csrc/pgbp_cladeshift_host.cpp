// Preorder ranks of the family tree, the checks of a per-site clade-shift setting and the clusters its correction visits
// (pgbp_cladeshift_host.hpp).
#include "pgbp_cladeshift_host.hpp"

#include <algorithm>
#include <cmath>

namespace pgbp {

bool clade_plan_build(int32_t n_families, int32_t K, const int32_t* n_parents, const int32_t* parent_family, CladePlan& out,
                      std::string& err) {
  out.clear();
  if (n_families < 0 || K < 1 || (n_families > 0 && (!n_parents || !parent_family))) {
    err = "no table";
    return false;
  }
  const size_t nf = (size_t)n_families;
  std::vector<int32_t> pa(nf, -1);
  for (int32_t f = 0; f < n_families; ++f) {
    const int32_t np = n_parents[f];
    if (np < 0 || np > K) {
      err = "family " + std::to_string(f) + ": number of parents out of range";
      return false;
    }
    if (np == 0) continue;
    const int32_t pf = parent_family[(size_t)f * K];
    if (pf >= f) {
      err = "family " + std::to_string(f) + ", parent 0: parent family " + std::to_string(pf) +
            " does not come before its child (families are in preorder)";
      return false;
    }
    pa[f] = pf < 0 ? -1 : pf;
  }
  // sizes of the clades: a parent comes before its children, so one pass from the last family down sees every child first
  std::vector<int32_t> size(nf, 1);
  for (size_t f = nf; f-- > 0;)
    if (pa[f] >= 0) size[(size_t)pa[f]] += size[f];
  // ranks: a family's children take consecutive blocks after it in index order; `next[u]`: the rank the next child of u gets
  // (next of the forest's roots: one running counter)
  CladePlan P;
  P.pre.assign(nf, 0);
  P.last.assign(nf, 0);
  std::vector<int32_t> next(nf, 0);
  int32_t next_root = 0;
  for (size_t f = 0; f < nf; ++f) {
    int32_t& at = pa[f] >= 0 ? next[(size_t)pa[f]] : next_root;
    P.pre[f] = at;
    at += size[f];
    P.last[f] = P.pre[f] + size[f] - 1;
    next[f] = P.pre[f] + 1;
  }
  P.built = true;
  out = std::move(P);
  return true;
}

bool clade_setting_check(const CladePlan& plan, const int32_t* n_parents, int32_t n_slots, int32_t n_sites, const int32_t* family,
                         const double* delta, std::string& err) {
  if (n_slots < 0 || n_sites < 0) {
    err = "negative number of slots or sites";
    return false;
  }
  if (n_slots == 0) return true;
  if (!plan.built) {
    err = "no topology";
    return false;
  }
  if (!family || !delta || !n_parents) {
    err = "no table of families or of deltas";
    return false;
  }
  const int64_t nf = (int64_t)plan.pre.size();
  const size_t ns = (size_t)n_sites;
  for (size_t s = 0; s < ns; ++s)
    for (int32_t j = 0; j < n_slots; ++j) {
      const int32_t v = family[(size_t)j * ns + s];
      if (v == -1) continue;
      const std::string where = "slot " + std::to_string(j) + " at site " + std::to_string(s) + ": ";
      if (v < 0 || v >= nf) {
        err = where + "family " + std::to_string(v) + " out of range (" + std::to_string(nf) + " families; -1 marks an empty slot)";
        return false;
      }
      if (n_parents[v] == 0) {
        err = where + "family " + std::to_string(v) + " is a root-prior family: it has no parent edge whose optimum could shift";
        return false;
      }
      for (int32_t i = 0; i < j; ++i)
        if (family[(size_t)i * ns + s] == v) {
          err = where + "family " + std::to_string(v) + " appears twice at site " + std::to_string(s) + " (also in slot " +
                std::to_string(i) + ")";
          return false;
        }
      if (!std::isfinite(delta[(size_t)j * ns + s])) {
        err = where + "the delta of family " + std::to_string(v) + " is not finite";
        return false;
      }
    }
  return true;
}

bool clade_values_check(int32_t n_slots, int32_t n_sites, const int32_t* family, const double* delta, std::string& err) {
  if (n_slots <= 0) return true;
  if (!family || !delta) {
    err = "no values";
    return false;
  }
  const size_t ns = (size_t)n_sites;
  for (size_t s = 0; s < ns; ++s)
    for (int32_t j = 0; j < n_slots; ++j) {
      const int32_t v = family[(size_t)j * ns + s];
      if (v >= 0 && !std::isfinite(delta[(size_t)j * ns + s])) {
        err = "slot " + std::to_string(j) + " at site " + std::to_string(s) + ": the delta of family " + std::to_string(v) +
              " is not finite";
        return false;
      }
    }
  return true;
}

void clade_clusters(const CladePlan& plan, const int32_t* cluster, int32_t n_slots, int32_t n_sites, const int32_t* family,
                    std::vector<int32_t>& out) {
  out.clear();
  const size_t nf = plan.pre.size();
  if (!plan.built || nf == 0 || n_slots <= 0 || n_sites <= 0 || !family || !cluster) return;
  std::vector<int64_t> diff(nf + 1, 0);   // +1 at the first rank of an interval, -1 past its last
  const size_t n = (size_t)n_slots * (size_t)n_sites;
  for (size_t i = 0; i < n; ++i) {
    const int32_t v = family[i];
    if (v < 0 || (size_t)v >= nf) continue;
    ++diff[(size_t)plan.pre[(size_t)v]];
    --diff[(size_t)plan.last[(size_t)v] + 1];
  }
  std::vector<char> covered(nf, 0);   // by rank
  int64_t run = 0;
  for (size_t r = 0; r < nf; ++r) {
    run += diff[r];
    covered[r] = run > 0;
  }
  for (size_t f = 0; f < nf; ++f)
    if (covered[(size_t)plan.pre[f]]) out.push_back(cluster[f]);
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
}

}  // namespace pgbp

// The family table of pgbp_lg_setup on the host: its checks and the lists derived from it (pgbp_lgtable.hpp).
#include "pgbp_lgtable.hpp"

#include <algorithm>
#include <cmath>
#include <utility>

namespace pgbp {

static bool refuse(std::string& why, const std::string& msg) {
  why = msg;
  return false;
}

bool lg_table_build(const pgbp_lg_families* f, const int32_t* dims, int32_t n_clusters, int32_t n_sites, int32_t max_dim,
                    LgTable& out, std::string& why) {
  if (!f || f->p <= 0 || f->p > PGBP_MAX_DIM || f->n_families < 0 || f->max_parents < 1 || f->n_rates < 1 || f->n_rows < 0)
    return refuse(why, "");
  if (f->n_families > 0 && (!f->cluster || !f->n_parents || !f->child_pos || !f->data_row || !f->parent_pos || !f->length ||
                            !f->gamma || !f->color))
    return refuse(why, "");
  if (f->n_rows > 0 && !f->data) return refuse(why, "pgbp_lg_setup: data missing");
  const int nc = n_clusters, K = f->max_parents, pp = f->p;
  if ((f->child_mask || f->parent_mask) && pp > 64) return refuse(why, "pgbp_lg_setup: scope masks need p <= 64");
  LgTable T;
  T.p = pp;
  const unsigned long long full = T.full_mask();
  auto cmask = [&](int i) { return f->child_mask ? (unsigned long long)f->child_mask[i] & full : full; };
  auto pmask = [&](int i, int k) { return f->parent_mask ? (unsigned long long)f->parent_mask[(size_t)i * K + k] & full : full; };
  // every family fits its cluster; the blocks of one family do not overlap
  std::vector<int32_t> count(nc + 1, 0);
  if (f->n_rows > 0 && !f->child_mask)
    for (size_t i = 0, n = (size_t)n_sites * f->n_rows * pp; i < n; ++i)
      if (!std::isfinite(f->data[i]))
        return refuse(why, "pgbp_lg_setup: a tip value is missing or not finite (missing values need child_mask / parent_mask)");
  for (int i = 0; i < f->n_families; ++i) {
    const std::string where = "pgbp_lg_setup: family " + std::to_string(i) + ": ";
    const int c = f->cluster[i], np = f->n_parents[i];
    if (c < 0 || c >= nc) return refuse(why, where + "cluster out of range");
    if (np < 0 || np > K) return refuse(why, where + "number of parents out of range");
    const int m = dims[c];
    std::vector<std::pair<int, int>> pos;  // (first variable, number of variables) of every in-scope block
    const int cp = f->child_pos[i];
    const unsigned long long O = cmask(i);
    if (cp < 0 && O == 0 && f->child_mask) {
      // a node with nothing in scope (no data below it) or a tip with every trait missing: the factor integrates to 1
    } else if (cp < 0) {
      if (np == 0) return refuse(why, where + "a root prior needs the root in scope");
      if (f->data_row[i] < 0 || f->data_row[i] >= f->n_rows) return refuse(why, where + "data row out of range");
      for (int s2 = 0; s2 < n_sites; ++s2)
        for (int t = 0; t < pp; ++t)
          if (((O >> t) & 1ull) && !std::isfinite(f->data[((size_t)s2 * f->n_rows + f->data_row[i]) * pp + t]))
            return refuse(why, where + "a tip value is missing or not finite where child_mask says observed "
                                  "(missing values: clear the trait's bit in child_mask; one pattern for all sites)");
    } else {
      pos.push_back({cp, __builtin_popcountll(O)});
    }
    if (np == 0 && (f->color[(size_t)i * K] < 0 || f->color[(size_t)i * K] >= f->n_rates))
      return refuse(why, where + "rate index out of range");
    for (int k = 0; k < np; ++k) {
      const size_t o = (size_t)i * K + k;
      if (!(f->length[o] > 0.0) || !std::isfinite(f->length[o]))
        return refuse(why, where + "parent edge length must be positive (degenerate families are out of scope)");
      if (!std::isfinite(f->gamma[o])) return refuse(why, where + "inheritance not finite");
      if (f->color[o] < 0 || f->color[o] >= f->n_rates) return refuse(why, where + "rate index out of range");
      if (f->parent_pos[o] >= 0) {
        if ((O & ~pmask(i, k)) != 0) return refuse(why, where + "a trait kept by the child is out of the parent's scope");
        pos.push_back({f->parent_pos[o], __builtin_popcountll(pmask(i, k))});
      }
    }
    std::sort(pos.begin(), pos.end());
    for (size_t a = 0; a < pos.size(); ++a)
      if (pos[a].first + pos[a].second > m || (a > 0 && pos[a].first < pos[a - 1].first + pos[a - 1].second))
        return refuse(why, where + "variable blocks overlap or leave the cluster (dimension " + std::to_string(m) + ")");
    ++count[c + 1];
  }
  for (int c = 0; c < nc; ++c) count[c + 1] += count[c];
  std::vector<int32_t> fam(std::max(1, f->n_families));
  {
    std::vector<int32_t> at(count.begin(), count.end() - 1);
    for (int i = 0; i < f->n_families; ++i) fam[at[f->cluster[i]]++] = i;  // stable: the reference's loop order
  }
  const size_t nf = (size_t)f->n_families, nfk = nf * K;
  T.K = K, T.n_rates = f->n_rates, T.n_rows = f->n_rows, T.n_families = f->n_families, T.n_sites = n_sites;
  T.dims.assign(dims, dims + nc);
  T.cluster.assign(f->cluster, f->cluster + nf);   // (an empty table: null + 0)
  T.n_parents.assign(f->n_parents, f->n_parents + nf);
  T.child_pos.assign(f->child_pos, f->child_pos + nf);
  T.data_row.assign(f->data_row, f->data_row + nf);
  T.parent_pos.assign(f->parent_pos, f->parent_pos + nfk);
  T.color.assign(f->color, f->color + nfk);
  T.length.assign(f->length, f->length + nfk);
  T.gamma.assign(f->gamma, f->gamma + nfk);
  for (size_t i = 0; f->child_mask && i < nf; ++i) T.child_mask.push_back(cmask((int)i));
  for (size_t i = 0; f->parent_mask && i < nfk; ++i) T.parent_mask.push_back(pmask((int)(i / K), (int)(i % K)));
  T.tip.assign(nf, 0);
  for (size_t i = 0; i < nf; ++i) T.tip[i] = f->child_pos[i] < 0 && f->data_row[i] >= 0 && f->n_parents[i] >= 1;
  T.uni_ok = max_dim <= 2 && pp == 1;
  if (T.uni_ok && !f->child_mask && !f->parent_mask && f->n_families == nc) {
    std::vector<LgSimpleFam> sf(nc);
    std::vector<int32_t> sfam(nc);
    bool simple = true;
    for (int c = 0; c < nc && simple; ++c) {
      if (count[c + 1] - count[c] != 1) { simple = false; break; }
      const int i = fam[count[c]];
      const int np = f->n_parents[i];
      if (np > 1) { simple = false; break; }
      LgSimpleFam r{};
      r.np = np; r.cpos = f->child_pos[i]; r.row = f->data_row[i];
      r.ppos = np > 0 ? f->parent_pos[(size_t)i * K] : -1;
      r.color = f->color[(size_t)i * K];
      r.length = np > 0 ? f->length[(size_t)i * K] : 0.0;
      r.gamma = np > 0 ? f->gamma[(size_t)i * K] : 0.0;
      if (r.cpos > 1 || r.ppos > 1) { simple = false; break; }
      sf[c] = r;
      sfam[c] = i;
    }
    if (simple) {
      T.simple = std::move(sf);
      T.simple_fam = std::move(sfam);
    }
  }
  T.cl_off = std::move(count);
  T.cl_fam = std::move(fam);
  out = std::move(T);
  return true;
}

bool LgTable::check_edges(const double* new_length, const double* new_gamma, std::string& why) const {
  for (int i = 0; i < n_families; ++i)
    for (int k = 0; k < n_parents[i]; ++k) {
      const size_t o = (size_t)i * K + k;
      const bool bad_length = new_length && (!(new_length[o] > 0.0) || !std::isfinite(new_length[o]));
      if (bad_length || (new_gamma && !std::isfinite(new_gamma[o])))
        return refuse(why, "pgbp_lg_set_edges: family " + std::to_string(i) + ": " +
                               (bad_length ? "parent edge length must be positive (degenerate families are out of scope)"
                                           : "inheritance not finite"));
    }
  return true;
}

void LgTable::set_edges(const double* new_length, const double* new_gamma) {
  const size_t nfk = (size_t)n_families * K;
  if (new_length) length.assign(new_length, new_length + nfk);
  if (new_gamma) gamma.assign(new_gamma, new_gamma + nfk);
  for (size_t c = 0; c < simple.size(); ++c) {   // the per-cluster records of the thread-per-site fill carry their own copies
    LgSimpleFam& r = simple[c];
    if (r.np == 0) continue;
    const size_t o = (size_t)simple_fam[c] * K;
    r.length = length[o];
    r.gamma = gamma[o];
  }
}

bool LgTable::check_data(const char* fn, int32_t site_begin, int32_t site_end, const double* data, bool values,
                         std::string& why, const SiteMissPack* miss) const {
  if (site_begin < 0 || site_end < site_begin || site_end > n_sites)
    return refuse(why, std::string(fn) + ": site range [" + std::to_string(site_begin) + ", " + std::to_string(site_end) +
                           ") outside the engine's " + std::to_string(n_sites) + " sites");
  const size_t per = (size_t)n_rows * p, ns = (size_t)(site_end - site_begin);
  if (ns * per > 0 && !data) return refuse(why, std::string(fn) + ": no data buffer");
  if (!values) return true;
  if (miss && !miss->words.empty()) {   // (p = 1: the mask is accepted on univariate tables only)
    for (int f = 0; f < n_families; ++f) {
      if (!tip[f] || (!child_mask.empty() && !(child_mask[f] & 1ull))) continue;
      for (size_t s = 0; s < ns; ++s)
        if (!site_missing_test(*miss, data_row[f], site_begin + (int32_t)s) && !std::isfinite(data[(s * n_rows + data_row[f]) * p]))
          return refuse(why, std::string(fn) + ": family " + std::to_string(f) + ", site " + std::to_string(site_begin + (int32_t)s) +
                        ": a tip value is missing or not finite where neither child_mask nor the per-site mask says so");
    }
    return true;
  }
  if (child_mask.empty()) {
    for (size_t i = 0; i < ns * per; ++i)
      if (!std::isfinite(data[i]))
        return refuse(why, std::string(fn) + ": a tip value is missing or not finite (the table has no child_mask: the data are complete)");
    return true;
  }
  for (int f = 0; f < n_families; ++f) {
    if (!tip[f]) continue;
    const unsigned long long O = child_mask[f];
    for (size_t s = 0; s < ns; ++s)
      for (int t = 0; t < p; ++t)
        if (((O >> t) & 1ull) && !std::isfinite(data[(s * n_rows + data_row[f]) * p + t]))
          return refuse(why, std::string(fn) + ": family " + std::to_string(f) + ": a tip value is missing or not finite "
                        "where child_mask says observed (the missing-data pattern is the set-up's)");
  }
  return true;
}

// the distinct clusters of the listed families, in index order
static std::vector<int32_t> clusters_of(const std::vector<int32_t>& cluster, int32_t n, const int32_t* index, int32_t per_family) {
  std::vector<int32_t> cl;
  for (int i = 0; i < n; ++i) cl.push_back(cluster[index[i] / per_family]);
  std::sort(cl.begin(), cl.end());
  cl.erase(std::unique(cl.begin(), cl.end()), cl.end());
  return cl;
}

bool LgTable::shift_list(int32_t n_shifts, const int32_t* edge, const double* value, int32_t per_site, std::vector<int32_t>& slot,
                         std::vector<int32_t>& cl, std::string& why) const {
  if (n_shifts < 0 || (n_shifts > 0 && (!edge || !value))) return refuse(why, "pgbp_lg_set_shifts: a negative count or a missing array");
  const int nf = n_families;
  const size_t ns = per_site ? (size_t)n_sites : 1, n = (size_t)n_shifts;
  std::vector<int32_t> sl(std::max<size_t>(1, (size_t)nf * K), -1);
  for (int i = 0; i < n_shifts; ++i) {
    const std::string where = "pgbp_lg_set_shifts: entry " + std::to_string(i) + " (edge " + std::to_string(edge[i]) + "): ";
    if (edge[i] < 0 || (int64_t)edge[i] >= (int64_t)nf * K) return refuse(why, where + "edge index out of range");
    const int fam = edge[i] / K, k = edge[i] - fam * K;
    if (n_parents[fam] == 0) return refuse(why, where + "family " + std::to_string(fam) + " is a root prior, it has no edge");
    if (k >= n_parents[fam])
      return refuse(why, where + "family " + std::to_string(fam) + " has " + std::to_string(n_parents[fam]) + " parent edges, no edge " +
                    std::to_string(k));
    if (sl[edge[i]] >= 0)
      return refuse(why, where + "the edge is listed twice (entry " + std::to_string(sl[edge[i]]) + " has it too)");
    sl[edge[i]] = i;
    for (size_t s = 0; s < ns; ++s)
      for (int t = 0; t < p; ++t)
        if (!std::isfinite(value[(s * n + i) * p + t]))
          return refuse(why, where + "the value of trait " + std::to_string(t) + " is not finite");
  }
  slot = std::move(sl);
  cl = clusters_of(cluster, n_shifts, edge, K);
  return true;
}

bool LgTable::optima_list(int32_t n_regimes, const int32_t* regime, const double* value, int32_t per_site, std::vector<int32_t>& map,
                          std::vector<int32_t>& cl, std::string& why) const {
  if (n_regimes < 0 || (n_regimes > 0 && (!regime || !value))) return refuse(why, "pgbp_lg_set_optima: a negative count or a missing array");
  const int nf = n_families;
  const size_t ns = per_site ? (size_t)n_sites : 1, n = (size_t)n_regimes;
  std::vector<int32_t> mp(std::max<size_t>(1, (size_t)nf * K), 0), c;
  for (int f = 0; f < nf && n_regimes > 0; ++f) {
    bool painted = false;
    for (int k = 0; k < n_parents[f]; ++k) {
      const int32_t r = regime[(size_t)f * K + k];
      if (r < 0 || r > n_regimes)
        return refuse(why, "pgbp_lg_set_optima: entry " + std::to_string((size_t)f * K + k) + " (family " + std::to_string(f) + ", edge " +
                               std::to_string(k) + "): regime " + std::to_string(r) + " is not in 0 .. " + std::to_string(n_regimes));
      mp[(size_t)f * K + k] = r;
      painted |= r > 0;
    }
    if (painted) c.push_back(cluster[f]);
  }
  for (size_t s = 0; s < ns; ++s)
    for (size_t r = 0; r < n; ++r)
      for (int t = 0; t < p; ++t)
        if (!std::isfinite(value[(s * n + r) * p + t]))
          return refuse(why, "pgbp_lg_set_optima: value of regime " + std::to_string(r + 1) + (per_site ? " at site " + std::to_string(s) : std::string()) +
                                 ": trait " + std::to_string(t) + " is not finite");
  std::sort(c.begin(), c.end());
  c.erase(std::unique(c.begin(), c.end()), c.end());
  map = std::move(mp);
  cl = std::move(c);
  return true;
}

bool LgTable::noise_list(int32_t n, const int32_t* family, const double* scale, const double* sigma_e, const double* se2,
                         int32_t per_site, std::vector<int32_t>& slot, std::vector<double>& sig, std::vector<int32_t>& cl,
                         int32_t* max_dim, std::string& why) const {
  if (n < 0 || (n > 0 && (!family || !scale || !sigma_e)))
    return refuse(why, "pgbp_lg_set_tip_noise: a negative count or a missing array");
  const int nf = n_families, pp = p;
  const size_t ns = per_site ? (size_t)n_sites : 1, nn = (size_t)n;
  std::vector<int32_t> sl(std::max<size_t>(1, (size_t)nf), -1);
  std::vector<double> sg;   // sigma_e with the two triangles averaged: exactly symmetric on the device
  if (n > 0) {
    sg.assign(sigma_e, sigma_e + ns * pp * pp);
    for (size_t s = 0; s < ns; ++s) {
      const double* A = sigma_e + s * pp * pp;
      const std::string where = "pgbp_lg_set_tip_noise: sigma_e" + (per_site ? " of site " + std::to_string(s) : std::string()) + ": ";
      double big = 0.0;
      for (int a = 0; a < pp * pp; ++a) {
        if (!std::isfinite(A[a]))
          return refuse(why, where + "entry (" + std::to_string(a / pp) + ", " + std::to_string(a % pp) + ") is not finite");
        big = std::max(big, std::fabs(A[a]));
      }
      for (int i = 0; i < pp; ++i) {
        if (A[i * pp + i] < 0.0) return refuse(why, where + "diagonal entry " + std::to_string(i) + " is negative");
        for (int j = 0; j < i; ++j) {
          if (std::fabs(A[i * pp + j] - A[j * pp + i]) > 1e-12 * big)
            return refuse(why, where + "entries (" + std::to_string(i) + ", " + std::to_string(j) + ") and (" + std::to_string(j) + ", " +
                          std::to_string(i) + ") differ: the matrix is not symmetric");
          sg[s * pp * pp + i * pp + j] = sg[s * pp * pp + j * pp + i] = 0.5 * (A[i * pp + j] + A[j * pp + i]);
        }
      }
    }
  }
  for (int i = 0; i < n; ++i) {
    const std::string where = "pgbp_lg_set_tip_noise: entry " + std::to_string(i) + " (family " + std::to_string(family[i]) + "): ";
    if (family[i] < 0 || family[i] >= nf) return refuse(why, where + "family index out of range");
    if (!tip[family[i]]) return refuse(why, where + "not a tip family (child_pos < 0, a data row and a parent edge)");
    if (sl[family[i]] >= 0)
      return refuse(why, where + "the family is listed twice (entry " + std::to_string(sl[family[i]]) + " has it too)");
    sl[family[i]] = i;
    if (!std::isfinite(scale[i])) return refuse(why, where + "the scale is not finite");
    if (scale[i] < 0.0) return refuse(why, where + "the scale is negative");
    for (size_t s = 0; se2 && s < ns; ++s)
      for (int t = 0; t < pp; ++t) {
        const double v = se2[(s * nn + i) * pp + t];
        if (!std::isfinite(v)) return refuse(why, where + "se2 of trait " + std::to_string(t) + " is not finite");
        if (v < 0.0) return refuse(why, where + "se2 of trait " + std::to_string(t) + " is negative");
      }
  }
  slot = std::move(sl);
  sig = std::move(sg);
  cl = clusters_of(cluster, n, family, 1);
  int32_t mm = 0;
  for (int32_t c : cl) mm = std::max(mm, dims[c]);
  if (max_dim) *max_dim = mm;
  return true;
}

bool LgTable::cluster_dims(const char* fn, int limit, int* max_m, std::string& why) const {
  int mm = 0;
  for (int c = 0; c + 1 < (int)cl_off.size(); ++c)
    for (int q = cl_off[c]; q < cl_off[c + 1]; ++q) {
      if (limit > 0 && dims[c] > limit)
        return refuse(why, std::string(fn) + ": family " + std::to_string(cl_fam[q]) + " (cluster " + std::to_string(c) +
                               "): the cluster has more than " + std::to_string(limit) + " variables");
      mm = std::max(mm, (int)dims[c]);
    }
  if (max_m) *max_m = mm;
  return true;
}

std::vector<int32_t> LgTable::loo_tips() const {
  std::vector<int32_t> tips;
  for (int f = 0; f < n_families; ++f)
    if (child_pos[f] < 0 && data_row[f] >= 0 && (child_mask.empty() || child_mask[f] != 0)) tips.push_back(f);
  return tips;
}

void LgTable::impute_list(std::vector<int32_t>& fams, std::vector<unsigned long long>& predicted) const {
  const unsigned long long full = full_mask();
  fams.clear();
  predicted.clear();
  if (child_mask.empty() || parent_mask.empty()) return;   // complete data: nothing is listed
  for (int f = 0; f < n_families; ++f) {
    if (!tip[f]) continue;
    const unsigned long long miss = full & ~child_mask[f];
    if (!miss) continue;
    unsigned long long P = miss;
    for (int k = 0; k < n_parents[f] && k < K; ++k) {
      const unsigned long long mk = parent_mask[(size_t)f * K + k];
      if (!(parent_pos[(size_t)f * K + k] < 0 && mk == full)) P &= mk;   // a cluster parent (not the fixed root)
    }
    fams.push_back(f);
    predicted.push_back(P);
  }
}

}  // namespace pgbp

// The host-side plan of the preorder sweeps over a schedule tree (pgbp_sample_posterior and pgbp_posterior_cov in
// pgbp_sample.hip, pgbp_sample_posterior_sites in pgbp_post_uni.hip): the item of a cluster as the kernels read it, and the one
// walk of the tree that checks it and lists the items by dimension class and by preorder level.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "pgbp_kernels.hpp"

namespace pgbp {

// one cluster of the sweep
struct SampItem {
  int64_t rec_off;   // its record inside a site's belief pool
  int64_t f_off;     // its factor inside a site's factor pool: T' (r x r: T(i, l) at l * r + i), G' (s x r), a (r)
  int64_t x_off;     // its variables inside a (draw, site) of x
  int64_t px_off;    // its parent's
  int32_t cluster, m, r;
  int32_t perm;      // into the index pool: perm[0 .. r) = R, perm[r .. m) = S (positions in the cluster), then the s
                     // positions of S in the parent
};

// The host-side plan of a sweep over schedule tree `tree`, shared by pgbp_sample_posterior and pgbp_posterior_cov: the refusals
// (in the order of the header; `count` is n_draws or n_cols, `buffers` returns the text of a refusal of the call's own pointers
// or an empty string), every cluster's item, the items by dimension class (the factor phase) and by preorder level (the sweeps).
struct SampPlan {
  std::vector<SampItem> by_class, by_level;
  std::vector<int32_t> idx, order, level_off, level_mpad;
  int n_class[3] = {0, 0, 0}, max_m[3] = {0, 0, 0};
  int64_t size = 0, f_stride = 0;
  int nc = 0;
};

template <class Buffers>
inline int sample_plan(pgbp_engine* e, const std::string& fn, int32_t tree, int32_t site_begin, int32_t site_end, int32_t count,
                       const char* count_name, const char* count_unit, Buffers buffers, SampPlan& sp) {
  std::vector<SampItem>&by_class = sp.by_class, &by_level = sp.by_level;
  std::vector<int32_t>&idx = sp.idx, &order = sp.order, &level_off = sp.level_off, &level_mpad = sp.level_mpad;
  int* n_class = sp.n_class;
  int* max_m = sp.max_m;
  int64_t &size = sp.size, &f_stride = sp.f_stride;
  int& nc = sp.nc;
  {
    const Plan& p = *engine_peek(e).plan;
    nc = p.n_clusters;
    if (p.trees.empty()) return engine_fail(e, PGBP_ERR_STATE, fn + "no schedule: call pgbp_set_schedule first");
    if (tree < 0 || tree >= (int)p.trees.size())
      return engine_fail(e, PGBP_ERR_INVALID, fn + "schedule tree " + std::to_string(tree) + " out of range (the schedule has " +
                                                  std::to_string(p.trees.size()) + " trees)");
    const Tree& T = p.trees[tree];
    const int ne = (int)T.pa.size();
    // the sweep is the chain rule of a tree-structured joint: every sepset must be an edge of the tree, every cluster on it
    std::vector<int32_t> depth(nc, -1), par_edge(nc, -1);
    bool spans = p.n_sepsets == nc - 1 && ne == nc - 1;
    if (spans) {
      const int root = ne > 0 ? T.pa[0] : 0;
      depth[root] = 0;
      order.push_back(root);
      for (int j = 0; j < ne && spans; ++j) {
        const int pa = T.pa[j], ch = T.ch[j];
        if (depth[pa] < 0 || depth[ch] >= 0) { spans = false; break; }
        depth[ch] = depth[pa] + 1;
        par_edge[ch] = j;
        order.push_back(ch);
      }
    }
    if (!spans)
      return engine_fail(e, PGBP_ERR_INVALID, fn + "schedule tree " + std::to_string(tree) + " (" + std::to_string(ne) +
                                                  " edges) does not span the " + std::to_string(nc) + " clusters, or the graph has a cycle (" +
                                                  std::to_string(p.n_sepsets) + " sepsets): the sweep is exact on a clique tree only");
    for (int c = 0; c < nc; ++c)
      if (p.dims[c] > kLdsMaxDim)
        return engine_fail(e, PGBP_ERR_INVALID, fn + "belief " + std::to_string(c) + " has " + std::to_string(p.dims[c]) +
                                                    " variables, more than the " + std::to_string(kLdsMaxDim) +
                                                    " the moments kernels take");
    if (count < 1)
      return engine_fail(e, PGBP_ERR_INVALID, fn + count_name + " = " + std::to_string(count) + ", at least one " + count_unit + " is needed");
    if (site_begin < 0 || site_end < site_begin || site_end > p.n_sites)
      return engine_fail(e, PGBP_ERR_INVALID, fn + "site range [" + std::to_string(site_begin) + ", " + std::to_string(site_end) +
                                                  ") outside the engine's " + std::to_string(p.n_sites) + " sites");
    const std::string refused = buffers();
    if (!refused.empty()) return engine_fail(e, PGBP_ERR_INVALID, fn + refused);
    // items: where every cluster's variables sit in x, its split into R and S, its factor
    std::vector<int64_t> x_off(nc + 1, 0);
    for (int c = 0; c < nc; ++c) x_off[c + 1] = x_off[c] + p.dims[c];
    size = x_off[nc];
    std::vector<SampItem> all(nc);
    int max_depth = 0;
    for (int c = 0; c < nc; ++c) {
      const int m = p.dims[c];
      SampItem it{p.boff[c], f_stride, x_off[c], 0, c, m, m, (int32_t)idx.size()};
      std::vector<char> in_s(m, 0);
      const int32_t *cs = nullptr, *ps = nullptr;
      int s = 0;
      if (par_edge[c] >= 0) {
        const int k = T.sep[par_edge[c]], pa = T.pa[par_edge[c]];
        const int side = p.sepset_clusters[2 * k] == c ? 0 : 1;
        if (p.sepset_clusters[2 * k + side] != c || p.sepset_clusters[2 * k + 1 - side] != pa)
          return engine_fail(e, PGBP_ERR_INVALID, fn + "edge " + std::to_string(par_edge[c]) + " of schedule tree " +
                                                      std::to_string(tree) + " is not sepset " + std::to_string(k));
        cs = p.scope_idx.data() + p.scope_off[2 * k + side];
        ps = p.scope_idx.data() + p.scope_off[2 * k + 1 - side];
        s = (int)(p.scope_off[2 * k + side + 1] - p.scope_off[2 * k + side]);
        it.px_off = x_off[pa];
      }
      for (int j = 0; j < s; ++j) in_s[cs[j]] = 1;
      for (int v = 0; v < m; ++v)
        if (!in_s[v]) idx.push_back(v);
      for (int j = 0; j < s; ++j) idx.push_back(cs[j]);
      for (int j = 0; j < s; ++j) idx.push_back(ps[j]);
      it.r = m - s;
      f_stride += (int64_t)it.r * (m + 1);
      all[c] = it;
      max_depth = std::max(max_depth, depth[c]);
    }
    for (int cl = 0; cl < 3; ++cl)
      for (int c = 0; c < nc; ++c) {
        const int m = all[c].m;
        if (m == 0 || (m <= 16 ? 0 : (m <= 64 ? 1 : 2)) != cl) continue;
        by_class.push_back(all[c]);
        ++n_class[cl];
        max_m[cl] = std::max(max_m[cl], m);
      }
    // the preorder by levels (a cluster's level = its depth in the schedule tree: the level of the preorder message into it)
    std::vector<std::vector<int32_t>> lv(max_depth + 1);
    for (int c : order)
      if (all[c].m > 0) lv[depth[c]].push_back(c);
    level_off.push_back(0);
    for (auto& l : lv) {
      if (l.empty()) continue;
      int mp = 0;
      for (int c : l) { by_level.push_back(all[c]); mp = std::max(mp, all[c].m); }
      level_off.push_back((int32_t)by_level.size());
      level_mpad.push_back(mp);
    }
  }
  return PGBP_OK;
}

}  // namespace pgbp

// pgbp_sitemiss_host.hpp: the checks and the packing of a per-site mask, host only.
#include "pgbp_sitemiss_host.hpp"

#include <algorithm>

namespace pgbp {

static bool refuse(std::string& why, const std::string& msg) {
  why = msg;
  return false;
}

bool site_missing_pack(const SiteMissTable& T, const uint8_t* missing, SiteMissPack& out, std::string& why) {
  const char* fn = "pgbp_lg_set_site_missing: ";
  if (!missing) return refuse(why, std::string(fn) + "no mask");
  const int ns = T.n_sites, nr = T.n_rows, nf = T.n_families;
  // the tip family of a row (the first in table order), -1: none; and the tips the static mask leaves observed
  // (tip families may share a data row: the kernels test by row, so a masked row hides every one of them -- row_live counts
  // the statically observed tip families of a row, and a site's observed tips are counted in families, not rows)
  std::vector<int32_t> row_fam((size_t)std::max(0, nr), -1), row_live((size_t)std::max(0, nr), 0);
  int n_static = 0;
  for (int f = 0; f < nf; ++f) {
    if (!T.tip[f]) continue;
    const int r = T.data_row[f];
    if (r < 0 || r >= nr) continue;
    if (row_fam[r] < 0) row_fam[r] = f;
    if (!T.child_mask || (T.child_mask[f] & 1ull)) {
      ++n_static;
      ++row_live[r];
    }
  }
  SiteMissPack P;
  P.W = (ns + 63) / 64;
  P.words.assign((size_t)std::max(0, nr) * (size_t)P.W, 0);
  std::vector<char> row_hit((size_t)std::max(0, nr), 0);
  for (int s = 0; s < ns; ++s) {
    int masked = 0, hidden = 0;   // masked rows, and the tip families they hide
    for (int r = 0; r < nr; ++r) {
      if (!missing[(size_t)s * nr + r]) continue;
      const std::string where = std::string(fn) + "site " + std::to_string(s) + ", row " + std::to_string(r) + ": ";
      const int f = row_fam[r];
      if (f < 0) return refuse(why, where + "the row belongs to no tip family (child_pos < 0, a data row and a parent edge)");
      if (T.child_mask && !(T.child_mask[f] & 1ull))
        return refuse(why, where + "the tip (family " + std::to_string(f) + ") is already missing at every site by the set-up's child_mask");
      P.words[(size_t)r * P.W + (s >> 6)] |= 1ull << (s & 63);
      row_hit[r] = 1;
      ++masked;
      hidden += row_live[r];
    }
    if (masked > 0 && hidden >= n_static)
      return refuse(why, std::string(fn) + "site " + std::to_string(s) + " is left with no observed tip");
    P.count += masked;
  }
  for (int f = 0; f < nf; ++f)   // (every tip family that reads a masked row: the kernels test by row)
    if (T.tip[f] && T.data_row[f] >= 0 && T.data_row[f] < nr && row_hit[T.data_row[f]]) {
      P.fams.push_back(f);
      P.cl.push_back(T.cluster[f]);
    }
  std::sort(P.cl.begin(), P.cl.end());
  P.cl.erase(std::unique(P.cl.begin(), P.cl.end()), P.cl.end());
  out = std::move(P);
  return true;
}

void site_missing_unpack(const SiteMissPack& P, int32_t n_sites, int32_t n_rows, uint8_t* missing) {
  for (int s = 0; s < n_sites; ++s)
    for (int r = 0; r < n_rows; ++r) missing[(size_t)s * n_rows + r] = site_missing_test(P, r, s) ? 1 : 0;
}

}  // namespace pgbp

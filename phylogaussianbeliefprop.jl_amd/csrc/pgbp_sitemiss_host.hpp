// Host side of pgbp_lg_set_site_missing (include/pgbp.h): the checks of a per-site mask against the family table and its
// packing into the words the kernels read.  Plain C++ without the runtime, so that a stand-alone program can run it under a
// host sanitizer (tests/site_missing_check.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace pgbp {

// what the setter keeps of an accepted mask
struct SiteMissPack {
  int32_t W = 0;                      // words per row: ceil(n_sites / 64)
  std::vector<unsigned long long> words;   // [n_rows][W]: bit (s & 63) of word s >> 6 = site s
  std::vector<int32_t> fams;          // the tip families masked at some site, in family order
  std::vector<int32_t> cl;            // the clusters that hold one of them, sorted, each once
  int64_t count = 0;                  // masked (row, site) pairs
};

// The table as plain arrays: per family its cluster, data row (-1: none) and whether it is a tip family (child_pos < 0, a data
// row, a parent edge); child_mask may be null (complete data), else bit 0 of child_mask[f] = the trait is observed at all.
struct SiteMissTable {
  int32_t n_sites, n_rows, n_families;
  const int32_t *cluster, *data_row;
  const char* tip;
  const unsigned long long* child_mask;
};

// missing [n_sites][n_rows], nonzero = not observed.  false with the message in `why` ("pgbp_lg_set_site_missing: ...", the
// entry named) and `out` untouched for: a set entry at a row that belongs to no tip family, at a row whose tip the static
// child_mask already skips, and a site left with no observed tip.
bool site_missing_pack(const SiteMissTable& T, const uint8_t* missing, SiteMissPack& out, std::string& why);

// the mask back as bytes [n_sites][n_rows] (0 / 1)
void site_missing_unpack(const SiteMissPack& P, int32_t n_sites, int32_t n_rows, uint8_t* missing);

// is (row, site) masked?
inline bool site_missing_test(const SiteMissPack& P, int32_t row, int32_t site) {
  return !P.words.empty() && ((P.words[(size_t)row * P.W + (site >> 6)] >> (site & 63)) & 1u);
}

}  // namespace pgbp

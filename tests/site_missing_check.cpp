// Host side of pgbp_lg_set_site_missing (csrc/pgbp_sitemiss_host.cpp: the checks of a per-site mask and its packing into
// words) on a small table, the refused masks included.  Built by tests/test_site_missing_cpu.py with the host compiler under
// the address and undefined-behaviour sanitizers and run as a process of its own; prints "ok <what>" per check and
// "site missing ok" at the end.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pgbp_sitemiss_host.hpp"

using namespace pgbp;

static void check(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED %s\n", what);
    std::exit(1);
  }
  std::printf("ok %s\n", what);
}

int main() {
  // 7 families: a root prior, two internal nodes, four tips (rows 2, 0, 3, 1) in clusters 1 .. 4; row 4 belongs to no family
  const int ns = 65, nr = 5, nf = 7;
  const std::vector<int32_t> cluster{0, 0, 5, 1, 2, 3, 4}, row{-1, -1, -1, 2, 0, 3, 1};
  const std::vector<char> tip{0, 0, 0, 1, 1, 1, 1};
  const SiteMissTable T{ns, nr, nf, cluster.data(), row.data(), tip.data(), nullptr};
  std::vector<uint8_t> m((size_t)ns * nr, 0);
  auto at = [&](int s, int r) -> uint8_t& { return m[(size_t)s * nr + r]; };
  at(0, 2) = at(63, 2) = at(64, 2) = 1;
  at(7, 0) = 9;   // (any nonzero value)
  at(7, 3) = 1;
  SiteMissPack P;
  std::string why;
  check(site_missing_pack(T, m.data(), P, why) && P.W == 2 && P.words.size() == (size_t)nr * 2 && P.count == 5, "words of 65 sites");
  check(P.words[2 * 2] == ((1ull << 0) | (1ull << 63)) && P.words[2 * 2 + 1] == 1ull && P.words[0] == (1ull << 7) &&
            P.words[3 * 2] == (1ull << 7) && P.words[1 * 2] == 0 && P.words[4 * 2] == 0, "lanes 0, 63 and site 64");
  std::vector<uint8_t> back((size_t)ns * nr, 7);
  site_missing_unpack(P, ns, nr, back.data());
  bool same = true;
  for (size_t i = 0; i < m.size(); ++i) same = same && (back[i] == (m[i] ? 1 : 0));
  check(same && site_missing_test(P, 2, 64) && !site_missing_test(P, 2, 62), "round trip");
  check(P.fams == std::vector<int32_t>({3, 4, 5}) && P.cl == std::vector<int32_t>({1, 2, 3}), "families and clusters");
  // the refused masks leave the output untouched and name the entry
  const SiteMissPack keep = P;
  std::vector<uint8_t> bad = m;
  bad[(size_t)9 * nr + 4] = 1;
  check(!site_missing_pack(T, bad.data(), P, why) && why.find("site 9, row 4") != std::string::npos &&
            why.find("no tip family") != std::string::npos, "row without a tip");
  const std::vector<unsigned long long> cm{1, 1, 1, 1, 0, 1, 1};   // the tip of row 0 is statically missing
  const SiteMissTable Tm{ns, nr, nf, cluster.data(), row.data(), tip.data(), cm.data()};
  check(!site_missing_pack(Tm, m.data(), P, why) && why.find("site 7, row 0") != std::string::npos &&
            why.find("family 4") != std::string::npos, "statically missing tip");
  bad = m;
  for (int r = 0; r < 4; ++r) bad[(size_t)30 * nr + r] = 1;
  check(!site_missing_pack(T, bad.data(), P, why) && why.find("site 30") != std::string::npos &&
            why.find("no observed tip") != std::string::npos, "site with nothing observed");
  bad = m;   // with the static mask three tips are left: masking those three is refused as well
  bad[(size_t)7 * nr + 0] = 0;
  bad[(size_t)31 * nr + 1] = bad[(size_t)31 * nr + 2] = bad[(size_t)31 * nr + 3] = 1;
  check(!site_missing_pack(Tm, bad.data(), P, why) && why.find("site 31") != std::string::npos, "nothing observed under the static mask");
  check(!site_missing_pack(T, nullptr, P, why), "no mask");
  check(P.W == keep.W && P.words == keep.words && P.fams == keep.fams && P.cl == keep.cl && P.count == keep.count, "output untouched");
  {  // two tip families share row 2: masking rows 2 and 0 leaves one tip (row 1), masking 2, 0 and 1 none -- counted in families
    const std::vector<int32_t> row2{-1, -1, -1, 2, 0, 2, 1};
    const SiteMissTable Ts{ns, nr, nf, cluster.data(), row2.data(), tip.data(), nullptr};
    std::vector<uint8_t> two((size_t)ns * nr, 0);
    two[(size_t)5 * nr + 2] = two[(size_t)5 * nr + 0] = 1;
    check(site_missing_pack(Ts, two.data(), P, why) && P.fams == std::vector<int32_t>({3, 4, 5}) && P.count == 2, "shared row: both families listed");
    two[(size_t)5 * nr + 1] = 1;
    check(!site_missing_pack(Ts, two.data(), P, why) && why.find("site 5") != std::string::npos, "shared row: nothing observed");
    P = keep;
  }
  std::vector<uint8_t> none((size_t)ns * nr, 0);
  check(site_missing_pack(T, none.data(), P, why) && P.count == 0 && P.fams.empty() && P.cl.empty(), "empty mask");
  const SiteMissTable T0{0, 0, 0, nullptr, nullptr, nullptr, nullptr};
  check(site_missing_pack(T0, none.data(), P, why) && P.W == 0 && P.words.empty(), "empty table");
  std::printf("site missing ok\n");
  return 0;
}

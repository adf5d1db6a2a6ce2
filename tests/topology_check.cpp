// Host side of pgbp_lg_set_topology (csrc/pgbp_topology.cpp: validation and levelling) on a few tables, the invalid ones
// included.  Built by tests/test_simulate_cpu.py with the host compiler under the address and undefined-behaviour sanitizers and
// run as a process of its own; prints "ok <what>" per check and "topology ok" at the end.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pgbp_topology.hpp"

using pgbp::lg_topology_levels;

static void check(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED %s\n", what);
    std::exit(1);
  }
  std::printf("ok %s\n", what);
}

int main() {
  std::vector<int32_t> off, fam;
  int32_t improper = 7;
  std::string err;
  {  // a root prior, two children, a hybrid of the two, a tip below the hybrid; K = 2
    const std::vector<int32_t> np{0, 1, 1, 2, 1}, pf{-9, -9, 0, -9, 0, -9, 1, 2, 3, -9};
    check(lg_topology_levels(5, 2, np.data(), pf.data(), off, fam, &improper, err), "random root");
    check(off == std::vector<int32_t>({0, 1, 3, 4, 5}) && fam == std::vector<int32_t>({0, 1, 2, 3, 4}) && improper == -1, "random root levels");
  }
  {  // a fixed root: level 0 is empty; a hybrid one of whose parents is the root; families of a level in index order
    const std::vector<int32_t> np{1, 1, 2, 1}, pf{-1, 0, -1, 0, 0, -1, 1, 0};
    check(lg_topology_levels(4, 2, np.data(), pf.data(), off, fam, &improper, err), "fixed root");
    check(off == std::vector<int32_t>({0, 0, 2, 4}) && fam == std::vector<int32_t>({0, 1, 2, 3}) && improper == -1, "fixed root levels");
  }
  {  // an improper root is valid here (the sweep refuses it) and its first entry is reported
    const std::vector<int32_t> np{1, 1, 1}, pf{-2, -2, 0};
    check(lg_topology_levels(3, 1, np.data(), pf.data(), off, fam, &improper, err) && improper == 0, "improper root");
    check(off == std::vector<int32_t>({0, 0, 2, 3}), "improper root levels");
  }
  {  // a deep chain: levels out of index order are grouped by counting
    const std::vector<int32_t> np{0, 1, 1, 1, 1}, pf{0, 0, 1, 0, 2};
    check(lg_topology_levels(5, 1, np.data(), pf.data(), off, fam, &improper, err), "chain and bush");
    check(off == std::vector<int32_t>({0, 1, 3, 4, 5}) && fam == std::vector<int32_t>({0, 1, 3, 2, 4}), "chain and bush levels");
  }
  {  // the invalid ones leave the outputs untouched and name the entry
    const std::vector<int32_t> keep_off = off, keep_fam = fam;
    const int32_t keep_improper = improper;
    const std::vector<int32_t> np{0, 1, 2};
    const std::vector<int32_t> self{0, 0, 0, 0, 0, 2}, late{0, 0, 2, 0, 0, 1}, big{0, 0, 0, 0, 0, 3}, low{0, 0, -3, 0, 0, 1};
    check(!lg_topology_levels(3, 2, np.data(), self.data(), off, fam, &improper, err) && err.find("family 2, parent 1") == 0, "parent = the family itself");
    check(!lg_topology_levels(3, 2, np.data(), late.data(), off, fam, &improper, err) && err.find("family 1, parent 0") == 0, "parent after its child");
    check(!lg_topology_levels(3, 2, np.data(), big.data(), off, fam, &improper, err) && err.find("family 2, parent 1") == 0 &&
              err.find("out of range") != std::string::npos, "parent beyond the table");
    check(!lg_topology_levels(3, 2, np.data(), low.data(), off, fam, &improper, err) && err.find("family 1, parent 0") == 0, "parent below -2");
    const std::vector<int32_t> np_bad{0, 3, 1};
    check(!lg_topology_levels(3, 2, np_bad.data(), self.data(), off, fam, &improper, err), "more parents than K");
    check(!lg_topology_levels(3, 2, nullptr, self.data(), off, fam, &improper, err), "no table");
    check(off == keep_off && fam == keep_fam && improper == keep_improper, "outputs untouched");
  }
  {  // entries beyond n_parents are not read; an empty table
    const std::vector<int32_t> np{0, 1}, pf{99, -77, 0, 1234};
    check(lg_topology_levels(2, 2, np.data(), pf.data(), off, fam, &improper, err), "padding ignored");
    check(lg_topology_levels(0, 1, nullptr, nullptr, off, fam, &improper, err) && off == std::vector<int32_t>({0}) && fam.empty(), "empty table");
  }
  std::printf("topology ok\n");
  return 0;
}

// Host side of pgbp_lg_optimum_scan_sites (csrc/pgbp_optscan_host.cpp: child lists, heights, the families by height, the
// single-parent check, the scratch of a site) on a few tables, the invalid ones included.  Built by
// tests/test_optimum_scan_cpu.py with the host compiler under the address and undefined-behaviour sanitizers and run as a
// process of its own; prints "ok <what>" per check and "optimum scan ok" at the end.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pgbp_optscan_host.hpp"

using pgbp::OptScanPlan;
using pgbp::optscan_plan_build;
using pgbp::optscan_plan_single_parents;
typedef std::vector<int32_t> V;

static void check(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED %s\n", what);
    std::exit(1);
  }
  std::printf("ok %s\n", what);
}

int main() {
  OptScanPlan P;
  std::string err;
  {  // a fixed root with two children, the first with a cherry below: ((2,3)0,1)
    const V np{1, 1, 1, 1}, pf{-1, -1, 0, 0};
    check(optscan_plan_build(4, 1, np.data(), pf.data(), P, err) && P.built && P.multi == -1, "fixed root");
    check(P.child_off == V({0, 2, 2, 2, 2}) && P.child_fam == V({2, 3}), "fixed root children");
    check(P.height == V({1, 0, 0, 0}) && P.height_off == V({0, 3, 4}) && P.height_fam == V({1, 2, 3, 0}) && P.n_heights() == 2,
          "fixed root heights");
    check(optscan_plan_single_parents(P, np.data(), err), "a tree");
  }
  {  // a root prior (family 0), a caterpillar below it: heights out of index order, children in index order
    const V np{0, 1, 1, 1, 1, 1, 1}, pf{-9, 0, 0, 2, 2, 4, 4};
    check(optscan_plan_build(7, 1, np.data(), pf.data(), P, err), "caterpillar");
    check(P.child_off == V({0, 2, 2, 4, 4, 6, 6, 6}) && P.child_fam == V({1, 2, 3, 4, 5, 6}), "caterpillar children");
    check(P.height == V({3, 0, 2, 0, 1, 0, 0}) && P.height_off == V({0, 4, 5, 6, 7}) && P.height_fam == V({1, 3, 5, 6, 4, 2, 0}),
          "caterpillar heights");
  }
  {  // an improper root and a trifurcation; a breadth-first table
    const V np{1, 1, 1, 1, 1}, pf{-2, -2, 0, 0, 0};
    check(optscan_plan_build(5, 1, np.data(), pf.data(), P, err), "improper root");
    check(P.child_off == V({0, 3, 3, 3, 3, 3}) && P.child_fam == V({2, 3, 4}) && P.height == V({1, 0, 0, 0, 0}), "trifurcation");
  }
  {  // a hybrid: accepted by the plan, named by the check; entries beyond n_parents are not read
    const V np{0, 1, 1, 2, 1}, pf{-9, 77, 0, -5, 0, 1234, 1, 2, 3, -9};
    check(optscan_plan_build(5, 2, np.data(), pf.data(), P, err) && P.multi == 3, "hybrid accepted");
    check(!optscan_plan_single_parents(P, np.data(), err) && err.find("family 3 has 2 parents") == 0, "hybrid named");
  }
  {  // the invalid ones clear the plan and never index outside
    const V np{0, 1, 1}, late{0, 2, 0}, self{0, 0, 2}, np_bad{0, 3, 1}, ok{0, 0, 0};
    check(!optscan_plan_build(3, 1, np.data(), late.data(), P, err) && !P.built && err.find("family 1, parent 0") == 0, "parent after its child");
    check(!optscan_plan_build(3, 1, np.data(), self.data(), P, err) && err.find("family 2, parent 0") == 0, "parent = the family itself");
    check(!optscan_plan_build(3, 1, np_bad.data(), ok.data(), P, err), "more parents than K");
    check(!optscan_plan_build(3, 1, nullptr, ok.data(), P, err) && !optscan_plan_build(3, 0, np.data(), ok.data(), P, err), "no table");
    check(P.child_off.empty() && P.height_fam.empty() && P.n_heights() == 0, "plan cleared");
  }
  {  // an empty table; clear
    check(optscan_plan_build(0, 1, nullptr, nullptr, P, err) && P.built && P.child_off == V({0}) && P.n_heights() == 0, "empty table");
    P.clear();
    check(!P.built, "clear");
  }
  {  // the scratch of a site: four state rows, the tables, the candidates and the fold's records
    check(pgbp::optscan_per_site(130, 0, true, 3, 3) == 130 * 5 + 6 + 3, "scratch, top only");
    check(pgbp::optscan_per_site(130, 3, false, 3, 3) == 130 * 7 + 3, "scratch, tables only");
    check(pgbp::optscan_per_site(39998, 0, false, 625, 625) * 256 > ((int64_t)32 << 20), "scratch, 39 998 families above the default");
  }
  std::printf("optimum scan ok\n");
  return 0;
}

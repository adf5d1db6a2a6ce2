// Host side of pgbp_lg_set_clade_shifts_sites (csrc/pgbp_cladeshift_host.cpp: the preorder ranks of the family tree, the checks
// of a setting, the clusters its correction visits) on a few tables, the invalid ones included.  Built by
// tests/test_clade_shift_cpu.py with the host compiler under the address and undefined-behaviour sanitizers and run as a
// process of its own; prints "ok <what>" per check and "clade shift ok" at the end.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "pgbp_cladeshift_host.hpp"

using pgbp::CladePlan;
using pgbp::clade_clusters;
using pgbp::clade_plan_build;
using pgbp::clade_setting_check;
using pgbp::clade_values_check;
typedef std::vector<int32_t> V;
typedef std::vector<double> D;

static void check(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED %s\n", what);
    std::exit(1);
  }
  std::printf("ok %s\n", what);
}

// membership by the ranks against membership by walking up the parents
static bool membership_agrees(const CladePlan& P, const V& np, const V& pf, int K) {
  const int nf = (int)P.pre.size();
  std::vector<char> seen(nf, 0);
  for (int f = 0; f < nf; ++f) {
    if (P.pre[f] < 0 || P.pre[f] >= nf || seen[P.pre[f]]) return false;   // a permutation
    seen[P.pre[f]] = 1;
  }
  for (int v = 0; v < nf; ++v)
    for (int f = 0; f < nf; ++f) {
      bool in = false;
      for (int a = f; a >= 0; a = (np[a] >= 1 && pf[(size_t)a * K] >= 0) ? pf[(size_t)a * K] : -1)
        if (a == v) { in = true; break; }
      if (in != (P.pre[v] <= P.pre[f] && P.pre[f] <= P.last[v])) return false;
    }
  return true;
}

int main() {
  CladePlan P;
  std::string err;
  {  // a fixed root with two children, the first with a cherry below: ((2,3)0,1): a forest of two trees
    const V np{1, 1, 1, 1}, pf{-1, -1, 0, 0};
    check(clade_plan_build(4, 1, np.data(), pf.data(), P, err) && P.built, "fixed root");
    check(P.pre == V({0, 3, 1, 2}) && P.last == V({2, 3, 1, 2}), "fixed root ranks");
    check(membership_agrees(P, np, pf, 1), "fixed root membership");
  }
  {  // a root prior (family 0) and a caterpillar in a breadth-first-like order: ranks differ from the indices
    const V np{0, 1, 1, 1, 1, 1, 1}, pf{-9, 0, 0, 2, 2, 4, 4};
    check(clade_plan_build(7, 1, np.data(), pf.data(), P, err), "caterpillar");
    check(P.pre == V({0, 1, 2, 3, 4, 5, 6}) && P.last == V({6, 1, 6, 3, 6, 5, 6}), "caterpillar ranks");
    check(membership_agrees(P, np, pf, 1), "caterpillar membership");
  }
  {  // a balanced tree given level by level: ((3,4)1,(5,6)2) under a root prior 0
    const V np{0, 1, 1, 1, 1, 1, 1}, pf{0, 0, 0, 1, 1, 2, 2};
    check(clade_plan_build(7, 1, np.data(), pf.data(), P, err), "levels");
    check(P.pre == V({0, 1, 4, 2, 3, 5, 6}) && P.last == V({6, 3, 6, 2, 3, 5, 6}), "levels ranks");
    check(membership_agrees(P, np, pf, 1), "levels membership");
    // settings on it: 2 slots x 3 sites
    const V cl{0, 1, 2, 3, 4, 5, 6};
    const D d{0.5, 0.0, -1.0, 2.0, 0.0, 0.0};
    {
      const V fam{1, -1, 3, 5, -1, -1};   // site 0: clade(1), tip 5; site 1: none; site 2: tip 3
      check(clade_setting_check(P, np.data(), 2, 3, fam.data(), d.data(), err), "setting accepted");
      V out;
      clade_clusters(P, cl.data(), 2, 3, fam.data(), out);
      check(out == V({1, 3, 4, 5}), "clusters: the union of the intervals");
      const V two{0, 0, 1, 1, 1, 2, 2};   // two families per cluster
      clade_clusters(P, two.data(), 2, 3, fam.data(), out);
      check(out == V({0, 1, 2}), "clusters: each once, sorted");
    }
    {
      const V none{-1, -1, -1, -1, -1, -1};
      V out{7};
      check(clade_setting_check(P, np.data(), 2, 3, none.data(), d.data(), err), "all slots empty");
      clade_clusters(P, cl.data(), 2, 3, none.data(), out);
      check(out.empty(), "no cluster without a used slot");
    }
    {
      const V nested{1, -1, -1, 3, -1, -1};   // clade(3) inside clade(1) at site 0
      V out;
      check(clade_setting_check(P, np.data(), 2, 3, nested.data(), d.data(), err), "nested accepted");
      clade_clusters(P, cl.data(), 2, 3, nested.data(), out);
      check(out == V({1, 3, 4}), "nested clusters");
    }
    {
      const V range{1, -1, 7, -1, -1, -1}, neg{1, -2, -1, -1, -1, -1}, root{1, -1, -1, -1, 0, -1}, twice{1, -1, 4, -1, -1, 4};
      check(!clade_setting_check(P, np.data(), 2, 3, range.data(), d.data(), err) && err.find("family 7 out of range") != std::string::npos,
            "family out of range");
      check(!clade_setting_check(P, np.data(), 2, 3, neg.data(), d.data(), err) && err.find("family -2 out of range") != std::string::npos,
            "negative family");
      check(!clade_setting_check(P, np.data(), 2, 3, root.data(), d.data(), err) && err.find("root-prior") != std::string::npos &&
                err.find("site 1") != std::string::npos, "root-prior family");
      check(!clade_setting_check(P, np.data(), 2, 3, twice.data(), d.data(), err) &&
                err.find("family 4 appears twice at site 2") != std::string::npos, "duplicate names site and family");
    }
    {
      const V fam{1, -1, 3, 5, -1, -1};
      D bad = d;
      bad[3] = std::numeric_limits<double>::quiet_NaN();
      check(!clade_setting_check(P, np.data(), 2, 3, fam.data(), bad.data(), err) && err.find("not finite") != std::string::npos &&
                err.find("slot 1 at site 0") != std::string::npos, "delta not finite");
      check(!clade_values_check(2, 3, fam.data(), bad.data(), err) && err.find("family 5") != std::string::npos, "update: not finite");
      bad[3] = 2.0;
      bad[1] = std::numeric_limits<double>::infinity();   // an empty slot: not read
      check(clade_setting_check(P, np.data(), 2, 3, fam.data(), bad.data(), err) && clade_values_check(2, 3, fam.data(), bad.data(), err),
            "the delta of an empty slot is not read");
      check(!clade_setting_check(P, np.data(), 2, 3, nullptr, d.data(), err) && !clade_setting_check(P, np.data(), -1, 3, fam.data(), d.data(), err),
            "no table, negative slots");
      check(clade_setting_check(P, np.data(), 0, 3, nullptr, nullptr, err), "no slots");
    }
  }
  {  // a trifurcation under an improper root; a hybrid: the first parent is read
    const V np{1, 1, 1, 1, 1}, pf{-2, -2, 0, 0, 0};
    check(clade_plan_build(5, 1, np.data(), pf.data(), P, err) && P.pre == V({0, 4, 1, 2, 3}) && P.last == V({3, 4, 1, 2, 3}), "trifurcation");
    const V nph{0, 1, 1, 2, 1}, pfh{-9, 77, 0, -5, 0, 1234, 1, 2, 3, -9};
    check(clade_plan_build(5, 2, nph.data(), pfh.data(), P, err) && P.built, "hybrid accepted");
  }
  {  // the invalid ones clear the plan and never index outside
    const V np{0, 1, 1}, late{0, 2, 0}, self{0, 0, 2}, np_bad{0, 3, 1}, ok{0, 0, 0};
    check(!clade_plan_build(3, 1, np.data(), late.data(), P, err) && !P.built && err.find("family 1, parent 0") == 0, "parent after its child");
    check(!clade_plan_build(3, 1, np.data(), self.data(), P, err) && err.find("family 2, parent 0") == 0, "parent = the family itself");
    check(!clade_plan_build(3, 1, np_bad.data(), ok.data(), P, err), "more parents than K");
    check(!clade_plan_build(3, 1, nullptr, ok.data(), P, err) && !clade_plan_build(3, 0, np.data(), ok.data(), P, err), "no table");
    check(P.pre.empty() && P.last.empty(), "plan cleared");
    const V fam{1};
    const D d{1.0};
    check(!clade_setting_check(P, np.data(), 1, 1, fam.data(), d.data(), err) && err == "no topology", "setting without a plan");
    V out{3};
    clade_clusters(P, ok.data(), 1, 1, fam.data(), out);
    check(out.empty(), "clusters without a plan");
  }
  {  // an empty table
    check(clade_plan_build(0, 1, nullptr, nullptr, P, err) && P.built && P.pre.empty(), "empty table");
    P.clear();
    check(!P.built, "clear");
  }
  std::printf("clade shift ok\n");
  return 0;
}

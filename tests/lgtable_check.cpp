// The host side of the family table (csrc/pgbp_lgtable.cpp) on the tables tests/test_lgtable_cpu.py writes: it reads a script of
// whitespace-separated words and prints one line per answer, which the test compares with answers stated in numpy.  Built by
// that test with the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own.
//   table p K n_rates n_rows n_families n_clusters n_sites max_dim, then twelve arrays "n v1 .. vn" (n = -1: a null pointer):
//         dims cluster n_parents child_pos data_row parent_pos length gamma color data child_mask parent_mask
//   dims limit | edges <length> <gamma> | data fn site_begin site_end values <data> | shifts n per_site <edge> <value>
//   noise n per_site <family> <scale> <sigma_e> <se2>                                        (<x>: an array as above)
// A refusal prints "<command> refused <message>"; the last line is "lgtable ok".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <type_traits>
#include <vector>

#include "pgbp_lgtable.hpp"

using pgbp::LgTable;

static std::ifstream in;

template <class T>
static T word() {
  T v{};
  if (!(in >> v)) {
    std::printf("FAILED: the script ends inside a command\n");
    std::exit(2);
  }
  return v;
}
static double real() { return std::strtod(word<std::string>().c_str(), nullptr); }   // ("nan" included)

// an array "n v1 .. vn"; null: n was -1
template <class T>
struct Arr {
  std::vector<T> v;
  bool null = false;
  const T* ptr() const { return null ? nullptr : v.data(); }
};
template <class T>
static Arr<T> arr() {
  Arr<T> a;
  const long n = word<long>();
  a.null = n < 0;
  for (long i = 0; i < n; ++i) {
    if constexpr (std::is_same<T, double>::value) a.v.push_back(real());
    else a.v.push_back(word<T>());
  }
  if (!a.null) a.v.reserve(a.v.size() + 1);   // (data() of an empty array is not null either)
  return a;
}

template <class V>
static void line(const char* name, const V& v) {
  std::printf("%s", name);
  for (const auto& x : v) {
    if constexpr (std::is_same<typename V::value_type, double>::value) std::printf(" %.17g", x);
    else std::printf(" %lld", (long long)x);
  }
  std::printf("\n");
}
static void masks(const char* name, const std::vector<unsigned long long>& v) {
  std::printf("%s", name);
  for (unsigned long long x : v) std::printf(" %llu", x);
  std::printf("\n");
}

static void print_simple(const LgTable& T) {
  std::printf("simple %zu\n", T.simple.size());
  for (size_t c = 0; c < T.simple.size(); ++c) {
    const pgbp::LgSimpleFam& r = T.simple[c];
    std::printf("record %d %d %d %d %d %.17g %.17g %d\n", r.np, r.cpos, r.ppos, r.row, r.color, r.length, r.gamma, T.simple_fam[c]);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  in.open(argv[1]);
  LgTable T;
  std::string cmd, why;
  while (in >> cmd) {
    why.clear();
    if (cmd == "table") {
      pgbp_lg_families f{};
      f.p = word<int32_t>();
      f.max_parents = word<int32_t>();
      f.n_rates = word<int32_t>();
      f.n_rows = word<int32_t>();
      f.n_families = word<int32_t>();
      const int32_t nc = word<int32_t>(), n_sites = word<int32_t>(), max_dim = word<int32_t>();
      const Arr<int32_t> dims = arr<int32_t>(), cluster = arr<int32_t>(), np = arr<int32_t>(), cpos = arr<int32_t>(),
                         row = arr<int32_t>(), ppos = arr<int32_t>();
      const Arr<double> length = arr<double>(), gamma = arr<double>();
      const Arr<int32_t> color = arr<int32_t>();
      const Arr<double> data = arr<double>();
      const Arr<uint64_t> cm = arr<uint64_t>(), pm = arr<uint64_t>();
      f.cluster = cluster.ptr(); f.n_parents = np.ptr(); f.child_pos = cpos.ptr(); f.data_row = row.ptr();
      f.parent_pos = ppos.ptr(); f.length = length.ptr(); f.gamma = gamma.ptr(); f.color = color.ptr();
      f.data = data.ptr(); f.child_mask = cm.ptr(); f.parent_mask = pm.ptr();
      const LgTable before = T;
      if (!pgbp::lg_table_build(&f, dims.ptr(), nc, n_sites, max_dim, T, why)) {
        std::printf("table refused %s\n", why.c_str());
        if (T.n_families != before.n_families || T.cluster != before.cluster || T.cl_off != before.cl_off)
          std::printf("FAILED: a refused table changed the one before it\n");
        continue;
      }
      std::printf("table built %d %d %d %d %d %d\n", T.p, T.K, T.n_rates, T.n_rows, T.n_families, (int)T.uni_ok);
      line("cl_off", T.cl_off);
      line("cl_fam", T.cl_fam);
      line("cluster", T.cluster);
      line("tip", T.tip);
      masks("child_mask", T.child_mask);
      masks("parent_mask", T.parent_mask);
      print_simple(T);
      line("loo", T.loo_tips());
      std::vector<int32_t> fams;
      std::vector<unsigned long long> pred;
      T.impute_list(fams, pred);
      line("impute", fams);
      masks("predicted", pred);
    } else if (cmd == "dims") {
      int max_m = -1;
      const int limit = word<int>();
      if (T.cluster_dims("fn", limit, &max_m, why)) std::printf("dims ok %d\n", max_m);
      else std::printf("dims refused %s\n", why.c_str());
    } else if (cmd == "edges") {
      const Arr<double> length = arr<double>(), gamma = arr<double>();
      if (!T.check_edges(length.ptr(), gamma.ptr(), why)) {
        std::printf("edges refused %s\n", why.c_str());
        continue;
      }
      T.set_edges(length.ptr(), gamma.ptr());
      std::printf("edges ok\n");
      line("length", T.length);
      line("gamma", T.gamma);
      print_simple(T);
    } else if (cmd == "data") {
      const std::string fn = word<std::string>();
      const int32_t sb = word<int32_t>(), se = word<int32_t>(), values = word<int32_t>();
      const Arr<double> data = arr<double>();
      if (T.check_data(fn.c_str(), sb, se, data.ptr(), values != 0, why)) std::printf("data ok\n");
      else std::printf("data refused %s\n", why.c_str());
    } else if (cmd == "shifts") {
      const int32_t n = word<int32_t>(), per_site = word<int32_t>();
      const Arr<int32_t> edge = arr<int32_t>();
      const Arr<double> value = arr<double>();
      std::vector<int32_t> slot{77}, cl{77};
      if (!T.shift_list(n, edge.ptr(), value.ptr(), per_site, slot, cl, why)) {
        std::printf("shifts refused %s\n", why.c_str());
        if (slot != std::vector<int32_t>{77} || cl != std::vector<int32_t>{77}) std::printf("FAILED: a refused list wrote its outputs\n");
        continue;
      }
      std::printf("shifts ok\n");
      line("slot", slot);
      line("cl", cl);
    } else if (cmd == "noise") {
      const int32_t n = word<int32_t>(), per_site = word<int32_t>();
      const Arr<int32_t> family = arr<int32_t>();
      const Arr<double> scale = arr<double>(), sigma_e = arr<double>(), se2 = arr<double>();
      std::vector<int32_t> slot{77}, cl{77};
      std::vector<double> sig;
      int32_t max_dim = -1;
      if (!T.noise_list(n, family.ptr(), scale.ptr(), sigma_e.ptr(), se2.ptr(), per_site, slot, sig, cl, &max_dim, why)) {
        std::printf("noise refused %s\n", why.c_str());
        if (slot != std::vector<int32_t>{77} || cl != std::vector<int32_t>{77} || max_dim != -1)
          std::printf("FAILED: a refused list wrote its outputs\n");
        continue;
      }
      std::printf("noise ok %d\n", max_dim);
      line("slot", slot);
      line("sig", sig);
      line("cl", cl);
    } else {
      std::printf("FAILED: unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  std::printf("lgtable ok\n");
  return 0;
}

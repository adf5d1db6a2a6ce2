// Stand-alone check of the plane-split packed layout (csrc/pgbp_bs16.hpp) on the host: for every even P from 2 to 16 and
// m in {P, 2P}: (i) J_off over the canonical pairs is a bijection onto the stored slots, (r, c) and (c, r) share one;
// (ii) h, g and the record lengths are what they were before the planes; (iii) every wave-instruction of a tile access -- the lanes in lane order
// G b + a, one plane -- covers one contiguous run of 16 bytes per lane.  Built (optionally with -fsanitize=address,undefined)
// and run as a child process by tests/test_bs16_planes_cpu.py; prints one "ok" line per check, exits non-zero at the first
// failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#include "pgbp_bs16.hpp"

namespace bs = pgbp::bs16;

namespace {
[[noreturn]] void fail(const char* what, int P, int m, int x, int y) {
  std::printf("FAILED %s: P = %d, m = %d, (%d, %d)\n", what, P, m, x, y);
  std::exit(1);
}

// (i)
void check_bijection(int P, int m) {
  const int stored = m == P ? bs::h1(P) : bs::h2(P);   // the tiles come first in a record, back to back
  std::vector<int> hits(stored, 0);
  int n = 0;
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < m; ++c) {
      const int o = bs::J_off(m, r, c, P);
      if (o < 0 || o >= stored) fail("J_off out of the tiles", P, m, r, c);
      // (a diagonal block stores all four of its entries; everything else is stored once, for both triangles)
      if ((r >> 1) != (c >> 1) && o != bs::J_off(m, c, r, P)) fail("J_off(r, c) != J_off(c, r)", P, m, r, c);
      if ((r >> 1) == (c >> 1) && r != c && o == bs::J_off(m, c, r, P)) fail("a diagonal block lost an entry", P, m, r, c);
      if (bs::canonical(m, r, c, P)) {
        ++hits[o];
        ++n;
      }
    }
  if (n != stored) fail("canonical pairs != stored slots", P, m, n, stored);
  for (int o = 0; o < stored; ++o)
    if (hits[o] != 1) fail("slot not hit exactly once", P, m, o, hits[o]);
}

// (ii): the values of the layout before the planes, from its description: sym = 2 G (G + 1), [T00 | h | g] and
// [T00 | T10 P*P | T11 | h 2P | g]
void check_tail(int P, int m) {
  const int G = P / 2, sym = 2 * G * (G + 1);
  const int h = m == P ? sym : 2 * sym + P * P, g = h + m, len = g + 1;
  for (int r = 0; r < m; ++r)
    if (bs::h_off(m, r, P) != h + r) fail("h_off", P, m, r, bs::h_off(m, r, P));
  if (bs::g_off(m, P) != g) fail("g_off", P, m, g, bs::g_off(m, P));
  if (bs::rec_len(m, P) != len) fail("rec_len", P, m, len, bs::rec_len(m, P));
  if (bs::t10(P) != sym || bs::t11(P) != sym + P * P) fail("t10 / t11", P, m, bs::t10(P), bs::t11(P));
}

// (iii) tile at rows r0.., columns c0.. of the record, symmetric (lanes a <= b) or full (all lanes), starting at `base` doubles
void check_planes(int P, int m, int r0, int c0, bool sym, int base) {
  const int G = P / 2;
  const int nb = sym ? G * (G + 1) / 2 : G * G;
  for (int q = 0; q < 2; ++q) {   // q = 0: the left columns, 1: the right columns
    int i = 0;
    for (int lane = 0; lane < G * G; ++lane) {
      const int a = lane % G, b = lane / G;
      if (sym && a > b) continue;
      const int lo = bs::J_off(m, r0 + 2 * a, c0 + 2 * b + q, P), hi = bs::J_off(m, r0 + 2 * a + 1, c0 + 2 * b + q, P);
      const long bytes = 8L * (lo - base - q * 2 * nb);
      if (bytes != 16L * i) fail("a plane is not one contiguous run in lane order", P, m, lane, (int)bytes);
      if (hi != lo + 1) fail("the two rows of a column are not 16 bytes together", P, m, lane, hi - lo);
      if ((8L * lo) % 16 != 0) fail("a 16-byte access is not aligned", P, m, lane, lo);
      ++i;
    }
    if (i != nb) fail("lanes of a tile", P, m, i, nb);
  }
}
}  // namespace

int main() {
  for (int P = 2; P <= 16; P += 2)
    for (int m = P; m <= 2 * P; m += P) {
      check_bijection(P, m);
      check_tail(P, m);
      check_planes(P, m, 0, 0, true, 0);
      if (m == 2 * P) {
        check_planes(P, m, P, 0, false, bs::t10(P));
        check_planes(P, m, P, P, true, bs::t11(P));
      }
    }
  std::printf("ok bijection\nok tail\nok planes\n");
  // the P = 16 values in numbers
  if (bs::h_off(16, 0, 16) != 144 || bs::h_off(32, 0, 16) != 544 || bs::g_off(32, 16) != 576 || bs::rec_len(32, 16) != 577 ||
      bs::g_off(16, 16) != 160 || bs::rec_len(16, 16) != 161)
    fail("P = 16 offsets", 16, 0, bs::h_off(32, 0, 16), bs::g_off(16, 16));
  if (8 * bs::sym_plane(16) != 576 || 8 * bs::full_plane(16) != 1024) fail("P = 16 plane strides", 16, 0, bs::sym_plane(16), bs::full_plane(16));
  std::printf("ok p16\nbs16 planes ok\n");
  return 0;
}

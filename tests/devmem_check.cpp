// Stand-alone check of csrc/pgbp_devmem.hpp against a counting stand-in for the runtime: malloc / free with a count of live
// allocations and a switch that fails the N-th one.  Built with -fsanitize=address,undefined and run as a child process by
// tests/test_devmem_cpu.py; prints one "ok" line per check, exits non-zero at the first failure.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "pgbp_devmem.hpp"

namespace {
int g_live = 0, g_live_events = 0;
int g_calls = 0, g_fail_at = 0;   // g_fail_at = N > 0: the N-th allocation (memory and events count together) fails

bool next_call_fails() { return ++g_calls == g_fail_at; }
void arm(int fail_at) {
  g_calls = 0;
  g_fail_at = fail_at;
}
}  // namespace

int pgbp::dev_malloc_bytes(void** p, size_t bytes) {
  *p = nullptr;
  if (next_call_fails()) return 2;
  *p = std::malloc(bytes);
  if (!*p) return 2;
  ++g_live;
  return 0;
}
void pgbp::dev_free_bytes(void* p) {
  --g_live;
  std::free(p);   // (a double release is the sanitizer's to report)
}
int pgbp::dev_event_create(void** ev) {
  *ev = nullptr;
  if (next_call_fails()) return 2;
  *ev = std::malloc(1);
  ++g_live_events;
  return 0;
}
void pgbp::dev_event_destroy(void* ev) {
  --g_live_events;
  std::free(ev);
}

using pgbp::DevBuf;
using pgbp::EventPair;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                           \
    }                                                                     \
  } while (0)

namespace {

// the eight buffers that have to exist together, as pgbp_engine holds the site-minor set
struct Group {
  DevBuf<double> pool, fpool, rpool, kldiv;
  DevBuf<int> flags, status, klflags, poison;
  const void* ptr(int i) const {
    const void* q[8] = {pool.get(), fpool.get(), rpool.get(), flags.get(), status.get(), klflags.get(), kldiv.get(), poison.get()};
    return q[i];
  }
};

// the acquisition pattern of the engine: everything into locals, the destination takes them after the last one succeeded
int acquire(Group& g, size_t n) {
  DevBuf<double> pool, fpool, rpool, kldiv;
  DevBuf<int> flags, status, klflags, poison;
  int rc;
  if ((rc = pool.alloc(n))) return rc;
  if ((rc = fpool.alloc(n))) return rc;
  if ((rc = rpool.alloc(n))) return rc;
  if ((rc = flags.alloc(n))) return rc;
  if ((rc = status.alloc(n))) return rc;
  if ((rc = klflags.alloc(n))) return rc;
  if ((rc = kldiv.alloc(n))) return rc;
  if ((rc = poison.alloc(n))) return rc;
  g.pool = std::move(pool);
  g.fpool = std::move(fpool);
  g.rpool = std::move(rpool);
  g.flags = std::move(flags);
  g.status = std::move(status);
  g.klflags = std::move(klflags);
  g.kldiv = std::move(kldiv);
  g.poison = std::move(poison);
  return 0;
}

int run() {
  arm(0);
  {  // scope exit
    DevBuf<double> a;
    CHECK(!a && a.get() == nullptr);
    CHECK(a.alloc(16) == 0 && a && g_live == 1);
    a.get()[15] = 1.0;
  }
  CHECK(g_live == 0);
  std::printf("ok scope exit\n");

  {  // reset, and a second reset
    DevBuf<int> a;
    CHECK(a.alloc(4) == 0 && g_live == 1);
    a.reset();
    CHECK(g_live == 0 && !a);
    a.reset();
    CHECK(g_live == 0);
  }
  CHECK(g_live == 0);
  std::printf("ok reset\n");

  {  // alloc over a live buffer releases it; alloc(0) is one element, not null
    DevBuf<int> a;
    CHECK(a.alloc(4) == 0 && a.alloc(8) == 0 && g_live == 1);
    a.get()[7] = 7;
    CHECK(a.alloc(0) == 0 && a && g_live == 1);
    a.get()[0] = 1;
    arm(1);   // a failed alloc leaves it holding nothing
    CHECK(a.alloc(4) != 0 && !a && g_live == 0);
    arm(0);
  }
  CHECK(g_live == 0);
  std::printf("ok alloc\n");

  {  // move construction and move assignment over a live buffer
    DevBuf<int> a, b;
    CHECK(a.alloc(4) == 0 && b.alloc(4) == 0 && g_live == 2);
    int* const pb = b.get();
    a = std::move(b);
    CHECK(g_live == 1 && a.get() == pb && !b);
    DevBuf<int> c(std::move(a));
    CHECK(g_live == 1 && c.get() == pb && !a);
    DevBuf<int>& self = c;
    c = std::move(self);
    CHECK(g_live == 1 && c.get() == pb);
  }
  CHECK(g_live == 0);
  std::printf("ok move\n");

  {  // swap keeps both
    DevBuf<int> a, b, none;
    CHECK(a.alloc(1) == 0 && b.alloc(2) == 0);
    int *const pa = a.get(), *const pb = b.get();
    a.get()[0] = 10;
    b.get()[1] = 20;
    a.swap(b);
    CHECK(g_live == 2 && a.get() == pb && b.get() == pa && a.get()[1] == 20 && b.get()[0] == 10);
    a.swap(none);
    CHECK(g_live == 2 && !a && none.get() == pb);
  }
  CHECK(g_live == 0);
  std::printf("ok swap\n");

  for (int had = 0; had < 2; ++had) {  // the group of eight: into an empty destination, and over an earlier complete group
    for (int k = 1; k <= 8; ++k) {
      Group g;
      arm(0);
      if (had) CHECK(acquire(g, 3) == 0 && g_live == 8);
      const void* before[8];
      for (int i = 0; i < 8; ++i) before[i] = g.ptr(i);
      arm(k);
      CHECK(acquire(g, 5) != 0);
      arm(0);
      CHECK(g_live == (had ? 8 : 0));
      for (int i = 0; i < 8; ++i) CHECK(g.ptr(i) == before[i]);
      CHECK(acquire(g, 5) == 0 && g_live == 8);   // ... and the retry takes
      for (int i = 0; i < 8; ++i) CHECK(g.ptr(i) != nullptr);
    }
    CHECK(g_live == 0);
  }
  std::printf("ok group of eight\n");

  {  // the event pair: both or none
    EventPair a;
    CHECK(a.first() == nullptr && a.second() == nullptr);
    CHECK(a.create() == 0 && g_live_events == 2 && a.first() && a.second() && a.first() != a.second());
    CHECK(a.create() == 0 && g_live_events == 2);
    EventPair b(std::move(a));
    CHECK(g_live_events == 2 && a.first() == nullptr && b.first());
    EventPair c;
    CHECK(c.create() == 0 && g_live_events == 4);
    c = std::move(b);
    CHECK(g_live_events == 2);
    for (int k = 1; k <= 2; ++k) {
      EventPair d;
      arm(k);
      CHECK(d.create() != 0 && d.first() == nullptr && d.second() == nullptr && g_live_events == 2);
      arm(0);
    }
  }
  CHECK(g_live_events == 0 && g_live == 0);
  std::printf("ok event pair\n");
  return 0;
}

}  // namespace

int main() {
  const int rc = run();
  if (rc == 0) std::printf("devmem ok\n");
  return rc;
}

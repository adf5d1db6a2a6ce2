// Owners of device memory and of HIP event pairs.  Every device allocation of the library belongs to exactly one DevBuf:
// it is released when its owner goes out of scope, is reset, or is assigned over.  Kernel-argument structs (DevState,
// EngineView, LgStatic, LgParams) carry BORROWED pointers taken with get().
// Plain C++: the four functions below are the only doors to the runtime (pgbp_engine.hip defines them over hipMalloc /
// hipFree / hipEventCreate / hipEventDestroy; tests/devmem_check.cpp over a counting stand-in).
#pragma once
#include <cstddef>
#include <memory>

namespace pgbp {

int dev_malloc_bytes(void** p, size_t bytes);  // 0 and *p, or the runtime's error code (a hipError_t)
void dev_free_bytes(void* p);
int dev_event_create(void** ev);               // 0 and *ev, or the error code with *ev null
void dev_event_destroy(void* ev);

// move-only: moving from a buffer leaves it empty, assigning over a live one releases it
template <class T>
class DevBuf {
 public:
  T* get() const { return p_.get(); }
  explicit operator bool() const { return bool(p_); }
  void reset() { p_.reset(); }
  // n elements (n == 0: one, so that a live buffer is never null) in place of what it held; on failure it holds nothing
  int alloc(size_t n) {
    reset();
    void* q = nullptr;
    const int rc = dev_malloc_bytes(&q, (n ? n : 1) * sizeof(T));
    if (rc == 0) p_.reset(static_cast<T*>(q));
    return rc;
  }
  void swap(DevBuf& o) noexcept { p_.swap(o.p_); }

 private:
  struct Free { void operator()(T* p) const { dev_free_bytes(p); } };
  std::unique_ptr<T, Free> p_;
};

// Two events, both or none, move-only as well.  The handles are the runtime's (hipEvent_t is a pointer).
class EventPair {
 public:
  int create() {
    reset();
    void *a = nullptr, *b = nullptr;
    int rc = dev_event_create(&a);
    a_.reset(a);
    if (rc == 0 && (rc = dev_event_create(&b)) != 0) reset();
    b_.reset(b);
    return rc;
  }
  void reset() { a_.reset(); b_.reset(); }
  void* first() const { return a_.get(); }
  void* second() const { return b_.get(); }

 private:
  struct Destroy { void operator()(void* ev) const { dev_event_destroy(ev); } };
  std::unique_ptr<void, Destroy> a_, b_;
};

}  // namespace pgbp

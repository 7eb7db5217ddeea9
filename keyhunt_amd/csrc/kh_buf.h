// kh_buf.h -- move-only owners of device memory, pinned host memory and events.  An owner holds the
// pointer together with its element capacity and frees in its destructor, so a buffer and its size
// cannot drift apart and no return path leaks.  These are the library's only allocation calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <utility>

struct kh_ctx;

namespace kh {

// sets ctx->err to "<what>: <HIP error string>"; KH_E_NOMEM for out-of-memory, else KH_E_HIP (kh_ctx.h)
int hip_fail(kh_ctx *c, const char *what, hipError_t e);

struct dev_alloc {
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void *p) { (void)hipFree(p); }
  static constexpr const char *name = "hipMalloc";
};
struct pinned_alloc {
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void *p) { (void)hipHostFree(p); }
  static constexpr const char *name = "hipHostMalloc";
};

template <class T, class A>
class gpu_buf {
  T *p_ = nullptr;
  size_t cap_ = 0;

 public:
  gpu_buf() = default;
  gpu_buf(gpu_buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  gpu_buf &operator=(gpu_buf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~gpu_buf() { reset(); }
  T *get() const { return p_; }
  size_t cap() const { return cap_; }  // elements
  explicit operator bool() const { return p_ != nullptr; }
  void reset() {
    if (p_) A::free(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // Room for n elements.  A buffer that already holds n is left alone; otherwise the old one is freed
  // BEFORE the new one is allocated (the BSGS pad is 64 GB and must never exist twice).  On failure the
  // owner is empty with capacity 0 and ctx->err is set.
  int reserve(kh_ctx *c, size_t n) {
    if (n <= cap_) return 0;
    reset();
    void *p = nullptr;
    hipError_t e = A::alloc(&p, n * sizeof(T));
    if (e != hipSuccess) return hip_fail(c, A::name, e);
    p_ = (T *)p;
    cap_ = n;
    return 0;
  }
};
template <class T>
using dev_buf = gpu_buf<T, dev_alloc>;
template <class T>
using pinned_buf = gpu_buf<T, pinned_alloc>;

class gpu_event {
  hipEvent_t e_ = nullptr;

 public:
  gpu_event() = default;
  gpu_event(const gpu_event &) = delete;
  gpu_event &operator=(const gpu_event &) = delete;
  ~gpu_event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  hipEvent_t get() const { return e_; }
  int create(kh_ctx *c) {  // no-op once created
    if (e_) return 0;
    hipError_t e = hipEventCreate(&e_);
    return e == hipSuccess ? 0 : hip_fail(c, "hipEventCreate", e);
  }
};

}  // namespace kh

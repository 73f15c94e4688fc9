// Ownership of everything the host side takes from the HIP runtime: device buffers, pinned host buffers, streams and events.  Host code
// only.  This is the one file that allocates and frees them (the exceptions: mogp_dev_malloc / mogp_dev_free hand raw memory to the
// caller, and the signal word of Engine comes from hipExtMallocWithFlags).  Every owner is move-only and releases in its destructor, so a
// constructor or a function that throws half-way gives back what it had taken.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <exception>

namespace mogp {

void hip_check(hipError_t e, const char* what);
#define HIPCK(x) hip_check((x), #x)

// device bytes currently held by DevBuf objects of this process (mogp_profile_counter "device_bytes_live")
inline std::atomic<long long> g_device_bytes_live{0};

template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  explicit DevBuf(size_t count) { reserve(count); }      // count = 0: one element, so that the pointer is never null
  ~DevBuf() { reset(); }
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p_, o.p_);
      std::swap(n_, o.n_);
    }
    return *this;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t size() const { return n_; }
  void reset() noexcept {
    if (p_) {
      (void)hipFree(p_);
      g_device_bytes_live -= (long long)bytes(n_);
    }
    p_ = nullptr;
    n_ = 0;
  }
  // Only grows; the contents are not kept.  Frees first and allocates then -- these buffers are up to tens of GB, the other order would
  // double the peak -- and is empty in between, so a failed allocation leaves an empty buffer behind, not a stale pointer.
  void reserve(size_t count) {
    if (p_ && count <= n_) return;
    reset();
    hip_check(hipMalloc(reinterpret_cast<void**>(&p_), bytes(count)), "hipMalloc");
    n_ = count;
    g_device_bytes_live += (long long)bytes(n_);
  }

 private:
  static size_t bytes(size_t count) { return std::max<size_t>(count, 1) * sizeof(T); }
  T* p_ = nullptr;
  size_t n_ = 0;
};

// pinned host memory
template <class T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  explicit PinnedBuf(size_t count) : n_(count) {
    hip_check(hipHostMalloc(reinterpret_cast<void**>(&p_), std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault), "hipHostMalloc");
  }
  ~PinnedBuf() { reset(); }
  PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p_, o.p_);
      std::swap(n_, o.n_);
    }
    return *this;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t size() const { return n_; }
  void reset() noexcept {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    n_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// a stream or an event; converts to the runtime's handle wherever one is asked for
template <class H, hipError_t (*Destroy)(H)>
class Owned {
 public:
  Owned() = default;
  explicit Owned(H h) : h_(h) {}
  ~Owned() { reset(); }
  Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(h_, o.h_);
    }
    return *this;
  }
  operator H() const { return h_; }
  void reset() noexcept {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }

 private:
  H h_ = nullptr;
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

inline Stream make_stream(unsigned flags) {
  hipStream_t s = nullptr;
  hip_check(hipStreamCreateWithFlags(&s, flags), "hipStreamCreateWithFlags");
  return Stream(s);
}
inline Stream make_stream(unsigned flags, int priority) {
  hipStream_t s = nullptr;
  hip_check(hipStreamCreateWithPriority(&s, flags, priority), "hipStreamCreateWithPriority");
  return Stream(s);
}
inline Event make_event(unsigned flags) {
  hipEvent_t e = nullptr;
  hip_check(hipEventCreateWithFlags(&e, flags), "hipEventCreateWithFlags");
  return Event(e);
}
// a timing event, or an empty owner when the runtime has none to give (the profiling hooks then skip the launch)
inline Event try_make_timing_event() noexcept {
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) e = nullptr;
  return Event(e);
}

// Declared AFTER the buffers that kernels on `s` use: when the scope is left through an exception, the stream is drained before those
// buffers are freed (hipFree is not relied on for that).
struct SyncOnUnwind {
  hipStream_t s;
  int live = std::uncaught_exceptions();
  ~SyncOnUnwind() { if (std::uncaught_exceptions() > live) (void)hipStreamSynchronize(s); }
};

}  // namespace mogp

// mcs_hip_owned.h -- what the context of mcs_api.hip owns, each in a type that cannot be left half-valid: device and pinned
// buffers, the particle population's nine arrays, streams, events.  (The rules by which the library reads its environment, once
// declared here, live with the option table in mcs_options.h, which this header includes.)
// Host code only (the runtime API, no kernels): a plain C++ compiler builds it, tests/host/hip_owned_main.cpp does.
#pragma once
#include <hip/hip_runtime_api.h>

#include "mcs_options.h"

#include <cstdint>
#include <cstdlib>
#include <utility>

// the size a per-particle array grows to when n particles no longer fit (tables, counters and launch constants are sized exactly)
inline long long grow_cap(long long n) { return n + n / 8 + 1024; }

// A block of `cap` elements of device (DevBuf) or pinned host (PinnedBuf) memory, or nothing: {nullptr, 0}.
template <class T, bool Pinned>
class HipBuf {
 public:
  HipBuf() = default;
  HipBuf(HipBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  HipBuf& operator=(HipBuf&& o) noexcept { if (this != &o) { reset(); std::swap(p_, o.p_); std::swap(cap_, o.cap_); } return *this; }
  ~HipBuf() { reset(); }
  static const char* alloc_name() { return Pinned ? "hipHostMalloc" : "hipMalloc"; }
  // room for n elements: nothing happens when they fit, else the old block is freed (its contents are lost) and one of exactly n
  // elements allocated; after a failure the buffer is empty
  hipError_t reserve(long long n) {
    if (n <= cap_) return hipSuccess;
    reset();
    void* p = nullptr;
    const size_t bytes = (size_t)n * sizeof(T);
    const hipError_t e = Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e == hipSuccess) { p_ = static_cast<T*>(p); cap_ = n; }
    return e;
  }
  void reset() { if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; cap_ = 0; }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  long long cap() const { return cap_; }

 private:
  T* p_ = nullptr;
  long long cap_ = 0;
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinnedBuf = HipBuf<T, true>;

template <class... B> void reset_all(B&... b) { (b.reset(), ...); }

// The resident population's arrays: the eight fp64 fields in the order of DevPop / mcs_soa, and the packed meta word.
// All nine hold cap() entries, or none exists.
struct PopBuf {
  DevBuf<double> f[8];
  DevBuf<uint32_t> meta;
  static const char* alloc_name() { return "hipMalloc"; }
  long long cap() const { return meta.cap(); }      // (meta is allocated last)
  void reset() { for (auto& b : f) b.reset(); meta.reset(); }
  hipError_t reserve(long long n) {
    if (n <= cap()) return hipSuccess;
    hipError_t e = hipSuccess;
    for (auto& b : f) if (e == hipSuccess) e = b.reserve(n);
    if (e == hipSuccess) e = meta.reserve(n);
    if (e != hipSuccess) reset();
    return e;
  }
};

// A stream or an event the context created (null: none).
template <class H, hipError_t (*Destroy)(H)>
class HipHandle {
 public:
  HipHandle() = default;
  HipHandle(HipHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  HipHandle& operator=(HipHandle&& o) noexcept { if (this != &o) { reset(); std::swap(h_, o.h_); } return *this; }
  ~HipHandle() { reset(); }
  void reset() { if (h_) (void)Destroy(h_); h_ = nullptr; }
  operator H() const { return h_; }

 protected:
  H* fresh() { reset(); return &h_; }                                                    // where a create call puts the new handle ...
  hipError_t created(hipError_t e) { if (e != hipSuccess) h_ = nullptr; return e; }      // ... and nothing after a failed one
  H h_ = nullptr;
};
struct Stream : HipHandle<hipStream_t, hipStreamDestroy> {
  hipError_t create() { return created(hipStreamCreate(fresh())); }
  hipError_t create_non_blocking() { return created(hipStreamCreateWithFlags(fresh(), hipStreamNonBlocking)); }
  hipError_t create_cu_masked(uint32_t words, const uint32_t* mask) { return created(hipExtStreamCreateWithCUMask(fresh(), words, mask)); }
};
struct Event : HipHandle<hipEvent_t, hipEventDestroy> {
  hipError_t create() { return created(hipEventCreate(fresh())); }
  hipError_t create_untimed() { return created(hipEventCreateWithFlags(fresh(), hipEventDisableTiming)); }
};

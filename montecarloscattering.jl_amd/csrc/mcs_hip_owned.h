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

// SEVERAL buffers that exist together or not at all.  A group derives from BufGroup, names its members, reads cap() from one of them
// and says in grow(n) what each holds for n entries (a failed grow leaves every member empty); reserve(n) is a no-op while n fit.
template <class G> struct BufGroup {
  static const char* alloc_name() { return "hipMalloc"; }
  hipError_t reserve(long long n) { G& g = static_cast<G&>(*this); return n <= g.cap() ? hipSuccess : g.grow(n); }
};
// what grow() is made of: b[i] gets n[i] elements.  The blocks they hold are freed first: old and new never lie side by side.
template <class... B> hipError_t reserve_all(const long long (&n)[sizeof...(B)], B&... b) {
  reset_all(b...);
  hipError_t e = hipSuccess;
  int i = 0;
  ((e = e == hipSuccess ? b.reserve(n[i++]) : e), ...);
  if (e != hipSuccess) reset_all(b...);
  return e;
}

// The resident population's arrays: the eight fp64 fields in the order of DevPop / mcs_soa, and the packed meta word.
struct PopBuf : BufGroup<PopBuf> {
  DevBuf<double> f[8];
  DevBuf<uint32_t> meta;
  long long cap() const { return meta.cap(); }      // (meta is allocated last)
  hipError_t grow(long long n) { return reserve_all({n, n, n, n, n, n, n, n, n}, f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], meta); }
};
// The per-particle end states a debug run records (mcs_set_debug_finals).
struct FinalsBuf : BufGroup<FinalsBuf> {
  DevBuf<int32_t> reason, helix, retro; DevBuf<double> ptot, x;
  long long cap() const { return x.cap(); }
  hipError_t grow(long long n) { return reserve_all({n, n, n, n, n}, reason, helix, retro, ptot, x); }
};
// The compaction's scratch for cap() status bytes: the count and the offset of every block of them, the index list src[].
struct ScanScratch : BufGroup<ScanScratch> {
  static constexpr long long kBlock = 1024;      // entries per block of the compaction kernels (mcs_k_count_saved & co., mcs_population.hip)
  static long long blocks(long long n) { return (n + kBlock - 1) / kBlock; }
  DevBuf<unsigned int> bcounts; DevBuf<unsigned long long> boffs; DevBuf<long long> src;
  long long cap() const { return src.cap(); }
  hipError_t grow(long long n) { return reserve_all({blocks(n), blocks(n), n}, bcounts, boffs, src); }
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

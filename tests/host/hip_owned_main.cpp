// The owning types and environment rules of csrc/mcs_hip_owned.h on the CPU: the HIP calls the header makes are defined HERE, over
// malloc, with counters and "fail the k-th allocation" -- what an out-of-memory return does to a buffer cannot be tried on a GPU.
// Built with -fsanitize=address,undefined by tests/test_hip_owned.py: a double free, a leak or a use of a freed block ends the run.
#include "mcs_hip_owned.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

static long g_allocs = 0, g_frees = 0, g_live = 0, g_alloc_index = 0, g_fail_at = -1, g_handles = 0;
static size_t g_last_bytes = 0;
static bool g_fail_handles = false;

static hipError_t stub_alloc(void** p, size_t bytes) {
  if (g_alloc_index++ == g_fail_at) { *p = (void*)(uintptr_t)0x10; return hipErrorOutOfMemory; }      // (a failed call's output is not a pointer)
  *p = std::malloc(bytes ? bytes : 1);
  ++g_allocs; ++g_live; g_last_bytes = bytes;
  return hipSuccess;
}
static hipError_t stub_free(void* p) { std::free(p); ++g_frees; --g_live; return hipSuccess; }
template <class H> static hipError_t stub_handle(H* h) {
  if (g_fail_handles) { *h = (H)(uintptr_t)0x10; return hipErrorOutOfMemory; }
  *h = (H)std::malloc(1); ++g_handles;
  return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return stub_alloc(p, bytes); }
hipError_t hipFree(void* p) { return stub_free(p); }
hipError_t hipHostFree(void* p) { return stub_free(p); }
hipError_t hipStreamCreate(hipStream_t* s) { return stub_handle(s); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return stub_handle(s); }
hipError_t hipExtStreamCreateWithCUMask(hipStream_t* s, uint32_t, const uint32_t*) { return stub_handle(s); }
hipError_t hipStreamDestroy(hipStream_t s) { std::free(s); --g_handles; return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { return stub_handle(e); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return stub_handle(e); }
hipError_t hipEventDestroy(hipEvent_t e) { std::free(e); --g_handles; return hipSuccess; }
}

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

struct Calls { long allocs, frees; };
static Calls calls() { return {g_allocs, g_frees}; }
static bool no_calls_since(Calls c) { return g_allocs == c.allocs && g_frees == c.frees; }
static void fail_allocation(long k) { g_alloc_index = 0; g_fail_at = k; }      // the k-th allocation from here on fails (-1: none)

template <class Buf, class T> static void test_buffer() {
  {
    Buf b;
    CHECK(b.get() == nullptr && b.cap() == 0);
    Calls c0 = calls();
    CHECK(b.reserve(0) == hipSuccess && no_calls_since(c0));
    CHECK(b.reserve(100) == hipSuccess && b.get() && b.cap() == 100);
    CHECK(g_allocs == c0.allocs + 1 && g_frees == c0.frees && g_last_bytes == 100 * sizeof(T));
    b.get()[99] = T();                   // (the block has room for every element: ASan checks it)
    // no-op reserve
    Calls c1 = calls();
    T* const p = b.get();
    CHECK(b.reserve(100) == hipSuccess && b.reserve(1) == hipSuccess && b.reserve(0) == hipSuccess);
    CHECK(no_calls_since(c1) && b.get() == p && b.cap() == 100);
    // a grow: one free, one allocation of exactly n elements
    CHECK(b.reserve(101) == hipSuccess);
    CHECK(g_allocs == c1.allocs + 1 && g_frees == c1.frees + 1 && g_last_bytes == 101 * sizeof(T) && b.cap() == 101);
    b.get()[100] = T();
  }
  CHECK(g_live == 0);
  // the scenario reserve(10), reserve(20) makes two allocations: fail each in turn
  for (long k = 0; k < 2; ++k) {
    {
      Buf b;
      fail_allocation(k);
      const hipError_t e1 = b.reserve(10);
      CHECK((e1 == hipSuccess) == (k != 0));
      if (k == 0) CHECK(b.get() == nullptr && b.cap() == 0 && g_live == 0);
      const hipError_t e2 = b.reserve(20);
      if (k == 0) CHECK(e2 == hipSuccess && b.cap() == 20);      // (the later reserve succeeds)
      else CHECK(e2 == hipErrorOutOfMemory && b.get() == nullptr && b.cap() == 0 && g_live == 0);
      fail_allocation(-1);
      CHECK(b.reserve(30) == hipSuccess && b.get() && b.cap() == 30 && g_live == 1);
      b.get()[29] = T();
    }
    CHECK(g_live == 0);
  }
  // move and swap: pointer and capacity travel together, the moved-from buffer is empty, nothing is allocated or freed
  {
    Buf a;
    CHECK(a.reserve(8) == hipSuccess);
    T* const pa = a.get();
    Calls c0 = calls();
    Buf b(std::move(a));
    CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 8 && no_calls_since(c0));
    CHECK(a.reserve(3) == hipSuccess);
    T* const pa2 = a.get();
    Calls c1 = calls();
    std::swap(a, b);
    CHECK(a.get() == pa && a.cap() == 8 && b.get() == pa2 && b.cap() == 3 && no_calls_since(c1));
    b = std::move(a);                    // (b's own block is freed, once)
    CHECK(g_frees == c1.frees + 1 && g_allocs == c1.allocs && b.get() == pa && b.cap() == 8 && a.get() == nullptr && a.cap() == 0);
    b.reset();
    CHECK(b.get() == nullptr && b.cap() == 0 && g_live == 0);
  }
  CHECK(g_live == 0);
}

static bool pop_empty(const PopBuf& b) {
  for (const auto& f : b.f) if (f.get() || f.cap()) return false;
  return !b.meta.get() && !b.meta.cap() && b.cap() == 0;
}
static bool pop_holds(const PopBuf& b, long long n) {
  for (const auto& f : b.f) if (!f.get() || f.cap() != n) return false;
  return b.meta.get() && b.meta.cap() == n && b.cap() == n;
}
static void test_popbuf() {
  // reserve(100), reserve(300): 18 allocations.  Whichever fails, the population's buffer is empty afterwards -- all nine or none
  for (long k = 0; k < 18; ++k) {
    {
      PopBuf b;
      CHECK(pop_empty(b));
      fail_allocation(k);
      const hipError_t e1 = b.reserve(100);
      if (k < 9) {
        CHECK(e1 == hipErrorOutOfMemory && pop_empty(b) && g_live == 0);
      } else {
        CHECK(e1 == hipSuccess && pop_holds(b, 100) && g_live == 9);
        Calls c0 = calls();
        CHECK(b.reserve(100) == hipSuccess && b.reserve(7) == hipSuccess && no_calls_since(c0) && pop_holds(b, 100));
        // the grow fails at field k - 9: the fields before it hold 300 entries by then, those after it nothing (a group frees first)
        CHECK(b.reserve(300) == hipErrorOutOfMemory && pop_empty(b) && g_live == 0);
      }
      fail_allocation(-1);
      CHECK(b.reserve(300) == hipSuccess && pop_holds(b, 300) && g_live == 9);
      b.f[7].get()[299] = 1.0; b.meta.get()[299] = 1u;
    }
    CHECK(g_live == 0);
  }
  {
    PopBuf a, b;
    CHECK(a.reserve(5) == hipSuccess && b.reserve(9) == hipSuccess);
    double* const pa = a.f[0].get();
    uint32_t* const mb = b.meta.get();
    Calls c0 = calls();
    std::swap(a, b);                     // the rotation of the context's buffers
    CHECK(pop_holds(a, 9) && pop_holds(b, 5) && b.f[0].get() == pa && a.meta.get() == mb && no_calls_since(c0));
    PopBuf n;
    CHECK(n.reserve(20) == hipSuccess);
    a = std::move(n);                    // the preserving grow: the old nine blocks are freed, the new ones move in
    CHECK(g_frees == c0.frees + 9 && pop_holds(a, 20) && pop_empty(n));
  }
  CHECK(g_live == 0);
}

// Groups of buffers (BufGroup + reserve_all): state(g, n) says that every member of g holds what n entries take -- n == 0: nothing,
// and no block -- and that the capacity read from the members is n.
static bool fin_state(const FinalsBuf& b, long long n) {
  const long long caps[5] = {b.reason.cap(), b.helix.cap(), b.retro.cap(), b.ptot.cap(), b.x.cap()};
  const void* const ps[5] = {b.reason.get(), b.helix.get(), b.retro.get(), b.ptot.get(), b.x.get()};
  for (int i = 0; i < 5; ++i) if (caps[i] != n || (ps[i] != nullptr) != (n > 0)) return false;
  return b.cap() == n;
}
static bool scan_state(const ScanScratch& b, long long n) {
  const long long nb = ScanScratch::blocks(n);
  if (b.bcounts.cap() != nb || b.boffs.cap() != nb || b.src.cap() != n || b.cap() != n) return false;
  return (b.bcounts.get() != nullptr) == (n > 0) && (b.boffs.get() != nullptr) == (n > 0) && (b.src.get() != nullptr) == (n > 0);
}
template <class G, class State> static void test_group(long members, State state) {
  {
    G g;
    CHECK(state(g, 0));
    Calls c0 = calls();
    CHECK(g.reserve(0) == hipSuccess && no_calls_since(c0) && state(g, 0));
    // a first reserve: one allocation per member
    CHECK(g.reserve(100) == hipSuccess && state(g, 100) && g_allocs == c0.allocs + members && g_frees == c0.frees && g_live == members);
    // no-op reserve
    Calls c1 = calls();
    CHECK(g.reserve(100) == hipSuccess && g.reserve(7) == hipSuccess && g.reserve(0) == hipSuccess && no_calls_since(c1) && state(g, 100));
    // a grow: every member is freed and allocated again, with its own exact size
    CHECK(g.reserve(2000) == hipSuccess && state(g, 2000) && g_allocs == c1.allocs + members && g_frees == c1.frees + members && g_live == members);
  }
  CHECK(g_live == 0);
  // reserve(100), reserve(2000) makes 2 * members allocations: whichever fails, every member is empty afterwards, the capacity is 0 and
  // nothing of the group is left allocated; a later reserve succeeds
  for (long k = 0; k < 2 * members; ++k) {
    {
      PopBuf other;                      // (somebody else's blocks stay)
      CHECK(other.reserve(3) == hipSuccess);
      const long live0 = g_live;
      G g;
      fail_allocation(k);
      const hipError_t e1 = g.reserve(100);
      if (k < members) {
        CHECK(e1 == hipErrorOutOfMemory && state(g, 0) && g.cap() == 0 && g_live == live0);
      } else {
        CHECK(e1 == hipSuccess && state(g, 100) && g_live == live0 + members);
        CHECK(g.reserve(2000) == hipErrorOutOfMemory && state(g, 0) && g.cap() == 0 && g_live == live0);
      }
      fail_allocation(-1);
      CHECK(g.reserve(2000) == hipSuccess && state(g, 2000) && g_live == live0 + members);
    }
    CHECK(g_live == 0);
  }
}
static void test_groups() {
  test_group<FinalsBuf>(5, fin_state);
  test_group<ScanScratch>(3, scan_state);
  // the scan scratch has one count and one offset per 1024 status bytes, the block of the compaction kernels
  CHECK(ScanScratch::blocks(0) == 0 && ScanScratch::blocks(1) == 1 && ScanScratch::blocks(1024) == 1 && ScanScratch::blocks(1025) == 2);
  for (long long n : {1LL, 1024LL, 1025LL}) {
    ScanScratch s;
    CHECK(s.reserve(n) == hipSuccess && scan_state(s, n) && s.bcounts.cap() == (n + 1023) / 1024);
    s.src.get()[n - 1] = 0; s.bcounts.get()[s.bcounts.cap() - 1] = 0u; s.boffs.get()[s.boffs.cap() - 1] = 0ull;      // (ASan: there is room)
  }
  {
    FinalsBuf a, b;
    CHECK(a.reserve(5) == hipSuccess && b.reserve(9) == hipSuccess);
    a.x.get()[4] = 1.0; a.reason.get()[4] = 1;
    Calls c0 = calls();
    a = std::move(b);                    // (a's five blocks are freed, b's move in)
    CHECK(g_frees == c0.frees + 5 && g_allocs == c0.allocs && fin_state(a, 9) && fin_state(b, 0));
  }
  CHECK(g_live == 0);
}

static void test_handles() {
  {
    Stream s, nb, cu;
    Event e, u;
    CHECK(!s && !e);
    const uint32_t mask[1] = {0xffu};
    CHECK(s.create() == hipSuccess && nb.create_non_blocking() == hipSuccess && cu.create_cu_masked(1, mask) == hipSuccess);
    CHECK(e.create() == hipSuccess && u.create_untimed() == hipSuccess);
    CHECK(s && nb && cu && e && u && g_handles == 5);
    hipStream_t raw = s;
    Stream t(std::move(s));
    CHECK(!s && (hipStream_t)t == raw && g_handles == 5);
    nb = std::move(t);                   // (nb's own stream is destroyed)
    CHECK(!t && (hipStream_t)nb == raw && g_handles == 4);
    cu.reset();
    CHECK(!cu && g_handles == 3);
    g_fail_handles = true;
    CHECK(cu.create() != hipSuccess && !cu && u.create() != hipSuccess && !u && g_handles == 2);      // (a failed create leaves nothing)
    g_fail_handles = false;
  }
  CHECK(g_handles == 0);
}

static void put(const char* name, const char* v) { if (v) setenv(name, v, 1); else unsetenv(name); }
static void test_env() {
  const char* const vals[6] = {nullptr, "", "0", "1", "2", "x"};      // nullptr: unset
  const bool on[6] = {false, false, false, true, false, false};
  const bool not_off[6] = {true, true, false, true, true, true};
  const int tri[6] = {2, 2, 0, 1, 2, 2};
  for (const char* name : {"MCS_FORCE_GENERAL", "MCS_F32_LOOP", "MCS_F32_EXACT", "MCS_TALLY_REPLICAS_OFF"})
    for (int i = 0; i < 6; ++i) { put(name, vals[i]); CHECK(env_on(name) == on[i]); }
  for (const char* name : {"MCS_TAIL_MERGE", "MCS_PARK", "MCS_TAIL_RING"})
    for (int i = 0; i < 6; ++i) { put(name, vals[i]); CHECK(env_not_off(name) == not_off[i]); }
  for (int i = 0; i < 6; ++i) { put("MCS_K1_WS", vals[i]); CHECK(env_tristate("MCS_K1_WS") == tri[i]); }
  put("MCS_K1_WS", "10"); CHECK(env_tristate("MCS_K1_WS") == 1);      // (the first character decides)
  put("MCS_PARK", "01"); CHECK(!env_not_off("MCS_PARK"));
  put("MCS_F32_LOOP", "1x"); CHECK(env_on("MCS_F32_LOOP"));
  // "" and "x" read as 0 (atoi): accepted where 0 lies in the range
  struct Row { const char* name; long long lo, hi, dflt; long long want[6]; };
  const Row rows[] = {
      {"MCS_TAIL_LOOP", 0, 32, 12, {12, 0, 0, 1, 2, 0}},
      {"MCS_TAIL_BUDGET", 0, LLONG_MAX, 5, {5, 0, 0, 1, 2, 0}},
      {"MCS_PIPE_SIDE_CUS", 0, 128, 12, {12, 0, 0, 1, 2, 0}},
      {"MCS_REFILL_MIN", 1, 48, 12, {12, 12, 12, 1, 2, 12}},
      {"MCS_DEFER_K", 1, 40, 8, {8, 8, 8, 1, 2, 8}},
      {"MCS_WS_AUTO_MIN", 0, LLONG_MAX, 6000000, {6000000, 0, 0, 1, 2, 0}},
  };
  for (const Row& r : rows) {
    for (int i = 0; i < 6; ++i) { put(r.name, vals[i]); CHECK(env_int(r.name, r.lo, r.hi, r.dflt) == r.want[i]); }
    put(r.name, std::to_string(r.lo - 1).c_str()); CHECK(env_int(r.name, r.lo, r.hi, r.dflt) == r.dflt);
    put(r.name, std::to_string(r.lo).c_str()); CHECK(env_int(r.name, r.lo, r.hi, r.dflt) == r.lo);
    put(r.name, std::to_string(r.hi).c_str()); CHECK(env_int(r.name, r.lo, r.hi, r.dflt) == r.hi);
    if (r.hi < LLONG_MAX) { put(r.name, std::to_string(r.hi + 1).c_str()); CHECK(env_int(r.name, r.lo, r.hi, r.dflt) == r.dflt); }
    put(r.name, nullptr);
  }
}

int main() {
  for (long long n : {0LL, 1LL, 247LL, 4096LL, 100000000LL}) CHECK(grow_cap(n) == n + n / 8 + 1024);
  CHECK(grow_cap(0) == 1024 && grow_cap(247) == 1301 && grow_cap(100000000LL) == 112501024LL);
  test_buffer<DevBuf<double>, double>();
  test_buffer<PinnedBuf<uint32_t>, uint32_t>();
  test_popbuf();
  test_groups();
  test_handles();
  test_env();
  CHECK(g_live == 0 && g_handles == 0 && g_allocs == g_frees);
  std::printf("HIP_OWNED_OK %ld allocations, %ld frees\n", g_allocs, g_frees);
  return 0;
}

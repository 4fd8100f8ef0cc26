// mcs_ensemble.hip -- K8: per-word mean and sum of squared deviations of the tallies over the iterations of a fixed-profile run,
// accumulated on the device (include/mcs.h, "ensemble statistics").
//
// Every kernel here is elementwise over a sample vector except the two marginal kernels, which reduce the three big histograms
// ([n_grid][ntht+2][nmom+2], momentum fastest) along one index in a FIXED order: no atomics, one thread per output word, so that
// every word is reproducible bit for bit from a serial sum (the build forms no fma: -ffp-contract=off).
//   momentum marginal  thread (z, i) walks the angle index; neighbouring threads read neighbouring words of every row
//   angle marginal     one block per (histogram, zone): tiles of MARG_COLS momentum columns of all rows go through LDS (read along
//                      the momentum index), thread j then adds its row's columns of the tile in ascending order
// A context is seen through mcs_ctx_view.h; its stream carries the work, an event of the accumulator orders successive operations
// that were queued on different streams.
#include <hip/hip_runtime.h>

#include "mcs_ctx_view.h"
#include "mcs_hip_owned.h"

#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

namespace {

constexpr int ENS_THREADS = 256;
constexpr int ENS_MAX_BLOCKS = 2048;       // grid-stride loops: 8 blocks per CU of the chip
constexpr int MARG_ROWS = 256;             // angle rows a block of the angle marginal can hold (ntht + 2 <= MCS_PSD_MAX + 2)
constexpr int MARG_COLS = 16;              // momentum columns per tile: 128 B of every row
constexpr int MARG_PITCH = MARG_COLS + 1;  // LDS row pitch (odd: thread j's reads of one column fall into different banks)

// the never-reset sections inside [esc_flux, energy_recv_pool): half-open ranges of buffer words that enter as increments
struct IncRanges { long long lo[3], hi[3]; };

int grid_for(long long n) {
  const long long b = (n + ENS_THREADS - 1) / ENS_THREADS;
  return (int)(b < 1 ? 1 : (b > ENS_MAX_BLOCKS ? ENS_MAX_BLOCKS : b));
}

__device__ inline void welford(double* mean, double* m2, long long w, double x, double n) {
  const double m0 = mean[w];
  const double d = x - m0;
  const double m1 = m0 + d / n;
  mean[w] = m1;
  m2[w] = m2[w] + d * (x - m1);
}

// out: [3] x { [n_grid][nm] }, at h * marg_stride
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_marg_mom(const double* __restrict__ hist, double* __restrict__ out, long long ng,
                                                                  int nm, int nt, long long marg_stride) {
  const long long per = ng * nm, total = 3 * per, slab = (long long)nm * nt;
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (long long)gridDim.x * blockDim.x) {
    const long long h = w / per, r = w - h * per, z = r / nm, i = r - z * nm;
    const double* p = hist + (h * ng + z) * slab + i;
    double acc = p[0];
    for (int j = 1; j < nt; ++j) acc = acc + p[(long long)j * nm];
    out[h * marg_stride + r] = acc;
  }
}

// out: [3] x { [n_grid][nt] }, at h * marg_stride + n_grid * nm; grid (n_grid, 3), nt <= MARG_ROWS
__global__ void __launch_bounds__(MARG_ROWS) mcs_k_ens_marg_tht(const double* __restrict__ hist, double* __restrict__ out, long long ng,
                                                                int nm, int nt, long long marg_stride) {
  __shared__ double tile[MARG_ROWS * MARG_PITCH];
  const long long z = blockIdx.x, h = blockIdx.y;
  const int t = threadIdx.x;
  const double* src = hist + (h * ng + z) * ((long long)nm * nt);
  double acc = 0.0;
  for (int c0 = 0; c0 < nm; c0 += MARG_COLS) {
    const int ncol = nm - c0 < MARG_COLS ? nm - c0 : MARG_COLS;
    for (int e = t; e < nt * MARG_COLS; e += MARG_ROWS) {
      const int r = e / MARG_COLS, col = e - r * MARG_COLS;
      if (col < ncol) tile[r * MARG_PITCH + col] = src[(long long)r * nm + c0 + col];
    }
    __syncthreads();
    if (t < nt) {
      for (int col = 0; col < ncol; ++col) {
        const double v = tile[t * MARG_PITCH + col];
        acc = (c0 == 0 && col == 0) ? v : acc + v;
      }
    }
    __syncthreads();
  }
  if (t < nt) out[h * marg_stride + ng * nm + z * nt + t] = acc;
}

__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_add_species(double* __restrict__ mean, double* __restrict__ m2, const double* __restrict__ T,
                                                                     const unsigned long long* __restrict__ I, const double* __restrict__ marg,
                                                                     mcs_ens_layout E, double n) {
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < E.sp_total; w += (long long)gridDim.x * blockDim.x) {
    double x;
    if (w < E.sp_recv_pool) x = T[E.tally_sp_first + w];
    else if (w < E.sp_num_crossings) x = T[E.tally_recv_pool + (w - E.sp_recv_pool)];
    else if (w < E.sp_psd_mom) x = (double)(long long)I[w - E.sp_num_crossings];
    else x = marg[w - E.sp_psd_mom];
    welford(mean, m2, w, x, n);
  }
}

__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_add_iteration(double* __restrict__ mean, double* __restrict__ m2, const double* __restrict__ T,
                                                                       const double* __restrict__ snap, mcs_ens_layout E, IncRanges inc, double n) {
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < E.it_total; w += (long long)gridDim.x * blockDim.x) {
    double x;
    if (w < E.it_scalars) {
      const long long tw = E.tally_it_first + w;
      x = T[tw];
      if ((tw >= inc.lo[0] && tw < inc.hi[0]) || (tw >= inc.lo[1] && tw < inc.hi[1]) || (tw >= inc.lo[2] && tw < inc.hi[2])) x = x - snap[w];
    } else {
      x = T[E.tally_scalars + (w - E.it_scalars)];
    }
    welford(mean, m2, w, x, n);
  }
}

// Chan: f_mean = nb / n, f_m2 = na * nb / n (host doubles)
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_merge(double* __restrict__ ma, double* __restrict__ qa, const double* __restrict__ mb,
                                                               const double* __restrict__ qb, long long total, double f_mean, double f_m2) {
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (long long)gridDim.x * blockDim.x) {
    const double a = ma[w];
    const double d = mb[w] - a;
    ma[w] = a + d * f_mean;
    qa[w] = (qa[w] + qb[w]) + (d * d) * f_m2;
  }
}

__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_load_mean(const double* __restrict__ mean, double* __restrict__ T, unsigned long long* __restrict__ I,
                                                                   mcs_ens_layout E) {
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < E.sp_psd_mom; w += (long long)gridDim.x * blockDim.x) {
    const double x = mean[w];
    if (w < E.sp_recv_pool) T[E.tally_sp_first + w] = x;
    else if (w < E.sp_num_crossings) T[E.tally_recv_pool + (w - E.sp_recv_pool)] = x;
    else I[w - E.sp_num_crossings] = (unsigned long long)__double2ll_rn(x);
  }
}

int fail(const std::string& msg) { return mcs_ctx_view_fail(msg.c_str()); }
#define ENSCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

void ens_layout(const mcs_params* p, mcs_ens_layout* E) {
  mcs_layout L;
  mcs_tally_layout(p, &L);
  const int64_t ng = p->n_grid, nm = p->num_psd_mom_bins + 2, nt = p->num_psd_tht_bins + 2;
  int64_t o = 0;
  E->sp_tallies = o;       E->sp_tallies_n = L.esc_flux - L.psd;  o += E->sp_tallies_n;
  E->sp_recv_pool = o;     E->sp_recv_pool_n = ng;                o += ng;
  E->sp_num_crossings = o; E->sp_num_crossings_n = ng;            o += ng;
  E->sp_marg_mom_n = ng * nm; E->sp_marg_tht_n = ng * nt;
  E->sp_psd_mom = o;       o += ng * nm;
  E->sp_psd_tht = o;       o += ng * nt;
  E->sp_therm_sf_mom = o;  o += ng * nm;
  E->sp_therm_sf_tht = o;  o += ng * nt;
  E->sp_therm_pf_mom = o;  o += ng * nm;
  E->sp_therm_pf_tht = o;  o += ng * nt;
  E->sp_total = o;
  E->it_sums = 0;          E->it_sums_n = L.energy_recv_pool - L.esc_flux;
  E->it_scalars = E->it_sums_n; E->it_scalars_n = L.total - L.scalars;
  E->it_total = E->it_scalars + E->it_scalars_n;
  E->tally_sp_first = L.psd; E->tally_it_first = L.esc_flux; E->tally_recv_pool = L.energy_recv_pool; E->tally_scalars = L.scalars;
}

}  // namespace

struct mcs_ens {
  int device = 0;
  mcs_ctx* home = nullptr;
  mcs_params P;
  mcs_layout L;
  mcs_ens_layout E;
  IncRanges inc;
  int n_slots = 0;                            // the species slots and, last, the iteration slot
  std::vector<long long> n;                   // samples of every slot
  std::vector<DevBuf<double>> mean, m2;       // per slot: sp_total (it_total for the last) doubles each
  DevBuf<double> marg;                        // the marginals of the sample being added (part 4)
  DevBuf<double> snap;                        // [esc_flux, energy_recv_pool) of snap_of at the last begin-iteration call
  mcs_ctx* snap_of = nullptr;                 // (null: no snapshot since the last iteration sample)
  Event ev;                                   // recorded after every operation on the stream that carried it
  bool ev_set = false;
  long long len(int slot) const { return slot == n_slots - 1 ? E.it_total : E.sp_total; }
};

namespace {

// ctx is on the accumulator's device and has its layout -> its view, replicas folded in
int view_of(mcs_ens* e, mcs_ctx* ctx, const char* who, McsCtxView* v) {
  // (a refused call leaves *v as it was; the fold that the view queues changes no tally a reader sees)
  McsCtxView probe;
  if (mcs_ctx_view_get(ctx, &probe)) return 1;
  if (probe.device != e->device) return fail(std::string(who) + ": the context is on another device than the accumulator");
  if (probe.L.total != e->L.total || probe.P.n_grid != e->P.n_grid || probe.P.n_ions != e->P.n_ions || probe.P.n_itrs != e->P.n_itrs ||
      probe.P.num_psd_mom_bins != e->P.num_psd_mom_bins || probe.P.num_psd_tht_bins != e->P.num_psd_tht_bins)
    return fail(std::string(who) + ": the context's tally layout differs from the accumulator's");
  *v = probe;
  return 0;
}

int enter(mcs_ens* e, hipStream_t st) {
  if (e->ev_set) ENSCHK(hipStreamWaitEvent(st, e->ev, 0));
  return 0;
}
int leave(mcs_ens* e, hipStream_t st) {
  ENSCHK(hipEventRecord(e->ev, st));
  e->ev_set = true;
  return 0;
}

}  // namespace

extern "C" {

int mcs_ens_get_layout(const mcs_params* p, mcs_ens_layout* out) {
  if (!p || !out) return fail("mcs_ens_get_layout: null argument");
  ens_layout(p, out);
  return 0;
}

int mcs_ens_create(mcs_ctx* home, int n_species_slots, mcs_ens** out) {
  if (!home || !out) return fail("mcs_ens_create: null argument");
  if (n_species_slots < 0 || n_species_slots > 4096) return fail("mcs_ens_create: n_species_slots outside 0..4096");
  McsCtxView v;
  if (mcs_ctx_view_get(home, &v)) return 1;
  if (v.P.num_psd_tht_bins + 2 > MARG_ROWS) return fail("mcs_ens_create: more angle bins than the angle-marginal kernel holds");
  std::unique_ptr<mcs_ens> e(new mcs_ens());
  e->device = v.device; e->home = home; e->P = v.P; e->L = v.L;
  ens_layout(&v.P, &e->E);
  const mcs_layout& L = v.L;
  e->inc = IncRanges{{L.esc_flux, L.esc_energy_eff, L.spectra_coupled}, {L.px_esc_feb, L.weight_coupled, L.energy_transfer_pool}};
  e->n_slots = n_species_slots + 1;
  e->n.assign((size_t)e->n_slots, 0);
  e->mean.resize((size_t)e->n_slots); e->m2.resize((size_t)e->n_slots);
  for (int s = 0; s < e->n_slots; ++s) {
    const long long len = e->len(s);
    for (DevBuf<double>* b : {&e->mean[(size_t)s], &e->m2[(size_t)s]}) {
      const hipError_t a = b->reserve(len);
      if (a != hipSuccess) return fail(std::string("mcs_ens_create: hipMalloc: ") + hipGetErrorString(a));
      ENSCHK(hipMemsetAsync(b->get(), 0, (size_t)len * sizeof(double), v.stream));
    }
  }
  hipError_t a = e->marg.reserve(e->E.sp_total - e->E.sp_psd_mom);
  if (a == hipSuccess) a = e->snap.reserve(e->E.it_sums_n);
  if (a != hipSuccess) return fail(std::string("mcs_ens_create: hipMalloc: ") + hipGetErrorString(a));
  ENSCHK(e->ev.create_untimed());
  if (leave(e.get(), v.stream)) return 1;
  *out = e.release();
  return 0;
}

int mcs_ens_destroy(mcs_ens* e) {
  if (!e) return 0;
  (void)hipSetDevice(e->device);
  if (e->ev_set) (void)hipEventSynchronize(e->ev);      // (nothing queued may still use the buffers)
  delete e;
  return 0;
}

int mcs_ens_begin_iteration(mcs_ens* e, mcs_ctx* src) {
  if (!e || !src) return fail("mcs_ens_begin_iteration: null argument");
  McsCtxView v;
  if (view_of(e, src, "mcs_ens_begin_iteration", &v)) return 1;
  if (enter(e, v.stream)) return 1;
  ENSCHK(hipMemcpyAsync(e->snap, v.T + e->E.tally_it_first, (size_t)e->E.it_sums_n * sizeof(double), hipMemcpyDeviceToDevice, v.stream));
  e->snap_of = src;
  return leave(e, v.stream);
}

int mcs_ens_add_species(mcs_ens* e, mcs_ctx* src, int slot) {
  if (!e || !src) return fail("mcs_ens_add_species: null argument");
  if (slot < 0 || slot >= e->n_slots) return fail("mcs_ens_add_species: slot " + std::to_string(slot) + " outside 0.." + std::to_string(e->n_slots - 1));
  if (slot == e->n_slots - 1) return fail("mcs_ens_add_species: slot " + std::to_string(slot) + " is the iteration slot; it takes no species sample");
  McsCtxView v;
  if (view_of(e, src, "mcs_ens_add_species", &v)) return 1;
  if (enter(e, v.stream)) return 1;
  const mcs_ens_layout& E = e->E;
  const int nm = e->P.num_psd_mom_bins + 2, nt = e->P.num_psd_tht_bins + 2;
  const long long ng = e->P.n_grid, marg_stride = E.sp_marg_mom_n + E.sp_marg_tht_n;
  hipLaunchKernelGGL(mcs_k_ens_marg_mom, dim3(grid_for(3 * E.sp_marg_mom_n)), dim3(ENS_THREADS), 0, v.stream, v.T + e->L.psd, e->marg.get(), ng, nm, nt,
                     marg_stride);
  ENSCHK(hipGetLastError());
  hipLaunchKernelGGL(mcs_k_ens_marg_tht, dim3((unsigned)ng, 3), dim3(MARG_ROWS), 0, v.stream, v.T + e->L.psd, e->marg.get(), ng, nm, nt, marg_stride);
  ENSCHK(hipGetLastError());
  const long long n = e->n[(size_t)slot] + 1;
  hipLaunchKernelGGL(mcs_k_ens_add_species, dim3(grid_for(E.sp_total)), dim3(ENS_THREADS), 0, v.stream, e->mean[(size_t)slot].get(), e->m2[(size_t)slot].get(),
                     v.T, v.I, e->marg.get(), E, (double)n);
  ENSCHK(hipGetLastError());
  e->n[(size_t)slot] = n;
  return leave(e, v.stream);
}

int mcs_ens_add_iteration(mcs_ens* e, mcs_ctx* src) {
  if (!e || !src) return fail("mcs_ens_add_iteration: null argument");
  McsCtxView v;
  if (view_of(e, src, "mcs_ens_add_iteration", &v)) return 1;
  if (e->snap_of != src) return fail("mcs_ens_add_iteration: no mcs_ens_begin_iteration snapshot of this context since the last iteration sample");
  if (enter(e, v.stream)) return 1;
  const int slot = e->n_slots - 1;
  const long long n = e->n[(size_t)slot] + 1;
  hipLaunchKernelGGL(mcs_k_ens_add_iteration, dim3(grid_for(e->E.it_total)), dim3(ENS_THREADS), 0, v.stream, e->mean[(size_t)slot].get(),
                     e->m2[(size_t)slot].get(), v.T, e->snap.get(), e->E, e->inc, (double)n);
  ENSCHK(hipGetLastError());
  e->n[(size_t)slot] = n;
  e->snap_of = nullptr;
  return leave(e, v.stream);
}

int mcs_ens_merge(mcs_ens* dst, mcs_ens* src) {
  if (!dst || !src) return fail("mcs_ens_merge: null argument");
  if (dst == src) return fail("mcs_ens_merge: dst and src are the same accumulator");
  if (dst->device != src->device) return fail("mcs_ens_merge: the accumulators are on different devices");
  if (dst->n_slots != src->n_slots || dst->E.sp_total != src->E.sp_total || dst->E.it_total != src->E.it_total || dst->L.total != src->L.total ||
      dst->P.n_grid != src->P.n_grid || dst->P.n_ions != src->P.n_ions || dst->P.n_itrs != src->P.n_itrs)
    return fail("mcs_ens_merge: the accumulators' slots or layouts differ");
  McsCtxView v;
  if (mcs_ctx_view_get(dst->home, &v)) return 1;
  if (enter(dst, v.stream) || enter(src, v.stream)) return 1;
  for (int s = 0; s < dst->n_slots; ++s) {
    const long long na = dst->n[(size_t)s], nb = src->n[(size_t)s], len = dst->len(s);
    if (nb == 0) continue;
    if (na == 0) {
      ENSCHK(hipMemcpyAsync(dst->mean[(size_t)s], src->mean[(size_t)s], (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, v.stream));
      ENSCHK(hipMemcpyAsync(dst->m2[(size_t)s], src->m2[(size_t)s], (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, v.stream));
    } else {
      const double n = (double)(na + nb);
      hipLaunchKernelGGL(mcs_k_ens_merge, dim3(grid_for(len)), dim3(ENS_THREADS), 0, v.stream, dst->mean[(size_t)s].get(), dst->m2[(size_t)s].get(),
                         src->mean[(size_t)s].get(), src->m2[(size_t)s].get(), len, (double)nb / n, (double)na * (double)nb / n);
      ENSCHK(hipGetLastError());
    }
    dst->n[(size_t)s] = na + nb;
  }
  if (leave(dst, v.stream)) return 1;
  return leave(src, v.stream);
}

int mcs_ens_count(mcs_ens* e, int slot, int64_t* n) {
  if (!e || !n) return fail("mcs_ens_count: null argument");
  if (slot < 0 || slot >= e->n_slots) return fail("mcs_ens_count: slot " + std::to_string(slot) + " outside 0.." + std::to_string(e->n_slots - 1));
  *n = e->n[(size_t)slot];
  return 0;
}

int mcs_ens_read(mcs_ens* e, int slot, int what, int64_t first, int64_t count, double* host) {
  if (!e || (count > 0 && !host)) return fail("mcs_ens_read: null argument");
  if (slot < 0 || slot >= e->n_slots) return fail("mcs_ens_read: slot " + std::to_string(slot) + " outside 0.." + std::to_string(e->n_slots - 1));
  if (what < 0 || what > 2) return fail("mcs_ens_read: what must be 0 (mean), 1 (M2) or 2 (standard error)");
  if (first < 0 || count < 0 || first + count > e->len(slot)) return fail("mcs_ens_read: range outside the slot's sample vector");
  const long long n = e->n[(size_t)slot];
  if (what == 2 && n < 2) return fail("mcs_ens_read: the standard error needs at least two samples; the slot has " + std::to_string(n));
  McsCtxView v;
  if (mcs_ctx_view_get(e->home, &v)) return 1;
  if (enter(e, v.stream)) return 1;
  const double* from = what == 0 ? e->mean[(size_t)slot].get() : e->m2[(size_t)slot].get();
  if (count > 0) ENSCHK(hipMemcpyAsync(host, from + first, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  ENSCHK(hipStreamSynchronize(v.stream));
  if (what == 2) {
    const double denom = (double)n * (double)(n - 1);
    for (int64_t k = 0; k < count; ++k) host[k] = std::sqrt(host[k] / denom);
  }
  return 0;
}

int mcs_ens_load_mean(mcs_ens* e, int slot, mcs_ctx* dst) {
  if (!e || !dst) return fail("mcs_ens_load_mean: null argument");
  if (slot < 0 || slot >= e->n_slots) return fail("mcs_ens_load_mean: slot " + std::to_string(slot) + " outside 0.." + std::to_string(e->n_slots - 1));
  if (slot == e->n_slots - 1) return fail("mcs_ens_load_mean: slot " + std::to_string(slot) + " is the iteration slot; only a species slot has histograms");
  McsCtxView v;
  if (view_of(e, dst, "mcs_ens_load_mean", &v)) return 1;
  if (enter(e, v.stream)) return 1;
  hipLaunchKernelGGL(mcs_k_ens_load_mean, dim3(grid_for(e->E.sp_psd_mom)), dim3(ENS_THREADS), 0, v.stream, e->mean[(size_t)slot].get(), v.T, v.I, e->E);
  ENSCHK(hipGetLastError());
  mcs_ctx_view_tallies_written(dst);
  return leave(e, v.stream);
}

}  // extern "C"

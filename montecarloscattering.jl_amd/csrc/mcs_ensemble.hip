// mcs_ensemble.hip -- K8: per-word mean and sum of squared deviations of the tallies over the iterations of a fixed-profile run,
// accumulated on the device (include/mcs.h, "ensemble statistics").
//
// Every kernel here is elementwise over a sample vector except the two marginal kernels, which reduce the three big histograms
// ([n_grid][ntht+2][nmom+2], momentum fastest) along one index in a FIXED order: no atomics, one thread per output word, so that
// every word is reproducible bit for bit from a serial sum (the build forms no fma: -ffp-contract=off).
//   momentum marginal  thread (z, i) walks the angle index; neighbouring threads read neighbouring words of every row
//   angle marginal     one block per (histogram, zone): tiles of MARG_COLS momentum columns of all rows go through LDS (read along
//                      the momentum index), thread j then adds its row's columns of the tile in ascending order
// The summary of word ranges (mcs_ens_summarize) is the one reduction to a handful of numbers: two sweeps over every range -- the
// largest |mean|, then the relative errors of the words that pass the floor it sets -- each thread over its words in ascending
// order, then per wave by shuffles, per block through LDS, one partial per block into a scratch buffer of the accumulator, and a
// last kernel that folds a range's partials in index order.  No atomics: the same state gives the same bits.
// The comparison of two slots (mcs_ens_compare) is the same walk over the (mean, M2) pairs of both with a record of its own: the
// four sweep kernels share one routine, walk, for which words a thread sees and in which order.
// Host side: every slot of every kind -- species, iteration, products, photons, source, escape, angles, tcuts, profile, detectors -- is one Slot (count, mean, M2); decode reads
// a slot number's bits, slot_ref finds its Slot, reserve allocates it, merge_slot merges it, and plan_ranges checks the ranges of a
// summary or comparison and lays out their blocks in one pass.
// A context is seen through mcs_ctx_view.h; its stream carries the work, an event of the accumulator orders successive operations
// that were queued on different streams.
#include <hip/hip_runtime.h>

#include "mcs_ctx_view.h"
#include "mcs_hip_owned.h"
#include "mcs_slope.h"
#include "../../include/mcs_math.h"

#include <climits>
#include <cstddef>
#include <cmath>
#include <cstdio>
#include <cstring>
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

// The slope of log10 dN/dp against x_log over the window's valid bins (include/mcs.h, "products sample"): one thread per
// (frame, zone) row of dndp [3 * ng][nm], its sums serial in ascending bin order.  A row is read three times (count and sums, then
// the squares about the means); log10 gives the same bits each time.  3 * ng rows of at most nm - 1 bins: a few hundred threads, each
// on a row of its own -- too little work to be worth a wave per row and the fixed-order join that would need.
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_slope(const double* __restrict__ dndp, const double* __restrict__ x_log,
                                                               double* __restrict__ slope, long long rows, int nm, int l_lo, int l_hi) {
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (long long)gridDim.x * blockDim.x) {
    const double* row = dndp + r * nm;
    slope[r] = mcs_slope_rule(l_lo, l_hi, [&](int l) { return row[l] > 1.0e-99; }, [&](int l) { return x_log[l]; },
                              [&](int l) { return mcsm::log10(row[l]); });
  }
}

// cout: the context's consumer output buffer, n_cout = 3 ng nm + 3 ng words; the last 3 ng words of the sample are the slopes
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_add_products(double* __restrict__ mean, double* __restrict__ m2, const double* __restrict__ cout,
                                                                      const double* __restrict__ slope, long long n_cout, long long total, double n) {
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (long long)gridDim.x * blockDim.x)
    welford(mean, m2, w, w < n_cout ? cout[w] : slope[w - n_cout], n);
}

// The photons sample (include/mcs.h, "photons sample"): sections synch | ic | pion, each [rows][n_p] as mcs_photon_observe left it on
// the context (a null pointer: the process was not observed, every word 1e-99), then total [rows][n_pts].  A word of the total is
// recomputed from the three sections by the thread that owns it: a shell row adds, to 1e-99, the lit words of pion decay, synchrotron
// and inverse Compton in that order; the last row is the serial sum of the shell rows as they stand.
struct PhotonSrc { const double* obs[3]; long long off[4]; int n[3], start[3]; int n_shells, n_pts; long long total; };
__device__ inline double photon_total_word(const PhotonSrc& S, int s, int t) {
  double x = 1.0e-99;
  const int order[3] = {MCS_PHOTON_PION, MCS_PHOTON_SYNCH, MCS_PHOTON_IC};
  for (int q = 0; q < 3; ++q) {
    const int p = order[q];
    if (!S.obs[p] || t < S.start[p] || t >= S.start[p] + S.n[p]) continue;
    const double sh = S.obs[p][(long long)s * S.n[p] + (t - S.start[p])];
    x = x + (sh > 1.0e-99 ? sh : 0.0);
  }
  return x;
}
// word w of the sample: the one place where it is formed, for the plain sample and for the one that also deposits
__device__ inline double photon_sample_word(const PhotonSrc& S, long long w) {
  if (w < S.off[3]) {
    const int p = w < S.off[1] ? 0 : w < S.off[2] ? 1 : 2;
    return S.obs[p] ? S.obs[p][w - S.off[p]] : 1.0e-99;
  }
  const int s = (int)((w - S.off[3]) / S.n_pts), t = (int)((w - S.off[3]) % S.n_pts);
  if (s < S.n_shells) return photon_total_word(S, s, t);
  double x = 0.0;
  for (int r = 0; r < S.n_shells; ++r) x = x + photon_total_word(S, r, t);
  return x;
}
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_add_photons(double* __restrict__ mean, double* __restrict__ m2, PhotonSrc S, double n) {
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < S.total; w += (long long)gridDim.x * blockDim.x)
    welford(mean, m2, w, photon_sample_word(S, w), n);
}

// The same sample, and its deposit into the pending vector of the source slot (include/mcs.h, "source sample"): the word is formed
// once, updates the species' photons slot, and its lit part joins pending[w] -- which the first deposit since the last take starts
// at 1e-99 without reading it.  Uniform over the four sections, the all-shells rows included.
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_add_photons_deposit(double* __restrict__ mean, double* __restrict__ m2, PhotonSrc S, double n,
                                                                             double* __restrict__ pending, int first) {
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < S.total; w += (long long)gridDim.x * blockDim.x) {
    const double x = photon_sample_word(S, w);
    welford(mean, m2, w, x, n);
    const double base = first ? 1.0e-99 : pending[w];
    pending[w] = base + (x > 1.0e-99 ? x : 0.0);
  }
}

// a sample that lies on the device as a vector (the source sample: the pending vector)
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_add_vector(double* __restrict__ mean, double* __restrict__ m2, const double* __restrict__ x,
                                                                    long long total, double n) {
  for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (long long)gridDim.x * blockDim.x)
    welford(mean, m2, w, x[w], n);
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

// ---- the summary of word ranges --------------------------------------------------------------------------------------------
constexpr int SUM_MAX_RANGES = 256;
constexpr int SUM_CHUNK = 4096;            // words of a range per block (16 per thread) before a range gets ...
constexpr int SUM_MAX_BLOCKS = 2048;       // ... this many blocks, which then stride on: 8 per CU
constexpr int SUM_WAVES = ENS_THREADS / 64;

struct SumRange { long long first, count; double floor_frac, tol; };
// block b of the launch works on range r, off[r] <= b < off[r + 1], as its block b - off[r] (a range of no words has no block)
struct SumParams { SumRange r[SUM_MAX_RANGES]; int off[SUM_MAX_RANGES + 1]; int n_ranges; };
// What a thread, a wave, a block, a range has seen.  amax: over the finite words; amax_used: the one the selection was made with;
// arg: LLONG_MAX while nothing is selected (max_rel is then -1: every relative error beats it).
struct SumRec { double amax, amax_used, max_rel, sum_se, sum_abs, sum_rel2; long long n_sel, n_over, n_nonf, arg; };

__device__ inline SumRec rec_empty(double amax_used) { return SumRec{0.0, amax_used, -1.0, 0.0, 0.0, 0.0, 0, 0, 0, LLONG_MAX}; }

__device__ inline bool finite_(double x) {
  return (__double_as_longlong(x) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}

// b joins a; a holds the words (or partials) before b's: the sums add in that order, equal relative errors keep the lower word
__device__ inline void rec_join(SumRec& a, const SumRec& b) {
  a.amax = b.amax > a.amax ? b.amax : a.amax;
  if (b.max_rel > a.max_rel || (b.max_rel == a.max_rel && b.arg < a.arg)) { a.max_rel = b.max_rel; a.arg = b.arg; }
  a.sum_se = a.sum_se + b.sum_se;
  a.sum_abs = a.sum_abs + b.sum_abs;
  a.sum_rel2 = a.sum_rel2 + b.sum_rel2;
  a.n_sel += b.n_sel; a.n_over += b.n_over; a.n_nonf += b.n_nonf;
}

__device__ inline SumRec rec_shfl_down(const SumRec& v, int d) {
  SumRec o;
  o.amax = __shfl_down(v.amax, d, 64); o.amax_used = v.amax_used; o.max_rel = __shfl_down(v.max_rel, d, 64);
  o.sum_se = __shfl_down(v.sum_se, d, 64); o.sum_abs = __shfl_down(v.sum_abs, d, 64); o.sum_rel2 = __shfl_down(v.sum_rel2, d, 64);
  o.n_sel = __shfl_down(v.n_sel, d, 64); o.n_over = __shfl_down(v.n_over, d, 64); o.n_nonf = __shfl_down(v.n_nonf, d, 64);
  o.arg = __shfl_down(v.arg, d, 64);
  return o;
}

// the block's threads' records joined in a fixed order -> thread 0's v (a binary tree over the lanes of a wave, then the waves
// in order); tmp: SUM_WAVES records of LDS.  Rec: SumRec, or the CmpRec of the comparison below, with its rec_join / rec_shfl_down
template <class Rec>
__device__ inline void rec_block_join(Rec& v, Rec* tmp) {
  const int lane = threadIdx.x & 63;
  for (int d = 1; d < 64; d <<= 1) {
    const Rec o = rec_shfl_down(v, d);
    if ((lane & (2 * d - 1)) == 0) rec_join(v, o);      // (lane + d holds the lanes lane + d .. lane + 2 d - 1)
  }
  if (lane == 0) tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < SUM_WAVES; ++k) rec_join(v, tmp[k]);
}

__device__ inline double block_max(double v, double* tmp) {      // -> every thread
  for (int d = 32; d > 0; d >>= 1) { const double o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
  if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  double m = tmp[0];
  for (int k = 1; k < SUM_WAVES; ++k) m = tmp[k] > m ? tmp[k] : m;
  __syncthreads();
  return m;
}

__device__ inline int range_of_block(const SumParams* __restrict__ P, int b) {
  int lo = 0, hi = P->n_ranges;                     // off[lo] <= b < off[hi]
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (P->off[mid] <= b) lo = mid; else hi = mid; }
  return lo;
}

// A block's words of the range [first, first + count): the whole 16-byte pairs inside it, pair j for the block's thread
// j mod (blocks * ENS_THREADS); the odd word at either end goes to thread 0 of the range's first block.  A thread sees its words
// in ascending order.
struct SumSpan { long long first, count, pair0, n_pairs, j0, stride; bool ends; };
__device__ inline SumSpan span_of(const SumRange& R, int blk, int n_blk) {
  SumSpan s;
  s.first = R.first; s.count = R.count;
  const long long a0 = (R.first + 1) & ~1LL, a1 = (R.first + R.count) & ~1LL;
  s.pair0 = a0 >> 1; s.n_pairs = a1 > a0 ? (a1 - a0) >> 1 : 0;
  s.j0 = (long long)blk * ENS_THREADS + threadIdx.x; s.stride = (long long)n_blk * ENS_THREADS;
  s.ends = blk == 0 && threadIdx.x == 0;
  return s;
}

// Where the sweeps take a word's (mean, M2) from.  A source says how many pairs a thread loads before it looks at them (LOADS);
// which words a thread sees, and in which order, is the business of span_of and walk alone, the same for every source.
//   SrcOne         the two vectors of one accumulator
//   SrcMerged<N>   the Chan merge of N >= 2 accumulators, folded per word in registers in list order with the factors of every
//                  step (f_mean[k] = nb / n, f_m2[k] = na * nb / n, host doubles as in mcs_k_ens_merge); nothing is written back
struct SrcOne {
  static constexpr int LOADS = 4;
  const double* mean; const double* m2;
  __device__ double mean_at(long long w) const { return mean[w]; }
  __device__ double2 mean_pair(long long p) const { return reinterpret_cast<const double2*>(mean)[p]; }
  __device__ void at(long long w, double& m, double& q) const { m = mean[w]; q = m2[w]; }
  __device__ void pair(long long p, double2& m, double2& q) const {
    m = reinterpret_cast<const double2*>(mean)[p]; q = reinterpret_cast<const double2*>(m2)[p];
  }
};

template <int N>
struct SrcMerged {
  // One pair in flight per thread and sweep whatever N is: a pair already costs 2 N loads of 16 bytes, and the registers that
  // LOADS > 1 would take grow with N.  For N = 2 that is half the bytes SrcOne keeps in flight; no other value has been measured.
  static constexpr int LOADS = 1;
  const double* mean[N]; const double* m2[N];
  double f_mean[N], f_m2[N];               // [0] unused: accumulator 0 is the fold's start
  // Step k of the fold: accumulator k's word (x, y) joins (m, q).  The one place where the formula stands: both sweeps, pairs and
  // single words, go through it, so a word's merged mean has the same bits wherever it is computed (a caller that wants the mean
  // only passes a q it throws away).
  __device__ void step(double& m, double& q, double x, double y, int k) const {
    const double d = x - m;
    m = m + d * f_mean[k];
    q = (q + y) + (d * d) * f_m2[k];
  }
  __device__ double mean_at(long long w) const {
    double x[N];
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = mean[k][w];
    double m = x[0], q = 0.0;
#pragma unroll
    for (int k = 1; k < N; ++k) step(m, q, x[k], 0.0, k);
    return m;
  }
  __device__ double2 mean_pair(long long p) const {
    double2 x[N];
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = reinterpret_cast<const double2*>(mean[k])[p];
    double2 m = x[0], q = {0.0, 0.0};
#pragma unroll
    for (int k = 1; k < N; ++k) { step(m.x, q.x, x[k].x, 0.0, k); step(m.y, q.y, x[k].y, 0.0, k); }
    return m;
  }
  __device__ void at(long long w, double& m, double& q) const {
    double x[N], y[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { x[k] = mean[k][w]; y[k] = m2[k][w]; }
    m = x[0]; q = y[0];
#pragma unroll
    for (int k = 1; k < N; ++k) step(m, q, x[k], y[k], k);
  }
  __device__ void pair(long long p, double2& m, double2& q) const {
    double2 x[N], y[N];
#pragma unroll
    for (int k = 0; k < N; ++k) { x[k] = reinterpret_cast<const double2*>(mean[k])[p]; y[k] = reinterpret_cast<const double2*>(m2[k])[p]; }
    m = x[0]; q = y[0];
#pragma unroll
    for (int k = 1; k < N; ++k) { step(m.x, q.x, x[k].x, y[k].x, k); step(m.y, q.y, x[k].y, y[k].y, k); }
  }
};

// The one walk of a thread over its words of a span, which all four sweeps take: the odd word in front, U pairs at a time (all
// loaded before any is looked at), the pairs that are left, the odd word at the end.  rd reads a single word (at) or a 16-byte pair
// of every vector it covers (pair; lo / hi: its two words); see(i, word) gets every word with its index i in the range.
template <int U, class Reader, class See>
__device__ inline void walk(const SumSpan& s, const Reader& rd, See&& see) {
  const long long i0 = 2 * s.pair0 - s.first;        // word index - first of pair 0's first word
  if (s.ends && (s.first & 1)) see(0, rd.at(s.first));
  long long j = s.j0;
  for (; j + (U - 1) * s.stride < s.n_pairs; j += U * s.stride) {
    typename Reader::Pair p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) p[u] = rd.pair(s.pair0 + j + u * s.stride);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long ju = j + u * s.stride;
      see(i0 + 2 * ju, rd.lo(p[u])); see(i0 + 2 * ju + 1, rd.hi(p[u]));
    }
  }
  for (; j < s.n_pairs; j += s.stride) {
    const typename Reader::Pair p = rd.pair(s.pair0 + j);
    see(i0 + 2 * j, rd.lo(p)); see(i0 + 2 * j + 1, rd.hi(p));
  }
  if (s.ends && ((s.first + s.count) & 1) && s.count > (s.first & 1)) see(s.count - 1, rd.at(s.first + s.count - 1));
}

// the readers of a summary's source: the means alone (sweep 1), mean and M2 (sweep 2)
template <class Src>
struct ReadMean {
  using Pair = double2;
  const Src& src;
  __device__ double at(long long w) const { return src.mean_at(w); }
  __device__ double2 pair(long long p) const { return src.mean_pair(p); }
  __device__ double lo(const double2& p) const { return p.x; }
  __device__ double hi(const double2& p) const { return p.y; }
};
struct MeanM2 { double m, q; };
template <class Src>
struct ReadBoth {
  struct Pair { double2 m, q; };
  const Src& src;
  __device__ MeanM2 at(long long w) const { MeanM2 r; src.at(w, r.m, r.q); return r; }
  __device__ Pair pair(long long p) const { Pair r; src.pair(p, r.m, r.q); return r; }
  __device__ MeanM2 lo(const Pair& p) const { return MeanM2{p.m.x, p.q.x}; }
  __device__ MeanM2 hi(const Pair& p) const { return MeanM2{p.m.y, p.q.y}; }
};

// sweep 1: the largest |mean| over the words whose mean is finite, per block
template <class Src>
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_sum_amax(const Src src, const SumParams* __restrict__ P, double* __restrict__ pmax) {
  __shared__ double tmp[SUM_WAVES];
  const int r = range_of_block(P, blockIdx.x), o0 = P->off[r];
  const SumSpan s = span_of(P->r[r], blockIdx.x - o0, P->off[r + 1] - o0);
  double a = 0.0;
  walk<Src::LOADS>(s, ReadMean<Src>{src}, [&](long long, double m) { const double x = fabs(m); if (finite_(m) && x > a) a = x; });
  a = block_max(a, tmp);
  if (threadIdx.x == 0) pmax[blockIdx.x] = a;
}

// sweep 2: with amax_used = the largest of the range's pmax, the record of the block's words
template <class Src>
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_sum_stats(const Src src, const SumParams* __restrict__ P, const double* __restrict__ pmax,
                                                                   SumRec* __restrict__ part, double denom) {
  __shared__ double tmp[SUM_WAVES];
  __shared__ SumRec rtmp[SUM_WAVES];
  const int r = range_of_block(P, blockIdx.x), o0 = P->off[r], n_blk = P->off[r + 1] - o0;
  const SumRange R = P->r[r];
  const SumSpan s = span_of(R, blockIdx.x - o0, n_blk);
  double a = 0.0;
  for (int k = threadIdx.x; k < n_blk; k += ENS_THREADS) { const double x = pmax[o0 + k]; a = x > a ? x : a; }
  const double amax_used = block_max(a, tmp);
  const double floor_abs = R.floor_frac * amax_used, tol = R.tol;
  SumRec v = rec_empty(amax_used);
  walk<Src::LOADS>(s, ReadBoth<Src>{src}, [&](long long idx, const MeanM2& w) {
    const double m = w.m, q = w.q;
    if (!finite_(m) || !finite_(q)) { v.n_nonf += 1; return; }
    const double x = fabs(m);
    v.amax = x > v.amax ? x : v.amax;
    if (x > 0.0 && x >= floor_abs) {
      const double se = mcsm::sqrt_(q / denom);
      const double rel = se / x;
      v.n_sel += 1;
      if (rel > tol) v.n_over += 1;
      v.sum_se = v.sum_se + se;
      v.sum_abs = v.sum_abs + x;
      v.sum_rel2 = v.sum_rel2 + rel * rel;
      if (rel > v.max_rel || (rel == v.max_rel && idx < v.arg)) { v.max_rel = rel; v.arg = idx; }
    }
  });
  rec_block_join(v, rtmp);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// one block per range: its partials joined in index order (thread t: t, t + ENS_THREADS, ..; then the block's tree).  The
// range's pmax become amax of the finite words: a second sweep 2, needed when that is not what the first one used, finds it there.
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_sum_final(const SumParams* __restrict__ P, const SumRec* __restrict__ part,
                                                                   double* __restrict__ pmax, SumRec* __restrict__ out) {
  __shared__ SumRec rtmp[SUM_WAVES];
  __shared__ double amax;
  const int r = blockIdx.x, o0 = P->off[r], o1 = P->off[r + 1];
  SumRec v = rec_empty(0.0);
  for (int k = o0 + threadIdx.x; k < o1; k += ENS_THREADS) rec_join(v, part[k]);
  rec_block_join(v, rtmp);
  if (threadIdx.x == 0) {
    v.amax_used = o1 > o0 ? part[o0].amax_used : 0.0;
    if (v.arg == LLONG_MAX) { v.arg = -1; v.max_rel = v.n_sel > 0 ? __builtin_nan("") : 0.0; }
    out[r] = v;
    amax = v.amax;
  }
  __syncthreads();
  for (int k = o0 + threadIdx.x; k < o1; k += ENS_THREADS) pmax[k] = amax;
}

// ---- the comparison of two slots (mcs_ens_compare) -------------------------------------------------------------------------
// The walk of the summary -- span_of, range_of_block, SumParams (a range's tol holds its zcut), pmax, the joins -- over the words of
// TWO (mean, M2) pairs with another record.  Both sweeps read all four words of a word: whether it is finite depends on all of
// them, so sweep 1 takes amax over exactly the words that sweep 2 calls finite and no sweep is ever repeated.
// arg: LLONG_MAX while no z has been seen (max_z is then -1: every |z| beats it).  amax: the one the selection was made with.
struct CmpRec { double amax, max_z, sum_z, sum_abs_z, sum_z2, sum_diff, sum_scale; long long n_sel, n_over, n_nonf, n_degen, arg; };

__device__ inline CmpRec cmp_empty(double amax) { return CmpRec{amax, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, LLONG_MAX}; }

// b joins a; a holds the words (or partials) before b's: the sums add in that order, equal |z| keep the lower word
__device__ inline void rec_join(CmpRec& a, const CmpRec& b) {
  if (b.max_z > a.max_z || (b.max_z == a.max_z && b.arg < a.arg)) { a.max_z = b.max_z; a.arg = b.arg; }
  a.sum_z = a.sum_z + b.sum_z;
  a.sum_abs_z = a.sum_abs_z + b.sum_abs_z;
  a.sum_z2 = a.sum_z2 + b.sum_z2;
  a.sum_diff = a.sum_diff + b.sum_diff;
  a.sum_scale = a.sum_scale + b.sum_scale;
  a.n_sel += b.n_sel; a.n_over += b.n_over; a.n_nonf += b.n_nonf; a.n_degen += b.n_degen;
}

__device__ inline CmpRec rec_shfl_down(const CmpRec& v, int d) {
  CmpRec o;
  o.amax = v.amax; o.max_z = __shfl_down(v.max_z, d, 64); o.sum_z = __shfl_down(v.sum_z, d, 64);
  o.sum_abs_z = __shfl_down(v.sum_abs_z, d, 64); o.sum_z2 = __shfl_down(v.sum_z2, d, 64);
  o.sum_diff = __shfl_down(v.sum_diff, d, 64); o.sum_scale = __shfl_down(v.sum_scale, d, 64);
  o.n_sel = __shfl_down(v.n_sel, d, 64); o.n_over = __shfl_down(v.n_over, d, 64); o.n_nonf = __shfl_down(v.n_nonf, d, 64);
  o.n_degen = __shfl_down(v.n_degen, d, 64); o.arg = __shfl_down(v.arg, d, 64);
  return o;
}

// What the definition makes of one word of A and B (include/mcs.h): every operation a separate rounding.
struct CmpWord { double d, s2, scale; bool finite; };
// The two slots.  den_a = (double)n_a * (double)(n_a - 1), den_b likewise.
struct SrcCmp {
  // Pairs a thread loads before it looks at them: a pair is four loads of 16 bytes, so 2 keep in flight the 128 bytes per thread that
  // SrcOne's sweep 2 keeps with its 4.  Not measured against other values.
  static constexpr int LOADS = 2;
  const double* ma; const double* qa; const double* mb; const double* qb;
  double den_a, den_b;
  __device__ CmpWord word(double xa, double ya, double xb, double yb) const {
    CmpWord w;
    const double va = ya / den_a, vb = yb / den_b;
    w.s2 = va + vb;
    w.d = xa - xb;
    const double fa = fabs(xa), fb = fabs(xb);
    w.scale = fa > fb ? fa : fb;
    w.finite = finite_(xa) && finite_(ya) && finite_(xb) && finite_(yb) && finite_(w.d) && finite_(w.s2);
    return w;
  }
  // (its own reader for walk)
  struct Pair { double2 xa, ya, xb, yb; };
  __device__ CmpWord at(long long i) const { return word(ma[i], qa[i], mb[i], qb[i]); }
  __device__ Pair pair(long long p) const {
    return Pair{reinterpret_cast<const double2*>(ma)[p], reinterpret_cast<const double2*>(qa)[p], reinterpret_cast<const double2*>(mb)[p],
                reinterpret_cast<const double2*>(qb)[p]};
  }
  __device__ CmpWord lo(const Pair& p) const { return word(p.xa.x, p.ya.x, p.xb.x, p.yb.x); }
  __device__ CmpWord hi(const Pair& p) const { return word(p.xa.y, p.ya.y, p.xb.y, p.yb.y); }
};

// sweep 1: the largest scale = max(|ma|, |mb|) over the finite words, per block
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_cmp_amax(const SrcCmp src, const SumParams* __restrict__ P, double* __restrict__ pmax) {
  __shared__ double tmp[SUM_WAVES];
  const int r = range_of_block(P, blockIdx.x), o0 = P->off[r];
  const SumSpan s = span_of(P->r[r], blockIdx.x - o0, P->off[r + 1] - o0);
  double a = 0.0;
  walk<SrcCmp::LOADS>(s, src, [&](long long, const CmpWord& w) { if (w.finite && w.scale > a) a = w.scale; });
  a = block_max(a, tmp);
  if (threadIdx.x == 0) pmax[blockIdx.x] = a;
}

// sweep 2: with amax = the largest of the range's pmax, the record of the block's words
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_cmp_stats(const SrcCmp src, const SumParams* __restrict__ P, const double* __restrict__ pmax,
                                                                   CmpRec* __restrict__ part) {
  __shared__ double tmp[SUM_WAVES];
  __shared__ CmpRec rtmp[SUM_WAVES];
  const int r = range_of_block(P, blockIdx.x), o0 = P->off[r], n_blk = P->off[r + 1] - o0;
  const SumRange R = P->r[r];
  const SumSpan s = span_of(R, blockIdx.x - o0, n_blk);
  double a = 0.0;
  for (int k = threadIdx.x; k < n_blk; k += ENS_THREADS) { const double x = pmax[o0 + k]; a = x > a ? x : a; }
  const double amax = block_max(a, tmp);
  const double floor_abs = R.floor_frac * amax, zcut = R.tol;
  CmpRec v = cmp_empty(amax);
  walk<SrcCmp::LOADS>(s, src, [&](long long idx, const CmpWord& w) {
    if (!w.finite) { v.n_nonf += 1; return; }
    if (w.scale > 0.0 && w.scale >= floor_abs) {
      v.n_sel += 1;
      v.sum_diff = v.sum_diff + fabs(w.d);
      v.sum_scale = v.sum_scale + w.scale;
      if (w.s2 == 0.0 && w.d != 0.0) { v.n_degen += 1; return; }
      const double z = w.s2 == 0.0 ? 0.0 : w.d / mcsm::sqrt_(w.s2);
      const double az = fabs(z);
      if (az > zcut) v.n_over += 1;
      v.sum_z = v.sum_z + z;
      v.sum_abs_z = v.sum_abs_z + az;
      v.sum_z2 = v.sum_z2 + z * z;
      if (az > v.max_z || (az == v.max_z && idx < v.arg)) { v.max_z = az; v.arg = idx; }
    }
  });
  rec_block_join(v, rtmp);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// one block per range: its partials joined in index order, as mcs_k_ens_sum_final joins a summary's
__global__ void __launch_bounds__(ENS_THREADS) mcs_k_ens_cmp_final(const SumParams* __restrict__ P, const CmpRec* __restrict__ part,
                                                                   CmpRec* __restrict__ out) {
  __shared__ CmpRec rtmp[SUM_WAVES];
  const int r = blockIdx.x, o0 = P->off[r], o1 = P->off[r + 1];
  CmpRec v = cmp_empty(0.0);
  for (int k = o0 + threadIdx.x; k < o1; k += ENS_THREADS) rec_join(v, part[k]);
  rec_block_join(v, rtmp);
  if (threadIdx.x == 0) {
    v.amax = o1 > o0 ? part[o0].amax : 0.0;
    if (v.arg == LLONG_MAX) { v.arg = -1; v.max_z = v.n_sel > v.n_degen ? __builtin_nan("") : 0.0; }
    out[r] = v;
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

void products_layout(const mcs_params* p, mcs_ens_products_layout* PL) {
  const int64_t ng = p->n_grid, nm = p->num_psd_mom_bins + 2;
  PL->dNdp_n = ng * nm; PL->zone_n = ng;
  PL->dNdp_sf = 0; PL->dNdp_pf = ng * nm; PL->dNdp_isf = 2 * ng * nm;
  int64_t o = 3 * ng * nm;
  PL->P_psd_par = o;          o += ng;
  PL->P_psd_perp = o;         o += ng;
  PL->energy_density_psd = o; o += ng;
  PL->slope_sf = o;           o += ng;
  PL->slope_pf = o;           o += ng;
  PL->slope_isf = o;          o += ng;
  PL->total = o;
}

void escape_layout(const mcs_params* p, mcs_ens_escape_layout* XL) {
  const int64_t nm = p->num_psd_mom_bins + 2;
  XL->row_n = nm;
  XL->dNdp = 0; XL->number = 6 * nm; XL->slope = 6 * nm + 6;
  XL->total = 6 * nm + 12;
}

void angles_layout(const mcs_params* p, int n_win, mcs_ens_angles_layout* AL) {
  const int64_t nt = p->num_psd_tht_bins + 2, rows = 3 * (int64_t)p->n_grid * n_win;
  AL->row_n = nt; AL->rows = rows;
  AL->dist = 0; AL->number = rows * nt; AL->mean_mu = rows * nt + rows; AL->mean_mu2 = rows * nt + 2 * rows;
  AL->total = rows * nt + 3 * rows;
}
// the windows of an angles sample by the rules of mcs_angle_dist: null if they are good
const char* angle_windows_error(const mcs_params* p, int n_win, const int32_t* l_lo, const int32_t* l_hi) {
  if (n_win < 1 || n_win > MCS_ANGLE_MAX_WINDOWS) return "n_win outside 1..MCS_ANGLE_MAX_WINDOWS";
  for (int m = 0; m < n_win; ++m)
    if (l_lo[m] < 0 || l_lo[m] >= l_hi[m] || l_hi[m] > p->num_psd_mom_bins + 1) return "a window needs 0 <= l_lo < l_hi <= nmom + 1";
  return nullptr;
}

void photons_layout(int n_shells, const int n[3], int n_pts, mcs_ens_photons_layout* HL) {
  const int64_t rows = (int64_t)n_shells + 1;
  HL->rows = rows; HL->n_synch = n[0]; HL->n_ic = n[1]; HL->n_pion = n[2]; HL->n_pts = n_pts;
  HL->synch = 0; HL->ic = rows * n[0]; HL->pion = HL->ic + rows * n[1]; HL->total_section = HL->pion + rows * n[2];
  HL->total = HL->total_section + rows * n_pts;
}
const char* photons_layout_error(int n_shells, const int n[3], const int start[3], int n_pts) {
  if (n_shells < 1 || n_shells > 4096) return "n_shells outside 1..4096";
  if (n_pts < 1 || n_pts > 65536) return "n_pts outside 1..65536";
  for (int p = 0; p < 3; ++p)
    if (n[p] < 1 || n[p] > 255 || start[p] < 0 || start[p] + n[p] > n_pts) return "a process needs 1..255 energy words that lie inside the common grid";
  return nullptr;
}

constexpr int PRODUCTS_BIT = 1 << 30;      // MCS_ENS_PRODUCTS
constexpr int PHOTONS_BIT = 1 << 29;       // MCS_ENS_PHOTONS
constexpr int PHOTONS_ALL = 1 << 28;       // MCS_ENS_PHOTONS_ALL
constexpr int ESCAPE_BIT = 1 << 27;        // MCS_ENS_ESCAPE
constexpr int ANGLES_BIT = 1 << 26;        // MCS_ENS_ANGLES
constexpr int TCUTS_BIT = 1 << 25;         // MCS_ENS_TCUTS
constexpr int PROFILE_SLOT = 1 << 24;      // MCS_ENS_PROFILE
constexpr int DETECTORS_BIT = 1 << 23;     // MCS_ENS_DETECTORS

// The ten kinds of slot, and the one place where the bits of a slot number are read: -> its kind and the species slot it belongs
// to (s; not yet held against the accumulator's species slots, slot_ref does that; -1 for the iteration, the source and the profile slot).
// A negative number has every high bit set: it is no companion slot, and is refused as a species slot outside the range.
// The source slot has the photons slots' vector and layout rules; it is a kind of its own in a comparison.
enum Kind { SPECIES, ITERATION, PRODUCTS, PHOTONS, SOURCE, ESCAPE, ANGLES, TCUTS, PROFILE, DETECTORS, N_KINDS };
const char* const KIND_NAME[] = {"species", "iteration", "products", "photons", "source", "escape", "angles", "tcuts", "profile", "detectors"};
struct SlotId { Kind kind; int s; };
SlotId decode(int slot, int n_slots) {
  if (slot == PHOTONS_ALL) return SlotId{SOURCE, -1};
  if (slot == PROFILE_SLOT) return SlotId{PROFILE, -1};
  if (slot >= 0 && (slot & PRODUCTS_BIT) != 0) return SlotId{PRODUCTS, slot ^ PRODUCTS_BIT};
  if (slot >= 0 && (slot & PHOTONS_BIT) != 0) return SlotId{PHOTONS, slot ^ PHOTONS_BIT};
  if (slot >= 0 && (slot & ESCAPE_BIT) != 0) return SlotId{ESCAPE, slot ^ ESCAPE_BIT};
  if (slot >= 0 && (slot & ANGLES_BIT) != 0) return SlotId{ANGLES, slot ^ ANGLES_BIT};
  if (slot >= 0 && (slot & TCUTS_BIT) != 0) return SlotId{TCUTS, slot ^ TCUTS_BIT};
  if (slot >= 0 && (slot & DETECTORS_BIT) != 0) return SlotId{DETECTORS, slot ^ DETECTORS_BIT};
  return slot == n_slots - 1 ? SlotId{ITERATION, -1} : SlotId{SPECIES, slot};
}
bool has_photon_vector(Kind k) { return k == PHOTONS || k == SOURCE; }
bool has_window_vector(Kind k) { return k == PRODUCTS || k == ESCAPE; }      // (its sample holds slopes over the slope window)

// What every slot is: the samples it has taken and its two vectors (those of a products, photons, source, escape, angles or tcuts slot from its first
// sample or merge on, nothing before)
struct Slot { long long n = 0; DevBuf<double> mean, m2; };

}  // namespace

struct mcs_ens {
  int device = 0;
  mcs_ctx* home = nullptr;
  mcs_params P;
  mcs_layout L;
  mcs_ens_layout E;
  IncRanges inc;
  int n_slots = 0;                            // the species slots and, last, the iteration slot
  std::vector<Slot> main;                     // those: sp_total (it_total for the last) doubles per vector
  DevBuf<double> marg;                        // the marginals of the sample being added (part 4)
  DevBuf<double> snap;                        // [esc_flux, energy_recv_pool) of snap_of at the last begin-iteration call
  mcs_ctx* snap_of = nullptr;                 // (null: no snapshot since the last iteration sample)
  Event ev;                                   // recorded after every operation on the stream that carried it
  bool ev_set = false;
  // mcs_ens_summarize, allocated at its first call: the ranges of a call and its results (pinned, and on the device), and one
  // pmax / one record per block of the largest call so far
  PinnedBuf<SumParams> sum_par_h; DevBuf<SumParams> sum_par;
  PinnedBuf<SumRec> sum_out_h;    DevBuf<SumRec> sum_out;
  DevBuf<double> sum_pmax;        DevBuf<SumRec> sum_part;
  // mcs_ens_compare with this accumulator as A shares sum_par and sum_pmax with it; its records are another type
  PinnedBuf<CmpRec> cmp_out_h;    DevBuf<CmpRec> cmp_out, cmp_part;
  // the products slots, one beside every species slot (include/mcs.h, "products sample"): PL.total doubles per vector
  mcs_ens_products_layout PL;
  std::vector<Slot> products;
  int win_lo = 0, win_hi = 0;                 // the slope window; none while x_log_h is empty
  std::vector<double> x_log_h;                // [nmom+1]
  DevBuf<double> x_log, slope;                // its device copy; the slopes of the sample being added [3][n_grid]
  bool products_sampled = false;              // some products or escape slot has taken a sample (or a merge): the window is fixed
  // the escape slots, likewise (include/mcs.h, "escape sample"): XL.total doubles per vector; the slopes of the sample being added
  mcs_ens_escape_layout XL;
  std::vector<Slot> escape;
  DevBuf<double> esc_slope;                   // [2][3]
  // the angles slots, likewise (include/mcs.h, "angles sample"): AL.total doubles per vector; no windows while ang_n_win is 0
  mcs_ens_angles_layout AL{};
  int ang_n_win = 0;
  int32_t ang_lo[MCS_ANGLE_MAX_WINDOWS] = {}, ang_hi[MCS_ANGLE_MAX_WINDOWS] = {};
  std::vector<Slot> angles;
  bool angles_sampled = false;                // some angles slot has taken a sample (or a merge): the windows are fixed
  // the tcuts slots, likewise (include/mcs.h, "tcuts sample"): TL.total doubles per vector; tc_n, the n_tcuts of the first tcuts sample
  // (or merge), is fixed from then on; 0: none yet
  mcs_ens_tcuts_layout TL{};
  int tc_n = 0;
  std::vector<Slot> tcuts;
  // the profile slot MCS_ENS_PROFILE (include/mcs.h, "profile sample"): FL.total doubles per vector; prof_set, the settings of the first
  // profile sample's mcs_profile_in (F_px_upstream .. i_trans), is fixed from then on; prof_taken: there is one
  mcs_ens_profile_layout FL{};
  mcs_profile_in prof_set{};
  bool prof_taken = false;
  Slot profile;
  // the detectors slots, like the tcuts slots (include/mcs.h, "detectors sample"): DL.total doubles per vector; the settings of the first
  // detectors sample (or merge) -- det_n detectors, the window, x_unit and x_spec -- are fixed from then on; det_n 0: none yet
  mcs_ens_detectors_layout DL{};
  int det_n = 0, det_lo = 0, det_hi = 0;
  double det_x_unit = 0.0;
  std::vector<double> det_x_spec;
  std::vector<Slot> detectors;
  // the photons slots, likewise (include/mcs.h, "photons sample"): HL.total doubles per vector; no layout while ph_shells is 0
  mcs_ens_photons_layout HL{};
  int ph_shells = 0, ph_n[3] = {0, 0, 0}, ph_start[3] = {0, 0, 0}, ph_npts = 0;
  std::vector<Slot> photons;
  bool photons_sampled = false;               // some photons slot has taken a sample (or a merge): the layout is fixed
  // the source slot MCS_ENS_PHOTONS_ALL (include/mcs.h, "source sample"), of the photons layout; the pending vector from the first
  // deposit on; the species slots deposited since the last take, in call order (host bookkeeping)
  Slot source;
  DevBuf<double> pending;
  std::vector<int> deposited;
  bool has_photon_layout() const { return ph_shells > 0; }
  bool has_window() const { return !x_log_h.empty(); }
  bool has_angle_windows() const { return ang_n_win > 0; }
  bool has_tcuts() const { return tc_n > 0; }
  bool has_profile() const { return prof_taken; }
  bool has_detectors() const { return det_n > 0; }
  // the one way from a (checked) slot number to its record, and the length of the vectors of a kind
  Slot& at(SlotId id) {
    return id.kind == SOURCE ? source : id.kind == PHOTONS ? photons[(size_t)id.s] : id.kind == PRODUCTS ? products[(size_t)id.s]
           : id.kind == ESCAPE ? escape[(size_t)id.s] : id.kind == ANGLES ? angles[(size_t)id.s]
           : id.kind == TCUTS ? tcuts[(size_t)id.s] : id.kind == PROFILE ? profile
           : id.kind == DETECTORS ? detectors[(size_t)id.s]
           : main[(size_t)(id.kind == ITERATION ? n_slots - 1 : id.s)];
  }
  long long len(Kind k) const {
    return has_photon_vector(k) ? (has_photon_layout() ? HL.total : 0) : k == PRODUCTS ? PL.total : k == ESCAPE ? XL.total : k == ANGLES ? (has_angle_windows() ? AL.total : 0) : k == TCUTS ? (has_tcuts() ? TL.total : 0) : k == PROFILE ? (has_profile() ? FL.total : 0) : k == DETECTORS ? (has_detectors() ? DL.total : 0) : k == ITERATION ? E.it_total : E.sp_total;
  }
  // every slot number the accumulator has
  std::vector<int> slot_numbers() const {
    std::vector<int> all;
    for (int s = 0; s < n_slots; ++s) all.push_back(s);
    for (int s = 0; s < n_slots - 1; ++s) { all.push_back(s | PRODUCTS_BIT); all.push_back(s | PHOTONS_BIT); all.push_back(s | ESCAPE_BIT); all.push_back(s | ANGLES_BIT); all.push_back(s | TCUTS_BIT); all.push_back(s | DETECTORS_BIT); }
    all.push_back(PHOTONS_ALL);
    all.push_back(PROFILE_SLOT);
    return all;
  }
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

// What a count, read, summary or comparison call works on: the slot of that number, its kind and the length of its vectors
// (which are null for a products, photons, source, escape, angles or tcuts slot that was never sampled; n is then 0).
struct SlotRef { Kind kind; Slot* slot; long long len; };
int slot_ref(mcs_ens* e, const std::string& who, int slot, SlotRef* out) {
  const SlotId id = decode(slot, e->n_slots);
  if ((id.kind == PRODUCTS || id.kind == PHOTONS || id.kind == ESCAPE || id.kind == ANGLES || id.kind == TCUTS || id.kind == DETECTORS) && id.s >= e->n_slots - 1)
    return fail(who + ": " + KIND_NAME[id.kind] + " slot of slot " + std::to_string(id.s) + ", which is no species slot (0.." + std::to_string(e->n_slots - 2) + ")");
  if (id.kind == SPECIES && (slot < 0 || slot >= e->n_slots)) return fail(who + ": slot " + std::to_string(slot) + " outside 0.." + std::to_string(e->n_slots - 1));
  *out = SlotRef{id.kind, &e->at(id), e->len(id.kind)};
  return 0;
}

// slot is a species slot, where a call takes nothing else; tail: what the caller says of the iteration slot
int species_slot(const mcs_ens* e, const std::string& who, int slot, const char* tail) {
  if (slot < 0 || slot >= e->n_slots) return fail(who + ": slot " + std::to_string(slot) + " outside 0.." + std::to_string(e->n_slots - 1));
  if (slot == e->n_slots - 1) return fail(who + ": slot " + std::to_string(slot) + " is the iteration slot; " + tail);
  return 0;
}

// the two accumulators have the same tally, binning and sample layout (whether they have as many slots is the caller's question)
bool same_layout(const mcs_ens* a, const mcs_ens* b) {
  return a->E.sp_total == b->E.sp_total && a->E.it_total == b->E.it_total && a->L.total == b->L.total && a->P.n_grid == b->P.n_grid &&
         a->P.n_ions == b->P.n_ions && a->P.n_itrs == b->P.n_itrs && a->P.num_psd_mom_bins == b->P.num_psd_mom_bins &&
         a->P.num_psd_tht_bins == b->P.num_psd_tht_bins;
}

// both have a slope window, and the two differ in a bound or in the bits of an x_log word
bool windows_differ(const mcs_ens* a, const mcs_ens* b) {
  if (!a->has_window() || !b->has_window()) return false;
  return a->win_lo != b->win_lo || a->win_hi != b->win_hi || a->x_log_h.size() != b->x_log_h.size() ||
         memcmp(a->x_log_h.data(), b->x_log_h.data(), a->x_log_h.size() * sizeof(double)) != 0;
}

// both have angle windows, and the two differ
bool angle_windows_differ(const mcs_ens* a, const mcs_ens* b) {
  if (!a->has_angle_windows() || !b->has_angle_windows()) return false;
  return a->ang_n_win != b->ang_n_win || memcmp(a->ang_lo, b->ang_lo, sizeof a->ang_lo) != 0 || memcmp(a->ang_hi, b->ang_hi, sizeof a->ang_hi) != 0;
}
void angle_windows_take(mcs_ens* e, int n_win, const int32_t* l_lo, const int32_t* l_hi) {
  e->ang_n_win = n_win;
  for (int m = 0; m < MCS_ANGLE_MAX_WINDOWS; ++m) { e->ang_lo[m] = m < n_win ? l_lo[m] : 0; e->ang_hi[m] = m < n_win ? l_hi[m] : 0; }
  angles_layout(&e->P, n_win, &e->AL);
}

// both have taken tcuts samples, and their n_tcuts differ
bool tcuts_differ(const mcs_ens* a, const mcs_ens* b) { return a->has_tcuts() && b->has_tcuts() && a->tc_n != b->tc_n; }
void tcuts_take(mcs_ens* e, int n_tcuts) {
  e->tc_n = n_tcuts;
  mcs_tcut_get_layout(&e->P, n_tcuts, &e->TL);
}

// both have taken profile samples, and the settings of their mcs_profile_in (the bytes up to n_hist) differ in some bit
bool profile_settings_differ(const mcs_profile_in& a, const mcs_profile_in& b) { return std::memcmp(&a, &b, offsetof(mcs_profile_in, n_hist)) != 0; }
bool profiles_differ(const mcs_ens* a, const mcs_ens* b) { return a->has_profile() && b->has_profile() && profile_settings_differ(a->prof_set, b->prof_set); }
void profile_take(mcs_ens* e, const mcs_profile_in& in) {
  e->prof_set = in;
  e->prof_taken = true;
  mcs_profile_get_layout(&e->P, &e->FL);
}

// both have taken detectors samples, and their settings (nd, window, the bits of x_unit and of x_spec) differ
bool detector_settings_differ(int na, int lo_a, int hi_a, double xu_a, const double* xs_a, int nb, int lo_b, int hi_b, double xu_b, const double* xs_b) {
  return na != nb || lo_a != lo_b || hi_a != hi_b || std::memcmp(&xu_a, &xu_b, sizeof(double)) != 0 ||
         std::memcmp(xs_a, xs_b, sizeof(double) * (size_t)na) != 0;
}
bool detectors_differ(const mcs_ens* a, const mcs_ens* b) {
  return a->has_detectors() && b->has_detectors() &&
         detector_settings_differ(a->det_n, a->det_lo, a->det_hi, a->det_x_unit, a->det_x_spec.data(), b->det_n, b->det_lo, b->det_hi, b->det_x_unit,
                                  b->det_x_spec.data());
}
void detectors_take(mcs_ens* e, int nd, int l_lo, int l_hi, double x_unit, const double* x_spec) {
  e->det_n = nd; e->det_lo = l_lo; e->det_hi = l_hi; e->det_x_unit = x_unit;
  e->det_x_spec.assign(x_spec, x_spec + nd);
  mcs_detector_get_layout(&e->P, nd, &e->DL);
}

// both have a photon layout, and the two differ
bool photon_layouts_differ(const mcs_ens* a, const mcs_ens* b) {
  if (!a->has_photon_layout() || !b->has_photon_layout()) return false;
  return a->ph_shells != b->ph_shells || a->ph_npts != b->ph_npts || memcmp(a->ph_n, b->ph_n, sizeof a->ph_n) != 0 ||
         memcmp(a->ph_start, b->ph_start, sizeof a->ph_start) != 0;
}
void photon_layout_take(mcs_ens* e, int n_shells, const int n[3], const int start[3], int n_pts) {
  e->ph_shells = n_shells; e->ph_npts = n_pts;
  for (int p = 0; p < 3; ++p) { e->ph_n[p] = n[p]; e->ph_start[p] = start[p]; }
  photons_layout(n_shells, n, n_pts, &e->HL);
}

// room for the two vectors of a slot, len doubles each, zeroed on st when they are new
int reserve(Slot& s, long long len, const std::string& who, hipStream_t st) {
  if (s.mean.get() && s.m2.get()) return 0;
  hipError_t a = s.mean.reserve(len);
  if (a == hipSuccess) a = s.m2.reserve(len);
  if (a != hipSuccess) { s.mean.reset(); s.m2.reset(); return fail(who + ": hipMalloc: " + hipGetErrorString(a)); }
  ENSCHK(hipMemsetAsync(s.mean.get(), 0, (size_t)len * sizeof(double), st));
  ENSCHK(hipMemsetAsync(s.m2.get(), 0, (size_t)len * sizeof(double), st));
  return 0;
}

// Chan's merge of slot b into slot a, both of len words, on st: nothing for an empty b, a copy into an empty a, else one launch
int merge_slot(Slot& a, const Slot& b, long long len, hipStream_t st) {
  if (b.n == 0) return 0;
  if (reserve(a, len, "mcs_ens_merge", st)) return 1;
  if (a.n == 0) {
    ENSCHK(hipMemcpyAsync(a.mean, b.mean, (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, st));
    ENSCHK(hipMemcpyAsync(a.m2, b.m2, (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, st));
  } else {
    const double n = (double)(a.n + b.n);
    hipLaunchKernelGGL(mcs_k_ens_merge, dim3(grid_for(len)), dim3(ENS_THREADS), 0, st, a.mean.get(), a.m2.get(), b.mean.get(), b.m2.get(), len,
                       (double)b.n / n, (double)a.n * (double)b.n / n);
    ENSCHK(hipGetLastError());
  }
  a.n += b.n;
  return 0;
}

// The ranges of a summary (cut: their tol) or of a comparison (their zcut; cut_name says which) against a vector of len words:
// checked and, in the same pass, written with their block offsets into e's pinned SumParams -> the blocks they take
// (every earlier call has waited for its copies: the pinned block is free)
template <class Range>
int plan_ranges(const std::string& who, mcs_ens* e, long long len, int n_ranges, const Range* ranges, double Range::*cut, const char* cut_name,
                long long* n_blocks) {
  const hipError_t a = e->sum_par_h.reserve(1);
  if (a != hipSuccess) return fail(who + ": scratch allocation: " + hipGetErrorString(a));
  SumParams* P = e->sum_par_h.get();
  P->n_ranges = n_ranges;
  P->off[0] = 0;
  for (int r = 0; r < n_ranges; ++r) {
    const Range& R = ranges[r];
    const std::string which = who + ": range " + std::to_string(r);
    if (R.first < 0 || R.count < 0 || R.first > len || R.count > len - R.first) return fail(which + " lies outside the slot's sample vector");
    if (!(R.floor_frac >= 0.0 && R.floor_frac <= 1.0)) return fail(which + ": floor_frac outside [0, 1]");
    if (!(R.*cut >= 0.0)) return fail(which + ": " + cut_name + " is negative or not a number");
    P->r[r] = SumRange{R.first, R.count, R.floor_frac, R.*cut};
    const long long b = (R.count + SUM_CHUNK - 1) / SUM_CHUNK;
    P->off[r + 1] = P->off[r] + (int)(b > SUM_MAX_BLOCKS ? SUM_MAX_BLOCKS : b);
  }
  *n_blocks = P->off[n_ranges];
  return 0;
}

// the rest of e's scratch for a planned call of n_blocks blocks whose records are Rec
template <class Rec>
int reserve_scratch(const std::string& who, mcs_ens* e, PinnedBuf<Rec>& out_h, DevBuf<Rec>& out, DevBuf<Rec>& part, long long n_blocks) {
  hipError_t a = e->sum_par.reserve(1);
  if (a == hipSuccess) a = out_h.reserve(SUM_MAX_RANGES);
  if (a == hipSuccess) a = out.reserve(SUM_MAX_RANGES);
  if (a == hipSuccess) a = e->sum_pmax.reserve(n_blocks);
  if (a == hipSuccess) a = part.reserve(n_blocks);
  if (a != hipSuccess) return fail(who + ": scratch allocation: " + hipGetErrorString(a));
  return 0;
}

template <int N>
SrcMerged<N> merged_src(const double* const* mean, const double* const* m2, const double* f_mean, const double* f_m2) {
  SrcMerged<N> s;
  for (int k = 0; k < N; ++k) { s.mean[k] = mean[k]; s.m2[k] = m2[k]; s.f_mean[k] = f_mean[k]; s.f_m2[k] = f_m2[k]; }
  return s;
}

// The ranges that plan_ranges has left in list[0]'s pinned SumParams, n_blocks blocks, summarised from the word source src with
// the count n: on the stream of list[0]'s home context, after what every accumulator of the list queued last, with list[0]'s
// scratch; waits for the device.
template <class Src>
int sum_run(const std::string& who, mcs_ens* const* list, int n_list, const Src& src, long long n, int n_ranges, long long n_blocks,
            mcs_ens_summary* out) {
  mcs_ens* e = list[0];
  McsCtxView v;
  if (mcs_ctx_view_get(e->home, &v)) return 1;
  if (reserve_scratch(who, e, e->sum_out_h, e->sum_out, e->sum_part, n_blocks)) return 1;
  for (int k = 0; k < n_list; ++k)
    if (enter(list[k], v.stream)) return 1;
  const double denom = (double)n * (double)(n - 1);
  ENSCHK(hipMemcpyAsync(e->sum_par.get(), e->sum_par_h.get(), sizeof(SumParams), hipMemcpyHostToDevice, v.stream));
  if (n_blocks > 0) {
    hipLaunchKernelGGL(mcs_k_ens_sum_amax<Src>, dim3((unsigned)n_blocks), dim3(ENS_THREADS), 0, v.stream, src, e->sum_par.get(), e->sum_pmax.get());
    ENSCHK(hipGetLastError());
  }
  // One pass gives the answer unless a word with a finite mean and a non-finite M2 carried the largest |mean| of a range: sweep 1
  // reads the means alone, sweep 2 sees it.  The second pass then selects with the amax of the finite words (and waits once more).
  const SumRec* got = e->sum_out_h.get();
  for (int pass = 0; pass < 2; ++pass) {
    if (n_blocks > 0) {
      hipLaunchKernelGGL(mcs_k_ens_sum_stats<Src>, dim3((unsigned)n_blocks), dim3(ENS_THREADS), 0, v.stream, src, e->sum_par.get(), e->sum_pmax.get(),
                         e->sum_part.get(), denom);
      ENSCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(mcs_k_ens_sum_final, dim3((unsigned)n_ranges), dim3(ENS_THREADS), 0, v.stream, e->sum_par.get(), e->sum_part.get(),
                       e->sum_pmax.get(), e->sum_out.get());
    ENSCHK(hipGetLastError());
    ENSCHK(hipMemcpyAsync(e->sum_out_h.get(), e->sum_out.get(), (size_t)n_ranges * sizeof(SumRec), hipMemcpyDeviceToHost, v.stream));
    ENSCHK(hipStreamSynchronize(v.stream));
    bool again = false;
    for (int r = 0; r < n_ranges; ++r) again = again || got[r].amax != got[r].amax_used;
    if (!again) break;
  }
  for (int r = 0; r < n_ranges; ++r) {
    const SumRec& g = got[r];
    out[r] = mcs_ens_summary{g.amax, g.max_rel, g.sum_se, g.sum_abs, g.sum_rel2, g.n_sel, g.n_over, g.n_nonf, g.arg};
  }
  return 0;
}

}  // namespace

extern "C" {

int mcs_ens_get_layout(const mcs_params* p, mcs_ens_layout* out) {
  if (!p || !out) return fail("mcs_ens_get_layout: null argument");
  ens_layout(p, out);
  return 0;
}

int mcs_ens_products_get_layout(const mcs_params* p, mcs_ens_products_layout* out) {
  if (!p || !out) return fail("mcs_ens_products_get_layout: null argument");
  products_layout(p, out);
  return 0;
}

int mcs_ens_escape_get_layout(const mcs_params* p, mcs_ens_escape_layout* out) {
  if (!p || !out) return fail("mcs_ens_escape_get_layout: null argument");
  escape_layout(p, out);
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
  products_layout(&v.P, &e->PL);
  e->products.resize((size_t)n_species_slots);
  e->photons.resize((size_t)n_species_slots);
  escape_layout(&v.P, &e->XL);
  e->escape.resize((size_t)n_species_slots);
  e->angles.resize((size_t)n_species_slots);
  e->tcuts.resize((size_t)n_species_slots);
  e->detectors.resize((size_t)n_species_slots);
  const mcs_layout& L = v.L;
  e->inc = IncRanges{{L.esc_flux, L.esc_energy_eff, L.spectra_coupled}, {L.px_esc_feb, L.weight_coupled, L.energy_transfer_pool}};
  e->n_slots = n_species_slots + 1;
  e->main.resize((size_t)e->n_slots);
  for (int s = 0; s < e->n_slots; ++s)
    if (reserve(e->main[(size_t)s], e->len(s == e->n_slots - 1 ? ITERATION : SPECIES), "mcs_ens_create", v.stream)) return 1;
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
  if (species_slot(e, "mcs_ens_add_species", slot, "it takes no species sample")) return 1;
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
  Slot& sl = e->main[(size_t)slot];
  hipLaunchKernelGGL(mcs_k_ens_add_species, dim3(grid_for(E.sp_total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), v.T, v.I,
                     e->marg.get(), E, (double)(sl.n + 1));
  ENSCHK(hipGetLastError());
  sl.n += 1;
  return leave(e, v.stream);
}

int mcs_ens_add_iteration(mcs_ens* e, mcs_ctx* src) {
  if (!e || !src) return fail("mcs_ens_add_iteration: null argument");
  McsCtxView v;
  if (view_of(e, src, "mcs_ens_add_iteration", &v)) return 1;
  if (e->snap_of != src) return fail("mcs_ens_add_iteration: no mcs_ens_begin_iteration snapshot of this context since the last iteration sample");
  if (enter(e, v.stream)) return 1;
  Slot& sl = e->main.back();
  hipLaunchKernelGGL(mcs_k_ens_add_iteration, dim3(grid_for(e->E.it_total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), v.T,
                     e->snap.get(), e->E, e->inc, (double)(sl.n + 1));
  ENSCHK(hipGetLastError());
  sl.n += 1;
  e->snap_of = nullptr;
  return leave(e, v.stream);
}

int mcs_ens_set_slope_window(mcs_ens* e, int l_lo, int l_hi, const double* x_log) {
  const std::string who = "mcs_ens_set_slope_window";
  if (!e || !x_log) return fail(who + ": null argument");
  if (e->products_sampled) return fail(who + ": a products or escape slot has taken a sample; the window stays as it is");
  const int nx = e->P.num_psd_mom_bins + 1;
  if (l_lo < 0 || l_hi > nx || l_hi - l_lo < 3)
    return fail(who + ": window [" + std::to_string(l_lo) + ", " + std::to_string(l_hi) + ") needs 0 <= l_lo, l_hi <= " + std::to_string(nx) +
                " and at least three bins");
  for (int l = 0; l < nx; ++l)
    if (!std::isfinite(x_log[l])) return fail(who + ": x_log[" + std::to_string(l) + "] is not finite");
  McsCtxView v;
  if (mcs_ctx_view_get(e->home, &v)) return 1;
  hipError_t a = e->x_log.reserve(nx);
  if (a == hipSuccess) a = e->slope.reserve(3LL * e->P.n_grid);
  if (a != hipSuccess) return fail(who + ": hipMalloc: " + hipGetErrorString(a));
  if (enter(e, v.stream)) return 1;
  ENSCHK(hipMemcpyAsync(e->x_log.get(), x_log, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, v.stream));
  ENSCHK(hipStreamSynchronize(v.stream));      // (the caller's array is free again)
  e->x_log_h.assign(x_log, x_log + nx);
  e->win_lo = l_lo; e->win_hi = l_hi;
  return leave(e, v.stream);
}

int mcs_ens_add_products(mcs_ens* e, mcs_ctx* src, int slot) {
  const std::string who = "mcs_ens_add_products";
  if (!e || !src) return fail(who + ": null argument");
  if (species_slot(e, who, slot, "only a species slot has a products slot")) return 1;
  if (!e->has_window()) return fail(who + ": no slope window (mcs_ens_set_slope_window)");
  McsCtxView v;
  if (view_of(e, src, who.c_str(), &v)) return 1;
  if (!v.have_dndp_cr || !v.have_thermo || !v.cout)
    return fail(who + ": the context needs an mcs_dndp_cr and an mcs_thermo_calcs since its last mcs_begin_species and its last products sample");
  if (enter(e, v.stream)) return 1;
  Slot& sl = e->products[(size_t)slot];
  if (reserve(sl, e->PL.total, who, v.stream)) return 1;
  const long long ng = e->P.n_grid, n_cout = e->PL.slope_sf;
  const int nm = e->P.num_psd_mom_bins + 2;
  hipLaunchKernelGGL(mcs_k_ens_slope, dim3(grid_for(3 * ng)), dim3(ENS_THREADS), 0, v.stream, v.cout, e->x_log.get(), e->slope.get(), 3 * ng, nm,
                     e->win_lo, e->win_hi);
  ENSCHK(hipGetLastError());
  hipLaunchKernelGGL(mcs_k_ens_add_products, dim3(grid_for(e->PL.total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), v.cout,
                     e->slope.get(), n_cout, (long long)e->PL.total, (double)(sl.n + 1));
  ENSCHK(hipGetLastError());
  sl.n += 1;
  e->products_sampled = true;
  mcs_ctx_view_products_taken(src);
  return leave(e, v.stream);
}

int mcs_ens_add_escape(mcs_ens* e, mcs_ctx* src, int slot) {
  const std::string who = "mcs_ens_add_escape";
  if (!e || !src) return fail(who + ": null argument");
  if (species_slot(e, who, slot, "only a species slot has an escape slot")) return 1;
  if (!e->has_window()) return fail(who + ": no slope window (mcs_ens_set_slope_window)");
  McsCtxView v;
  if (view_of(e, src, who.c_str(), &v)) return 1;
  if (!v.have_esc || !v.esc_out)
    return fail(who + ": the context needs an mcs_dndp_esc since its last mcs_begin_species and its last escape sample");
  const hipError_t a = e->esc_slope.reserve(6);
  if (a != hipSuccess) return fail(who + ": hipMalloc: " + hipGetErrorString(a));
  if (enter(e, v.stream)) return 1;
  Slot& sl = e->escape[(size_t)slot];
  if (reserve(sl, e->XL.total, who, v.stream)) return 1;
  // the sample is the call's result (dNdp | number) as it lies on the device, then the six slopes of its rows
  hipLaunchKernelGGL(mcs_k_ens_slope, dim3(1), dim3(ENS_THREADS), 0, v.stream, v.esc_out, e->x_log.get(), e->esc_slope.get(), 6LL, (int)e->XL.row_n,
                     e->win_lo, e->win_hi);
  ENSCHK(hipGetLastError());
  hipLaunchKernelGGL(mcs_k_ens_add_products, dim3(grid_for(e->XL.total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), v.esc_out,
                     e->esc_slope.get(), (long long)e->XL.slope, (long long)e->XL.total, (double)(sl.n + 1));
  ENSCHK(hipGetLastError());
  sl.n += 1;
  e->products_sampled = true;
  mcs_ctx_view_escape_taken(src);
  return leave(e, v.stream);
}

int mcs_ens_angles_get_layout(const mcs_params* p, int n_win, mcs_ens_angles_layout* out) {
  if (!p || !out) return fail("mcs_ens_angles_get_layout: null argument");
  if (n_win < 1 || n_win > MCS_ANGLE_MAX_WINDOWS) return fail("mcs_ens_angles_get_layout: n_win outside 1.." + std::to_string(MCS_ANGLE_MAX_WINDOWS));
  angles_layout(p, n_win, out);
  return 0;
}

int mcs_ens_set_angle_windows(mcs_ens* e, int n_win, const int32_t* l_lo, const int32_t* l_hi) {
  const std::string who = "mcs_ens_set_angle_windows";
  if (!e || !l_lo || !l_hi) return fail(who + ": null argument");
  if (e->angles_sampled) return fail(who + ": an angles slot has taken a sample; the windows stay as they are");
  if (const char* msg = angle_windows_error(&e->P, n_win, l_lo, l_hi)) return fail(who + ": " + msg);
  angle_windows_take(e, n_win, l_lo, l_hi);
  return 0;
}

int mcs_ens_add_angles(mcs_ens* e, mcs_ctx* src, int slot) {
  const std::string who = "mcs_ens_add_angles";
  if (!e || !src) return fail(who + ": null argument");
  if (species_slot(e, who, slot, "only a species slot has an angles slot")) return 1;
  if (!e->has_angle_windows()) return fail(who + ": no angle windows (mcs_ens_set_angle_windows)");
  McsCtxView v;
  if (view_of(e, src, who.c_str(), &v)) return 1;
  if (!v.have_ang || !v.ang_out)
    return fail(who + ": the context needs an mcs_angle_dist since its last mcs_begin_species, tally write and angles sample");
  if (v.ang_n_win != e->ang_n_win || memcmp(v.ang_lo, e->ang_lo, sizeof e->ang_lo) != 0 || memcmp(v.ang_hi, e->ang_hi, sizeof e->ang_hi) != 0)
    return fail(who + ": the windows of the context's mcs_angle_dist differ from the accumulator's");
  if (enter(e, v.stream)) return 1;
  Slot& sl = e->angles[(size_t)slot];
  if (reserve(sl, e->AL.total, who, v.stream)) return 1;
  // the sample is the call's result as it lies on the device
  hipLaunchKernelGGL(mcs_k_ens_add_vector, dim3(grid_for(e->AL.total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), v.ang_out,
                     (long long)e->AL.total, (double)(sl.n + 1));
  ENSCHK(hipGetLastError());
  sl.n += 1;
  e->angles_sampled = true;
  mcs_ctx_view_angles_taken(src);
  return leave(e, v.stream);
}

int mcs_ens_tcuts_get_layout(const mcs_params* p, int n_tcuts, mcs_ens_tcuts_layout* out) {
  if (!p || !out) return fail("mcs_ens_tcuts_get_layout: null argument");
  return mcs_tcut_get_layout(p, n_tcuts, out);
}

int mcs_ens_add_tcuts(mcs_ens* e, mcs_ctx* src, int slot) {
  const std::string who = "mcs_ens_add_tcuts";
  if (!e || !src) return fail(who + ": null argument");
  if (species_slot(e, who, slot, "only a species slot has a tcuts slot")) return 1;
  McsCtxView v;
  if (view_of(e, src, who.c_str(), &v)) return 1;
  if (!v.have_tcut || !v.tcut_out)
    return fail(who + ": the context needs an mcs_tcut_spectra since its last mcs_begin_species and its last tcuts sample");
  if (e->has_tcuts() && v.tcut_n != e->tc_n)
    return fail(who + ": the context's mcs_tcut_spectra had " + std::to_string(v.tcut_n) + " time cuts, the accumulator's tcuts samples have " +
                std::to_string(e->tc_n));
  if (enter(e, v.stream)) return 1;
  if (!e->has_tcuts()) tcuts_take(e, v.tcut_n);
  Slot& sl = e->tcuts[(size_t)slot];
  if (reserve(sl, e->TL.total, who, v.stream)) return 1;
  // the sample is the call's result as it lies on the device
  hipLaunchKernelGGL(mcs_k_ens_add_vector, dim3(grid_for(e->TL.total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), v.tcut_out,
                     (long long)e->TL.total, (double)(sl.n + 1));
  ENSCHK(hipGetLastError());
  sl.n += 1;
  mcs_ctx_view_tcuts_taken(src);
  return leave(e, v.stream);
}

int mcs_ens_profile_get_layout(const mcs_params* p, mcs_ens_profile_layout* out) {
  if (!p || !out) return fail("mcs_ens_profile_get_layout: null argument");
  return mcs_profile_get_layout(p, out);
}

int mcs_ens_add_profile(mcs_ens* e, mcs_ctx* src) {
  const std::string who = "mcs_ens_add_profile";
  if (!e || !src) return fail(who + ": null argument");
  McsCtxView v;
  if (view_of(e, src, who.c_str(), &v)) return 1;
  if (!v.have_prof || !v.prof_out)
    return fail(who + ": the context needs an mcs_profile_update since its last mcs_begin_species, tally write and profile sample");
  if (e->has_profile() && profile_settings_differ(e->prof_set, v.prof_in))
    return fail(who + ": the settings of the context's mcs_profile_update differ from those of the accumulator's profile samples");
  if (enter(e, v.stream)) return 1;
  if (!e->has_profile()) profile_take(e, v.prof_in);
  Slot& sl = e->profile;
  if (reserve(sl, e->FL.total, who, v.stream)) return 1;
  // the sample is the call's result as it lies on the device
  hipLaunchKernelGGL(mcs_k_ens_add_vector, dim3(grid_for(e->FL.total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), v.prof_out,
                     (long long)e->FL.total, (double)(sl.n + 1));
  ENSCHK(hipGetLastError());
  sl.n += 1;
  mcs_ctx_view_profile_taken(src);
  return leave(e, v.stream);
}

int mcs_ens_detectors_get_layout(const mcs_params* p, int n_det, mcs_ens_detectors_layout* out) {
  if (!p || !out) return fail("mcs_ens_detectors_get_layout: null argument");
  return mcs_detector_get_layout(p, n_det, out);
}

int mcs_ens_add_detectors(mcs_ens* e, mcs_ctx* src, int slot) {
  const std::string who = "mcs_ens_add_detectors";
  if (!e || !src) return fail(who + ": null argument");
  if (species_slot(e, who, slot, "only a species slot has a detectors slot")) return 1;
  McsCtxView v;
  if (view_of(e, src, who.c_str(), &v)) return 1;
  if (!v.have_det || !v.det_out || !v.det_x_spec)
    return fail(who + ": the context needs an mcs_detector_spectra since its last mcs_begin_species and its last detectors sample");
  if (e->has_detectors() && detector_settings_differ(e->det_n, e->det_lo, e->det_hi, e->det_x_unit, e->det_x_spec.data(), v.det_n, v.det_lo,
                                                     v.det_hi, v.det_x_unit, v.det_x_spec))
    return fail(who + ": the settings of the context's mcs_detector_spectra (" + std::to_string(v.det_n) + " detectors, window [" +
                std::to_string(v.det_lo) + ", " + std::to_string(v.det_hi) + "), x_unit, x_spec) differ from those of the accumulator's detectors samples (" +
                std::to_string(e->det_n) + " detectors, window [" + std::to_string(e->det_lo) + ", " + std::to_string(e->det_hi) + "))");
  if (enter(e, v.stream)) return 1;
  if (!e->has_detectors()) detectors_take(e, v.det_n, v.det_lo, v.det_hi, v.det_x_unit, v.det_x_spec);
  Slot& sl = e->detectors[(size_t)slot];
  if (reserve(sl, e->DL.total, who, v.stream)) return 1;
  // the sample is the call's result as it lies on the device
  hipLaunchKernelGGL(mcs_k_ens_add_vector, dim3(grid_for(e->DL.total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), v.det_out,
                     (long long)e->DL.total, (double)(sl.n + 1));
  ENSCHK(hipGetLastError());
  sl.n += 1;
  mcs_ctx_view_detectors_taken(src);
  return leave(e, v.stream);
}

int mcs_ens_photons_get_layout(int n_shells, int n_synch, int n_ic, int n_pion, int n_pts, mcs_ens_photons_layout* out) {
  if (!out) return fail("mcs_ens_photons_get_layout: null argument");
  const int n[3] = {n_synch, n_ic, n_pion}, start[3] = {0, 0, 0};
  if (n_pts >= 1 && (n_synch > n_pts || n_ic > n_pts || n_pion > n_pts)) return fail("mcs_ens_photons_get_layout: a process has more energy words than the common grid");
  if (const char* msg = photons_layout_error(n_shells, n, start, n_pts)) return fail(std::string("mcs_ens_photons_get_layout: ") + msg);
  photons_layout(n_shells, n, n_pts, out);
  return 0;
}

int mcs_ens_set_photon_layout(mcs_ens* e, int n_shells, int n_synch, int n_ic, int n_pion, int start_synch, int start_ic, int start_pion, int n_pts) {
  const std::string who = "mcs_ens_set_photon_layout";
  if (!e) return fail(who + ": null argument");
  if (e->photons_sampled) return fail(who + ": a photons slot has taken a sample; the layout stays as it is");
  const int n[3] = {n_synch, n_ic, n_pion}, start[3] = {start_synch, start_ic, start_pion};
  if (const char* msg = photons_layout_error(n_shells, n, start, n_pts)) return fail(who + ": " + msg);
  photon_layout_take(e, n_shells, n, start, n_pts);
  return 0;
}

// mcs_ens_add_photons (deposit false) and mcs_ens_add_photons_deposit: one launch either way
static int add_photons(mcs_ens* e, mcs_ctx* src, int slot, const std::string& who, bool deposit) {
  if (!e || !src) return fail(who + ": null argument");
  if (species_slot(e, who, slot, "only a species slot has a photons slot")) return 1;
  if (!e->has_photon_layout()) return fail(who + ": no photon layout (mcs_ens_set_photon_layout)");
  McsCtxView v;
  if (view_of(e, src, who.c_str(), &v)) return 1;
  PhotonSrc S{};
  bool any = false;
  for (int p = 0; p < 3; ++p) {
    S.n[p] = e->ph_n[p]; S.start[p] = e->ph_start[p];
    if (v.pobs_n[p] == 0 || !v.pobs[p]) continue;
    if (v.pobs_n[p] != e->ph_n[p] || v.pobs_shells[p] != e->ph_shells)
      return fail(who + ": process " + std::to_string(p) + " was observed with " + std::to_string(v.pobs_shells[p]) + " shells of " + std::to_string(v.pobs_n[p]) +
                  " energy words, the layout has " + std::to_string(e->ph_shells) + " of " + std::to_string(e->ph_n[p]));
    S.obs[p] = v.pobs[p];
    any = true;
  }
  if (!any) return fail(who + ": the context holds no mcs_photon_observe result since its last mcs_begin_species, tally write or photons sample");
  S.off[0] = e->HL.synch; S.off[1] = e->HL.ic; S.off[2] = e->HL.pion; S.off[3] = e->HL.total_section;
  S.n_shells = e->ph_shells; S.n_pts = e->ph_npts; S.total = e->HL.total;
  if (deposit) {
    for (int s : e->deposited)
      if (s == slot) return fail(who + ": species slot " + std::to_string(slot) + " has been deposited since the last mcs_ens_add_photons_all");
    const hipError_t a = e->pending.reserve(e->HL.total);
    if (a != hipSuccess) return fail(who + ": hipMalloc: " + hipGetErrorString(a));
  }
  if (enter(e, v.stream)) return 1;
  Slot& sl = e->photons[(size_t)slot];
  if (reserve(sl, e->HL.total, who, v.stream)) return 1;
  if (deposit)
    hipLaunchKernelGGL(mcs_k_ens_add_photons_deposit, dim3(grid_for(S.total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), S,
                       (double)(sl.n + 1), e->pending.get(), e->deposited.empty() ? 1 : 0);
  else
    hipLaunchKernelGGL(mcs_k_ens_add_photons, dim3(grid_for(S.total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), S, (double)(sl.n + 1));
  ENSCHK(hipGetLastError());
  sl.n += 1;
  e->photons_sampled = true;
  if (deposit) e->deposited.push_back(slot);
  mcs_ctx_view_photons_taken(src);
  return leave(e, v.stream);
}

int mcs_ens_add_photons(mcs_ens* e, mcs_ctx* src, int slot) { return add_photons(e, src, slot, "mcs_ens_add_photons", false); }

int mcs_ens_add_photons_deposit(mcs_ens* e, mcs_ctx* src, int slot) { return add_photons(e, src, slot, "mcs_ens_add_photons_deposit", true); }

int mcs_ens_add_photons_all(mcs_ens* e) {
  const std::string who = "mcs_ens_add_photons_all";
  if (!e) return fail(who + ": null argument");
  if (e->deposited.empty()) return fail(who + ": no deposit pending (mcs_ens_add_photons_deposit)");
  McsCtxView v;
  if (mcs_ctx_view_get(e->home, &v)) return 1;
  if (enter(e, v.stream)) return 1;
  Slot& sl = e->source;
  if (reserve(sl, e->HL.total, who, v.stream)) return 1;
  hipLaunchKernelGGL(mcs_k_ens_add_vector, dim3(grid_for(e->HL.total)), dim3(ENS_THREADS), 0, v.stream, sl.mean.get(), sl.m2.get(), e->pending.get(),
                     (long long)e->HL.total, (double)(sl.n + 1));
  ENSCHK(hipGetLastError());
  sl.n += 1;
  e->photons_sampled = true;
  e->deposited.clear();
  return leave(e, v.stream);
}

int mcs_ens_drop_pending_photons(mcs_ens* e) {
  if (!e) return fail("mcs_ens_drop_pending_photons: null argument");
  e->deposited.clear();
  return 0;
}

int mcs_ens_merge(mcs_ens* dst, mcs_ens* src) {
  if (!dst || !src) return fail("mcs_ens_merge: null argument");
  if (dst == src) return fail("mcs_ens_merge: dst and src are the same accumulator");
  if (dst->device != src->device) return fail("mcs_ens_merge: the accumulators are on different devices");
  if (dst->n_slots != src->n_slots || !same_layout(dst, src)) return fail("mcs_ens_merge: the accumulators' slots or layouts differ");
  if (windows_differ(dst, src)) return fail("mcs_ens_merge: the accumulators' slope windows differ");
  if (photon_layouts_differ(dst, src)) return fail("mcs_ens_merge: the accumulators' photon layouts differ");
  if (angle_windows_differ(dst, src)) return fail("mcs_ens_merge: the accumulators' angle windows differ");
  if (tcuts_differ(dst, src)) return fail("mcs_ens_merge: the accumulators' tcuts samples differ in n_tcuts");
  if (profiles_differ(dst, src)) return fail("mcs_ens_merge: the settings of the accumulators' profile samples differ");
  if (detectors_differ(dst, src)) return fail("mcs_ens_merge: the settings of the accumulators' detectors samples differ");
  McsCtxView v;
  if (mcs_ctx_view_get(dst->home, &v)) return 1;
  const std::vector<int> slots = dst->slot_numbers();
  bool any[N_KINDS] = {};      // per kind: src has samples in a slot of it
  for (int slot : slots) {
    const SlotId id = decode(slot, src->n_slots);
    any[id.kind] = any[id.kind] || src->at(id).n > 0;
  }
  const bool any_products = any[PRODUCTS] || any[ESCAPE], any_photons = any[PHOTONS] || any[SOURCE];
  if (any_products && !dst->has_window()) {
    hipError_t a = dst->x_log.reserve((long long)src->x_log_h.size());
    if (a == hipSuccess) a = dst->slope.reserve(3LL * dst->P.n_grid);
    if (a != hipSuccess) return fail(std::string("mcs_ens_merge: hipMalloc: ") + hipGetErrorString(a));
  }
  if (enter(dst, v.stream) || enter(src, v.stream)) return 1;
  // an accumulator without a window or a photon layout takes the one its samples were made with
  if (any_products && !dst->has_window()) {
    ENSCHK(hipMemcpyAsync(dst->x_log.get(), src->x_log.get(), src->x_log_h.size() * sizeof(double), hipMemcpyDeviceToDevice, v.stream));
    dst->x_log_h = src->x_log_h; dst->win_lo = src->win_lo; dst->win_hi = src->win_hi;
  }
  if (any_photons && !dst->has_photon_layout()) photon_layout_take(dst, src->ph_shells, src->ph_n, src->ph_start, src->ph_npts);
  if (any[ANGLES] && !dst->has_angle_windows()) angle_windows_take(dst, src->ang_n_win, src->ang_lo, src->ang_hi);
  if (any[TCUTS] && !dst->has_tcuts()) tcuts_take(dst, src->tc_n);
  if (any[PROFILE] && !dst->has_profile()) profile_take(dst, src->prof_set);
  if (any[DETECTORS] && !dst->has_detectors()) detectors_take(dst, src->det_n, src->det_lo, src->det_hi, src->det_x_unit, src->det_x_spec.data());
  // (the source slot merges like a photons slot; what is pending on either side stays where it is)
  for (int slot : slots) {
    const SlotId id = decode(slot, dst->n_slots);
    if (merge_slot(dst->at(id), src->at(id), dst->len(id.kind), v.stream)) return 1;
  }
  dst->products_sampled = dst->products_sampled || any_products;
  dst->photons_sampled = dst->photons_sampled || any_photons;
  dst->angles_sampled = dst->angles_sampled || any[ANGLES];
  if (leave(dst, v.stream)) return 1;
  return leave(src, v.stream);
}

int mcs_ens_count(mcs_ens* e, int slot, int64_t* n) {
  if (!e || !n) return fail("mcs_ens_count: null argument");
  SlotRef r;
  if (slot_ref(e, "mcs_ens_count", slot, &r)) return 1;
  *n = r.slot->n;
  return 0;
}

int mcs_ens_read(mcs_ens* e, int slot, int what, int64_t first, int64_t count, double* host) {
  if (!e || (count > 0 && !host)) return fail("mcs_ens_read: null argument");
  SlotRef r;
  if (slot_ref(e, "mcs_ens_read", slot, &r)) return 1;
  if (what < 0 || what > 2) return fail("mcs_ens_read: what must be 0 (mean), 1 (M2) or 2 (standard error)");
  if (first < 0 || count < 0 || first + count > r.len) return fail("mcs_ens_read: range outside the slot's sample vector");
  const long long n = r.slot->n;
  if (r.kind >= PRODUCTS && n == 0) return fail(std::string("mcs_ens_read: the ") + KIND_NAME[r.kind] + " slot has never taken a sample");
  if (what == 2 && n < 2) return fail("mcs_ens_read: the standard error needs at least two samples; the slot has " + std::to_string(n));
  McsCtxView v;
  if (mcs_ctx_view_get(e->home, &v)) return 1;
  if (enter(e, v.stream)) return 1;
  const double* from = what == 0 ? r.slot->mean.get() : r.slot->m2.get();
  if (count > 0) ENSCHK(hipMemcpyAsync(host, from + first, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, v.stream));
  ENSCHK(hipStreamSynchronize(v.stream));
  if (what == 2) {
    const double denom = (double)n * (double)(n - 1);
    for (int64_t k = 0; k < count; ++k) host[k] = std::sqrt(host[k] / denom);
  }
  return 0;
}

int mcs_ens_summarize(mcs_ens* e, int slot, int n_ranges, const mcs_ens_range* ranges, mcs_ens_summary* out) {
  const std::string who = "mcs_ens_summarize";
  if (!e) return fail(who + ": null argument");
  SlotRef sr;
  if (slot_ref(e, who, slot, &sr)) return 1;
  if (n_ranges < 0 || n_ranges > SUM_MAX_RANGES) return fail(who + ": n_ranges outside 0.." + std::to_string(SUM_MAX_RANGES));
  if (n_ranges == 0) return 0;
  if (!ranges || !out) return fail(who + ": null argument");
  const long long n = sr.slot->n;
  if (n < 2) return fail(who + ": the standard error needs at least two samples; the slot has " + std::to_string(n));
  long long n_blocks = 0;
  if (plan_ranges(who, e, sr.len, n_ranges, ranges, &mcs_ens_range::tol, "tol", &n_blocks)) return 1;
  mcs_ens* list[1] = {e};
  return sum_run(who, list, 1, SrcOne{sr.slot->mean, sr.slot->m2}, n, n_ranges, n_blocks, out);
}

int mcs_ens_summarize_merged(int n_ens, mcs_ens* const* ens, int slot, int n_ranges, const mcs_ens_range* ranges, mcs_ens_summary* out,
                             int64_t* n_total) {
  const std::string who = "mcs_ens_summarize_merged";
  if (!ens || !n_total) return fail(who + ": null argument");
  if (n_ens < 1 || n_ens > MCS_ENS_MAX_MERGED) return fail(who + ": n_ens outside 1.." + std::to_string(MCS_ENS_MAX_MERGED));
  for (int k = 0; k < n_ens; ++k) {
    if (!ens[k]) return fail(who + ": null argument (accumulator " + std::to_string(k) + " of the list)");
    for (int j = 0; j < k; ++j)
      if (ens[j] == ens[k]) return fail(who + ": accumulators " + std::to_string(j) + " and " + std::to_string(k) + " of the list are the same one");
  }
  mcs_ens* a = ens[0];
  for (int k = 1; k < n_ens; ++k) {
    const mcs_ens* b = ens[k];
    if (a->device != b->device) return fail(who + ": the accumulators are on different devices");
    if (a->n_slots != b->n_slots || !same_layout(a, b)) return fail(who + ": the accumulators' slots or layouts differ");
  }
  SlotRef sr;
  if (slot_ref(a, who, slot, &sr)) return 1;
  if (has_window_vector(sr.kind))
    for (int k = 1; k < n_ens; ++k)
      for (int j = 0; j < k; ++j)
        if (windows_differ(ens[j], ens[k])) return fail(who + ": the accumulators' slope windows differ");
  long long len = sr.len;
  if (sr.kind == ANGLES)
    for (int k = 1; k < n_ens; ++k) {
      for (int j = 0; j < k; ++j)
        if (angle_windows_differ(ens[j], ens[k])) return fail(who + ": the accumulators' angle windows differ");
      if (ens[k]->len(sr.kind) > len) len = ens[k]->len(sr.kind);      // (an accumulator without windows has no angles sample)
    }
  if (sr.kind == TCUTS)
    for (int k = 1; k < n_ens; ++k) {
      for (int j = 0; j < k; ++j)
        if (tcuts_differ(ens[j], ens[k])) return fail(who + ": the accumulators' tcuts samples differ in n_tcuts");
      if (ens[k]->len(sr.kind) > len) len = ens[k]->len(sr.kind);      // (an accumulator that took no tcuts sample has no length)
    }
  if (sr.kind == PROFILE)
    for (int k = 1; k < n_ens; ++k) {
      for (int j = 0; j < k; ++j)
        if (profiles_differ(ens[j], ens[k])) return fail(who + ": the settings of the accumulators' profile samples differ");
      if (ens[k]->len(sr.kind) > len) len = ens[k]->len(sr.kind);      // (an accumulator that took no profile sample has no length)
    }
  if (sr.kind == DETECTORS)
    for (int k = 1; k < n_ens; ++k) {
      for (int j = 0; j < k; ++j)
        if (detectors_differ(ens[j], ens[k])) return fail(who + ": the settings of the accumulators' detectors samples differ");
      if (ens[k]->len(sr.kind) > len) len = ens[k]->len(sr.kind);      // (an accumulator that took no detectors sample has no length)
    }
  if (has_photon_vector(sr.kind))
    for (int k = 1; k < n_ens; ++k) {
      for (int j = 0; j < k; ++j)
        if (photon_layouts_differ(ens[j], ens[k])) return fail(who + ": the accumulators' photon layouts differ");
      if (ens[k]->len(sr.kind) > len) len = ens[k]->len(sr.kind);      // (an accumulator without a layout has no photons sample)
    }
  if (n_ranges < 0 || n_ranges > SUM_MAX_RANGES) return fail(who + ": n_ranges outside 0.." + std::to_string(SUM_MAX_RANGES));
  if (n_ranges > 0 && (!ranges || !out)) return fail(who + ": null argument");
  // the accumulators that have samples in this slot, in list order, and the factors of every step of the fold (as mcs_ens_merge)
  mcs_ens* list[MCS_ENS_MAX_MERGED];
  const double *mean[MCS_ENS_MAX_MERGED], *m2[MCS_ENS_MAX_MERGED];
  double f_mean[MCS_ENS_MAX_MERGED], f_m2[MCS_ENS_MAX_MERGED];
  long long n = 0;
  int m = 0;
  for (int k = 0; k < n_ens; ++k) {
    list[k] = ens[k];
    (void)slot_ref(ens[k], who, slot, &sr);      // (the slot exists in every accumulator: their slots are the same)
    const long long nb = sr.slot->n;
    if (nb == 0) continue;
    const double nn = (double)(n + nb);
    f_mean[m] = m ? (double)nb / nn : 0.0;
    f_m2[m] = m ? (double)n * (double)nb / nn : 0.0;
    mean[m] = sr.slot->mean; m2[m] = sr.slot->m2;
    n += nb; ++m;
  }
  if (n < 2) return fail(who + ": the standard error needs at least two samples; the slot has " + std::to_string(n) + " over the list");
  long long n_blocks = 0;
  if (plan_ranges(who, a, len, n_ranges, ranges, &mcs_ens_range::tol, "tol", &n_blocks)) return 1;
  *n_total = n;
  if (n_ranges == 0) return 0;
  switch (m) {
    case 1: return sum_run(who, list, n_ens, SrcOne{mean[0], m2[0]}, n, n_ranges, n_blocks, out);
    case 2: return sum_run(who, list, n_ens, merged_src<2>(mean, m2, f_mean, f_m2), n, n_ranges, n_blocks, out);
    case 3: return sum_run(who, list, n_ens, merged_src<3>(mean, m2, f_mean, f_m2), n, n_ranges, n_blocks, out);
    case 4: return sum_run(who, list, n_ens, merged_src<4>(mean, m2, f_mean, f_m2), n, n_ranges, n_blocks, out);
    case 5: return sum_run(who, list, n_ens, merged_src<5>(mean, m2, f_mean, f_m2), n, n_ranges, n_blocks, out);
    case 6: return sum_run(who, list, n_ens, merged_src<6>(mean, m2, f_mean, f_m2), n, n_ranges, n_blocks, out);
    case 7: return sum_run(who, list, n_ens, merged_src<7>(mean, m2, f_mean, f_m2), n, n_ranges, n_blocks, out);
    default: return sum_run(who, list, n_ens, merged_src<8>(mean, m2, f_mean, f_m2), n, n_ranges, n_blocks, out);
  }
}

int mcs_ens_compare(mcs_ens* a, int slot_a, mcs_ens* b, int slot_b, int n_ranges, const mcs_ens_cmp_range* ranges, mcs_ens_difference* out) {
  const std::string who = "mcs_ens_compare";
  if (!a || !b) return fail(who + ": null argument");
  SlotRef ra, rb;
  if (slot_ref(a, who + " (A)", slot_a, &ra) || slot_ref(b, who + " (B)", slot_b, &rb)) return 1;
  if (a == b && slot_a == slot_b) return fail(who + ": A and B are the same slot of the same accumulator");
  if (a->device != b->device) return fail(who + ": the accumulators are on different devices");
  if (!same_layout(a, b)) return fail(who + ": the accumulators' layouts differ");
  const Slot &sa = *ra.slot, &sb = *rb.slot;
  const long long len = ra.len;
  if (ra.kind == TCUTS && rb.kind == TCUTS && tcuts_differ(a, b)) return fail(who + ": the accumulators' tcuts samples differ in n_tcuts");
  if (ra.kind == PROFILE && rb.kind == PROFILE && profiles_differ(a, b)) return fail(who + ": the settings of the accumulators' profile samples differ");
  if (ra.kind == DETECTORS && rb.kind == DETECTORS && detectors_differ(a, b)) return fail(who + ": the settings of the accumulators' detectors samples differ");
  if (ra.kind != rb.kind || len != rb.len) return fail(who + ": the two slots differ in kind or length");
  if (n_ranges < 0 || n_ranges > SUM_MAX_RANGES) return fail(who + ": n_ranges outside 0.." + std::to_string(SUM_MAX_RANGES));
  if (n_ranges == 0) return 0;
  if (!ranges || !out) return fail(who + ": null argument");
  if (has_window_vector(ra.kind)) {
    if (sa.n == 0 || sb.n == 0) return fail(who + (ra.kind == ESCAPE ? ": an escape" : ": a products") + " slot has never taken a sample");
    if (windows_differ(a, b)) return fail(who + ": the accumulators' slope windows differ");
  }
  if (ra.kind == ANGLES) {
    if (sa.n == 0 || sb.n == 0) return fail(who + ": an angles slot has never taken a sample");
    if (angle_windows_differ(a, b)) return fail(who + ": the accumulators' angle windows differ");
  }
  if (ra.kind == TCUTS) {
    if (sa.n == 0 || sb.n == 0) return fail(who + ": a tcuts slot has never taken a sample");
  }
  if (ra.kind == PROFILE) {
    if (sa.n == 0 || sb.n == 0) return fail(who + ": a profile slot has never taken a sample");
  }
  if (ra.kind == DETECTORS) {
    if (sa.n == 0 || sb.n == 0) return fail(who + ": a detectors slot has never taken a sample");
  }
  if (has_photon_vector(ra.kind)) {
    if (sa.n == 0 || sb.n == 0) return fail(who + ": a photons slot has never taken a sample");
    if (photon_layouts_differ(a, b)) return fail(who + ": the accumulators' photon layouts differ");
  }
  if (sa.n < 2 || sb.n < 2)
    return fail(who + ": a standard error needs at least two samples; A has " + std::to_string(sa.n) + ", B has " + std::to_string(sb.n));
  long long n_blocks = 0;
  if (plan_ranges(who, a, len, n_ranges, ranges, &mcs_ens_cmp_range::zcut, "zcut", &n_blocks)) return 1;
  McsCtxView v;
  if (mcs_ctx_view_get(a->home, &v)) return 1;
  if (reserve_scratch(who, a, a->cmp_out_h, a->cmp_out, a->cmp_part, n_blocks)) return 1;
  if (enter(a, v.stream) || (b != a && enter(b, v.stream))) return 1;
  const SrcCmp src{sa.mean, sa.m2, sb.mean, sb.m2, (double)sa.n * (double)(sa.n - 1), (double)sb.n * (double)(sb.n - 1)};
  ENSCHK(hipMemcpyAsync(a->sum_par.get(), a->sum_par_h.get(), sizeof(SumParams), hipMemcpyHostToDevice, v.stream));
  if (n_blocks > 0) {
    hipLaunchKernelGGL(mcs_k_ens_cmp_amax, dim3((unsigned)n_blocks), dim3(ENS_THREADS), 0, v.stream, src, a->sum_par.get(), a->sum_pmax.get());
    ENSCHK(hipGetLastError());
    hipLaunchKernelGGL(mcs_k_ens_cmp_stats, dim3((unsigned)n_blocks), dim3(ENS_THREADS), 0, v.stream, src, a->sum_par.get(), a->sum_pmax.get(),
                       a->cmp_part.get());
    ENSCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(mcs_k_ens_cmp_final, dim3((unsigned)n_ranges), dim3(ENS_THREADS), 0, v.stream, a->sum_par.get(), a->cmp_part.get(), a->cmp_out.get());
  ENSCHK(hipGetLastError());
  ENSCHK(hipMemcpyAsync(a->cmp_out_h.get(), a->cmp_out.get(), (size_t)n_ranges * sizeof(CmpRec), hipMemcpyDeviceToHost, v.stream));
  ENSCHK(hipStreamSynchronize(v.stream));
  const CmpRec* got = a->cmp_out_h.get();
  for (int r = 0; r < n_ranges; ++r) {
    const CmpRec& g = got[r];
    out[r] = mcs_ens_difference{g.amax, g.max_z, g.sum_z, g.sum_abs_z, g.sum_z2, g.sum_diff, g.sum_scale, g.n_sel, g.n_over, g.n_nonf, g.n_degen, g.arg};
  }
  return 0;
}

int mcs_ens_load_mean(mcs_ens* e, int slot, mcs_ctx* dst) {
  if (!e || !dst) return fail("mcs_ens_load_mean: null argument");
  if (species_slot(e, "mcs_ens_load_mean", slot, "only a species slot has histograms")) return 1;
  McsCtxView v;
  if (view_of(e, dst, "mcs_ens_load_mean", &v)) return 1;
  if (enter(e, v.stream)) return 1;
  hipLaunchKernelGGL(mcs_k_ens_load_mean, dim3(grid_for(e->E.sp_psd_mom)), dim3(ENS_THREADS), 0, v.stream, e->main[(size_t)slot].mean.get(), v.T, v.I, e->E);
  ENSCHK(hipGetLastError());
  mcs_ctx_view_tallies_written(dst);
  return leave(e, v.stream);
}

}  // extern "C"

// mcs_api.hip -- the C ABI of include/mcs.h over the gfx950 kernels.
//
// A context owns: device mirrors of the grid/cut tables, the resident particle
// population (three rotating SoA buffers: current, saved and the target of the next
// split; a second saved set for the pipelined loop) and, unless the caller binds its
// own (mcs_bind_tallies), the flat fp64/int64 tally buffers.  Every block of memory,
// stream and event is a member of an owning type of mcs_hip_owned.h: deleting the
// context releases them, a failed allocation leaves its owner empty.  All work is
// queued on ONE HIP stream (the pipelined loop adds a side stream); mcs_run_pcut is
// synchronous only for the 8-byte n_saved.  There is no CPU code path in this library.
#include "mcs_launch.h"      // (and mcs_device.h)
#include "mcs_hip_owned.h"
#include "mcs_ctx_view.h"
#include "../../include/mcs_ic.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <chrono>
#include <cstdarg>
#include <memory>
#include <utility>

#define MCS_MEV_ERG_ 1.602176634e-6
namespace {
thread_local std::string g_err;

int fail(const std::string& msg) { g_err = msg; return 1; }
#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)
// The top of every ABI call that takes a context and returns a status: a null context is an error, else its device is made current.
#define MCS_ENTER_AS(c, who) do { if (!(c)) return fail(std::string(who) + ": null context"); HIPCHK(hipSetDevice((c)->device)); } while (0)
#define MCS_ENTER(c) MCS_ENTER_AS(c, __func__)

std::string format(const char* f, ...) {
  char b[320];
  va_list ap; va_start(ap, f); std::vsnprintf(b, sizeof b, f, ap); va_end(ap);
  return b;
}
// reserve() of a DevBuf, PinnedBuf or PopBuf as a step of an ABI call
template <class B> int reserve(B& b, long long n) {
  const hipError_t e = b.reserve(n);
  return e == hipSuccess ? 0 : fail(std::string(B::alloc_name()) + ": " + hipGetErrorString(e));
}

// the eight fp64 fields of a particle, in the order of PopBuf::f
constexpr double* DevPop::*kPopF64[8] = {&DevPop::weight, &DevPop::ptot_pf, &DevPop::pb_pf, &DevPop::x_PT_cm,
                                         &DevPop::xn_per, &DevPop::prp_x_cm, &DevPop::acctime_sec, &DevPop::phi_rad};
constexpr double* mcs_soa::*kSoaF64[8] = {&mcs_soa::weight, &mcs_soa::ptot_pf, &mcs_soa::pb_pf, &mcs_soa::x_PT_cm,
                                          &mcs_soa::xn_per, &mcs_soa::prp_x_cm, &mcs_soa::acctime_sec, &mcs_soa::phi_rad};
// what the kernels take: the arrays of b, from particle `first` on
DevPop pop_view(const PopBuf& b, long long first = 0) {
  DevPop d{};
  for (int i = 0; i < 8; ++i) d.*kPopF64[i] = b.f[i] + first;
  d.meta = b.meta + first;
  return d;
}

// two export buffers of cap() lane states each (sliced launches): a launch resumes from one and exports into the other
struct StragBuf : BufGroup<StragBuf> {
  DevBuf<double> d[2];
  long long cap() const { return d[1].cap() / MCS_STRAG_WORDS; }
  hipError_t grow(long long n) { return reserve_all({n * MCS_STRAG_WORDS, n * MCS_STRAG_WORDS}, d[0], d[1]); }
};
// the fused species loop's launch constants and device-decided words for cap() pcuts (one PcutDev more: the population after the last)
struct FusedBuf : BufGroup<FusedBuf> {
  PinnedBuf<KArgs> h_args; PinnedBuf<PcutDev> h_pd; DevBuf<KArgs> d_args; DevBuf<PcutDev> d_pd;
  long long cap() const { return d_args.cap(); }
  hipError_t grow(long long n) { return reserve_all({n, n + 1, n, n + 1}, h_args, h_pd, d_args, d_pd); }
};

// The words of mcs_ctx::d_counters (h_back holds the host's copy of a word at the same index): the next unclaimed particle of a launch |
// the kernel's own count of saved particles | the compaction's count of l_save flags | EXPORT has TWO meanings: the particles a sliced
// launch exported, and the panic code of a wave-specialised launch (which is never sliced) | fused loop: set on the device when SAVED and
// SCAN of some pcut differed.
enum Ctr { CTR_WORK, CTR_SAVED, CTR_SCAN, CTR_EXPORT, CTR_MISMATCH, CTR_COUNT = 8 };
// The pipelined loop's own words (pp_dpc; pp_hpc is the host's copy), a work / saved pair for every launch that can be in flight at once:
// the main launch's pair | count of the main group's saved particles that are not long | EXPORT + q: particles exported by the launches of
// pcut parity q (two words) | the pair of the resumed long histories | the late launch's pair | count of the saved long particles.
enum PipeCtr { PC_WORK, PC_SAVED, PC_SCAN, PC_EXPORT, PC_RES_WORK = PC_EXPORT + 2, PC_RES_SAVED, PC_LATE_WORK, PC_LATE_SAVED, PC_LATE_SCAN, PC_COUNT = 16 };
// points a launch at its own words of `ctr`
void set_counters(KArgs& a, unsigned long long* ctr, int work, int saved, int exported) {
  a.work_counter = ctr + work; a.n_saved = ctr + saved; a.strag_count = ctr + exported;
}
}  // namespace

struct mcs_ctx {
  mcs_params P;
  mcs_layout L;
  int device = 0;
  Stream own_stream;           // (first member: destroyed after everything that was used on it)
  hipStream_t stream = nullptr;     // own_stream, or the caller's
  // tables
  DevBuf<double> d_tab;        // 8 tables x (n_grid+2)
  DevBuf<double> d_cuts;       // pcuts | tcuts | x_spec | inj_fracs | eps_target
  DevTables tb{};
  std::vector<double> h_inj_fracs, h_pcuts, h_ux;
  // tallies
  DevBuf<double> own_T; DevBuf<unsigned long long> own_I;
  double* d_T = nullptr; unsigned long long* d_I = nullptr;      // own_T / own_I, or the caller's (mcs_bind_tallies)
  // population
  PopBuf cur, sav, spare;      // spare: target of the next split (buffers rotate, no per-pcut allocation)
  DevBuf<uint8_t> d_lsave;
  long long n = 0;             // current population size
  long long n_saved_last = 0;
  long long n_run_last = 0;    // population size of the last mcs_run_pcut (the saved arrays and src[] refer to it)
  long long idx_first = 0, idx_stride = 1;   // global index of local particle k in that run: idx_first + k * idx_stride
  const long long* idx_gidx = nullptr;       // ... or idx_gidx[k] (mcs_run_pcut_indexed; caller-owned device memory)
  bool debug_finals = false;   // mcs_set_debug_finals: record per-particle end states (tests)
  int retro_cap = MCS_RETRO_CAP;
  // sliced tail (mcs_set_tail_slicing; KArgs "sliced launches"): after the queue is exhausted a wave makes tail_budget more trips,
  // exports its live particles and ends; the host relaunches them, spread over the chip's waves, until none is left
  // (the budget, in trips, is MCS_OPT_TAIL_BUDGET; 0 = one launch per pcut, run to the end)
  int tail_rounds_last = 0;    // launches the last mcs_run_pcut* took
  StragBuf strag;
  // The run options (enum mcs_option of include/mcs.h, one value per key; the table of mcs_options.h says what each allows): set at
  // creation from the built-in defaults, the environment and the caller's list, changed by mcs_set_option, read where a launch is
  // planned.  Notes on some of them:
  //   F32_EXACT  the plain loop with the exact fp32 primitives (include/mcs_math_f32.h): the kernel the CPU restatement
  //              oracle/mcs_oracle_f32.inc reproduces bit for bit (tests)
  //   F32_LOOP   the fp32-state variant as a plain per-lane loop (the reference semantics of that variant; tests)
  //   K1_WS      the wave-specialised kernels (mcs_transport_ws.inc), where they apply: 1 always, 0 never, 2 (default) for populations of
  //              at least WS_AUTO_MIN particles -- measured level with transport_body at 4e6 particles, 3.8 % faster at 1e7 and 7 % slower
  //              at 2e6, where its missing tail consolidation shows (profiles/r04_ws_kernel_ab.txt)
  //   TAIL_RING, TAIL_LOOP, REFILL_MIN, DEFER_K, PARK, TAIL_MERGE   A/B measurements of the tail's parts
  int64_t opt[MCS_OPT_COUNT] = {};
  long long o(int key) const { return opt[key]; }
  FinalsBuf fin; ScanScratch scan;      // the end states of a debug run; the compaction's scratch (src[]: the saved particles' indices)
  DevBuf<double> d_tally_rep;                  // replicas of the histograms at the head of the tally buffer (KArgs::tally_rep)
  long long rep_n = 0;                         // doubles per replica (0: no replicas)
  bool rep_dirty = false;                    // a launch may have added to the replicas since the last fold
  DevBuf<unsigned long long> d_counters;      // CTR_COUNT words, named by enum Ctr above
  // staging for init_pop
  DevBuf<double> d_stage;
  // launch constants: host copy in PINNED memory (the upload is then a true async copy: no staging through the runtime's
  // bounce buffer, ~10 us per pcut) and device copy; read-back words of a pcut, pinned for the same reason
  PinnedBuf<KArgs> h_args_pin; DevBuf<KArgs> d_args;
  PinnedBuf<unsigned long long> h_back;       // the words of d_counters a call reads back, each at its own index
  // species
  int i_iter = 1, i_ion = 1;
  double aa = 1, zzq = MCS_QCGS, m = MCS_MP, mc = MCS_MP * MCS_C, pmax_cutoff = 0, density = 1, ewf = 1;
  bool have_grid = false, have_cuts = false;
  bool all_parallel = false;   // theta == 0 in every zone (mcs_set_grid)
  int kernel_last = -1;        // mcs_last_kernel
  // fused species loop (mcs_run_pcuts_fused): launch constants of every pcut (pinned + device), the per-pcut words decided on the
  // device, one event pair per pcut
  FusedBuf fused;
  std::vector<Event> f_ev;
  // pipelined pcut loop (mcs_run_pcuts_pipelined): the side stream on which a pcut's long histories finish while the next pcut runs,
  // the second set of saved arrays / status bytes (pcut p's are still written while pcut p + 1 runs), the late group's scan scratch,
  // per-launch counters (device, and pinned for the one read-back per pcut), three launch-constant slots, the late group's sizes
  Stream pp_s2; Event pp_reset;
  // ... and, when the runtime grants them, two streams with complementary CU masks: the side stream's waves then have their SIMDs to
  // themselves (beside a wave of the main launch on the same SIMD a long history advances at half the speed -- the kernel is issue-bound
  // -- and the side chain, not the main launch, ends the pcut); a pcut with side work runs its main launch on the masked main stream
  Stream pp_s1m, pp_s2m; bool pp_masks_tried = false;      // (MCS_OPT_PIPE_SIDE_CUS of the chip's CUs for the side stream; 0: no masks)
  PopBuf pp_sav2; DevBuf<uint8_t> pp_lsave2; ScanScratch pp_scan;
  DevBuf<unsigned long long> pp_dpc; PinnedBuf<unsigned long long> pp_hpc;      // PC_COUNT words, named by enum PipeCtr above
  PinnedBuf<KArgs> pp_hargs; DevBuf<KArgs> pp_dargs; DevBuf<PcutDev> pp_dpdl; PinnedBuf<PcutDev> pp_hpdl;
  int pp_waits_last = 0;       // pcuts of the last pipelined run whose i_mult had to wait for the long histories
  // consumers (K4): table staging, outputs, thermo scratch slab
  DevBuf<double> d_ctab, d_cout, d_cscratch; DevBuf<unsigned long long> d_cdiag;
  // d_cout holds the result of a whole mcs_dndp_cr / mcs_thermo_calcs: each consumer sets its own flag, mcs_begin_species and a
  // products sample of the ensemble statistics (mcs_ens_add_products) clear both.  No other call writes d_cout: mcs_dndp_2d writes
  // d_cscratch and d_c2d (consumers_ready only sizes d_cout, whose size never changes), the photon folds stage their inputs in d_stage and
  // write d_pemis (below).
  bool have_cout_dndp = false, have_cout_thermo = false;
  // K10: what the last mcs_dndp_esc left, dNdp [2][3][nmom+2] then number [2][3]; have_esc: a whole result since the last
  // mcs_begin_species and the last escape sample of the ensemble statistics.  Only that call writes it, its row scratch and its counts.
  DevBuf<double> d_esc_out, d_esc_rows; DevBuf<unsigned int> d_esc_rowdiag; DevBuf<unsigned long long> d_esc_diag;
  bool have_esc = false;
  // K11: what the last mcs_angle_dist left, in the layout of an angles sample (dist | number | mean_mu | mean_mu2), its tables and
  // its windows; have_ang: a whole result since the last mcs_begin_species, tally write and angles sample.  Only that call writes them.
  DevBuf<double> d_ang_out, d_ang_tab;
  bool have_ang = false;
  int ang_n_win = 0;
  int32_t ang_lo[MCS_ANGLE_MAX_WINDOWS] = {}, ang_hi[MCS_ANGLE_MAX_WINDOWS] = {};
  // K12: d_tcut_base, the current species' block of spectra_coupled as mcs_begin_species found it ([MCS_NA_C][201]; taken only with
  // do_tcuts); what the last mcs_tcut_spectra left, in mcs_tcut_layout, its n_tcuts and its counts; have_tcut: a whole result since the
  // last mcs_begin_species and the last tcuts sample.  Only those two calls write them.  species_begun: mcs_begin_species has run.
  DevBuf<double> d_tcut_base, d_tcut_out; DevBuf<unsigned int> d_tcut_rowneg; DevBuf<unsigned long long> d_tcut_diag;
  bool have_tcut = false, species_begun = false;
  int tcut_n = 0;
  // K13: what the last mcs_profile_update left, in mcs_profile_layout, its counts, its tables (pxx_EM | en_EM | atan_x, then the caller's
  // pressures when it passed some) and the settings of its mcs_profile_in; have_prof: a whole result since the last mcs_begin_species,
  // tally write and profile sample.  Only that call writes them.
  DevBuf<double> d_prof_out, d_prof_tab; DevBuf<unsigned long long> d_prof_diag;
  bool have_prof = false;
  mcs_profile_in prof_in{};
  // K14: d_det_base, rows 0..nd-1 of spectra_sf and spectra_pf as mcs_begin_species found them ([2][nd][201]; taken only with cuts set
  // and n_xspec >= 1; have_det_base: there is one for the cuts in force); what the last mcs_detector_spectra left, in
  // mcs_detector_layout, its counts and its settings; have_det: a whole result since the last mcs_begin_species, mcs_set_cuts and
  // detectors sample.  h_x_spec: the host copy of x_spec.
  DevBuf<double> d_det_base, d_det_out, d_det_tab; DevBuf<unsigned int> d_det_rowneg; DevBuf<unsigned long long> d_det_diag;
  bool have_det = false, have_det_base = false;
  int det_n = 0, det_lo = 0, det_hi = 0;
  double det_x_unit = 0.0;
  std::vector<double> h_x_spec;
  DevBuf<double> d_c2d; bool have_c2d = false;    // d2N/dp dcos of the last mcs_dndp_2d ([n_grid][ntht+2][nmom+2]), the input of mcs_photon_ic
  // K9, per process (MCS_PHOTON_SYNCH / _IC / _PION): d_pemis the emis[n_grid][n_photon] its fold left (pemis_n: that n_photon, 0 =
  // nothing), d_pobs the [n_shells+1][n] of the last mcs_photon_observe (pobs_n: its n, 0 = nothing; pobs_shells).  Only those calls
  // write them; mcs_begin_species, the tally writes and a photons sample of the ensemble statistics clear the flags (photon_flags_clear).
  // d_ptab / d_pnb: the tables and the per-zone spectra of one mcs_photon_observe.
  DevBuf<double> d_pemis[3], d_pobs[3], d_ptab, d_pnb;
  int pemis_n[3] = {0, 0, 0}, pobs_n[3] = {0, 0, 0}, pobs_shells[3] = {0, 0, 0};
  void photon_flags_clear() { for (int p = 0; p < 3; ++p) pemis_n[p] = pobs_n[p] = pobs_shells[p] = 0; }
  // launch
  int blocks = 0, threads = 256;
  Event ev0, ev1;
  Event acc_ev;                 // mcs_accumulate_tallies: orders the two contexts' streams (no timing; ev0 / ev1 time K1)
  double last_ms = 0.0;
  int n_cu = 256;
};

namespace {

int ensure_capacity(mcs_ctx* c, long long n) {
  // both buffers and every per-particle side array hold at least n entries
  if (n > c->cur.cap() || n > c->sav.cap()) {
    const long long cap = grow_cap(n);
    // growing must preserve the current population
    if (c->n > 0 && c->cur.cap() < cap) {
      PopBuf nb;
      if (reserve(nb, cap)) return 1;
      for (int i = 0; i < 8; ++i) HIPCHK(hipMemcpyAsync(nb.f[i], c->cur.f[i], (size_t)c->n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(nb.meta, c->cur.meta, (size_t)c->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      c->cur = std::move(nb);
    } else if (reserve(c->cur, cap)) return 1;
    if (reserve(c->sav, cap)) return 1;
  }
  if (n > c->d_lsave.cap() && reserve(c->d_lsave, grow_cap(n))) return 1;
  if (c->debug_finals && n > c->fin.cap() && reserve(c->fin, grow_cap(n))) return 1;
  if (n > c->scan.cap() && reserve(c->scan, grow_cap(n))) return 1;
  return 0;
}

// the grid of mcs_k_split_dev (grid-stride, 256 threads a block) for at most n_max children: per_cu blocks per CU at the most --
// 16 behind a fused pcut, 4 for a late group, which shares the chip with the next pcut's main launch --, one at the least
int split_blocks(const mcs_ctx* c, long long n_max, int per_cu) {
  const long long b = std::min<long long>((n_max + 255) / 256, (long long)c->n_cu * per_cu);
  return b < 1 ? 1 : (int)b;
}

int fill(mcs_ctx* c, long long off, long long n, double v) {
  HIPCHK(mcs_launch_fill(c->d_T + off, n, v, c->stream));
  return 0;
}

// host <-> packed device SoA
int upload_soa(mcs_ctx* c, const PopBuf& b, long long n, const mcs_soa* h) {
  for (int i = 0; i < 8; ++i) HIPCHK(hipMemcpyAsync(b.f[i], h->*kSoaF64[i], (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  std::vector<uint32_t> meta((size_t)n);
  for (long long k = 0; k < n; ++k) meta[k] = mcs_pack_meta((int)h->grid[k], (int)h->tcut[k], h->downstream[k] != 0, h->inj[k] != 0);
  HIPCHK(hipMemcpyAsync(b.meta, meta.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int download_soa(mcs_ctx* c, const PopBuf& b, long long n, mcs_soa* h) {
  for (int i = 0; i < 8; ++i) HIPCHK(hipMemcpyAsync(h->*kSoaF64[i], b.f[i], (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  std::vector<uint32_t> meta((size_t)n);
  HIPCHK(hipMemcpyAsync(meta.data(), b.meta, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (long long k = 0; k < n; ++k) {
    const uint32_t mm = meta[k];
    h->grid[k] = (int64_t)(mm & 0xffffu); h->tcut[k] = (int64_t)((mm >> 16) & 0xffu);
    h->downstream[k] = (uint8_t)((mm >> 24) & 1u); h->inj[k] = (uint8_t)((mm >> 25) & 1u);
  }
  return 0;
}

}  // namespace

extern "C" {

// The thermal histograms are tallied into MCS_TALLY_REPLICAS private copies (mcs_device.h); everything that reads
// or rewrites the tally buffer folds them in first.
static int fold_replicas(mcs_ctx* c) {
  if (!c->rep_dirty || !c->d_tally_rep) return 0;
  HIPCHK(mcs_launch_fold_replicas(c->d_T, c->d_tally_rep, c->rep_n, MCS_TALLY_REPLICAS, c->stream));
  c->rep_dirty = false;
  return 0;
}

int mcs_abi_version(void) { return MCS_ABI_VERSION; }
const char* mcs_last_error(void) { return g_err.c_str(); }
int mcs_get_layout(const mcs_params* p, mcs_layout* out) { mcs_tally_layout(p, out); return 0; }

int mcs_create(const mcs_params* p, int device, void* stream, mcs_ctx** out) {
  return mcs_create_with_options(p, device, stream, nullptr, nullptr, 0, 1, out);
}

int mcs_option_count(void) { return MCS_OPT_COUNT; }
int mcs_option_describe(int key, mcs_option_desc* out) {
  if (!out) return fail("mcs_option_describe: null argument");
  const McsOptionRow* r = mcs_option_row(key);
  if (!r) return fail(format("mcs_option_describe: unknown option key %d (the keys are 0..%d, enum mcs_option)", key, MCS_OPT_COUNT - 1));
  *out = mcs_option_desc{r->key, r->when, r->applies, 0, r->min, r->max, r->dflt, r->name, r->env};
  return 0;
}

int mcs_create_with_options(const mcs_params* p, int device, void* stream, const int32_t* keys, const int64_t* values, int n_options,
                            int use_env, mcs_ctx** out) {
  if (!p || !out) return fail("mcs_create: null argument");
  if (p->abi_version != MCS_ABI_VERSION) return fail("mcs_create: abi_version mismatch");
  if (p->use_custom_frg) return fail("Use of custom f(r_g) not yet supported. Add functionality or use standard. (src/scattering.jl:52-53)");
  if (!p->do_retro) return fail("Code not set up for analytical PRP calculations. (src/prob_return.jl:134)");
  if (p->num_psd_mom_bins + 1 > MCS_PSD_MAX || p->num_psd_tht_bins + 1 > MCS_PSD_MAX) return fail("mcs_create: psd bins exceed psd_max (src/parameters.jl:18)");
  if (p->n_grid < 1 || p->n_grid + 2 > mcs_transport_max_entries()) return fail("mcs_create: n_grid + 2 exceeds the LDS table size (208 entries; psd_max = 200 in src/parameters.jl:18)");
  // the options, before the device is touched: a bad list fails the same way without a GPU
  int64_t opt[MCS_OPT_COUNT];
  std::string why;
  if (mcs_options_resolve(keys, values, n_options, use_env != 0, p->state_fp32, opt, &why) != MCS_OPTION_OK)
    return fail("mcs_create_with_options: " + why);
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail("mcs_create: no HIP device visible; the transport path has no CPU fallback");
  if (device < 0 || device >= ndev) return fail("mcs_create: device ordinal out of range");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<mcs_ctx> c(new mcs_ctx());      // (a failing call below must not leak the context and what it has allocated so far)
  std::memcpy(c->opt, opt, sizeof opt);
  c->P = *p;
  mcs_tally_layout(p, &c->L);
  c->device = device;
  if (stream) c->stream = (hipStream_t)stream;
  else { HIPCHK(c->own_stream.create()); c->stream = c->own_stream; }
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  c->n_cu = prop.multiProcessorCount;
  const int ne = p->n_grid + 2;
  if (reserve(c->d_tab, (long long)8 * ne) || reserve(c->d_counters, CTR_COUNT) || reserve(c->d_args, 1) || reserve(c->h_args_pin, 1) ||
      reserve(c->h_back, CTR_COUNT))
    return 1;
  if (c->o(MCS_OPT_TALLY_REPLICAS)) {
    c->rep_n = c->L.total;     // the whole tally buffer: the three big histograms are 99 % of it
    const size_t nrep = (size_t)MCS_TALLY_REPLICAS * (size_t)c->rep_n;
    if (reserve(c->d_tally_rep, (long long)nrep)) return 1;
    HIPCHK(hipMemsetAsync(c->d_tally_rep, 0, nrep * sizeof(double), c->stream));
  }
  HIPCHK(hipMemsetAsync(c->d_counters, 0, CTR_COUNT * sizeof(unsigned long long), c->stream));
  if (reserve(c->own_T, c->L.total) || reserve(c->own_I, mcs_i64_total(p))) return 1;
  c->d_T = c->own_T; c->d_I = c->own_I;
  HIPCHK(hipMemsetAsync(c->d_T, 0, (size_t)c->L.total * sizeof(double), c->stream));
  HIPCHK(hipMemsetAsync(c->d_I, 0, (size_t)mcs_i64_total(p) * sizeof(unsigned long long), c->stream));
  HIPCHK(c->ev0.create());
  HIPCHK(c->ev1.create());
  HIPCHK(c->acc_ev.create_untimed());

  HIPCHK(hipStreamSynchronize(c->stream));
  *out = c.release();
  return 0;
}

int mcs_destroy(mcs_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete c;
  return 0;
}

int mcs_sync(mcs_ctx* c) {
  MCS_ENTER(c);
  if (fold_replicas(c)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int mcs_bind_tallies(mcs_ctx* c, double* dev_f64, int64_t n_f64, int64_t* dev_i64, int64_t n_i64) {
  MCS_ENTER(c);
  if (fold_replicas(c)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (dev_f64) {
    if (n_f64 < c->L.total) return fail("mcs_bind_tallies: f64 buffer smaller than layout.total");
    c->own_T.reset();
    c->d_T = dev_f64;
  }
  if (dev_i64) {
    if (n_i64 < mcs_i64_total(&c->P)) return fail("mcs_bind_tallies: i64 buffer too small");
    c->own_I.reset();
    c->d_I = (unsigned long long*)dev_i64;
  }
  return 0;
}
double* mcs_tallies_f64_devptr(mcs_ctx* c) { return c->d_T; }
int64_t* mcs_tallies_i64_devptr(mcs_ctx* c) { return (int64_t*)c->d_I; }

int mcs_set_grid(mcs_ctx* c, int n_entries, const double* x_grid_cm, const double* ux, const double* uz, const double* utot,
                 const double* gam_sf, const double* gam_ef, const double* beta_ef, const double* btot, const double* theta) {
  MCS_ENTER(c);
  const int ne = c->P.n_grid + 2;
  if (n_entries != ne) return fail("mcs_set_grid: n_entries != n_grid+2");
  for (int i = 0; i < ne; ++i) {
    if (!(btot[i] > 0) || !(utot[i] != 0)) return fail("mcs_set_grid: btot must be > 0 and utot != 0 in every zone");
    if (!std::isfinite(x_grid_cm[i])) return fail("mcs_set_grid: x_grid_cm must be finite (use +-1e30*rg0 sentinels)");
  }
  (void)beta_ef;  // passed by the reference (main_loops.jl:256) but never read by the path
  // The kernel detects "something happened at this move" by zone changes, so two facts of the
  // reference's grid are relied upon (setup_grid, src/initializers.jl:403-476): the shock x = 0 is a
  // zone boundary, and the upstream FEB lies inside zone i_grid_feb (MonteCarloScattering.jl:414).
  {
    bool has_zero = false;
    for (int i = 0; i < ne; ++i) {
      if (x_grid_cm[i] == 0.0) has_zero = true;
      if (i > 0 && !(x_grid_cm[i] > x_grid_cm[i - 1])) return fail("mcs_set_grid: x_grid_cm must be strictly increasing");
    }
    if (!has_zero) return fail("mcs_set_grid: x_grid_cm must contain the shock position 0.0 as a zone boundary");
    const int k = c->P.i_grid_feb;
    if (k < 0 || k + 1 >= ne || !(x_grid_cm[k + 1] > c->P.feb_upstream))
      return fail("mcs_set_grid: feb_upstream must lie below x_grid_cm[i_grid_feb+1]");
  }
  const double* src[8] = {x_grid_cm, ux, uz, utot, gam_sf, gam_ef, btot, theta};
  std::vector<double> h((size_t)8 * ne);
  for (int t = 0; t < 8; ++t) std::memcpy(&h[(size_t)t * ne], src[t], (size_t)ne * sizeof(double));
  HIPCHK(hipMemcpyAsync(c->d_tab, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->tb.x_grid = c->d_tab; c->tb.ux = c->d_tab + ne; c->tb.uz = c->d_tab + 2 * ne; c->tb.utot = c->d_tab + 3 * ne;
  c->tb.gsf = c->d_tab + 4 * ne; c->tb.gef = c->d_tab + 5 * ne; c->tb.btot = c->d_tab + 6 * ne; c->tb.theta = c->d_tab + 7 * ne;
  c->h_ux.assign(ux, ux + ne);
  c->all_parallel = true;
  for (int i = 0; i < ne; ++i) if (theta[i] != 0.0) c->all_parallel = false;
  c->have_grid = true;
  return 0;
}

int mcs_set_cuts(mcs_ctx* c, int n_pcuts, const double* pcuts, int n_tcuts, const double* tcuts, int n_xspec,
                 const double* x_spec, const double* inj_fracs, const double* eps_target) {
  MCS_ENTER(c);
  if (n_pcuts < 1 || n_pcuts > MCS_NA_C) return fail("momentum-cutoffs: parameter na_c smaller than desired number of pcuts.");
  if (n_tcuts + 1 > MCS_NA_C) return fail("TCUTS: parameter na_c smaller than desired number of tcuts.");
  if (n_tcuts > 255) return fail("mcs_set_cuts: n_tcuts > 255");
  if (n_xspec > c->P.n_grid) return fail("mcs_set_cuts: n_xspec > n_grid");
  const int ng = c->P.n_grid, ni = c->P.n_ions;
  std::vector<double> h;
  h.insert(h.end(), pcuts, pcuts + n_pcuts);
  h.insert(h.end(), tcuts, tcuts + n_tcuts);
  h.insert(h.end(), x_spec, x_spec + n_xspec);
  h.insert(h.end(), inj_fracs, inj_fracs + ni);
  h.insert(h.end(), eps_target, eps_target + ng);
  c->have_cuts = false;      // (the table pointers of c->tb lead into the block that is replaced)
  c->have_det = c->have_det_base = false;      // (K14's base and result belong to the detectors that are replaced)
  c->d_cuts.reset();
  if (reserve(c->d_cuts, (long long)h.size())) return 1;
  HIPCHK(hipMemcpyAsync(c->d_cuts, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  double* q = c->d_cuts;
  c->tb.pcuts = q; q += n_pcuts; c->tb.tcuts = q; q += n_tcuts; c->tb.x_spec = q; q += n_xspec;
  c->tb.inj_fracs = q; q += ni; c->tb.eps_target = q;
  c->tb.n_pcuts = n_pcuts; c->tb.n_tcuts = n_tcuts; c->tb.n_xspec = n_xspec;
  c->h_pcuts.assign(pcuts, pcuts + n_pcuts);
  c->h_inj_fracs.assign(inj_fracs, inj_fracs + ni);
  c->h_x_spec.assign(x_spec, x_spec + (n_xspec > 0 ? n_xspec : 0));
  c->have_cuts = true;
  return 0;
}

int mcs_begin_iteration(mcs_ctx* c, int i_iter) {
  MCS_ENTER(c);
  if (i_iter < 1 || i_iter > c->P.n_itrs) return fail("mcs_begin_iteration: i_iter out of 1..n_itrs");
  const mcs_params& P = c->P;
  c->i_iter = i_iter;
  if (fill(c, c->L.pxx_flux, P.n_grid, MCS_FLOOR) || fill(c, c->L.pxz_flux, P.n_grid, MCS_FLOOR) ||
      fill(c, c->L.energy_flux, P.n_grid, MCS_FLOOR) || fill(c, c->L.weight_coupled, (long long)MCS_NA_C * P.n_ions, MCS_FLOOR) ||
      fill(c, c->L.scalars, 4, MCS_FLOOR) || fill(c, c->L.energy_transfer_pool, P.n_grid, 0.0) ||
      fill(c, c->L.energy_recv_pool, P.n_grid, 0.0))
    return 1;
  return 0;
}

int mcs_begin_species(mcs_ctx* c, int i_iter, int i_ion, double aa, double zz, double pmax_cutoff, double density, double ewf) {
  MCS_ENTER(c);
  const mcs_params& P = c->P;
  if (i_ion < 1 || i_ion > P.n_ions) return fail("mcs_begin_species: i_ion out of 1..n_ions");
  if (i_iter < 1 || i_iter > P.n_itrs) return fail("mcs_begin_species: i_iter out of 1..n_itrs");
  if (!(aa > 0) || zz == 0) return fail("mcs_begin_species: aa must be > 0 and zz != 0");
  c->i_iter = i_iter; c->i_ion = i_ion; c->aa = aa; c->zzq = zz * MCS_QCGS; c->m = aa * MCS_MP; c->mc = c->m * MCS_C;
  c->pmax_cutoff = pmax_cutoff; c->density = density; c->ewf = ewf;
  c->have_cout_dndp = c->have_cout_thermo = false;
  c->have_esc = false;
  c->have_ang = false;
  c->have_tcut = false;
  c->have_prof = false;
  c->have_det = false;
  c->photon_flags_clear();
  if (fold_replicas(c)) return 1;      // (the previous species' replicas, before its histograms are cleared)
  if (P.do_tcuts) {      // K12's base: the species' block of spectra_coupled as it stands now
    const long long nb = (long long)MCS_NA_C * (MCS_PSD_MAX + 1);
    if (reserve(c->d_tcut_base, nb)) return 1;
    HIPCHK(hipMemcpyAsync(c->d_tcut_base, c->d_T + c->L.spectra_coupled + nb * (i_ion - 1), (size_t)nb * sizeof(double), hipMemcpyDeviceToDevice,
                          c->stream));
  }
  if (c->have_cuts && c->tb.n_xspec >= 1) {      // K14's base: rows 0..nd-1 of spectra_sf and of spectra_pf as they stand now, in one copy
    const long long pm1 = MCS_PSD_MAX + 1, nd = c->tb.n_xspec;
    c->have_det_base = false;
    if (reserve(c->d_det_base, 2 * nd * pm1)) return 1;
    HIPCHK(hipMemcpy2DAsync(c->d_det_base, (size_t)(nd * pm1) * sizeof(double), c->d_T + c->L.spectra_sf,
                            (size_t)(c->L.spectra_pf - c->L.spectra_sf) * sizeof(double), (size_t)(nd * pm1) * sizeof(double), 2,
                            hipMemcpyDeviceToDevice, c->stream));
    c->have_det_base = true;
  }
  c->species_begun = true;
  const long long npsd = c->L.psd_stride_zone * P.n_grid;
  const long long pm = MCS_PSD_MAX + 1;
  if (fill(c, c->L.psd, npsd, MCS_FLOOR) || fill(c, c->L.therm_sf, 2 * npsd, 0.0) ||
      fill(c, c->L.esc_psd_up, 2 * pm * pm, MCS_FLOOR) || fill(c, c->L.pxx_flux, 3LL * P.n_grid, 0.0))
    return 1;
  HIPCHK(hipMemsetAsync(c->d_I + MCS_I_NUM_CROSSINGS, 0, (size_t)P.n_grid * sizeof(unsigned long long), c->stream));
  HIPCHK(mcs_launch_copy(c->d_T + c->L.energy_recv_pool, c->d_T + c->L.energy_transfer_pool, P.n_grid, c->stream));
  return 0;
}

int mcs_set_fluxes(mcs_ctx* c, const double* pxx, const double* pxz, const double* en) {
  MCS_ENTER(c);
  const int ng = c->P.n_grid;
  HIPCHK(hipMemcpyAsync(c->d_T + c->L.pxx_flux, pxx, ng * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->d_T + c->L.pxz_flux, pxz, ng * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->d_T + c->L.energy_flux, en, ng * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int mcs_pop_upload(mcs_ctx* c, int64_t n, const mcs_soa* host) {
  MCS_ENTER(c);
  if (n < 0) return fail("mcs_pop_upload: n < 0");
  for (int64_t k = 0; k < n; ++k) {
    if (!(host->ptot_pf[k] > 0)) return fail("mcs_pop_upload: ptot_pf must be > 0 (zero-momentum particle: reference quirk G6)");
    if (host->grid[k] < 0 || host->grid[k] > c->P.n_grid) return fail("mcs_pop_upload: grid index out of 0..n_grid");
    if (host->tcut[k] < 1 || host->tcut[k] > 255) return fail("mcs_pop_upload: tcut out of range");
    // a non-finite position or momentum never satisfies an exit test (NaN compares false): the helix loop would run
    // into its cap and the retro walk into MCS_RETRO_CAP -- refuse it here (the reference would loop forever)
    if (!std::isfinite(host->ptot_pf[k]) || !std::isfinite(host->pb_pf[k]) || !std::isfinite(host->x_PT_cm[k]) ||
        !std::isfinite(host->prp_x_cm[k]) || !std::isfinite(host->acctime_sec[k]) || !std::isfinite(host->phi_rad[k]) ||
        !std::isfinite(host->weight[k]))
      return fail("mcs_pop_upload: weight, ptot_pf, pb_pf, x_PT_cm, prp_x_cm, acctime_sec and phi_rad must be finite");
    if (!(host->xn_per[k] > 0) || !std::isfinite(host->xn_per[k])) return fail("mcs_pop_upload: xn_per must be finite and > 0");
  }
  c->n = 0; c->n_run_last = -1; c->n_saved_last = 0; c->idx_gidx = nullptr;   // the saved arrays / src[] of the last run no longer describe this population
  if (ensure_capacity(c, n)) return 1;
  if (n > 0 && upload_soa(c, c->cur, n, host)) return 1;
  c->n = n;
  return 0;
}
int mcs_pop_download(mcs_ctx* c, int64_t n, mcs_soa* host) {
  MCS_ENTER(c);
  if (n > c->n) return fail("mcs_pop_download: n exceeds the population size");
  return download_soa(c, c->cur, n, host);
}
int mcs_saved_download(mcs_ctx* c, int64_t n, mcs_soa* host, uint8_t* l_save) {
  MCS_ENTER(c);
  if (n > c->n) return fail("mcs_saved_download: n exceeds the population size");
  if (host && download_soa(c, c->sav, n, host)) return 1;
  std::vector<uint8_t> own;
  if (!l_save && host) { own.resize((size_t)n); l_save = own.data(); }
  if (l_save) {
    HIPCHK(hipMemcpyAsync(l_save, c->d_lsave, (size_t)n, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream));
    for (int64_t k = 0; k < n; ++k) l_save[k] = l_save[k] == 1;      // (the device byte is a status: 1 saved, 2 ended)
  }
  if (host) {       // the *_saved arrays of the reference hold zeros where nothing was saved (main_loops.jl:184-197)
    for (int64_t k = 0; k < n; ++k) {
      if (l_save[k]) continue;
      for (auto f : kSoaF64) (host->*f)[k] = 0;
      host->grid[k] = 0; host->tcut[k] = 0; host->downstream[k] = 0; host->inj[k] = 0;
    }
  }
  return 0;
}
int64_t mcs_pop_size(mcs_ctx* c) { return c->n; }

int mcs_init_pop(mcs_ctx* c, int64_t n, int64_t j_offset, int64_t n_total, const double* ptot_pf_in, const double* weight_in,
                 double x_start_cm, int i_grid_start, int relativistic, int fast_push) {
  MCS_ENTER(c);
  if (!c->have_grid) return fail("mcs_init_pop: call mcs_set_grid first");
  if (n < 0 || i_grid_start < 0 || i_grid_start > c->P.n_grid) return fail("mcs_init_pop: bad arguments");
  if (!std::isfinite(x_start_cm)) return fail("mcs_init_pop: x_start_cm must be finite");
  for (int64_t k = 0; k < n; ++k)
    if (!(ptot_pf_in[k] > 0) || !std::isfinite(ptot_pf_in[k]) || !std::isfinite(weight_in[k]))
      return fail("mcs_init_pop: ptot_pf must be finite and > 0 (reference quirk G6), weight finite");
  c->n = 0; c->n_run_last = -1; c->n_saved_last = 0; c->idx_gidx = nullptr;   // the saved arrays / src[] of the last run no longer describe this population
  if (ensure_capacity(c, n)) return 1;
  if (reserve(c->d_stage, 2 * n + 2)) return 1;
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(c->d_stage, ptot_pf_in, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_stage + n, weight_in, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const unsigned long long key = (unsigned long long)((long long)(c->i_iter - 1) * c->P.n_ions + (c->i_ion - 1));
    HIPCHK(mcs_launch_init_pop(pop_view(c->cur), c->d_stage, c->d_stage + n, n, j_offset, 1, n_total, key, c->m, c->h_ux[i_grid_start],
                               x_start_cm, i_grid_start, relativistic, fast_push, c->P.xn_per_fine, c->P.x_grid_stop, 0, nullptr, nullptr, nullptr,
                               c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  c->n = n;
  return 0;
}

int mcs_init_pop_binned(mcs_ctx* c, int64_t n, int64_t j_offset, int64_t n_total, int n_bins, const double* bin_ptot_pf,
                        const double* bin_weight, const int64_t* bin_start, double x_start_cm, int i_grid_start,
                        int relativistic, int fast_push) {
  return mcs_init_pop_binned_strided(c, n, j_offset, 1, n_total, n_bins, bin_ptot_pf, bin_weight, bin_start, x_start_cm,
                                     i_grid_start, relativistic, fast_push);
}

int mcs_init_pop_binned_strided(mcs_ctx* c, int64_t n, int64_t j_offset, int64_t j_stride, int64_t n_total, int n_bins,
                                const double* bin_ptot_pf, const double* bin_weight, const int64_t* bin_start, double x_start_cm,
                                int i_grid_start, int relativistic, int fast_push) {
  MCS_ENTER(c);
  if (!c->have_grid) return fail("mcs_init_pop_binned: call mcs_set_grid first");
  if (n < 0 || n_bins < 1 || n_bins > 4096 || i_grid_start < 0 || i_grid_start > c->P.n_grid || !bin_ptot_pf || !bin_weight || !bin_start)
    return fail("mcs_init_pop_binned: bad arguments");
  if (bin_start[0] != 0 || bin_start[n_bins] != n_total || j_offset < 0 || j_stride < 1 ||
      (n > 0 && j_offset + (n - 1) * j_stride >= n_total))
    return fail("mcs_init_pop_binned: bin_start must run from 0 to n_total and the shard must lie inside");
  for (int b = 0; b < n_bins; ++b) {
    if (bin_start[b + 1] < bin_start[b]) return fail("mcs_init_pop_binned: bin_start must be non-decreasing");
    if (bin_start[b + 1] > bin_start[b] && (!(bin_ptot_pf[b] > 0) || !std::isfinite(bin_ptot_pf[b]) || !std::isfinite(bin_weight[b])))
      return fail("mcs_init_pop_binned: ptot_pf must be finite and > 0 (reference quirk G6), weight finite");
  }
  if (!std::isfinite(x_start_cm)) return fail("mcs_init_pop_binned: x_start_cm must be finite");
  c->n = 0; c->n_run_last = -1; c->n_saved_last = 0; c->idx_gidx = nullptr;   // the saved arrays / src[] of the last run no longer describe this population
  if (ensure_capacity(c, n)) return 1;
  const size_t nd = (size_t)3 * n_bins + 1;      // ptot | weight | start (int64 in a double slot)
  if (reserve(c->d_stage, (long long)nd + 2)) return 1;
  if (n > 0) {
    std::vector<double> h(nd);
    std::memcpy(h.data(), bin_ptot_pf, sizeof(double) * n_bins);
    std::memcpy(h.data() + n_bins, bin_weight, sizeof(double) * n_bins);
    std::memcpy(h.data() + 2 * n_bins, bin_start, sizeof(int64_t) * (n_bins + 1));
    HIPCHK(hipMemcpyAsync(c->d_stage, h.data(), nd * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const unsigned long long key = (unsigned long long)((long long)(c->i_iter - 1) * c->P.n_ions + (c->i_ion - 1));
    HIPCHK(mcs_launch_init_pop(pop_view(c->cur), nullptr, nullptr, n, j_offset, j_stride, n_total, key, c->m, c->h_ux[i_grid_start], x_start_cm,
                               i_grid_start, relativistic, fast_push, c->P.xn_per_fine, c->P.x_grid_stop, n_bins, c->d_stage,
                               c->d_stage + n_bins, (const long long*)(c->d_stage + 2 * n_bins), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));     // h goes out of scope
  }
  c->n = n;
  return 0;
}

int mcs_num_cus(mcs_ctx* c) { return c->n_cu; }

int mcs_set_launch(mcs_ctx* c, int blocks, int threads) {
  MCS_ENTER(c);
  if (threads != 0 && (threads % 64 != 0 || threads > 256)) return fail("mcs_set_launch: threads must be a multiple of 64, <= 256");
  c->blocks = blocks; c->threads = threads ? threads : 256;
  return 0;
}

int mcs_set_debug_finals(mcs_ctx* c, int on) { MCS_ENTER(c); c->debug_finals = on != 0; return 0; }
// Host words only: the launches that are queued have their constants already, the next ones read these.
int mcs_set_option(mcs_ctx* c, int key, int64_t value) {
  MCS_ENTER(c);
  std::string why;
  if (mcs_option_check_set(key, value, c->P.state_fp32, c->pp_masks_tried, &why) != MCS_OPTION_OK) return fail("mcs_set_option: " + why);
  c->opt[key] = value;
  return 0;
}
int mcs_get_option(mcs_ctx* c, int key, int64_t* value) {
  MCS_ENTER(c);
  if (!value) return fail("mcs_get_option: null argument");
  if (!mcs_option_row(key)) return fail(format("mcs_get_option: unknown option key %d (the keys are 0..%d, enum mcs_option)", key, MCS_OPT_COUNT - 1));
  *value = c->opt[key];
  return 0;
}
int mcs_set_tail_slicing(mcs_ctx* c, int budget_trips) {
  MCS_ENTER(c);
  switch (mcs_option_check_set(MCS_OPT_TAIL_BUDGET, budget_trips, c->P.state_fp32, c->pp_masks_tried, nullptr)) {
    case MCS_OPTION_OK: break;
    case MCS_OPTION_APPLIES: return fail("mcs_set_tail_slicing: the fp32-state kernels are not sliced (fp64 contexts only)");
    default: return fail("mcs_set_tail_slicing: budget out of range");
  }
  c->opt[MCS_OPT_TAIL_BUDGET] = budget_trips;
  return 0;
}
int mcs_last_launches(mcs_ctx* c) { return c->tail_rounds_last; }
int mcs_last_kernel(mcs_ctx* c) { return c->kernel_last; }
int mcs_set_retro_cap(mcs_ctx* c, int64_t cap) {
  MCS_ENTER(c);
  if (cap < 0 || cap > 2000000000LL) return fail("mcs_set_retro_cap: cap out of range");
  c->retro_cap = cap > 0 ? (int)cap : MCS_RETRO_CAP;
  return 0;
}

// ---- K1 launches: which kernel, its geometry, the launch constants

// The K1 kernel the context's current species runs, its block size and the workgroups of it a CU holds (2 for the fp64 kernels --
// 78 KB of LDS each --, 1 for the wave-specialised ones, 3 for the fp32-state kernels -- the organised one: 168 VGPRs, 51 KB).
// n: the population that decides the wave-specialised form (MCS_OPT_K1_WS, MCS_OPT_WS_AUTO_MIN).  sliced: a launch that suspends and resumes
// particles -- the tail slicing of mcs_run_pcut* (mcs_set_tail_slicing) runs the general kernel's sliced form for every species, the
// pipelined loop (which refuses tail slicing) the sliced form of the species' own kernel.  explicit_geometry: the launch has the
// geometry of mcs_set_launch (never the wave-specialised form).
struct K1Plan { int kernel, threads, per_cu; };
static bool is_ws(int kernel) { return kernel == K1_WS || kernel == K1_WS_ETF; }
static K1Plan k1_plan(const mcs_ctx* c, long long n, bool sliced, bool explicit_geometry) {
  const mcs_params& P = c->P;
  // the specialised kernel for the common configuration (see transport_body<PLAIN> in mcs_transport.hip)
  const bool plain_but_etf = !c->o(MCS_OPT_FORCE_GENERAL) && c->all_parallel && !P.dont_scatter && !P.use_custom_epsB && !P.dont_DSA &&
                             !(P.feb_downstream > 0) && c->aa >= 1 && c->tb.n_xspec == 0 && !(c->h_inj_fracs[c->i_ion - 1] < 1);
  const bool plain = plain_but_etf && !(P.energy_transfer_frac > 0);
  const bool plain_etf = plain_but_etf && !plain;      // the ions of a run with energy transfer: PLAIN with that one flag at run time
  // the specialised kernel for electrons with radiative losses (transport_body<false, LOSSY>): the loss in line in the common pass
  const bool lossy = !c->o(MCS_OPT_FORCE_GENERAL) && P.do_rad_losses && c->aa < 1 && !P.use_custom_epsB && !P.dont_scatter;
  if (P.state_fp32) return {c->o(MCS_OPT_F32_EXACT) ? K1_F32_LOOP_EXACT : (c->o(MCS_OPT_F32_LOOP) ? K1_F32_LOOP : (lossy ? K1_F32_LOSSY : K1_F32)), 256, 3};
  if (sliced && c->o(MCS_OPT_TAIL_BUDGET) > 0) return {K1_SLICED, 256, 2};
  if (sliced) return {plain ? K1_PLAIN_SLICED : (lossy ? K1_LOSSY_SLICED : (plain_etf ? K1_PLAIN_ETF_SLICED : K1_SLICED)), 256, 2};
  // the wave-specialised form of PLAIN / PLAIN_ETF (mcs_transport_ws.inc), not with an explicit launch geometry
  if ((plain || plain_etf) && !explicit_geometry && (c->o(MCS_OPT_K1_WS) == 1 || (c->o(MCS_OPT_K1_WS) == 2 && n >= c->o(MCS_OPT_WS_AUTO_MIN))))
    return {plain ? K1_WS : K1_WS_ETF, mcs_transport_ws_threads(), 1};
  return {plain ? K1_PLAIN : (lossy ? K1_LOSSY : (plain_etf ? K1_PLAIN_ETF : K1_GENERAL)), 256, 2};
}

// The workgroups of the current species' K1 kernel that one CU holds when the launch geometry is explicit (mcs_set_launch: never
// the wave-specialised form).  0, with a message, before mcs_set_cuts.
int mcs_k1_blocks_per_cu(mcs_ctx* c) {
  if (!c || !c->have_cuts) { (void)fail("mcs_k1_blocks_per_cu: cuts not set"); return 0; }
  return k1_plan(c, c->n, false, true).per_cu;
}

// persistent lanes: fill the chip (`full` workgroups), never launch more lanes than particles, at least one workgroup
static int persistent_grid(long long n, int threads, long long full) {
  return (int)std::max(1LL, std::min((n + threads - 1) / threads, full));
}

// live particles a wave holds at most (KArgs::claim_max) and the two flags that go with it: a sparse wave (fewer than 64) neither
// defers its rare work nor waits for company nor consolidates
static void set_claim(const mcs_ctx* c, KArgs& a, int claim_max) {
  const bool dense = claim_max >= 64;
  a.claim_max = claim_max;
  // a wave whose live lanes all wait for company (fewer than defer_k of them) must be able to refill: with
  // defer_k + refill_min <= 64 either defer_k lanes are live or refill_min are idle (see the deferral in transport_body)
  a.defer_k = dense ? (int)std::min(c->o(MCS_OPT_DEFER_K), 64 - c->o(MCS_OPT_REFILL_MIN)) : 1;
  a.wait_full = dense && c->o(MCS_OPT_PARK);
  a.tail_merge = dense && c->o(MCS_OPT_TAIL_MERGE);
}

// A launch of n_x resumed particles spread over `waves` waves: a pass costs a wave the same with 1 live lane as with 64, but the rare
// work of every live lane stalls all the others, so the fewer particles share a wave the faster each history advances -- and the
// launch waits for its longest one.  Measured (profiles/r03_tau_vs_lanes.txt: 2048 particles, kernel time of 14 pcuts): 64 particles
// per wave 45.6 ms, 32: 38.1, 16: 35.6, 8: 33.4, 4: 31.6, 2 (one wave per SIMD): 31.7, 1 (two waves per SIMD): 37.9 -- so as few
// particles per wave as `waves` allow, and a dense launch when that would be more than 16.  Sets the claim of `a`; returns the
// workgroups, at most `full`.
static int sparse_claim(const mcs_ctx* c, KArgs& a, long long n_x, long long waves, int threads, long long full) {
  long long cm = (n_x + waves - 1) / waves;
  if (cm > 16) cm = 64;
  set_claim(c, a, (int)cm);
  const long long per_block = (long long)(threads / 64) * cm;
  return (int)std::min((n_x + per_block - 1) / per_block, full);
}

// two export buffers of need_cap lane states each (sliced launches)
static int ensure_strag(mcs_ctx* c, long long need_cap) {
  if (need_cap <= c->strag.cap()) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));      // (queued launches may still export into the blocks that are freed)
  return reserve(c->strag, need_cap);
}

// the launch constants of one pcut that do not depend on the kernel chosen (shared by mcs_run_pcut* and mcs_run_pcuts_fused)
static void fill_kargs(mcs_ctx* c, KArgs& a, int i_pcut, long long n, long long i_prt_offset, long long i_prt_stride, const long long* dev_gidx, int budget) {
  std::memset(&a, 0, sizeof(a));
  a.P = c->P; a.L = c->L; a.tb = c->tb; a.in = pop_view(c->cur); a.sv = pop_view(c->sav); a.l_save = c->d_lsave;
  a.T = c->d_T; a.I = c->d_I;
  a.aa = c->aa; a.zzq = c->zzq; a.m = c->m; a.mc = c->mc; a.pmax_cutoff = c->pmax_cutoff; a.density = c->density; a.ewf = c->ewf;
  a.inj_frac = c->h_inj_fracs[c->i_ion - 1];
  a.pcut = c->h_pcuts[i_pcut - 1];
  a.pcut_prev = i_pcut > 1 ? c->h_pcuts[i_pcut - 2] : 0.0;
  a.i_iter = c->i_iter; a.i_ion = c->i_ion; a.i_pcut = i_pcut;
  a.n = n; a.i_prt_offset = i_prt_offset; a.i_prt_stride = i_prt_stride; a.gidx = dev_gidx;
  a.retro_cap = c->retro_cap;
  a.refill_min = (int)c->o(MCS_OPT_REFILL_MIN);
  set_claim(c, a, 64);
  a.tail_ring = c->o(MCS_OPT_TAIL_RING) ? 1 : 0;
  a.tail_loop = c->o(MCS_OPT_TAIL_RING) ? (int)c->o(MCS_OPT_TAIL_LOOP) : 0;
  // iseed_mod - i_prt, src/particle_loop.jl:35-40
  a.seed_base = (unsigned long long)((long long)(c->i_iter - 1) * c->P.n_pts_max * c->tb.n_pcuts * c->P.n_ions +
                                     (long long)(c->i_ion - 1) * c->P.n_pts_max * c->tb.n_pcuts +
                                     (long long)(i_pcut - 1) * c->P.n_pts_max);
  set_counters(a, c->d_counters, CTR_WORK, CTR_SAVED, CTR_EXPORT);
  a.tally_rep = c->d_tally_rep; a.rep_n = c->d_tally_rep ? c->rep_n : 0;
  if (c->debug_finals) { a.f_reason = c->fin.reason; a.f_helix = c->fin.helix; a.f_retro = c->fin.retro; a.f_ptot = c->fin.ptot; a.f_x = c->fin.x; }
  a.budget_trips = budget;
  a.strag_out = c->strag.d[0];
  a.ws_pop_max = mcs_transport_ws_threads() + 160;      // (read by the wave-specialised kernels only)
  a.ws_serve_min = 64;
}

static int run_pcut_impl(mcs_ctx* c, int i_pcut, int64_t i_prt_offset, int64_t i_prt_stride, const int64_t* dev_gidx, int64_t* n_saved) {
  MCS_ENTER_AS(c, "mcs_run_pcut");
  if (i_prt_offset < 0 || i_prt_stride < 1) return fail("mcs_run_pcut: i_prt_first must be >= 0 and i_prt_stride >= 1");
  if (!c->have_grid || !c->have_cuts) return fail("mcs_run_pcut: grid/cuts not set");
  if (i_pcut < 1 || i_pcut > c->tb.n_pcuts) return fail("mcs_run_pcut: i_pcut out of range");
  const long long n = c->n;
  if (ensure_capacity(c, n)) return 1;
  // main_loops.jl:184-197: l_save and the *_saved arrays start at zero.  On the device only l_save is cleared: K2 and the
  // exports read saved entries through the compacted index list, and mcs_saved_download zeroes the entries of unsaved
  // particles in the host copy it hands out (nine fills per pcut less in the timed path).
  if (n > 0) HIPCHK(hipMemsetAsync(c->d_lsave, 0, (size_t)n, c->stream));
  HIPCHK(hipMemsetAsync(c->d_counters, 0, (CTR_EXPORT + 1) * sizeof(unsigned long long), c->stream));
  const int budget = (c->P.state_fp32 || n == 0) ? 0 : (int)c->o(MCS_OPT_TAIL_BUDGET);      // (the fp32 study kernel is not sliced)
  if (budget > 0) {
    // one entry per lane a launch can hold: 2 workgroups of 256 threads per CU, or the geometry of mcs_set_launch if that is larger
    long long need_cap = (long long)2 * c->n_cu * 256;
    if (c->blocks > 0 && (long long)c->blocks * c->threads > need_cap) need_cap = (long long)c->blocks * c->threads;
    if (ensure_strag(c, need_cap)) return 1;
  }

  KArgs& a = *c->h_args_pin;     // (every launch below is followed by a stream synchronisation before this is written again)
  fill_kargs(c, a, i_pcut, n, i_prt_offset, i_prt_stride, (const long long*)dev_gidx, budget);

  const K1Plan k1 = k1_plan(c, n, budget > 0, c->blocks > 0);
  const bool ws = is_ws(k1.kernel);
  // the geometry of mcs_set_launch, else the persistent grid (mcs_set_launch's block size sizes the grid of the fp32-state kernels
  // too, which always run k1.threads)
  const int threads = ws ? k1.threads : c->threads;
  const int launch_threads = c->P.state_fp32 ? k1.threads : threads;
  const long long full = (long long)c->n_cu * k1.per_cu;
  int blocks = c->blocks > 0 ? c->blocks : persistent_grid(n, threads, full);
  if (budget > 0 && (long long)blocks * threads > c->strag.cap()) return fail("mcs_run_pcut: launch geometry exceeds the export buffer of a sliced run");
  double ms_total = 0.0;
  c->tail_rounds_last = 0;
  c->kernel_last = k1.kernel;
  for (int round = 0;; ++round) {
    HIPCHK(hipMemcpyAsync(c->d_args, c->h_args_pin, sizeof(KArgs), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    if (n > 0) {
      HIPCHK(mcs_launch_transport(c->d_args, k1.kernel, blocks, launch_threads, c->stream));
      c->rep_dirty = true;
    }
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    ++c->tail_rounds_last;
    if (budget == 0) break;
    // sliced run: how many particles did the launch export?  They are the next launch's queue, spread over the chip's waves
    HIPCHK(hipMemcpyAsync(c->h_back + CTR_EXPORT, c->d_counters + CTR_EXPORT, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const unsigned long long n_x = c->h_back[CTR_EXPORT];
    float ms_r = 0.f;
    HIPCHK(hipEventElapsedTime(&ms_r, c->ev0, c->ev1));
    ms_total += ms_r;
    if (n_x == 0) break;
    if ((long long)n_x > c->strag.cap()) return fail("mcs_run_pcut: export buffer overrun");
    HIPCHK(hipMemsetAsync(c->d_counters + CTR_WORK, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(c->d_counters + CTR_EXPORT, 0, sizeof(unsigned long long), c->stream));
    a.strag_in = c->strag.d[round & 1]; a.strag_out = c->strag.d[(round + 1) & 1];
    a.n_resume = (long long)n_x; a.fresh_lo = n;
    blocks = sparse_claim(c, a, (long long)n_x, (long long)c->n_cu * (threads / 64), threads, full);     // one wave per SIMD
    // few particles per wave already: nothing left to gain from another slice
    a.budget_trips = a.claim_max <= 4 ? 0 : budget;
  }
  // the compaction half of new_pcut, queued behind the kernel: src[] for mcs_new_pcut / mcs_saved_export and an
  // independent count of the l_save flags next to the kernel's own n_saved counter, read back together
  HIPCHK(mcs_launch_compact(c->d_lsave, n, c->scan.bcounts, c->scan.boffs, c->d_counters + CTR_SCAN, c->scan.src, c->stream));
  HIPCHK(hipMemcpyAsync(c->h_back + CTR_SAVED, c->d_counters + CTR_SAVED, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));      // SAVED, SCAN, EXPORT
  HIPCHK(hipStreamSynchronize(c->stream));
  const unsigned long long ns[2] = {c->h_back[CTR_SAVED], c->h_back[CTR_SCAN]};
  if (ws && c->h_back[CTR_EXPORT] != 0) {
    return fail(format("mcs_run_pcut: a bounded wait of the wave-specialised kernel ran out (the launch is incomplete; code 0x%llx)", (unsigned long long)c->h_back[CTR_EXPORT]));
  }
  if (budget == 0) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    ms_total = ms;
  }
  c->last_ms = ms_total;
  c->n_saved_last = (long long)ns[0];
  c->n_run_last = n; c->idx_first = i_prt_offset; c->idx_stride = i_prt_stride; c->idx_gidx = (const long long*)dev_gidx;
  // every entry point that hands out l_save or the saved arrays goes through here (a spilling build of the kernel
  // once miscompiled the l_save byte store, see csrc/Makefile)
  if (ns[0] != ns[1]) return fail("mcs_run_pcut: the kernel's n_saved counter and the count of l_save flags differ");
  if (n_saved) *n_saved = (int64_t)ns[0];
  return 0;
}
int mcs_run_pcut_strided(mcs_ctx* c, int i_pcut, int64_t i_prt_offset, int64_t i_prt_stride, int64_t* n_saved) {
  return run_pcut_impl(c, i_pcut, i_prt_offset, i_prt_stride, nullptr, n_saved);
}
int mcs_run_pcut(mcs_ctx* c, int i_pcut, int64_t i_prt_offset, int64_t* n_saved) { return run_pcut_impl(c, i_pcut, i_prt_offset, 1, nullptr, n_saved); }
int mcs_run_pcut_indexed(mcs_ctx* c, int i_pcut, const int64_t* dev_gidx, int64_t* n_saved) {
  MCS_ENTER(c);
  if (!dev_gidx && c->n > 0) return fail("mcs_run_pcut_indexed: null index list");
  return run_pcut_impl(c, i_pcut, 0, 1, dev_gidx, n_saved);
}

// the per-pcut outputs of a species loop: host arrays with one entry per pcut (strag: two); kernel_ms and strag may be null
struct PcutOut { int64_t *n_use, *n_saved, *i_mult; double* kernel_ms; int64_t* strag; };

// What mcs_run_pcuts_fused and mcs_run_pcuts_pipelined (`who`) do before they diverge: the arguments they share are checked, and the
// population, saved and spare buffers hold *cap_n particles -- every population of the species fits:
// n_new = n_saved * (n_target / n_saved) <= max(n_target, n_saved)
static int species_loop_open(mcs_ctx* c, const char* who, int i_pcut_first, int i_pcut_last, const int64_t* n_target, const PcutOut& o, long long* cap_n) {
  const std::string w = std::string(who) + ": ";
  if (!c->have_grid || !c->have_cuts) return fail(w + "grid/cuts not set");
  if (i_pcut_first < 1 || i_pcut_last > c->tb.n_pcuts || i_pcut_last < i_pcut_first) return fail(w + "pcut range");
  if (!n_target || !o.n_use || !o.n_saved || !o.i_mult) return fail(w + "null argument");
  if (c->o(MCS_OPT_TAIL_BUDGET) > 0 || c->blocks > 0) return fail(w + "not with sliced launches or an explicit launch geometry");
  *cap_n = c->n;
  for (int k = 0; k <= i_pcut_last - i_pcut_first; ++k) { if (n_target[k] < 1) return fail(w + "n_target < 1"); if (n_target[k] > *cap_n) *cap_n = n_target[k]; }
  return ensure_capacity(c, *cap_n) || reserve(c->spare, grow_cap(*cap_n));
}

// ---- A species' pcuts queued back to back (the device side of it): transport, pcut_finalize and new_pcut of every
// pcut first .. last with NOTHING read back in between -- n_saved, i_mult = max(n_target / n_saved, 1) (src/cuts.jl:42) and the
// size of the next population are decided on the device (mcs_k_pcut_decide) and the next launch reads its population size there.
// One shard with global indices 0, 1, 2, ... (a single rank); not for sliced launches or an explicit launch geometry.
// n_target[k]: the target population after pcut first + k.  Outputs (host, length last - first + 1): what mcs_run_pcut / mcs_new_pcut
// would have returned per pcut, and each transport launch's kernel time.  Pcuts after the one that saved nobody run empty.
int mcs_run_pcuts_fused(mcs_ctx* c, int i_pcut_first, int i_pcut_last, const int64_t* n_target, int64_t* n_use_out, int64_t* n_saved_out,
                        int64_t* i_mult_out, double* kernel_ms_out) {
  MCS_ENTER(c);
  const PcutOut o{n_use_out, n_saved_out, i_mult_out, kernel_ms_out, nullptr};
  const int npc = i_pcut_last - i_pcut_first + 1;
  long long cap_n = 0;
  if (species_loop_open(c, "mcs_run_pcuts_fused", i_pcut_first, i_pcut_last, n_target, o, &cap_n)) return 1;
  if (npc > c->fused.cap()) {
    HIPCHK(hipStreamSynchronize(c->stream));      // (queued launches may still read the constants that are freed)
    if (reserve(c->fused, npc)) return 1;
  }
  while ((int)c->f_ev.size() < 2 * npc) { Event e; HIPCHK(e.create()); c->f_ev.push_back(std::move(e)); }
  // launch constants of every pcut: the buffers rotate (cur -> saved -> spare -> cur) independently of the sizes: pcut k reads
  // pop[k & 1] and its split writes the other one; c->cur and c->spare themselves are swapped once the species is through
  const DevPop pop[2] = {pop_view(c->cur), pop_view(c->spare)}, sav = pop_view(c->sav);
  for (int k = 0; k < npc; ++k) {
    KArgs& a = c->fused.h_args[k];
    fill_kargs(c, a, i_pcut_first + k, 0, 0, 1, nullptr, 0);
    a.in = pop[k & 1]; a.sv = sav;
    a.n_dev = &c->fused.d_pd[k].n_use;
  }
  const K1Plan k1 = k1_plan(c, cap_n, false, false);
  const int blocks = persistent_grid(cap_n, k1.threads, (long long)c->n_cu * k1.per_cu);
  std::memset(c->fused.h_pd, 0, sizeof(PcutDev) * (size_t)(npc + 1));
  c->fused.h_pd[0].n_use = c->n;
  HIPCHK(hipMemcpyAsync(c->fused.d_args, c->fused.h_args, sizeof(KArgs) * (size_t)npc, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->fused.d_pd, c->fused.h_pd, sizeof(PcutDev) * (size_t)(npc + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(c->d_counters, 0, CTR_COUNT * sizeof(unsigned long long), c->stream));
  const int n_split_blocks = split_blocks(c, cap_n, 16);      // (cap_n >= 1)
  for (int k = 0; k < npc; ++k) {
    HIPCHK(hipMemsetAsync(c->d_lsave, 0, (size_t)cap_n, c->stream));
    HIPCHK(hipEventRecord(c->f_ev[2 * k], c->stream));
    HIPCHK(mcs_launch_transport(c->fused.d_args + k, k1.kernel, blocks, k1.threads, c->stream));
    HIPCHK(hipEventRecord(c->f_ev[2 * k + 1], c->stream));
    HIPCHK(mcs_launch_finalize_split_dev(c->d_lsave, cap_n, c->scan.bcounts, c->scan.boffs, c->d_counters + CTR_SCAN, c->scan.src, c->fused.d_pd + k, c->fused.d_pd + k + 1,
                                         c->d_counters, (long long)n_target[k], c->d_counters + CTR_MISMATCH, sav, pop[(k + 1) & 1], n_split_blocks, c->stream));
  }
  c->rep_dirty = true;
  HIPCHK(hipMemcpyAsync(c->fused.h_pd, c->fused.d_pd, sizeof(PcutDev) * (size_t)(npc + 1), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(c->h_back + CTR_EXPORT, c->d_counters + CTR_EXPORT, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));      // EXPORT, MISMATCH
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->h_back[CTR_MISMATCH] != 0) return fail("mcs_run_pcuts_fused: the kernel's n_saved counter and the count of l_save flags differ");
  if (is_ws(k1.kernel) && c->h_back[CTR_EXPORT] != 0) return fail("mcs_run_pcuts_fused: a bounded wait of the wave-specialised kernel ran out (a launch is incomplete)");
  double ms_sum = 0.0;
  for (int k = 0; k < npc; ++k) {
    o.n_use[k] = c->fused.h_pd[k].n_use; o.n_saved[k] = c->fused.h_pd[k].n_saved; o.i_mult[k] = c->fused.h_pd[k].i_mult;
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->f_ev[2 * k], c->f_ev[2 * k + 1]));
    if (o.kernel_ms) o.kernel_ms[k] = ms;
    ms_sum += ms;
  }
  // what the mcs_run_pcut / mcs_new_pcut sequence leaves: it ends with the first pcut that saved nobody, whose population stays as it
  // ran (the pcuts after it ran empty and wrote nothing); if every pcut saved somebody, the children of the last split
  int n_split = 0; while (n_split < npc && c->fused.h_pd[n_split].n_saved > 0) ++n_split;
  if (n_split & 1) std::swap(c->cur, c->spare);
  c->n = c->fused.h_pd[n_split].n_use;
  c->n_run_last = -1; c->n_saved_last = 0;
  c->last_ms = ms_sum; c->tail_rounds_last = npc;
  c->kernel_last = k1.kernel;
  return 0;
}

// The pcut loop of mcs_run_pcuts_pipelined: on failure it returns at once, its caller drains the streams.  It keeps the context's own
// words as it goes: c->cur / c->spare are the population of the current pcut and the target of its split (swapped per pcut), c->n the
// size of the last population it has put into the outputs, c->last_ms the kernel time of the main launches.
static int pipelined_pcuts(mcs_ctx* c, const K1Plan& k1, int i_pcut_first, int npc, long long cap_n, const int64_t* n_target,
                           int64_t long_draws, int64_t long_imult_max, const PcutOut& o) {
  unsigned long long* const pc = c->pp_dpc;      // (the words of enum PipeCtr)
  const bool masked = c->pp_s1m && c->pp_s2m;      // the two streams with complementary CU masks exist (MCS_PIPE_SIDE_CUS)
  hipStream_t s1 = c->stream;                      // the main stream of the CURRENT pcut: the masked one when the pcut has side work
  hipStream_t const s2 = masked ? c->pp_s2m : c->pp_s2;
  hipStream_t const s_alone = masked ? c->stream : c->pp_s2;   // long histories the pcut waits for: the whole chip
  const int side_max = 64;     // workgroups (of 2 per CU) the main launch leaves free for the side stream at most
  const int threads = k1.threads;
  const long long full = (long long)c->n_cu * k1.per_cu;
  const DevPop savb[2] = {pop_view(c->sav), pop_view(c->pp_sav2)};
  uint8_t* lsv[2] = {c->d_lsave, c->pp_lsave2};
  long long nA = c->n, nL = 0;
  // long histories are told apart in pcut k only when the pcut before it split by at most long_imult_max (<= 0: always): where few
  // particles are saved and each is split a hundredfold, i_mult hangs on the last long history and the pcut would wait for them anyway
  // (a rule on numbers the oracle has too: driver.py applies it to set_long_draws)
  long long Bk = long_draws;
  bool side_pending = false;
  int side_blocks = 0;               // workgroups the side stream's launches of this pcut need resident beside the main launch
  long long n1_prev = 0, sofar_prev = 0;
  c->pp_waits_last = 0;
  c->tail_rounds_last = 0;
  c->last_ms = 0.0;
  const bool dbg_pipe = std::getenv("MCS_PIPE_DEBUG") != nullptr;
  for (int k = 0; k < npc; ++k) { o.n_use[k] = 0; o.n_saved[k] = 0; o.i_mult[k] = 1; if (o.kernel_ms) o.kernel_ms[k] = 0.0; if (o.strag) { o.strag[2 * k] = 0; o.strag[2 * k + 1] = 0; } }
  HIPCHK(hipMemsetAsync(pc, 0, PC_COUNT * sizeof(unsigned long long), s1));
  if (nA > 0) HIPCHK(hipMemsetAsync(lsv[0], 0, (size_t)nA, s1));
  // the launch of the exported particles of pcut `i_pcut` (parity q), to their end, on `st`
  auto launch_resume = [&](int i_pcut, int q, long long n_pop, long long n_x, hipStream_t st, bool alone) -> int {
    KArgs& a = c->pp_hargs[1];
    fill_kargs(c, a, i_pcut, n_pop, 0, 1, nullptr, 0);
    a.in = pop_view(c->cur); a.sv = savb[q]; a.l_save = lsv[q];
    set_counters(a, pc, PC_RES_WORK, PC_RES_SAVED, PC_EXPORT + (q ^ 1)); a.strag_out = c->strag.d[q ^ 1];
    a.strag_in = c->strag.d[q]; a.n_resume = n_x; a.fresh_lo = n_pop; a.long_draws = (unsigned int)Bk; a.budget_trips = 0;
    // few particles per wave (sparse_claim), on at most one wave per SIMD of the chip (alone on the chip -- the pcut waits for them --
    // one wave per SIMD; beside a main launch every wave they hold is taken from it: 16 particles per wave cost 12 % on the longest
    // history and 1 / 16 of the slots)
    const int blocks = sparse_claim(c, a, n_x, alone ? (long long)c->n_cu * (threads / 64) : (n_x + 15) / 16, threads, full);
    HIPCHK(hipMemcpyAsync(c->pp_dargs + 1, &a, sizeof(KArgs), hipMemcpyHostToDevice, st));
    HIPCHK(mcs_launch_transport(c->pp_dargs + 1, k1.kernel, blocks, threads, st));
    if (!alone) side_blocks += blocks;
    ++c->tail_rounds_last;
    return 0;
  };
  for (int k = 0; k < npc; ++k) {
    const int i_pcut = i_pcut_first + k, q = k & 1;
    // ---- the main launch: particles 0 .. nA-1 of the population
    if (nA > 0) {
      KArgs& a = c->pp_hargs[0];
      fill_kargs(c, a, i_pcut, nA, 0, 1, nullptr, Bk > 0 ? 1 : 0);
      a.in = pop_view(c->cur); a.sv = savb[q]; a.l_save = lsv[q];
      set_counters(a, pc, PC_WORK, PC_SAVED, PC_EXPORT + q); a.strag_out = c->strag.d[q];
      a.long_draws = (unsigned int)Bk;
      HIPCHK(hipMemcpyAsync(c->pp_dargs, &a, sizeof(KArgs), hipMemcpyHostToDevice, s1));
      HIPCHK(hipEventRecord(c->ev0, s1));
      // (the main launch is persistent and fills every slot of the chip: it leaves room for the side stream's workgroups, which would
      // otherwise wait for its workgroups to leave -- and run after it instead of beside it)
      int blocks_a = persistent_grid(nA, threads, full);
      if (masked) { if (s1 == c->pp_s1m && blocks_a > 2 * (c->n_cu - (int)c->o(MCS_OPT_PIPE_SIDE_CUS))) blocks_a = 2 * (c->n_cu - (int)c->o(MCS_OPT_PIPE_SIDE_CUS)); }
      else if (side_blocks > 0 && blocks_a > full - side_blocks) blocks_a = (int)(full - side_blocks);
      HIPCHK(mcs_launch_transport(c->pp_dargs, k1.kernel, blocks_a, threads, s1));
      HIPCHK(hipEventRecord(c->ev1, s1));
      ++c->tail_rounds_last;
    }
    c->rep_dirty = true;
    // ---- join: the side stream (the previous pcut's long histories, its late split, this pcut's late launch), then the main launch,
    // the compaction of the particles that were saved and are not long, one read-back
    const auto tj0 = std::chrono::steady_clock::now();
    if (side_pending) HIPCHK(hipStreamSynchronize(s2));
    const auto tj1 = std::chrono::steady_clock::now();
    if (side_pending) HIPCHK(hipMemcpyAsync(c->pp_hpdl + q, c->pp_dpdl + q, sizeof(PcutDev), hipMemcpyDeviceToHost, s1));
    // (the late group's size is on the device until here: the compaction below covers every index it can have)
    const long long n_hi = nA + nL;       // nL: the host's upper bound while side_pending
    HIPCHK(mcs_launch_compact_match(lsv[q], n_hi, c->scan.bcounts, c->scan.boffs, pc + PC_SCAN, c->scan.src, 1u, s1));
    HIPCHK(hipMemcpyAsync(c->pp_hpc, pc, PC_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, s1));
    HIPCHK(hipStreamSynchronize(s1));
    const auto tj2 = std::chrono::steady_clock::now();
    float ms_main = 0.f;
    if (nA > 0) { HIPCHK(hipEventElapsedTime(&ms_main, c->ev0, c->ev1)); if (o.kernel_ms) o.kernel_ms[k] = ms_main; c->last_ms += ms_main; }
    const unsigned long long* h = c->pp_hpc;
    double dbg_wait_ms = 0.0;
    if (side_pending) {
      // the previous pcut is complete now: its saved long particles, the size of this pcut's late group
      const long long n5_prev = c->pp_hpdl[q].n_saved;
      nL = c->pp_hpdl[q].n_new;
      o.n_saved[k - 1] = n1_prev + n5_prev;
      if (sofar_prev + (long long)h[PC_RES_SAVED] != o.n_saved[k - 1]) {
        return fail(format("mcs_run_pcuts_pipelined: pcut %d: the kernels' n_saved counters (%lld + %llu resumed) and the count of status bytes (%lld + %lld long) differ",
                           i_pcut - 1, sofar_prev, (unsigned long long)h[PC_RES_SAVED], n1_prev, n5_prev));
      }
    }
    side_pending = false;
    c->n = o.n_use[k] = nA + nL;
    const long long n1 = (long long)h[PC_SCAN], n_T = (long long)h[PC_EXPORT + q];
    long long sofar = (long long)h[PC_SAVED] + (long long)h[PC_LATE_SAVED];        // saved by the main and the late launch: not long, or long and already ended
    if (o.strag) o.strag[2 * k] = n_T;
    if (n_T > c->strag.cap()) return fail("mcs_run_pcuts_pipelined: export buffer overrun");
    if (sofar < n1) {
      return fail(format("mcs_run_pcuts_pipelined: pcut %d: the kernels' n_saved counters (%llu main + %llu late) are below the count of status bytes (%lld)",
                         i_pcut, (unsigned long long)h[PC_SAVED], (unsigned long long)h[PC_LATE_SAVED], n1));
    }
    const long long target = (long long)n_target[k];
    const bool last = k == npc - 1;
    long long n_open = n_T;                 // exported particles that have not been resumed yet
    if (sofar + n_T == 0) { o.n_saved[k] = 0; break; }                       // nobody left: the species ends here
    const long long im_hi = target / (sofar + n_T) > 1 ? target / (sofar + n_T) : 1;
    const long long im_lo = sofar > 0 ? (target / sofar > 1 ? target / sofar : 1) : -1;
    // (more long histories than the side stream's CUs hold at 16 per wave, twice over: beside the main launch they would outlast it)
    const long long side_cap = masked ? (long long)(int)c->o(MCS_OPT_PIPE_SIDE_CUS) * 8 * 16 * 2 : (long long)side_max * 4 * 16 * 2;
    if ((last || im_lo != im_hi || n_T > side_cap) && n_T > 0) {
      // i_mult depends on how many of the long histories end saved (or this is the last pcut, or they are too many): they finish first
      HIPCHK(hipMemsetAsync(pc + PC_RES_WORK, 0, 2 * sizeof(unsigned long long), s_alone));      // RES_WORK, RES_SAVED
      if (launch_resume(i_pcut, q, nA + nL, n_T, s_alone, true)) return 1;
      HIPCHK(hipMemcpyAsync(c->pp_hpc + PC_RES_SAVED, pc + PC_RES_SAVED, sizeof(unsigned long long), hipMemcpyDeviceToHost, s_alone));
      const auto tw0 = std::chrono::steady_clock::now();
      HIPCHK(hipStreamSynchronize(s_alone));
      dbg_wait_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
      sofar += (long long)c->pp_hpc[PC_RES_SAVED];
      n_open = 0;
      if (o.strag) o.strag[2 * k + 1] = 1;
      ++c->pp_waits_last;
    }
    if (dbg_pipe)
      std::fprintf(stderr, "[pipe] pcut %2d n_use %8lld (late %7lld) main %6.2f ms | side-sync %6.2f ms main-sync %6.2f ms | saved so far %8lld exported %6lld %s %6.2f ms\n",
                   i_pcut, nA + nL, nL, ms_main, std::chrono::duration<double, std::milli>(tj1 - tj0).count(),
                   std::chrono::duration<double, std::milli>(tj2 - tj1).count(), sofar, n_T, n_open == 0 && n_T > 0 ? "WAITED" : "      ", dbg_wait_ms);
    if (sofar + n_open == 0) { o.n_saved[k] = 0; break; }                  // (the long histories all ended: the species ends here)
    const long long i_mult = target / (sofar + n_open) > 1 ? target / (sofar + n_open) : 1;     // (== for both bounds when n_open > 0)
    o.i_mult[k] = i_mult;
    o.n_saved[k] = sofar;                 // (complete unless long histories are still open: then the next join adds those that end saved)
    if (last || sofar + n_open == 0) break;
    const long long B_next = (long_imult_max <= 0 || i_mult <= long_imult_max) ? long_draws : 0;
    // ---- the next pcut: main group = children of the saved particles that are not long; late group = children of the saved long ones
    const long long nA_next = n1 * i_mult;
    const long long n5_max = sofar - n1 + n_open;               // long particles that are saved, or still running
    const long long nL_max = n5_max * i_mult;
    // ((sofar + n_open) * i_mult <= max(n_target, sofar + n_open) <= cap_n: every buffer holds it)
    if (nA_next + nL_max > cap_n) return fail("mcs_run_pcuts_pipelined: the next population exceeds the buffers");
    // (the long histories go first: their few waves must be resident before the next main launch fills every slot of the chip --
    // queued behind it they would start when its workgroups leave, i.e. run after it instead of beside it.  Their counters are the side
    // stream's own words; everything else is cleared on the main stream, and the late split / late launch wait for that.)
    side_blocks = 0;
    s1 = (masked && n5_max > 0) ? c->pp_s1m : c->stream;      // (both are idle: the join synchronised the host with every stream)
    if (n5_max > 0) {
      HIPCHK(hipMemsetAsync(pc + PC_RES_WORK, 0, 2 * sizeof(unsigned long long), s2));
      if (n_open > 0 && launch_resume(i_pcut, q, nA + nL, n_open, s2, false)) return 1;
    }
    HIPCHK(hipMemsetAsync(pc, 0, PC_RES_WORK * sizeof(unsigned long long), s1));                 // the main launch's words, both export counts
    HIPCHK(hipMemsetAsync(pc + PC_LATE_WORK, 0, 3 * sizeof(unsigned long long), s1));            // LATE_WORK, LATE_SAVED, LATE_SCAN
    if (nA_next + nL_max > 0) HIPCHK(hipMemsetAsync(lsv[q ^ 1], 0, (size_t)(nA_next + nL_max), s1));
    HIPCHK(hipEventRecord(c->pp_reset, s1));
    HIPCHK(mcs_launch_split(savb[q], pop_view(c->spare), c->scan.src, nA_next, i_mult, s1));
    n1_prev = n1; sofar_prev = sofar;
    if (n5_max > 0) {
      HIPCHK(hipStreamWaitEvent(s2, c->pp_reset, 0));
      HIPCHK(mcs_launch_late_split(lsv[q], nA + nL, c->pp_scan.bcounts, c->pp_scan.boffs, pc + PC_LATE_SCAN, c->pp_scan.src, c->pp_dpdl + (q ^ 1), i_mult, nA_next, savb[q],
                                   pop_view(c->spare, nA_next), split_blocks(c, nL_max, 4), s2));
      // the late launch of the next pcut: particles nA_next .. of its population, their number read on the device
      KArgs& a = c->pp_hargs[2];
      fill_kargs(c, a, i_pcut + 1, nA_next, 0, 1, nullptr, B_next > 0 ? 1 : 0);
      a.in = pop_view(c->spare); a.sv = savb[q ^ 1]; a.l_save = lsv[q ^ 1];
      a.n_dev = &c->pp_dpdl[q ^ 1].n_use; a.fresh_lo = nA_next;
      set_counters(a, pc, PC_LATE_WORK, PC_LATE_SAVED, PC_EXPORT + (q ^ 1)); a.strag_out = c->strag.d[q ^ 1];
      a.long_draws = (unsigned int)B_next;
      HIPCHK(hipMemcpyAsync(c->pp_dargs + 2, &a, sizeof(KArgs), hipMemcpyHostToDevice, s2));
      const int blocks_l = persistent_grid(nL_max, threads, full);
      HIPCHK(mcs_launch_transport(c->pp_dargs + 2, k1.kernel, blocks_l, threads, s2));
      side_blocks += blocks_l;
      if (side_blocks > side_max) side_blocks = side_max;
      ++c->tail_rounds_last;
      side_pending = true;
      nL = nL_max;
    } else {
      nL = 0;
    }
    nA = nA_next;
    Bk = B_next;
    std::swap(c->cur, c->spare);
  }
  return 0;
}

// ---- A species' pcuts with the long histories of pcut p finishing BESIDE pcut p + 1 (DESIGN.md "Pipelined pcuts").
// A launch waits for its longest histories -- 10^4 passes of single particles while the chip idles (40 % of an iteration at 10^6
// particles).  What stands in the way of starting the next pcut is the ORDER of its population: child o of the split is a copy of
// saved particle o / i_mult in index order (src/cuts.jl:66-92), and the index keys the child's random stream -- one unresolved
// particle leaves every index behind it open.  Here the order is made independent of the schedule: a particle is LONG in a pcut when its
// history there took at least `long_draws` random draws (a property of its stream alone), and the next population is the children of
// the saved particles that are not long, in index order, followed by the children of the saved long ones, in index order.  The oracle
// orders the same way (orc_set_long_draws), so parity stays bit for bit; long_draws is a parameter of the algorithm like the seeds.
// Per pcut: the main launch (stream) and the late launch (side stream: the children of the previous pcut's saved long particles)
// export the particles that are still running once they are long and end; both join; the main group is split and the next main
// launch starts, while on the side stream the exported particles run to their end, the late group is split and the next late launch
// runs.  i_mult = max(n_target / n_saved, 1) needs the number of long particles that will be saved: it is taken as soon as both
// bounds give the same quotient, else the pcut waits for them (counted in strag_out).  One rank, global indices 0, 1, 2, ...; fp64 state.
// Outputs as mcs_run_pcuts_fused; strag_out (or NULL): [2k] particles pcut k exported, [2k + 1] 1 if its i_mult had to wait.
int mcs_run_pcuts_pipelined(mcs_ctx* c, int i_pcut_first, int i_pcut_last, const int64_t* n_target, int64_t long_draws, int64_t long_imult_max,
                            int64_t* n_use_out, int64_t* n_saved_out, int64_t* i_mult_out, double* kernel_ms_out, int64_t* strag_out) {
  MCS_ENTER(c);
  if (c->P.state_fp32) return fail("mcs_run_pcuts_pipelined: not for the fp32-state variant");
  if (long_draws < 64 || long_draws > 2000000000LL) return fail("mcs_run_pcuts_pipelined: long_draws out of range (64 .. 2e9)");
  const PcutOut o{n_use_out, n_saved_out, i_mult_out, kernel_ms_out, strag_out};
  const int npc = i_pcut_last - i_pcut_first + 1;
  long long cap_n = 0;
  if (species_loop_open(c, "mcs_run_pcuts_pipelined", i_pcut_first, i_pcut_last, n_target, o, &cap_n)) return 1;
  const long long cap = grow_cap(cap_n);
  if (reserve(c->pp_sav2, cap)) return 1;
  if (c->pp_lsave2.cap() < cap || c->pp_scan.cap() < cap) {
    HIPCHK(hipStreamSynchronize(c->stream));      // (queued work may still use the blocks that are freed)
    if (reserve(c->pp_lsave2, cap) || reserve(c->pp_scan, cap)) return 1;
  }
  // what the first call creates (each guarded by itself: a call that failed half-way is made up for by the next one)
  if (!c->pp_s2) HIPCHK(c->pp_s2.create_non_blocking());
  if (!c->pp_reset) HIPCHK(c->pp_reset.create_untimed());
  if (reserve(c->pp_dpc, PC_COUNT) || reserve(c->pp_hpc, PC_COUNT) || reserve(c->pp_hargs, 3) || reserve(c->pp_dargs, 3) || reserve(c->pp_dpdl, 2) ||
      reserve(c->pp_hpdl, 2))
    return 1;
  if (!c->pp_masks_tried) {
    c->pp_masks_tried = true;
    if ((int)c->o(MCS_OPT_PIPE_SIDE_CUS) > 0 && (int)c->o(MCS_OPT_PIPE_SIDE_CUS) < c->n_cu) {
      const int words = (c->n_cu + 31) / 32;
      std::vector<uint32_t> m_side((size_t)words, 0u), m_main((size_t)words, 0u);
      for (int i = 0; i < c->n_cu; ++i) (i < (int)c->o(MCS_OPT_PIPE_SIDE_CUS) ? m_side : m_main)[(size_t)(i >> 5)] |= 1u << (i & 31);
      if (c->pp_s1m.create_cu_masked((uint32_t)words, m_main.data()) != hipSuccess ||
          c->pp_s2m.create_cu_masked((uint32_t)words, m_side.data()) != hipSuccess) {
        (void)hipGetLastError();
        reset_all(c->pp_s1m, c->pp_s2m);
      }
    }
  }
  // the sliced form of the species' kernel (PLAIN, LOSSY, PLAIN_ETF, general); a wave exports at most its 64 lanes, once: room for the
  // main and the late launch of one pcut
  const K1Plan k1 = k1_plan(c, 0, true, false);
  if (ensure_strag(c, 2 * (long long)c->n_cu * k1.per_cu * k1.threads)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));
  int rc = pipelined_pcuts(c, k1, i_pcut_first, npc, cap_n, n_target, long_draws, long_imult_max, o);
  // every exit of the loop, a failed one too: no stream may still write the population, the saved arrays or the tallies
  for (hipStream_t st : {(hipStream_t)c->pp_s2, (hipStream_t)c->pp_s2m, (hipStream_t)c->pp_s1m, c->stream}) {
    if (!st) continue;
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess && rc == 0) rc = fail(std::string("mcs_run_pcuts_pipelined: hipStreamSynchronize: ") + hipGetErrorString(e));
  }
  if (rc) c->n = 0;      // (the population is half-written: it is not run or split again before the next mcs_init_pop* / mcs_pop_upload)
  c->n_run_last = -1; c->n_saved_last = 0;
  c->kernel_last = k1.kernel;
  return rc;
}

int mcs_new_pcut(mcs_ctx* c, int64_t i_mult, int64_t* n_new_out) {
  MCS_ENTER(c);
  if (i_mult < 1) return fail("mcs_new_pcut: i_mult < 1");
  if (c->n != c->n_run_last) return fail("mcs_new_pcut: no mcs_run_pcut since the population changed");
  const long long n_saved = c->n_saved_last;
  const long long n_new = n_saved * i_mult;
  // the split (src[] was computed behind the transport kernel) writes into the spare buffer, then the buffers
  // rotate; nothing is read back: the new size is known on the host
  if (reserve(c->spare, grow_cap(n_new))) return 1;
  HIPCHK(mcs_launch_split(pop_view(c->sav), pop_view(c->spare), c->scan.src, n_new, i_mult, c->stream));
  std::swap(c->cur, c->spare);
  c->n = n_new; c->n_run_last = -1;
  if (ensure_capacity(c, n_new)) return 1;
  if (n_new_out) *n_new_out = n_new;
  return 0;
}

// mcs_saved_export, and mcs_saved_gidx (`state` false: the global indices alone)
static int saved_export(mcs_ctx* c, const char* who, bool state, int64_t cap, int64_t* dev_gidx, double* dev_f64, uint32_t* dev_meta) {
  MCS_ENTER_AS(c, who);
  const std::string w = std::string(who) + ": ";
  if (c->n != c->n_run_last) return fail(w + "no mcs_run_pcut since the population changed");
  if (cap < c->n_saved_last) return fail(w + "cap < n_saved");
  if (c->n_saved_last > 0 && (!dev_gidx || (state && (!dev_f64 || !dev_meta)))) return fail(w + "null buffer");
  HIPCHK(mcs_launch_saved_export(pop_view(c->sav), c->scan.src, c->n_saved_last, cap, c->idx_first, c->idx_stride, c->idx_gidx,
                                 (long long*)dev_gidx, dev_f64, dev_meta, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));      // the caller's library (RCCL on another stream) may read the buffers now
  return 0;
}
int mcs_saved_export(mcs_ctx* c, int64_t cap, int64_t* dev_gidx, double* dev_f64, uint32_t* dev_meta) {
  return saved_export(c, "mcs_saved_export", true, cap, dev_gidx, dev_f64, dev_meta);
}
int mcs_saved_gidx(mcs_ctx* c, int64_t cap, int64_t* dev_gidx) { return saved_export(c, "mcs_saved_gidx", false, cap, dev_gidx, nullptr, nullptr); }

int mcs_split_import(mcs_ctx* c, int64_t n_parents, int64_t cap, const double* dev_f64, const uint32_t* dev_meta, int64_t i_mult,
                     int64_t first, int64_t stride, int64_t n_local) {
  MCS_ENTER(c);
  if (i_mult < 1 || stride < 1 || first < 0 || n_local < 0 || n_parents < 0 || cap < n_parents)
    return fail("mcs_split_import: bad arguments");
  if (n_local > 0 && (first + (n_local - 1) * stride) / i_mult >= n_parents)
    return fail("mcs_split_import: the local slice reaches past n_parents * i_mult");
  if (n_local > 0 && (!dev_f64 || !dev_meta)) return fail("mcs_split_import: null buffer");
  if (reserve(c->spare, grow_cap(n_local))) return 1;
  HIPCHK(mcs_launch_split_import(pop_view(c->spare), dev_f64, dev_meta, cap, i_mult, first, stride, n_local, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));      // the caller may free or reuse its buffers
  std::swap(c->cur, c->spare);
  c->n = n_local; c->n_run_last = -1;
  if (ensure_capacity(c, n_local)) return 1;
  return 0;
}

int mcs_run_pcut_host(mcs_ctx* c, int i_pcut, int64_t n_pts_use, int64_t i_prt_offset, const mcs_soa* in, mcs_soa* saved_out,
                      uint8_t* l_save, int64_t* n_saved) {
  if (mcs_pop_upload(c, n_pts_use, in)) return 1;
  if (mcs_run_pcut(c, i_pcut, i_prt_offset, n_saved)) return 1;
  return mcs_saved_download(c, n_pts_use, saved_out, l_save);
}

int mcs_read_tallies(mcs_ctx* c, double* host_f64, int64_t* host_i64) {
  MCS_ENTER(c);
  return mcs_read_tallies_part(c, 0, host_f64 ? c->L.total : 0, host_f64, host_i64);
}
int mcs_read_tallies_part(mcs_ctx* c, int64_t first, int64_t count, double* host_f64, int64_t* host_i64) {
  MCS_ENTER(c);
  if (first < 0 || count < 0 || first + count > c->L.total || (count > 0 && !host_f64)) return fail("mcs_read_tallies_part: range outside the tally buffer");
  if (fold_replicas(c)) return 1;
  if (count > 0) HIPCHK(hipMemcpyAsync(host_f64, c->d_T + first, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (host_i64) HIPCHK(hipMemcpyAsync(host_i64, c->d_I, (size_t)mcs_i64_total(&c->P) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int mcs_write_tallies_part(mcs_ctx* c, int64_t first, int64_t count, const double* host_f64) {
  MCS_ENTER(c);
  if (first < 0 || count < 0 || first + count > c->L.total || (count > 0 && !host_f64)) return fail("mcs_write_tallies_part: range outside the tally buffer");
  if (fold_replicas(c)) return 1;
  c->photon_flags_clear();
  c->have_ang = false;
  c->have_prof = false;
  if (count > 0) HIPCHK(hipMemcpyAsync(c->d_T + first, host_f64, (size_t)count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int mcs_write_tallies(mcs_ctx* c, const double* host_f64, const int64_t* host_i64) {
  MCS_ENTER(c);
  if (fold_replicas(c)) return 1;
  c->photon_flags_clear();
  c->have_ang = false;
  c->have_prof = false;
  if (host_f64) HIPCHK(hipMemcpyAsync(c->d_T, host_f64, (size_t)c->L.total * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (host_i64) HIPCHK(hipMemcpyAsync(c->d_I, host_i64, (size_t)mcs_i64_total(&c->P) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// The running sums of src added into dst's and cleared in src (the split of the layout: include/mcs.h, beside mcs_tally_layout).
// Ordered on the two streams, no host synchronisation: dst's stream waits for what src's stream has queued, runs the kernel, and src's
// stream waits for the kernel before anything else may add to the sums it clears.
int mcs_accumulate_tallies(mcs_ctx* dst, mcs_ctx* src) {
  if (!dst || !src) return fail("mcs_accumulate_tallies: null context");
  if (dst == src) return fail("mcs_accumulate_tallies: dst and src are the same context");
  if (dst->device != src->device) return fail("mcs_accumulate_tallies: the contexts are on different devices");
  if (dst->L.total != src->L.total || dst->P.n_grid != src->P.n_grid || dst->P.n_ions != src->P.n_ions || dst->P.n_itrs != src->P.n_itrs)
    return fail("mcs_accumulate_tallies: the contexts' tally layouts differ (total, n_grid, n_ions or n_itrs)");
  MCS_ENTER(dst);
  if (fold_replicas(src) || fold_replicas(dst)) return 1;
  const mcs_layout& L = dst->L;
  HIPCHK(hipEventRecord(src->acc_ev, src->stream));
  HIPCHK(hipStreamWaitEvent(dst->stream, src->acc_ev, 0));
  HIPCHK(mcs_launch_accumulate_tallies(dst->d_T, src->d_T, dst->d_I, src->d_I, L.esc_flux, L.energy_recv_pool - L.esc_flux, L.scalars, 4,
                                       dst->P.n_grid, MCS_IC_COUNT, dst->stream));
  HIPCHK(hipEventRecord(dst->acc_ev, dst->stream));
  HIPCHK(hipStreamWaitEvent(src->stream, dst->acc_ev, 0));
  return 0;
}

// fn < MCS_FN_SQRT_FAST: mcs_k_eval_fn in mcs_population.hip (the build of K3); from there on: mcs_k_eval_hot in mcs_transport.hip,
// the transport kernel's own forms in its own translation unit
int mcs_eval_fn(mcs_ctx* c, int fn, int64_t n, const double* a, const double* b, double* out) {
  MCS_ENTER(c);
  if (n < 0 || (n > 0 && (!a || !out))) return fail("mcs_eval_fn: null argument or negative n");
  if (fn < 0 || fn >= MCS_FN_COUNT) return fail("mcs_eval_fn: unknown fn " + std::to_string(fn) + " (enum mcs_fn, include/mcs.h)");
  if (reserve(c->d_stage, 3 * n + 3)) return 1;
  double *da = c->d_stage, *db = c->d_stage + n, *dout = c->d_stage + 2 * n;
  HIPCHK(hipMemcpyAsync(da, a, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(db, b ? b : a, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(fn < MCS_FN_SQRT_FAST ? mcs_launch_eval(fn, n, da, db, dout, c->stream) : mcs_launch_eval_hot(fn, n, da, db, dout, c->stream));
  HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// One scatter per state in the transport kernel's three spellings (include/mcs.h).  The kernel reads pe_crit, game_crit and eta_mfp
// where K1 reads them: from a KArgs in the constant address space -- the context's own, with nothing but the parameters filled in.
int mcs_eval_scatter(mcs_ctx* c, int form, int64_t n, const double* in, double* out) {
  MCS_ENTER(c);
  if (n < 0 || (n > 0 && (!in || !out))) return fail("mcs_eval_scatter: null argument or negative n");
  if (form < 0 || form > 2) return fail("mcs_eval_scatter: unknown form " + std::to_string(form) + " (0, 1 or 2: include/mcs.h)");
  if (reserve(c->d_stage, 15 * n + 2) || reserve(c->d_args, 1) || reserve(c->h_args_pin, 1)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));         // (nothing queued may still read the launch constants)
  KArgs& a = *c->h_args_pin;
  a = KArgs{};
  a.P = c->P;
  double *din = c->d_stage, *dout = c->d_stage + 10 * n;
  HIPCHK(hipMemcpyAsync(c->d_args, c->h_args_pin, sizeof(KArgs), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(din, in, (size_t)n * 10 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(mcs_launch_eval_scatter(c->d_args, form, n, din, dout, c->stream));
  HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * 5 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// The caller's tally records through K1's own tally code (include/mcs.h): launch constants from fill_kargs, as a transport launch of
// pcut 1 over an empty population has them; the replicas marked as such a launch marks them.  Every record is checked before anything
// is queued: the kernel indexes LDS tables and the tally buffer with what the words say.
int mcs_eval_tally(mcs_ctx* c, int form, int64_t n_pass, int64_t n_thread, const double* rec, const uint64_t* word) {
  MCS_ENTER(c);
  const std::string w = "mcs_eval_tally: ";
  if (n_pass < 0 || n_thread < 0 || (n_pass > 0 && n_thread > 0 && (!rec || !word))) return fail(w + "null argument or negative count");
  if (form < 0 || form > 2) return fail(w + "unknown form " + std::to_string(form) + " (0, 1 or 2: include/mcs.h)");
  if (!c->have_grid || !c->have_cuts) return fail(w + "grid/cuts not set");
  if (c->n != 0) return fail(w + "the context holds a population (the launch constants are those of an empty one)");
  if (n_pass > 0 && n_thread > INT64_MAX / n_pass / (MCS_TALLY_REC_F64 + 1)) return fail(w + "n_pass * n_thread is too large");
  const int64_t n = n_pass * n_thread;
  const int ng = c->P.n_grid;
  for (int64_t e = 0; e < n; ++e) {
    const uint64_t u = word[e];
    const int kind = (int)((u >> 40) & 0xffu), aux = (int)((u >> 32) & 0xffu);
    const int i_grid = (int)(u & 0xffu), i_grid_old = (int)((u >> 8) & 0xffu), ig3 = (int)((u >> 16) & 0xffu);
    const std::string at = w + "record " + std::to_string(e) + ": ";
    if ((u >> 48) != 0 || ((u >> 25) & 0x7fu) != 0 || kind > 3) return fail(at + "unknown kind or stray bits in the word (include/mcs.h)");
    if (kind == 0) continue;
    const double* r = rec + MCS_TALLY_REC_F64 * e;
    for (int j = 0; j < MCS_TALLY_REC_F64; ++j) {
      if (!std::isfinite(r[j])) return fail(at + "value " + std::to_string(j) + " is not finite");
      if (form == 2 && (double)(float)r[j] != r[j]) return fail(at + "value " + std::to_string(j) + " is no float (form 2 takes fp32 values)");
    }
    if (i_grid > ng + 1 || i_grid_old > ng + 1 || ig3 > ng + 1) return fail(at + "zone index outside [0, n_grid + 1]");
    if (kind == 1) {
      // F_stream! walks zones i_grid_old + 1 .. i_grid (x > x_old) or i_grid_old .. i_grid + 1 (else): all_flux! leaves both in [0, n_grid]
      const double x = form == 2 ? (double)(float)r[6] : r[6], x_old = form == 2 ? (double)(float)r[7] : r[7];
      const bool down = x > x_old;
      const int lo = down ? i_grid_old + 1 : i_grid + 1, hi = down ? i_grid : i_grid_old;
      if (lo <= hi && (lo < 1 || hi > ng)) return fail(at + "the crossing would tally outside zones 1 .. n_grid");
    } else if (kind == 2) {
      if (aux < 1 || aux > 4) return fail(at + "i_reason outside 1 .. 4");
    } else {
      if (aux < 1 || aux > c->tb.n_tcuts) return fail(at + "time cut outside [1, n_tcuts]");
    }
  }
  if (form != 0) {
    // A wave's stack: drained to below `drain_at` at the top of a pass, then one record per pushing lane.  The capacity rests on at most
    // two passes' worth of pushes between drains (MCS_EV_CAP, mcs_device.h); this layout keeps to it by construction, and the walk below
    // refuses whatever would not.
    int cap = 0, drain_at = 0;
    if (mcs_eval_tally_stack(form, &cap, &drain_at)) return fail(w + "no stack for this form");
    const int64_t n_wave = (n_thread + 63) / 64;
    std::vector<int> height((size_t)n_wave, 0);
    for (int64_t p = 0; p < n_pass; ++p)
      for (int64_t t = 0; t < n_thread; ++t) {
        int& h = height[(size_t)(t / 64)];
        if (t % 64 == 0) while (h >= drain_at) h -= std::min(h, 64);
        const int kind = (int)((word[p * n_thread + t] >> 40) & 0xffu);
        if (kind == 1 || kind == 2) {
          if (++h > cap) return fail(w + "pass " + std::to_string(p) + ": more records pending than a wave's stack holds");
        }
      }
  }
  if (n == 0) return 0;
  if (reserve(c->d_stage, (MCS_TALLY_REC_F64 + 1) * n + 2) || reserve(c->d_args, 1) || reserve(c->h_args_pin, 1)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));         // (nothing queued may still read the launch constants)
  KArgs& a = *c->h_args_pin;
  fill_kargs(c, a, 1, 0, 0, 1, nullptr, 0);
  double* drec = c->d_stage;
  unsigned long long* dword = (unsigned long long*)(c->d_stage + MCS_TALLY_REC_F64 * n);
  HIPCHK(hipMemcpyAsync(c->d_args, c->h_args_pin, sizeof(KArgs), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(drec, rec, (size_t)n * MCS_TALLY_REC_F64 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dword, word, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(mcs_launch_eval_tally(c->d_args, form, n_pass, n_thread, drec, dword, c->stream));
  c->rep_dirty = true;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// One move of Code Block 2 per state of the context's population through K1's own move and post-move code (include/mcs.h): launch
// constants from fill_kargs, as a transport launch of pcut i_pcut over this population has them; the replicas marked as such a launch
// marks them.  The states' indices were checked by mcs_pop_upload; the kernel writes only `out`, `word` and the tallies.
int mcs_eval_move(mcs_ctx* c, int form, int post, int i_pcut, int64_t n, const double* x_thr, double* out, uint64_t* word) {
  MCS_ENTER(c);
  const std::string w = "mcs_eval_move: ";
  if (n < 0 || (n > 0 && (!out || !word))) return fail(w + "null argument or negative count");
  if (form < 0 || form > 3) return fail(w + "unknown form " + std::to_string(form) + " (0 .. 3: include/mcs.h)");
  if (post < 0 || post > 4) return fail(w + "unknown post " + std::to_string(post) + " (0 .. 4: include/mcs.h)");
  if (form != 0 && n > 0 && !x_thr) return fail(w + "null argument (forms 1 .. 3 take x_thr)");
  if (!c->have_grid || !c->have_cuts) return fail(w + "grid/cuts not set");
  if (i_pcut < 1 || i_pcut > c->tb.n_pcuts) return fail(w + "i_pcut outside [1, n_pcuts]");
  if (c->P.state_fp32) return fail(w + "the context holds fp32 state (the move of the fp32 kernels is another function)");
  if (n != c->n) return fail(w + "n is not the size of the context's population (mcs_pop_upload)");
  if (form != 0)
    for (int64_t k = 0; k < n; ++k)
      if (!std::isfinite(x_thr[k])) return fail(w + "x_thr[" + std::to_string(k) + "] is not finite");
  if (n == 0) return 0;
  if (n > INT64_MAX / (MCS_MOVE_OUT_F64 + 2)) return fail(w + "n is too large");
  if (reserve(c->d_stage, (MCS_MOVE_OUT_F64 + 2) * n) || reserve(c->d_args, 1) || reserve(c->h_args_pin, 1)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));         // (nothing queued may still read the launch constants)
  KArgs& a = *c->h_args_pin;
  fill_kargs(c, a, i_pcut, n, 0, 1, nullptr, 0);
  a.f_reason = nullptr; a.f_helix = nullptr; a.f_retro = nullptr; a.f_ptot = nullptr; a.f_x = nullptr;
  double* dthr = c->d_stage;
  double* dout = c->d_stage + n;
  unsigned long long* dword = (unsigned long long*)(c->d_stage + (MCS_MOVE_OUT_F64 + 1) * n);
  HIPCHK(hipMemcpyAsync(c->d_args, c->h_args_pin, sizeof(KArgs), hipMemcpyHostToDevice, c->stream));
  if (form != 0) HIPCHK(hipMemcpyAsync(dthr, x_thr, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(mcs_launch_eval_move(c->d_args, form, post, n, dthr, dout, dword, c->stream));
  c->rep_dirty = true;
  HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * MCS_MOVE_OUT_F64 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(word, dword, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// One pass boundary per state of the context's population through K1's own move, slow_post and slow_pre (include/mcs.h): launch
// constants and replicas as in mcs_eval_move.  The kernel writes only `out`, `word` and the tallies.
int mcs_eval_pass(mcs_ctx* c, int form, int i_pcut, int64_t n, const int32_t* helix, double* out, uint64_t* word) {
  MCS_ENTER(c);
  const std::string w = "mcs_eval_pass: ";
  if (n < 0 || (n > 0 && (!helix || !out || !word))) return fail(w + "null argument or negative count");
  if (form < 0 || form > 1) return fail(w + "unknown form " + std::to_string(form) + " (0 .. 1: include/mcs.h)");
  if (!c->have_grid || !c->have_cuts) return fail(w + "grid/cuts not set");
  if (i_pcut < 1 || i_pcut > c->tb.n_pcuts) return fail(w + "i_pcut outside [1, n_pcuts]");
  if (c->P.state_fp32) return fail(w + "the context holds fp32 state (the pass head of the fp32 kernels is another function)");
  if (form == 1 && !(c->aa < 1 && c->P.do_rad_losses && !c->P.use_custom_epsB && !c->P.dont_scatter))
    return fail(w + "form 1 is the LOSSY kernel's: a species with aa < 1, do_rad_losses, no custom eps_B, no dont_scatter");
  if (n != c->n) return fail(w + "n is not the size of the context's population (mcs_pop_upload)");
  for (int64_t k = 0; k < n; ++k)
    if (helix[k] < 1 || helix[k] > 16000) return fail(w + "helix[" + std::to_string(k) + "] outside [1, 16000]");
  if (n == 0) return 0;
  if (n > INT64_MAX / (MCS_PASS_OUT_F64 + 2)) return fail(w + "n is too large");
  if (reserve(c->d_stage, (MCS_PASS_OUT_F64 + 2) * n) || reserve(c->d_args, 1) || reserve(c->h_args_pin, 1)) return 1;
  HIPCHK(hipStreamSynchronize(c->stream));         // (nothing queued may still read the launch constants)
  KArgs& a = *c->h_args_pin;
  fill_kargs(c, a, i_pcut, n, 0, 1, nullptr, 0);
  a.f_reason = nullptr; a.f_helix = nullptr; a.f_retro = nullptr; a.f_ptot = nullptr; a.f_x = nullptr;
  double* dstage = c->d_stage;
  int* dhelix = (int*)dstage;                      // (n ints in the first n doubles)
  double* dout = dstage + n;
  unsigned long long* dword = (unsigned long long*)(dstage + (MCS_PASS_OUT_F64 + 1) * n);
  HIPCHK(hipMemcpyAsync(c->d_args, c->h_args_pin, sizeof(KArgs), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dhelix, helix, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(mcs_launch_eval_pass(c->d_args, form, n, dhelix, dout, dword, c->stream));
  c->rep_dirty = true;
  HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * MCS_PASS_OUT_F64 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(word, dword, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// K2 on the caller's status bytes and saved states (include/mcs.h): the launchers mcs_run_pcut / mcs_new_pcut / mcs_saved_export (form 0),
// mcs_run_pcuts_fused (form 1) and pipelined_pcuts (form 2) call, with their grids, on the context's own saved arrays, status bytes,
// scan scratch and counter words; the target is the spare buffer between two guards.  Everything is checked before anything is
// changed; the number of children is known on the host (a count of the caller's bytes), so a target that is too small is refused.
int mcs_eval_pcut_split(mcs_ctx* c, mcs_pcut_eval* io) {
  MCS_ENTER(c);
  const std::string w = "mcs_eval_pcut_split: ";
  if (!io) return fail(w + "null argument");
  const long long n = io->n, cap_n = io->cap_n, guard = io->guard, out_cap = io->out_cap, exp_cap = io->exp_cap;
  const int form = io->form;
  if (form < 0 || form > 2) return fail(w + "unknown form " + std::to_string(form) + " (0, 1 or 2: include/mcs.h)");
  if (n < 0 || cap_n < n) return fail(w + "n < 0 or n > cap_n");
  if (guard < 0 || out_cap < 0 || guard > (1LL << 40) || out_cap > (1LL << 40)) return fail(w + "guard or out_cap out of range");
  const long long total = 2 * guard + out_cap;
  if (cap_n > 0) {
    if (!io->l_save || !io->saved || !io->src) return fail(w + "null buffer");
    for (auto f : kSoaF64) if (!(io->saved->*f)) return fail(w + "null buffer");
    if (!io->saved->grid || !io->saved->tcut || !io->saved->downstream || !io->saved->inj) return fail(w + "null buffer");
    if (io->src_fill < 0 || io->src_fill >= cap_n) return fail(w + "src_fill outside [0, cap_n)");
  }
  if (total > 0 && (!io->out_f64 || !io->out_meta)) return fail(w + "null buffer");
  if (form != 0 && io->export_mode != 0) return fail(w + "export_mode only with form 0");
  if (form == 0 && io->match != 1 && io->match != 5) return fail(w + "match must be 1 or 5");
  if (form == 0 && (io->export_mode < 0 || io->export_mode > 2)) return fail(w + "unknown export_mode");
  if (form != 1 && io->i_mult < 1) return fail(w + "i_mult < 1");
  if (form == 1 && (io->n_target < 1 || cap_n < 1)) return fail(w + "n_target < 1 or cap_n < 1");
  if (form == 2 && c->P.state_fp32) return fail(w + "the late form is not for the fp32-state variant");
  if (form == 2 && io->n_main_next < 0) return fail(w + "n_main_next < 0");
  for (long long k = 0; k < cap_n; ++k)
    if (io->saved->grid[k] < 0 || io->saved->grid[k] > 0xffff || io->saved->tcut[k] < 0 || io->saved->tcut[k] > 0xff)
      return fail(w + "a saved state's grid or tcut does not fit the packed word");
  const unsigned int match = form == 0 ? (unsigned int)io->match : form == 1 ? 1u : 5u;
  long long ns = 0;
  for (long long k = 0; k < n; ++k) ns += io->l_save[k] == match;
  const long long im = form == 1 ? (ns > 0 && io->n_target / ns > 1 ? io->n_target / ns : 1) : (long long)io->i_mult;
  const long long off = form == 2 ? (long long)io->n_main_next : 0;
  if (off > out_cap || (ns > 0 && im > (out_cap - off) / ns)) return fail(w + "the children do not fit out_cap");
  const bool exporting = form == 0 && io->export_mode != 0, states = io->export_mode == 2;
  if (exporting) {
    if (exp_cap < ns || exp_cap > (1LL << 40)) return fail(w + "exp_cap < n_saved");
    if (exp_cap > 0 && (!io->exp_gidx || (states && (!io->exp_f64 || !io->exp_meta)))) return fail(w + "null buffer");
  }
  // ---- nothing was changed so far
  hipStream_t st = c->stream;
  HIPCHK(hipStreamSynchronize(st));      // (queued work may still use the blocks that are freed)
  if (ensure_capacity(c, cap_n) || reserve(c->spare, total) || reserve(c->fused, 1)) return 1;
  if (exporting && reserve(c->d_stage, n + 9 * exp_cap + exp_cap / 2 + 2)) return 1;
  c->n_run_last = -1; c->n_saved_last = 0; c->idx_gidx = nullptr;      // the saved arrays / src[] no longer describe a run
  if (cap_n > 0) {
    HIPCHK(hipMemcpyAsync(c->d_lsave, io->l_save, (size_t)cap_n, hipMemcpyHostToDevice, st));
    if (upload_soa(c, c->sav, cap_n, io->saved)) return 1;
    const std::vector<long long> stale((size_t)cap_n, (long long)io->src_fill);
    HIPCHK(hipMemcpyAsync(c->scan.src, stale.data(), (size_t)cap_n * sizeof(long long), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (total > 0) {
    for (int i = 0; i < 8; ++i) HIPCHK(hipMemsetAsync(c->spare.f[i], 0xA5, (size_t)total * sizeof(double), st));
    HIPCHK(hipMemsetAsync(c->spare.meta, 0xA5, (size_t)total * sizeof(uint32_t), st));
  }
  PcutDev h_pd[2] = {{form == 1 ? n : -7, -7, -7, -7}, {-7, -7, -7, -7}};
  unsigned long long h_ctr[CTR_COUNT] = {};
  if (form == 1) { h_ctr[CTR_WORK] = io->ctr_work; h_ctr[CTR_SAVED] = io->ctr_saved; }
  HIPCHK(hipMemcpyAsync(c->fused.d_pd, h_pd, sizeof h_pd, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->d_counters, h_ctr, sizeof h_ctr, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  const DevPop sav = pop_view(c->sav);
  unsigned long long* const scan_total = c->d_counters + CTR_SCAN;
  if (form == 0) {
    HIPCHK(mcs_launch_compact_match(c->d_lsave, n, c->scan.bcounts, c->scan.boffs, scan_total, c->scan.src, match, st));
    HIPCHK(hipMemcpyAsync(c->h_back + CTR_SCAN, scan_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const long long n_saved = (long long)c->h_back[CTR_SCAN];
    if (n_saved != ns) return fail(w + format("the compaction counted %lld saved particles, the host %lld: the split was not run", n_saved, ns));
    HIPCHK(mcs_launch_split(sav, pop_view(c->spare, guard), c->scan.src, n_saved * im, im, st));
    if (exporting) {
      long long* d_gin = (long long*)c->d_stage.get();
      long long* d_gidx = d_gin + n;
      double* d_f64 = c->d_stage + n + exp_cap;
      uint32_t* d_meta = (uint32_t*)(c->d_stage + n + 9 * exp_cap);
      if (io->exp_gin && n > 0) HIPCHK(hipMemcpyAsync(d_gin, io->exp_gin, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemsetAsync(d_gidx, 0xA5, (size_t)(9 * exp_cap + exp_cap / 2 + 1) * sizeof(double), st));
      HIPCHK(mcs_launch_saved_export(sav, c->scan.src, n_saved, exp_cap, io->exp_first, io->exp_stride, io->exp_gin ? d_gin : nullptr, d_gidx,
                                     states ? d_f64 : nullptr, states ? d_meta : nullptr, st));
      if (exp_cap > 0) {
        HIPCHK(hipMemcpyAsync(io->exp_gidx, d_gidx, (size_t)exp_cap * sizeof(long long), hipMemcpyDeviceToHost, st));
        // (indices only: the state buffers, where the caller wants them, must come back as they were filled)
        if (io->exp_f64) HIPCHK(hipMemcpyAsync(io->exp_f64, d_f64, (size_t)(8 * exp_cap) * sizeof(double), hipMemcpyDeviceToHost, st));
        if (io->exp_meta) HIPCHK(hipMemcpyAsync(io->exp_meta, d_meta, (size_t)exp_cap * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      }
    }
  } else if (form == 1) {
    HIPCHK(mcs_launch_finalize_split_dev(c->d_lsave, cap_n, c->scan.bcounts, c->scan.boffs, scan_total, c->scan.src, c->fused.d_pd, c->fused.d_pd + 1,
                                         c->d_counters, (long long)io->n_target, c->d_counters + CTR_MISMATCH, sav, pop_view(c->spare, guard),
                                         split_blocks(c, cap_n, 16), st));
  } else {
    HIPCHK(mcs_launch_late_split(c->d_lsave, n, c->scan.bcounts, c->scan.boffs, scan_total, c->scan.src, c->fused.d_pd, im, off, sav,
                                 pop_view(c->spare, guard + off), split_blocks(c, ns * im, 4), st));
  }
  if (cap_n > 0) HIPCHK(hipMemcpyAsync(io->src, c->scan.src, (size_t)cap_n * sizeof(long long), hipMemcpyDeviceToHost, st));
  for (int i = 0; i < 8 && total > 0; ++i)
    HIPCHK(hipMemcpyAsync(io->out_f64 + (size_t)i * (size_t)total, c->spare.f[i], (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st));
  if (total > 0) HIPCHK(hipMemcpyAsync(io->out_meta, c->spare.meta, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h_pd, c->fused.d_pd, sizeof h_pd, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h_ctr, c->d_counters, sizeof h_ctr, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemsetAsync(c->d_counters, 0, sizeof h_ctr, st));
  HIPCHK(hipStreamSynchronize(st));
  io->scan_total = h_ctr[CTR_SCAN]; io->ctr_work_after = h_ctr[CTR_WORK]; io->ctr_saved_after = h_ctr[CTR_SAVED]; io->mismatch = h_ctr[CTR_MISMATCH];
  for (int k = 0; k < 2; ++k) {
    int64_t* o = k ? io->pd_next : io->pd;
    o[0] = h_pd[k].n_use; o[1] = h_pd[k].n_saved; o[2] = h_pd[k].i_mult; o[3] = h_pd[k].n_new;
  }
  return 0;
}

int mcs_final_download(mcs_ctx* c, int64_t n, int32_t* reason, int32_t* helix_count, int32_t* retro_count, double* ptot_pf,
                       double* x_PT_cm) {
  MCS_ENTER(c);
  if (!c->debug_finals) return fail("mcs_final_download: end states are recorded only after mcs_set_debug_finals(ctx, 1)");
  if (n > c->fin.cap()) return fail("mcs_final_download: n too large");
  if (reason) HIPCHK(hipMemcpyAsync(reason, c->fin.reason, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (helix_count) HIPCHK(hipMemcpyAsync(helix_count, c->fin.helix, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (retro_count) HIPCHK(hipMemcpyAsync(retro_count, c->fin.retro, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (ptot_pf) HIPCHK(hipMemcpyAsync(ptot_pf, c->fin.ptot, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  if (x_PT_cm) HIPCHK(hipMemcpyAsync(x_PT_cm, c->fin.x, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

double mcs_last_kernel_ms(mcs_ctx* c) { return c->last_ms; }

// ---- consumers of the tallies (K4) ------------------------------------------------------
static int consumers_ready(mcs_ctx* c, const mcs_consumer_in* in, const char* who) {
  if (!in) return fail(std::string(who) + ": null argument");
  if (!c->have_grid) return fail(std::string(who) + ": grid not set");
  if (c->P.num_psd_mom_bins + 2 > 208 || c->P.num_psd_tht_bins + 2 > 208) return fail(std::string(who) + ": too many PSD bins");
  const int NM = c->P.num_psd_mom_bins + 2, NT = c->P.num_psd_tht_bins + 2, ng = c->P.n_grid;
  return reserve(c->d_ctab, 3 * NM + 2 * NT + 4 * ng) || reserve(c->d_cout, 3 * ng * NM + 3 * ng) || reserve(c->d_cdiag, 2);
}

int mcs_dndp_cr(mcs_ctx* c, const mcs_consumer_in* in, double* dNdp, int64_t* diag) {
  MCS_ENTER(c);
  if (consumers_ready(c, in, "mcs_dndp_cr")) return 1;
  if (fold_replicas(c)) return 1;
  if (!in->mom_log_cgs || !in->mom_edge_cgs || !in->cos_edge || !in->zone_pop || !dNdp) return fail("mcs_dndp_cr: null table");
  c->have_cout_dndp = false;
  const int NM = c->P.num_psd_mom_bins + 2, NT = c->P.num_psd_tht_bins + 2, ng = c->P.n_grid;
  std::vector<double> h((size_t)(2 * NM + NT + ng));
  memcpy(h.data(), in->mom_log_cgs, sizeof(double) * NM);
  memcpy(h.data() + NM, in->mom_edge_cgs, sizeof(double) * NM);
  memcpy(h.data() + 2 * NM, in->cos_edge, sizeof(double) * NT);
  memcpy(h.data() + 2 * NM + NT, in->zone_pop, sizeof(double) * ng);
  HIPCHK(hipMemcpyAsync(c->d_ctab, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(c->d_cdiag, 0, sizeof(unsigned long long) * 2, c->stream));
  HIPCHK(mcs_launch_dndp_cr(&c->P, c->d_T + c->L.psd, c->tb.gsf, c->tb.ux, c->d_ctab, in->rest_energy, in->n0, in->gam0,
                            c->d_cout, c->d_cdiag, c->stream));
  HIPCHK(hipMemcpyAsync(dNdp, c->d_cout, sizeof(double) * (size_t)(3 * ng * NM), hipMemcpyDeviceToHost, c->stream));
  unsigned long long hd[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(hd, c->d_cdiag, sizeof(hd), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (diag) { diag[0] = (int64_t)hd[0]; diag[1] = (int64_t)hd[1]; }
  c->have_cout_dndp = true;
  return 0;
}

int mcs_dndp_esc(mcs_ctx* c, const mcs_consumer_in* in, const double* gam_pf, double* dNdp, double* number, int64_t* diag) {
  MCS_ENTER(c);
  if (consumers_ready(c, in, "mcs_dndp_esc")) return 1;
  if (fold_replicas(c)) return 1;
  if (!in->mom_log_cgs || !in->mom_edge_cgs || !in->cos_edge || !gam_pf || !dNdp || !number) return fail("mcs_dndp_esc: null table");
  const int NM = c->P.num_psd_mom_bins + 2, NT = c->P.num_psd_tht_bins + 2;
  if (NM > MCS_PSD_MAX + 1 || NT > MCS_PSD_MAX + 1) return fail("mcs_dndp_esc: more PSD bins than an escape slab holds");
  if (!(gam_pf[0] >= 1) || !(gam_pf[1] >= 1) || !(in->gam0 >= 1)) return fail("mcs_dndp_esc: a Lorentz factor below 1");
  c->have_esc = false;
  const size_t n_out = (size_t)6 * NM + 6;
  if (reserve(c->d_esc_out, (long long)n_out) || reserve(c->d_esc_rows, 4LL * NT * NM) || reserve(c->d_esc_rowdiag, 8LL * NT) ||
      reserve(c->d_esc_diag, 4))
    return 1;
  std::vector<double> h((size_t)(2 * NM + NT));
  memcpy(h.data(), in->mom_log_cgs, sizeof(double) * NM);
  memcpy(h.data() + NM, in->mom_edge_cgs, sizeof(double) * NM);
  memcpy(h.data() + 2 * NM, in->cos_edge, sizeof(double) * NT);
  HIPCHK(hipMemcpyAsync(c->d_ctab, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(mcs_launch_dndp_esc(&c->P, c->d_T + c->L.esc_psd_up, c->d_ctab, in->rest_energy, gam_pf, in->gam0, c->d_esc_rows, c->d_esc_rowdiag,
                             c->d_esc_out, c->d_esc_diag, c->stream));
  std::vector<double> o(n_out);
  unsigned long long hd[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(o.data(), c->d_esc_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hd, c->d_esc_diag, sizeof(hd), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  memcpy(dNdp, o.data(), sizeof(double) * 6 * NM);
  memcpy(number, o.data() + 6 * NM, sizeof(double) * 6);
  if (diag) for (int q = 0; q < 4; ++q) diag[q] = (int64_t)hd[q];
  c->have_esc = true;
  return 0;
}

int mcs_angle_dist(mcs_ctx* c, const mcs_consumer_in* in, int n_win, const int32_t* l_lo, const int32_t* l_hi, double* dist, double* number,
                   double* moments) {
  MCS_ENTER(c);
  const std::string who = "mcs_angle_dist";
  if (!in || !l_lo || !l_hi) return fail(who + ": null argument");
  if (!c->have_grid) return fail(who + ": grid not set");
  const int nm = c->P.num_psd_mom_bins, nt = c->P.num_psd_tht_bins, ng = c->P.n_grid;
  const int NM = nm + 2, NT = nt + 2;
  if (NM > 208 || NT > 208) return fail(who + ": too many PSD bins");
  if (!in->pt_center || !in->cos_center || !in->cos_edge) return fail(who + ": null table");
  if (!(in->gam0 >= 1)) return fail(who + ": a Lorentz factor below 1");
  if (n_win < 1 || n_win > MCS_ANGLE_MAX_WINDOWS) return fail(who + ": n_win outside 1.." + std::to_string(MCS_ANGLE_MAX_WINDOWS));
  for (int m = 0; m < n_win; ++m)
    if (l_lo[m] < 0 || l_lo[m] >= l_hi[m] || l_hi[m] > nm + 1)
      return fail(who + ": window " + std::to_string(m) + " [" + std::to_string(l_lo[m]) + ", " + std::to_string(l_hi[m]) +
                  ") needs 0 <= l_lo < l_hi <= " + std::to_string(nm + 1));
  if (fold_replicas(c)) return 1;
  const long long rows = 3LL * ng * n_win, n_out = rows * (NT + 3);
  if (reserve(c->d_ang_out, 3LL * ng * MCS_ANGLE_MAX_WINDOWS * (NT + 3)) || reserve(c->d_ang_tab, NM + 2 * NT)) return 1;
  c->have_ang = false;
  std::vector<double> h((size_t)(NM + 2 * NT), 0.0);
  memcpy(h.data(), in->pt_center, sizeof(double) * (NM - 1));
  memcpy(h.data() + NM, in->cos_center, sizeof(double) * (NT - 1));
  memcpy(h.data() + NM + NT, in->cos_edge, sizeof(double) * NT);
  HIPCHK(hipMemcpyAsync(c->d_ang_tab, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(mcs_launch_angle_dist(&c->P, c->d_T + c->L.psd, c->d_T + c->L.therm_sf, c->d_I + MCS_I_NUM_CROSSINGS, c->tb.gsf, c->d_ang_tab,
                               in->rest_energy, in->gam0, in->therm_from_hist, n_win, l_lo, l_hi, c->d_ang_out, c->stream));
  std::vector<double> o((size_t)n_out);
  HIPCHK(hipMemcpyAsync(o.data(), c->d_ang_out, sizeof(double) * (size_t)n_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (dist) memcpy(dist, o.data(), sizeof(double) * (size_t)(rows * NT));
  const double* tail = o.data() + rows * NT;      // number | mean_mu | mean_mu2
  if (number) memcpy(number, tail, sizeof(double) * (size_t)rows);
  if (moments)
    for (long long r = 0; r < rows; ++r) { moments[2 * r] = tail[rows + r]; moments[2 * r + 1] = tail[2 * rows + r]; }
  c->ang_n_win = n_win;
  for (int m = 0; m < MCS_ANGLE_MAX_WINDOWS; ++m) { c->ang_lo[m] = m < n_win ? l_lo[m] : 0; c->ang_hi[m] = m < n_win ? l_hi[m] : 0; }
  c->have_ang = true;
  return 0;
}

int mcs_tcut_get_layout(const mcs_params* p, int n_tcuts, mcs_tcut_layout* out) {
  if (!p || !out) return fail("mcs_tcut_get_layout: null argument");
  if (n_tcuts < 1 || n_tcuts >= MCS_NA_C) return fail("mcs_tcut_get_layout: n_tcuts outside 1.." + std::to_string(MCS_NA_C - 1));
  const int64_t nm = p->num_psd_mom_bins + 2, nt = n_tcuts;
  out->row_n = nm; out->n_tcuts = nt;
  out->spectrum = 0; out->weight = nt * nm; out->number = nt * nm + nt; out->mean_log_p = nt * nm + 2 * nt;
  out->quantile = nt * nm + 3 * nt; out->index = nt * nm + (3 + MCS_TCUT_NQ) * nt;
  out->total = nt * nm + (3 + MCS_TCUT_NQ) * nt + MCS_TCUT_NQ;
  return 0;
}

int mcs_tcut_spectra(mcs_ctx* c, const mcs_consumer_in* in, double* out, int64_t* diag) {
  MCS_ENTER(c);
  const std::string who = "mcs_tcut_spectra";
  if (!in || !out) return fail(who + ": null argument");
  if (!c->P.do_tcuts) return fail(who + ": the context tracks no time cuts (do_tcuts)");
  if (!c->have_cuts) return fail(who + ": cuts not set (mcs_set_cuts)");
  if (c->tb.n_tcuts < 1) return fail(who + ": no time cut is set");
  if (!c->species_begun) return fail(who + ": no species has begun (mcs_begin_species takes the base)");
  if (!in->mom_log_cgs) return fail(who + ": null table");
  const int NM = c->P.num_psd_mom_bins + 2, nt = c->tb.n_tcuts;
  if (NM > MCS_PSD_MAX + 1) return fail(who + ": more PSD bins than a row of spectra_coupled holds");
  if (fold_replicas(c)) return 1;
  mcs_tcut_layout TL;
  if (mcs_tcut_get_layout(&c->P, nt, &TL)) return 1;
  c->have_tcut = false;
  if (reserve(c->d_tcut_out, TL.total) || reserve(c->d_ctab, NM) || reserve(c->d_tcut_rowneg, nt) || reserve(c->d_tcut_diag, 2)) return 1;
  HIPCHK(hipMemcpyAsync(c->d_ctab, in->mom_log_cgs, sizeof(double) * NM, hipMemcpyHostToDevice, c->stream));
  const long long nb = (long long)MCS_NA_C * (MCS_PSD_MAX + 1);
  HIPCHK(mcs_launch_tcut_spectra(&c->P, c->d_T + c->L.spectra_coupled + nb * (c->i_ion - 1), c->d_tcut_base,
                                 c->d_T + c->L.weight_coupled + (long long)MCS_NA_C * (c->i_ion - 1), c->d_ctab, c->tb.tcuts, nt, c->d_tcut_out,
                                 c->d_tcut_rowneg, c->d_tcut_diag, c->stream));
  std::vector<double> o((size_t)TL.total);
  unsigned long long hd[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(o.data(), c->d_tcut_out, sizeof(double) * o.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hd, c->d_tcut_diag, sizeof(hd), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  memcpy(out, o.data(), sizeof(double) * o.size());
  if (diag) { diag[0] = (int64_t)hd[0]; diag[1] = (int64_t)hd[1]; }
  c->tcut_n = nt;
  c->have_tcut = true;
  return 0;
}

int mcs_detector_get_layout(const mcs_params* p, int n_det, mcs_detector_layout* out) {
  if (!p || !out) return fail("mcs_detector_get_layout: null argument");
  if (n_det < 1 || n_det > p->n_grid) return fail("mcs_detector_get_layout: n_det outside 1..n_grid (" + std::to_string(p->n_grid) + ")");
  const int64_t nm = p->num_psd_mom_bins + 2, r = 2 * (int64_t)n_det;
  out->row_n = nm; out->n_det = n_det;
  out->spectrum = 0; out->dndp = r * nm; out->number = 2 * r * nm; out->mean_log_p = 2 * r * nm + r; out->quantile = 2 * r * nm + 2 * r;
  out->slope = 2 * r * nm + (2 + MCS_TCUT_NQ) * r; out->gradient = 2 * r * nm + (3 + MCS_TCUT_NQ) * r;
  out->total = 2 * r * nm + (3 + MCS_TCUT_NQ) * r + nm;
  return 0;
}

int mcs_detector_spectra(mcs_ctx* c, const mcs_consumer_in* in, int l_lo, int l_hi, double x_unit, double* out, int64_t* diag) {
  MCS_ENTER(c);
  const std::string who = "mcs_detector_spectra";
  if (!in || !out) return fail(who + ": null argument");
  if (!c->have_cuts) return fail(who + ": cuts not set (mcs_set_cuts)");
  if (c->tb.n_xspec < 1) return fail(who + ": no detector is set (n_xspec of mcs_set_cuts)");
  if (!c->species_begun) return fail(who + ": no species has begun (mcs_begin_species takes the base)");
  if (!c->have_det_base) return fail(who + ": no base (the cuts were set after the species began; mcs_begin_species takes the base)");
  if (!in->mom_log_cgs || !in->mom_edge_cgs) return fail(who + ": null table");
  const int nm = c->P.num_psd_mom_bins, NM = nm + 2, nd = c->tb.n_xspec;
  if (NM > MCS_PSD_MAX + 1) return fail(who + ": more PSD bins than a row of spectra_sf holds");
  if (l_lo < 0 || l_hi > nm + 1 || l_hi - l_lo < 3)
    return fail(who + ": window [" + std::to_string(l_lo) + ", " + std::to_string(l_hi) + ") needs 0 <= l_lo, l_hi <= " + std::to_string(nm + 1) +
                " and at least three bins");
  if (!std::isfinite(x_unit) || !(x_unit > 0)) return fail(who + ": x_unit must be finite and positive");
  for (int l = 0; l + 1 < NM; ++l)
    if (!(in->mom_edge_cgs[l + 1] > in->mom_edge_cgs[l])) return fail(who + ": mom_edge_cgs is not strictly ascending at entry " + std::to_string(l + 1));
  if (fold_replicas(c)) return 1;
  mcs_detector_layout DL;
  if (mcs_detector_get_layout(&c->P, nd, &DL)) return 1;
  c->have_det = false;
  if (reserve(c->d_det_out, DL.total) || reserve(c->d_det_tab, 2 * (long long)NM) || reserve(c->d_det_rowneg, 2 * (long long)nd) ||
      reserve(c->d_det_diag, 3))
    return 1;
  std::vector<double> h((size_t)2 * NM);
  memcpy(h.data(), in->mom_log_cgs, sizeof(double) * NM);
  memcpy(h.data() + NM, in->mom_edge_cgs, sizeof(double) * NM);
  HIPCHK(hipMemcpyAsync(c->d_det_tab, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(mcs_launch_detector_spectra(&c->P, c->d_T + c->L.spectra_sf, c->d_T + c->L.spectra_pf, c->d_det_base, c->d_det_tab, c->d_det_tab + NM,
                                     c->tb.x_spec, nd, l_lo, l_hi, x_unit, c->d_det_out, c->d_det_rowneg, c->d_det_diag, c->stream));
  std::vector<double> o((size_t)DL.total);
  unsigned long long hd[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(o.data(), c->d_det_out, sizeof(double) * o.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hd, c->d_det_diag, sizeof(hd), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));      // (also: h has been read)
  memcpy(out, o.data(), sizeof(double) * o.size());
  if (diag) for (int k = 0; k < 3; ++k) diag[k] = (int64_t)hd[k];
  c->det_n = nd; c->det_lo = l_lo; c->det_hi = l_hi; c->det_x_unit = x_unit;
  c->have_det = true;
  return 0;
}

int mcs_profile_get_layout(const mcs_params* p, mcs_profile_layout* out) {
  if (!p || !out) return fail("mcs_profile_get_layout: null argument");
  if (p->n_grid < 3) return fail("mcs_profile_get_layout: a profile has at least three zones");
  const int64_t n = p->n_grid;
  out->flux_px = 0; out->flux_en = n; out->gamma_ad = 2 * n; out->p_flux = 3 * n; out->p_used = 4 * n; out->ux_px = 5 * n; out->ux_en = 6 * n;
  out->ux_pred = 7 * n; out->ux_next = 8 * n; out->shift = 9 * n; out->scalars = MCS_PROFILE_ROWS * n;
  out->row_n = n; out->n_scalars = MCS_PROFILE_SCALARS; out->total = MCS_PROFILE_ROWS * n + MCS_PROFILE_SCALARS;
  return 0;
}

int mcs_profile_update(mcs_ctx* c, const mcs_profile_in* in, const double* pressures, double* out, int64_t* diag) {
  MCS_ENTER(c);
  const std::string who = "mcs_profile_update";
  if (!in || !out) return fail(who + ": null argument");
  if (!in->pxx_EM || !in->en_EM || !in->atan_x) return fail(who + ": null table");
  if (!c->have_grid) return fail(who + ": grid not set (mcs_set_grid)");
  if (!c->species_begun) return fail(who + ": no species has begun (the fluxes and running scalars are those of a species' transport)");
  const int n = c->P.n_grid;
  if (in->i_trans < 0 || in->i_trans > c->P.i_shock || in->i_trans > n)
    return fail(who + ": i_trans " + std::to_string(in->i_trans) + " outside 0..i_shock (" + std::to_string(c->P.i_shock) + ")");
  if (c->P.i_shock > n) return fail(who + ": i_shock beyond the grid");
  if (in->n_hist < 0 || in->n_hist > MCS_PROFILE_MAX_HIST)
    return fail(who + ": " + std::to_string(in->n_hist) + " earlier (q_px, q_en) pairs; at most " + std::to_string(MCS_PROFILE_MAX_HIST));
  if (!pressures && !c->have_cout_thermo)
    return fail(who + ": no pressures on the context (mcs_thermo_calcs has not run since the last mcs_begin_species or products sample) and none passed");
  mcs_profile_layout PL;
  if (mcs_profile_get_layout(&c->P, &PL)) return 1;
  if ((size_t)4 * n * sizeof(double) > (size_t)48 * 1024) return fail(who + ": n_grid too large for the kernel's rows (4 n_grid doubles of LDS, 48 KB)");
  if (fold_replicas(c)) return 1;
  c->have_prof = false;
  if (reserve(c->d_prof_out, PL.total) || reserve(c->d_prof_tab, 6 * (long long)n) || reserve(c->d_prof_diag, 3)) return 1;
  std::vector<double> h((size_t)(pressures ? 6 : 3) * n);
  memcpy(h.data(), in->pxx_EM, sizeof(double) * n);
  memcpy(h.data() + n, in->en_EM, sizeof(double) * n);
  memcpy(h.data() + 2 * (size_t)n, in->atan_x, sizeof(double) * n);
  if (pressures) memcpy(h.data() + 3 * (size_t)n, pressures, sizeof(double) * 3 * n);
  HIPCHK(hipMemcpyAsync(c->d_prof_tab, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  const double* pres = c->d_prof_tab + 3 * (size_t)n;
  if (!pressures) {
    pres = c->d_cout + (size_t)3 * n * (c->P.num_psd_mom_bins + 2);
  }
  HIPCHK(mcs_launch_profile_update(&c->P, in, c->d_T + c->L.pxx_flux, c->d_T + c->L.energy_flux, c->d_T + c->L.scalars, c->tb.ux, c->tb.gsf,
                                   c->tb.x_grid, pres, c->d_prof_tab, c->d_prof_out, c->d_prof_diag, c->stream));
  std::vector<double> o((size_t)PL.total);
  unsigned long long hd[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(o.data(), c->d_prof_out, sizeof(double) * o.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hd, c->d_prof_diag, sizeof(hd), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  memcpy(out, o.data(), sizeof(double) * o.size());
  if (diag) for (int k = 0; k < 3; ++k) diag[k] = (int64_t)hd[k];
  c->prof_in = *in;
  c->prof_in.pxx_EM = c->prof_in.en_EM = c->prof_in.atan_x = nullptr;
  c->prof_in.n_hist = 0;
  for (int k = 0; k < MCS_PROFILE_MAX_HIST; ++k) c->prof_in.hist_q_px[k] = c->prof_in.hist_q_en[k] = 0.0;
  c->have_prof = true;
  return 0;
}

int mcs_thermo_calcs(mcs_ctx* c, const mcs_consumer_in* in, double* P_par, double* P_perp, double* energy_density) {
  MCS_ENTER(c);
  if (consumers_ready(c, in, "mcs_thermo_calcs")) return 1;
  if (fold_replicas(c)) return 1;
  if (!in->cos_center || !in->pt_center || !in->zone_pop || !in->density_loc || !in->cold_pressure || !P_par || !P_perp || !energy_density)
    return fail("mcs_thermo_calcs: null table");
  c->have_cout_thermo = false;
  const int NM = c->P.num_psd_mom_bins + 2, NT = c->P.num_psd_tht_bins + 2, ng = c->P.n_grid;
  if (reserve(c->d_cscratch, (long long)NM * NT * ng)) return 1;
  std::vector<double> h((size_t)(NT + NM + 3 * ng), 0.0);
  memcpy(h.data(), in->cos_center, sizeof(double) * (NT - 1));
  memcpy(h.data() + NT, in->pt_center, sizeof(double) * (NM - 1));
  memcpy(h.data() + NT + NM, in->zone_pop, sizeof(double) * ng);
  memcpy(h.data() + NT + NM + ng, in->density_loc, sizeof(double) * ng);
  memcpy(h.data() + NT + NM + 2 * ng, in->cold_pressure, sizeof(double) * ng);
  HIPCHK(hipMemcpyAsync(c->d_ctab, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  double* out3 = c->d_cout + (size_t)3 * ng * NM;
  HIPCHK(mcs_launch_thermo(&c->P, c->d_T + c->L.psd, c->d_T + c->L.therm_pf, c->d_I + MCS_I_NUM_CROSSINGS, c->tb.gsf, c->tb.ux,
                           c->d_ctab, in->rest_energy, in->mc, in->n0, in->therm_from_hist, c->d_cscratch, out3, c->stream));
  std::vector<double> o((size_t)3 * ng);
  HIPCHK(hipMemcpyAsync(o.data(), out3, sizeof(double) * o.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  memcpy(P_par, o.data(), sizeof(double) * ng);
  memcpy(P_perp, o.data() + ng, sizeof(double) * ng);
  memcpy(energy_density, o.data() + 2 * ng, sizeof(double) * ng);
  c->have_cout_thermo = true;
  return 0;
}

int mcs_photon_synch(mcs_ctx* c, const double* dNdp_pf, const double* mom_edge_cgs, double mc, int n_photon, double emin_mev,
                     double bins_per_dec, double* energy_erg, double* emis) {
  MCS_ENTER(c);
  if (!dNdp_pf || !mom_edge_cgs || !emis) return fail("mcs_photon_synch: null argument");
  if (!c->have_grid) return fail("mcs_photon_synch: grid not set");
  if (n_photon < 1 || n_photon > 4096 || !(emin_mev > 0) || !(bins_per_dec > 0) || !(mc > 0)) return fail("mcs_photon_synch: bad arguments");
  const int NM = c->P.num_psd_mom_bins + 2, ng = c->P.n_grid;
  if (NM > 208) return fail("mcs_photon_synch: too many momentum bins");
  const size_t n_in = (size_t)ng * NM + NM, n_out = (size_t)ng * n_photon;
  if (reserve(c->d_stage, (long long)n_in + 4) || reserve(c->d_pemis[MCS_PHOTON_SYNCH], (long long)n_out)) return 1;
  c->pemis_n[MCS_PHOTON_SYNCH] = 0;
  double* d_in = c->d_stage; double* d_out = c->d_pemis[MCS_PHOTON_SYNCH];      // (kept for mcs_photon_observe)
  HIPCHK(hipMemcpyAsync(d_in, dNdp_pf, sizeof(double) * (size_t)ng * NM, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_in + (size_t)ng * NM, mom_edge_cgs, sizeof(double) * NM, hipMemcpyHostToDevice, c->stream));
  const double log_emin = std::log10(emin_mev * MCS_MEV_ERG_);
  HIPCHK(mcs_launch_photon_synch(d_in, d_in + (size_t)ng * NM, c->tb.btot, ng, NM, n_photon, log_emin, bins_per_dec, mc, d_out, c->stream));
  HIPCHK(hipMemcpyAsync(emis, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (energy_erg) for (int j = 0; j < n_photon; ++j) energy_erg[j] = std::pow(10.0, log_emin + j * (1.0 / bins_per_dec));
  c->pemis_n[MCS_PHOTON_SYNCH] = n_photon;
  return 0;
}

// The pion-decay fold (include/mcs_pion.h) over the plasma-frame dN/dp of a nucleus species.
int mcs_photon_pion(mcs_ctx* c, const double* dNdp_pf, const double* mom_edge_cgs, double mc, double aa, const double* target_density, double scaling,
                    int i_data, int n_photon, double emin_mev, double bins_per_dec, double* energy_erg, double* emis) {
  MCS_ENTER(c);
  if (!dNdp_pf || !mom_edge_cgs || !target_density || !emis) return fail("mcs_photon_pion: null argument");
  if (!c->have_grid) return fail("mcs_photon_pion: grid not set");
  if (n_photon < 1 || n_photon > 4096 || !(emin_mev > 0) || !(bins_per_dec > 0) || !(mc > 0) || !(aa >= 1) || !(scaling >= 0))
    return fail("mcs_photon_pion: bad arguments");
  if (i_data < 1 || i_data > 4) return fail("mcs_photon_pion: i_data must be between 1 and 4");        // pion_kafexhiu.jl:81-88
  const int NM = c->P.num_psd_mom_bins + 2, ng = c->P.n_grid;
  if (NM > 208) return fail("mcs_photon_pion: too many momentum bins");
  const size_t n_in = (size_t)ng * NM + NM + ng, n_out = (size_t)ng * n_photon;
  if (reserve(c->d_stage, (long long)n_in + 4) || reserve(c->d_pemis[MCS_PHOTON_PION], (long long)n_out)) return 1;
  c->pemis_n[MCS_PHOTON_PION] = 0;
  double* d_in = c->d_stage; double* d_out = c->d_pemis[MCS_PHOTON_PION];       // (kept for mcs_photon_observe)
  HIPCHK(hipMemcpyAsync(d_in, dNdp_pf, sizeof(double) * (size_t)ng * NM, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_in + (size_t)ng * NM, mom_edge_cgs, sizeof(double) * NM, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_in + (size_t)ng * NM + NM, target_density, sizeof(double) * ng, hipMemcpyHostToDevice, c->stream));
  const double log_emin = std::log10(emin_mev * MCS_MEV_ERG_);
  HIPCHK(mcs_launch_photon_pion(d_in, d_in + (size_t)ng * NM, d_in + (size_t)ng * NM + NM, ng, NM, n_photon, log_emin, bins_per_dec, mc, aa, scaling,
                                i_data, d_out, c->stream));
  HIPCHK(hipMemcpyAsync(emis, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (energy_erg) for (int j = 0; j < n_photon; ++j) energy_erg[j] = std::pow(10.0, log_emin + j * (1.0 / bins_per_dec));
  c->pemis_n[MCS_PHOTON_PION] = n_photon;
  return 0;
}

// get_dNdp_2D (src/particle_counter.jl:343-627) on the resident psd / therm_sf / num_crossings: the d2N/dp dcos of every zone in
// the frame that moves with (gam_x, beta_x) against the shock frame (the ISM frame: gam0, beta0).  The result stays on the device
// for mcs_photon_ic; d2N (host, [n_grid][ntht+2][nmom+2], momentum fastest) may be null.
int mcs_dndp_2d(mcs_ctx* c, const mcs_consumer_in* in, double gam_x, double beta_x, double* d2N) {
  MCS_ENTER(c);
  if (consumers_ready(c, in, "mcs_dndp_2d")) return 1;
  if (fold_replicas(c)) return 1;
  if (!in->mom_edge_cgs || !in->cos_center || !in->pt_center || !in->zone_pop) return fail("mcs_dndp_2d: null table");
  if (!(gam_x >= 1) || !(beta_x >= 0 && beta_x < 1)) return fail("mcs_dndp_2d: bad frame");
  const int NM = c->P.num_psd_mom_bins + 2, NT = c->P.num_psd_tht_bins + 2, ng = c->P.n_grid;
  const size_t slab = (size_t)NM * NT * ng;
  if (reserve(c->d_cscratch, (long long)slab) || reserve(c->d_c2d, (long long)slab)) return 1;
  std::vector<double> h((size_t)(2 * NM + NT + ng), 0.0);
  memcpy(h.data(), in->mom_edge_cgs, sizeof(double) * NM);
  memcpy(h.data() + NM, in->cos_center, sizeof(double) * (NT - 1));
  memcpy(h.data() + NM + NT, in->pt_center, sizeof(double) * (NM - 1));
  memcpy(h.data() + 2 * NM + NT, in->zone_pop, sizeof(double) * ng);
  HIPCHK(hipMemcpyAsync(c->d_ctab, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(mcs_launch_dndp_2d(&c->P, c->d_T + c->L.psd, c->d_T + c->L.therm_sf, c->d_I + MCS_I_NUM_CROSSINGS, c->d_ctab, in->rest_energy, in->n0,
                            in->therm_from_hist, gam_x, beta_x, c->d_cscratch, c->d_c2d, c->stream));
  if (d2N) HIPCHK(hipMemcpyAsync(d2N, c->d_c2d, sizeof(double) * slab, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->have_c2d = true;
  return 0;
}

// The inverse-Compton fold (include/mcs_ic.h) over the d2N/dp dcos the last mcs_dndp_2d left on the device.
int mcs_photon_ic(mcs_ctx* c, const double* mom_edge_cgs, double mc_e, int j_max, int n_nu, const double* alpha_in, const double* n_in, int n_photon,
                  double emin_mev, double bins_per_dec, double beam_area, double* energy_erg, double* emis) {
  MCS_ENTER(c);
  if (!mom_edge_cgs || !alpha_in || !n_in || !emis) return fail("mcs_photon_ic: null argument");
  if (!c->have_c2d) return fail("mcs_photon_ic: no mcs_dndp_2d result on the device");
  const int NM = c->P.num_psd_mom_bins + 2, NT = c->P.num_psd_tht_bins + 2, ng = c->P.n_grid;
  if (NM > 208) return fail("mcs_photon_ic: too many momentum bins");
  if (n_photon < 1 || n_photon > 4096 || n_nu < 1 || n_nu > MCS_IC_NNU || j_max < 0 || j_max > NT - 2 || !(emin_mev > 0) || !(bins_per_dec > 0) ||
      !(mc_e > 0) || !(beam_area > 0))
    return fail("mcs_photon_ic: bad arguments");
  const size_t n_in_w = (size_t)NM + 2 * (size_t)n_nu, n_out = (size_t)ng * n_photon;
  if (reserve(c->d_stage, (long long)n_in_w + 4) || reserve(c->d_pemis[MCS_PHOTON_IC], (long long)n_out)) return 1;
  c->pemis_n[MCS_PHOTON_IC] = 0;
  double* d_in = c->d_stage; double* d_out = c->d_pemis[MCS_PHOTON_IC];         // (kept for mcs_photon_observe)
  HIPCHK(hipMemcpyAsync(d_in, mom_edge_cgs, sizeof(double) * NM, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_in + NM, alpha_in, sizeof(double) * n_nu, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_in + NM + n_nu, n_in, sizeof(double) * n_nu, hipMemcpyHostToDevice, c->stream));
  const double log_min_rm = std::log10(emin_mev * MCS_MEV_ERG_ / (MCS_ME * MCS_C * MCS_C));
  HIPCHK(mcs_launch_photon_ic(c->d_c2d, d_in, d_in + NM, ng, NM, NT, j_max, n_nu, n_photon, log_min_rm, bins_per_dec, mc_e, beam_area, d_out, c->stream));
  HIPCHK(hipMemcpyAsync(emis, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (energy_erg) for (int k = 0; k < n_photon; ++k) energy_erg[k] = mcs_ic_alpha_out(log_min_rm, bins_per_dec, k) * (MCS_ME * MCS_C * MCS_C);
  c->pemis_n[MCS_PHOTON_IC] = n_photon;
  return 0;
}

// K9: the observed shell spectra of one emission process (include/mcs.h has the definition and the refusals).  Everything is checked
// before anything is queued or changed.
int mcs_photon_observe(mcs_ctx* c, int process, int n_photon, const double* emis, const double* energy_div, const double* energy_grid, double area,
                       double dlog, double last_mid_ratio, const double* cos_edge, const double* gam_ef, const double* beta_ef, const double* gam3_ef,
                       int n_shells, const int64_t* shell_ends, double* out) {
  MCS_ENTER(c);
  const std::string who = "mcs_photon_observe: ";
  if (process != MCS_PHOTON_SYNCH && process != MCS_PHOTON_IC && process != MCS_PHOTON_PION) return fail(who + "process must be MCS_PHOTON_SYNCH, _IC or _PION");
  if (!energy_div || !energy_grid || !cos_edge || !gam_ef || !beta_ef || !gam3_ef || !shell_ends) return fail(who + "null table");
  if (n_photon < 3 || n_photon > 256) return fail(who + format("n_photon = %d; the kernel holds a zone's tables in LDS and takes 3..256 energies", n_photon));
  if (n_shells < 1 || n_shells > 4096) return fail(who + "n_shells must be 1..4096");
  if (!emis && c->pemis_n[process] == 0)
    return fail(who + "no emission of this process on the context (its fold has not run since the last mcs_begin_species, tally write or photons sample)");
  if (!emis && c->pemis_n[process] != n_photon)
    return fail(who + format("the fold of this process left %d energies on the context, the call names %d", c->pemis_n[process], n_photon));
  const int ng = c->P.n_grid, n = n_photon - 1;
  const bool shifted = process != MCS_PHOTON_IC;
  if (!(dlog > 0) || !std::isfinite(dlog)) return fail(who + "dlog must be positive and finite");
  if (!(last_mid_ratio >= 1) || !std::isfinite(last_mid_ratio)) return fail(who + "last_mid_ratio must be finite and at least 1");
  if (shifted && (!(area > 0) || !std::isfinite(area))) return fail(who + "area must be positive and finite");
  for (int j = 0; j < n_photon; ++j) {
    if (!(energy_div[j] > 0) || !std::isfinite(energy_div[j]) || !(energy_grid[j] > 0) || !std::isfinite(energy_grid[j]))
      return fail(who + format("energy %d is not positive and finite", j));
    if (j > 0 && energy_grid[j] < energy_grid[j - 1]) return fail(who + format("energy_grid decreases at entry %d", j));
  }
  for (int l = 0; l <= 180; ++l)
    if (!std::isfinite(cos_edge[l]) || cos_edge[l] < -1 || cos_edge[l] > 1) return fail(who + format("cos_edge[%d] is not a cosine", l));
  for (int z = 0; z < ng; ++z) {
    if (!(gam_ef[z] > 0) || !std::isfinite(gam_ef[z]) || !std::isfinite(gam3_ef[z])) return fail(who + format("gam_ef / gam3_ef of zone %d is not positive and finite", z + 1));
    if (!(beta_ef[z] >= 0 && beta_ef[z] < 1)) return fail(who + format("beta_ef of zone %d is outside [0, 1)", z + 1));
  }
  for (int s = 0; s <= n_shells; ++s)
    if (shell_ends[s] < 0 || shell_ends[s] > (int64_t)ng + 1) return fail(who + format("shell_ends[%d] is outside 0 .. n_grid + 1", s));
  const size_t n_tab = 2 * (size_t)n_photon + 181 + 3 * (size_t)ng + (size_t)n_shells + 1, n_out = ((size_t)n_shells + 1) * n;
  if (reserve(c->d_ptab, (long long)n_tab) || reserve(c->d_pnb, (long long)ng * n) || (emis && reserve(c->d_stage, (long long)ng * n_photon))) return 1;
  // (the kept result last: growing its buffer drops it, so its flag goes first; every other allocation has succeeded by now)
  if (c->d_pobs[process].cap() < (long long)n_out) c->pobs_n[process] = 0;
  if (reserve(c->d_pobs[process], (long long)n_out)) return 1;
  std::vector<double> h(n_tab);
  double* q = h.data();
  memcpy(q, energy_div, sizeof(double) * n_photon); q += n_photon;
  memcpy(q, energy_grid, sizeof(double) * n_photon); q += n_photon;
  memcpy(q, cos_edge, sizeof(double) * 181); q += 181;
  memcpy(q, gam_ef, sizeof(double) * ng); q += ng;
  memcpy(q, beta_ef, sizeof(double) * ng); q += ng;
  memcpy(q, gam3_ef, sizeof(double) * ng); q += ng;
  for (int s = 0; s <= n_shells; ++s) q[s] = (double)shell_ends[s];
  c->pobs_n[process] = 0;
  HIPCHK(hipMemcpyAsync(c->d_ptab, h.data(), sizeof(double) * n_tab, hipMemcpyHostToDevice, c->stream));
  const double* d_emis = c->d_pemis[process];
  if (emis) {
    HIPCHK(hipMemcpyAsync(c->d_stage, emis, sizeof(double) * (size_t)ng * n_photon, hipMemcpyHostToDevice, c->stream));
    d_emis = c->d_stage;
  }
  HIPCHK(mcs_launch_photon_observe(d_emis, c->d_ptab, process, ng, n_photon, area, dlog, last_mid_ratio, n_shells, c->d_pnb, c->d_pobs[process], c->stream));
  if (out) HIPCHK(hipMemcpyAsync(out, c->d_pobs[process], sizeof(double) * n_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->pobs_n[process] = n; c->pobs_shells[process] = n_shells;
  return 0;
}

// ---- the view of a context that mcs_ensemble.hip (K8) works through (mcs_ctx_view.h) ----
int mcs_ctx_view_get(mcs_ctx* c, McsCtxView* out) {
  MCS_ENTER(c);
  if (fold_replicas(c)) return 1;
  *out = McsCtxView{c->device, c->stream, c->d_T, c->d_I, c->P, c->L, c->d_cout, c->have_cout_dndp, c->have_cout_thermo, {}, {}, {},
                    c->d_esc_out, c->have_esc, c->d_ang_out, c->have_ang, c->ang_n_win, {}, {},
                    c->d_tcut_out, c->have_tcut, c->tcut_n, c->d_prof_out, c->have_prof, c->prof_in,
                    c->d_det_out, c->have_det, c->det_n, c->det_lo, c->det_hi, c->det_x_unit, c->h_x_spec.data()};
  out->prof_in.pxx_EM = out->prof_in.en_EM = out->prof_in.atan_x = nullptr;      // (the caller's tables are not kept)
  for (int m = 0; m < MCS_ANGLE_MAX_WINDOWS; ++m) { out->ang_lo[m] = c->ang_lo[m]; out->ang_hi[m] = c->ang_hi[m]; }
  for (int p = 0; p < 3; ++p) { out->pobs[p] = c->d_pobs[p]; out->pobs_n[p] = c->pobs_n[p]; out->pobs_shells[p] = c->pobs_shells[p]; }
  return 0;
}
void mcs_ctx_view_tallies_written(mcs_ctx* c) { c->have_c2d = false; c->have_ang = false; c->have_prof = false; c->photon_flags_clear(); }
void mcs_ctx_view_products_taken(mcs_ctx* c) { c->have_cout_dndp = c->have_cout_thermo = false; }
void mcs_ctx_view_photons_taken(mcs_ctx* c) { c->photon_flags_clear(); }
void mcs_ctx_view_escape_taken(mcs_ctx* c) { c->have_esc = false; }
void mcs_ctx_view_angles_taken(mcs_ctx* c) { c->have_ang = false; }
void mcs_ctx_view_tcuts_taken(mcs_ctx* c) { c->have_tcut = false; }
void mcs_ctx_view_profile_taken(mcs_ctx* c) { c->have_prof = false; }
void mcs_ctx_view_detectors_taken(mcs_ctx* c) { c->have_det = false; }
int mcs_ctx_view_fail(const char* msg) { return fail(msg); }

}  // extern "C"

/* mcs.h -- C ABI of the MI355X-native per-particle transport path.
 *
 * Drop-in boundary: the `for i_prt in 1:n_pts_use` loop of the reference,
 * /root/reference/src/main_loops.jl:228-292 (particle_loop + particle_finish!),
 * batched into ONE call per (iteration, species, pcut).  The reference has no
 * FFI for this path (it is pure Julia); INTEGRATION.md shows the `ccall` shim a
 * maintainer would put in place of that loop.  All quantities are fp64 cgs, as
 * in the reference after `ustrip`.
 *
 * Index conventions
 *   grid tables : n_grid+2 entries, C index == Julia OffsetVector index 0:n_grid+1
 *   zones       : Julia 1:n_grid  ->  C slot (i-1)
 *   PSD bins    : 0-based in both
 *   pcut/tcut/ion/iter numbers are passed 1-based (they enter the RNG seed formula
 *   of src/particle_loop.jl:35-40 and index pₓ_esc_feb[i_ion, i_iter]).
 *
 * Error model: every entry point returns 0 on success, non-zero otherwise;
 * mcs_last_error() returns the message (the reference's `error(...)` sites:
 * src/particle_finish.jl:104, src/all_flux.jl:73-75, src/scattering.jl:52-53,
 * src/prob_return.jl:134).  Warn-paths of the reference (@warn) are counters.
 *
 * Threading: one context per GPU; calls on one context must be serialised by
 * the caller (the reference is single-threaded and not re-entrant).
 */
#ifndef MCS_H
#define MCS_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCS_ABI_VERSION 3

/* ---- physical constants (cgs).  The reference takes them from Unitful /
 * UnitfulGaussian / PhysicalConstants.CODATA2018 (src/MonteCarloScattering.jl:10-12,
 * src/constants.jl:3); Project.toml has no lockfile, these are the CODATA-2018
 * values those packages carry. */
#define MCS_MP     1.67262192369e-24      /* proton mass [g] */
#define MCS_ME     9.1093837015e-28       /* electron mass [g] */
#define MCS_C      2.99792458e10          /* speed of light [cm/s] */
#define MCS_QCGS   4.803204712570263e-10  /* elementary charge [esu] = 1.602176634e-19 C * c/10 */
#define MCS_KB     1.380649e-16           /* Boltzmann [erg/K] */
#define MCS_SIGMA_T 6.6524587321e-25      /* Thomson cross-section [cm^2] */
#define MCS_B_CMB0 3.27e-6                /* src/constants.jl:10 [G] */
/* src/constants.jl:30: rad_loss_fac = 4/3 c sigma_T / (c^3 me^2 8 pi)  [s^2/g^2] */
#define MCS_RAD_LOSS_FAC ((4.0/3.0) * MCS_C * MCS_SIGMA_T / (MCS_C*MCS_C*MCS_C * MCS_ME*MCS_ME * 8.0 * 3.141592653589793))

/* ---- compile-time constants of the path (src/parameters.jl, src/all_flux.jl:4,
 * src/particle_finish.jl:5, src/particle_loop.jl:162, src/prob_return.jl:229) */
#define MCS_PSD_MAX      200     /* parameters.jl:18 */
#define MCS_NA_C         100     /* parameters.jl:11 */
#define MCS_E_REL_PT     0.005   /* parameters.jl:32 */
#define MCS_SPIKE_AWAY   1000.0  /* all_flux.jl:4, particle_finish.jl:5 */
#define MCS_HELIX_CAP    10000   /* particle_loop.jl:162 */
#define MCS_RETRO_XN_PER 10.0    /* prob_return.jl:229 */
/* The reference's retro_time loop is uncapped (prob_return.jl:257); a walk that never comes back to the
 * PRP would hang the GPU.  After this many inner steps of ONE walk the particle ends with i_reason 3
 * and MCS_IC_RETRO_CAP is bumped (identically in the oracle).  mcs_set_retro_cap overrides it (tests). */
#define MCS_RETRO_CAP    10000000
#define MCS_FLOOR        1.0e-99 /* particle_loop.jl:315-317, ion_init.jl:11-13 */

/* i_reason codes (src/particle_loop.jl:138, src/particle_finish.jl:81-105) */
#define MCS_REASON_SAVED      0  /* reached pcut, kept for next pcut (l_save) */
#define MCS_REASON_DOWNSTREAM 1
#define MCS_REASON_UPSTREAM   2  /* pmax or upstream FEB */
#define MCS_REASON_AGE        3
#define MCS_REASON_ZERO_E     4

/* Scalars and flags handed to particle_loop at src/main_loops.jl:236-264. */
typedef struct mcs_params {
  int32_t abi_version;          /* = MCS_ABI_VERSION */
  int32_t n_ions, n_grid, n_itrs;
  int64_t n_pts_max;            /* MonteCarloScattering.jl:488; enters the seed formula */
  int32_t i_grid_feb, i_shock;  /* MonteCarloScattering.jl:414,478 (Julia zone numbers) */
  int32_t num_psd_mom_bins, num_psd_tht_bins;
  int32_t psd_bins_per_dec_mom, psd_bins_per_dec_tht;
  double  psd_cos_fine, psd_dcos, psd_tht_min, psd_mom_min;
  double  gam0, beta0, u0, u2, bmag2;
  double  pe_crit, game_crit, eta_mfp;
  double  energy_transfer_frac;
  double  feb_upstream, feb_downstream, x_grid_stop;
  double  B_CMBz, age_max;
  double  xn_per_fine, xn_per_coarse;
  int32_t use_custom_epsB, do_rad_losses, do_retro, do_tcuts;
  int32_t dont_DSA, dont_scatter, use_custom_frg;
  int32_t track_thermal;        /* A9: bin non-injected crossings on the fly */
  int32_t state_fp32;           /* 0: fp64 particle state (the reference's precision).  1: the fp32-state variant of K1 --
                                 * state and per-step arithmetic in fp32 in normalised units (p / m_p c, x / rg0, t c / rg0),
                                 * population in HBM and all tallies fp64 (BASELINE config[4]; DESIGN.md "fp32-state variant") */
} mcs_params;

/* One particle population, struct-of-arrays, host side; element types follow the
 * Julia arrays at src/MonteCarloScattering.jl:556-585 (Float64 / Int / Bool). */
typedef struct mcs_soa {
  double  *weight, *ptot_pf, *pb_pf, *x_PT_cm, *xn_per, *prp_x_cm, *acctime_sec, *phi_rad;
  int64_t *grid, *tcut;
  uint8_t *downstream, *inj;
} mcs_soa;

/* Offsets (in doubles) of every fp64 tally inside ONE flat buffer, so that a
 * multi-GPU run merges all of them with a single sum-all-reduce.  Shapes and
 * reset cadence: SURVEY.md section 8(a) "Tally arrays". */
typedef struct mcs_layout {
  int64_t psd;            /* [nmom+2][ntht+2][n_grid], momentum fastest (MonteCarloScattering.jl:519) */
  int64_t therm_sf;       /* same shape as psd: non-injected crossings, shock frame   (A9) */
  int64_t therm_pf;       /* same shape as psd: non-injected crossings, plasma frame of zone i (A9) */
  int64_t esc_psd_up;     /* [201][201], ip fastest (MonteCarloScattering.jl:537) */
  int64_t esc_psd_down;   /* [201][201] */
  int64_t pxx_flux, pxz_flux, energy_flux;    /* [n_grid] */
  int64_t esc_flux;       /* [n_ions] */
  int64_t px_esc_feb, energy_esc_feb;         /* [n_ions][n_itrs], ion fastest */
  int64_t esc_energy_eff, esc_num_eff;        /* [201][n_ions], ip fastest */
  int64_t weight_coupled;                     /* [100][n_ions] */
  int64_t spectra_coupled;                    /* [201][100][n_ions] */
  int64_t spectra_sf, spectra_pf;             /* [201][n_grid] (2nd index = x_spec number) */
  int64_t energy_transfer_pool, energy_recv_pool; /* [n_grid] */
  int64_t scalars;        /* [4]: sumP_downstream, sumKEdensity_downstream, px_esc_upstream, energy_esc_upstream */
  int64_t total;          /* number of doubles */
  int64_t psd_stride_tht, psd_stride_zone;    /* nmom+2, (nmom+2)*(ntht+2) */
} mcs_layout;

/* int64 tallies / diagnostics, one flat buffer */
enum {
  MCS_I_NUM_CROSSINGS = 0,      /* [n_grid] src/all_flux.jl:254 */
  /* the following are offsets from n_grid */
  MCS_IC_STEPS_HELIX = 0,       /* passes of src/particle_loop.jl:154-499 */
  MCS_IC_STEPS_RETRO,           /* passes of src/prob_return.jl:257-338 */
  MCS_IC_HELIX_CAP,             /* particle_loop.jl:162 hits */
  MCS_IC_PPERP_CLAMP,           /* particle_loop.jl:640-644 hits */
  MCS_IC_PSP_CLAMP,             /* transformers.jl:562-568,592-598 hits */
  MCS_IC_MOMBIN_CLAMP,          /* get_psd_bins.jl:29-36 hits */
  MCS_IC_REASON0, MCS_IC_REASON1, MCS_IC_REASON2, MCS_IC_REASON3, MCS_IC_REASON4,
  MCS_IC_TCUT_OVERRUN,          /* tcut index past n_tcuts (reference would throw BoundsError) */
  MCS_IC_RNG_DRAWS,
  MCS_IC_ZONE_FAIL,              /* src/all_flux.jl:73-75 would throw */
  MCS_IC_RETRO_CAP,              /* retro_time walks ended by MCS_RETRO_CAP (the reference would never return) */
  MCS_IC_COUNT
};

static inline int64_t mcs_i64_total(const mcs_params* p) { return (int64_t)p->n_grid + MCS_IC_COUNT; }

/* Two kinds of sections, by what happens to them between the species of an iteration:
 *
 *   buffer  words                                  kind            sections
 *   fp64    [psd, esc_flux)                        per-species     psd, therm_sf, therm_pf, esc_psd_up, esc_psd_down,
 *                                                                  pxx_flux, pxz_flux, energy_flux
 *   fp64    [energy_recv_pool, scalars)            per-species     energy_recv_pool
 *   int64   [0, n_grid)                            per-species     num_crossings
 *   fp64    [esc_flux, energy_recv_pool)           running sum     esc_flux, px_esc_feb, energy_esc_feb, esc_energy_eff,
 *                                                                  esc_num_eff, weight_coupled, spectra_coupled, spectra_sf,
 *                                                                  spectra_pf, energy_transfer_pool
 *   fp64    [scalars, total)                       running sum     scalars
 *   int64   [n_grid, n_grid + MCS_IC_COUNT)        running sum     the event counters
 *
 * mcs_begin_species resets or sets the per-species sections; every later species adds to the running sums.
 * mcs_accumulate_tallies moves the running sums of one context into another's. */
static inline void mcs_tally_layout(const mcs_params* p, mcs_layout* L) {
  const int64_t nm = p->num_psd_mom_bins + 2, nt = p->num_psd_tht_bins + 2, ng = p->n_grid;
  const int64_t pm = MCS_PSD_MAX + 1;
  int64_t o = 0;
  L->psd_stride_tht = nm; L->psd_stride_zone = nm * nt;
  L->psd = o;            o += nm * nt * ng;
  L->therm_sf = o;       o += nm * nt * ng;
  L->therm_pf = o;       o += nm * nt * ng;
  L->esc_psd_up = o;     o += pm * pm;
  L->esc_psd_down = o;   o += pm * pm;
  L->pxx_flux = o;       o += ng;
  L->pxz_flux = o;       o += ng;
  L->energy_flux = o;    o += ng;
  L->esc_flux = o;       o += p->n_ions;
  L->px_esc_feb = o;     o += (int64_t)p->n_ions * p->n_itrs;
  L->energy_esc_feb = o; o += (int64_t)p->n_ions * p->n_itrs;
  L->esc_energy_eff = o; o += pm * p->n_ions;
  L->esc_num_eff = o;    o += pm * p->n_ions;
  L->weight_coupled = o; o += (int64_t)MCS_NA_C * p->n_ions;
  L->spectra_coupled = o; o += pm * MCS_NA_C * p->n_ions;
  L->spectra_sf = o;     o += pm * ng;
  L->spectra_pf = o;     o += pm * ng;
  L->energy_transfer_pool = o; o += ng;
  L->energy_recv_pool = o;     o += ng;
  L->scalars = o;        o += 4;
  L->total = o;
}

/* ---- run options of a context ------------------------------------------------
 * Every switch of the transport path is an option of the context, with a key of this enum.  A new context takes the built-in
 * default of each, then -- unless it was created with use_env = 0 -- what the option's environment variable says, then what the
 * caller's list says (mcs_create_with_options).  The variables are read once, at creation; they are the DEFAULT of a context that
 * was not told otherwise (a host that must not depend on its shell passes use_env = 0).  mcs_get_option reads an option back,
 * mcs_set_option changes it where "when" allows, mcs_option_describe hands out this table (csrc/mcs_options.h holds it).
 *
 * key                      variable                  default    range        when  applies   meaning
 * MCS_OPT_FORCE_GENERAL    MCS_FORCE_GENERAL [on]    0          0..1         L     any       1: always the general transport kernel
 *                                                                                            (mcs_last_kernel 0), never a specialisation
 * MCS_OPT_K1_WS            MCS_K1_WS [tri]           2          0..2         L     any       the wave-specialised kernels (mcs_last_kernel
 *                                                                                            7 / 8) where they apply: 0 never, 1 always,
 *                                                                                            2 for populations of >= WS_AUTO_MIN particles
 * MCS_OPT_WS_AUTO_MIN      MCS_WS_AUTO_MIN [int]     6000000    0..INT64_MAX L     any       that population size
 * MCS_OPT_TAIL_MERGE       MCS_TAIL_MERGE [not off]  1          0..1         L     any       0: sparse waves are not consolidated
 * MCS_OPT_PARK             MCS_PARK [not off]        1          0..1         L     any       0: lanes that need the rare code run it at
 *                                                                                            once instead of waiting for company
 * MCS_OPT_TAIL_RING        MCS_TAIL_RING [not off]   1          0..1         L     any       0: no precomputed scatter draws in the tail
 *                                                                                            (and no tail loop)
 * MCS_OPT_TAIL_LOOP        MCS_TAIL_LOOP [int]       12         0..32        L     any       live lanes at or below which an exhausted
 *                                                                                            wave runs the tight tail loop (0: never)
 * MCS_OPT_REFILL_MIN       MCS_REFILL_MIN [int]      12         1..48        L     any       idle lanes at which a wave claims new work
 * MCS_OPT_DEFER_K          MCS_DEFER_K [int]         8          1..40        L     any       lanes a wave collects before it runs their
 *                                                                                            rare code (1: no deferral); a launch uses
 *                                                                                            min(DEFER_K, 64 - REFILL_MIN)
 * MCS_OPT_TAIL_BUDGET      MCS_TAIL_BUDGET [int]     0          0..2^24      L     fp64 > 0  the sliced tail of mcs_set_tail_slicing
 *                                                                                            (trips; 0 = one launch per pcut)
 * MCS_OPT_PIPE_SIDE_CUS    MCS_PIPE_SIDE_CUS [int]   12         0..128       P     any       compute units the side stream of
 *                                                                                            mcs_run_pcuts_pipelined has to itself (0: no
 *                                                                                            CU masks)
 * MCS_OPT_TALLY_REPLICAS   MCS_TALLY_REPLICAS_OFF    1          0..1         C     any       0: tally straight into the tally buffer, no
 *                          [on, inverted]                                                    private copies (they cost device memory: 16
 *                                                                                            times the tally buffer)
 * MCS_OPT_F32_LOOP         MCS_F32_LOOP [on]         0          0..1         L     fp32      1: the fp32-state kernel as a plain per-lane
 *                                                                                            loop (mcs_last_kernel 4)
 * MCS_OPT_F32_EXACT        MCS_F32_EXACT [on]        0          0..1         L     fp32      1: that loop with the exact fp32 primitives
 *                                                                                            (mcs_last_kernel 9; wins over F32_LOOP)
 *
 * How a variable is read: [on] 1 iff its first character is '1'; [not off] 0 iff its first character is '0'; [tri] '1' -> 1,
 * '0' -> 0, anything else -> 2; [int] the number, if it lies inside the range.  An unset variable, or an [int] outside the range,
 * leaves the built-in default, silently.  (MCS_TAIL_BUDGET once took numbers up to INT_MAX; it now has the range of the option.)
 * A variable is not asked whether it applies: MCS_F32_EXACT=1 is carried by a fp64 context without effect, as it always was.
 * when: L -- between launches: a change holds for the launches queued by calls made after it; P -- until the context's first
 * mcs_run_pcuts_pipelined (the masked streams are made once); C -- at creation only (it decides an allocation).
 * applies: fp32 -- the key is refused for a context with fp64 particle state (mcs_params.state_fp32 = 0); fp64 > 0 -- a value
 * above 0 is refused for a context with fp32 particle state.
 * Not options, because no property of a context: MCS_PIPE_DEBUG (a trace on stderr) and MCS_HIP_LIB (the file the Python package
 * loads).  The Python driver's own four (MCS_FUSED_PCUTS, MCS_FUSED_CHUNK, MCS_LONG_DRAWS, MCS_LONG_IMULT_MAX) are the defaults of
 * arguments of driver.run. */
enum mcs_option {
  MCS_OPT_FORCE_GENERAL = 0, MCS_OPT_K1_WS, MCS_OPT_WS_AUTO_MIN, MCS_OPT_TAIL_MERGE, MCS_OPT_PARK, MCS_OPT_TAIL_RING,
  MCS_OPT_TAIL_LOOP, MCS_OPT_REFILL_MIN, MCS_OPT_DEFER_K, MCS_OPT_TAIL_BUDGET, MCS_OPT_PIPE_SIDE_CUS, MCS_OPT_TALLY_REPLICAS,
  MCS_OPT_F32_LOOP, MCS_OPT_F32_EXACT,
  MCS_OPT_COUNT
};
enum mcs_option_when { MCS_WHEN_BETWEEN_LAUNCHES = 0, MCS_WHEN_BEFORE_PIPELINED_RUN = 1, MCS_WHEN_CREATION = 2 };
enum mcs_option_applies { MCS_APPLIES_ANY = 0, MCS_APPLIES_FP64_IF_POSITIVE = 1, MCS_APPLIES_FP32 = 2 };
/* One row of the table; name and env point to static strings of the library. */
typedef struct mcs_option_desc {
  int32_t key, when, applies, reserved;
  int64_t min, max, dflt;
  const char* name;   /* lower case, the key without MCS_OPT_: "defer_k" */
  const char* env;    /* the variable that seeds the default */
} mcs_option_desc;

typedef struct mcs_ctx mcs_ctx;

/* ---- lifecycle ---------------------------------------------------------- */
int         mcs_abi_version(void);
/* non-inline export of mcs_tally_layout for FFI callers (Julia ccall, ctypes) */
int         mcs_get_layout(const mcs_params* p, mcs_layout* out);
const char* mcs_last_error(void);
/* device: HIP device ordinal; stream: hipStream_t (NULL = default stream). */
int mcs_create(const mcs_params* p, int device, void* stream, mcs_ctx** out);
/* The same with run options (enum mcs_option): n_options pairs keys[i], values[i]; use_env = 0: no environment variable is read.
 * Initial values: built-in default < environment (use_env != 0) < the list, in its order.  A pair the table does not allow --
 * unknown key, value outside the range, a fp32 key for a fp64 context, MCS_OPT_TAIL_BUDGET > 0 for a fp32 one -- fails the call
 * with a message that names the option and its range, BEFORE the device is touched (the same on a machine without a GPU).
 * mcs_create(p, device, stream, out) is mcs_create_with_options(p, device, stream, NULL, NULL, 0, 1, out). */
int mcs_create_with_options(const mcs_params* p, int device, void* stream, const int32_t* keys, const int64_t* values, int n_options,
                            int use_env, mcs_ctx** out);
/* Rows of the option table, and the row of one key (0 .. count - 1).  They need no context and no GPU. */
int mcs_option_count(void);
int mcs_option_describe(int key, mcs_option_desc* out);
/* Change an option of a context for the launches queued by later calls; no synchronisation.  Refused, with a message and nothing
 * changed: what mcs_create_with_options refuses, a creation-only key, MCS_OPT_PIPE_SIDE_CUS after the first pipelined run, a null
 * context. */
int mcs_set_option(mcs_ctx* ctx, int key, int64_t value);
/* The value the next launch will use.  A null context or a null value pointer is an error. */
int mcs_get_option(mcs_ctx* ctx, int key, int64_t* value);
int mcs_destroy(mcs_ctx* ctx);
int mcs_sync(mcs_ctx* ctx);

/* Optional: make the context accumulate into caller-owned DEVICE buffers (e.g.
 * torch tensors, so that torch.distributed can all-reduce them in place).
 * Without this call the context allocates its own. */
int mcs_bind_tallies(mcs_ctx* ctx, double* dev_f64, int64_t n_f64, int64_t* dev_i64, int64_t n_i64);
double*  mcs_tallies_f64_devptr(mcs_ctx* ctx);
int64_t* mcs_tallies_i64_devptr(mcs_ctx* ctx);

/* ---- per-iteration / per-species inputs (host pointers) ----------------- */
/* grid tables at src/main_loops.jl:255-260; n_entries = n_grid+2 */
int mcs_set_grid(mcs_ctx* ctx, int n_entries, const double* x_grid_cm,
                 const double* ux_sk, const double* uz_sk, const double* utot,
                 const double* gam_sf, const double* gam_ef, const double* beta_ef,
                 const double* btot, const double* theta);
/* pcuts/tcuts/x_spec/inj_fracs/eps_target at src/main_loops.jl:244,259-262 */
int mcs_set_cuts(mcs_ctx* ctx, int n_pcuts, const double* pcuts, int n_tcuts, const double* tcuts,
                 int n_xspec, const double* x_spec, const double* inj_fracs /*[n_ions]*/,
                 const double* eps_target /*[n_grid]*/);
/* resets of src/main_loops.jl:59-86 (fluxes, weight_coupled := 1e-99; pools := 0; scalars := 1e-99) */
int mcs_begin_iteration(mcs_ctx* ctx, int i_iter);
/* src/main_loops.jl:97-121,164 + clear_psd! (src/ion_init.jl:1-16): psd/esc_psd := 1e-99,
 * num_crossings/therm := 0, fluxes := 0 (quirk Q2), recv_pool := transfer_pool.
 * With do_tcuts it also queues, on the context's stream, one device-to-device copy of the species' block
 * spectra_coupled[i_ion][0..MCS_NA_C)[0..201) into a base buffer that the context owns (mcs_tcut_spectra, K12, reads it); without
 * do_tcuts nothing is queued.  With cuts set and n_xspec >= 1 it queues likewise one copy of rows 0..n_xspec-1 of spectra_sf and
 * spectra_pf (mcs_detector_spectra, K14, reads it); with no detector nothing is queued. */
int mcs_begin_species(mcs_ctx* ctx, int i_iter, int i_ion, double aa, double zz,
                      double pmax_cutoff, double density, double electron_weight_fac);
/* analytic fast-push fluxes of init_pop/F_update! (src/initializers.jl:1054-1068,1156) */
int mcs_set_fluxes(mcs_ctx* ctx, const double* pxx, const double* pxz, const double* energy);

/* ---- population (device resident) --------------------------------------- */
int mcs_pop_upload(mcs_ctx* ctx, int64_t n, const mcs_soa* host);
int mcs_pop_download(mcs_ctx* ctx, int64_t n, mcs_soa* host);          /* current ("new") population */
int mcs_saved_download(mcs_ctx* ctx, int64_t n, mcs_soa* host, uint8_t* l_save); /* *_saved arrays */
int64_t mcs_pop_size(mcs_ctx* ctx);
/* K3: fast-push part of init_pop (src/initializers.jl:1078-1131) +
 * assign_particle_properties_to_population! (src/ion_init.jl:29-53), on device.
 * ptot_pf_in/weight_in: host, n entries.  Population RNG: Philox key
 * (i_iter-1)*n_ions+(i_ion-1) (src/main_loops.jl:120), draw j-1 = pitch of
 * particle j, draw n_total+j-1 = phase of particle j (global j = j_offset+local). */
int mcs_init_pop(mcs_ctx* ctx, int64_t n, int64_t j_offset, int64_t n_total,
                 const double* ptot_pf_in, const double* weight_in,
                 double x_start_cm, int i_grid_start, int relativistic, int fast_push);
/* The same from the host's momentum discretisation instead of per-particle arrays (set_inj_dist,
 * src/initializers.jl:1251-1328, gives every particle of a bin the same ptot and weight): particle j
 * (global, 0-based) lies in the bin b with bin_start[b] <= j < bin_start[b+1]; bin_start has n_bins+1
 * entries, bin_start[n_bins] = n_total.  O(bins) host work and upload instead of O(N). */
int mcs_init_pop_binned(mcs_ctx* ctx, int64_t n_local, int64_t j_offset, int64_t n_total, int n_bins,
                        const double* bin_ptot_pf, const double* bin_weight, const int64_t* bin_start,
                        double x_start_cm, int i_grid_start, int relativistic, int fast_push);
/* ... for a strided shard: local particle k is global particle j_first + k * j_stride (multi-GPU: rank r of W takes
 * j_first = r, j_stride = W, so that every rank holds the same mix of the momentum-sorted injection). */
int mcs_init_pop_binned_strided(mcs_ctx* ctx, int64_t n_local, int64_t j_first, int64_t j_stride, int64_t n_total, int n_bins,
                                const double* bin_ptot_pf, const double* bin_weight, const int64_t* bin_start,
                                double x_start_cm, int i_grid_start, int relativistic, int fast_push);

/* K1: the particle loop of one pcut over the resident population.
 * i_prt_offset: global index of local particle 0 minus 1 (multi-GPU shards;
 * the RNG key uses the global i_prt).  n_saved: particles that reached pcut. */
int mcs_run_pcut(mcs_ctx* ctx, int i_pcut, int64_t i_prt_offset, int64_t* n_saved);
/* The same over a strided shard: local particle k carries the global 0-based index
 * i_prt_first + k * i_prt_stride (its RNG key uses that index + 1, as i_prt in
 * src/particle_loop.jl:35-40).  mcs_run_pcut(c, i, off, ns) == mcs_run_pcut_strided(c, i, off, 1, ns). */
int mcs_run_pcut_strided(mcs_ctx* ctx, int i_pcut, int64_t i_prt_first, int64_t i_prt_stride, int64_t* n_saved);
/* The same with an explicit index list: local particle k carries the global 0-based index dev_gidx[k] (DEVICE
 * memory, n = mcs_pop_size entries, owned by the caller and kept alive until the next mcs_run_pcut* or
 * mcs_new_pcut / mcs_split_import).  This is what a multi-GPU driver needs after a LOCAL split of an interleaved
 * shard: the children of rank r's saved particles are not an arithmetic progression of the global split. */
int mcs_run_pcut_indexed(mcs_ctx* ctx, int i_pcut, const int64_t* dev_gidx, int64_t* n_saved);
/* K2: pcut_finalize/new_pcut (src/cuts.jl:34-124) on device: stable compaction
 * of l_save and i_mult-fold replication with weight/i_mult. Returns new size. */
int mcs_new_pcut(mcs_ctx* ctx, int64_t i_mult, int64_t* n_new);
/* Multi-GPU form of new_pcut.  The reference builds the next population from ALL saved particles
 * (src/cuts.jl:34-98); with the population sharded over GPUs a local split leaves the late pcuts -- a
 * handful of saved particles, each replicated 10^5 times -- on one or two ranks.  Instead:
 *   mcs_saved_export  writes the saved particles of the last mcs_run_pcut*, compacted in index order, into
 *     caller-owned DEVICE buffers (torch tensors, all-gathered by the caller over RCCL):
 *     gidx[r] = global 0-based index of the r-th saved particle, f64[f * cap + r] = field f of it (the 8
 *     doubles of mcs_soa, in that order), meta[r] = grid | tcut << 16 | downstream << 24 | inj << 25.
 *     cap >= n_saved of that run.
 *   mcs_split_import  makes the new local population from n_parents parents in device buffers of the same
 *     layout, sorted by global index by the caller: local particle k is element o = first + k * stride of
 *     the global split population  o -> parent[o / i_mult]  with weight / i_mult  (the index arithmetic of
 *     src/cuts.jl:66-92 with a global o).  Global indices -- hence RNG keys -- are those of a one-GPU run. */
int mcs_saved_export(mcs_ctx* ctx, int64_t cap, int64_t* dev_gidx, double* dev_f64, uint32_t* dev_meta);
/* The index column of mcs_saved_export alone (8 B per saved particle): enough for the ranks to agree on every saved
 * particle's position in the global order, from which a local mcs_new_pcut's children get their global indices
 * (position * i_mult + j) without any particle leaving its GPU. */
int mcs_saved_gidx(mcs_ctx* ctx, int64_t cap, int64_t* dev_gidx);
int mcs_split_import(mcs_ctx* ctx, int64_t n_parents, int64_t cap, const double* dev_f64, const uint32_t* dev_meta,
                     int64_t i_mult, int64_t first, int64_t stride, int64_t n_local);

/* Host-buffer form of K1, the literal drop-in for the loop at main_loops.jl:228-292:
 * upload `in`, run, download saved arrays + l_save. */
int mcs_run_pcut_host(mcs_ctx* ctx, int i_pcut, int64_t n_pts_use, int64_t i_prt_offset,
                      const mcs_soa* in, mcs_soa* saved_out, uint8_t* l_save, int64_t* n_saved);

/* A species' pcuts with the long histories of every pcut finishing BESIDE the next pcut, on a second stream (the loop at
 * src/main_loops.jl:184-292 with pcut_finalize / new_pcut, src/cuts.jl:34-124, as mcs_run_pcuts_fused).  A particle is LONG in a pcut when
 * its history there took at least long_draws random draws; the next population is the children of the saved particles that are not
 * long, in index order, followed by the children of the saved long ones, in index order (the reference's order for long_draws =
 * infinity; the index keys a child's random stream, so the order is part of the result -- the oracle orders the same way:
 * orc_set_long_draws).  long_imult_max > 0: long histories are told apart only in the first pcut and in pcuts whose predecessor split by
 * at most that factor (elsewhere the pcut runs as one launch, in the reference's order): where few particles are saved and each is split a
 * hundredfold, i_mult hangs on the last long history.  n_target[k]: the target population after pcut first + k.  Outputs (host, length last - first + 1): n_use,
 * n_saved, i_mult per pcut, the main launch's kernel time; strag_out (or NULL, length 2 per pcut): particles exported, and 1 where
 * i_mult had to wait for them.  One rank with global indices 0, 1, 2, ...; fp64 state; not with sliced launches. */
int mcs_run_pcuts_pipelined(mcs_ctx* ctx, int i_pcut_first, int i_pcut_last, const int64_t* n_target, int64_t long_draws, int64_t long_imult_max,
                            int64_t* n_use_out, int64_t* n_saved_out, int64_t* i_mult_out, double* kernel_ms_out, int64_t* strag_out);

/* ---- tallies ------------------------------------------------------------ */
int mcs_read_tallies(mcs_ctx* ctx, double* host_f64 /*layout.total*/, int64_t* host_i64 /*mcs_i64_total*/);
/* A slice of the fp64 buffer, words [first, first + count) of the layout, into host_f64[0 .. count) (+ all int64 tallies
 * when host_i64 is not null).  The three histograms psd | therm_sf | therm_pf are 99 % of the buffer and have consumers on
 * the device (mcs_dndp_cr, mcs_thermo_calcs); what iter_finalize needs on the host -- fluxes, escape spectra, scalars,
 * pools (src/iter_finalize.jl:27-70) -- is the tail of the layout from esc_psd_up on: 0.8 MB instead of 61. */
int mcs_read_tallies_part(mcs_ctx* ctx, int64_t first, int64_t count, double* host_f64, int64_t* host_i64);
int mcs_write_tallies(mcs_ctx* ctx, const double* host_f64, const int64_t* host_i64);
/* The mirror of mcs_read_tallies_part: words [first, first + count) of the fp64 buffer from host_f64[0 .. count).  What the
 * host rewrites in place between iterations is small: tcut_print normalises spectra_coupled and floors weight_coupled
 * (src/io.jl:28-45, called at src/main_loops.jl:383-389). */
int mcs_write_tallies_part(mcs_ctx* ctx, int64_t first, int64_t count, const double* host_f64);
/* The running sums of src (the table beside mcs_tally_layout) added into dst's, word by word (each fp64 word is one plain
 * dst + src), and then set to zero in src; the per-species sections of both contexts are left as they are.  For species that ran
 * on a second context of the same problem (the ion species of an iteration do not depend on each other).
 * Both contexts' tally replicas are folded in first.  Ordered on the two contexts' streams, with no host synchronisation: dst's
 * stream waits for the work queued on src's, and src's stream waits for the add.  Refused, with nothing changed: a null
 * context, dst == src, contexts on different devices, or layouts that differ (total, n_grid, n_ions, n_itrs).  The caller
 * serialises the call with every other call on either context. */
int mcs_accumulate_tallies(mcs_ctx* dst, mcs_ctx* src);

/* ---- consumers of the tallies, on the device-resident histograms ----
 * Host-made tables (O(bins), O(n_grid)); the edges are cgs momenta and true cos(theta) in the
 * intended order (consumer quirks C1, C2 in DESIGN.md). */
typedef struct mcs_consumer_in {
  const double* mom_log_cgs;    /* [nmom+2] log10 of the momentum bin edges (cgs)               */
  const double* mom_edge_cgs;   /* [nmom+2] the edges themselves                                */
  const double* cos_edge;       /* [ntht+2] true cos(theta) of the angle bin edges              */
  const double* cos_center;     /* [ntht+1] thermo_calcs.jl:57-73                               */
  const double* pt_center;      /* [nmom+1] thermo_calcs.jl:75-80 (cgs)                         */
  const double* zone_pop;       /* [n_grid] set_grid_volumes! (particle_counter.jl:1466-1524)   */
  const double* density_loc;    /* [n_grid] gam0 beta0 n0 / sqrt(gam_sf^2 - 1) (thermo_calcs.jl:258) */
  const double* cold_pressure;  /* [n_grid] density_loc^(5/3) kB T0 (thermo_calcs.jl:266)       */
  double rest_energy;           /* m c^2 of the species                                         */
  double mc;                    /* m c                                                          */
  double n0;                    /* far-upstream density of the species                          */
  double gam0;
  int therm_from_hist;          /* 1: thermal crossings from the therm_pf histogram (A9, C5)    */
} mcs_consumer_in;
/* get_dNdp_cr + the CR normalisation of get_normalized_dNdp (src/particle_counter.jl:29-306,
 * 733-790) on the resident psd.  dNdp: host [3][n_grid][nmom+2] (frame: shock, plasma, ISM).
 * diag: host [2] (cells skipped on identify_corners error paths; searches that left the table). */
int mcs_dndp_cr(mcs_ctx* ctx, const mcs_consumer_in* in, double* dNdp, int64_t* diag);
/* thermo_calcs (src/thermo_calcs.jl:30-352) on the resident psd / therm_pf / num_crossings.
 * Outputs: host [n_grid] each. */
int mcs_thermo_calcs(mcs_ctx* ctx, const mcs_consumer_in* in, double* P_par, double* P_perp, double* energy_density);
/* K10: dN/dp of the particles that LEAVE the shock, from the two escape slabs of the tallies (the reference's print_dNdp_esc call at
 * src/ion_finalize.jl:65-68 has no body; the slabs are binned and weighted as psd is, so this is get_dNdp_cr of one zone whose slab
 * is a door's, up to and including dN -> dN/dp, particle_counter.jl:295-304, without the zone normalisation: a door has no volume).
 *   door 0: esc_psd_up (upstream free-escape boundary and p_max), door 1: esc_psd_down (the downstream end);
 *   frame 0: the shock frame, frame 1: the plasma frame of the door, Lorentz factor gam_pf[door] (beta by the rule of
 *   transformers.jl:639, 0 below 1.000001), frame 2: the ISM frame, in->gam0.
 * It reads mom_log_cgs, mom_edge_cgs, cos_edge, rest_energy and gam0 of `in`; gam_pf: host [2], each >= 1.
 * dNdp: host [2][3][nmom+2] (door, frame); entry nmom+1 of every row is 1e-99, a bin whose dN is below 1e-66 is 1e-99.
 * number: host [2][3], the row's dN summed over the bins 0..nmom in ascending order, before the division by the bin widths.
 * diag: host [2][2] or null, per door the cells skipped on identify_corners error paths and the bin searches that left the table,
 * both frames 1 and 2 counted, as mcs_dndp_cr counts them.
 * A slab is [201][201] with the momentum index fastest, whatever the binning; only ip < nmom+2, jtheta < ntht+2 are ever written,
 * and nothing else is read.  Cells, thresholds and the spreading of a cell over the bins are those of mcs_dndp_cr.
 * ORDER OF THE ADDS (normative; no floating-point atomics, so every call on the same tallies gives the same bits):
 *   frames 1, 2: every angle row j = 0..ntht has a partial histogram R_j[l] that starts at 0.0 and takes the parts of its lit cells
 *   with ip ascending (a cell's parts in the order triangular_distribution! makes them);
 *   dN[l] = ((0.0 + R_0[l]) + R_1[l]) + ... + R_ntht[l];
 *   frame 0: dN[l] = the cells > 0 of column l added to 0.0 with jtheta = 0..ntht+1 ascending;
 *   number = ((0.0 + dN[0]) + dN[1]) + ... + dN[nmom].
 * The result also stays on the device, in a buffer that no other call writes, for the escape sample of the ensemble statistics
 * (below); mcs_begin_species and that sample invalidate it. */
int mcs_dndp_esc(mcs_ctx* ctx, const mcs_consumer_in* in, const double* gam_pf, double* dNdp, double* number, int64_t* diag);
/* K11: the pitch-angle distribution of every grid zone over up to MCS_ANGLE_MAX_WINDOWS momentum windows, in three frames, from the
 * resident psd, therm_sf and num_crossings and the grid tables (gam_sf).  Of `in` it reads pt_center, cos_center, cos_edge,
 * rest_energy, gam0 and therm_from_hist.
 *   frame 0: the shock frame; frame 1: the plasma frame of the zone, Lorentz factor gam_sf[zone] as mcs_dndp_cr takes it;
 *   frame 2: the ISM frame, in->gam0.  beta by the rule of transformers.jl:639 (0 below 1.000001).
 * Window m is the momentum bins l_lo[m] <= kX < l_hi[m] OF THE TARGET FRAME; 0 <= l_lo < l_hi <= nmom + 1, 1 <= n_win <=
 * MCS_ANGLE_MAX_WINDOWS; windows may overlap.  Anything else is refused with a message and nothing is changed.
 * CELLS: with NM = nmom + 2, NT = ntht + 2, the cells j <= ntht, k <= nmom of psd[z][j][k] (momentum fastest).  A cell's weight:
 *   v = 0.0;  if therm_from_hist and num_crossings[z] != 0: v = v + therm_sf[z][j][k];  if psd[z][j][k] > 1e-66: v = v + psd[z][j][k];
 * the cell is lit if v > 1e-66 (a NaN cell is not lit).
 * IMAGE of cell (j, k): itself in frame 0 (nothing is computed); in frames 1 and 2 the centre-point rebin of mcs_dndp_2d, every
 * operation rounded separately:
 *   px = pt_center[k] * cos_center[j];  pc = pt_center[k] * c;  et = sqrt(pc*pc + E0*E0);
 *   pxX = gam * (px - beta * et / c);   ptX = sqrt(pt*pt - px*px + pxX*pxX);
 *   kX = the momentum bin of ptX, jX = the angle bin of (pxX, ptX), as mcs_dndp_2d finds them; both clamped into 0..nmom, 0..ntht.
 * OUTPUTS (host; each may be null): dist [3][n_grid][n_win][NT], number [3][n_grid][n_win], moments [3][n_grid][n_win][2].
 * ORDER OF THE ADDS (normative; no floating-point atomics, so every call on the same tallies gives the same bits):
 *   A[jX] = the weights of the lit cells whose image lies in row jX and in the window, added to 0.0 with j ascending and, within
 *   a row, k ascending;
 *   number = ((0.0 + A[0]) + A[1]) + ... + A[ntht];
 *   dist[j] = (A[j] / number) / (cos_edge[j+1] - cos_edge[j]) where A[j] > 0, else 1e-99;  dist[ntht+1] = 1e-99;
 *   a window that no cell reaches has number = 0.0 and all of dist at 1e-99;
 *   moments[0] = <mu> = s1 / number, s1 the serial sum from 0.0 over j = 0..ntht of t_j = A[j] * cos_center[j];
 *   moments[1] = <mu^2> = s2 / number, s2 the serial sum of t_j * cos_center[j];
 *   with number == 0 both moments are a quiet NaN -- the convention of the slope words of the products sample: a summary counts
 *   such a word in n_nonfinite, no trigger on it is met, and ONE empty sample keeps the word's mean non-finite.  Windows belong on
 *   zones and momenta that the population reaches.
 * The result also stays on the device, in a buffer that no other call writes, for the angles sample of the ensemble statistics
 * (below); mcs_begin_species, a write of the tallies and that sample invalidate it.  The call changes neither the tallies nor what
 * mcs_dndp_cr, mcs_thermo_calcs, mcs_dndp_2d and mcs_dndp_esc left on the device. */
#define MCS_ANGLE_MAX_WINDOWS 8
int mcs_angle_dist(mcs_ctx* ctx, const mcs_consumer_in* in, int n_win, const int32_t* l_lo, const int32_t* l_hi,
                   double* dist, double* number, double* moments);
/* K12: the spectra of the time cuts, "how far has acceleration got after time t" (the reference's tcut_print, src/io.jl:21-76,
 * called at src/main_loops.jl:383-389), for the context's CURRENT species and the n_tcuts (nt) cuts of mcs_set_cuts, from the
 * resident weight_coupled and spectra_coupled.  Of `in` it reads only mom_log_cgs (e[l], NM = nmom + 2 edges).
 * BASE.  spectra_coupled is never reset, so a species' contribution in one iteration is the growth of its row block over the
 * base that mcs_begin_species took: independent of earlier iterations, of tcut_print's rewrite and of mcs_accumulate_tallies.
 * All deposits are positive and fl(base + w) >= base, so the growth g = now - base (one subtraction per word) is never negative,
 * and exactly 0.0 where nothing was deposited.
 * out: host, laid out as mcs_tcut_get_layout says (it needs no GPU; 1 <= n_tcuts < MCS_NA_C):
 *   spectrum [nt][NM] | weight [nt] | number [nt] | mean_log_p [nt] | quantile [3][nt] | index [3];  total nt (NM + 6) + 3.
 * Every operation is a separate fp64 rounding; there are no floating-point atomics, so every call on the same buffers gives the
 * same bits.
 *   BINS: a row has the bins l = 0..nmom, with edges e[l] and e[l+1].  Entry nmom+1 of spectrum is 1e-99.  Words with l > nmom of
 *   the 201-wide tally row, and rows k >= nt, are never read.
 *   GROWTH AND NUMBER: g[l] = now[l] - base[l];  number[k] = ((0.0 + g[0]) + g[1]) + ... + g[nmom], serial and ascending.
 *   WEIGHT: weight[k] is weight_coupled[i_ion][k] as it stands, or 1e-99 where it is below 1e-60 (tcut_print's floor).
 *   LIVE AND DEAD ROWS: a row is live if number[k] > 1e-99.
 *     live: spectrum[k][l] = g[l] / number[k], or 1e-99 where that is below 1e-60 (tcut_print's normalisation and floor);
 *     dead: spectrum all 1e-99, number 0.0, mean_log_p and the three quantiles a quiet NaN -- the convention of the slope words of
 *     the products sample: a summary counts them in n_nonfinite and no trigger on them is ever met.  Triggers belong on cuts below
 *     age_max: the last cut must lie above 10 x age_max and stays dead.
 *   MEAN: mean_log_p[k] = (sum_l g[l] * c_l) / number[k] with c_l = 0.5 * (e[l] + e[l+1]); the sum serial and ascending from 0.0.
 *   QUANTILES: MCS_TCUT_Q, q = 0.5, 0.9, 0.99.  T = q * number[k];  C_0 = 0.0, C_{l+1} = C_l + g[l];  l* is the first l with
 *     g[l] > 0 and C_{l+1} >= T;  f = (T - C_{l*}) / g[l*].  If the last lit bin's C falls short of T through rounding, l* is that
 *     bin and f is 1.0.  quantile = e[l*] + f * (e[l*+1] - e[l*]): log10 of the momentum below which the fraction q of the
 *     still-coupled weight lies, "p reached by time t".
 *   INDEX: index[j] is the least-squares slope of quantile[j][k] against log10(tcuts[k]) (the deterministic log10 of
 *     include/mcs_math.h) over the live rows, k ascending, exactly by the rule of the products slope below ("Slope of frame m":
 *     a live row is a valid bin, x = log10 tcuts[k], y = quantile[j][k]); fewer than three live rows give a quiet NaN.
 * diag: host [2] or null: the number of live rows, and the number of words read with now < base.  The second must be 0; it is
 * there so that a caller who overwrote the tallies sees it.
 * The result also stays on the device, in a buffer that no other call writes, for the tcuts sample of the ensemble statistics
 * (below); mcs_begin_species and that sample invalidate it.
 * Refused, with a message: a context without do_tcuts, before mcs_set_cuts (or with no time cut set), before the first
 * mcs_begin_species, a null table or output. */
#define MCS_TCUT_NQ 3
#define MCS_TCUT_Q {0.5, 0.9, 0.99}
typedef struct mcs_tcut_layout {
  int64_t spectrum, weight, number, mean_log_p, quantile, index;   /* offsets, in doubles */
  int64_t row_n;                                            /* nmom + 2: the length of a spectrum row */
  int64_t n_tcuts;                                          /* the length of weight, number, mean_log_p and of a quantile row */
  int64_t total;
} mcs_tcut_layout;
int mcs_tcut_get_layout(const mcs_params* p, int n_tcuts, mcs_tcut_layout* out);     /* needs no GPU */
int mcs_tcut_spectra(mcs_ctx* ctx, const mcs_consumer_in* in, double* out, int64_t* diag);

/* K14: the spectra at the detectors, "what does a detector at a fixed place see" (the reference's calculate_x_spec_spectra!,
 * src/all_flux.jl:164-190, fills spectra_sf and spectra_pf at every crossing of an XSPEC position; nothing in the reference reads
 * them), for the context's CURRENT species and the nd = n_xspec detectors of mcs_set_cuts, from the resident spectra_sf (frame
 * f = 0, shock frame) and spectra_pf (f = 1, plasma frame).  Of `in` it reads mom_log_cgs (e[l]) and mom_edge_cgs (E[l]), NM = nmom + 2
 * edges each.
 * BASE.  Both sections are shared by all species and never reset.  With cuts set and n_xspec >= 1, mcs_begin_species queues, on the
 * context's stream, ONE device-to-device copy of rows 0..nd-1 of both sections into a base buffer that the context owns
 * ([2][nd][201]); with no detector nothing is queued.  A species' contribution in one iteration is the growth of the rows over that
 * base: g = now - base, one subtraction per word, exactly 0.0 where nothing was deposited.  The deposits of spectra_pf are positive
 * (weight |p / p_x| F), so g[1] is never negative.  Those of spectra_sf are SIGNED as in the reference (weight p / p_x in the shock
 * frame, negative for a crossing towards upstream): a row of frame 0 is the NET flux-weighted count, its number is close to the
 * injected flux at every upstream detector, and in a real run single bins of it may come out negative.  The rules below take such
 * a word as it is: it enters number, mean and the cumulative sums, its spectrum word falls to the floor, its dndp is negative, and it
 * is no valid bin of a slope or of the gradient (which need g > 0).  mcs_set_cuts drops the base.  Because the rows are not per species, anything else that adds
 * into them between mcs_begin_species and this call -- another species, mcs_accumulate_tallies of a secondary context -- is counted
 * as the current species' growth: one context, one species at a time.
 * out: host, laid out as mcs_detector_get_layout says (it needs no GPU; 1 <= n_det <= n_grid):
 *   spectrum [2][nd][NM] | dndp [2][nd][NM] | number [2][nd] | mean_log_p [2][nd] | quantile [3][2][nd] | slope [2][nd] | gradient [NM];
 *   total 2 nd (2 NM + 6) + NM.
 * Every operation is a separate fp64 rounding; sums are serial and ascending from 0.0; there are no floating-point atomics, so
 * every call on the same buffers gives the same bits.
 *   BINS: a row has the bins l = 0..nmom.  Words with l > nmom of the 201-wide tally row, and rows >= nd, are never read.
 *   GROWTH AND NUMBER: g[f][d][l] = now - base;  number[f][d] = ((0.0 + g[0]) + g[1]) + ... + g[nmom].
 *   LIVE AND DEAD ROWS: a row is live if number > 1e-99.  A dead row has spectrum and dndp all 1e-99, number 0.0, and mean_log_p,
 *     the three quantiles and slope a quiet NaN (K12's convention: a summary counts them in n_nonfinite, no trigger on them is met).
 *   SPECTRUM, MEAN, QUANTILES: K12's rules word for word (mcs_tcut_spectra above: spectrum[l] = g[l] / number or 1e-99 where that
 *     is below 1e-60, entry nmom+1 1e-99; MEAN; QUANTILES with MCS_TCUT_Q and the f = 1 fall-back).
 *   DNDP: on a live row dndp[l] = g[l] / (E[l+1] - E[l]), or 1e-99 where g[l] is 0.0; entry nmom+1 is 1e-99.  A table whose E is
 *     not strictly ascending is refused.
 *   SLOPE: slope[f][d] is the least-squares slope ("Slope of frame m" below) over the window l_lo <= l < l_hi of a live row: a bin
 *     is valid if g[l] > 0, x = 0.5 (e[l] + e[l+1]), y = log10(dndp[l]) (the deterministic log10 of include/mcs_math.h); fewer than
 *     three valid bins give a quiet NaN.  The window needs 0 <= l_lo, l_hi <= nmom + 1, l_hi - l_lo >= 3.
 *   GRADIENT: frame 0 only, for l = 0..nmom: the same slope rule over the detectors d = 0..nd-1 in index order (whatever their
 *     order in x).  A detector is valid if x_spec[d] < 0.0 (upstream; one at exactly 0.0 is not) and g[0][d][l] > 0;
 *     x = x_spec[d] / x_unit, y = log10(g[0][d][l]).  Fewer than three valid detectors give a quiet NaN; gradient[nmom+1] is a quiet
 *     NaN.  x_unit must be finite and positive; a driver passes rg0.  DSA predicts n(x, p) ~ exp(u0 x / D(p)) upstream, so
 *     ln 10 * gradient[l] is u0 / D(p_l) in units of 1 / x_unit: the inverse e-fold length of the precursor at that momentum.  Bins
 *     that few particles reach are NOISY -- three points through counts of a few -- which is what the error bar of the detectors
 *     sample is for.
 * diag: host [3] or null: the number of live rows (of 2 nd); the number of words read with now < base (0 on rows that took only
 *   positive deposits, so a caller who overwrote such tallies sees it; in a real run the signed frame-0 bins described under BASE
 *   are counted here); the number of finite gradient words.
 * The result also stays on the device, in a buffer that no other call writes, for the detectors sample of the ensemble statistics
 * (below); mcs_begin_species, mcs_set_cuts and that sample invalidate it.
 * Refused, with a message and nothing written: a null argument or table, before mcs_set_cuts, with no detector set, before the
 * first mcs_begin_species, without a base (cuts set after the species began), a bad window, a bad x_unit, a table E that does not
 * ascend. */
typedef struct mcs_detector_layout {
  int64_t spectrum, dndp, number, mean_log_p, quantile, slope, gradient;   /* offsets, in doubles */
  int64_t row_n;                                            /* nmom + 2: the length of a spectrum or dndp row and of gradient */
  int64_t n_det;                                            /* nd */
  int64_t total;
} mcs_detector_layout;
int mcs_detector_get_layout(const mcs_params* p, int n_det, mcs_detector_layout* out);     /* needs no GPU; 1 <= n_det <= n_grid */
int mcs_detector_spectra(mcs_ctx* ctx, const mcs_consumer_in* in, int l_lo, int l_hi, double x_unit, double* out, int64_t* diag);

/* K13: the shock-profile update, "which profile would smooth_grid_par write from this iteration" (the reference's iter_finalize,
 * src/iter_finalize.jl:1-110, with smooth_grid_par / new_velocity_profile / smooth_profile!, src/smoothers.jl:54-604, as the host's
 * iter_finalize.py restates them), up to and including ux_new = (ux_new + w ux) / (1 + w).  The refresh of the grid tables that
 * follows (gam_sf, beta_ef, btot ...) is not part of it, and nothing on the context but the result buffer is written.
 * READ WHERE IT LIES: pxx_flux, energy_flux [n_grid] and scalars [4] of the resident tallies; ux, gam_sf, x_grid_cm of mcs_set_grid
 * (entries 1..n_grid); P_par | P_perp | energy_density [n_grid] each as the last mcs_thermo_calcs left them on the device -- or,
 * with a non-null `pressures`, 3 n_grid host doubles in that order in their place (crafted inputs; pressures made elsewhere).  No
 * other tally word is read.  u0, beta0, gam0, n_grid, i_shock are the context's parameters.
 * PASSED BY THE HOST in a mcs_profile_in, none of which depends on the iteration's tallies: the upstream fluxes, the species sums P0 = kB sum
 * n T and rho0 = sum n m of q_esc_calcs, n0_aa = sum n aa, r_comp, r_RH, u2, beta2, gam2, SMMOE, SMPFP, the old-profile weight w AFTER
 * the increase_old_profile_weighting rule, i_trans (the Julia zone number at which the artificial arctangent section starts; 0 = no
 * artificial smoothing), n_hist <= 3 earlier (q_px, q_en) pairs oldest first, and three tables of n_grid doubles for zones 1..n_grid:
 * pxx_EM, en_EM (the electromagnetic fluxes of the current profile and field) and atan_x = atan(x_grid_rg).
 * ARITHMETIC: fp64, every operation rounded separately, in the order of the Python expressions of iter_finalize.py as Python
 * evaluates them, with their parentheses; the numpy lines elementwise.  Only + - * /, sqrt_ (mcs_math.h), rint, copysign, fabs and
 * comparisons; no transcendental is evaluated on the device.  POWERS ARE PRODUCTS: a**2 is a*a, a**3 is (a*a)*a.  This is a
 * deliberate difference from iter_finalize.py: CPython's x**2 is pow(x, 2), which differs from x*x in about 1 of 1200 doubles (x**3
 * from (x*x)*x in 26 %), so this statement is NOT bit-equal to the host file; it agrees with it to rounding.
 * NaN and infinity propagate as IEEE gives them (arr[0] == avg is a division by zero); max(a, 1e-99) is (1e-99 > a ? 1e-99 : a).
 * With c = MCS_C, mp = MCS_MP, zone j = 0..n-1 (table entry j + 1), sc = scalars:
 *   SCALARS  px_esc = sc[2] / F_px_upstream; en_esc = sc[3] / F_energy_upstream; gamma_down = 1 + sc[0] / sc[1].
 *   Q  (q_esc_calcs; its two returns bound to (q_px, q_en) in the reference's order)  r_comp == r_RH: both 0.  Else Gf = G / (G - 1)
 *     with G = gamma_down, rho2 = ((rho0 gam0) beta0) / (gam2 beta2), and for beta0 >= 0.02 (the RELATIVISTIC branch, also below):
 *       q_fac = c sqrt_((1 + beta0) / 2); e = rho0 (c c) + 2.5 P0; Fp = ((gam0 gam0)(beta0 beta0)) e + P0; Fe = ((gam0 gam0) u0) e;
 *       aux = (gam2 gam2)(q_fac (beta2 beta2) - u2); P2 = ((q_fac Fp - Fe) - (aux rho2)(c c)) / (q_fac + Gf aux); t = gam2 beta2;
 *       Qp = (Fp - (t t)(rho2 (c c) + Gf P2)) - P2; q_px = (Qp q_fac) / (Fe - ((gam0 u0) rho0)(c c)); q_en = Qp / Fp
 *     otherwise (CLASSICAL): Fp = rho0 (u0 u0) + P0; Fe = (rho0 ((u0 u0) u0)) / 2 + (2.5 P0) u0; P2 = Fp - rho2 (u2 u2);
 *       q_px = ((Fe - ((rho0 u0)(u2 u2)) / 2) - (P2 u2) Gf) / Fe; q_en = 0.
 *     AVERAGE: q_avg = (((h0 + h1) + h2) + q) / k over the n_hist history values in their order and then this iteration's, k = n_hist + 1
 *     (the sum starts with its first term).
 *   ROUNDING  pxx[j] = rint(pxx_flux[j] 1e13) / 1e13, en[j] likewise (np.round(x, 13)); rows flux_px = pxx / F_px_upstream, flux_en.
 *   GAMMA  Ptot = P_par + P_perp; G[j] = 1 + Ptot / e_dens, but 1e-99 where e_dens == 1e-99; Xi = G / (G - 1).
 *   Qpx = q_px_avg pxx[0] (relativistic; 0.0 classical); Qen = q_en_avg en[0]; u = ux[j]; b = u / c; g = gam_sf[j].
 *   RELATIVISTIC ZONE  gb = g b; gb2 = gb gb; dens = ((gam0 beta0) / (g b)) n0_aa; p_px = (pxx - ((gb2 dens) mp)(c c)) / (1 + gb2 Xi);
 *     p_loc = (1 - SMPFP) p_px + SMPFP Ptot; y = (((F_px - Qpx) - pxx_EM) - p_loc) / (((gam0 beta0) n0_aa)(mp (c c) + (p_loc Xi) / dens));
 *     ux_px = (y / sqrt_(1 + y y)) c; K = ((F_en - Qen) - en_EM) / (c ((dens mp)(c c) + Xi p_loc)); z = (-1 + sqrt_(1 + (4 K) K)) / 2;
 *     y = copysign(sqrt_(z), K); ux_en = (y / sqrt_(1 + y y)) c.
 *   CLASSICAL ZONE  rm = n0_aa mp; p_px = (pxx - ((rm u0) u)(1 + b b)) / (1 + (b b) Xi); p_loc as above; A = (F_px - Qpx) - pxx_EM;
 *     B = (F_en - Qen) - en_EM.  NEWTON: x from x0, at most 10000 times { dx = f / f'; x = x - dx; stop when |dx| <= 1e-14 |x| } (a NaN
 *     never passes: such a zone runs all its steps).  Momentum, x0 = (u0 / c) 1e-4: f = (A - ((rm u0)(x c))(1 + x x)) - (1 + (x x) Xi) p_loc,
 *     f' = -(((rm u0) c)(1 + (3 x) x) + ((2 x) Xi) p_loc); ux_px = x c.  Energy, x0 = u0 1e-4, t = x / c, t2 = t t:
 *     f = (B - ((((0.5 rm) u0) x) x)(1 + 1.25 t2)) - ((Xi p_loc) x)(1 + t2), f' = -(((rm u0) x)(1 + 2.5 t2) + (Xi p_loc)(1 + 3 t2)); ux_en = x.
 *   LAST TEN  avg = (0.0 + a[n-10] + ... + a[n-1]) / 10 for a = ux_px and ux_en, ascending from zone max(0, n - 10), before any smoothing,
 *     divided by 10 whatever n_grid.
 *   SMOOTH (smooth_profile!)  for i = n-1 down to 1: if a[i-1] < a[i] then a[i-1] = a[i].  Then from the row as that pass left it:
 *     d[1] = ((2 a[0] + a[1]) + a[2]) / 4; d[i] = ((a[i-1] + a[i]) + a[i+1]) / 3 for 2 <= i <= n-3; d[n-2] = ((a[n-3] + a[n-2]) + 2 a[n-1]) / 4
 *     (in this order, a later one replacing an earlier); a[1..n-2] = d[1..n-2].
 *   RESCALE  s = (u0 - u2) / (a[0] - avg); a[j] = s (a[j] - avg) + u2 for every j, from the a[0] before it; then zones with
 *     x_grid_cm >= 0 are pinned to u2.  Relativistic: smooth, then rescale; classical: rescale, then smooth.
 *   BLEND  ux_pred = (1 - SMMOE) ux_px + SMMOE ux_en (the return of new_velocity_profile).
 *   ARTIFICIAL (i_trans > 0)  s = -(ux_pred[i_trans-1] - ux_pred[n-1]) / atan_x[i_trans-1]; zones i_trans..i_shock (j = i_trans-1 .. i_shock-1):
 *     v[j] = (-atan_x[j]) s + ux_pred[n-1]; elsewhere v = ux_pred.
 *   WEIGHT  ux_next = (v + w u) / (1 + w).  SHIFT  shift = (ux_pred - u) / u0; shift_rms = sqrt_(S / n), S = 0.0 + shift[0]^2 + ..., ascending.
 * out: host, laid out as mcs_profile_get_layout says (it needs no GPU): ten rows of n_grid doubles -- flux_px, flux_en, gamma_ad (G),
 *   p_flux (p_px), p_used (p_loc), ux_px, ux_en (after rescale and smooth), ux_pred, ux_next, shift -- then the eight scalars gamma_down,
 *   px_esc_up, en_esc_up (= max(., 1e-99), as the host floors them last), q_px, q_en, q_px_avg, q_en_avg, shift_rms.  Total 10 n_grid + 8.
 * diag: host [3] or null: the number of non-finite words of out; the number of zones in which a Newton iteration ran out of steps;
 *   the largest Newton step count (0 in the relativistic branch).
 * One launch of one workgroup, no atomics: every call on the same inputs gives the same bits.  The result also stays on the device, in
 * a buffer that no other call writes, for the profile sample of the ensemble statistics (below); mcs_begin_species, a tally write and
 * that sample invalidate it.
 * Refused, with a message: before mcs_set_grid, before the first mcs_begin_species, pressures == NULL on a context whose
 * mcs_thermo_calcs result is not whole (never run, or taken by a products sample), i_trans outside [0, i_shock], n_hist outside
 * [0, 3], n_grid < 3, a null table or output. */
#define MCS_PROFILE_ROWS 10
#define MCS_PROFILE_SCALARS 8
#define MCS_PROFILE_MAX_HIST 3
#define MCS_PROFILE_NEWTON_MAX 10000
typedef struct mcs_profile_in {
  double F_px_upstream, F_energy_upstream, P0, rho0, n0_aa, r_comp, r_RH, u2, beta2, gam2, SMMOE, SMPFP, w;
  int32_t i_trans;                       /* the settings end here: an ensemble keeps the fields above and this one */
  int32_t n_hist;
  double hist_q_px[MCS_PROFILE_MAX_HIST], hist_q_en[MCS_PROFILE_MAX_HIST];
  const double *pxx_EM, *en_EM, *atan_x; /* host [n_grid] each */
} mcs_profile_in;
typedef struct mcs_profile_layout {
  int64_t flux_px, flux_en, gamma_ad, p_flux, p_used, ux_px, ux_en, ux_pred, ux_next, shift, scalars;   /* offsets, in doubles */
  int64_t row_n;                                            /* n_grid: the length of each of the ten rows */
  int64_t n_scalars;                                        /* 8 */
  int64_t total;
} mcs_profile_layout;
int mcs_profile_get_layout(const mcs_params* p, mcs_profile_layout* out);     /* needs no GPU */
int mcs_profile_update(mcs_ctx* ctx, const mcs_profile_in* in, const double* pressures_or_null, double* out, int64_t* diag);

/* ---- photon post-processing: the synchrotron fold of src/synch_emission.jl:27-171 over the plasma-frame
 * dN/dp of an electron species (frame 2 of mcs_dndp_cr), for every grid zone with the zone's field of the grid tables.
 * dNdp_pf: host [n_grid][nmom+2]; mom_edge_cgs: host [nmom+2]; mc of the species; photon energies
 * E_j = emin_mev * 10^(j / bins_per_dec), j = 0 .. n_photon-1 (photon_calcs.jl:11-19,51: 1e-13 MeV, 10 per decade, 180 bins).
 * Outputs (host): energy_erg[n_photon] (may be null), emis[n_grid][n_photon] = dP/d(ln E) in erg/s per zone, floor 1e-99.
 * The photon stack is dead code in the reference and is followed as specification; F(x) is restated (include/mcs_synch.h). */
int mcs_photon_synch(mcs_ctx* ctx, const double* dNdp_pf, const double* mom_edge_cgs, double mc, int n_photon, double emin_mev,
                     double bins_per_dec, double* energy_erg, double* emis);

/* The pion-decay fold of src/photon_pion_decay.jl:40-183 -> src/pion_kafexhiu.jl:37-245 (Kafexhiu et al. 2014, src/KATV2014.jl) over the
 * plasma-frame dN/dp of a nucleus species (aa >= 1; frame 2 of mcs_dndp_cr; the thermal histogram of get_normalized_dNdp is empty, quirk C4),
 * for every grid zone.  dNdp_pf: host [n_grid][nmom+2]; mom_edge_cgs: host [nmom+2]; mc, aa of the species; target_density: host [n_grid]
 * = n0[1] gam0 beta0 / sqrt(gam_sf^2 - 1) (photon_pion_decay.jl:62-63); scaling: the heavy-nuclei factor of pion_kafexhiu.jl:60-65; i_data:
 * 1 GEANT 4 (what the reference hard-wires), 2 PYTHIA 8, 3 SIBYLL 2.1, 4 QGSJET-I; photon energies E_j = emin_mev * 10^(j / bins_per_dec)
 * (photon_calcs.jl:15-16,49: 1 MeV, 10 per decade, 120 bins).  Outputs (host): energy_erg[n_photon] (may be NULL), emis[n_grid][n_photon] =
 * dP/d(ln E) in erg/s per zone, floor 1e-99.  Dead code in the reference, followed as specification (include/mcs_pion.h: P1-P3). */
int mcs_photon_pion(mcs_ctx* ctx, const double* dNdp_pf, const double* mom_edge_cgs, double mc, double aa, const double* target_density, double scaling,
                    int i_data, int n_photon, double emin_mev, double bins_per_dec, double* energy_erg, double* emis);

/* get_dNdp_2D (src/particle_counter.jl:343-627, called at src/ion_finalize.jl:50-59) on the resident psd / therm_sf / num_crossings:
 * d2N/dp dcos of every zone, normalised to the zone population, rebinned by cell centres into the frame that moves with
 * (gam_x, beta_x) against the shock frame -- the ISM frame for (gam0, beta0), the only frame the function returns (m = 2, :538).
 * Uses mom_edge_cgs, cos_center, pt_center, zone_pop, rest_energy, n0, therm_from_hist of `in`.  The array stays on the device for
 * mcs_photon_ic; d2N: host [n_grid][ntht+2][nmom+2] (momentum fastest), floor 1e-99, may be NULL. */
int mcs_dndp_2d(mcs_ctx* ctx, const mcs_consumer_in* in, double gam_x, double beta_x, double* d2N);
/* The inverse-Compton fold of src/inverse_compton.jl:36-311 (photon_IC -> IC_emission_FCJ: Jones 1968, eq. 9) over the array the last
 * mcs_dndp_2d left on the device, per grid zone.  j_max: last angle bin inside the jet cone (inverse_compton.jl:215); alpha_in /
 * n_in [n_nu <= 60]: energies (in m_e c^2) and number densities of the incoming photon field (photon_field!, :313-383: host table);
 * photon energies E_k = emin_mev * 10^(k / bins_per_dec); beam_area = 4 pi d_lum^2 jet_sph_frac.  Outputs (host): energy_erg[n_photon]
 * (may be NULL), emis[n_grid][n_photon] = observed energy flux per d(ln E) at Earth in erg / (s cm^2), floor 1e-99 (:285-308).
 * Dead code in the reference, followed as specification (include/mcs_ic.h lists where it cannot run as written). */
int mcs_photon_ic(mcs_ctx* ctx, const double* mom_edge_cgs, double mc_e, int j_max, int n_nu, const double* alpha_in, const double* n_in, int n_photon,
                  double emin_mev, double bins_per_dec, double beam_area, double* energy_erg, double* emis);

/* ---- observed shell spectra (K9): what an observer at Earth sees of one emission process -- the per-zone emission of a fold above
 * turned into a photon flux, shifted from the plasma frame of every zone into the ISM frame, summed over the zones of every photon
 * shell (the arithmetic of src/get_summed_emission.jl:37-413 as consumers.py restates it: S1-S6 there), on the device.
 * Each of the three folds above keeps its emis[n_grid][n_photon] in a buffer of the context that nothing else writes, one per
 * process, with a flag that records n_photon; a begin-species call, a write of the tally buffer and a photons sample of the ensemble
 * statistics clear the flags.
 * process: MCS_PHOTON_SYNCH, MCS_PHOTON_IC or MCS_PHOTON_PION.  All arrays are host arrays; the call looks nothing up itself:
 *   emis            [n_grid][n_photon], or NULL: what the last fold of that process left on the context (refused when its flag is
 *                   clear or records another n_photon)
 *   energy_div      [n_photon] the energies the energy flux is divided by (MeV for synchrotron and inverse Compton, erg for pion decay)
 *   energy_grid     [n_photon] the MeV grid of the Doppler step
 *   area            4 pi d_L^2 (synchrotron, pion decay; the inverse-Compton fold has its beam area inside already and ignores it)
 *   dlog, last_mid_ratio      the logarithmic bin width and 10^dlog as the host computes it
 *   cos_edge        [181] the boundaries of the 180 slices in cos(theta), -1 .. 1
 *   gam_ef, beta_ef, gam3_ef  [n_grid] each, zones 1..n_grid: the flow's Lorentz factor and speed against the ISM, and the host's gam^3
 *                   (a table on purpose: a power function and g*g*g differ in the last bit)
 *   shell_ends      [n_shells + 1] 1-based zone numbers, 0 = no zone: shell s holds zones shell_ends[s] .. shell_ends[s+1] - 1
 * out [n_shells + 1][n], n = n_photon - 1 (the last energy of a spectrum is dropped): photons per bin of every shell, then of all
 * shells, floor 1e-99; to the host (may be NULL), and kept on the device per process with a flag of its own (cleared like the others).
 * Definition, every operation a separate rounding, / and sqrt correctly rounded, E = energy_grid, z a zone, j an energy < n:
 *   1  flux  x = emis[z][j];  synchrotron: e = x / area, e = e > 1e-99 ? e : 1e-99, e = e > 1e-99 ? e / MeV : 1e-99;
 *            inverse Compton: e = x > 1e-99 ? x / MeV : 1e-99;  pion decay: e = x / area, e = e >= 1e-99 ? e : 1e-99   (MeV = 1.602176634e-6 erg)
 *            f = e <= 1e-99 ? 1e-99 : e / energy_div[j];   g = f > 1e-90 ? f * dlog : f
 *   2  frame inverse Compton: nb[z][j] = g.  Otherwise num_j = g / 180; mid_j = sqrt(E[j] E[j+1]) for j < n - 1, mid_(n-1) =
 *            mid_(n-2) * last_mid_ratio; fac_l = gam sqrt((1 - beta c_l)(1 - beta c_(l+1))); the target of (l, j) is the first m >= 1
 *            with E[m] >= mid_j * fac_l, and the pair counts if num_j > 1e-99 and m < n.  acc_b = the serial sum, starting from 1e-99,
 *            of num_j over the pairs with m - 1 = b, in ascending l and within l ascending j;  nb[z][b] = acc_b > 1e-95 ? acc_b * gam3 : 1e-99
 *   3  shell s with lo = shell_ends[s] >= 1 and hi = shell_ends[s+1] - 1 >= lo: a = the serial sum from 0 over z = lo .. hi of
 *            (nb[z][j] > 1e-95 ? nb[z][j] : 0); out[s][j] = a > 1e-99 ? a : 1e-99.  Otherwise out[s][j] = 1e-99
 *   4  out[n_shells][j]: the serial sum from 0 over s of (out[s][j] > 1e-99 ? out[s][j] : 0), then the same floor.
 * Step 2 is a scatter as written; the device gathers in the same order (no atomics: the same input gives the same bits).
 * The emission itself is not checked: a NaN is no flux (every comparison of step 1 is false for it), +infinity stays one.
 * Refused, with a message and nothing changed: a null context or table, a process outside the three, n_photon outside 3..256 (a
 * zone's tables live in LDS), n_shells outside 1..4096, a clear flag with emis = NULL, a non-finite or non-positive energy, area, dlog
 * or gam, last_mid_ratio not finite or below 1, beta outside [0, 1), gam3 or a slice boundary not finite, a boundary outside [-1, 1],
 * energies that decrease, a shell end outside 0 .. n_grid + 1. */
enum { MCS_PHOTON_SYNCH = 0, MCS_PHOTON_IC = 1, MCS_PHOTON_PION = 2 };
int mcs_photon_observe(mcs_ctx* ctx, int process, int n_photon, const double* emis, const double* energy_div, const double* energy_grid,
                       double area, double dlog, double last_mid_ratio, const double* cos_edge, const double* gam_ef, const double* beta_ef,
                       const double* gam3_ef, int n_shells, const int64_t* shell_ends, double* out);

/* ---- ensemble statistics (K8): per-word mean and standard error over the iterations of a fixed-profile run --------------------
 * With a fixed shock profile the iterations of a run are independent realisations.  An accumulator keeps, on the device, a running
 * mean and a sum of squared deviations M2 of every word of a SAMPLE vector, per slot; a slot takes species samples or iteration
 * samples, never both.  Create gives n_species_slots species slots (0 .. n_species_slots - 1; a driver uses slot i_ion - 1) and one
 * iteration slot (index n_species_slots).
 *
 * Species sample, taken at the end of a species, tally replicas folded in:
 *   1  words [psd, esc_flux) of the fp64 buffer: psd, therm_sf, therm_pf, esc_psd_up, esc_psd_down and the three flux vectors
 *   2  energy_recv_pool [n_grid]
 *   3  num_crossings [n_grid], converted to double (exact below 2^53)
 *   4  the marginals of psd, therm_sf, therm_pf, in that order, for each the momentum marginal [n_grid][nmom+2] (summed over the
 *      angle index) and then the angle marginal [n_grid][ntht+2] (summed over the momentum index); every word is the serial sum of
 *      its terms in ascending index order, starting from the first term.  (The variance of a marginal cannot be had from the
 *      per-cell variances, so the marginal itself is sampled.)
 * Iteration sample, taken at the end of an iteration: words [esc_flux, energy_recv_pool) and then [scalars, total).  The sections
 * the transport never resets -- esc_flux, esc_energy_eff, esc_num_eff, spectra_coupled, spectra_sf, spectra_pf -- enter as their
 * growth since the snapshot of the begin-iteration call below; weight_coupled, energy_transfer_pool, scalars and the two arrays
 * indexed by iteration (px_esc_feb, energy_esc_feb, whose statistics mean nothing) enter as they stand.
 *
 * Update of a slot by a sample x, per word, no fused operation:   n += 1; d = x - mean; mean = mean + d / n; M2 = M2 + d * (x - mean)
 * Merge of slot b into slot a (Chan), per word:                   n = na + nb; d = mb - ma; mean = ma + d * (nb / n);
 *                                                                 M2 = (qa + qb) + (d * d) * (na * nb / n)
 * (all of n, na, nb as doubles); an empty b changes nothing, an empty a takes b as it is.
 * Device memory: two vectors of the sample length per slot -- for a species slot about twice the tally buffer -- plus one marginal
 * vector and one snapshot of [esc_flux, energy_recv_pool).
 *
 * The contexts handed to these calls may be any context on the accumulator's device with the accumulator's tally layout (species
 * that ran on a secondary context are sampled there).  Work is queued on that context's stream, after what the accumulator's
 * previous operation queued (an event orders them, as in the accumulate-tallies call); merge, read and load-mean of a source
 * accumulator are ordered the same way.  Only count and read synchronise with the host.  The `home` context of create gives the
 * device, the layout and the stream that merge and read use; it must outlive the accumulator.  The caller serialises the calls on
 * one accumulator, and each with the calls on the context it names.
 * Refused, with a message and nothing changed: a null argument, a slot out of range, a species sample for the iteration slot or
 * the reverse, a context on another device or with another layout, a merge of an accumulator into itself or of accumulators with
 * different slots, an iteration sample without a snapshot of that context taken since the last one, a standard error with n < 2. */
typedef struct mcs_ens mcs_ens;
/* Offsets and lengths, in doubles, of the parts of the two sample vectors, and where the parts lie in the fp64 tally buffer. */
typedef struct mcs_ens_layout {
  int64_t sp_tallies, sp_tallies_n;               /* part 1: sample word sp_tallies + w is buffer word tally_sp_first + w */
  int64_t sp_recv_pool, sp_recv_pool_n;           /* part 2 */
  int64_t sp_num_crossings, sp_num_crossings_n;   /* part 3 */
  int64_t sp_psd_mom, sp_psd_tht, sp_therm_sf_mom, sp_therm_sf_tht, sp_therm_pf_mom, sp_therm_pf_tht;   /* part 4 */
  int64_t sp_marg_mom_n, sp_marg_tht_n;           /* n_grid * (nmom+2), n_grid * (ntht+2) */
  int64_t sp_total;
  int64_t it_sums, it_sums_n;                     /* sample word it_sums + w is buffer word tally_it_first + w */
  int64_t it_scalars, it_scalars_n;
  int64_t it_total;
  int64_t tally_sp_first, tally_it_first, tally_recv_pool, tally_scalars;   /* psd, esc_flux, energy_recv_pool, scalars of mcs_layout */
} mcs_ens_layout;
int mcs_ens_get_layout(const mcs_params* p, mcs_ens_layout* out);      /* needs no GPU */
int mcs_ens_create(mcs_ctx* home, int n_species_slots, mcs_ens** out);
int mcs_ens_destroy(mcs_ens* ens);
/* snapshot of src's [esc_flux, energy_recv_pool), the base of the next iteration sample from src */
int mcs_ens_begin_iteration(mcs_ens* ens, mcs_ctx* src);
int mcs_ens_add_species(mcs_ens* ens, mcs_ctx* src, int slot);
int mcs_ens_add_iteration(mcs_ens* ens, mcs_ctx* src);
/* every slot of src merged into the same slot of dst; src is left as it is */
int mcs_ens_merge(mcs_ens* dst, mcs_ens* src);
int mcs_ens_count(mcs_ens* ens, int slot, int64_t* n);
/* words [first, first + count) of a slot's sample vector into host[0 .. count): what = 0 the mean, 1 M2, 2 the standard error of
 * the mean, sqrt(M2 / (n (n - 1))) */
int mcs_ens_read(mcs_ens* ens, int slot, int what, int64_t first, int64_t count, double* host);
/* The mean of a species slot written into dst's per-species sections: parts 1 and 2 into the fp64 buffer, part 3, rounded to
 * nearest, into num_crossings.  The consumers above then run unchanged on the ensemble-mean histograms (what a two-dimensional
 * consumer call left on the device is dropped). */
int mcs_ens_load_mean(mcs_ens* ens, int slot, mcs_ctx* dst);
/* A summary of word ranges of a slot, reduced on the device: what a stop rule ("tally trigger") needs of the error bars without
 * reading the vectors.  For one range [first, first + count) of a slot with n >= 2 samples, every operation a separate rounding:
 *   finite word    mean[w] and M2[w] are both finite; n_nonfinite counts the others, which take part in nothing else
 *   amax           the maximum of |mean[w]| over the finite words; 0 for an empty range
 *   selected word  a finite word with |mean[w]| > 0 and |mean[w]| >= floor_frac * amax; n_selected counts them
 *   per selected word   se = sqrt(M2[w] / (n (n - 1))), the denominator (double)n * (double)(n - 1) as in the read call;
 *                       rel = se / |mean[w]|         (sqrt and / correctly rounded)
 *   max_rel        the maximum of rel (0 when nothing is selected); argmax: the lowest w - first that attains it, -1 when
 *                  nothing is selected
 *   n_over         the selected words with rel > tol
 *   sum_se, sum_abs_mean, sum_rel2   the sums over the selected words of se, |mean| and rel * rel
 * One call serves all its ranges (at most 256; they may overlap and start at any word) and waits for the device once; it is
 * ordered like the read call: on the home context's stream, after what the accumulator queued last.  Two sweeps over a range --
 * the means for amax, then means and M2 -- each thread over its words in ascending order, the threads of a block joined by
 * shuffles and LDS, one partial per block in a scratch buffer of the accumulator (allocated at the first call, sized by the
 * largest), the partials of a range joined in index order: no atomics, and the same state gives the same bits in every field.
 * The three sums are sums of non-negative terms in an order the call fixes: within n_selected * 2^-53 relative of the exact sum.
 * (A word with a finite mean and a non-finite M2 that carries a range's largest |mean| is seen only by the second sweep; the
 * call then repeats that sweep with the amax of the finite words and waits a second time.)
 * n_ranges = 0 does nothing and returns 0.  Refused, with a message, nothing changed and nothing queued: a null argument, a slot
 * out of range, a slot with n < 2, n_ranges outside 0..256, a range outside the slot's vector or with a negative count,
 * floor_frac not in [0, 1] (NaN included), tol negative or NaN. */
typedef struct mcs_ens_range   { int64_t first, count; double floor_frac, tol; } mcs_ens_range;
typedef struct mcs_ens_summary { double amax, max_rel, sum_se, sum_abs_mean, sum_rel2;
                                 int64_t n_selected, n_over, n_nonfinite, argmax; } mcs_ens_summary;
int mcs_ens_summarize(mcs_ens* ens, int slot, int n_ranges, const mcs_ens_range* ranges, mcs_ens_summary* out);
/* The same summary of the MERGE of several accumulators, without forming it: what a stop rule needs when every context of an
 * overlapped run owns an accumulator (a scratch accumulator to merge them into would cost two more vectors per slot, and every
 * check would rewrite it whole).  For every word w of the slot the merged pair (mean, M2) is the left fold of the merge formula
 * above over the accumulators of the list that have samples in this slot, in list order, every operation a separate rounding:
 *   the first non-empty accumulator gives (m, q, na); each further non-empty accumulator b merges in with
 *   n = na + nb; d = mb - m; m = m + d * f_mean; q = (q + qb) + (d * d) * f_m2; na = n,
 *   f_mean = (double)nb / n and f_m2 = (double)na * (double)nb / n computed on the host exactly as the merge call does;
 *   an empty accumulator is skipped (an empty b changes nothing, an empty a takes b).
 * The total count n = sum of the n_k is returned in *n_total; the denominator is (double)n * (double)(n - 1).  On these merged
 * words the summary is word for word that of mcs_ens_summarize: a word is finite or not by its MERGED mean and M2 (a word finite in
 * every accumulator whose merge is not -- d * d overflows -- is counted in n_nonfinite), and the repeated second sweep applies
 * when a finite merged mean with a non-finite merged M2 carried a range's amax.  Each word's fold is made in registers; no
 * accumulator is changed and nothing but the block partials is written.  Which words a thread sees, in which order, and how
 * threads, waves, blocks and partials are joined depends on the ranges alone, so every field, the three sums included, has the
 * bits that merging the same accumulators in the same order into an empty accumulator with mcs_ens_merge and calling
 * mcs_ens_summarize on it gives; with n_ens = 1 the result is that of mcs_ens_summarize.
 * Work is queued on the stream of ens[0]'s home context, after what every accumulator of the list queued last; the call waits for
 * the device before it returns.  Scratch (parameters, partials, pinned results) is ens[0]'s, shared with mcs_ens_summarize.
 * n_ranges = 0 returns 0 and still writes *n_total.  The count is checked before that, here and not in mcs_ens_summarize: a total
 * below 2 is refused even with n_ranges = 0, where mcs_ens_summarize returns 0; the two calls agree from two samples on.  Refused, with a message, nothing changed and nothing queued: a null argument
 * or null entry, n_ens outside 1..MCS_ENS_MAX_MERGED, the same accumulator twice, accumulators on different devices or with
 * different slots or layouts (the conditions of mcs_ens_merge), a slot out of range, a total count below 2, and every condition on
 * the ranges that mcs_ens_summarize refuses. */
#define MCS_ENS_MAX_MERGED 8
int mcs_ens_summarize_merged(int n_ens, mcs_ens* const* ens, int slot, int n_ranges, const mcs_ens_range* ranges,
                             mcs_ens_summary* out, int64_t* n_total);

/* ---- products sample: error bars of what a run publishes -- dN/dp in the three frames, the pressures and the energy density of
 * ion_finalize, the spectral slope.  They are non-linear in the tallies (a normalisation, a rebinning between frames, a fit), so
 * their error bars cannot be had from the per-cell ones: they are sampled once per iteration.
 * Every species slot s has a companion PRODUCTS slot, MCS_ENS_PRODUCTS(s) in the count, read, summarize and summarize-merged
 * calls.  Its two vectors are allocated at its first sample: an accumulator that never takes one costs no more memory and behaves
 * as before.  The sample holds 3 n_grid NM + 6 n_grid doubles (NM = nmom + 2), mcs_ens_products_layout:
 *   dNdp_sf, dNdp_pf, dNdp_isf                     [n_grid][NM] each: frames 0, 1, 2 of the last mcs_dndp_cr on the context, as that
 *                                                  call left them on the device
 *   P_psd_par, P_psd_perp, energy_density_psd      [n_grid] each: the last mcs_thermo_calcs on the context
 *   slope_sf, slope_pf, slope_isf                  [n_grid] each: per zone the least-squares slope of log10 dN/dp against
 *                                                  log10 p over the slope window
 * Slope of frame m in zone z, over the window bins l_lo <= l < l_hi with x_l = x_log[l]: bin l is VALID if
 * d = dNdp[m][z][l] > 1.0e-99 (the consumers' floor marks an empty bin); y_l = log10(d), the deterministic log10 of
 * include/mcs_math.h.  With the k valid bins in ascending l, every operation a separate rounding, serial sums that start from 0:
 *   xbar = (sum x_l) / k;  ybar = (sum y_l) / k;  Sxx = sum (x_l - xbar)(x_l - xbar);  Sxy = sum (x_l - xbar)(y_l - ybar);
 *   slope = Sxy / Sxx
 * k < 3 gives a quiet NaN.  The word's mean then stays non-finite: a summary counts it in n_nonfinite, and a stop rule over it is
 * never met -- a slope trigger belongs on zones that the accelerated population reaches.  It is the slope of dN/dp, about -2.2
 * behind a strong shock, not the index of f(p).
 * mcs_ens_set_slope_window: x_log is a host array [nmom+1], log10 of each momentum bin's centre, copied to the device; the window
 * needs 0 <= l_lo, l_hi <= nmom + 1, l_hi - l_lo >= 3 and finite x_log.  It may be called again until the first products sample of
 * any slot and is refused afterwards, so that the samples of a slot stay comparable; the call waits for its copy.
 * mcs_ens_add_products: one sample from what mcs_dndp_cr AND mcs_thermo_calcs left on src.  Refused unless both have run on src
 * since its last mcs_begin_species and since the last products sample taken from it (no other call writes the buffer they leave
 * their results in), without a slope window, and for what mcs_ens_add_species refuses.  Queued on src's stream behind the
 * accumulator's event, no host synchronisation.
 * mcs_ens_merge merges the products slots that src has, allocating in dst where needed; a dst without a window takes src's.  A
 * merge, or a merged summary of a products slot, of accumulators that both have a window is refused when the windows differ in a
 * bound or in the bits of any x_log word.  A products slot that was never sampled has count 0, and its reads are refused.
 * mcs_ens_load_mean takes species slots only. */
#define MCS_ENS_PRODUCTS(s) ((s) | (1 << 30))
typedef struct mcs_ens_products_layout {
  int64_t dNdp_sf, dNdp_pf, dNdp_isf;                       /* offsets, in doubles */
  int64_t dNdp_n;                                           /* n_grid * (nmom+2): the length of each of the three */
  int64_t P_psd_par, P_psd_perp, energy_density_psd;
  int64_t slope_sf, slope_pf, slope_isf;
  int64_t zone_n;                                           /* n_grid: the length of each of the six */
  int64_t total;
} mcs_ens_products_layout;
int mcs_ens_products_get_layout(const mcs_params* p, mcs_ens_products_layout* out);      /* needs no GPU */
int mcs_ens_set_slope_window(mcs_ens* ens, int l_lo, int l_hi, const double* x_log);
int mcs_ens_add_products(mcs_ens* ens, mcs_ctx* src, int species_slot);

/* ---- escape sample: error bars of the spectra of the escaping particles.  Every species slot s has a third companion, the ESCAPE
 * slot MCS_ENS_ESCAPE(s), which behaves as its products slot does in the count, read, merge, summarize, summarize-merged and compare
 * calls (vectors allocated at the first sample; reads of a slot that never took one are refused).  The sample holds
 * 6 NM + 12 doubles (NM = nmom + 2), mcs_ens_escape_layout:
 *   dNdp    [2][3][NM]  door, frame: the last mcs_dndp_esc on the context, as that call left it on the device
 *   number  [2][3]      likewise
 *   slope   [2][3]      the slope of each dNdp row over the accumulator's slope window, by the rule of the products sample
 *                       (valid bin: dN/dp > 1e-99; fewer than three valid bins: NaN)
 * mcs_ens_add_escape: refused unless mcs_dndp_esc has run on src since its last mcs_begin_species and since the last escape sample
 * taken from it, without a slope window, and for what mcs_ens_add_species refuses.  Queued on src's stream behind the accumulator's
 * event, no host synchronisation.  The slope window is fixed from the first products OR escape sample on, and the window rules of
 * merge, merged summary and comparison hold for escape slots as for products slots. */
#define MCS_ENS_ESCAPE(s) ((s) | (1 << 27))
typedef struct mcs_ens_escape_layout {
  int64_t dNdp, number, slope;                              /* offsets, in doubles */
  int64_t row_n;                                            /* nmom + 2: the length of a dNdp row; number and slope have 6 words */
  int64_t total;
} mcs_ens_escape_layout;
int mcs_ens_escape_get_layout(const mcs_params* p, mcs_ens_escape_layout* out);      /* needs no GPU */
int mcs_ens_add_escape(mcs_ens* ens, mcs_ctx* src, int species_slot);

/* ---- angles sample: error bars of the pitch-angle distributions.  Every species slot s has a fourth companion, the ANGLES slot
 * MCS_ENS_ANGLES(s), which behaves as its escape slot does in the count, read, merge, summarize, summarize-merged and compare calls
 * (vectors allocated at the first sample; reads of a slot that never took one are refused).  The accumulator holds the momentum
 * windows of its angles samples, mcs_ens_set_angle_windows (the rules of mcs_angle_dist): they may be set again until the first
 * angles sample of any slot and are fixed from then on.  With rows = 3 * n_grid * n_win and row = (frame * n_grid + zone) * n_win +
 * window, the sample holds rows * (ntht + 5) doubles, mcs_ens_angles_layout:
 *   dist     [rows][ntht+2]   the last mcs_angle_dist on the context, as that call left it on the device
 *   number   [rows]           likewise
 *   mean_mu  [rows]           moments[.][0] of that call
 *   mean_mu2 [rows]           moments[.][1]
 * mcs_ens_add_angles: refused unless mcs_angle_dist has run on src since its last mcs_begin_species and since the last angles
 * sample taken from it, without windows, where that call's windows differ from the accumulator's, and for what
 * mcs_ens_add_species refuses.  Queued on src's stream behind the accumulator's event, no host synchronisation.
 * A merge, a merged summary or a comparison of accumulators whose windows differ is refused; a destination without windows takes
 * the source's.  mcs_ens_load_mean takes species slots only. */
#define MCS_ENS_ANGLES(s) ((s) | (1 << 26))
typedef struct mcs_ens_angles_layout {
  int64_t dist, number, mean_mu, mean_mu2;                  /* offsets, in doubles */
  int64_t row_n;                                            /* ntht + 2: the length of a dist row */
  int64_t rows;                                             /* 3 * n_grid * n_win */
  int64_t total;
} mcs_ens_angles_layout;
int mcs_ens_angles_get_layout(const mcs_params* p, int n_win, mcs_ens_angles_layout* out);   /* needs no GPU */
int mcs_ens_set_angle_windows(mcs_ens* ens, int n_win, const int32_t* l_lo, const int32_t* l_hi);
int mcs_ens_add_angles(mcs_ens* ens, mcs_ctx* src, int species_slot);

/* ---- tcuts sample: error bars of the time-cut spectra.  Every species slot s has a fifth companion, the TCUTS slot
 * MCS_ENS_TCUTS(s), which behaves as its escape slot does in the count, read, merge, summarize, summarize-merged and compare calls
 * (vectors allocated at the first sample; reads of a slot that never took one are refused).  The sample is the last
 * mcs_tcut_spectra on the context as that call left it on the device, in its layout (mcs_ens_tcuts_get_layout gives that of
 * mcs_tcut_get_layout): spectrum [nt][nmom+2], weight, number, mean_log_p [nt], quantile [3][nt], index [3].
 * n_tcuts is fixed by the accumulator's first tcuts sample (or by a merge into an accumulator that has none): a later sample,
 * merge, merged summary or comparison with another n_tcuts is refused.
 * mcs_ens_add_tcuts: refused unless mcs_tcut_spectra has run on src since its last mcs_begin_species and since the last tcuts
 * sample taken from it, and for what mcs_ens_add_species refuses.  Queued on src's stream behind the accumulator's event, no host
 * synchronisation.  mcs_ens_load_mean takes species slots only. */
#define MCS_ENS_TCUTS(s) ((s) | (1 << 25))
typedef mcs_tcut_layout mcs_ens_tcuts_layout;
int mcs_ens_tcuts_get_layout(const mcs_params* p, int n_tcuts, mcs_ens_tcuts_layout* out);    /* needs no GPU */
int mcs_ens_add_tcuts(mcs_ens* ens, mcs_ctx* src, int species_slot);

/* ---- profile sample: error bars of the predicted shock profile.  With a FIXED profile every iteration's mcs_profile_update is an
 * independent sample of the profile that smooth_grid_par would write; its mean and standard error say how far the current profile is
 * from self-consistency.  The PROFILE slot MCS_ENS_PROFILE, one per accumulator like the source slot, behaves as the source slot does
 * in the count, read, merge, summarize, summarize-merged and compare calls (vectors allocated at the first sample; reads of a slot
 * that never took one are refused).  The sample is the last mcs_profile_update on the context as that call left it on the device, in
 * its layout (mcs_ens_profile_get_layout gives that of mcs_profile_get_layout): ten rows of n_grid doubles, then eight scalars.
 * The accumulator keeps the SETTINGS of its first sample's mcs_profile_in -- the fields F_px_upstream .. i_trans; the q history and
 * the tables are not kept -- (or takes them in a merge into an accumulator that has none): a later sample, merge, merged summary or
 * comparison whose settings differ in any bit is refused.
 * mcs_ens_add_profile: refused unless mcs_profile_update has run on src since its last mcs_begin_species, tally write and profile
 * sample.  Queued on src's stream behind the accumulator's event, no host synchronisation.  mcs_ens_load_mean takes species slots only. */
#define MCS_ENS_PROFILE (1 << 24)
typedef mcs_profile_layout mcs_ens_profile_layout;
int mcs_ens_profile_get_layout(const mcs_params* p, mcs_ens_profile_layout* out);    /* needs no GPU */
int mcs_ens_add_profile(mcs_ens* ens, mcs_ctx* src);

/* ---- detectors sample: error bars of the detector spectra.  Every species slot s has a sixth companion, the DETECTORS slot
 * MCS_ENS_DETECTORS(s), which behaves as its tcuts slot does in the count, read, merge, summarize, summarize-merged and compare
 * calls (vectors allocated at the first sample; reads of a slot that never took one are refused).  The sample is the last
 * mcs_detector_spectra on the context as that call left it on the device, in its layout (mcs_ens_detectors_get_layout gives that of
 * mcs_detector_get_layout): spectrum, dndp [2][nd][nmom+2], number, mean_log_p [2][nd], quantile [3][2][nd], slope [2][nd],
 * gradient [nmom+2].
 * The accumulator keeps the SETTINGS of its first detectors sample -- nd, the window l_lo, l_hi, and the bits of x_unit and of
 * x_spec[0..nd) -- (or takes them in a merge into an accumulator that has none): a later sample, merge, merged summary or comparison
 * whose settings differ is refused.
 * mcs_ens_add_detectors: refused unless mcs_detector_spectra has run on src since its last mcs_begin_species and since the last
 * detectors sample taken from it, and for what mcs_ens_add_species refuses.  Queued on src's stream behind the accumulator's event,
 * no host synchronisation.  mcs_ens_load_mean takes species slots only. */
#define MCS_ENS_DETECTORS(s) ((s) | (1 << 23))
typedef mcs_detector_layout mcs_ens_detectors_layout;
int mcs_ens_detectors_get_layout(const mcs_params* p, int n_det, mcs_ens_detectors_layout* out);    /* needs no GPU */
int mcs_ens_add_detectors(mcs_ens* ens, mcs_ctx* src, int species_slot);

/* ---- photons sample: error bars of the photon spectra at Earth.  A shell spectrum is a sum over zones, slices and processes: its
 * variance does not follow from per-cell variances, so the spectrum itself is sampled once per iteration, from what
 * mcs_photon_observe left on a context.
 * Every species slot s has a second companion, the PHOTONS slot MCS_ENS_PHOTONS(s), in the count, read, summarize, summarize-merged
 * and compare calls.  Like the products slot it is allocated at its first sample: an accumulator that never takes one costs no
 * more memory and behaves as before.
 * mcs_ens_set_photon_layout fixes the sample vector: n_shells shells (rows = n_shells + 1, the last row all shells), the energy words
 * per process n_synch, n_ic, n_pion (the n = n_photon - 1 of mcs_photon_observe), their offsets start_* on the common energy grid
 * and its length n_pts (the stock run: 179, 139, 119 at 0, 110, 130 of 250).  It needs 1 <= n_shells <= 4096, 1 <= n <= 255 and
 * 0 <= start, start + n <= n_pts <= 65536; it may be called again until the first photons sample (or merge) of any slot and is
 * refused afterwards.  The vector has four sections, mcs_ens_photons_layout:
 *   synch, ic, pion   [rows][n] each: the last mcs_photon_observe of that process on the context; a process not observed there since
 *                     the last begin-species call, tally write or photons sample enters as 1e-99 throughout
 *   total             [rows][n_pts]: total[s][t], s < n_shells, starts at 1e-99 and adds (x > 1e-99 ? x : 0) of x = pion[s][t - start_pion],
 *                     synch[s][t - start_synch], ic[s][t - start_ic], in that order, where t lies in the process' window; the last
 *                     row is the serial sum from 0 over s, ascending, of total[s][t] as they stand, floors included
 * mcs_ens_add_photons: one sample; the update is that of every slot.  Refused unless the context holds at least one observation,
 * when an observation's shells or energy words differ from the layout, without a layout, and for what mcs_ens_add_products refuses.
 * Queued on src's stream behind the accumulator's event, no host synchronisation; it clears the context's photon flags.
 * mcs_ens_merge merges the photons slots that src has, allocating in dst where needed; a dst without a layout takes src's.  A merge,
 * a comparison or a merged summary of a photons slot of accumulators that both have a layout is refused when the layouts differ.  A
 * photons slot that was never sampled has count 0, and its reads are refused.  mcs_ens_load_mean takes species slots only. */
#define MCS_ENS_PHOTONS(s) ((s) | (1 << 29))
typedef struct mcs_ens_photons_layout {
  int64_t synch, ic, pion, total_section;                   /* offsets, in doubles */
  int64_t n_synch, n_ic, n_pion, n_pts;                     /* the row length of each section */
  int64_t rows;                                             /* n_shells + 1 */
  int64_t total;
} mcs_ens_photons_layout;
int mcs_ens_photons_get_layout(int n_shells, int n_synch, int n_ic, int n_pion, int n_pts, mcs_ens_photons_layout* out);      /* needs no GPU */
int mcs_ens_set_photon_layout(mcs_ens* ens, int n_shells, int n_synch, int n_ic, int n_pion, int start_synch, int start_ic, int start_pion,
                              int n_pts);
int mcs_ens_add_photons(mcs_ens* ens, mcs_ctx* src, int species_slot);

/* ---- source sample: error bars of the photon spectrum summed over species.  An observer sees one spectrum from the source; the
 * species of one iteration share a shock profile and an energy-transfer pool and are correlated, so the variance of the sum is not
 * the sum of the species' variances: the sum itself is sampled, once per iteration.
 * The SOURCE slot MCS_ENS_PHOTONS_ALL, one per accumulator and no companion of a species slot, has exactly the photons layout above
 * -- synch | ic | pion | total, the same offsets, the same mcs_ens_photons_layout -- in the count, read, summarize, summarize-merged,
 * compare and merge calls.  The accumulator keeps a PENDING vector of layout.total doubles on the device, allocated at the first
 * deposit, and on the host the species slots deposited since the last take, in call order; the two vectors of the source slot are
 * allocated at its first sample or merge.  An accumulator that never deposits allocates nothing more and behaves as before.
 * mcs_ens_add_photons_deposit: everything mcs_ens_add_photons does -- the species' photons slot ends with the same bits -- and, in
 * the same kernel launch, the deposit of the sample into the pending vector.  A thread forms its word x[w] of the species' sample
 * once, makes the update of the species' slot, and then, every operation a separate rounding (no fused multiply-add):
 *   the first deposit since the last take    pending[w] = 1.0e-99 + (x[w] > 1.0e-99 ? x[w] : 0.0)       (pending[w] is not read)
 *   a later one                              pending[w] = pending[w] + (x[w] > 1.0e-99 ? x[w] : 0.0)
 * uniformly over the four sections, the all-shells rows included: the source's all-shells row is the sum over species of the
 * species' all-shells rows (each the sum over its shells), not a sum over the source's shell rows.  The deposit order is the call
 * order.  Queued on src's stream behind the accumulator's event, no host synchronisation; it clears the context's photon flags.
 * Refused, with nothing changed (species slot, pending vector, flags, bookkeeping): everything mcs_ens_add_photons refuses, and a
 * species slot already deposited since the last take.
 * mcs_ens_add_photons_all: the take -- one sample x[w] = pending[w] into the source slot with the update of every slot, on the home
 * context's stream behind the accumulator's event; the deposits are then forgotten.  Refused with no deposit pending.  It fixes the
 * photon layout like a photons sample.
 * mcs_ens_drop_pending_photons: forgets the deposits (host bookkeeping only: the next first deposit overwrites the vector); returns 0
 * also when nothing is pending.  A run that raised in mid-iteration calls it so that the next iteration starts clean.
 * mcs_ens_merge merges the source slot like a photons slot (allocating in dst; a dst without a layout takes src's); pending deposits
 * are not merged and do not hinder a merge.  A source slot that was never sampled has count 0, and its reads are refused.  The
 * refusals of differing layouts apply as to the photons slots.  mcs_ens_compare takes it against another source slot only: it is a
 * kind of its own, and against a species' photons slot the slots "differ in kind".  mcs_ens_load_mean refuses it. */
#define MCS_ENS_PHOTONS_ALL (1 << 28)
int mcs_ens_add_photons_deposit(mcs_ens* ens, mcs_ctx* src, int species_slot);
int mcs_ens_add_photons_all(mcs_ens* ens);
int mcs_ens_drop_pending_photons(mcs_ens* ens);

/* ---- comparison of two slots: does run B agree with run A within their error bars?  Per-word z-scores and their chi-square,
 * reduced on the device.  Slot slot_a of accumulator a (A, n_a >= 2 samples) against slot slot_b of b (B, n_b >= 2): two slots of
 * the same kind and length -- both species slots, both iteration slots or both products slots -- of accumulators on one device
 * with one tally layout.  For every word w of a range [first, first + count), every operation a separate rounding, sqrt and /
 * correctly rounded as in mcs_ens_summarize (ma, qa: mean and M2 of A; mb, qb: of B):
 *   va = qa[w] / ((double)n_a * (double)(n_a - 1))      vb likewise      (the variance of each mean)
 *   s2 = va + vb            d = ma[w] - mb[w]           scale = max(|ma[w]|, |mb[w]|)
 *   finite word      ma, qa, mb, qb, d and s2 are all finite; n_nonfinite counts the others, which take part in nothing else
 *   amax             the maximum of scale over the finite words; 0 for an empty range
 *   selected word    a finite word with scale > 0 and scale >= floor_frac * amax; n_selected counts them
 *   degenerate word  a selected word with s2 == 0 and d != 0: counted in n_degenerate, in sum_abs_diff and sum_scale, nothing else
 *   z                0 for a selected word with s2 == 0 and d == 0; d / sqrt(s2) for every other selected word
 * Over the selected words that are not degenerate:
 *   max_abs_z        the maximum of |z| (0 when there is none); argmax: the lowest w - first that attains it, -1 when there is none
 *   n_over           the words with |z| > zcut
 *   sum_z, sum_abs_z, sum_z2     the sums of z, |z| and z * z; sum_z2 is the chi-square
 * Over all selected words:
 *   sum_abs_diff, sum_scale      the sums of |d| and scale
 * With few samples z follows Welch's t and not a normal law: under the null E[z^2] = nu / (nu - 2) with nu between
 * min(n_a, n_b) - 1 and n_a + n_b - 2, so a threshold is best calibrated on a null pair (two runs of one configuration over
 * different iteration numbers).
 * One call serves all its ranges (at most 256; they may overlap and start at any word) and waits for the device once.  a == b is
 * allowed when the slots differ (protons against He).  Work is queued on the stream of a's home context, after what both
 * accumulators queued last; neither accumulator is changed; scratch is a's, shared with the summaries.
 * Two sweeps over a range, both of whole (mean, M2) pairs of A and B: whether a word is finite depends on all four of its words,
 * so the first sweep takes amax over exactly the words the second calls finite, and no sweep is ever repeated.  Which words a
 * thread sees and in which order, and how threads, waves, blocks and partials join, is the summary's walk and depends on the
 * ranges alone: no atomics, the same state gives the same bits in every field, equal |z| keep the lower word at every join.
 * Swapping A and B leaves the bits of every field as they are, except that sum_z changes its sign bit (unless it is zero).
 * sum_abs_z, sum_z2, sum_abs_diff and sum_scale are sums of non-negative terms: within n_selected * 2^-53 relative of the exact
 * sum; sum_z within n_selected * 2^-53 * sum_abs_z of it.
 * n_ranges = 0 does nothing and returns 0.  Refused, with a message, nothing changed and nothing queued: a null argument, a slot
 * out of range, the same slot of the same accumulator, accumulators on different devices or with different layouts, slots of
 * different kind or length, n_ranges outside 0..256, a products slot that never took a sample, products slots of accumulators
 * whose slope windows differ in a bound or in the bits of any x_log word (the condition of mcs_ens_merge), either count below 2,
 * a range outside the slot's vector or with a negative count, floor_frac not in [0, 1] (NaN included), zcut negative or NaN. */
typedef struct mcs_ens_cmp_range  { int64_t first, count; double floor_frac, zcut; } mcs_ens_cmp_range;
typedef struct mcs_ens_difference { double amax, max_abs_z, sum_z, sum_abs_z, sum_z2, sum_abs_diff, sum_scale;
                                    int64_t n_selected, n_over, n_nonfinite, n_degenerate, argmax; } mcs_ens_difference;
int mcs_ens_compare(mcs_ens* a, int slot_a, mcs_ens* b, int slot_b, int n_ranges, const mcs_ens_cmp_range* ranges,
                    mcs_ens_difference* out);

/* ---- test / measurement hooks ------------------------------------------- */
/* evaluate device math/RNG primitives (bit-parity tests): fn ids in mcs_fn */
enum mcs_fn { MCS_FN_SIN = 0, MCS_FN_COS, MCS_FN_ASIN, MCS_FN_ACOS, MCS_FN_ATAN2, MCS_FN_LOG10,
              MCS_FN_MOD2PI, MCS_FN_SQRT, MCS_FN_DIV, MCS_FN_HYPOT1, MCS_FN_UNIFORM,
              /* The forms the transport kernel itself runs, evaluated by a kernel inside ITS translation unit (mcs_k_eval_hot in
               * csrc/mcs_transport.hip: MCS_DEVICE_FAST_SQRT, the kernel's own division helpers and coefficient tables); the codes
               * above are evaluated in csrc/mcs_population.hip, the build of K3.  SQRT_FAST / SQRT_NN: mcsm::sqrt_ / sqrt_nn_;
               * SQRT_NN_K, ASIN_TK, MOD2PI_K: the tail loop's spellings; HYPOT1_HOT: mcsm::hypot1; FDIV: fdiv(a, b);
               * DIV_R / DIV_R2: div_r(a, b, r) and div_r(2 a, b, r) with ONE r = rcp_refined(b) per lane (DIV_R2 must be exactly
               * twice DIV_R); SIN_T / COS_T: the two outputs of mcsm::sincos_t; ASIN_T: mcsm::asin_t. */
              MCS_FN_SQRT_FAST, MCS_FN_SQRT_NN, MCS_FN_SQRT_NN_K, MCS_FN_HYPOT1_HOT, MCS_FN_FDIV, MCS_FN_DIV_R, MCS_FN_DIV_R2,
              MCS_FN_SIN_T, MCS_FN_COS_T, MCS_FN_ASIN_T, MCS_FN_ASIN_TK, MCS_FN_MOD2PI_K,
              MCS_FN_COUNT };
/* an fn outside the enum is an error (with a message), not a result */
int mcs_eval_fn(mcs_ctx* ctx, int fn, int64_t n, const double* a, const double* b, double* out);
/* One scatter (src/scattering.jl:29-101) of n particle states, in the spelling `form` of the transport kernel:
 *   0  refresh_scatter + scattering(): the common pass of every K1 kernel;
 *   1  refresh_scatter_k, scatter_draws, scatter_cone, scattering_rest: the in-line loss of the lossy kernel and the tail ring;
 *   2  the same with scattering_rest_k and the TailK constants: the tail loop.
 * in [n][10]: key (the 64 bits of the slot are the particle's RNG key, not a number), draw index (even, < 2^32), aa, gyro_denom,
 * ptot_pf, gam_pf, xn_per, pb_pf, p_perp, phi.  out [n][5]: pb_pf, p_perp, phi, gyro_period, cos_max.  pe_crit, game_crit and eta_mfp
 * are those of the context's mcs_params.  All three forms must equal the oracle bit for bit (tests/test_gpu_math_forms.py). */
int mcs_eval_scatter(mcs_ctx* ctx, int form, int64_t n, const double* in, double* out);
/* The pcut bookkeeping (K2: compaction of the status bytes, pcut_finalize, new_pcut; src/cuts.jl:34-124) on the CALLER's status bytes
 * and saved states, through the launchers and the launch geometry of mcs_run_pcut*, in one of three forms:
 *   0  host-sized (mcs_run_pcut + mcs_new_pcut [+ mcs_saved_export / mcs_saved_gidx]): bytes equal to `match` count as saved, i_mult given;
 *   1  device-sized (one pcut of mcs_run_pcuts_fused): n is read on the device, the grids are sized for cap_n, i_mult from n_target;
 *      ctr_work / ctr_saved are the launch's two counter words before the call (ctr_saved: the transport kernel's own count);
 *   2  late (the late group of mcs_run_pcuts_pipelined; fp64 state only): status 5 counts, the children go behind n_main_next others.
 * In: l_save[cap_n] and saved[cap_n] (cap_n >= n; what lies beyond n is stale and must be ignored), src_fill in [0, cap_n): every
 * word of src[] before the call.  The target holds guard + out_cap + guard particles, every byte 0xA5 before the split; the
 * children are written from particle `guard` on (form 2: guard + n_main_next).  A call whose children would not fit is refused.
 * export_mode (form 0): 0 none, 1 the global indices only, 2 indices and states, into buffers of exp_cap (>= n_saved) entries whose
 * bytes are 0xA5 before the call (mode 1 returns exp_f64 / exp_meta, where given, as they were filled); the global index of local particle j is exp_gin[j], or exp_first + j * exp_stride when exp_gin is NULL.
 * Out (host arrays of the caller): src[cap_n]; out_f64[8][guard + out_cap + guard] in the field order of mcs_soa and out_meta of the
 * same length (the packed word: grid | tcut << 16 | downstream << 24 | inj << 25); exp_gidx[exp_cap], exp_f64[8][exp_cap],
 * exp_meta[exp_cap]; scan_total; pd / pd_next: n_use, n_saved, i_mult, n_new as the device holds them after the call, every word
 * -7 before it but pd.n_use = n in form 1; the two counter words and the mismatch word (0 before the call) after it.
 * Refused with a message, the context unchanged: a null argument, a form outside 0..2, cap_n < n, n < 0, i_mult < 1, n_target < 1,
 * n_main_next < 0, match other than 1 or 5, src_fill outside [0, cap_n), a saved state whose grid (0..65535) or tcut (0..255) does not fit the packed word, children that
 * do not fit out_cap, exp_cap < n_saved, form 2 with fp32 state, export_mode outside 0..2 or set in forms 1 and 2.  The population
 * of the context is not touched; the saved arrays of the last mcs_run_pcut are replaced. */
typedef struct mcs_pcut_eval {
  int32_t form, match, export_mode, reserved;
  int64_t n, cap_n, src_fill, i_mult, n_target, n_main_next, guard, out_cap, exp_cap, exp_first, exp_stride;
  uint64_t ctr_work, ctr_saved;
  const uint8_t* l_save; const mcs_soa* saved; const int64_t* exp_gin;
  int64_t* src; double* out_f64; uint32_t* out_meta; int64_t* exp_gidx; double* exp_f64; uint32_t* exp_meta;
  uint64_t scan_total, ctr_work_after, ctr_saved_after, mismatch;
  int64_t pd[4], pd_next[4];
} mcs_pcut_eval;
int mcs_eval_pcut_split(mcs_ctx* ctx, mcs_pcut_eval* io);
/* The step where a particle event becomes numbers in the tally buffer, on the CALLER's records: the transport kernel's own flux_tally,
 * particle_finish, tcut_track, record stack, tally replicas and block flush, in a kernel inside its translation unit
 * (mcs_k_eval_tally in csrc/mcs_transport.hip), between block_prologue and block_flush as transport_body runs them.  Called after
 * mcs_begin_iteration / mcs_begin_species on a context with an empty population; the launch constants are the context's own (those of
 * a transport launch of pcut 1), the replicas are marked as a transport launch marks them, and the results are read with
 * mcs_read_tallies.  n_pass x n_thread records, record (pass, thread) at index pass * n_thread + thread; thread t is lane t % 64 of
 * wave (t % 256) / 64 of block t / 256 (blocks of 256 threads), and a pass is one round in which every thread handles its record.
 *   rec [n][8]  pb_pf, p_perp, ptot_pf, gam_pf, phi, weight, x, x_old   (form 2: in the fp32 kernels' normalised units, every value an
 *               exact float: momenta in m_p c, lengths in rg0 = gam0 beta0 m_p c^2 / (e B[0]); the tally sees (double) f * unit)
 *   word [n]    i_grid | i_grid_old << 8 | ig3 << 16 | inj << 24 | aux << 32 | kind << 40
 *               kind 0 idle (the thread sits the pass out), 1 zone crossing (flux_tally), 2 finished particle (particle_finish; aux =
 *               i_reason 1..4), 3 time cut (tcut_track; aux = the index of the cut, 1..n_tcuts)
 * form 0  direct: every thread calls the tally function on its record (the DIRECT sites of the loop, and a lane's third event);
 *      1  the stack: per pass a wave drains when 64 records are pending, then the threads with a record of kind 1 or 2 push it
 *         (push_record; an idle thread takes no part in the ballot); drain_events(all) after the last pass.  Kind 3 is called directly.
 *      2  the fp32 kernels' stack: the same through push_record_k / drain_events_k (which drains at 32).  The fp32 kernels are part of
 *         every build, so the context need not be an fp32-state one.
 * Refused with a message, nothing queued: a null or negative argument, a form outside 0..2, a kind outside 0..3, a non-finite value, a
 * zone index outside [0, n_grid + 1], a crossing that would tally outside zones 1..n_grid, i_reason outside 1..4, a cut outside
 * [1, n_tcuts], form 2 with a value that is no float, a population, and a layout whose pending records would exceed a wave's stack (with one push per
 * lane and pass between two drain checks none does: the stack's capacity rests on at most two; the check guards the invariant). */
#define MCS_TALLY_REC_F64 8
int mcs_eval_tally(mcs_ctx* ctx, int form, int64_t n_pass, int64_t n_thread, const double* rec, const uint64_t* word);
/* The move of Code Block 2 and the decision what that move triggers, on the CALLER's states: the transport kernel's own
 * load_particle, refresh_move / refresh_time / refresh_dtest, one of the four spellings of the move, then slow_post or plain_crossing,
 * in a kernel inside its translation unit (mcs_k_eval_move in csrc/mcs_transport.hip), between block_prologue and block_flush as
 * transport_body runs them.  The states are the context's population (mcs_pop_upload after mcs_begin_iteration / mcs_begin_species),
 * one state per thread, n = the population's size: weight, ptot_pf, pb_pf, x, xn_per, prp, acctime, phi, grid, tcut, downstream, inj
 * as the move sees them, i.e. AFTER the scatter and the clock of a pass; gam_pf, gyro_denom, gyro_rad_tot, gyro_period (that of the
 * prologue: 2 pi gam m c / (Z e B)), p_perp and the zone's properties and edges are the kernel's own derivation.  The launch constants
 * are those of a transport launch of pcut i_pcut over this population (which fixes pcut_prev, and the RNG key of state k: that of
 * particle k + 1).  Neither the population nor the saved arrays are written; tallies are read with mcs_read_tallies.
 * form 0  move_and_detect: the exact one, as Code Block 1 passes and the rare region use it
 *      1  refresh_thr then move_and_detect_thr: the common pass
 *      2  form 1 with the tail loop's literals (mod2pi_k, whose domain is that of mod2pi: |phi + 2 pi / xn_per| < 1e5)
 *      3  the lossy kernel: refresh_dtest_k, refresh_thr without the fine / coarse switch, move_and_detect_thr(xn_is_threshold = false)
 *      In forms 1-3 the two thresholds are computed with the position set to x_thr[k] (the lane's last visit to the rare region),
 *      the state otherwise its own; then the move is made from the state's own x.  x_thr = x is the ordinary case.  Form 0 ignores
 *      x_thr (may be NULL).
 * post 0  nothing follows the move          1  slow_post, its record pushed and drained          2  slow_post tallying directly
 *      3  plain_crossing, its record pushed and drained                                          4  plain_crossing tallying directly
 *      Posts 1-4 run on the moved state whether or not the move reported an event.
 * out [n][MCS_MOVE_OUT_F64]  x, x_old, phi, pb_pf, p_perp, ptot_pf, gam_pf, prp, acctime, t_hi, t_lo, x_dt, z_lo, z_hi, z_ux, z_gsf,
 *      z_bcos, z_gef   (t_hi, t_lo: 0 in form 0)
 * word [n]  i_grid | i_grid_old << 8 | ig3 << 16 | tcut << 24 | downstream << 32 | inj << 33 | end << 34 (3 bits: slow_post's end code
 *      1..4, 7 = goes on / no slow_post) | F_B1 << 37 | F_CROSSED << 38 | F_ZONE << 39 | the move's returned event bit << 40 |
 *      its ev_cross << 41 | plain_crossing's return value << 42 | records pushed << 43 (2 bits) | min(n_retro, 511) << 45 |
 *      min(draws taken, 1023) << 54
 * Refused with a message, nothing queued: a null or negative argument, form outside 0..3, post outside 0..4, i_pcut outside
 * [1, n_pcuts], n other than the population's size, a non-finite x_thr, a context with fp32 state. */
#define MCS_MOVE_OUT_F64 18
int mcs_eval_move(mcs_ctx* ctx, int form, int post, int i_pcut, int64_t n, const double* x_thr, double* out, uint64_t* word);
/* One pass boundary on the CALLER's states: the move of Code Block 2 with what it triggers (as mcs_eval_move, form 0, post 2), then the
 * head of Code Block 3 -- everything between the end of one move and the next scatter -- through the transport kernel's own slow_pre,
 * in a kernel inside its translation unit (mcs_k_eval_pass in csrc/mcs_transport.hip).  The states are the context's population, one
 * per thread, n = its size, as mcs_eval_move reads them (the row AFTER the scatter and the clock of the pass that moves); helix[k] is
 * the count of that pass (the particle's first: 1), which load_particle's value is overridden with.  Before the move the derived
 * quantities and flags are those the slow_pre of that pass left: cos_max, 1/ptot and the gyro period of the scatter's statements with
 * the state's xn_per, t_step, 2 pi / xn_per, 1/(gam m), x_dt; F_NEARP and F_SAVE by their predicates; no refresh pending.  What the
 * pass head then recomputes is what a flag raised by the move's events or by the head's own branches asks for.
 * form 0  slow_pre (the general kernel), t_clock = the move's t_step
 *      1  the LOSSY kernel's in-line radiative loss (lossy_inline_loss) with the constants as that kernel holds them, on the state as
 *         slow_post left it.  Species with aa < 1 only, do_rad_losses set, no custom eps_B, no dont_scatter: the LOSSY kernel's domain.
 * The head runs if the particle goes on after the move and its next pass is no Code Block 1 pass (no PRP return).
 * out [n][MCS_PASS_OUT_F64]
 *       0 pb_pf   1 p_perp   2 ptot_pf   3 gam_pf   4 phi   5 x   6 x_old   7 prp   8 acctime
 *       9 gyro_denom   10 gyro_rad   11 gyro_rad_tot   12 gyro_period   13 cm_val (cos_max)   14 rp_val (1/ptot_pf)   15 xn_per
 *      16 dphi   17 t_step   18 rg_val (1/(gam_pf m))   19 x_dt   20 t_hi   21 t_lo (form 1 only, else 0)
 *      22 z_lo   23 z_hi   24 z_ux   25 z_gsf   26 z_bcos   27 z_gef
 * word [n]  i_grid | i_grid_old << 8 | ig3 << 16 | tcut << 24 | downstream << 32 | inj << 33 | slow_post's end code << 34 (3 bits: 1..4,
 *      7 = goes on) | (the head's end code + 1) << 37 (3 bits: 0 = goes on to the scatter, 1 = saved for the next pcut, 2..5 = i_reason
 *      1..4, 7 = the head did not run) | F_SAVE << 40 | F_NEARP << 41 | helix after << 42 (14 bits) | min(draws taken, 7) << 56 |
 *      min(n_retro, 7) << 59 | the move's event bit << 62 | its ev_cross << 63
 * Neither the population nor the saved arrays are written; the tallies (the time cuts' sums, MCS_IC_HELIX_CAP, MCS_IC_PSP_CLAMP, the
 * receivers' energy pool) stay in the context for mcs_read_tallies.
 * Refused with a message, nothing queued: a null or negative argument, form outside 0..1, form 1 outside the LOSSY kernel's domain,
 * i_pcut outside [1, n_pcuts], n other than the population's size, helix[k] outside [1, 16000], a context with fp32 state. */
#define MCS_PASS_OUT_F64 28
int mcs_eval_pass(mcs_ctx* ctx, int form, int i_pcut, int64_t n, const int32_t* helix, double* out, uint64_t* word);
/* per-particle end state of the last mcs_run_pcut (bit-parity tests): i_reason
 * (0 = saved), helix_count, retro step count, final ptot_pf and x. Any pointer may be NULL.
 * The kernel records them only after mcs_set_debug_finals(ctx, 1) (24 B of stores per particle
 * and pcut that the product path does not need); otherwise mcs_final_download fails. */
int mcs_set_debug_finals(mcs_ctx* ctx, int on);
/* inner-step cap of one retro_time walk (0 = MCS_RETRO_CAP); tests lower it to reach the cap path */
int mcs_set_retro_cap(mcs_ctx* ctx, int64_t cap);
int mcs_final_download(mcs_ctx* ctx, int64_t n, int32_t* reason, int32_t* helix_count,
                       int32_t* retro_count, double* ptot_pf, double* x_PT_cm);
/* kernel time [ms] of the last mcs_run_pcut, from HIP events on the context stream */
double mcs_last_kernel_ms(mcs_ctx* ctx);
/* launch geometry override: blocks (0 = auto), threads per block (0 = auto) */
int mcs_set_launch(mcs_ctx* ctx, int blocks, int threads);
/* Sliced tail of mcs_run_pcut* (0 = off: one launch per pcut).  A launch cannot end before its longest history does, and
 * a history is up to 10^4 sequential passes (src/particle_loop.jl:162) while the bulk of a 10^6-particle pcut takes the
 * chip a few thousand: with budget_trips > 0 every wave that has found the work queue empty makes budget_trips more
 * trips through its loop (6 passes each), writes the complete lane state of its live particles to a device buffer and
 * ends; the library relaunches them spread over the chip's waves -- a particle that shares its wave with few others
 * advances faster, its neighbours' rare work no longer stalls it -- until none is left.  A history is the same bit for
 * bit however often it is suspended (state and RNG stream position travel with the particle).
 * mcs_last_launches: launches the last mcs_run_pcut* took.
 * mcs_last_kernel: which transport kernel they ran -- 0 the general kernel, 1 its specialisation for the common configuration,
 * 2 the one for electrons with radiative losses, 3 the fp32-state kernel, 4 its plain-loop form, 5 its specialisation for
 * electrons with radiative losses, 6 the common configuration with ion -> electron energy transfer on.  * 7 / 8: the wave-specialised kernel for the common configuration / the same with energy transfer (MCS_OPT_K1_WS), 9: the fp32-state
 * plain loop with the exact primitives (MCS_OPT_F32_EXACT), 10: the general kernel's form for sliced launches, 11 / 12 / 13: the sliced forms
 * of 1 / 2 / 6 (what mcs_run_pcuts_pipelined launches).
 * mcs_set_tail_slicing(ctx, b) is mcs_set_option(ctx, MCS_OPT_TAIL_BUDGET, b) with messages of its own. */
int mcs_set_tail_slicing(mcs_ctx* ctx, int budget_trips);
/* A species' pcuts first .. last queued back to back: transport, pcut_finalize and new_pcut (src/cuts.jl:34-124) of every pcut with
 * nothing read back in between -- n_saved, i_mult = max(n_target / n_saved, 1) (src/cuts.jl:42) and the size of the next population
 * are decided on the device.  What the loop `for i_pcut` of src/main_loops.jl:184-292 + :293-330 does for ONE rank whose shard is
 * the whole population (global indices 0, 1, 2, ...).  n_target[k]: target population after pcut first + k (N_PTS_PCUT or
 * N_PTS_PCUT_HI).  Outputs (host arrays of last - first + 1 entries): population, saved particles and i_mult of every pcut, the
 * kernel time of each transport launch (may be NULL).  Pcuts after one that saved nobody run on an empty population.  Per-particle
 * results are those of the mcs_run_pcut / mcs_new_pcut sequence, bit for bit. */
int mcs_run_pcuts_fused(mcs_ctx* ctx, int i_pcut_first, int i_pcut_last, const int64_t* n_target, int64_t* n_use, int64_t* n_saved,
                        int64_t* i_mult, double* kernel_ms);
int mcs_last_launches(mcs_ctx* ctx);
int mcs_last_kernel(mcs_ctx* ctx);
/* compute units of the context's device (the default grid of mcs_run_pcut* is 2 workgroups per CU; a caller that keeps two
 * contexts busy on one device gives each of them one per CU: mcs_set_launch(ctx, mcs_num_cus(ctx), 256)) */
int mcs_num_cus(mcs_ctx* ctx);
/* workgroups of the current species' transport kernel that one CU holds under an explicit launch geometry (mcs_set_launch):
 * 2 for the fp64 kernels, 3 for the fp32-state ones.  A caller that runs two species side by side splits
 * mcs_num_cus * this between their launches.  0 before mcs_set_cuts. */
int mcs_k1_blocks_per_cu(mcs_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MCS_H */

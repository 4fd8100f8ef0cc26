// mcs_launch.h -- what one translation unit of the library calls in another, each declared ONCE: mcs_api.hip calls them, and the files
// that define them (mcs_transport.hip, mcs_population.hip, mcs_consumers.hip) include this too.  They are extern "C": no mangling tells
// two signatures apart, so a drift shows only where the compiler sees declaration and definition together.
#pragma once
#include "mcs_device.h"

extern "C" {
int mcs_transport_max_entries(void);
hipError_t mcs_launch_transport(const KArgs* a_dev, int kernel, int blocks, int threads, hipStream_t st);
int mcs_transport_ws_threads(void);
hipError_t mcs_launch_finalize_split_dev(const uint8_t* l_save, long long cap_n, unsigned int* block_counts, unsigned long long* block_offsets,
                                         unsigned long long* scan_total, long long* src, PcutDev* pd, PcutDev* pd_next, unsigned long long* counters,
                                         long long n_target, unsigned long long* err, DevPop sv, DevPop out, int split_blocks, hipStream_t st);
hipError_t mcs_launch_compact(const uint8_t* l_save, long long n, unsigned int* block_counts, unsigned long long* block_offsets,
                              unsigned long long* total_dev, long long* src, hipStream_t st);
hipError_t mcs_launch_split(DevPop sv, DevPop out, const long long* src, long long n_new, long long i_mult, hipStream_t st);
hipError_t mcs_launch_compact_match(const uint8_t* l_save, long long n, unsigned int* block_counts, unsigned long long* block_offsets,
                                    unsigned long long* total_dev, long long* src, unsigned int match, hipStream_t st);
hipError_t mcs_launch_late_split(const uint8_t* l_save, long long n, unsigned int* block_counts, unsigned long long* block_offsets,
                                 unsigned long long* total_dev, long long* src, PcutDev* pd, long long i_mult, long long n_main_next, DevPop sv,
                                 DevPop out_at_main_end, int split_blocks, hipStream_t st);
hipError_t mcs_launch_saved_export(DevPop sv, const long long* src, long long n_saved, long long cap, long long first,
                                   long long stride, const long long* gin, long long* gidx, double* f64, uint32_t* meta,
                                   hipStream_t st);
hipError_t mcs_launch_split_import(DevPop out, const double* f64, const uint32_t* meta, long long cap, long long i_mult,
                                   long long first, long long stride, long long n_local, hipStream_t st);
hipError_t mcs_launch_init_pop(DevPop out, const double* ptot_in, const double* weight_in, long long n, long long j_offset,
                               long long j_stride, long long n_total, unsigned long long key, double m, double u, double x_start,
                               int i_grid_start, int relativistic, int fast_push, double xn_per_fine, double x_grid_stop,
                               int n_bins, const double* bin_ptot, const double* bin_weight, const long long* bin_start,
                               hipStream_t st);
hipError_t mcs_launch_fill(double* p, long long n, double v, hipStream_t st);
hipError_t mcs_launch_fold_replicas(double* dst, double* rep, long long n, int n_rep, hipStream_t st);
hipError_t mcs_launch_accumulate_tallies(double* dT, double* sT, unsigned long long* dI, unsigned long long* sI, long long a_lo,
                                         long long a_n, long long b_lo, long long b_n, long long i_lo, long long i_n, hipStream_t st);
hipError_t mcs_launch_copy(double* dst, const double* src, long long n, hipStream_t st);
hipError_t mcs_launch_eval(int fn, long long n, const double* a, const double* b, double* out, hipStream_t st);
hipError_t mcs_launch_eval_hot(int fn, long long n, const double* a, const double* b, double* out, hipStream_t st);
hipError_t mcs_launch_eval_scatter(const KArgs* a_dev, int form, long long n, const double* in, double* out, hipStream_t st);
hipError_t mcs_launch_eval_tally(const KArgs* a_dev, int form, long long n_pass, long long n_thread, const double* rec,
                                 const unsigned long long* word, hipStream_t st);
int mcs_eval_tally_stack(int form, int* cap, int* drain_at);
hipError_t mcs_launch_eval_move(const KArgs* a_dev, int form, int post, long long n, const double* x_thr, double* out,
                                unsigned long long* word, hipStream_t st);
hipError_t mcs_launch_eval_pass(const KArgs* a_dev, int form, long long n, const int* helix, double* out, unsigned long long* word,
                                hipStream_t st);
hipError_t mcs_launch_dndp_cr(const mcs_params* P, const double* psd, const double* gam_sf, const double* ux, const double* tabs,
                              double rest_energy, double n0, double gam0, double* out_dndp, unsigned long long* diag, hipStream_t st);
hipError_t mcs_launch_dndp_esc(const mcs_params* P, const double* esc, const double* tabs, double rest_energy, const double gam_pf[2], double gam0,
                               double* rows, unsigned int* row_diag, double* out, unsigned long long* diag, hipStream_t st);
hipError_t mcs_launch_angle_dist(const mcs_params* P, const double* psd, const double* therm_sf, const unsigned long long* num_crossings,
                                 const double* gam_sf, const double* tabs, double rest_energy, double gam0, int therm_from_hist, int n_win,
                                 const int32_t* l_lo, const int32_t* l_hi, double* out, hipStream_t st);
hipError_t mcs_launch_tcut_spectra(const mcs_params* P, const double* now, const double* base, const double* weight, const double* mom_log,
                                   const double* tcuts, int n_tcuts, double* out, unsigned int* row_neg, unsigned long long* diag, hipStream_t st);
hipError_t mcs_launch_profile_update(const mcs_params* P, const mcs_profile_in* in, const double* pxx_flux, const double* energy_flux,
                                     const double* scalars, const double* ux, const double* gam_sf, const double* x_grid, const double* pres,
                                     const double* tab, double* out, unsigned long long* diag, hipStream_t st);
hipError_t mcs_launch_detector_spectra(const mcs_params* P, const double* now_sf, const double* now_pf, const double* base, const double* mom_log,
                                       const double* mom_edge, const double* x_spec, int n_det, int l_lo, int l_hi, double x_unit, double* out,
                                       unsigned int* row_neg, unsigned long long* diag, hipStream_t st);
hipError_t mcs_launch_dndp_2d(const mcs_params* P, const double* psd, const double* therm_sf, const unsigned long long* num_crossings, const double* tabs,
                              double rest_energy, double n0, int therm_from_hist, double gam_x, double beta_x, double* scratch, double* ef, hipStream_t st);
hipError_t mcs_launch_photon_ic(const double* ef, const double* p_edge, const double* field, int n_grid, int NM, int NT, int j_max, int n_nu, int n_photon,
                                double log_min_rm, double bins_per_dec, double mc_e, double beam_area, double* out, hipStream_t st);
hipError_t mcs_launch_photon_observe(const double* emis, const double* tabs, int process, int n_grid, int n_photon, double area, double dlog,
                                     double last_mid_ratio, int n_shells, double* nb, double* out, hipStream_t st);
hipError_t mcs_launch_photon_pion(const double* dndp_pf, const double* p_edge, const double* target, int n_grid, int NM, int n_photon,
                                  double log_emin_erg, double bins_per_dec, double mc, double aa, double scaling, int i_data, double* out, hipStream_t st);
hipError_t mcs_launch_photon_synch(const double* dndp_pf, const double* p_edge, const double* btot, int n_grid, int NM, int n_photon,
                                   double log_emin_erg, double bins_per_dec, double mc, double* out, hipStream_t st);
hipError_t mcs_launch_thermo(const mcs_params* P, const double* psd, const double* therm_pf, const unsigned long long* num_crossings,
                             const double* gam_sf, const double* ux, const double* tabs, double rest_energy, double mc, double n0,
                             int therm_from_hist, double* scratch, double* out3, hipStream_t st);
}

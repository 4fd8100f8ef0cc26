// mcs_ctx_view.h -- what a translation unit beside mcs_api.hip may see of a context (struct mcs_ctx is private to that file):
// its device, stream, tally buffers, parameters, layout and consumer output buffer.  mcs_ensemble.hip (K8) works through this view.
// Not part of the C ABI of include/mcs.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include "../../include/mcs.h"

struct McsCtxView {
  int device;
  hipStream_t stream;
  double* T;                  // flat fp64 tallies (layout L)
  unsigned long long* I;      // int64 tallies
  mcs_params P;
  mcs_layout L;
  // the consumer output buffer, [3][n_grid][nmom+2] of mcs_dndp_cr then 3 x [n_grid] of mcs_thermo_calcs (null before the first
  // consumer call), and whether each has left a whole result there since the last mcs_begin_species / products sample
  const double* cout;
  bool have_dndp_cr, have_thermo;
  // per photon process (MCS_PHOTON_SYNCH / _IC / _PION): what the last mcs_photon_observe of it left on the device, [shells + 1][n]
  // (pobs_n: that n, 0 = nothing since the last mcs_begin_species, tally write or photons sample)
  const double* pobs[3];
  int pobs_n[3], pobs_shells[3];
  // what the last mcs_dndp_esc left on the device, dNdp [2][3][nmom+2] then number [2][3] (null before the first call), and whether
  // it is a whole result since the last mcs_begin_species / escape sample
  const double* esc_out;
  bool have_esc;
  // what the last mcs_angle_dist left on the device, in the layout of an angles sample (mcs_ens_angles_layout; null before the first
  // call), whether it is a whole result since the last mcs_begin_species / tally write / angles sample, and that call's windows
  const double* ang_out;
  bool have_ang;
  int ang_n_win;
  int32_t ang_lo[MCS_ANGLE_MAX_WINDOWS], ang_hi[MCS_ANGLE_MAX_WINDOWS];
  // what the last mcs_tcut_spectra left on the device, in mcs_tcut_layout (null before the first call), whether it is a whole result
  // since the last mcs_begin_species / tcuts sample, and that call's n_tcuts
  const double* tcut_out;
  bool have_tcut;
  int tcut_n;
  // what the last mcs_profile_update left on the device, in mcs_profile_layout (null before the first call), whether it is a whole result
  // since the last mcs_begin_species / tally write / profile sample, and the settings of that call's mcs_profile_in (F_px_upstream ..
  // i_trans; no history, null tables)
  const double* prof_out;
  bool have_prof;
  mcs_profile_in prof_in;
  // what the last mcs_detector_spectra left on the device, in mcs_detector_layout (null before the first call), whether it is a whole
  // result since the last mcs_begin_species / mcs_set_cuts / detectors sample, and that call's settings: nd, window, x_unit and the
  // host copy of x_spec[0..nd) that the context keeps (valid until its next mcs_set_cuts)
  const double* det_out;
  bool have_det;
  int det_n, det_lo, det_hi;
  double det_x_unit;
  const double* det_x_spec;
};

extern "C" {
// The view of ctx, with its device made current and its tally replicas folded into T (queued on its stream), as every reader of
// the tally buffer does.  Non-zero, with the message set: the fold could not be queued.
int mcs_ctx_view_get(mcs_ctx* ctx, McsCtxView* out);
// The tally buffer of ctx has been rewritten: what was derived from the old contents (the d2N/dp dcos array of the last
// two-dimensional consumer call) is no longer valid.
void mcs_ctx_view_tallies_written(mcs_ctx* ctx);
// A products sample of the ensemble statistics has been queued from ctx's consumer output buffer: both consumers have to run again
// before the next one.
void mcs_ctx_view_products_taken(mcs_ctx* ctx);
// A photons sample has been queued from ctx's observed spectra: the folds and mcs_photon_observe have to run again before the next.
void mcs_ctx_view_photons_taken(mcs_ctx* ctx);
// An escape sample has been queued from ctx's mcs_dndp_esc result: that call has to run again before the next.
void mcs_ctx_view_escape_taken(mcs_ctx* ctx);
// An angles sample has been queued from ctx's mcs_angle_dist result: that call has to run again before the next.
void mcs_ctx_view_angles_taken(mcs_ctx* ctx);
// A tcuts sample has been queued from ctx's mcs_tcut_spectra result: that call has to run again before the next.
void mcs_ctx_view_tcuts_taken(mcs_ctx* ctx);
// A profile sample has been queued from ctx's mcs_profile_update result: that call has to run again before the next.
void mcs_ctx_view_profile_taken(mcs_ctx* ctx);
// A detectors sample has been queued from ctx's mcs_detector_spectra result: that call has to run again before the next.
void mcs_ctx_view_detectors_taken(mcs_ctx* ctx);
// Sets the message of the calling thread's last error (what the ABI's error call returns); returns 1.
int mcs_ctx_view_fail(const char* msg);
}

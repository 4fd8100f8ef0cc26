// mcs_consumers.hip -- K4: the immediate consumers of the PSD tallies, on the device.
//
//   mcs_k_dndp_cr  : get_dNdp_cr (src/particle_counter.jl:29-306) incl. get_transform_dN /
//                    triangular_distribution! / transform_psd_corners (src/transformers.jl:29-312,
//                    634-682) and identify_corners (src/identify_corners.jl), followed by the CR
//                    normalisation of get_normalized_dNdp (src/particle_counter.jl:733-790);
//   mcs_k_thermo   : thermo_calcs (src/thermo_calcs.jl:30-352).
//
// Both read the 22 MB psd where it already is (HBM, written by K1) and hand back O(n_grid x bins)
// numbers, so the 66 MB tally buffer never crosses PCIe for them.  One workgroup owns one grid
// zone: the zone's psd slab (nmom+2)(ntht+2) fp64 is streamed once, momentum-fastest =
// coalesced; the dN(p) histograms of the three frames are accumulated in LDS (ds_add_f64) and
// written once.  HBM-bound: 8 B per PSD cell per kernel (+ 16 B per cell for the thermo scratch).
// The reference's consumer quirks C1-C6 are handled as DESIGN.md section 3b says.
#include "mcs_device.h"
#include "mcs_launch.h"
#include "mcs_slope.h"
#include "../../include/mcs_math.h"
#include "../../include/mcs_synch.h"
#include "../../include/mcs_ic.h"
#include "../../include/mcs_pion.h"

#pragma clang fp contract(off)

namespace {

#define KC_MAXB 208            // >= psd_max + 2 bins per axis

__device__ __forceinline__ int c_bin_mom(const mcs_params& P, double p) {
  int b = p < P.psd_mom_min ? 0 : (int)trunc(mcsm::log10(p / P.psd_mom_min) * P.psd_bins_per_dec_mom) + 1;
  return b > P.num_psd_mom_bins ? P.num_psd_mom_bins : b;
}
__device__ __forceinline__ int c_bin_ang(const mcs_params& P, double px, double pt) {
  if (pt == 0.0) return 0;
  const double c = -px / pt;
  int b;
  if (c < P.psd_cos_fine) b = P.num_psd_tht_bins - (int)trunc((c + 1) / P.psd_dcos);
  else {
    const double th = mcsm::acos(c);
    b = th < P.psd_tht_min ? 0 : (int)trunc(mcsm::log10(th / P.psd_tht_min) * P.psd_bins_per_dec_tht) + 1;
  }
  return b < P.num_psd_tht_bins ? b : P.num_psd_tht_bins;
}

// one transformed corner (src/transformers.jl:662-676): log10 of the momentum and the cosine
__device__ __forceinline__ void c_corner(double gam, double beta, double E0, double p_edge, double cos_edge, double& lpt, double& ct) {
  const double px = p_edge * cos_edge;
  const double pc = p_edge * MCS_C;
  const double etot = __builtin_sqrt(pc * pc + E0 * E0);
  const double pxt = gam * (px - beta * etot / MCS_C);
  const double ptt = __builtin_sqrt(p_edge * p_edge + pxt * pxt - px * px);
  lpt = mcsm::log10(ptt);
  ct = pxt / ptt;
}

// identify_corners (src/identify_corners.jl): lowest / highest momentum corner, then the lower /
// higher cosine of the other two, with the tie rules; false on the reference's error() paths.
__device__ bool c_identify(const double pts[4], const double cts[4], double& lo_pt, double& hi_pt, double& clo_pt, double& chi_pt) {
  int i_lo = 0, i_hi = 0;
  for (int q = 1; q < 4; ++q) { if (pts[q] < pts[i_lo]) i_lo = q; if (pts[q] > pts[i_hi]) i_hi = q; }
  int n_lo = 0, n_hi = 0;
  for (int q = 0; q < 4; ++q) { n_lo += pts[q] == pts[i_lo]; n_hi += pts[q] == pts[i_hi]; }
  unsigned mask = 0xFu & ~(1u << i_lo) & ~(1u << i_hi);
  int j_hi = -1, j_lo = -1;
  for (int q = 0; q < 4; ++q) if (((mask >> q) & 1u) && (j_hi < 0 || cts[q] > cts[j_hi])) j_hi = q;
  if (j_hi < 0) return false;
  mask &= ~(1u << j_hi);
  for (int q = 0; q < 4; ++q) if (((mask >> q) & 1u) && (j_lo < 0 || cts[q] < cts[j_lo])) j_lo = q;
  if (j_lo < 0) return false;
  double a_lo_pt = pts[i_lo], a_lo_ct = cts[i_lo], a_hi_pt = pts[i_hi], a_hi_ct = cts[i_hi];
  double b_hi_pt = pts[j_hi], b_hi_ct = cts[j_hi], b_lo_pt = pts[j_lo], b_lo_ct = cts[j_lo];
  if (b_hi_ct == b_lo_ct) {
    if (b_hi_pt < b_lo_pt) { b_hi_pt = pts[j_lo]; b_hi_ct = cts[j_lo]; b_lo_pt = pts[j_hi]; b_lo_ct = cts[j_hi]; }
    else if (!(b_hi_pt > b_lo_pt)) return false;
  }
  if (n_lo > 1) {
    if (a_lo_pt == b_lo_pt) {
      if (a_lo_ct > b_lo_ct) { a_lo_pt = pts[j_lo]; a_lo_ct = cts[j_lo]; b_lo_pt = pts[i_lo]; b_lo_ct = cts[i_lo]; }
      else if (!(a_lo_ct < b_lo_ct)) return false;
    } else if (a_lo_pt == b_hi_pt) {
      if (a_lo_ct > b_hi_ct) { a_lo_pt = pts[j_hi]; a_lo_ct = cts[j_hi]; b_hi_pt = pts[i_lo]; b_hi_ct = cts[i_lo]; }
      else if (!(a_lo_ct < b_hi_ct)) return false;
    } else return false;
  }
  if (n_hi > 1) {
    if (a_hi_pt == b_lo_pt) {
      if (a_hi_ct > b_lo_ct) { a_hi_pt = pts[j_lo]; a_hi_ct = cts[j_lo]; b_lo_pt = pts[i_hi]; b_lo_ct = cts[i_hi]; }
      else if (!(a_hi_ct < b_lo_ct)) return false;
    } else if (a_hi_pt == b_hi_pt) {
      if (a_hi_ct > b_hi_ct) { a_hi_pt = pts[j_hi]; a_hi_ct = cts[j_hi]; b_hi_pt = pts[i_hi]; b_hi_ct = cts[i_hi]; }
      else if (!(a_hi_ct < b_hi_ct)) return false;
    } else return false;
  }
  lo_pt = a_lo_pt; hi_pt = a_hi_pt; clo_pt = b_lo_pt; chi_pt = b_hi_pt;
  return true;
}

typedef __attribute__((address_space(3))) double ldbl;
typedef __attribute__((address_space(1))) double gdbl;
__device__ __forceinline__ void c_ladd(double* p, double v) { (void)__builtin_amdgcn_ds_atomic_fadd_f64((ldbl*)p, v); }
__device__ __forceinline__ void c_gadd(double* p, double v) { (void)__builtin_amdgcn_global_atomic_fadd_f64((gdbl*)p, v); }

// triangular_distribution! with i_approx = 2 (src/transformers.jl:209-312); add(&dN[l], part) is how a part joins its bin
template <class Add>
__device__ __forceinline__ void c_triangular_to(Add add, double* dN, double p_hi, double p_lo, double clo_pt, double chi_pt, double w, int l_lo,
                                                int l_hi, const double* lb, int nmax1) {
  const double length_tot = 1 / (p_hi - p_lo);
  const double ct_height = 2 * w / length_tot;
  double p_bottom = p_lo;
  const double p_peak = (clo_pt + chi_pt) / 2;
  const double p_denom_lo = 1 / (p_peak - p_lo);
  const double p_denom_hi = 1 / (p_hi - p_peak);
  double fractional_area = 0;
  for (int l = l_lo; l <= l_hi; ++l) {
    if (l + 1 > nmax1) break;
    if (p_hi < lb[l_lo + 1]) { add(&dN[l], w); break; }
    const double top = lb[l + 1];
    if (top <= p_peak) {
      const double p_base = top - p_bottom;
      const double rh = (top - p_lo) * p_denom_lo * ct_height;
      const double lh = p_bottom == p_lo ? 0.0 : (p_bottom - p_lo) * p_denom_lo * ct_height;
      const double part = p_base / 2 * (lh + rh);
      add(&dN[l], part);
      p_bottom = top;
      fractional_area += part;
      continue;
    }
    if (top < p_hi) {
      const double p_base = p_hi - top;
      const double lh = p_base * p_denom_hi * ct_height;
      const double missing = p_base / 2 * lh;
      const double part = (w - fractional_area) - missing;
      add(&dN[l], part);
      p_bottom = top;
      fractional_area += part;
      continue;
    }
    add(&dN[l], w - fractional_area);
    break;
  }
}

// ... into the LDS histogram of a workgroup (ds_add_f64)
__device__ void c_triangular(double* dN, double p_hi, double p_lo, double clo_pt, double chi_pt, double w, int l_lo, int l_hi,
                             const double* lb, int nmax1) {
  c_triangular_to([](double* p, double v) { c_ladd(p, v); }, dN, p_hi, p_lo, clo_pt, chi_pt, w, l_lo, l_hi, lb, nmax1);
}

struct ConsArgs {
  mcs_params P;
  const double* psd;        // tallies + L.psd
  const double* therm_pf;   // tallies + L.therm_pf
  const unsigned long long* num_crossings;
  const double *gam_sf, *ux;            // device grid tables, n_grid+2
  const double *mom_log, *mom_edge, *cos_edge, *cos_center, *pt_center, *zone_pop, *density_loc, *cold_pressure;
  double rest_energy, mc, n0, gam0;
  int therm_from_hist;
  double* out_dndp;         // [3][n_grid][nmom+2]
  unsigned long long* diag; // [2]
  double* scratch;          // [n_grid][ntht+2][nmom+2]
  double *out_par, *out_perp, *out_edens;
};

__global__ void __launch_bounds__(256) mcs_k_dndp_cr(ConsArgs a) {
  __shared__ double s_lb[KC_MAXB], s_pe[KC_MAXB], s_ce[KC_MAXB];
  __shared__ double s_dn[3][KC_MAXB];
  __shared__ double s_norm[3];
  const mcs_params& P = a.P;
  const int nm = P.num_psd_mom_bins, nt = P.num_psd_tht_bins, ng = P.n_grid;
  const int NM = nm + 2, NT = nt + 2;
  const int k = blockIdx.x + 1;                 // zone, 1-based
  const double* psd = a.psd + (long long)NM * NT * (k - 1);
  for (int i = threadIdx.x; i < NM; i += blockDim.x) { s_lb[i] = a.mom_log[i]; s_pe[i] = a.mom_edge[i]; s_dn[1][i] = 0.0; s_dn[2][i] = 0.0; }
  for (int i = threadIdx.x; i < NT; i += blockDim.x) s_ce[i] = a.cos_edge[i];
  // shock frame (particle_counter.jl:81-85): one thread per momentum bin, theta ascending
  for (int i = threadIdx.x; i < NM; i += blockDim.x) {
    double acc = 0.0;
    for (int j = 0; j < NT; ++j) { const double v = psd[i + NM * j]; if (v > 0) acc += v; }
    s_dn[0][i] = acc;
  }
  __syncthreads();
  // plasma and ISM frames
  const double gam2 = a.gam_sf[k], gam3 = a.gam0;
  const int ncell = (nm + 1) * (nt + 1);
  for (int q = threadIdx.x; q < ncell; q += blockDim.x) {
    const int i = q % (nm + 1), j = q / (nm + 1);
    const double v = psd[i + NM * j];
    if (v < 1.0e-66) continue;
    for (int m = 2; m <= 3; ++m) {
      const double gam = m == 2 ? gam2 : gam3;
      const double beta = gam >= 1.000001 ? __builtin_sqrt(1 - 1 / (gam * gam)) : 0.0;
      const double w = v / gam;
      double pts[4], cts[4];
      c_corner(gam, beta, a.rest_energy, s_pe[i], s_ce[j], pts[0], cts[0]);
      c_corner(gam, beta, a.rest_energy, s_pe[i + 1], s_ce[j], pts[1], cts[1]);
      c_corner(gam, beta, a.rest_energy, s_pe[i], s_ce[j + 1], pts[2], cts[2]);
      c_corner(gam, beta, a.rest_energy, s_pe[i + 1], s_ce[j + 1], pts[3], cts[3]);
      double p_lo, p_hi, clo, chi;
      if (!c_identify(pts, cts, p_lo, p_hi, clo, chi)) { atomicAdd(&a.diag[0], 1ull); continue; }
      // first edge above p_lo, minus one (the reference scans; the edges increase, so a bisection finds the same index in 8
      // dependent LDS reads instead of up to 174: the scan was most of this kernel's time)
      int l_lo = -1;
      {
        int lo = 0, hi = NM;                       // smallest l in [0, NM) with s_lb[l] > p_lo, NM if there is none
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_lb[mid] > p_lo) hi = mid; else lo = mid + 1; }
        if (lo < NM) l_lo = lo - 1;
      }
      if (l_lo < 0) { l_lo = nm; atomicAdd(&a.diag[1], 1ull); }
      int l_hi = -1;
      for (int l = l_lo; l < NM; ++l) if (s_lb[l] >= p_hi) { l_hi = l; break; }
      if (l_hi < 0) { l_hi = nm; atomicAdd(&a.diag[1], 1ull); }
      c_triangular(s_dn[m - 1], p_hi, p_lo, clo, chi, w, l_lo, l_hi, s_lb, nm + 1);
    }
  }
  __syncthreads();
  // dN(p) -> dN/dp (particle_counter.jl:295-304)
  for (int l = threadIdx.x; l <= nm; l += blockDim.x)
    for (int m = 0; m < 3; ++m) {
      const double d = s_dn[m][l];
      s_dn[m][l] = d < 1.0e-66 ? 1.0e-99 : d / (s_pe[l + 1] - s_pe[l]);
    }
  __syncthreads();
  // normalisation (particle_counter.jl:733-790, thermal area == 0: quirk C4); serial = reference order
  if (threadIdx.x < 3) {
    const int m = threadIdx.x;
    double area = 0.0;
    for (int j = 0; j <= nm; ++j) if (s_dn[m][j] > 1.0e-99) area += s_dn[m][j] * (s_pe[j + 1] - s_pe[j]);
    double area_tot;
    if (area > 0) {
      const double density_pf = a.n0 * a.gam0 * a.ux[1] / (a.gam_sf[k] * a.ux[k]);
      area_tot = density_pf / a.ux[k] + area;
    } else area_tot = 0.0 + area;
    s_norm[m] = area_tot > 0 ? a.zone_pop[k - 1] / area_tot : 0.0;
  }
  __syncthreads();
  for (int l = threadIdx.x; l < NM; l += blockDim.x)
    for (int m = 0; m < 3; ++m) {
      double d = s_dn[m][l];
      if (l <= nm && d > 1.0e-99) d *= s_norm[m];
      a.out_dndp[((long long)m * ng + (k - 1)) * NM + l] = d;
    }
}

// block-wide sum / max of one double per thread (256 threads)
__device__ double c_block_sum(double v, double* s_red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[w] = v;
  __syncthreads();
  return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}
__device__ double c_block_max(double v, double* s_red) {
  for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(v, off); v = o > v ? o : v; }
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[w] = v;
  __syncthreads();
  double m = s_red[0];
  for (int q = 1; q < 4; ++q) m = s_red[q] > m ? s_red[q] : m;
  return m;
}

__global__ void __launch_bounds__(256) mcs_k_thermo(ConsArgs a) {
  __shared__ double s_red[4];
  const mcs_params& P = a.P;
  const int nm = P.num_psd_mom_bins, nt = P.num_psd_tht_bins;
  const int NM = nm + 2, NT = nt + 2;
  const int i = blockIdx.x + 1;
  const long long slab = (long long)NM * NT;
  const double* psd = a.psd + slab * (i - 1);
  const double* thp = a.therm_pf + slab * (i - 1);
  double* d2 = a.scratch + slab * (i - 1);
  const unsigned long long ncross = a.num_crossings[i - 1];
  const double E0 = a.rest_energy, mc = a.mc;
  // d2N_pf = 1e-99 (+ thermal crossings, already binned in the plasma frame by K1: A9)
  for (long long q = threadIdx.x; q < slab; q += blockDim.x) d2[q] = a.therm_from_hist ? 1.0e-99 + thp[q] : 1.0e-99;
  __threadfence(); __syncthreads();
  // CR cells: centre-point rebinning into the plasma frame (thermo_calcs.jl:179-211)
  const double gam = a.gam_sf[i], beta = a.ux[i] / MCS_C;
  const int ncell = (nm + 1) * (nt + 1);
  for (int q = threadIdx.x; q < ncell; q += blockDim.x) {
    const int k = q % (nm + 1), j = q / (nm + 1);
    const double w = psd[k + NM * j];
    if (w <= 1.0e-66) continue;
    const double cs = a.cos_center[j], pt = a.pt_center[k];
    const double px = pt * cs;
    const double pc = pt * MCS_C;
    const double et = __builtin_sqrt(pc * pc + E0 * E0);
    const double pxX = gam * (px - beta * et / MCS_C);
    const double ptX = __builtin_sqrt(pt * pt - px * px + pxX * pxX);
    c_gadd(&d2[c_bin_mom(P, ptX) + NM * c_bin_ang(P, pxX, ptX)], w);
  }
  __threadfence(); __syncthreads();
  // normalisation to the zone population (thermo_calcs.jl:213-232)
  double part = 0.0;
  for (long long q = threadIdx.x; q < slab; q += blockDim.x) { const double v = d2[q]; if (v > 1.0e-66) part += v; }
  double norm_fac = c_block_sum(part, s_red);
  if (ncross == 0ull && norm_fac > 0) norm_fac += a.n0 / a.ux[i];
  if (norm_fac > 0) norm_fac = a.zone_pop[i - 1] / norm_fac;
  double ppart = 0.0, mpart = 0.0;
  for (long long q = threadIdx.x; q < slab; q += blockDim.x) {
    double v = d2[q];
    if (v > 1.0e-66) { v *= norm_fac; d2[q] = v; }
    if (v > 1.0e-66) ppart += v;
    mpart = v > mpart ? v : mpart;
  }
  const double pop = c_block_sum(ppart, s_red);
  const double dmax = c_block_max(mpart, s_red);
  __threadfence(); __syncthreads();
  // pressure and energy density (thermo_calcs.jl:258-347)
  const double density_loc = a.density_loc[i - 1];
  double pressure_loc = a.cold_pressure[i - 1];
  double pp0 = 0.0, pq0 = 0.0, ed0 = 0.0, nf = 0.0;
  bool cold_only = false;
  if (dmax < 1.0e-66 && ncross == 0ull) {
    pp0 = 1.0 / 3 * pressure_loc; pq0 = 2.0 / 3 * pressure_loc; ed0 = 1.5 * pressure_loc;
    cold_only = true;
  } else if (ncross == 0ull) {
    pressure_loc *= 1 - pop / a.zone_pop[i - 1];
    pp0 = 1.0 / 3 * pressure_loc; pq0 = 2.0 / 3 * pressure_loc; ed0 = 1.5 * pressure_loc;
    nf = density_loc / a.zone_pop[i - 1];
  } else {
    nf = density_loc / a.zone_pop[i - 1];
  }
  double sp = 0.0, sq = 0.0, se = 0.0;
  if (!cold_only) {
    for (int q = threadIdx.x; q < ncell; q += blockDim.x) {
      const int k = q % (nm + 1), j = q / (nm + 1);
      const double c = d2[k + NM * j];
      if (c < 1.0e-66) continue;
      const double pt = a.pt_center[k];
      const double t = pt / mc;
      const double gtmp = __builtin_sqrt(1 + t * t);
      const double vel = pt * MCS_C / (mc * gtmp);
      const double pfac = 1.0 / 3 * pt * vel * nf;
      const double efac = (gtmp - 1) * E0;
      const double cs = a.cos_center[j];
      sp += c * pfac * (cs * cs);
      sq += c * pfac * (1 - cs * cs);
      se += efac * c * nf;
    }
  }
  sp = c_block_sum(sp, s_red); sq = c_block_sum(sq, s_red); se = c_block_sum(se, s_red);
  if (threadIdx.x == 0) { a.out_par[i - 1] = pp0 + sp; a.out_perp[i - 1] = pq0 + sq; a.out_edens[i - 1] = ed0 + se; }
}



// ---- K6: get_dNdp_2D (src/particle_counter.jl:343-627, called at src/ion_finalize.jl:50-59) and the inverse-Compton fold
// (src/inverse_compton.jl:36-311, called at src/photon_calcs.jl:116-138) -- SURVEY.md 8(f-4) --------------------------------------
// mcs_k_dndp_2d: one workgroup per grid zone.  d2N/dp dcos of the zone in the shock frame = the thermal crossings (binned on the
// fly by K1 into therm_sf: A9) + the psd cells above 1e-66, divided by dp, normalised to the zone population (:376-519); then the
// centre-point rebin of every cell into the frame moving with (gam_x, beta_x) against the shock frame -- the ISM frame, m = 2 of
// :531-598 (the plasma-frame array of the same loop is never read and is not built).  `sf`: the zone's slab of a scratch buffer,
// `ef`: of the output; both [ntht+2][nmom+2], momentum fastest (the psd's own layout).
__global__ void __launch_bounds__(256) mcs_k_dndp_2d(ConsArgs a, const double* __restrict__ therm_sf, double gam_x, double beta_x, double* __restrict__ ef_out) {
  __shared__ double s_red[4];
  __shared__ double s_dp[KC_MAXB];
  const mcs_params& P = a.P;
  const int nm = P.num_psd_mom_bins, nt = P.num_psd_tht_bins;
  const int NM = nm + 2, NT = nt + 2;
  const int i = blockIdx.x + 1;
  const long long slab = (long long)NM * NT;
  const double* psd = a.psd + slab * (i - 1);
  const double* ths = therm_sf + slab * (i - 1);
  double* sf = a.scratch + slab * (i - 1);
  double* ef = ef_out + slab * (i - 1);
  const unsigned long long ncross = a.num_crossings[i - 1];
  const double E0 = a.rest_energy;
  for (int k = threadIdx.x; k <= nm; k += blockDim.x) s_dp[k] = a.mom_edge[k + 1] - a.mom_edge[k];      // Delta p (:376-380; C1: cgs edges)
  __syncthreads();
  // thermal crossings (:430-451), CR cells (:466-472), dN -> dN/dp (:475-480)
  double part = 0.0;
  for (long long q = threadIdx.x; q < slab; q += blockDim.x) {
    const int k = (int)(q % NM), j = (int)(q / NM);
    double v = 1.0e-99;
    if (ncross != 0ull && a.therm_from_hist) v += ths[q];
    if (k <= nm && j <= nt) { const double w = psd[q]; if (w > 1.0e-66) v += w; }
    if (k <= nm && v > 1.0e-66) v /= s_dp[k];
    sf[q] = v;
    ef[q] = 1.0e-99;
    if (v > 1.0e-66) part += v;
  }
  // density of the array and the rescaling to the zone population (:487-519)
  double dens = c_block_sum(part, s_red);
  if (ncross == 0ull && dens > 0) dens += a.n0;
  const double norm = dens > 0 ? a.zone_pop[i - 1] / dens : 0.0;
  __threadfence(); __syncthreads();
  // the centre-point rebin (:548-598)
  const int ncell = (nm + 1) * (nt + 1);
  for (int q = threadIdx.x; q < ncell; q += blockDim.x) {
    const int k = q % (nm + 1), j = q / (nm + 1);
    double v = sf[k + NM * j];
    v = (v > 1.0e-99 && norm > 0) ? v * norm : 1.0e-99;
    if (v <= 1.0e-66) continue;
    const double w = v * s_dp[k];
    const double cs = a.cos_center[j], pt = a.pt_center[k];
    const double px = pt * cs;
    const double pc = pt * MCS_C;
    const double et = __builtin_sqrt(pc * pc + E0 * E0);                  // hypot(ptot c, E0)
    const double pxX = gam_x * (px - beta_x * et / MCS_C);
    const double ptX = __builtin_sqrt(pt * pt - px * px + pxX * pxX);
    const int kX = c_bin_mom(P, ptX), jX = c_bin_ang(P, pxX, ptX);
    c_gadd(&ef[kX + NM * jX], w / s_dp[kX]);
  }
}

// mcs_k_photon_ic: one workgroup per grid zone, one thread per outgoing photon energy; every thread walks the electron momentum
// bins and the incoming photon bins in the reference's order (include/mcs_ic.h), so a spectrum is the same sum in the same order
// on the CPU twin.  The electrons of a momentum bin inside the jet cone are counted once per zone (one thread per bin, angle bins in
// order: photon_IC's conversion to particle counts, inverse_compton.jl:54-61, and the sums of :235-238).
__global__ void __launch_bounds__(256) mcs_k_photon_ic(const double* __restrict__ ef /*[n_grid][NT][NM]*/, const double* __restrict__ p_edge /*[NM]*/,
                                                      const double* __restrict__ field /*alpha_in[n_nu] | n_in[n_nu]*/, int NM, int NT, int j_max, int n_nu,
                                                      int n_photon, double log_min_rm, double bins_per_dec, double mc_e, double beam_area,
                                                      double* __restrict__ out /*[n_grid][n_photon]*/) {
  __shared__ double s_x[KC_MAXB], s_g[KC_MAXB], s_a[MCS_IC_NNU], s_n[MCS_IC_NNU];
  const int zone = blockIdx.x + 1, nm = NM - 2;
  const double* d2 = ef + (long long)(zone - 1) * NM * NT;
  for (int i = threadIdx.x; i <= nm; i += blockDim.x) {
    const double dp = p_edge[i + 1] - p_edge[i];
    double mx = 0.0, sum = 0.0;
    for (int j = 0; j <= j_max; ++j) {
      const double v = d2[i + NM * j];
      const double c = v <= 1.0e-99 ? 1.0e-99 : v * dp;
      mx = c > mx ? c : mx;
      sum += c;
    }
    s_x[i] = mx <= 1.0e-99 ? 0.0 : sum;
    s_g[i] = mcs_ic_gamma(p_edge[i], p_edge[i + 1], mc_e);
  }
  for (int j = threadIdx.x; j < n_nu; j += blockDim.x) { s_a[j] = field[j]; s_n[j] = field[n_nu + j]; }
  __syncthreads();
  for (int k = threadIdx.x; k < n_photon; k += blockDim.x) {
    const double ao = mcs_ic_alpha_out(log_min_rm, bins_per_dec, k);
    out[(long long)(zone - 1) * n_photon + k] = mcs_ic_emis(mcs_ic_fold_one(s_x, s_g, nm + 1, s_a, s_n, n_nu, ao), ao, beam_area);
  }
}

// ---- K10: dN/dp of the escaping particles (the reference's print_dNdp_esc call, src/ion_finalize.jl:65-68, has no body; its slabs
// are binned and weighted as psd is, so this is get_dNdp_cr, particle_counter.jl:29-304, of one "zone" whose slab is a door's) -----
// A door's slab is esc[ip + ESC_STRIDE * jtheta]; only ip < nmom+2, jtheta < ntht+2 are ever written.  Door 0: esc_psd_up, door 1:
// esc_psd_down, which follows it in the tally buffer.  Two launches, no floating-point atomics, one fixed order of the adds
// (include/mcs.h): the results are the same bits in every call.
#define ESC_STRIDE (MCS_PSD_MAX + 1)
#define ESC_ROWS_THREADS 64

struct EscArgs {
  const double* esc;        // tallies + L.esc_psd_up: [2][ESC_STRIDE][ESC_STRIDE]
  const double *mom_log, *mom_edge, *cos_edge;
  double rest_energy;
  double gam[2][2];         // [door][frame - 1]: the door's plasma frame, the ISM frame
  int nm, nt;
  double* rows;             // scratch [2 doors][2 frames][nt+2][nm+2]: R_j of the header
  unsigned int* row_diag;   // scratch [2][2][nt+2][2]
  double* out;              // dNdp [2][3][nm+2] | number [2][3]
  unsigned long long* diag; // [2][2]
};

// One lane per (door, frame 1 or 2, angle row j <= nt): it walks the row's cells with i ascending and adds their parts into its own
// row of the scratch, which it zeroes first.  The transformed right corners of cell i are the left corners of cell i + 1 (the same
// operations on the same edges: the same bits), so a lit cell behind a lit cell costs two corners instead of four.
__global__ void __launch_bounds__(ESC_ROWS_THREADS) mcs_k_dndp_esc_rows(EscArgs a) {
  __shared__ double s_lb[KC_MAXB], s_pe[KC_MAXB], s_ce[KC_MAXB];
  const int nm = a.nm, nt = a.nt, NM = nm + 2, NT = nt + 2;
  for (int i = threadIdx.x; i < NM; i += blockDim.x) { s_lb[i] = a.mom_log[i]; s_pe[i] = a.mom_edge[i]; }
  for (int i = threadIdx.x; i < NT; i += blockDim.x) s_ce[i] = a.cos_edge[i];
  __syncthreads();
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 4 * (nt + 1)) return;
  const int j = q % (nt + 1), df = q / (nt + 1), door = df >> 1, f = df & 1;
  const double* slab = a.esc + (long long)door * ESC_STRIDE * ESC_STRIDE + (long long)ESC_STRIDE * j;
  double* R = a.rows + ((long long)df * NT + j) * NM;
  for (int l = 0; l < NM; ++l) R[l] = 0.0;
  const double gam = a.gam[door][f];
  const double beta = gam >= 1.000001 ? __builtin_sqrt(1 - 1 / (gam * gam)) : 0.0;
  unsigned int n_skip = 0, n_clamp = 0;
  double pts[4], cts[4];
  int i_right = -1;                               // pts / cts [1] and [3] hold the corners at momentum edge i_right
  for (int i = 0; i <= nm; ++i) {
    const double v = slab[i];
    if (v < 1.0e-66) continue;
    const double w = v / gam;
    if (i_right == i) { pts[0] = pts[1]; cts[0] = cts[1]; pts[2] = pts[3]; cts[2] = cts[3]; }
    else {
      c_corner(gam, beta, a.rest_energy, s_pe[i], s_ce[j], pts[0], cts[0]);
      c_corner(gam, beta, a.rest_energy, s_pe[i], s_ce[j + 1], pts[2], cts[2]);
    }
    c_corner(gam, beta, a.rest_energy, s_pe[i + 1], s_ce[j], pts[1], cts[1]);
    c_corner(gam, beta, a.rest_energy, s_pe[i + 1], s_ce[j + 1], pts[3], cts[3]);
    i_right = i + 1;
    double p_lo, p_hi, clo, chi;
    if (!c_identify(pts, cts, p_lo, p_hi, clo, chi)) { ++n_skip; continue; }
    int l_lo = -1;
    {
      int lo = 0, hi = NM;                        // smallest l in [0, NM) with s_lb[l] > p_lo, NM if there is none
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_lb[mid] > p_lo) hi = mid; else lo = mid + 1; }
      if (lo < NM) l_lo = lo - 1;
    }
    if (l_lo < 0) { l_lo = nm; ++n_clamp; }
    int l_hi = -1;
    for (int l = l_lo; l < NM; ++l) if (s_lb[l] >= p_hi) { l_hi = l; break; }
    if (l_hi < 0) { l_hi = nm; ++n_clamp; }
    c_triangular_to([](double* p, double x) { *p = *p + x; }, R, p_hi, p_lo, clo, chi, w, l_lo, l_hi, s_lb, nm + 1);
  }
  a.row_diag[((long long)df * NT + j) * 2] = n_skip;
  a.row_diag[((long long)df * NT + j) * 2 + 1] = n_clamp;
}

// One workgroup: per door and frame the rows join per bin with j ascending (frame 0: the theta-ascending column sum of the slab's
// written rows, as mcs_k_dndp_cr has it), the number is the serial sum of the bins, then dN -> dN/dp (particle_counter.jl:295-304).
__global__ void __launch_bounds__(256) mcs_k_dndp_esc_join(EscArgs a) {
  __shared__ double s_dn[6][KC_MAXB];
  const int nm = a.nm, nt = a.nt, NM = nm + 2, NT = nt + 2;
  for (int q = threadIdx.x; q < 6 * NM; q += blockDim.x) {
    const int l = q % NM, dm = q / NM, door = dm / 3, m = dm % 3;
    double acc = 0.0;
    if (m == 0) {
      const double* slab = a.esc + (long long)door * ESC_STRIDE * ESC_STRIDE;
      for (int j = 0; j < NT; ++j) { const double v = slab[l + ESC_STRIDE * j]; if (v > 0) acc += v; }
    } else {
      const double* rows = a.rows + (long long)(door * 2 + (m - 1)) * NT * NM;
      for (int j = 0; j <= nt; ++j) acc = acc + rows[(long long)j * NM + l];
    }
    s_dn[dm][l] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double n = 0.0;
    for (int l = 0; l <= nm; ++l) n = n + s_dn[threadIdx.x][l];
    a.out[6 * NM + threadIdx.x] = n;
  }
  if (threadIdx.x >= 64 && threadIdx.x < 68) {
    const int q = threadIdx.x - 64, door = q >> 1, which = q & 1;
    unsigned long long n = 0ull;
    for (int f = 0; f < 2; ++f)
      for (int j = 0; j <= nt; ++j) n += a.row_diag[((long long)(door * 2 + f) * NT + j) * 2 + which];
    a.diag[q] = n;
  }
  for (int q = threadIdx.x; q < 6 * NM; q += blockDim.x) {
    const int l = q % NM, dm = q / NM;
    const double d = s_dn[dm][l];
    a.out[q] = (l > nm || d < 1.0e-66) ? 1.0e-99 : d / (a.mom_edge[l + 1] - a.mom_edge[l]);
  }
}

// ---- K11: the pitch-angle distribution of every zone over momentum windows, in the shock frame, the zone's plasma frame and the
// ISM frame (include/mcs.h, mcs_angle_dist).  The cells are K6's (thermal crossings + psd above 1e-66) and so is the image of a cell
// in a moving frame, the centre-point rebin; what is kept is the angle, not the momentum.  No floating-point atomics: the header
// fixes the order of every add, so the same tallies give the same bits.
// One workgroup per (zone, frame).  The cells are taken in their order, ANG_CHUNK at a time: first every thread makes the weight
// and the image of its cells of the chunk into LDS, one transform per cell -- the image as jX | mask << 8, bit m of the mask set
// where window m holds kX; ANG_DARK, a row that no thread owns, for a cell that is not lit or lies in no window --; then thread j,
// the owner of target row j, walks the chunk in cell order, ANG_STEP cells per step (their images and weights read from LDS
// together: all lanes read the same words, a broadcast), and adds the weights whose image lies in its row to its accumulators of
// the windows in the mask.  A wave none of whose rows is hit skips the adds.
#define ANG_CHUNK 2048
#define ANG_STEP 8
#define ANG_DARK 0x00FFu

struct AngArgs {
  mcs_params P;
  const double *psd, *therm_sf;                   // tallies + L.psd, + L.therm_sf
  const unsigned long long* num_crossings;
  const double* gam_sf;                           // device grid table, n_grid+2
  const double *pt_center, *cos_center, *cos_edge;
  double rest_energy, gam0;
  int therm_from_hist, n_win;
  int l_lo[MCS_ANGLE_MAX_WINDOWS], l_hi[MCS_ANGLE_MAX_WINDOWS];      // (unused windows: 0, 0 -- they hold no bin)
  double* out;                                    // dist [rows][NT] | number [rows] | mean_mu [rows] | mean_mu2 [rows]
};

__global__ void __launch_bounds__(256) mcs_k_angle_dist(AngArgs a) {
  __shared__ __attribute__((aligned(16))) double s_v[ANG_CHUNK];
  __shared__ __attribute__((aligned(16))) unsigned short s_im[ANG_CHUNK];
  __shared__ double s_A[MCS_ANGLE_MAX_WINDOWS][KC_MAXB];
  __shared__ double s_num[MCS_ANGLE_MAX_WINDOWS];
  __shared__ double s_pt[KC_MAXB], s_cc[KC_MAXB];
  const mcs_params& P = a.P;
  const int nm = P.num_psd_mom_bins, nt = P.num_psd_tht_bins, ng = P.n_grid;
  const int NM = nm + 2, NT = nt + 2;
  const int z = blockIdx.x, f = blockIdx.y;       // zone (0-based), frame
  const long long slab = (long long)NM * NT;
  const double* psd = a.psd + slab * z;
  const double* ths = a.therm_sf + slab * z;
  const bool with_therm = a.therm_from_hist && a.num_crossings[z] != 0ull;
  const double E0 = a.rest_energy;
  const double gam = f == 1 ? a.gam_sf[z + 1] : a.gam0;
  const double beta = gam >= 1.000001 ? __builtin_sqrt(1 - 1 / (gam * gam)) : 0.0;      // transformers.jl:639
  for (int i = threadIdx.x; i <= nm; i += blockDim.x) s_pt[i] = a.pt_center[i];
  for (int i = threadIdx.x; i <= nt; i += blockDim.x) s_cc[i] = a.cos_center[i];
  const int row = threadIdx.x;                    // the target row this thread owns, if row <= nt
  double acc[MCS_ANGLE_MAX_WINDOWS];
#pragma unroll
  for (int m = 0; m < MCS_ANGLE_MAX_WINDOWS; ++m) acc[m] = 0.0;
  const int ncell = (nm + 1) * (nt + 1);
  for (int c0 = 0; c0 < ncell; c0 += ANG_CHUNK) {
    const int n = ncell - c0 < ANG_CHUNK ? ncell - c0 : ANG_CHUNK;
    __syncthreads();                              // (the tables are there; the last chunk has been walked)
    const int n_pad = (n + ANG_STEP - 1) / ANG_STEP * ANG_STEP;      // (<= ANG_CHUNK, a multiple of ANG_STEP)
    for (int i = threadIdx.x; i < n_pad; i += blockDim.x) {
      if (i >= n) { s_v[i] = 0.0; s_im[i] = (unsigned short)ANG_DARK; continue; }
      const int q = c0 + i, k = q % (nm + 1), j = q / (nm + 1);
      const int at = k + NM * j;
      double v = 0.0;
      if (with_therm) v = v + ths[at];
      const double w = psd[at];
      if (w > 1.0e-66) v = v + w;
      unsigned int im = ANG_DARK;
      if (v > 1.0e-66) {
        int kX = k, jX = j;
        if (f != 0) {
          const double pt = s_pt[k], cs = s_cc[j];
          const double px = pt * cs;
          const double pc = pt * MCS_C;
          const double et = __builtin_sqrt(pc * pc + E0 * E0);
          const double pxX = gam * (px - beta * et / MCS_C);
          const double ptX = __builtin_sqrt(pt * pt - px * px + pxX * pxX);
          kX = c_bin_mom(P, ptX); jX = c_bin_ang(P, pxX, ptX);
          kX = kX < 0 ? 0 : (kX > nm ? nm : kX);
          jX = jX < 0 ? 0 : (jX > nt ? nt : jX);
        }
        unsigned int mask = 0u;
#pragma unroll
        for (int m = 0; m < MCS_ANGLE_MAX_WINDOWS; ++m) mask |= (kX >= a.l_lo[m] && kX < a.l_hi[m]) ? (1u << m) : 0u;
        if (mask != 0u) im = (unsigned int)jX | (mask << 8);
      }
      s_v[i] = v;
      s_im[i] = (unsigned short)im;
    }
    __syncthreads();
    if (row <= nt) {
      for (int i0 = 0; i0 < n_pad; i0 += ANG_STEP) {
        const uint4 w = *reinterpret_cast<const uint4*>(&s_im[i0]);
        const unsigned int ws[4] = {w.x, w.y, w.z, w.w};
        double v[ANG_STEP];
#pragma unroll
        for (int u = 0; u < ANG_STEP; ++u) v[u] = s_v[i0 + u];
#pragma unroll
        for (int u = 0; u < ANG_STEP; ++u) {
          const unsigned int im = (ws[u >> 1] >> (16 * (u & 1))) & 0xFFFFu;
          if ((int)(im & 255u) != row) continue;
#pragma unroll
          for (int m = 0; m < MCS_ANGLE_MAX_WINDOWS; ++m) acc[m] = ((im >> (8 + m)) & 1u) ? acc[m] + v[u] : acc[m];
        }
      }
    }
  }
  if (row <= nt) {
#pragma unroll
    for (int m = 0; m < MCS_ANGLE_MAX_WINDOWS; ++m) s_A[m][row] = acc[m];
  }
  __syncthreads();
  const long long rows = 3LL * ng * a.n_win, row0 = ((long long)f * ng + z) * a.n_win;
  double* o_dist = a.out;
  double* o_num = a.out + rows * NT;
  if ((int)threadIdx.x < a.n_win) {
    const int m = threadIdx.x;
    double num = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = 0; j <= nt; ++j) {
      const double A = s_A[m][j];
      const double t = A * s_cc[j];
      num = num + A;
      s1 = s1 + t;
      s2 = s2 + t * s_cc[j];
    }
    s_num[m] = num;
    o_num[row0 + m] = num;
    o_num[rows + row0 + m] = num == 0.0 ? __builtin_nan("") : s1 / num;
    o_num[2 * rows + row0 + m] = num == 0.0 ? __builtin_nan("") : s2 / num;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < a.n_win * NT; q += blockDim.x) {
    const int m = q / NT, j = q % NT;
    double d = 1.0e-99;
    if (j <= nt) {
      const double A = s_A[m][j];
      if (A > 0) d = (A / s_num[m]) / (a.cos_edge[j + 1] - a.cos_edge[j]);
    }
    o_dist[(row0 + m) * NT + j] = d;
  }
}

// ---- K12: the spectra of the time cuts (include/mcs.h, mcs_tcut_spectra; the reference's tcut_print, src/io.jl:21-76) --------------
// now: the current species' block of spectra_coupled, [MCS_NA_C][TCUT_STRIDE] with the momentum index fastest; base: what
// mcs_begin_species copied of it; only rows k < nt and words l <= nm are read.  Two launches, no floating-point atomics, one
// fixed order of the adds (include/mcs.h): the same bits in every call.
#define TCUT_STRIDE (MCS_PSD_MAX + 1)

struct TcutArgs {
  const double *now, *base;
  const double* weight;     // weight_coupled of the species: [MCS_NA_C]
  const double* mom_log;    // e[l], [nm+2]
  const double* tcuts;      // [nt]
  int nm, nt;
  double* out;              // mcs_tcut_layout: spectrum [nt][nm+2] | weight | number | mean_log_p [nt] | quantile [3][nt] | index [3]
  unsigned int* row_neg;    // scratch [nt]: the words of a row with now < base
  unsigned long long* diag; // [2]
};

// log10 of the momentum below which the share T / number of a live row's growth lies (include/mcs.h, QUANTILES)
__device__ double tcut_quantile(const double* g, const double* e, int nm, double T) {
  double C = 0.0;
  int last = -1;
  for (int l = 0; l <= nm; ++l) {
    const double gl = g[l];
    const double Cn = C + gl;
    if (gl > 0) {
      if (Cn >= T) {
        const double f = (T - C) / gl;
        return e[l] + f * (e[l + 1] - e[l]);
      }
      last = l;
    }
    C = Cn;
  }
  if (last < 0) return __builtin_nan("");
  return e[last] + 1.0 * (e[last + 1] - e[last]);      // (the last lit bin's C fell short of T through rounding: f = 1)
}

// The ordered part of a row, one lane's work out of LDS (include/mcs.h, GROWTH AND NUMBER, LIVE AND DEAD ROWS, MEAN, QUANTILES): shared by
// K12 and K14.  number is 0.0, mean and the quantiles a quiet NaN in a dead row.
struct TcutRowStats { double number, mean, quant[MCS_TCUT_NQ]; };
__device__ TcutRowStats tcut_row_stats(const double* s_g, const double* s_e, int nm) {
  TcutRowStats r;
  double num = 0.0;
  for (int l = 0; l <= nm; ++l) num = num + s_g[l];
  const bool live = num > 1.0e-99;
  const double nan = __builtin_nan("");
  r.number = live ? num : 0.0;
  double mean = nan;
  if (live) {
    double s = 0.0;
    for (int l = 0; l <= nm; ++l) {
      const double c = 0.5 * (s_e[l] + s_e[l + 1]);
      s = s + s_g[l] * c;
    }
    mean = s / num;
  }
  r.mean = mean;
  const double q[MCS_TCUT_NQ] = MCS_TCUT_Q;
  for (int j = 0; j < MCS_TCUT_NQ; ++j) r.quant[j] = live ? tcut_quantile(s_g, s_e, nm, q[j] * num) : nan;
  return r;
}
// word l of a row's spectrum (num: the row's number, 0.0 in a dead row): the normalisation and floor of tcut_print
__device__ double tcut_spectrum_word(const double* s_g, int l, int nm, double num) {
  double d = 1.0e-99;
  if (num > 0 && l <= nm) {
    const double s = s_g[l] / num;
    d = s < 1.0e-60 ? 1.0e-99 : s;
  }
  return d;
}

// One wave per cut: the lanes stride the row for the loads, the subtraction and the stores; the ordered sums are lane 0's, out of LDS.
__global__ void __launch_bounds__(64) mcs_k_tcut_rows(TcutArgs a) {
  __shared__ double s_g[KC_MAXB], s_e[KC_MAXB];
  __shared__ unsigned int s_neg[64];
  __shared__ double s_num;
  const int nm = a.nm, NM = nm + 2, nt = a.nt, k = blockIdx.x;
  const double* now = a.now + (long long)TCUT_STRIDE * k;
  const double* base = a.base + (long long)TCUT_STRIDE * k;
  unsigned int neg = 0;
  for (int l = threadIdx.x; l < NM; l += 64) s_e[l] = a.mom_log[l];
  for (int l = threadIdx.x; l <= nm; l += 64) {
    const double n = now[l], b = base[l];
    if (n < b) ++neg;
    s_g[l] = n - b;
  }
  s_neg[threadIdx.x] = neg;
  __syncthreads();
  if (threadIdx.x == 0) {
    const TcutRowStats r = tcut_row_stats(s_g, s_e, nm);
    double* o = a.out + (long long)nt * NM;      // weight | number | mean_log_p | quantile [3]
    const double w = a.weight[k];
    o[k] = w < 1.0e-60 ? 1.0e-99 : w;
    o[nt + k] = r.number;
    o[2 * nt + k] = r.mean;
    for (int j = 0; j < MCS_TCUT_NQ; ++j) o[(3 + j) * nt + k] = r.quant[j];
    unsigned int t = 0;
    for (int i = 0; i < 64; ++i) t += s_neg[i];
    a.row_neg[k] = t;
    s_num = r.number;
  }
  __syncthreads();
  const double num = s_num;
  for (int l = threadIdx.x; l < NM; l += 64) a.out[(long long)k * NM + l] = tcut_spectrum_word(s_g, l, nm, num);
}

// One wave: lanes 0..2 the index of a quantile each (the slope rule of the products sample over the live rows), lane 3 the counts.
__global__ void __launch_bounds__(64) mcs_k_tcut_index(TcutArgs a) {
  const int nt = a.nt, NM = a.nm + 2;
  const double* number = a.out + (long long)nt * NM + nt;
  const double* quant = a.out + (long long)nt * NM + 3 * nt;
  if (threadIdx.x < MCS_TCUT_NQ) {
    const double* y = quant + (long long)threadIdx.x * nt;
    a.out[(long long)nt * (NM + 6) + threadIdx.x] =
        mcs_slope_rule(0, nt, [&](int k) { return number[k] > 1.0e-99; }, [&](int k) { return mcsm::log10(a.tcuts[k]); }, [&](int k) { return y[k]; });
  }
  if (threadIdx.x == MCS_TCUT_NQ) {
    unsigned long long live = 0ull, neg = 0ull;
    for (int k = 0; k < nt; ++k) { if (number[k] > 1.0e-99) ++live; neg += a.row_neg[k]; }
    a.diag[0] = live; a.diag[1] = neg;
  }
}

// ---- K14: the spectra at the detectors (include/mcs.h, mcs_detector_spectra; the tallies of src/all_flux.jl:164-190) ---------------
// now_sf / now_pf: the sections spectra_sf and spectra_pf, [n_grid][TCUT_STRIDE] with the momentum index fastest; base: what
// mcs_begin_species copied of their rows 0..nd-1, [2][nd][TCUT_STRIDE]; only rows d < nd and words l <= nm are read.  Two launches, no
// floating-point atomics, one fixed order of the adds: the same bits in every call.
#define DET_JOIN_THREADS 256

struct DetArgs {
  const double *now_sf, *now_pf, *base;
  const double *mom_log, *mom_edge;   // e[l], E[l]: [nm+2] each
  const double* x_spec;               // [nd]
  double x_unit;
  int nm, nd, l_lo, l_hi;
  double* out;              // mcs_detector_layout
  unsigned int* row_neg;    // scratch [2 nd]: the words of a row with now < base
  unsigned long long* diag; // [3]
};

// One wave per (frame, detector), shaped like mcs_k_tcut_rows: the lanes stride the loads, the subtraction and the stores; lane 0
// does the ordered sums and the slope out of LDS.
__global__ void __launch_bounds__(64) mcs_k_detector_rows(DetArgs a) {
  __shared__ double s_g[KC_MAXB], s_e[KC_MAXB], s_w[KC_MAXB];      // growth, log10 edges, bin widths
  __shared__ unsigned int s_neg[64];
  __shared__ double s_num;
  const int nm = a.nm, NM = nm + 2, nd = a.nd, r = blockIdx.x, f = r / nd, d = r - f * nd;
  const double* now = (f == 0 ? a.now_sf : a.now_pf) + (long long)TCUT_STRIDE * d;
  const double* base = a.base + (long long)TCUT_STRIDE * r;
  unsigned int neg = 0;
  for (int l = threadIdx.x; l < NM; l += 64) s_e[l] = a.mom_log[l];
  for (int l = threadIdx.x; l <= nm; l += 64) {
    const double n = now[l], b = base[l];
    if (n < b) ++neg;
    s_g[l] = n - b;
    s_w[l] = a.mom_edge[l + 1] - a.mom_edge[l];
  }
  s_neg[threadIdx.x] = neg;
  __syncthreads();
  const long long rows = 2LL * nd;
  double* o = a.out + 2 * rows * NM;      // number | mean_log_p | quantile [3] | slope, [2][nd] each
  if (threadIdx.x == 0) {
    const TcutRowStats st = tcut_row_stats(s_g, s_e, nm);
    o[r] = st.number;
    o[rows + r] = st.mean;
    for (int j = 0; j < MCS_TCUT_NQ; ++j) o[(2 + j) * rows + r] = st.quant[j];
    double slope = __builtin_nan("");
    if (st.number > 0)
      slope = mcs_slope_rule(a.l_lo, a.l_hi, [&](int l) { return s_g[l] > 0; }, [&](int l) { return 0.5 * (s_e[l] + s_e[l + 1]); },
                             [&](int l) { return mcsm::log10(s_g[l] / s_w[l]); });
    o[(2 + MCS_TCUT_NQ) * rows + r] = slope;
    unsigned int t = 0;
    for (int i = 0; i < 64; ++i) t += s_neg[i];
    a.row_neg[r] = t;
    s_num = st.number;
  }
  __syncthreads();
  const double num = s_num;
  for (int l = threadIdx.x; l < NM; l += 64) {
    a.out[(long long)r * NM + l] = tcut_spectrum_word(s_g, l, nm, num);
    double dn = 1.0e-99;
    if (num > 0 && l <= nm && s_g[l] != 0.0) dn = s_g[l] / s_w[l];
    a.out[(rows + r) * NM + l] = dn;
  }
}

// The join, one block: a lane per momentum bin the gradient over the detectors (frame 0; now - base recomputed, the same bits), then
// lane 0 the counts.
__global__ void __launch_bounds__(DET_JOIN_THREADS) mcs_k_detector_join(DetArgs a) {
  __shared__ unsigned int s_fin[DET_JOIN_THREADS];
  const int nm = a.nm, NM = nm + 2, nd = a.nd;
  const long long rows = 2LL * nd;
  double* grad = a.out + rows * (2 * NM + 3 + MCS_TCUT_NQ);
  unsigned int fin = 0;
  for (int l = threadIdx.x; l < NM; l += DET_JOIN_THREADS) {
    double gr = __builtin_nan("");
    if (l <= nm) {
      auto g = [&](int d) { return a.now_sf[(long long)TCUT_STRIDE * d + l] - a.base[(long long)TCUT_STRIDE * d + l]; };
      gr = mcs_slope_rule(0, nd, [&](int d) { return a.x_spec[d] < 0.0 && g(d) > 0; }, [&](int d) { return a.x_spec[d] / a.x_unit; },
                          [&](int d) { return mcsm::log10(g(d)); });
    }
    grad[l] = gr;
    if (gr - gr == 0.0) ++fin;      // (finite)
  }
  s_fin[threadIdx.x] = fin;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double* number = a.out + 2 * rows * NM;
    unsigned long long live = 0ull, neg = 0ull, nf = 0ull;
    for (int r = 0; r < rows; ++r) { if (number[r] > 1.0e-99) ++live; neg += a.row_neg[r]; }
    for (int i = 0; i < DET_JOIN_THREADS; ++i) nf += s_fin[i];
    a.diag[0] = live; a.diag[1] = neg; a.diag[2] = nf;
  }
}

// ---- K13: the shock-profile update (include/mcs.h, mcs_profile_update; iter_finalize / smooth_grid_par / new_velocity_profile) -------
// One workgroup, no atomics.  Phase A: thread 0 the scalars and the q; then a lane per zone (striding) the rounding, Gamma, the two
// pressures and the two roots into LDS rows.  Phase B, the order-dependent parts out of LDS: thread 0 the momentum row, the first lane of
// the second wave the energy row (last-ten sum, monotone pass, filter, rescale).  Phase C: a lane per zone the blend, the artificial section,
// the weighting and the shift; thread 0 the serial rms and the counts.  Every expression is the header's, operation by operation.
#define PROF_THREADS 256

struct ProfArgs {
  mcs_profile_in in;                          // (its three table pointers are not read: tab below)
  const double *pxx_flux, *energy_flux, *scalars;
  const double *ux, *gsf, *xg;                // grid tables, entry 0 first
  const double* pres;                         // P_par | P_perp | e_dens, [n] each
  const double* tab;                          // pxx_EM | en_EM | atan_x, [n] each
  double u0, beta0, gam0;
  int n, i_shock;
  double* out;                                // mcs_profile_layout
  unsigned long long* diag;                   // [3]
};

__device__ double prof_newton_px(double A, double rmu0, double Xi, double pl, double x, int* steps, int* ran_out) {
  const double c = MCS_C;
  int k = 0;
  bool done = false;
  while (k < MCS_PROFILE_NEWTON_MAX && !done) {
    const double xx = x * x;
    const double f = (A - (rmu0 * (x * c)) * (1.0 + xx)) - (1.0 + xx * Xi) * pl;
    const double df = -((rmu0 * c) * (1.0 + (3.0 * x) * x) + ((2.0 * x) * Xi) * pl);
    const double dx = f / df;
    x = x - dx;
    ++k;
    done = __builtin_fabs(dx) <= 1.0e-14 * __builtin_fabs(x);
  }
  if (k > *steps) *steps = k;
  if (!done) *ran_out = 1;
  return x;
}

__device__ double prof_newton_en(double B, double rm, double u0, double Xi, double pl, double x, int* steps, int* ran_out) {
  const double c = MCS_C;
  int k = 0;
  bool done = false;
  while (k < MCS_PROFILE_NEWTON_MAX && !done) {
    const double t = x / c;
    const double t2 = t * t;
    const double f = (B - ((((0.5 * rm) * u0) * x) * x) * (1.0 + 1.25 * t2)) - ((Xi * pl) * x) * (1.0 + t2);
    const double df = -(((rm * u0) * x) * (1.0 + 2.5 * t2) + (Xi * pl) * (1.0 + 3.0 * t2));
    const double dx = f / df;
    x = x - dx;
    ++k;
    done = __builtin_fabs(dx) <= 1.0e-14 * __builtin_fabs(x);
  }
  if (k > *steps) *steps = k;
  if (!done) *ran_out = 1;
  return x;
}

// smooth_profile! on an LDS row a[n] with scratch d[n]
__device__ void prof_smooth(double* a, double* d, int n) {
  for (int i = n - 1; i >= 1; --i)
    if (a[i - 1] < a[i]) a[i - 1] = a[i];
  for (int i = 0; i < n; ++i) d[i] = a[i];
  d[1] = ((2.0 * a[0] + a[1]) + a[2]) / 4.0;
  for (int i = 2; i <= n - 3; ++i) d[i] = ((a[i - 1] + a[i]) + a[i + 1]) / 3.0;
  d[n - 2] = ((a[n - 3] + a[n - 2]) + 2.0 * a[n - 1]) / 4.0;
  for (int i = 1; i <= n - 2; ++i) a[i] = d[i];
}

__device__ void prof_rescale(double* a, int n, double avg, double u0, double u2, const double* xg) {
  const double s = (u0 - u2) / (a[0] - avg);
  for (int j = 0; j < n; ++j) {
    const double v = s * (a[j] - avg) + u2;
    a[j] = xg[j + 1] >= 0.0 ? u2 : v;
  }
}

__global__ void __launch_bounds__(PROF_THREADS) mcs_k_profile_update(ProfArgs a) {
  extern __shared__ double s_prof[];          // row_px [n] | row_en [n] | d_px [n] | d_en [n]
  __shared__ double s_sc[8];                  // the eight output scalars (shift_rms last)
  __shared__ int s_steps[PROF_THREADS], s_out[PROF_THREADS];
  const int n = a.n, tid = threadIdx.x;
  const mcs_profile_in& I = a.in;
  const double c = MCS_C, mp = MCS_MP;
  const double u0 = a.u0, b0 = a.beta0, g0 = a.gam0, u2 = I.u2;
  const bool rel = b0 >= 0.02;
  double* row_px = s_prof;
  double* row_en = s_prof + n;
  double* o = a.out;
  if (tid == 0) {
    const double* sc = a.scalars;
    const double px_esc = sc[2] / I.F_px_upstream, en_esc = sc[3] / I.F_energy_upstream;
    const double G = 1.0 + sc[0] / sc[1];
    double q_px = 0.0, q_en = 0.0;
    if (!(I.r_comp == I.r_RH)) {
      const double Gf = G / (G - 1.0);
      const double rho0 = I.rho0, P0 = I.P0, g2 = I.gam2, b2 = I.beta2;
      const double rho2 = ((rho0 * g0) * b0) / (g2 * b2);
      if (rel) {
        const double q_fac = c * mcsm::sqrt_((1.0 + b0) / 2.0);
        const double e = rho0 * (c * c) + 2.5 * P0;
        const double Fp = ((g0 * g0) * (b0 * b0)) * e + P0;
        const double Fe = ((g0 * g0) * u0) * e;
        const double aux = (g2 * g2) * (q_fac * (b2 * b2) - u2);
        const double P2 = ((q_fac * Fp - Fe) - (aux * rho2) * (c * c)) / (q_fac + Gf * aux);
        const double t = g2 * b2;
        const double Qp = (Fp - (t * t) * (rho2 * (c * c) + Gf * P2)) - P2;
        const double Qe = Qp * q_fac;
        q_px = Qe / (Fe - ((g0 * u0) * rho0) * (c * c));
        q_en = Qp / Fp;
      } else {
        const double Fp = rho0 * (u0 * u0) + P0;
        const double Fe = (rho0 * ((u0 * u0) * u0)) / 2.0 + (2.5 * P0) * u0;
        const double P2 = Fp - rho2 * (u2 * u2);
        const double Qe = (Fe - ((rho0 * u0) * (u2 * u2)) / 2.0) - (P2 * u2) * Gf;
        q_px = Qe / Fe;
        q_en = 0.0;
      }
    }
    double s_px = q_px, s_en = q_en;
    if (I.n_hist > 0) {
      s_px = I.hist_q_px[0]; s_en = I.hist_q_en[0];
      for (int k = 1; k < I.n_hist; ++k) { s_px = s_px + I.hist_q_px[k]; s_en = s_en + I.hist_q_en[k]; }
      s_px = s_px + q_px; s_en = s_en + q_en;
    }
    const double kk = (double)(I.n_hist + 1);
    s_sc[0] = G;
    s_sc[1] = 1.0e-99 > px_esc ? 1.0e-99 : px_esc;
    s_sc[2] = 1.0e-99 > en_esc ? 1.0e-99 : en_esc;
    s_sc[3] = q_px; s_sc[4] = q_en;
    s_sc[5] = s_px / kk; s_sc[6] = s_en / kk;
  }
  __syncthreads();
  // ---- phase A
  const double pxx0 = __builtin_rint(a.pxx_flux[0] * 1.0e13) / 1.0e13, en0 = __builtin_rint(a.energy_flux[0] * 1.0e13) / 1.0e13;
  const double Qpx = rel ? s_sc[5] * pxx0 : 0.0;
  const double Qen = s_sc[6] * en0;
  int steps = 0, ran_out = 0;
  for (int j = tid; j < n; j += PROF_THREADS) {
    const double pxx = __builtin_rint(a.pxx_flux[j] * 1.0e13) / 1.0e13, en = __builtin_rint(a.energy_flux[j] * 1.0e13) / 1.0e13;
    const double Ptot = a.pres[j] + a.pres[n + j], ed = a.pres[2 * n + j];
    double G = 1.0 + Ptot / ed;
    if (ed == 1.0e-99) G = 1.0e-99;
    const double Xi = G / (G - 1.0);
    const double u = a.ux[j + 1], g = a.gsf[j + 1];
    const double b = u / c;
    const double pxx_EM = a.tab[j], en_EM = a.tab[n + j];
    double p_px, p_loc, v_px, v_en;
    if (rel) {
      const double gb = g * b;
      const double gb2 = gb * gb;
      const double dens = ((g0 * b0) / (g * b)) * I.n0_aa;
      p_px = (pxx - ((gb2 * dens) * mp) * (c * c)) / (1.0 + gb2 * Xi);
      p_loc = (1.0 - I.SMPFP) * p_px + I.SMPFP * Ptot;
      double y = (((I.F_px_upstream - Qpx) - pxx_EM) - p_loc) / (((g0 * b0) * I.n0_aa) * (mp * (c * c) + (p_loc * Xi) / dens));
      v_px = (y / mcsm::sqrt_(1.0 + y * y)) * c;
      const double K = ((I.F_energy_upstream - Qen) - en_EM) / (c * ((dens * mp) * (c * c) + Xi * p_loc));
      const double z = (-1.0 + mcsm::sqrt_(1.0 + (4.0 * K) * K)) / 2.0;
      y = __builtin_copysign(mcsm::sqrt_(z), K);
      v_en = (y / mcsm::sqrt_(1.0 + y * y)) * c;
    } else {
      const double rm = I.n0_aa * mp;
      const double bb = b * b;
      p_px = (pxx - ((rm * u0) * u) * (1.0 + bb)) / (1.0 + bb * Xi);
      p_loc = (1.0 - I.SMPFP) * p_px + I.SMPFP * Ptot;
      const double A = (I.F_px_upstream - Qpx) - pxx_EM;
      const double B = (I.F_energy_upstream - Qen) - en_EM;
      int zone_out = 0;
      v_px = prof_newton_px(A, rm * u0, Xi, p_loc, (u0 / c) * 1.0e-4, &steps, &zone_out) * c;
      v_en = prof_newton_en(B, rm, u0, Xi, p_loc, u0 * 1.0e-4, &steps, &zone_out);
      ran_out += zone_out;
    }
    o[j] = pxx / I.F_px_upstream;
    o[n + j] = en / I.F_energy_upstream;
    o[2 * n + j] = G;
    o[3 * n + j] = p_px;
    o[4 * n + j] = p_loc;
    row_px[j] = v_px;
    row_en[j] = v_en;
  }
  s_steps[tid] = steps; s_out[tid] = ran_out;      // (ran_out: the lane's zones in which either iteration ran out of steps)
  __syncthreads();
  // ---- phase B: thread 0 the momentum row, the second wave's first lane the energy row
  if (tid == 0 || tid == 64) {
    double* row = tid == 0 ? row_px : row_en;
    double* d = s_prof + (tid == 0 ? 2 : 3) * n;
    double avg = 0.0;
    for (int j = n > 10 ? n - 10 : 0; j < n; ++j) avg = avg + row[j];
    avg = avg / 10.0;
    if (rel) { prof_smooth(row, d, n); prof_rescale(row, n, avg, u0, u2, a.xg); }
    else { prof_rescale(row, n, avg, u0, u2, a.xg); prof_smooth(row, d, n); }
  }
  __syncthreads();
  // ---- phase C
  const int it = I.i_trans;
  const double last = (1.0 - I.SMMOE) * row_px[n - 1] + I.SMMOE * row_en[n - 1];
  double s_art = 0.0;
  if (it > 0) {
    const double at = (1.0 - I.SMMOE) * row_px[it - 1] + I.SMMOE * row_en[it - 1];
    s_art = -(at - last) / a.tab[2 * n + it - 1];
  }
  for (int j = tid; j < n; j += PROF_THREADS) {
    const double u = a.ux[j + 1];
    const double pred = (1.0 - I.SMMOE) * row_px[j] + I.SMMOE * row_en[j];
    double v = pred;
    if (it > 0 && j >= it - 1 && j <= a.i_shock - 1) v = (-a.tab[2 * n + j]) * s_art + last;
    o[5 * n + j] = row_px[j];
    o[6 * n + j] = row_en[j];
    o[7 * n + j] = pred;
    o[8 * n + j] = (v + I.w * u) / (1.0 + I.w);
    o[9 * n + j] = (pred - u) / u0;
  }
  __syncthreads();
  if (tid == 0) {
    double S = 0.0;
    for (int j = 0; j < n; ++j) { const double sh = o[9 * n + j]; S = S + sh * sh; }
    s_sc[7] = mcsm::sqrt_(S / (double)n);
    unsigned long long bad = 0ull, outs = 0ull;
    int smax = 0;
    for (int k = 0; k < 8; ++k) { o[10 * n + k] = s_sc[k]; if (!__builtin_isfinite(s_sc[k])) ++bad; }
    for (long long k = 0; k < 10ll * n; ++k) if (!__builtin_isfinite(o[k])) ++bad;
    for (int k = 0; k < PROF_THREADS; ++k) { outs += (unsigned long long)s_out[k]; if (s_steps[k] > smax) smax = s_steps[k]; }
    a.diag[0] = bad; a.diag[1] = outs; a.diag[2] = (unsigned long long)smax;
  }
}

}  // namespace

// Host-callable launchers (pointers are device pointers; tables were uploaded by the caller)
extern "C" hipError_t mcs_launch_dndp_cr(const mcs_params* P, const double* psd, const double* gam_sf, const double* ux,
                                         const double* tabs /*mom_log|mom_edge|cos_edge|zone_pop*/, double rest_energy, double n0,
                                         double gam0, double* out_dndp, unsigned long long* diag, hipStream_t st) {
  ConsArgs a{};
  a.P = *P;
  const int NM = P->num_psd_mom_bins + 2, NT = P->num_psd_tht_bins + 2;
  a.psd = psd; a.gam_sf = gam_sf; a.ux = ux;
  a.mom_log = tabs; a.mom_edge = tabs + NM; a.cos_edge = tabs + 2 * NM; a.zone_pop = tabs + 2 * NM + NT;
  a.rest_energy = rest_energy; a.n0 = n0; a.gam0 = gam0;
  a.out_dndp = out_dndp; a.diag = diag;
  hipLaunchKernelGGL(mcs_k_dndp_cr, dim3(P->n_grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

extern "C" hipError_t mcs_launch_thermo(const mcs_params* P, const double* psd, const double* therm_pf,
                                        const unsigned long long* num_crossings, const double* gam_sf, const double* ux,
                                        const double* tabs /*cos_center|pt_center|zone_pop|density_loc|cold_pressure*/,
                                        double rest_energy, double mc, double n0, int therm_from_hist, double* scratch,
                                        double* out3 /*par|perp|edens, n_grid each*/, hipStream_t st) {
  ConsArgs a{};
  a.P = *P;
  const int NM = P->num_psd_mom_bins + 2, NT = P->num_psd_tht_bins + 2, ng = P->n_grid;
  a.psd = psd; a.therm_pf = therm_pf; a.num_crossings = num_crossings; a.gam_sf = gam_sf; a.ux = ux;
  a.cos_center = tabs; a.pt_center = tabs + NT; a.zone_pop = tabs + NT + NM; a.density_loc = tabs + NT + NM + ng;
  a.cold_pressure = tabs + NT + NM + 2 * ng;
  a.rest_energy = rest_energy; a.mc = mc; a.n0 = n0; a.therm_from_hist = therm_from_hist;
  a.scratch = scratch; a.out_par = out3; a.out_perp = out3 + ng; a.out_edens = out3 + 2 * ng;
  hipLaunchKernelGGL(mcs_k_thermo, dim3(P->n_grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

extern "C" hipError_t mcs_launch_dndp_esc(const mcs_params* P, const double* esc, const double* tabs /*mom_log|mom_edge|cos_edge*/,
                                          double rest_energy, const double gam_pf[2], double gam0, double* rows, unsigned int* row_diag,
                                          double* out, unsigned long long* diag, hipStream_t st) {
  EscArgs a{};
  const int NM = P->num_psd_mom_bins + 2;
  a.esc = esc; a.mom_log = tabs; a.mom_edge = tabs + NM; a.cos_edge = tabs + 2 * NM;
  a.rest_energy = rest_energy;
  for (int d = 0; d < 2; ++d) { a.gam[d][0] = gam_pf[d]; a.gam[d][1] = gam0; }
  a.nm = P->num_psd_mom_bins; a.nt = P->num_psd_tht_bins;
  a.rows = rows; a.row_diag = row_diag; a.out = out; a.diag = diag;
  const int lanes = 4 * (a.nt + 1);
  hipLaunchKernelGGL(mcs_k_dndp_esc_rows, dim3((lanes + ESC_ROWS_THREADS - 1) / ESC_ROWS_THREADS), dim3(ESC_ROWS_THREADS), 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mcs_k_dndp_esc_join, dim3(1), dim3(256), 0, st, a);
  return hipGetLastError();
}

extern "C" hipError_t mcs_launch_angle_dist(const mcs_params* P, const double* psd, const double* therm_sf, const unsigned long long* num_crossings,
                                            const double* gam_sf, const double* tabs /*pt_center|cos_center|cos_edge*/, double rest_energy,
                                            double gam0, int therm_from_hist, int n_win, const int32_t* l_lo, const int32_t* l_hi, double* out,
                                            hipStream_t st) {
  AngArgs a{};
  a.P = *P;
  const int NM = P->num_psd_mom_bins + 2, NT = P->num_psd_tht_bins + 2;
  a.psd = psd; a.therm_sf = therm_sf; a.num_crossings = num_crossings; a.gam_sf = gam_sf;
  a.pt_center = tabs; a.cos_center = tabs + NM; a.cos_edge = tabs + NM + NT;
  a.rest_energy = rest_energy; a.gam0 = gam0; a.therm_from_hist = therm_from_hist; a.n_win = n_win;
  for (int m = 0; m < n_win; ++m) { a.l_lo[m] = l_lo[m]; a.l_hi[m] = l_hi[m]; }
  a.out = out;
  hipLaunchKernelGGL(mcs_k_angle_dist, dim3(P->n_grid, 3), dim3(256), 0, st, a);
  return hipGetLastError();
}

extern "C" hipError_t mcs_launch_tcut_spectra(const mcs_params* P, const double* now, const double* base, const double* weight,
                                              const double* mom_log, const double* tcuts, int n_tcuts, double* out, unsigned int* row_neg,
                                              unsigned long long* diag, hipStream_t st) {
  TcutArgs a{};
  a.now = now; a.base = base; a.weight = weight; a.mom_log = mom_log; a.tcuts = tcuts;
  a.nm = P->num_psd_mom_bins; a.nt = n_tcuts;
  a.out = out; a.row_neg = row_neg; a.diag = diag;
  hipLaunchKernelGGL(mcs_k_tcut_rows, dim3(n_tcuts), dim3(64), 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mcs_k_tcut_index, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}

extern "C" hipError_t mcs_launch_detector_spectra(const mcs_params* P, const double* now_sf, const double* now_pf, const double* base,
                                                  const double* mom_log, const double* mom_edge, const double* x_spec, int n_det, int l_lo,
                                                  int l_hi, double x_unit, double* out, unsigned int* row_neg, unsigned long long* diag,
                                                  hipStream_t st) {
  DetArgs a{};
  a.now_sf = now_sf; a.now_pf = now_pf; a.base = base; a.mom_log = mom_log; a.mom_edge = mom_edge; a.x_spec = x_spec; a.x_unit = x_unit;
  a.nm = P->num_psd_mom_bins; a.nd = n_det; a.l_lo = l_lo; a.l_hi = l_hi;
  a.out = out; a.row_neg = row_neg; a.diag = diag;
  hipLaunchKernelGGL(mcs_k_detector_rows, dim3(2 * n_det), dim3(64), 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mcs_k_detector_join, dim3(1), dim3(DET_JOIN_THREADS), 0, st, a);
  return hipGetLastError();
}

// tab: pxx_EM | en_EM | atan_x; pres: P_par | P_perp | e_dens; the LDS rows take 4 n_grid doubles (the caller has checked that they fit)
extern "C" hipError_t mcs_launch_profile_update(const mcs_params* P, const mcs_profile_in* in, const double* pxx_flux, const double* energy_flux,
                                                const double* scalars, const double* ux, const double* gam_sf, const double* x_grid,
                                                const double* pres, const double* tab, double* out, unsigned long long* diag, hipStream_t st) {
  ProfArgs a{};
  a.in = *in;
  a.in.pxx_EM = a.in.en_EM = a.in.atan_x = nullptr;
  a.pxx_flux = pxx_flux; a.energy_flux = energy_flux; a.scalars = scalars;
  a.ux = ux; a.gsf = gam_sf; a.xg = x_grid; a.pres = pres; a.tab = tab;
  a.u0 = P->u0; a.beta0 = P->beta0; a.gam0 = P->gam0; a.n = P->n_grid; a.i_shock = P->i_shock;
  a.out = out; a.diag = diag;
  hipLaunchKernelGGL(mcs_k_profile_update, dim3(1), dim3(PROF_THREADS), sizeof(double) * 4 * (size_t)P->n_grid, st, a);
  return hipGetLastError();
}


// ---- K5: the synchrotron fold of the photon post-processing (include/mcs_synch.h) ------------------------
// One workgroup per grid zone, one thread per photon energy; every thread walks the electron momentum bins in the reference's
// order (synch_emission.jl:124-169), so a spectrum is the same sum in the same order on the CPU twin.  O(n_grid x n_photon x nmom)
// evaluations of F(x): 3e6 for the stock binning -- microseconds of the chip; it runs where the dN/dp it reads was made.
__global__ void __launch_bounds__(256) mcs_k_photon_synch(const double* __restrict__ dndp_pf /*[n_grid][NM]*/, const double* __restrict__ p_edge /*[NM]*/,
                                                         const double* __restrict__ btot /*[n_grid+2]*/, int NM, int n_photon, double log_emin_erg,
                                                         double bins_per_dec, double mc, double* __restrict__ out /*[n_grid][n_photon]*/) {
  __shared__ double s_d[KC_MAXB], s_p[KC_MAXB];
  const int zone = blockIdx.x + 1;
  for (int i = threadIdx.x; i < NM; i += blockDim.x) { s_d[i] = dndp_pf[(long long)(zone - 1) * NM + i]; s_p[i] = p_edge[i]; }
  __syncthreads();
  const double B = btot[zone];
  for (int j = threadIdx.x; j < n_photon; j += blockDim.x) {
    const double E = mcs_synch_energy(log_emin_erg, bins_per_dec, j);
    out[(long long)(zone - 1) * n_photon + j] = mcs_synch_fold_one(1.0e-99, s_d, s_p, NM - 2, B, mc, E);     // fill(1e-99), :64
  }
}

extern "C" hipError_t mcs_launch_photon_synch(const double* dndp_pf, const double* p_edge, const double* btot, int n_grid, int NM, int n_photon,
                                              double log_emin_erg, double bins_per_dec, double mc, double* out, hipStream_t st) {
  hipLaunchKernelGGL(mcs_k_photon_synch, dim3((unsigned)n_grid), dim3(256), 0, st, dndp_pf, p_edge, btot, NM, n_photon, log_emin_erg, bins_per_dec, mc, out);
  return hipGetLastError();
}

// ---- K7: the pion-decay fold of the photon post-processing (include/mcs_pion.h) --------------------------------
// One workgroup per grid zone.  First one thread per momentum bin prepares what does not depend on the photon energy (T_p, E_gamma^max,
// A_max, target density x count x speed: pion_kafexhiu.jl:171-193); then one thread per photon energy walks the bins in the reference's
// order, so a spectrum is the same sum in the same order on the CPU twin.  O(n_grid x n_photon x nmom) evaluations of F(T_p, E).
__global__ void __launch_bounds__(256) mcs_k_photon_pion(const double* __restrict__ dndp_pf /*[n_grid][NM]*/, const double* __restrict__ p_edge /*[NM]*/,
                                                        const double* __restrict__ target /*[n_grid]*/, int NM, int n_photon, double log_emin_erg,
                                                        double bins_per_dec, double mc, double aa, double scaling, int i_data,
                                                        double* __restrict__ out /*[n_grid][n_photon]*/) {
  __shared__ double s_pref[KC_MAXB], s_T[KC_MAXB], s_E[KC_MAXB], s_A[KC_MAXB];
  const int zone = blockIdx.x;
  const double n_t = target[zone];
  for (int i = threadIdx.x; i < NM - 1; i += blockDim.x) {
    const double d = dndp_pf[(long long)zone * NM + i];
    const double lo = p_edge[i], hi = p_edge[i + 1];
    const double cnt = d <= 1.0e-99 ? 1.0e-99 : d * (hi - lo);                                   // photon_pion_decay.jl:86-92
    double T = 0, v = 0, E = 1, A = 0;
    const int ok = mcs_pion_bin(cnt, lo, hi, mc, aa, i_data, &T, &v, &E, &A);
    s_pref[i] = ok ? n_t * cnt * v : 0.0; s_T[i] = T; s_E[i] = E; s_A[i] = A;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n_photon; j += blockDim.x) {
    const double e = pow(10.0, log_emin_erg + j * (1.0 / bins_per_dec));
    out[(long long)zone * n_photon + j] = mcs_pion_fold_one(s_pref, s_T, s_E, s_A, NM - 1, i_data, e, scaling);
  }
}
extern "C" hipError_t mcs_launch_photon_pion(const double* dndp_pf, const double* p_edge, const double* target, int n_grid, int NM, int n_photon,
                                             double log_emin_erg, double bins_per_dec, double mc, double aa, double scaling, int i_data, double* out,
                                             hipStream_t st) {
  hipLaunchKernelGGL(mcs_k_photon_pion, dim3((unsigned)n_grid), dim3(256), 0, st, dndp_pf, p_edge, target, NM, n_photon, log_emin_erg, bins_per_dec, mc,
                     aa, scaling, i_data, out);
  return hipGetLastError();
}

extern "C" hipError_t mcs_launch_dndp_2d(const mcs_params* P, const double* psd, const double* therm_sf, const unsigned long long* num_crossings,
                                         const double* tabs /*mom_edge[NM] | cos_center[NT] | pt_center[NM] | zone_pop[ng]*/, double rest_energy, double n0,
                                         int therm_from_hist, double gam_x, double beta_x, double* scratch, double* ef, hipStream_t st) {
  ConsArgs a{};
  a.P = *P;
  const int NM = P->num_psd_mom_bins + 2, NT = P->num_psd_tht_bins + 2;
  a.psd = psd; a.num_crossings = num_crossings;
  a.mom_edge = tabs; a.cos_center = tabs + NM; a.pt_center = tabs + NM + NT; a.zone_pop = tabs + 2 * NM + NT;
  a.rest_energy = rest_energy; a.n0 = n0; a.therm_from_hist = therm_from_hist; a.scratch = scratch;
  hipLaunchKernelGGL(mcs_k_dndp_2d, dim3(P->n_grid), dim3(256), 0, st, a, therm_sf, gam_x, beta_x, ef);
  return hipGetLastError();
}
extern "C" hipError_t mcs_launch_photon_ic(const double* ef, const double* p_edge, const double* field, int n_grid, int NM, int NT, int j_max, int n_nu,
                                           int n_photon, double log_min_rm, double bins_per_dec, double mc_e, double beam_area, double* out, hipStream_t st) {
  hipLaunchKernelGGL(mcs_k_photon_ic, dim3((unsigned)n_grid), dim3(256), 0, st, ef, p_edge, field, NM, NT, j_max, n_nu, n_photon, log_min_rm, bins_per_dec,
                     mc_e, beam_area, out);
  return hipGetLastError();
}

// ---- K9: the photon spectra an observer sees (include/mcs.h, "observed shell spectra"; DESIGN.md "K9") ---------------------------------
// mcs_k_photon_observe_zone: one workgroup per grid zone.  The zone's emission becomes a photon flux at Earth, one thread per energy
// (the conversions of the three host routines, each operation a separate rounding); inverse Compton is done with that.  Synchrotron and
// pion decay are re-binned by the Doppler-shifted energy of 180 slices in cos(theta): on the host a scatter (numpy's add.at, slices
// ascending and within a slice energies ascending), here a GATHER in that order -- one thread per target bin b walks the slices l in
// ascending order and adds, for each, the source bins j that land in b, ascending.  For a fixed slice the shifted energy
// mid[j] * fac[l] does not decrease with j (the launcher's caller checks: energies sorted, last_mid_ratio >= 1, gam > 0, 0 <= beta < 1),
// so those j are one contiguous range, found by two bisections over the products themselves: no table of targets, no atomics, and the
// same input gives the same bits.  LDS: 3 x 256 + 180 doubles.
#define KP_MAXN 256            // energies of a spectrum at the most (n_photon)
#define KP_NCOS 180            // get_summed_emission.jl:117

namespace {
// first j in [0, n] with mid[j] * fac > x (n: none)
__device__ __forceinline__ int p_first_above(const double* mid, int n, double fac, double x) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (mid[m] * fac > x) hi = m; else lo = m + 1; }
  return lo;
}
}  // namespace

__global__ void __launch_bounds__(256) mcs_k_photon_observe_zone(const double* __restrict__ emis /*[n_grid][n_photon]*/, const double* __restrict__ e_div,
                                                                const double* __restrict__ e_grid, const double* __restrict__ cos_edge /*[181]*/,
                                                                const double* __restrict__ gam, const double* __restrict__ beta,
                                                                const double* __restrict__ gam3, int process, int n_photon, double area, double dlog,
                                                                double last_mid_ratio, double* __restrict__ nb /*[n_grid][n_photon - 1]*/) {
  __shared__ double s_E[KP_MAXN], s_mid[KP_MAXN], s_num[KP_MAXN], s_fac[KP_NCOS];
  const int zone = blockIdx.x, n = n_photon - 1;                        // the last energy of a spectrum is not written out
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const double em = emis[(long long)zone * n_photon + j];
    double ef;                                                          // energy flux at Earth, floor 1e-99
    if (process == MCS_PHOTON_IC) ef = em > 1.0e-99 ? em / MCS_MEV_ERG : 1.0e-99;
    else if (process == MCS_PHOTON_SYNCH) { double fe = em / area; fe = fe > 1.0e-99 ? fe : 1.0e-99; ef = fe > 1.0e-99 ? fe / MCS_MEV_ERG : 1.0e-99; }
    else { const double fe = em / area; ef = fe >= 1.0e-99 ? fe : 1.0e-99; }
    const double f = ef <= 1.0e-99 ? 1.0e-99 : ef / e_div[j];            // photons per d(log E)
    const double per_bin = f > 1.0e-90 ? f * dlog : f;
    if (process == MCS_PHOTON_IC) nb[(long long)zone * n + j] = per_bin;  // (computed in the observer's frame)
    else { s_num[j] = per_bin / KP_NCOS; s_E[j] = e_grid[j]; }
  }
  if (process == MCS_PHOTON_IC) return;
  const double g = gam[zone], bt = beta[zone];
  for (int l = threadIdx.x; l < KP_NCOS; l += blockDim.x) s_fac[l] = g * __builtin_sqrt((1 - bt * cos_edge[l]) * (1 - bt * cos_edge[l + 1]));
  __syncthreads();
  for (int j = threadIdx.x; j < n - 1; j += blockDim.x) s_mid[j] = __builtin_sqrt(s_E[j] * s_E[j + 1]);
  __syncthreads();
  if (threadIdx.x == 0) s_mid[n - 1] = s_mid[n - 2] * last_mid_ratio;
  __syncthreads();
  for (int b = threadIdx.x; b < n; b += blockDim.x) {
    double acc = 1.0e-99;
    if (b < n - 1) {                                                    // (a photon shifted to the last energy or beyond is dropped: S3)
      const double e_lo = s_E[b], e_hi = s_E[b + 1];
      for (int l = 0; l < KP_NCOS; ++l) {
        const double fac = s_fac[l];
        const int j0 = b == 0 ? 0 : p_first_above(s_mid, n, fac, e_lo);  // (the search for the target starts at the second energy)
        const int j1 = p_first_above(s_mid, n, fac, e_hi);
        for (int j = j0; j < j1; ++j) { const double v = s_num[j]; if (v > 1.0e-99) acc += v; }
      }
    }
    nb[(long long)zone * n + b] = acc > 1.0e-95 ? acc * gam3[zone] : 1.0e-99;
  }
}

// mcs_k_photon_observe_shells: one thread per energy; shells ascending, within a shell its zones ascending, then the row of all shells.
__global__ void __launch_bounds__(256) mcs_k_photon_observe_shells(const double* __restrict__ nb /*[n_grid][n]*/, const double* __restrict__ ends /*[n_shells+1]*/,
                                                                  int n, int n_shells, double* __restrict__ out /*[n_shells+1][n]*/) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double all = 0.0;
  for (int s = 0; s < n_shells; ++s) {
    const int lo = (int)ends[s], hi = (int)ends[s + 1] - 1;
    double sh = 1.0e-99;
    if (lo >= 1 && hi >= lo) {
      double a = 0.0;
      for (int z = lo; z <= hi; ++z) { const double v = nb[(long long)(z - 1) * n + k]; a += v > 1.0e-95 ? v : 0.0; }      // S6
      sh = a > 1.0e-99 ? a : 1.0e-99;
    }
    out[(long long)s * n + k] = sh;
    all += sh > 1.0e-99 ? sh : 0.0;
  }
  out[(long long)n_shells * n + k] = all > 1.0e-99 ? all : 1.0e-99;
}

extern "C" hipError_t mcs_launch_photon_observe(const double* emis, const double* tabs /*e_div[np] | e_grid[np] | cos_edge[181] | gam | beta | gam3 [n_grid] | ends*/,
                                                int process, int n_grid, int n_photon, double area, double dlog, double last_mid_ratio, int n_shells,
                                                double* nb, double* out, hipStream_t st) {
  const double *e_div = tabs, *e_grid = tabs + n_photon, *cos_edge = tabs + 2 * n_photon, *gam = cos_edge + KP_NCOS + 1;
  const double *beta = gam + n_grid, *gam3 = beta + n_grid, *ends = gam3 + n_grid;
  const int n = n_photon - 1;
  hipLaunchKernelGGL(mcs_k_photon_observe_zone, dim3((unsigned)n_grid), dim3(256), 0, st, emis, e_div, e_grid, cos_edge, gam, beta, gam3, process, n_photon, area,
                     dlog, last_mid_ratio, nb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mcs_k_photon_observe_shells, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, nb, ends, n, n_shells, out);
  return hipGetLastError();
}

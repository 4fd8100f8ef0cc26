// mcs_transport_f32.inc -- the fp32-STATE variant of K1 (BASELINE config[4]: "fp32-state variant vs fp64 tolerance
// study").  Included at the end of mcs_transport.hip: it shares that file's LDS tables, staging arrays and the fp64
// tally functions.
//
// The reference is fp64 throughout (src/MonteCarloScattering.jl:556-585); cgs values such as p ~ 1e-17 g cm/s,
// p^2 ~ 1e-34 or the 1e-99 floors do not exist in fp32, so the particle state is kept in NORMALISED units:
//     momentum  p^ = p / (m_p c)            velocity  in c          mass  aa (= m / m_p)
//     length    x^ = x / L0,  L0 = rg0 = gamma0 beta0 m_p c^2 / (e B[0])   (the reference's rg0, from table entry 0)
//     time      t^ = t c / L0               field     in gauss (1e-6 .. 1e1: fine as it is)
//     gyro      g^ = m_p c^2 / (L0 Z e B):  r_g^ = p^ g^,   T_g^ = 2 pi gamma aa g^
// What is fp32: the per-particle state and every per-step operation of the helix loop -- scatter, clock, move, event
// tests, PRP logic, the retro walk, radiative losses (src/particle_loop.jl:154-499, src/scattering.jl,
// src/prob_return.jl).  What stays fp64: the population in HBM (the ABI and K2 / K3 are unchanged: the state is
// converted when a particle is loaded or saved), all tallies and the code that produces a tally from a state
// (transform_p_PS, bin look-ups: flux_tally, particle_finish, tcut_track get the state converted to cgs doubles), and the
// two rare momentum transforms that happen at most once per zone crossing (transform_p_PSP at a change of flow speed,
// do_energy_transfer), which reuse the fp64 functions on converted values.
// Random numbers: the same Philox stream as the fp64 path (key, draw order), a draw being the top 24 bits of the
// same 64-bit word -- so a history starts out identical and then drifts apart as roundings differ; the comparison with
// fp64 is statistical (DESIGN.md, "fp32-state variant").
//
// Organisation: one lane = one live particle, persistent lanes with a wave-aggregated claim of new particles, every
// lane running the reference's loop body as written (divergent code, tallies made on the spot).  None of the
// fp64 kernel's batching (flag-driven common pass, record stacks, parking, consolidation) is repeated here: this
// variant exists to measure what fp32 state does to the spectra, at a rate that makes 1e6-particle studies cheap.

namespace {

struct F32Units { double L0, P0, T0, invL0; };     // cgs per normalised unit: length, momentum, time

struct Pf {
  float w, ptot, pb, pperp, gam, x, x_old, phi, prp, acc, acc_c, xn;   // acc_c: Kahan compensation of the clock (see add_time)
  float gd, gr, grt, gper, t_step;
  float ux, gsf, gef, bsin, bcos, bmag;      // properties of zone ig3 (the zone Code Block 3 last ran in)
  float z_lo, z_hi;                            // edges of zone i_grid
  int i_grid, i_grid_old, ig3, helix, tcut, n_retro, i_return;
  bool downstream, inj;
};

// fp32 primitives of both fp32 kernels (the plain loop below and the organised kernel in mcs_transport_f32k.inc): hardware
// reciprocal / square root / sine / cosine -- one instruction each, ~1 ulp (sin / cos: ~1e-6 absolute, argument in revolutions) --
// instead of the IEEE-correct library sequences (10-60 instructions).  The variant is a statistical one (DESIGN.md section 4b);
// both kernels use the SAME functions in the same order, so they agree bit for bit with each other.
// X (EXACT): the same functions from correctly rounded fp32 operations only (include/mcs_math_f32.h) -- the form the CPU restatement
// (oracle/mcs_oracle_f32.inc) reproduces bit for bit; kernel mcs_k_transport_f32_loop_exact (MCS_F32_EXACT=1).  Default: hardware.
template <bool X = false> __device__ __forceinline__ float fdv(float a, float b) { if constexpr (X) return mcsf::div_(a, b); else return a * __builtin_amdgcn_rcpf(b); }
template <bool X = false> __device__ __forceinline__ float frcp(float b) { if constexpr (X) return mcsf::rcp_(b); else return __builtin_amdgcn_rcpf(b); }
template <bool X = false> __device__ __forceinline__ float fsq(float x) { if constexpr (X) return mcsf::sqrt_(x); else return __builtin_amdgcn_sqrtf(x); }
template <bool X = false> __device__ __forceinline__ float cos_rad(float x) { if constexpr (X) return mcsf::cos_rad_(x); else return __builtin_amdgcn_cosf(x * 0.15915494f); }
template <bool X = false> __device__ __forceinline__ void sincos_revf(float r, float& s, float& c) {      // sin / cos of 2 pi r
  if constexpr (X) mcsf::sincos_rev_(r, &s, &c); else { s = __builtin_amdgcn_sinf(r); c = __builtin_amdgcn_cosf(r); }
}
template <bool X = false> __device__ __forceinline__ float hyp1(float x) { return fsq<X>(x * x + 1.f); }                     // hypot(x, 1), |x| < 1e18
template <bool X = false> __device__ __forceinline__ float asin_f(float x) {
  // |x| <= 0.5: x + x^3 P(x^2); else pi/2 - 2 asin(sqrt((1 - |x|) / 2)) (the classic reduction; P: minimax of (asin(x) - x) / x^3)
  const float ax = __builtin_fabsf(x);
  const bool big = ax > 0.5f;
  const float z = big ? 0.5f * (1.f - ax) : x * x;
  const float r = big ? fsq<X>(z) : ax;
  float pl = 0.0421632007f;
  pl = pl * z + 0.0241813120f; pl = pl * z + 0.0454700254f; pl = pl * z + 0.0749530047f; pl = pl * z + 0.1666675359f;
  const float v = r + r * z * pl;
  const float res = big ? 1.5707964f - 2.f * v : v;
  return __builtin_copysignf(res, x);
}

__device__ __forceinline__ float unitf(uint32_t hi) { return (float)(hi >> 8) * 0x1.0p-24f; }
__device__ __forceinline__ float randf(Rng& rng) {           // one draw: index n, skip n+1 (as Rng::rand)
  const uint32_t j = rng.n; rng.n = j + 2u;
  uint32_t o0, o1, o2, o3;
  philox_block(j >> 1, 0u, 0u, 0u, rng.k0, rng.k1, o0, o1, o2, o3);
  return unitf(o1);
}
__device__ __forceinline__ void pairf(Rng& rng, float& u1, float& u2) {
  const uint32_t j = rng.n; rng.n = j + 2u;
  uint32_t o0, o1, o2, o3;
  philox_block(j >> 1, 0u, 0u, 0u, rng.k0, rng.k1, o0, o1, o2, o3);
  u1 = unitf(o1); u2 = unitf(o3);
}
__device__ __forceinline__ float mod2pif(float x) {
  const float t = 6.2831855f;
  float r = x - t * floorf(x * 0.15915494f);
  if (r < 0.f) r += t;
  if (r >= t) r -= t;
  return r;
}

// The acceleration clock sums ~1e4 steps per pcut over 40 pcuts and ends 1e9 times larger than its early increments:
// a bare fp32 sum loses whole steps (measured: 15 % more age-limit exits than fp64).  Compensated (Kahan) summation
// keeps the state fp32 -- two floats -- and the clock exact to fp32 rounding of the total.
__device__ __forceinline__ void add_time(Pf& p, float dt) {
  const float y = dt - p.acc_c;
  const float t = p.acc + y;
  p.acc_c = (t - p.acc) - y;
  p.acc = t;
}

// zone edge j in normalised units, as every comparison of the fp32 path sees it
__device__ __forceinline__ float edgef(int j, const F32Units& U) { return (float)(S_x[j] * U.invL0); }

// src/all_flux.jl:68-72 on the fp32 position
__device__ __forceinline__ int zone_search_f(float x, bool fwd, int i_grid, int ne, const F32Units& U) {
  if (fwd) { for (int j = i_grid + 1; j < ne; ++j) if (edgef(j, U) > x) return j - 1; }
  else { for (int j = i_grid; j >= 0; --j) if (edgef(j, U) <= x) return j; }
  return -1;
}

__device__ __forceinline__ void load_zone_f(Pf& p, int z, CK* a, const F32Units& U, bool custom_epsB, float x_stop) {
  p.ig3 = z;
  p.ux = (float)(S_ux[z] / MCS_C); p.gsf = (float)S_gsf[z]; p.gef = (float)S_gef[z];
  p.bsin = (float)S_bsin[z]; p.bcos = (float)S_bcos[z];
  double bm = S_bt[z];
  if (custom_epsB && p.x > x_stop) bm = S_bt[a->P.n_grid] * __builtin_sqrt((double)x_stop / (double)p.x);
  p.bmag = (float)bm;
  p.gd = (float)((MCS_MP * MCS_C * MCS_C * U.invL0) / (a->zzq * bm));
}

// the state as cgs doubles, for the fp64 tally functions
struct Cgs { double pb, pperp, ptot, gam, phi, w, x, x_old; };
__device__ __forceinline__ Cgs to_cgs(const Pf& p, const F32Units& U) {
  Cgs c;
  c.pb = (double)p.pb * U.P0; c.pperp = (double)p.pperp * U.P0; c.ptot = (double)p.ptot * U.P0; c.gam = (double)p.gam;
  c.phi = (double)p.phi; c.w = (double)p.w; c.x = (double)p.x * U.L0; c.x_old = (double)p.x_old * U.L0;
  return c;
}

// src/scattering.jl:29-101 in fp32, in pieces: what depends on slowly varying quantities only (the organised kernel caches it)
// and the per-step core.  cos_max depends on xn_per and eta only (r_g cancels, scattering.jl:60).
__device__ __forceinline__ float gper_f(float aa, float ptot, float gam, float gd, float pe_crit, float game_crit) {
  return (aa < 1.f && ptot < pe_crit) ? 6.2831855f * game_crit * aa * gd : 6.2831855f * gam * aa * gd;
}
template <bool X = false> __device__ __forceinline__ float omc_f(float xn, float eta) { return 1.f - cos_rad<X>(fsq<X>(fdv<X>(6.f * 6.2831855f, xn * eta))); }   // 1 - cos_max
template <bool X = false> __device__ __forceinline__ void scatter_core_f(float u1, float u2, float omc, float ptot, float& pb, float& pperp, float& phi) {
  const float rp = frcp<X>(ptot);
  const float cos_old = pb * rp, sin_old = pperp * rp;
  const float cos_d = 1.f - u1 * omc;
  const float sin_d = fsq<X>(fmaxf(1.f - cos_d * cos_d, 0.f));
  const float rev = u2 - 0.5f;                                       // phi_scat = 2 pi U2 - pi, in revolutions
  float s_ps, c_ps;
  sincos_revf<X>(rev, s_ps, c_ps);
  const float cos_new = cos_old * cos_d + sin_old * sin_d * c_ps;
  const float sin_new = fsq<X>(fmaxf(1.f - cos_new * cos_new, 0.f));
  pb = ptot * cos_new;
  pperp = ptot * sin_new;
  float sd = fdv<X>(s_ps * sin_d, sin_new);
  sd = fminf(fmaxf(sd, -0.99999994f), 0.99999994f);                  // prevfloat(1.0f): scattering.jl:3,96-98 (a NaN -- sin_new == 0 -- is discarded)
  const float adj = asin_f<X>(sd);
  phi = sin_new != 0.f ? phi + adj : phi;
}
template <bool X = false> __device__ __forceinline__ void scattering_f(CK* a, Rng& rng, Pf& p, float aa, float eta, float pe_crit, float game_crit) {
  p.gper = gper_f(aa, p.ptot, p.gam, p.gd, pe_crit, game_crit);
  float u1, u2;
  pairf(rng, u1, u2);
  scatter_core_f<X>(u1, u2, omc_f<X>(p.xn, eta), p.ptot, p.pb, p.pperp, p.phi);
}

// src/particle_loop.jl:578-592 with the loss constant in normalised units (krad = rad_loss_fac * P0 * T0, B in gauss)
template <bool X = false> __device__ __forceinline__ float radiation_loss_f(float krad, float B2, float pp, float dt) {
  const float dlnp = krad * B2 * pp * dt;
  return dlnp > 1.0e-2f ? fdv<X>(pp, 1.f + dlnp) : pp * (1.f - dlnp);
}

// src/prob_return.jl:217-344 (D1; capped: MCS_RETRO_CAP) in fp32.  Returns 0 = back at the PRP, 1 = all energy lost, 2 = capped.
template <bool X = false> __device__ __forceinline__ int retro_time_f(CK* a, Rng& rng, Pf& p, const F32Units& U, float aa, float krad, float x_stop, float tscale) {
  const auto& P = a->P;
  const int ng = P.n_grid;
  const float xn = (float)MCS_RETRO_XN_PER;
  const float phi_step = 6.2831855f / xn;
  float gd = p.gd;
  const float ux = -(float)(S_ux[ng] / MCS_C), gsf = (float)S_gsf[ng], gef = (float)S_gef[ng];
  const float bcos = (float)S_bcos[ng], bsin = (float)S_bsin[ng];
  float B = (float)S_bt[ng];
  if (P.use_custom_epsB) B *= fsq<X>(fdv<X>(x_stop, p.prp));
  const float Bc = (float)P.B_CMBz * gef;
  float B2 = B * B + Bc * Bc;
  float x = p.prp;
  p.phi = randf(rng) * 6.2831855f;
  const int n_tcuts = a->tb.n_tcuts;
  const int n0 = p.n_retro;
  int rc = 0;
  while (true) {
    ++p.n_retro;
    const float phi_old = p.phi;
    if (P.use_custom_epsB) {
      B = (float)S_bt[ng] * fsq<X>(fdv<X>(x_stop, x));
      B2 = B * B + Bc * Bc;
      gd = (float)((MCS_MP * MCS_C * MCS_C * U.invL0) / (a->zzq * (double)B));
    }
    const float t_fac = fdv<X>(6.2831855f * aa * gd, xn);
    const float gr = p.pperp * gd;
    p.phi = mod2pif(phi_old + phi_step);
    const float t_step = t_fac * p.gam;
    const float x_move = fdv<X>(p.pb * t_fac, aa);
    float gyr = 0.f;
    if (bsin != 0.f) gyr = gr * bsin * (cos_rad<X>(p.phi) - cos_rad<X>(phi_old));
    x = x + gsf * (x_move * bcos - gyr + ux * t_step);
    add_time(p, t_step * gef);
    if (P.do_tcuts) {
      if (p.tcut > n_tcuts) cnt(a, MCS_IC_TCUT_OVERRUN);
      else if (p.acc >= (float)(S_tc[p.tcut - 1] * tscale)) {
        tcut_track(a, p.tcut, (double)p.w, (double)p.ptot * U.P0);
        p.tcut += 1;
      }
    }
    p.phi = 6.2831855f * randf(rng);
    const float ptot_old = p.ptot;
    p.pb = (2.f * randf(rng) - 1.f) * p.ptot;
    p.pperp = fsq<X>(fmaxf(p.ptot * p.ptot - p.pb * p.pb, 0.f));
    const float cn = fdv<X>(p.pb, ptot_old), sn = fdv<X>(p.pperp, ptot_old);
    if (P.do_rad_losses && aa < 1.f) p.ptot = radiation_loss_f<X>(krad, B2, p.ptot, t_step);
    if (p.ptot <= 0.f) { p.ptot = 1e-30f; p.gam = 1.f; rc = 1; break; }
    p.pb = p.ptot * cn; p.pperp = p.ptot * sn;
    p.gam = hyp1<X>(fdv<X>(p.ptot, aa));
    if (x < p.prp) break;
    if (p.n_retro - n0 >= a->retro_cap) { cnt(a, MCS_IC_RETRO_CAP); rc = 2; break; }
  }
  p.gd = gd;
  return rc;
}

}  // namespace

// One helix pass of one particle (the body of `while keep_looping`, src/particle_loop.jl:154-499) in fp32.
// Returns -1 to go on, else the end code (0 = saved for the next pcut, 1..4 = i_reason).
template <bool X = false> __device__ __forceinline__ int f32_pass(CK* a, Rng& rng, Pf& p, const F32Units& U, long long k) {
  const auto& P = a->P;
  const float aa = (float)a->aa;
  const float eta = (float)P.eta_mfp, u2c = (float)(P.u2 / MCS_C);
  const float x_stop = (float)(P.x_grid_stop * U.invL0);
  const float pe_crit = (float)(P.pe_crit / U.P0), game_crit = (float)P.game_crit;
  const float krad = (float)(MCS_RAD_LOSS_FAC * U.P0 * U.T0);
  const float tscale_f = (float)(1.0 / U.T0);
  const bool custom_epsB = P.use_custom_epsB != 0;
  const int ne = P.n_grid + 2, n_tcuts = a->tb.n_tcuts;

  p.helix += 1;
  if (p.helix > MCS_HELIX_CAP) { cnt(a, MCS_IC_HELIX_CAP); return 1; }               // quirk Q5
  if (p.i_return == 1) {                                                              // Code Block 1
    if (p.ptot < fabsf(p.pb)) { cnt(a, MCS_IC_PPERP_CLAMP); p.pperp = 1.0e-6f * p.ptot; }
    else p.pperp = fsq<X>(p.ptot * p.ptot - p.pb * p.pb);
    p.gr = p.pperp * p.gd;
  } else {                                                                            // Code Block 3
    const int io = p.ig3;
    const float ux_old = p.ux;
    load_zone_f(p, p.i_grid, a, U, custom_epsB, x_stop);
    if (p.ux != ux_old) {                 // transform_p_PSP (transformers.jl:523-607): rare, in fp64 on converted values
      const Mom r = transform_p_PSP(a, io, p.i_grid, (double)p.pb * U.P0, (double)p.pperp * U.P0, (double)p.gam, (double)p.phi);
      p.ptot = (float)(r.ptot / U.P0); p.pb = (float)(r.pb / U.P0); p.pperp = (float)(r.pperp / U.P0);
      p.gam = (float)r.gam; p.phi = (float)r.phi;
      p.gr = p.pperp * p.gd; p.grt = p.ptot * p.gd;       // (only here, as in the reference: particle_loop.jl:225-226)
    }
    if (P.energy_transfer_frac > 0 && !p.inj && p.x_old <= 0.f && p.i_grid_old != p.i_grid) {
      Mom r; r.ptot = (double)p.ptot * U.P0; r.pb = (double)p.pb * U.P0; r.pperp = (double)p.pperp * U.P0; r.gam = (double)p.gam; r.phi = 0;
      r = do_energy_transfer(a, p.i_grid, p.i_grid_old, (double)p.w, r);
      p.ptot = (float)(r.ptot / U.P0); p.pb = (float)(r.pb / U.P0); p.pperp = (float)(r.pperp / U.P0); p.gam = (float)r.gam;
    }
    if (P.dont_scatter && p.x > 10.f * p.gr) return 1;
    if ((double)p.ptot * U.P0 > a->pmax_cutoff) {
      double ptot_sk, px, py, pz, gam_sk;
      transform_p_PS(a->aa, (double)p.pb * U.P0, (double)p.pperp * U.P0, (double)p.gam, (double)p.phi, S_ux[p.ig3], S_gsf[p.ig3],
                     S_bcos[p.ig3], S_bsin[p.ig3], ptot_sk, px, py, pz, gam_sk);
      if (ptot_sk > a->pmax_cutoff) return 2;
    }
    if (p.inj && p.x < (float)(P.feb_upstream * U.invL0)) return 2;
    if (P.age_max > 0 && p.acc > (float)(P.age_max / U.T0)) return 3;
    if (P.do_rad_losses && aa < 1.f) {
      const float ptot_old = p.ptot;
      const float Bc = (float)P.B_CMBz * p.gef;
      p.ptot = radiation_loss_f<X>(krad, p.bmag * p.bmag + Bc * Bc, p.ptot, p.t_step);
      if (p.ptot <= 0.f) { p.ptot = 1e-30f; p.pb = 1e-30f; p.pperp = 1e-30f; p.gam = 1.f; return 4; }
      p.gam = hyp1<X>(fdv<X>(p.ptot, aa));
      const float r = fdv<X>(p.ptot, ptot_old);
      p.pb *= r; p.pperp *= r;
      p.grt = p.ptot * p.gd; p.gr = p.pperp * p.gd;
    }
    if (!P.dont_scatter) scattering_f<X>(a, rng, p, aa, eta, pe_crit, game_crit);
    if (p.downstream) {
      add_time(p, p.t_step * p.gef);
      if (P.do_tcuts) {
        if (p.tcut > n_tcuts) cnt(a, MCS_IC_TCUT_OVERRUN);
        else if (p.acc >= (float)(S_tc[p.tcut - 1] * tscale_f)) { tcut_track(a, p.tcut, (double)p.w, (double)p.ptot * U.P0); p.tcut += 1; }
      }
      if ((double)p.ptot * U.P0 > a->pcut) {                          // saved for the next pcut (particle_loop.jl:361-380)
        a->l_save[k] = 1;
        a->sv.weight[k] = (double)p.w; a->sv.ptot_pf[k] = (double)p.ptot * U.P0; a->sv.pb_pf[k] = (double)p.pb * U.P0;
        a->sv.x_PT_cm[k] = (double)p.x * U.L0; a->sv.xn_per[k] = (double)p.xn;
        a->sv.prp_x_cm[k] = (double)(p.x < p.prp ? p.prp : p.x * 1.1f) * U.L0;
        a->sv.acctime_sec[k] = ((double)p.acc - (double)p.acc_c) * U.T0; a->sv.phi_rad[k] = (double)p.phi;
        a->sv.meta[k] = mcs_pack_meta(p.i_grid, p.tcut, p.downstream, p.inj);
        cnt(a, MCS_IC_COUNT);
        return 0;
      }
    }
    p.xn = p.x > p.grt ? (float)P.xn_per_coarse : (float)P.xn_per_fine;
  }

  // ---- Code Block 2: the move (no_DSA_loop, particle_loop.jl:510-571)
  p.x_old = p.x;
  const float phi_old = p.phi;
  p.t_step = fdv<X>(p.gper, p.xn);
  const float inj_frac = (float)a->inj_frac;
  while (true) {
    p.phi = mod2pif(p.phi + fdv<X>(6.2831855f, p.xn));
    const float x_move = fdv<X>(p.pb * p.t_step, p.gam * aa);
    float gyr = 0.f;
    if (p.bsin != 0.f) gyr = p.gr * p.bsin * (cos_rad<X>(p.phi) - cos_rad<X>(phi_old));
    p.x = p.x_old + p.gsf * (x_move * p.bcos - gyr + p.ux * p.t_step);
    if (p.x <= 0.f && p.x_old > 0.f && !p.inj && (P.dont_DSA || inj_frac < 1.f)) {
      if (P.dont_DSA || randf(rng) > inj_frac) { if (p.pb < 0.f) p.pb = -p.pb; else p.phi = randf(rng) * 6.2831855f; }
      else break;
    } else break;
  }
  if (p.x_old < 0.f && p.x >= 0.f) {
    p.downstream = true;
    const float L_diff = fdv<X>(eta / 3.f * p.grt * p.ptot, aa * p.gam * u2c);
    p.prp = fmaxf(p.prp, L_diff);
  }
  if (p.downstream && p.x < 0.f) p.inj = true;

  // all_flux! (all_flux.jl:45-162)
  p.i_grid_old = p.i_grid;
  {
    const bool fwd = p.x > p.x_old;
    const bool same = fwd ? (p.z_hi > p.x) : (p.z_lo <= p.x);
    if (!same) {
      const int found = zone_search_f(p.x, fwd, p.i_grid, ne, U);
      if (found < 0) { cnt(a, MCS_IC_ZONE_FAIL); return 3; }            // D6
      p.i_grid = found;
      p.z_lo = edgef(found, U); p.z_hi = edgef(found + 1, U);
    }
    if (!(p.i_grid == p.i_grid_old && p.i_grid > P.i_grid_feb && a->tb.n_xspec == 0)) {
      const Cgs c = to_cgs(p, U);
      flux_tally(a, c.pb, c.pperp, c.ptot, c.gam, c.phi, c.w, c.x, c.x_old, p.i_grid, p.i_grid_old, p.ig3, p.inj);
    }
  }

  // downstream_test (particle_loop.jl:595-637) and prob_return (prob_return.jl:36-173)
  p.i_return = 2;
  bool do_prob_ret = true;
  if (P.feb_downstream > 0 && p.x > (float)(P.feb_downstream * U.invL0)) { p.i_return = 0; do_prob_ret = false; }
  else if (p.x > 1.1f * p.prp) {
    float v_fac;
    if (aa < 1.f && p.ptot < pe_crit) v_fac = fdv<X>(pe_crit * p.gd * pe_crit, aa * game_crit * u2c);
    else v_fac = fdv<X>(p.grt * p.ptot, aa * p.gam * u2c);
    if (p.x > 6.91f * (eta / 3.f * v_fac)) { p.i_return = 0; do_prob_ret = false; }
  }
  int lose = 0;
  if (do_prob_ret) {
    if (p.x < x_stop) {
    } else if (p.x_old < x_stop && x_stop <= p.x) {
      const float gyro_tmp = (custom_epsB && p.x > x_stop) ? fsq<X>(fdv<X>(x_stop, p.x)) : 1.f;
      const float grt2 = p.ptot * gyro_tmp * (float)((MCS_MP * MCS_C * MCS_C * U.invL0) / (MCS_QCGS * P.bmag2));
      p.prp = p.x + 3.f * fdv<X>(eta / 3.f * grt2 * p.ptot, aa * p.gam * u2c);
    } else if (p.x_old < p.prp && p.x >= p.prp) {
      const float vt = fdv<X>(p.ptot, p.gam * aa);
      const float q = fdv<X>(vt - u2c, vt + u2c);
      if (vt < u2c || randf(rng) > q * q) p.i_return = 0;
      else {
        p.i_return = 1;
        lose = retro_time_f<X>(a, rng, p, U, aa, krad, x_stop, tscale_f);
        if (lose) p.i_return = 0;
        p.x = p.prp;
      }
    } else if (aa < 1.f && (double)p.ptot * U.P0 < a->pcut_prev && p.helix % 1000 == 0) {
      const float L_diff = fdv<X>(eta / 3.f * (p.ptot * p.gd) * p.ptot, aa * p.gam * u2c);
      if (p.x > 2.0e3f * L_diff) p.prp = 0.8f * p.x;
      else {
        const float r = fdv<X>((float)(a->pcut_prev / U.P0), p.ptot);
        const float r2 = r * r;
        p.prp = fminf(p.prp, x_stop + L_diff * (r2 * r2 * r));
      }
    }
  }
  if (p.i_return == 0) {
    if (lose == 2) return 3;   // MCS_RETRO_CAP: nothing added to the downstream sums
    const double m = a->m, pt = (double)p.ptot * U.P0, gm = (double)p.gam;
    double vel = pt / m;
    if ((gm - 1) >= MCS_E_REL_PT) vel /= gm;
    sadd(0, pt / 3 * vel * (double)p.w * a->density);
    sadd(1, (gm - 1) * m * (MCS_C * MCS_C) * (double)p.w * a->density);
    return lose == 1 ? 4 : 1;
  }
  return -1;
}

template <bool X> __device__ __forceinline__ void f32_loop_body(const KArgs* __restrict__ ka) {
  CK* a = (CK*)ka;
  if (a->n_dev && *a->n_dev == 0) return;
  block_prologue(a);
  __syncthreads();
  F32Units U;
  U.L0 = a->P.gam0 * a->P.beta0 * MCS_MP * MCS_C * MCS_C / (MCS_QCGS * S_bt[0]);
  U.P0 = MCS_MP * MCS_C; U.T0 = U.L0 / MCS_C; U.invL0 = 1.0 / U.L0;
  const unsigned lane = __lane_id();
  const unsigned long long n = (unsigned long long)(a->n_dev ? *a->n_dev : a->n);
  const float x_stop = (float)(a->P.x_grid_stop * U.invL0);
  Pf p;
  Rng rng; rng.init(0ull);
  p.helix = 0; p.n_retro = 0;
  bool active = false, exhausted = false;
  long long k = -1;
  while (true) {
    // wave-aggregated claim of new particles for the idle lanes
    const unsigned long long idle = ~__builtin_amdgcn_ballot_w64(active);
    if (!exhausted && (__popcll(idle) >= 8 || idle == ~0ull)) {      // (batched: a claim stalls the wave for a memory latency)
      const int nidle = __popcll(idle), leader = __ffsll((long long)idle) - 1;
      unsigned long long base = 0;
      if ((int)lane == leader) base = atomicAdd(a->work_counter, (unsigned long long)nidle);
      base = __shfl(base, leader);
      if (base >= n) exhausted = true;
      else if (!active) {
        const unsigned long long idx = base + below(idle);
        if (idx < n) {
          k = (long long)idx;
          p.w = (float)a->in.weight[k];
          p.ptot = (float)(a->in.ptot_pf[k] / U.P0); p.pb = (float)(a->in.pb_pf[k] / U.P0);
          p.x = (float)(a->in.x_PT_cm[k] * U.invL0); p.xn = (float)a->in.xn_per[k];
          p.prp = (float)(a->in.prp_x_cm[k] * U.invL0);
          { const double t = a->in.acctime_sec[k] / U.T0; p.acc = (float)t; p.acc_c = -(float)(t - (double)p.acc); }   // hi + lo of the fp64 clock
          p.phi = (float)a->in.phi_rad[k];
          const uint32_t meta = a->in.meta[k];
          p.i_grid = (int)(meta & 0xffffu); p.tcut = (int)((meta >> 16) & 0xffu);
          p.downstream = (meta >> 24) & 1u; p.inj = (meta >> 25) & 1u;
          p.i_grid_old = p.i_grid;
          p.helix = 0; p.n_retro = 0; p.i_return = -1; p.t_step = 0.f; p.x_old = 0.f;
          rng.init(a->seed_base + (unsigned long long)((a->gidx ? a->gidx[k] : a->i_prt_offset + k * a->i_prt_stride) + 1));
          // prologue of particle_loop (particle_loop.jl:44-153)
          const float aa = (float)a->aa;
          p.gam = hyp1<X>(fdv<X>(p.ptot, aa));
          load_zone_f(p, p.i_grid, a, U, a->P.use_custom_epsB != 0, x_stop);
          if (a->P.use_custom_epsB && p.x > x_stop) p.gd = (float)((MCS_MP * MCS_C * MCS_C * U.invL0) / (a->zzq * S_bt[p.i_grid])) * fsq<X>(fdv<X>(p.x, x_stop));
          p.grt = p.ptot * p.gd; p.gper = 6.2831855f * p.gam * aa * p.gd;
          if (p.ptot < fabsf(p.pb)) { cnt(a, MCS_IC_PPERP_CLAMP); p.pperp = 1.0e-6f * p.ptot; }
          else p.pperp = fsq<X>(p.ptot * p.ptot - p.pb * p.pb);
          p.gr = p.pperp * p.gd;
          p.z_lo = edgef(p.i_grid, U); p.z_hi = edgef(p.i_grid + 1, U);
          active = true;
        }
      }
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
    if (active) {
      const int end = f32_pass<X>(a, rng, p, U, k);
      if (end >= 0) {
        const int steps = p.helix > MCS_HELIX_CAP ? MCS_HELIX_CAP : p.helix;
        atomicAdd(&S_steps[0], (unsigned long long)steps); atomicAdd(&S_steps[1], (unsigned long long)p.n_retro);
        atomicAdd(&S_steps[2], (unsigned long long)rng.n);
        if (end != 0) {
          const Cgs c = to_cgs(p, U);
          particle_finish(a, end, c.pb, c.pperp, c.gam, c.phi, c.w, p.ig3);
        }
        cnt(a, MCS_IC_REASON0 + end);
        if (a->f_reason) {
          a->f_reason[k] = end; a->f_helix[k] = p.helix; a->f_retro[k] = p.n_retro; a->f_ptot[k] = (double)p.ptot * U.P0;
          a->f_x[k] = (double)p.x * U.L0;
        }
        active = false;
      }
    }
  }
  __syncthreads();
  block_flush(a);
}

extern "C" __global__ void __launch_bounds__(256) mcs_k_transport_f32_loop(const KArgs* __restrict__ ka) { f32_loop_body<false>(ka); }
// the same loop with the EXACT fp32 primitives (include/mcs_math_f32.h): bit-identical to oracle/mcs_oracle_f32.inc
extern "C" __global__ void __launch_bounds__(256) mcs_k_transport_f32_loop_exact(const KArgs* __restrict__ ka) { f32_loop_body<true>(ka); }

#include "mcs_transport_f32k.inc"

// mcs_transport_ws.inc -- K1 "wave-specialised": the transport kernel in which rare work leaves the wave that runs the passes.
// (included by mcs_transport.hip: same helpers, same arithmetic, same per-particle results as transport_body)
//
// transport_body keeps a particle in ONE lane from load to end, so every event of a particle (a zone crossing in 2.8 % of the
// lane-passes, the full Code Blocks in 0.2 %) is served by the wave that runs the passes: 85 % of the loop headers enter the rare
// region for ~12 of 64 lanes, the full Code Blocks run for 1-9 lanes, 8 of 55 live lanes sit out the rest of a trip
// (profiles/r02_event_profile.txt).  Here a particle is a 29-word record that moves:
//
//   * a wave runs trips of MCS_PASSES_PER_ITER common passes (the same straight-line code); at the loop header every lane whose
//     particle has something pending SWAPS it, through a slot of a block-wide LDS pool, for a particle that is ready to run
//     (ring R -> the lane; the lane's particle -> ring E), so all 64 lanes run the next trip;
//   * when 64 particles are pending in E, the wave that notices swaps ITS 64 particles out (to R) and the pending ones in, and
//     runs the rare code 64 lanes wide: classification, plain crossings and their tallies on the spot (no record stacks), light
//     paths; particles that need the full Code Blocks go on to ring H and are served, again 64 at a time, the same way; serviced
//     particles stay in the serving wave's lanes, which goes back to running passes with them;
//   * fresh particles are claimed by idle lanes when R is empty and the block holds fewer than `ws_pop_max` particles;
//   * after the launch's work counter is exhausted nothing waits for company: idle lanes take whatever is queued and every wave
//     serves the lanes it holds in place.
//
// State and RNG stream position travel with the particle (as in the tail consolidation of transport_body), and nothing of a
// particle changes while it sits in a slot: per-particle results are bit-identical to transport_body and to the oracle.
// Rings are multi-producer / multi-consumer queues of slot ids in LDS (monotonic head / tail, entry = id + 1, 0 = empty).
// Every wait is bounded: a spin that does not end sets W_panic, the block drains out and the host reports the launch as failed.

#define WS_NSLOT 320            // slots of the pool: particles queued in E + H + R (the others are in lanes)
#define WS_RCAP 512             // ring capacity (power of two > WS_NSLOT: an entry is never reused while its id is in flight)
#define WS_NW 29                // words per record
enum { WQ_F = 0, WQ_E = 1, WQ_H = 2, WQ_R = 3 };

__shared__ double W_slot[WS_NW][WS_NSLOT];      // word-major: lanes with consecutive slots touch consecutive addresses
__shared__ unsigned W_ring[4][WS_RCAP];
__shared__ __attribute__((aligned(16))) unsigned long long W_q[4];   // per ring: tail << 32 | head (both monotonic; one word, so that ONE read shows a consistent pair and one CAS claims)
__shared__ unsigned W_pop;       // particles this block owns (claimed, not ended) -- includes claims in progress
__shared__ __attribute__((aligned(8))) unsigned W_ctl[2];      // [0] the launch's work counter is exhausted, [1] a bounded wait ran out (panic code)
#define W_exh W_ctl[0]
#define W_panic W_ctl[1]

namespace {

typedef __attribute__((address_space(3))) unsigned lu32;
typedef __attribute__((address_space(3))) unsigned long long lu64;
__device__ __forceinline__ unsigned lds_ld(unsigned* p) { return __hip_atomic_load((lu32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_st(unsigned* p, unsigned v) { __hip_atomic_store((lu32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ unsigned lds_add(unsigned* p, unsigned v) { return __hip_atomic_fetch_add((lu32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ unsigned lds_sub(unsigned* p, unsigned v) { return __hip_atomic_fetch_sub((lu32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ unsigned long long lds_ld64(unsigned long long* p) { return __hip_atomic_load((lu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ unsigned wq_count(unsigned long long w) { return (unsigned)(w >> 32) - (unsigned)w; }

// the state of the four rings and the two control words, fetched together (one LDS round trip); wave-uniform
struct WsView { unsigned long long q[4]; unsigned exh, panic; };
__device__ __forceinline__ WsView ws_view() {
  WsView v;
  const unsigned long long q0 = lds_ld64(&W_q[0]), q1 = lds_ld64(&W_q[1]), q2 = lds_ld64(&W_q[2]), q3 = lds_ld64(&W_q[3]);
  const unsigned e = lds_ld(&W_ctl[0]), pn = lds_ld(&W_ctl[1]);
  auto u = [](unsigned long long x) -> unsigned long long {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(x >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x);
  };
  v.q[0] = u(q0); v.q[1] = u(q1); v.q[2] = u(q2); v.q[3] = u(q3);
  v.exh = (unsigned)__builtin_amdgcn_readfirstlane((int)e); v.panic = (unsigned)__builtin_amdgcn_readfirstlane((int)pn);
  return v;
}

// Lanes with `pred` push `id`.  The slot's words were written by this wave BEFORE (program order; LDS executes a wave's
// instructions in order), the entry is written last: a consumer that sees the entry sees the words.  The entry of the previous lap
// was consumed long ago: the ring is larger than the number of ids, and a consumer clears an entry right after its claim.
// Two halves, so that the reservation (an atomic with a return value: one LDS round trip) can be issued early and waited for late.
__device__ __forceinline__ unsigned wq_reserve(int q, unsigned long long m) {      // m: ballot of the pushing lanes (may be 0); the leader's lane gets the old tail
  unsigned long long old = 0ull;
  if (m != 0ull && (int)__lane_id() == __ffsll((long long)m) - 1)
    old = __hip_atomic_fetch_add((lu64*)&W_q[q], (unsigned long long)__popcll(m) << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return (unsigned)(old >> 32);
}
__device__ __forceinline__ void wq_commit(int q, unsigned long long m, unsigned res, bool pred, unsigned id) {
  if (m == 0ull) return;
  const unsigned base = (unsigned)__builtin_amdgcn_readlane((int)res, __ffsll((long long)m) - 1);
  if (pred) {
    asm volatile("" ::: "memory");
    lds_st(&W_ring[q][(base + below(m)) & (WS_RCAP - 1)], id + 1u);
  }
}
__device__ __forceinline__ void wq_push(int q, bool pred, unsigned id) {
  const unsigned long long m = __builtin_amdgcn_ballot_w64(pred);
  if (m == 0ull) return;
  wq_commit(q, m, wq_reserve(q, m), pred, id);
}
// Claim up to `want` entries (none when fewer than `min_take` are there).  `seen`: a recent value of the ring's word (ws_view) --
// when it is still current the claim is ONE compare-and-swap.  Returns the number claimed (wave-uniform); the claimed entries
// are positions h_out .. h_out + n - 1, to be read with wq_take.  Called by all lanes of the wave.
__device__ __forceinline__ unsigned wq_pop(int q, unsigned want, unsigned min_take, unsigned long long seen, unsigned& h_out) {
  unsigned take = 0, h = 0;
  if (__lane_id() == 0u) {
    unsigned long long w = seen;
    for (int tries = 0; tries < 1024; ++tries) {
      const unsigned avail = wq_count(w);
      take = avail < want ? avail : want;
      if (take < min_take || take == 0u) { take = 0u; break; }
      h = (unsigned)w;
      // head + take does not carry into the tail half: positions wrap at 2^32 only after 4e9 claims of one launch
      if (__hip_atomic_compare_exchange_strong((lu64*)&W_q[q], &w, w + take, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
      take = 0u;      // w now holds the current word: try again
    }
  }
  h_out = (unsigned)__builtin_amdgcn_readfirstlane((int)h);
  return (unsigned)__builtin_amdgcn_readfirstlane((int)take);
}
__device__ __forceinline__ unsigned wq_take(int q, unsigned pos) {
  unsigned* e = &W_ring[q][pos & (WS_RCAP - 1)];
  unsigned v;
  int spins = 0;
  while ((v = lds_ld(e)) == 0u) { if (++spins > (1 << 20)) { lds_st(&W_panic, 0x200u | (unsigned)q); v = 1u; break; } }   // (the producer is between its claim and its write)
  lds_st(e, 0u);
  asm volatile("" ::: "memory");
  return v - 1u;
}

// ---- the record: everything of a lane's particle that is not a pure function of the rest.  Not stored: the cached zone properties
// and edges (read back from the tables by ig3 / i_grid), t_ev / ovr_inc (refresh_time), the thresholds of the common pass
// (refresh_thr).  `t_clock`: the time step the clock of the particle's next pass uses (the one of its last move).
struct WsRec { double w[WS_NW]; };
__device__ __forceinline__ void ws_pack(WsRec& r, const Pt& p, const Rng& rng, long long k, int evw, double phi_prev, double t_clock) {
  r.w[0] = p.weight; r.w[1] = p.ptot_pf; r.w[2] = p.pb_pf; r.w[3] = p.p_perp; r.w[4] = p.gam_pf; r.w[5] = p.x; r.w[6] = p.x_old;
  r.w[7] = p.phi; r.w[8] = p.prp; r.w[9] = p.acctime; r.w[10] = p.xn_per; r.w[11] = p.dphi; r.w[12] = p.gyro_denom; r.w[13] = p.gyro_rad;
  r.w[14] = p.gyro_rad_tot; r.w[15] = p.gyro_period; r.w[16] = p.t_step; r.w[17] = p.rp_val; r.w[18] = p.cm_val; r.w[19] = p.rg_val;
  r.w[20] = p.x_dt; r.w[21] = phi_prev; r.w[22] = t_clock;
  r.w[23] = __longlong_as_double(k);
  const int gridpack = p.i_grid | (p.i_grid_old << 8) | (p.ig3 << 16) | (p.tcut << 24);
  const int bits = ((int)p.downstream << 1) | ((int)p.inj << 2) | ((evw & 15) << 3);
  r.w[24] = __hiloint2double(p.flags, (int)p.n_ovr);
  r.w[25] = __hiloint2double(gridpack, p.helix);
  r.w[26] = __hiloint2double(p.n_retro, bits);
  r.w[27] = __hiloint2double((int)rng.k0, (int)rng.k1);
  r.w[28] = __hiloint2double((int)rng.n, 0);
}
__device__ __forceinline__ void ws_unpack(CK* a, const Hot& h, const WsRec& r, Pt& p, Rng& rng, long long& k, int& evw, double& phi_prev, double& t_clock) {
  p.weight = r.w[0]; p.ptot_pf = r.w[1]; p.pb_pf = r.w[2]; p.p_perp = r.w[3]; p.gam_pf = r.w[4]; p.x = r.w[5]; p.x_old = r.w[6];
  p.phi = r.w[7]; p.prp = r.w[8]; p.acctime = r.w[9]; p.xn_per = r.w[10]; p.dphi = r.w[11]; p.gyro_denom = r.w[12]; p.gyro_rad = r.w[13];
  p.gyro_rad_tot = r.w[14]; p.gyro_period = r.w[15]; p.t_step = r.w[16]; p.rp_val = r.w[17]; p.cm_val = r.w[18]; p.rg_val = r.w[19];
  p.x_dt = r.w[20]; phi_prev = r.w[21]; t_clock = r.w[22];
  k = __double_as_longlong(r.w[23]);
  p.flags = __double2hiint(r.w[24]); p.n_ovr = (unsigned)__double2loint(r.w[24]);
  const int gridpack = __double2hiint(r.w[25]);
  p.helix = __double2loint(r.w[25]);
  p.i_grid = gridpack & 0xff; p.i_grid_old = (gridpack >> 8) & 0xff; p.ig3 = (gridpack >> 16) & 0xff; p.tcut = (gridpack >> 24) & 0xff;
  p.n_retro = __double2hiint(r.w[26]);
  const int bits = __double2loint(r.w[26]);
  p.downstream = (bits >> 1) & 1; p.inj = (bits >> 2) & 1; evw = (bits >> 3) & 15;
  rng.k0 = (uint32_t)__double2hiint(r.w[27]); rng.k1 = (uint32_t)__double2loint(r.w[27]);
  rng.n = (uint32_t)__double2hiint(r.w[28]);
  p.npush = 0;
  // the cached zone properties and edges and the next time cut, in ONE round of LDS reads
  {
    const int z = p.ig3, g = p.i_grid;
    const int tcx = p.tcut >= 1 && p.tcut <= MCS_NA_C ? p.tcut - 1 : 0;
    double v0 = S_gsf[z], v1 = S_bcos[z], v2 = S_ux[z], v3 = S_gef[z], v4 = S_x[g], v5 = S_x[g + 1], v6 = S_tc[tcx];
    asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6));
    p.z_gsf = v0; p.z_bcos = v1; p.z_ux = v2; p.z_gef = v3; p.z_lo = v4; p.z_hi = v5;
    // refresh_time with the value already read
    double t = (h.do_tcuts && p.tcut <= h.n_tcuts) ? v6 : __builtin_inf();
    if (h.age_max > 0 && h.age_max < t) t = h.age_max;
    p.t_ev = t;
    p.ovr_inc = (h.do_tcuts && p.downstream && p.tcut > h.n_tcuts) ? 1 : 0;
  }
  (void)a;
}
// the lane's particle goes into slot s; with TAKE the particle that was there comes into the lane (word by word: a read and a
// write of the same address, executed in order)
template <bool GIVE, bool TAKE>
__device__ __forceinline__ void ws_move(CK* a, const Hot& h, unsigned s, Pt& p, Rng& rng, long long& k, int& evw, double& phi_prev, double& t_clock) {
  WsRec r;
  if (GIVE) ws_pack(r, p, rng, k, evw, phi_prev, t_clock);
#pragma unroll
  for (int j = 0; j < WS_NW; ++j) {
    double t = 0.0;
    if (TAKE) t = W_slot[j][s];
    if (GIVE) W_slot[j][s] = r.w[j];
    r.w[j] = t;
  }
  if (TAKE) ws_unpack(a, h, r, p, rng, k, evw, phi_prev, t_clock);
}

}  // namespace

#ifdef MCS_PROF
#define WPROF_ADD(slot, v) do { const unsigned long long v__ = (unsigned long long)(v); if ((threadIdx.x & 63u) == 0u) atomicAdd(&S_prof[slot], v__); } while (0)
#else
#define WPROF_ADD(slot, v) do { } while (0)
#endif
#if defined(MCS_PROF) && defined(MCS_WS_TIMERS)      // s_memtime around the phases of a trip (intrusive: ratios)
#define WT_NOW() __builtin_amdgcn_s_memtime()
#define WT_ADD(slot, t0) do { const unsigned long long t1__ = __builtin_amdgcn_s_memtime(); WPROF_ADD(slot, t1__ - (t0)); } while (0)
#else
#define WT_NOW() 0ull
#define WT_ADD(slot, t0) do { } while (0)
#endif

// PLAIN / PLAIN_ETF as in transport_body (the host checks the conditions).
template <bool PLAIN_ETF>
__device__ __forceinline__ void transport_ws(const KArgs* __restrict__ ka) {
  constexpr bool LOSSY = false;
  CK* a = (CK*)ka;
  if (a->n_dev && *a->n_dev == 0) return;
  const int ne = a->P.n_grid + 2, ng = a->P.n_grid, ntc = a->tb.n_tcuts;
  block_prologue(a);
  for (int i = threadIdx.x; i < 4 * WS_RCAP; i += blockDim.x) (&W_ring[0][0])[i] = 0u;
  if (threadIdx.x < 4) W_q[threadIdx.x] = threadIdx.x == WQ_F ? ((unsigned long long)WS_NSLOT << 32) : 0ull;
  if (threadIdx.x == 0) { W_pop = 0u; W_exh = 0u; W_panic = 0u; }
  __syncthreads();
  for (int i = threadIdx.x; i < WS_NSLOT; i += blockDim.x) W_ring[WQ_F][i] = (unsigned)i + 1u;      // every slot is free
  __syncthreads();

  Hot h;
  h.m = vconst(a->m); h.x_grid_stop = vconst(a->P.x_grid_stop); h.xn_coarse = vconst(a->P.xn_per_coarse);
  h.u2 = sconst(a->P.u2); h.eta = sconst(a->P.eta_mfp); h.zzq = sconst(a->zzq); h.mc = sconst(a->mc);
  h.feb_down = sconst(a->P.feb_downstream); h.pcut = sconst(a->pcut); h.pmax_cutoff = sconst(a->pmax_cutoff);
  h.feb_up = sconst(a->P.feb_upstream); h.age_max = sconst(a->P.age_max); h.inj_frac = sconst(a->inj_frac);
  h.xn_fine = sconst(a->P.xn_per_fine); h.aa = sconst(a->aa);
  h.n_grid = sconsti(ng); h.i_grid_feb = sconsti(a->P.i_grid_feb); h.n_tcuts = sconsti(ntc); h.n_xspec = sconsti(a->tb.n_xspec);
  h.rad_losses = a->P.do_rad_losses != 0; h.do_tcuts = a->P.do_tcuts != 0;
  h.etf = PLAIN_ETF ? (a->P.energy_transfer_frac > 0) : false;
  h.custom_epsB = false; h.dont_scatter = false; h.dont_DSA = false; h.oblique = false; h.every_pass = false; h.odd_cfg = false;
  (void)ne;

  mcsm::HotCoef kc;
  hot_coef_init(kc);

  Pt p;
  Rng rng;
  p.weight = 0; p.ptot_pf = 1; p.pb_pf = 0; p.p_perp = 1; p.gam_pf = 1; p.x = 0; p.x_old = 0; p.phi = 0; p.prp = 0; p.acctime = 0;
  p.xn_per = 1; p.dphi = 0; p.gyro_denom = 0; p.gyro_rad = 0; p.gyro_rad_tot = 0; p.gyro_period = 0; p.t_step = 0;
  p.rp_val = 1; p.cm_val = 1; p.rg_val = 1; p.x_dt = 0; p.t_ev = 0; p.flags = 0; p.ovr_inc = 0; p.n_ovr = 0u;
  p.z_gsf = 1; p.z_bcos = 1; p.z_ux = 0; p.z_gef = 1; p.z_lo = 0; p.z_hi = 0; p.t_hi = 0; p.t_lo = 0; p.c_gef = 0; p.c_tev = 0;
  p.i_grid = 0; p.i_grid_old = 0; p.ig3 = 0; p.helix = 0; p.tcut = 1; p.n_retro = 0; p.downstream = false; p.inj = false; p.npush = 0;
  rng.init(0ull);
  int act = 0;                    // -1 while the lane holds a particle
  // bit 0 "ev" the last move needs slow_post, bit 1 a position threshold was reached, bit 2 the particle has moved since it was
  // loaded, bit 3 "go": serviced (or fresh from R) and not run since -- the lane runs the next pass whatever its flags say
  int evw = 0;
  double phi_prev = 0.0, t_clock = 0.0;
  long long k = -1;
  const unsigned lane = __lane_id();
  const unsigned long long n = (unsigned long long)(a->n_dev ? *a->n_dev : a->n);
  const unsigned pop_max = (unsigned)__builtin_amdgcn_readfirstlane(a->ws_pop_max);
  const unsigned serve_min = (unsigned)__builtin_amdgcn_readfirstlane(a->ws_serve_min);     // entries of E / H at which a wave serves them (64)
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
  unsigned tick = 0;
  bool done = false;
  bool w_exh = false;             // wave-uniform: this wave has seen the launch's work counter exhausted (W_exh) at a housekeeping
  const unsigned tail_loop_L = (unsigned)__builtin_amdgcn_readfirstlane(a->tail_loop);      // (KArgs::tail_loop)
  while (!done) {
    ++tick;
    bool need = (act != 0) & ((evw & 8) == 0) & (((evw & 3) | p.flags) != 0);
    {
      const unsigned long long m_need0 = __builtin_amdgcn_ballot_w64(need), m_act0 = __builtin_amdgcn_ballot_w64(act != 0);
      WPROF_ADD(0, 1); WPROF_ADD(8, __popcll(m_act0)); WPROF_ADD(13, __popcll(m_need0));
      if (MCS_UNLIKELY((m_need0 != 0ull) | (m_act0 != ~0ull))) {
        // =========================== housekeeping: particles change lanes ===========================
        [[maybe_unused]] const unsigned long long wt_hk = WT_NOW();
        const WsView V = ws_view();      // the rings and the control words as of now: one LDS round trip
        const bool exh = V.exh != 0u;
        w_exh = exh;
        bool svc_defer = false;       // the service below may send particles that need the full Code Blocks on to H
        // ---- (1) ready particles: into idle lanes; in exchange for a lane's pending particle (not once the queue is exhausted:
        //          every wave then serves the lanes it holds)
        {
          const unsigned long long m_x = exh ? ~m_act0 : (m_need0 | ~m_act0);
          const unsigned nx = (unsigned)__popcll(m_x);
          if (nx != 0u && wq_count(V.q[WQ_R]) != 0u) {
            unsigned h0;
            const unsigned got = wq_pop(WQ_R, nx, 1u, V.q[WQ_R], h0);
            if (got) {
              const unsigned r = below(m_x);
              const bool has = ((m_x >> lane) & 1ull) != 0ull && r < got;
              const bool gave = has & need;
              const unsigned long long m_gave = __builtin_amdgcn_ballot_w64(gave), m_free = __builtin_amdgcn_ballot_w64(has & !gave);
              const unsigned resE = wq_reserve(WQ_E, m_gave), resF = wq_reserve(WQ_F, m_free);     // (issued now, waited for after the swap)
              unsigned s = 0u;
              if (has) {
                s = wq_take(WQ_R, h0 + r);
                if (need) ws_move<true, true>(a, h, s, p, rng, k, evw, phi_prev, t_clock);
                else ws_move<false, true>(a, h, s, p, rng, k, evw, phi_prev, t_clock);
                refresh_thr<LOSSY>(h, p);
                act = -1; need = false;
              }
              wq_commit(WQ_E, m_gave, resE, gave, s);
              wq_commit(WQ_F, m_free, resF, has & !gave, s);
              WPROF_ADD(40, got);
            }
          }
        }
        // ---- (2) fresh particles into the lanes that are still idle
        if (!exh) {
          const unsigned long long m_i = ~__builtin_amdgcn_ballot_w64(act != 0);
          const unsigned ni = (unsigned)__popcll(m_i);
          if (ni) {
            unsigned c = 0u;
            unsigned long long base = 0ull;
            if (lane == 0u) {
              const unsigned pop = lds_add(&W_pop, ni);      // reserve first: W_pop == 0 then means that nothing is in flight
              c = pop >= pop_max ? 0u : (ni < pop_max - pop ? ni : pop_max - pop);
              if (c) {
                base = atomicAdd(a->work_counter, (unsigned long long)c);
                if (base >= n) { c = 0u; lds_st(&W_exh, 1u); }
                else if (base + c >= n) { c = (unsigned)(n - base); lds_st(&W_exh, 1u); }
              }
              if (c < ni) lds_sub(&W_pop, ni - c);
            }
            c = (unsigned)__builtin_amdgcn_readfirstlane((int)c);
            if (c) {
              const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)base), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(base >> 32));
              const unsigned long long b = ((unsigned long long)hi << 32) | lo;
              const unsigned r = below(m_i);
              if (act == 0 && r < c) {
                k = (long long)(b + r);
                load_particle(a, h, k, p, rng);
                act = -1; evw = 0; phi_prev = 0.0; t_clock = 0.0; need = true;
                __builtin_amdgcn_s_waitcnt(0x0F70);
              }
              WPROF_ADD(41, c);
            }
          }
        }
        // ---- (3) what this wave serves now
        const unsigned long long m_need1 = __builtin_amdgcn_ballot_w64(need);
        const unsigned nn = (unsigned)__popcll(m_need1);
        int q = -1;                    // ring to fill the wave from
        bool fill_swap = false;        // running lanes swap their particles out (to R) for queued ones
        // (the view is a few hundred cycles old: what it shows as pending is still there unless another wave has claimed it -- the
        // claim below decides; particles pushed since are seen at the next header)
        unsigned eh = wq_count(V.q[WQ_H]), ee = wq_count(V.q[WQ_E]);
        if (!exh) {
          if (nn >= 32u) {
            // half a wave of pending particles (fresh ones at the start of a launch): served in place, nothing moves
          } else {
            // the pending particles of this wave go to E (through free slots: R had nothing to swap them for)
            if (nn) {
              unsigned h0;
              const unsigned got = wq_pop(WQ_F, nn, 1u, V.q[WQ_F], h0);
              const unsigned r = below(m_need1);
              const bool has = need && r < got;
              const unsigned long long m_has = __builtin_amdgcn_ballot_w64(has);
              const unsigned resE = wq_reserve(WQ_E, m_has);
              unsigned s = 0u;
              if (has) {
                s = wq_take(WQ_F, h0 + r);
                ws_move<true, false>(a, h, s, p, rng, k, evw, phi_prev, t_clock);
                act = 0; p.flags = 0; p.helix = 0; evw = 0; need = false;
              }
              wq_commit(WQ_E, m_has, resE, has, s);
              ee += got;
            }
            const unsigned n_idle = 64u - (unsigned)__popcll(__builtin_amdgcn_ballot_w64(act != 0));
            if (eh >= serve_min) { q = WQ_H; fill_swap = true; }
            else if (ee >= serve_min) { q = WQ_E; fill_swap = true; svc_defer = true; }
            else if (n_idle >= 32u && (eh | ee) != 0u) { q = eh >= ee ? WQ_H : WQ_E; }      // starving: whatever is there, into the idle lanes
          }
        } else {
          // the queue is exhausted: idle lanes take whatever is pending, everything is served where it is
          if ((eh | ee) != 0u) q = ee >= eh ? WQ_E : WQ_H;
        }
        if (q >= 0) {
          const unsigned long long m_idle = ~__builtin_amdgcn_ballot_w64(act != 0);
          const unsigned long long m_run = fill_swap ? (__builtin_amdgcn_ballot_w64(act != 0) & ~__builtin_amdgcn_ballot_w64(need)) : 0ull;
          const unsigned n_idle = (unsigned)__popcll(m_idle);
          const unsigned want = n_idle + (unsigned)__popcll(m_run);
          if (want) {
            unsigned h0;
            const unsigned got = wq_pop(q, want, fill_swap ? (serve_min < want ? serve_min : want) : 1u, V.q[q], h0);
            if (got) {
              const bool idle = act == 0;
              const unsigned r = idle ? below(m_idle) : n_idle + below(m_run);     // idle lanes first
              const bool mine = idle | (((m_run >> lane) & 1ull) != 0ull);
              const bool has = mine && r < got;
              const bool gave = has & !idle;
              const unsigned long long m_gave = __builtin_amdgcn_ballot_w64(gave), m_free = __builtin_amdgcn_ballot_w64(has & !gave);
              const unsigned resR = wq_reserve(WQ_R, m_gave), resF = wq_reserve(WQ_F, m_free);
              unsigned s = 0u;
              if (has) {
                s = wq_take(q, h0 + r);
                if (idle) ws_move<false, true>(a, h, s, p, rng, k, evw, phi_prev, t_clock);
                else ws_move<true, true>(a, h, s, p, rng, k, evw, phi_prev, t_clock);
                act = -1; need = true;
              }
              wq_commit(WQ_R, m_gave, resR, gave, s);
              wq_commit(WQ_F, m_free, resF, has & !gave, s);
              WPROF_ADD(q == WQ_H ? 43 : 42, 1); WPROF_ADD(q == WQ_H ? 45 : 44, got);
            } else {
              svc_defer = false;
            }
          }
        }
        // =========================== service: the pending lanes of this wave ===========================
        const bool svc = need;
        WT_ADD(50, wt_hk);
        [[maybe_unused]] const unsigned long long wt_sv = WT_NOW();
        [[maybe_unused]] const int wt_kind = (q == WQ_E && fill_swap) ? 51 : ((q == WQ_H && fill_swap) ? 52 : 53);
        if (__builtin_amdgcn_ballot_w64(svc) != 0ull) {
          WPROF_ADD(12, 1); WPROF_ADD(46, __popcll(__builtin_amdgcn_ballot_w64(svc)));
          int end = -1;
          bool to_heavy = false;
          if (svc) {
            const bool moved = (evw & 4) != 0, thr = (evw & 2) != 0;
            bool ev = (evw & 1) != 0, ev_x = false;
            bool up_due = false, xn_due = false, feb_due = false;
            double t_clk = p.t_step;      // the clock of a pass uses the time step of the PREVIOUS move
            if (__builtin_amdgcn_ballot_w64(thr) != 0ull) {
              const bool fwd = p.x > p.x_old;
              const bool same_zone = (fwd & (p.z_hi > p.x)) | (!fwd & (p.z_lo <= p.x));
              const bool ev_up = ((p.x >= h.x_grid_stop) & ((p.x_old < h.x_grid_stop) | ((p.x_old < p.prp) & (p.x >= p.prp)))) | (p.x > p.x_dt);
              const bool ev_xn = (p.x > p.gyro_rad_tot) != (p.xn_per == h.xn_coarse);
              ev_x = thr & !same_zone;
              up_due = thr & ev_up; xn_due = thr & ev_xn;
              feb_due = thr & (p.i_grid <= h.i_grid_feb) & p.inj & (p.x < h.feb_up);
              ev = ev | up_due | xn_due | feb_due;
            }
            const bool post_pending = moved && (ev || ev_x || (p.flags & F_INJCHK) != 0);
            bool t_due = false, age_out = false;
            if (__builtin_amdgcn_ballot_w64(ev) != 0ull) {
              t_due = ev & p.downstream & (p.acctime >= p.t_ev);
              age_out = (h.age_max > 0) & (p.acctime > h.age_max);
            }
            const bool etf_due = h.etf & ev_x & !(p.inj | (p.downstream & (p.x < 0))) & (p.x_old <= 0);
            bool full = (p.flags & ~F_CM) != 0 || p.helix >= MCS_HELIX_CAP || etf_due || (ev && (up_due || age_out || feb_due));
            if (!full && ev_x) full = !plain_crossing<true>(a, h, p, 0u);
            if (svc_defer) {
              // the full Code Blocks are run 64 lanes wide too: such a particle goes on to H (nothing of it has been touched)
              to_heavy = full & ((p.flags & F_NOPARK) == 0);
              full = full & !to_heavy;
            }
            if (__builtin_amdgcn_ballot_w64(full || (!to_heavy && ((p.flags & F_CM) != 0 || t_due || xn_due))) != 0ull) {
              if (!full && !to_heavy) {
                if (p.flags & F_CM) {
                  refresh_scatter(a, p, h.aa, h.aa * MP_ * CC_, h.eta);
                  p.flags = 0;
                }
                if (t_due) {      // slow_post's time cut (cuts.jl:149-162)
                  if (h.do_tcuts && !(p.tcut > h.n_tcuts) && p.acctime >= tcut_next_of(a, h, p.tcut)) {
                    tcut_track(a, p.tcut, p.weight, p.ptot_pf);
                    p.tcut += 1;
                  }
                  refresh_time(a, h, p);
                }
                if (xn_due) {     // slow_pre's fine / coarse step (particle_loop.jl:382-385)
                  p.xn_per = p.x > p.gyro_rad_tot ? h.xn_coarse : h.xn_fine;
                  p.flags |= F_CM;
                  refresh_move(a, h, p);
                }
              }
              if (full) {
                bool pend = post_pending;
                for (;;) {
                  if (pend) { end = slow_post<true>(a, h, rng, p, phi_prev); if (end >= 0) break; }
                  if (!(p.flags & F_B1)) break;
                  pend = block1_step(a, h, p, phi_prev, end);
                  if (end >= 0) break;
                  pend = pend || p.i_grid <= h.i_grid_feb;
                  t_clk = p.t_step;
                }
                if (end < 0) end = slow_pre(a, h, kc, rng, p, t_clk, false);
              }
              if (end >= 0) {
                const int steps = p.helix > MCS_HELIX_CAP ? MCS_HELIX_CAP : p.helix;
                atomicAdd(&S_steps[0], (unsigned long long)steps); atomicAdd(&S_steps[1], (unsigned long long)p.n_retro);
                atomicAdd(&S_steps[2], (unsigned long long)rng.n);
                if (p.n_ovr) cnt(a, MCS_IC_TCUT_OVERRUN, p.n_ovr);
                if (end == 0) {
                  a->l_save[k] = 1;
                  a->sv.weight[k] = p.weight; a->sv.ptot_pf[k] = p.ptot_pf; a->sv.pb_pf[k] = p.pb_pf; a->sv.x_PT_cm[k] = p.x;
                  a->sv.xn_per[k] = p.xn_per;
                  a->sv.prp_x_cm[k] = p.x < p.prp ? p.prp : p.x * 1.1;   // quirk Q7
                  a->sv.acctime_sec[k] = p.acctime; a->sv.phi_rad[k] = p.phi;
                  a->sv.meta[k] = mcs_pack_meta(p.i_grid, p.tcut, p.downstream, p.inj);
                  cnt(a, MCS_IC_COUNT);
                } else {
                  a->l_save[k] = 2;
                }
                cnt(a, MCS_IC_REASON0 + end);
                if (a->f_reason) {
                  a->f_reason[k] = end; a->f_helix[k] = p.helix; a->f_retro[k] = p.n_retro; a->f_ptot[k] = p.ptot_pf; a->f_x[k] = p.x;
                }
              }
            }
            if (to_heavy) p.flags |= F_NOPARK;        // (it has waited for company once: the next service runs it)
            else if (end < 0) { refresh_thr<LOSSY>(h, p); t_clock = t_clk; evw |= 8; }
          }
          // ---- particle_finish! of the particles that ended (a population of replicas of one saved particle hits ONE bin of the
          // escape spectrum a million times: when every tally of the wave goes to the same bin the wave adds them up first)
          const unsigned long long m_end = __builtin_amdgcn_ballot_w64(end >= 0);
          if (m_end != 0ull) {
            long long foff = -1; double fval = 0.0;
            if (end >= 1) particle_finish(a, end, p.pb_pf, p.p_perp, p.gam_pf, p.phi, p.weight, p.ig3, &foff, &fval);
            const unsigned long long vm = __builtin_amdgcn_ballot_w64(foff >= 0);
            if (vm != 0ull) {
              const int first = __ffsll((long long)vm) - 1;
              const long long off0 = __shfl(foff, first);
              if (__builtin_amdgcn_ballot_w64(foff >= 0 && foff != off0) == 0ull) {
                double sum = foff >= 0 ? fval : 0.0;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
                if ((int)lane == first) tadd(a, off0, sum);
              } else if (foff >= 0) {
                tadd(a, foff, fval);
              }
            }
            if (end >= 0) { act = 0; p.flags = 0; p.helix = 0; evw = 0; }
            if (lane == 0u) lds_sub(&W_pop, (unsigned)__popcll(m_end));
            WPROF_ADD(10, __popcll(m_end));
          }
          // ---- particles for the full Code Blocks go on to H; without a free slot they stay and are run at the next header
          const unsigned long long m_h = __builtin_amdgcn_ballot_w64(to_heavy);
          if (m_h != 0ull) {
            unsigned h0;
            const unsigned got = wq_pop(WQ_F, (unsigned)__popcll(m_h), 1u, V.q[WQ_F], h0);
            const unsigned r = below(m_h);
            const bool has = to_heavy && r < got;
            const unsigned long long m_has = __builtin_amdgcn_ballot_w64(has);
            const unsigned resH = wq_reserve(WQ_H, m_has);
            unsigned s = 0u;
            if (has) {
              s = wq_take(WQ_F, h0 + r);
              ws_move<true, false>(a, h, s, p, rng, k, evw, phi_prev, t_clock);
              act = 0; p.flags = 0; p.helix = 0; evw = 0;
            }
            wq_commit(WQ_H, m_has, resH, has, s);
            WPROF_ADD(47, got);
          }
        }
        WT_ADD(wt_kind, wt_sv); WPROF_ADD(wt_kind + 4, 1);
        // ---- the end of the launch for this wave: nothing in its lanes, nothing left in the block
        const unsigned long long m_act2 = __builtin_amdgcn_ballot_w64(act != 0);
        if (m_act2 == 0ull) {
          const bool ex2 = __builtin_amdgcn_readfirstlane((int)lds_ld(&W_exh)) != 0;
          const unsigned pop2 = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_ld(&W_pop));
          done = ex2 & (pop2 == 0u);
          if (!done) {
            __builtin_amdgcn_s_sleep(16);
            if ((tick & 255u) == 0u && __builtin_amdgcn_s_memrealtime() - t_start > 3000000000ull) lds_st(&W_panic, 0x300u);      // 30 s
          }
        }
        if (V.panic != 0u) done = true;
      }
    }
    // ---- MCS_PASSES_PER_ITER common passes (as transport_body)
    [[maybe_unused]] const unsigned long long wt_ps = WT_NOW();
    bool run = (act != 0) & (((evw & 8) != 0) | (((evw & 3) | p.flags) == 0));
    const bool may_go_on = p.flags == 0;
    bool stopped = false;
    double t_clk_pass = ((evw & 8) != 0) ? t_clock : p.t_step;
    // ---- tail loop (as in transport_body; KArgs::tail_loop): once the launch's queue is dry, a wave that holds a handful of particles, all
    // of them ready to run, makes its passes in a loop of their own -- the pass as it stands here (this kernel has no tail ring), every
    // lane computing (idle lanes on the valid state they were initialised with or their last particle left), one exit test -- until a live
    // lane has an event or a flag; the housekeeping above then serves it in place, as always after exhaustion.
    bool tail_fast = false;
    unsigned long long am_t = 0ull;
    if (MCS_UNLIKELY(w_exh)) {
      am_t = __builtin_amdgcn_ballot_w64(act != 0);
      tail_fast = ((unsigned)__popcll(am_t) <= tail_loop_L) & (am_t != 0ull) & (__builtin_amdgcn_ballot_w64((act != 0) & !run) == 0ull);
    }
    if (MCS_UNLIKELY(tail_fast)) {
      const unsigned long long m_halt = __builtin_amdgcn_ballot_w64(!may_go_on);      // (flags do not change in a pass)
#pragma nounroll
      for (;;) {
        p.helix += 1;
        {
          double cos_d, sin_d, c_ps, ssd;
          const uint32_t jd = rng.n;
          rng.n = jd + 2u;
          double U1, s_ps;
          scatter_draws(rng.k0, rng.k1, jd >> 1, kc, U1, s_ps, c_ps);
          scatter_cone(U1, s_ps, 1 - p.cm_val, cos_d, sin_d, ssd);
          scattering_rest(p, kc, cos_d, sin_d, c_ps, ssd);
        }
        p.acctime = p.acctime + t_clk_pass * p.c_gef;
        p.n_ovr += (unsigned)p.ovr_inc;
        const bool ev_time = p.acctime >= p.c_tev;
        bool x1;
        const bool e1 = move_and_detect_thr(a, h, p, phi_prev, x1, true) | ev_time | (p.helix >= MCS_HELIX_CAP);
        evw = (e1 ? 5 : 4) | (x1 ? 2 : 0);
        t_clk_pass = p.t_step;
        if (((__builtin_amdgcn_ballot_w64(e1 | x1) | m_halt) & am_t) != 0ull) break;
      }
    } else
#pragma unroll
    for (int rep = 0; rep < MCS_PASSES_PER_ITER; ++rep) {
      if (rep > 0) {
        run = run & may_go_on & !stopped;
        t_clk_pass = p.t_step;
      }
      stopped = false;
      WPROF_ADD(7, 1); WPROF_ADD(9, __popcll(__builtin_amdgcn_ballot_w64(run)));
      if (run) {
        p.helix += 1;
        {
          double cos_d, sin_d, c_ps, ssd;
          const uint32_t jd = rng.n;
          rng.n = jd + 2u;
          double U1, s_ps;
          scatter_draws(rng.k0, rng.k1, jd >> 1, kc, U1, s_ps, c_ps);
          scatter_cone(U1, s_ps, 1 - p.cm_val, cos_d, sin_d, ssd);
          scattering_rest(p, kc, cos_d, sin_d, c_ps, ssd);
        }
        {
          p.acctime = p.acctime + t_clk_pass * p.c_gef;
          p.n_ovr += (unsigned)p.ovr_inc;
          const bool ev_time = p.acctime >= p.c_tev;
          bool x1;
          const bool e1 = move_and_detect_thr(a, h, p, phi_prev, x1, true) | ev_time | (p.helix >= MCS_HELIX_CAP);
          evw = (e1 ? 5 : 4) | (x1 ? 2 : 0);
          stopped = e1 | x1;
        }
      }
    }
    WT_ADD(54, wt_ps);
  }
  __syncthreads();
#ifdef MCS_PROF
  if (threadIdx.x < MCS_NPROF && S_prof[threadIdx.x]) atomicAdd(&g_prof[threadIdx.x], S_prof[threadIdx.x]);
#endif
  block_flush(a);
  if (threadIdx.x == 0 && W_panic)      // the host fails the launch; the word says which wait it was and what the block held
    atomicAdd(a->strag_count, 1ull | ((unsigned long long)W_panic << 8) | ((unsigned long long)W_pop << 20) |
                              ((unsigned long long)(wq_count(W_q[WQ_E]) & 0x3ffu) << 32) | ((unsigned long long)(wq_count(W_q[WQ_H]) & 0x3ffu) << 42) |
                              ((unsigned long long)(wq_count(W_q[WQ_R]) & 0x3ffu) << 52));
}

#ifndef MCS_WS_WAVES
#define MCS_WS_WAVES 2      // waves per SIMD (2: 512-thread blocks, 256 VGPRs; 3: 768 threads, 168 VGPRs)
#endif
extern "C" __global__ void __launch_bounds__(256 * MCS_WS_WAVES, MCS_WS_WAVES) mcs_k_transport_ws(const KArgs* __restrict__ ka) {
  transport_ws<false>(ka);
}
extern "C" __global__ void __launch_bounds__(256 * MCS_WS_WAVES, MCS_WS_WAVES) mcs_k_transport_ws_etf(const KArgs* __restrict__ ka) {
  transport_ws<true>(ka);
}
extern "C" int mcs_transport_ws_threads(void) { return 256 * MCS_WS_WAVES; }

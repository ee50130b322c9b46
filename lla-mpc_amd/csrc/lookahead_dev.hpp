// lookahead_dev.hpp — the plan launch's look-ahead block: the shared inputs staged in LDS
// (or the per-model raceline reference walked), every (model, candidate) of the block rolled
// out, the per-model argmin and the block's partial published (la_publish).  Included by
// plan_dev.hpp only; the controller and the NLP solve have look-ahead bodies of their own.
#pragma once
#include "dev_stamps.hpp"
#include "dev_wave.hpp"
#include "raceline.hpp"
#include "rollout_dev.hpp"

namespace llampc {

// ------------------------------------------------------------------------------------
// Look-ahead body.  Lane layout inside a block: sub = lane % LPM (LPM = 2: the lane pair
// of one rollout, front/rear chain), cl = lane / LPM; G candidate-lanes per model (power of two); a model's
// candidates c = g + j*G, j < cpl, run sequentially in its G*LPM lanes.
//   LDS from kScratchBytes: xref as [k][2]; U as [k][c][kStageW] (RK4: F0, F1, h/m sin,
//   h/m cos, h lf/Iz cos, delta; else pwm, delta, sin, cos; then
//   input-rate cost term, feasibility) when staged.
// ------------------------------------------------------------------------------------
// The block's partial of the look-ahead argmin over (model, candidate) in flattened order
// (goff+n)*C + c — (v, key) per lane (kNoIndex: none) and the lanes' non-finite counts:
// branch-free wave picks, one LDS exchange, thread 0 publishes (tagged words or plain).
template <int NW = kWaves>
__device__ __forceinline__ void la_publish(const LookaheadLaunch& a, int blk, const Scratch& sc, int par,
                                           double v, int64_t key, int nf) {
  // NW = 8 (the work-queue block) uses both halves of sv / si (par = 0 there) and sn[4..8)
  static_assert(NW == kWaves || NW == 8, "4- or 8-wave blocks");
  wave_pick_nl64(v, key);
  const int nfw = wave_sum(nf);
  double* sv = sc.sv + 4 * par;         // the buffer a span > 64 exchange did not use
  int64_t* si = sc.si + 4 * par;
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = v;
    si[threadIdx.x >> 6] = key;
    sc.sn[threadIdx.x >> 6] = nfw;
  }
  __syncthreads();
  // polled: lanes 0..4 of the first wave all fold the waves' picks (broadcast LDS reads; the pick left
  // wave 0's in every lane) and lane w stores tagged word w — one store instruction, not five in turn
  if (threadIdx.x < 5) {
    int nfs = sc.sn[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      const bool t = (int)(si[w] != kNoIndex) & (int)less_bf<0>(sv[w], si[w], v, key);
      v = t ? sv[w] : v;
      key = t ? si[w] : key;
      nfs += sc.sn[w];
    }
    if (a.poll) {
      uint64_t* r = a.blk_tag + 5 * (int64_t)blk;
      const uint64_t vb = (uint64_t)__double_as_longlong(v), kb = (uint64_t)key;
      const int w = threadIdx.x;
      uint32_t p = (uint32_t)(vb >> 32);
      p = w == 1 ? (uint32_t)vb : p;
      p = w == 2 ? (uint32_t)(kb >> 32) : p;
      p = w == 3 ? (uint32_t)kb : p;
      p = w == 4 ? (uint32_t)nfs : p;
      st_wt(&r[w], tag_word(a.seq, p));
    } else if (threadIdx.x == 0) {
      st_wt(&a.pv[blk], v);
      st_wt(&a.pidx[blk], key);
      st_wt(&a.pnf[blk], nfs);
    }
  }
}

// WQ (the throughput regime, launch_plan): a persistent layout — the grid holds one look-ahead
// block per CU and each wave takes units of 64 / G models (one model at G = 64) from the
// bank's work counter, so the staging prologue runs once per CU instead of once per 4 models
// and no CU waits for a new block between units (v29 stamps at C = 64: prologue 3.4 us and
// reduction 2 us of each 45 us block).
// (The track tick's look-ahead block, plan_track_dev.hpp track_lookahead_block, restates this function's
// kBatch / CORR path — prologue, stage_write, pin_consts, model_setup, rollouts, publication — with a poll
// of tagged words where this one loads ghp; tests/test_plan_track_gpu.py holds the two bitwise equal.  A
// change to that path here belongs there too.)
// CORR (the corridor look-ahead, plan_kernel_corr): the half-planes ghp [H][6] (global) are copied
// to LDS behind the staged inputs — loaded with the prologue's other inputs, stored ahead of its
// barrier — and every rollout adds cw times its summed squared slacks (rollout_dev.hpp kRCorr) on the
// unsplit rollout; a block-per-models launch on the shared xref only.
template <int INTEG, bool STAGE, int LPM, int XM, int WQ = 0, bool CORR = false>
__device__ __forceinline__ void lookahead_block(const LookaheadLaunch& a, int blk, int G, int cpl,
                                                unsigned char* smem, const Scratch& sc,
                                                const double* ghp = nullptr, double cw = 0.0) {
  static_assert(!CORR || (!XM && !WQ && INTEG != 2), "corridor look-ahead: shared xref, block per models, RK4 or NLP-Euler");
  LA_STAMP(blk, 0);
  constexpr int BT = wq_threads(WQ);   // threads of this block
  double* sx = reinterpret_cast<double*>(smem + kScratchBytes);
  double* su = sx + 2 * (a.H + 1);
  const int H = a.H, C = a.C;
  double* shp = nullptr;               // CORR: hp [H][6] after the staged inputs (16-B aligned rows)
  if constexpr (CORR) shp = su + (STAGE ? kStageW * C * H : 0);
  // this lane's model: its Pacejka row and the start state are loaded first, so they are in
  // flight while the block stages the shared inputs (one HBM round trip, not two)
  const int sub = threadIdx.x % LPM;
  const int cl = threadIdx.x / LPM;
  const int g = cl & (G - 1);
  const int64_t n = (int64_t)blk * (kBlock / (G * LPM)) + cl / G;
  const bool live = n < a.n;
  // XM: threads [0, mpb) walk the raceline; the U staging below runs on the threads after
  // them, so the two overlap (the walk is one lane's serial chain, latency-bound)
  const int mpb = kBlock / (G * LPM);
  const int soff = (XM && mpb < kBlock) ? mpb : 0;
  Tire t{};
  if (!WQ && live) t = load_tire(a.params, a.n, n);
  // kBatch: the shared-xref prologue that issues every input load in one batch (below).  The
  // raceline reference and the work-queue layout keep the plain prologue (the work-queue tick
  // measured 0.7 % slower with the batch and the argument touch, 358.8 -> 361.4 us at C = 64).
  constexpr bool kBatch = !XM && !WQ;
  double x0[6];
  if constexpr (!kBatch) {
#pragma unroll
    for (int m = 0; m < 6; ++m) x0[m] = a.x0[m];
  }
  // XM = 1 (per-model raceline reference): knots [n] and the x/y spline rows [2][4][n-1]
  // after the (optional) U staging; a.xref holds the shared start {s0, v0, scale}
  double* rl_knots = su + (STAGE ? kStageW * C * H : 0);
  double* rl_xy = rl_knots + a.rl.n + kKnotPad;
  if (XM) {
    const int nk = a.rl.n, nseg = a.rl.n - 1, nxy = 8 * nseg;
    const double* gk = a.rl.knots;                          // knots | xy contiguous
    const double* gmu = a.rl.mus;
    double* rl_mus = rl_xy + nxy;                           // [M], then the speed window
    // knots, the +inf pad (RaceRef::step), xy and mus in one batch (one memory round trip
    // per thread at the ETHZ size)
    copy_lds<4>(rl_knots, nk, [&](int e) { return gk[e]; });
    copy_lds<24>(rl_xy, nxy + a.rl.M, [&](int e) {
      const double* p = e < nxy ? gk + nk + e : gmu + (e - nxy);
      return *p;
    });
    if ((int)threadIdx.x < kKnotPad) rl_knots[nk + threadIdx.x] = __builtin_inf();
    // the window end: s0 plus the largest advance of H walker steps (one lap at most)
    const double s0 = a.xref[0];
    const double L = gk[nseg];
    const double adv = window_adv(a.xref[1], a.xref[2], a.Ts, H, a.rl.vmax);
    const bool bounded = adv < L && s0 >= 0.0 && s0 < L;
    double te = s0 + adv;
    if (te >= L) te -= L;
    __syncthreads();
    RL_STAMP(blk, 0);
    // bisect-right of s0 and te on the knots (RaceRef::init's: the largest i in [1, n-2]
    // with knots[i] <= s, else 0) as one parallel pass: with the knots ascending, exactly
    // one segment i has (i == 0 or knots[i] <= s) and (i == n-2 or not knots[i+1] <= s),
    // and it writes i.  XM leaves sx (the shared xref stage) unused: two ints there.
    int* rl_sel = reinterpret_cast<int*>(sx);
    for (int i = threadIdx.x; i < nseg; i += kBlock) {
      const double ki = rl_knots[i], kn = rl_knots[i + 1];
      const bool last = i == nseg - 1;
      if ((i == 0 || ki <= s0) && (last || !(kn <= s0))) rl_sel[0] = i;
      if ((i == 0 || ki <= te) && (last || !(kn <= te))) rl_sel[1] = i;
    }
    __syncthreads();
    // the speed profiles' window (raceline.hpp SpeedWin): from the start segment to the
    // window end; block-uniform
    SpeedWin sw{nullptr, 0, 0};
    const int seg0 = rl_sel[0];
    {
      const int lo = seg0, l2 = rl_sel[1];
      const double need = bounded ? (double)(l2 >= lo ? l2 - lo : l2 + nseg - lo) + 2.0 : 1e300;
#ifdef LLAMPC_STAMPS
      if (blk == 0 && threadIdx.x == 0) {
        g_rl_dbg[0] = need;
        g_rl_dbg[1] = a.rl.wcap;
        g_rl_dbg[2] = adv;
        g_rl_dbg[3] = a.xref[0];
        g_rl_dbg[4] = L;
        g_rl_dbg[5] = a.rl.vmax;
      }
#endif
      if (need <= (double)a.rl.wcap) {
        double* wl = rl_mus + ((a.rl.M + 1) & ~1);          // 16-B aligned
        sw.w = wl;
        sw.seg0 = lo;
        sw.W = (int)need;
        const int W = sw.W, tot = a.rl.M * 4 * W;
        const double* gsp = a.rl.speed;
        // element e = row W + j; copy_lds asks for e = threadIdx.x + i kBlock in order, so
        // (row, j) steps by kBlock without a division per element
        int row = (int)threadIdx.x / W, j = (int)threadIdx.x - row * W;
        const int drow = kBlock / W, dj = kBlock - drow * W, rows = a.rl.M * 4;
        copy_lds<24>(wl, tot, [&](int) {          // (row, j) past the end: clamped rows
          int sg = lo + j;
          if (sg >= nseg) sg -= nseg;
          const double v = gsp[(size_t)(row < rows ? row : rows - 1) * nseg + sg];
          row += drow;
          j += dj;
          if (j >= W) {
            j -= W;
            ++row;
          }
          return v;
        });
        __syncthreads();
      }
    }
    RL_STAMP(blk, 1);
    // one thread per model of this block walks ConstantSpeed into xref_pm[m][H][2]
    const int64_t m = (int64_t)blk * mpb + threadIdx.x;
    if ((int)threadIdx.x < mpb && m < a.n) {
      const double mu = (a.params[2 * a.n + m] + a.params[5 * a.n + m]) / (9.81 * a.veh.mass);
      // the table descriptor in registers: the walk's global stores cannot alias it
      const RacelineK rl = a.rl;
      RaceRef rr;
      rr.init(rl, rl_knots, rl_mus, mu, a.xref[0], a.xref[1], a.xref[2], a.Ts, seg0);
      double2* out = reinterpret_cast<double2*>(a.xref_pm + m * 2 * H);
      for (int k = 0; k < H; ++k) {
        double xr, yr;
        rr.step(rl, rl_knots, rl_xy, sw, xr, yr);
        out[k] = make_double2(xr, yr);
      }
    }
    RL_STAMP(blk, 2);
    __threadfence_block();
    RL_STAMP(blk, 3);
  } else if (!kBatch) {
    for (int e = threadIdx.x; e <= H; e += BT) {
      sx[2 * e] = a.xref[e];
      sx[2 * e + 1] = a.xref[(H + 1) + e];
    }
  }
  // One staged record [k][c] -> (pwm, delta, sin delta, cos delta): the steering's sincos depends
  // only on the shared candidates, so it is formed once per block (same evaluation as
  // make_input_fast: the fast core on its domain, the general function off it).  RK4 stages
  // the fused stages' input terms instead: (F0, F1, h/m sin d, h/m cos d, h lf/Iz cos d,
  // delta) — dyn.hpp fused_in, with the shared constants of make_fused.  (ua, dl): the
  // candidate's input at step k, (p0, p1): the input before it.
  auto stage_write = [&](int c, int k, double ua, double dl, double sd, double cd, double p0, double p1,
                         const FusedK& fq0) {
    double* o = su + kStageW * (k * C + c);
    const double d0 = ua - p0, d1 = dl - p1;
    if (INTEG == 0) {
      const FusedIn fi = fused_in(fq0, Input{ua, dl, sd, cd});
      o[0] = fi.F0;
      o[1] = fi.F1;
      o[2] = fi.hmsd;
      o[3] = fi.hmcd;
      o[4] = fi.c5a;
      o[5] = dl;
    } else {
      o[0] = ua;
      o[1] = dl;
      o[2] = sd;
      o[3] = cd;
    }
    o[6] = act_term(a.cost, d0, d1);
    o[7] = (!a.cost.enforce || input_feasible(a.cost, ua, dl, d0, d1)) ? 1.0 : 0.0;
  };
  // the rollouts' uniform constants in VGPRs (pin_vgpr, dev_wave.hpp)
  CostK q = a.cost;
  VehK veh = a.veh;
  double Ts = a.Ts;
  auto pin_consts = [&] {
    for (int m = 0; m < 4; ++m) {
      pin_vgpr(q.Q[m]);
      pin_vgpr(q.R[m]);
      pin_vgpr(q.P[m]);
    }
    for (int m = 0; m < 2; ++m) {
      pin_vgpr(q.umin[m]);
      pin_vgpr(q.umax[m]);
      pin_vgpr(q.dmax[m]);
    }
    pin_vgpr(veh.lf);
    pin_vgpr(veh.lr);
    pin_vgpr(veh.mass);
    pin_vgpr(veh.inv_mass);
    pin_vgpr(veh.inv_Iz);
    pin_vgpr(veh.Cm1);
    pin_vgpr(veh.Cm2);
    pin_vgpr(veh.Cr0);
    pin_vgpr(veh.Cr2);
    pin_vgpr(Ts);
  };
  // this lane's model: the stage constants of its Pacejka row.  LPM = 2: lane 0 of the pair
  // evaluates the front chain, lane 1 the rear (dyn.hpp); fused RK4 quads carry W = h omega
  // and Psi = (2/pi) psi (make_fused): the chains' lw / h turns W back into omega
  constexpr bool kScaled = (INTEG == 0 && scaled_yaw(LPM));
  StageK sk;
  FusedK fq;
  auto model_setup = [&] {
    // fused RK4 quads: lanes 2/3 return h sin / h cos psi, the rear lane (h/m) Fry (make_fused rear_hm)
    sk = make_stage<LPM>(veh, t, sub, INTEG == 0 ? Ts : 1.0, INTEG == 0 ? Ts * veh.inv_mass : 1.0);
    if (kScaled) sk.ch[0].lw = sk.ch[0].lw / Ts;
    if (kScaled && LPM == 1) sk.ch[1].lw = sk.ch[1].lw / Ts;
    if (kScaled && LPM == 4 && sub >= 2) {
      // lanes 2/3 run their (discarded) chain on zero operands — yy = z = 0, no extra
      // instruction: fewer toggling bits, a higher clock (A/B 28.86 -> 28.61 us/tick).
      // (Freezing the unused yaw of lanes 0/1 as well, by per-lane RK4 weights 0: 28.98.)
      sk.ch[0].lw = 0.0;
      sk.ch[0].sg = 0.0;
      sk.ch[0].B = 0.0;
      sk.ch[0].nsB = 0.0;
      sk.Bfw = 0.0;
    }
    fq = make_fused(veh, sk, Ts, kScaled, INTEG == 0 && LPM == 4);
  };
  // Shared xref: ONE FmK for the staging below and the rollouts (the staging uses its sincos
  // constants, the same in the lean and precise sets) instead of materialising the ~50
  // constants twice on the prologue's critical path; the raceline variant keeps two loads
  // (holding them across its prologue spilled, round 1).
  fm::FmK K0;
  double up0, up1;
  if constexpr (!kBatch) {
    if constexpr (!XM) K0 = load_la_consts<INTEG, LPM>();
    if (STAGE) {
      const fm::FmK K = [&] {
        if constexpr (XM) return fm::FmK::load();
        else return K0;
      }();
      const FusedK fq0 = make_fused(a.veh, make_stage<1>(a.veh, Tire{}, 0), a.Ts, scaled_yaw(LPM));
      for (int e = (int)threadIdx.x - soff; e < C * H; e += BT - soff) {
        if (e < 0) break;
        const int c = e / H, k = e - c * H;
        const double dl = a.U[2 * e + 1];
        double sd, cd;
        if (fm::sincos_fast_ok(dl)) fm::sincos_fast(dl, &sd, &cd, K);
        else LL_SINCOS(dl, &sd, &cd);
        const double ua = a.U[2 * e];
        const double p0 = k ? a.U[2 * e - 2] : a.uprev[0], p1 = k ? a.U[2 * e - 1] : a.uprev[1];
        stage_write(c, k, ua, dl, sd, cd, p0, p1, fq0);
      }
    }
    __syncthreads();
    pin_consts();
    up0 = a.uprev[0];
    up1 = a.uprev[1];
  } else {
    // Shared xref, a block per models: every input of the prologue in ONE memory round trip.  Behind the row loads
    // each thread issues the start state, the previous input, its reference element and its
    // staging element's inputs (the step's and the one before it) before anything waits for
    // any of them; the per-model setup runs under that latency, then the LDS writes and the
    // sincos from registers.  Indices are clamped and the loads unconditional (as copy_lds:
    // no load leaves its array, the surplus ones are not used).  The block-uniform start
    // state and previous input are loaded per lane through an opaque zero offset, so they are
    // vector loads counted in order with the others (a scalar load would be waited for at
    // once: its registers spill to lanes), and made uniform again by readfirstlane.
    const int CH = C * H, tid = (int)threadIdx.x;
    uint32_t zoff;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zoff));
    const double* gx0 = a.x0 + zoff;
    const double* gup = a.uprev + zoff;
    double xv[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) xv[m] = gx0[m];
    const double uv0 = gup[0], uv1 = gup[1];
    const int ex = tid < H ? tid : H;
    const double xr0 = a.xref[ex], xr1 = a.xref[(H + 1) + ex];
    // a staging element's loads: its input pair and the pair before it (element e - 1; at a
    // candidate's first step the previous input instead, chosen in stage_elem)
    auto stage_load = [&](int e, double& ua, double& dl, double& p0, double& p1) {
      const int ec = e < CH ? e : CH - 1, ep = ec > 0 ? ec - 1 : 0;
      ua = a.U[2 * ec];
      dl = a.U[2 * ec + 1];
      p0 = a.U[2 * ep];
      p1 = a.U[2 * ep + 1];
    };
    double sua = 0.0, sdl = 0.0, sp0 = 0.0, sp1 = 0.0;
    if (STAGE) stage_load(tid, sua, sdl, sp0, sp1);
    // CORR: this thread's two corridor elements (6 H <= 2 BT up to H = 85; the rest, if any, in a
    // plain loop below), clamped like the other loads
    [[maybe_unused]] double hv0 = 0.0, hv1 = 0.0;
    if constexpr (CORR) {
      const int nh = 6 * H;
      hv0 = ghp[tid < nh ? tid : nh - 1];
      hv1 = ghp[tid + BT < nh ? tid + BT : nh - 1];
    }
    // under the loads' latency: the polynomial constants, the pins, this lane's model
    K0 = load_la_consts<INTEG, LPM>();
    pin_consts();
    model_setup();
    for (int e = tid; e <= H; e += BT) {               // one pass unless H >= BT
      sx[2 * e] = e == tid ? xr0 : a.xref[e];
      sx[2 * e + 1] = e == tid ? xr1 : a.xref[(H + 1) + e];
    }
#pragma unroll
    for (int m = 0; m < 6; ++m) x0[m] = readfirstlane_d(xv[m]);
    up0 = readfirstlane_d(uv0);
    up1 = readfirstlane_d(uv1);
    if (STAGE) {
      const FusedK fq0 = make_fused(a.veh, make_stage<1>(a.veh, Tire{}, 0), a.Ts, scaled_yaw(LPM));
      auto stage_elem = [&](int e, double ua, double dl, double p0, double p1) {
        const int c = C == 1 ? 0 : e / H, k = e - c * H;     // C == 1: launch-uniform, no division
        double sd, cd;
        if (fm::sincos_fast_ok(dl)) fm::sincos_fast(dl, &sd, &cd, K0);
        else LL_SINCOS(dl, &sd, &cd);
        stage_write(c, k, ua, dl, sd, cd, k ? p0 : uv0, k ? p1 : uv1, fq0);
      };
      if (tid < CH) stage_elem(tid, sua, sdl, sp0, sp1);
      // C H above the block: kStageBatch elements per thread and pass, their loads together
      constexpr int kStageBatch = 4;
      for (int base = tid + BT; base < CH; base += kStageBatch * BT) {
        double ua[kStageBatch], dl[kStageBatch], p0[kStageBatch], p1[kStageBatch];
#pragma unroll
        for (int j = 0; j < kStageBatch; ++j) stage_load(base + j * BT, ua[j], dl[j], p0[j], p1[j]);
#pragma unroll
        for (int j = 0; j < kStageBatch; ++j)
          if (base + j * BT < CH) stage_elem(base + j * BT, ua[j], dl[j], p0[j], p1[j]);
      }
    }
    // a lane past the reference's or the staging's end never reads its clamped loads: without
    // this use the wait for them lands in the rollout loop, where their registers are reused
    asm volatile("" ::"v"(xr0), "v"(xr1), "v"(sua), "v"(sdl), "v"(sp0), "v"(sp1));
    if constexpr (CORR) {
      const int nh = 6 * H;
      if (tid < nh) shp[tid] = hv0;
      if (tid + BT < nh) shp[tid + BT] = hv1;
      for (int e = tid + 2 * BT; e < nh; e += BT) shp[e] = ghp[e];
      asm volatile("" ::"v"(hv0), "v"(hv1));
    }
    __syncthreads();
  }

  double bv = __builtin_nan("");
  int64_t bc = kNoIndex;
  int nf = 0;
  LA_STAMP(blk, 1);
  // position split of the quad (fused RK4, LPM = 4) when Q and P are diagonal (rt.py:60-62:
  // Q = diag(1, 1), P = 0): tested on the unpinned kernel-argument copy, so the branch is
  // scalar
  constexpr bool kSplit = (INTEG == 0 && LPM == 4);
  // the rollouts' variant: the re-run of bad lanes is kRF itself, the fast run adds kRFast
  constexpr unsigned kRF = (STAGE ? kRStage : 0u) | (XM ? kRXm : 0u);
  // the quad's position split, as a per-step quadrature in lanes 2/3 (dyn.hpp step_fused kPosQuadr)
  constexpr unsigned kRSplitQ = kSplit ? (kRSplit | kRQuadr) : 0u;
  const bool diagQP = a.cost.Q[1] == 0.0 && a.cost.Q[2] == 0.0 && a.cost.P[1] == 0.0 && a.cost.P[2] == 0.0;
  if constexpr (WQ) {
    static_assert(LPM == 1 && XM == 0, "work queue: LPM 1, shared xref");
    // Unit u = models [u mpw, (u + 1) mpw) of one wave.  Lane 0 takes unit numbers from the
    // bank's counter (relaxed agent-scope add; 0 at the launch's start: the block completing
    // the record resets it in final_write, after every look-ahead block has published, i.e.
    // after every take of the launch); the next take is issued before the current unit's
    // rollouts and read after them, so its latency is hidden.  The counter only grows within
    // a launch, so u >= 0 and every model index is checked against n.
    const int mpw = 64 / G;
    const int64_t units = (a.n + mpw - 1) / mpw;
    const int lm = (int)(threadIdx.x & 63) / G;
    // The take must stay in flight across the rollouts.  In v30 every unit waited for its
    // round trip (ISA: s_waitcnt vmcnt(0) right after the atomic): the atomic optimizer
    // rewrites an atomic on a uniform address into one lane's atomic plus a
    // readfirstlane/prefix epilogue that uses the result at once.  So the address carries an
    // opaque zero VGPR offset (not uniform to the compiler: no optimizer rewrite).  And with
    // the row loads and the atomic both pending, the waitcnt pass cannot count them apart
    // (a returning atomic and loads are different event kinds: it waits for vmcnt(0), i.e.
    // for the atomic too, at the first use of the row); so the offset of each take is a zero
    // that depends on the unit's Pacejka row (an asm reading the six values): the row is
    // waited for first, then the atomic goes out and nothing waits for it until take().
    uint32_t zoff;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zoff));
    auto issue = [&](uint32_t off) -> uint64_t {
      uint64_t v = 0;
      if ((threadIdx.x & 63) == 0)
        v = __hip_atomic_fetch_add(a.wq + off, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return v;
    };
    auto take = [&](uint64_t v) -> int64_t {
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 0);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 0);
      return (int64_t)(((uint64_t)hi << 32) | lo);
    };
    double vacc = __builtin_nan("");
    int64_t kacc = kNoIndex;
    int nfacc = 0;
    const fm::FmK K = K0;
#ifdef LLAMPC_STAMPS
    int ju = 0;                                             // this wave's unit count
#endif
    for (int64_t u = take(issue(zoff)); u < units;) {      // wave-uniform
      WQ_STAMP(blk, ju, 0);
      const int64_t nm = u * mpw + lm;
      const bool lv = nm < a.n;
      Tire tm{};
      if (lv) tm = load_tire(a.params, a.n, nm);
      uint32_t dep;
      asm volatile("v_mov_b32 %0, 0" : "=v"(dep) : "v"(tm.Bf), "v"(tm.Cf), "v"(tm.Df), "v"(tm.Br), "v"(tm.Cr), "v"(tm.Dr));
      WQ_STAMP(blk, ju, 1);
      const uint64_t nxt = issue(dep);
      double mv = __builtin_nan("");
      int64_t mc = kNoIndex;
      if (lv) {
        constexpr bool kScaled = (INTEG == 0 && scaled_yaw(1));
        StageK sk = make_stage<1>(veh, tm, 0, INTEG == 0 ? Ts : 1.0);
        if (kScaled) {                  // the chains' lw / h turns W back into omega
          sk.ch[0].lw = sk.ch[0].lw / Ts;
          sk.ch[1].lw = sk.ch[1].lw / Ts;
        }
        const FusedK fq = make_fused(veh, sk, Ts, kScaled);
        for (int j = 0; j < cpl; ++j) {
          const int c = g + j * G;
          if (c >= C) break;
          bool bad = false;
          double J = rollout<INTEG, 1, kRF | kRFast>(a, c, nm, x0, sx, su, veh, tm, sk, q, Ts, up0, up1, K, fq, bad);
          if (__builtin_expect(__any(bad), 0)) {
            bool unused = false;
            if (bad) J = rollout<INTEG, 1, kRF>(a, c, nm, x0, sx, su, veh, tm, sk, q, Ts, up0, up1, K, fq, unused);
          }
          if (a.cost_out) a.cost_out[nm * C + c] = J;
          nfacc += !isfinite(J);
          if (less_nan_last(J, c, mv, mc)) {
            mv = J;
            mc = c;
          }
        }
      }
      for (int off = G >> 1; off >= 1; off >>= 1) {        // the model's argmin over its lanes
        const double ov = __shfl_xor(mv, off, 64);
        const int64_t oc = __shfl_xor(mc, off, 64);
        if (less_nan_last(ov, oc, mv, mc)) {
          mv = ov;
          mc = oc;
        }
      }
      WQ_STAMP(blk, ju, 2);
      const int64_t un = take(nxt);                         // before the unit's stores
      if (lv && g == 0) {
        if (a.poll) {
          st_wt(&a.la_tag[nm], tag_word(a.seq, (uint32_t)(__double_as_longlong(mv) >> 32)));
          st_wt(&a.la_tag[a.n + nm], tag_word(a.seq, (uint32_t)__double_as_longlong(mv)));
          st_wt(&a.la_tag[2 * a.n + nm], tag_word(a.seq, (uint32_t)(int32_t)mc));
        } else {
          st_wt(&a.best_cand[nm], (int32_t)mc);
          st_wt(&a.best_cost[nm], mv);
        }
        if (mc != kNoIndex) {
          const int64_t key = (a.goff + nm) * C + mc;
          if (less_bf<0>(mv, key, vacc, kacc)) {
            vacc = mv;
            kacc = key;
          }
        }
      }
      WQ_STAMP(blk, ju, 3);
#ifdef LLAMPC_STAMPS
      ++ju;
#endif
      u = un;
    }
    LA_STAMP(blk, 2);
    la_publish<BT / 64>(a, blk, sc, 0, vacc, kacc, nfacc);
    LA_STAMP(blk, 3);
    return;
  }
  if (live) {
    if constexpr (!kBatch) model_setup();   // the batched prologue: ahead of the barrier
    const fm::FmK K = [&] {
      if constexpr (XM) return load_la_consts<INTEG, LPM>();
      else return K0;
    }();
    for (int j = 0; j < cpl; ++j) {
      const int c = g + j * G;
      if (c >= C) break;
      bool bad = false;
      double J;
      if constexpr (CORR)               // the unsplit rollout whatever Q and P: the lane needs X and Y
        J = rollout<INTEG, LPM, kRF | kRFast | kRCorr>(a, c, n, x0, sx, su, veh, t, sk, q, Ts, up0, up1, K, fq, bad,
                                                       nullptr, nullptr, nullptr, 0, nullptr, shp, cw);
      else if (kSplit && diagQP)        // launch-uniform (kernel arguments)
        J = rollout<INTEG, LPM, kRF | kRFast | kRSplitQ>(a, c, n, x0, sx, su, veh, t, sk, q, Ts, up0, up1, K, fq, bad);
      else
        J = rollout<INTEG, LPM, kRF | kRFast>(a, c, n, x0, sx, su, veh, t, sk, q, Ts, up0, up1, K, fq, bad);
      // merge_bad<LPM>(bad) (rollout_dev.hpp), open-coded: the call changes this kernel's
      // register allocation
      if (LPM == 2) {                   // the pair shares one rollout: re-run both or neither
        const int bi = bad;
        bad = __builtin_amdgcn_mov_dpp(bi, kPair0, 0xF, 0xF, false) |
              __builtin_amdgcn_mov_dpp(bi, kPair1, 0xF, 0xF, false);
      } else if (LPM == 4) {            // the quad shares one rollout
        int bi = bad;
        bi |= __builtin_amdgcn_mov_dpp(bi, kQuadX1, 0xF, 0xF, false);
        bi |= __builtin_amdgcn_mov_dpp(bi, kQuadX2, 0xF, 0xF, false);
        bad = bi;
      }
      if (__builtin_expect(__any(bad), 0)) {
        bool unused = false;
        if constexpr (CORR) {
          if (bad) J = rollout<INTEG, LPM, kRF | kRCorr>(a, c, n, x0, sx, su, veh, t, sk, q, Ts, up0, up1, K, fq, unused,
                                                         nullptr, nullptr, nullptr, 0, nullptr, shp, cw);
        } else {
          if (bad) J = rollout<INTEG, LPM, kRF>(a, c, n, x0, sx, su, veh, t, sk, q, Ts, up0, up1, K, fq, unused);
        }
      }
      if (sub == 0) {
        if (a.cost_out) a.cost_out[n * C + c] = J;
        nf += !isfinite(J);
      }
      if (less_nan_last(J, c, bv, bc)) {
        bv = J;
        bc = c;
      }
    }
  }
  LA_STAMP(blk, 2);
#ifdef LLAMPC_STAMPS
  if ((threadIdx.x & 63) == 0 && blk < 1024) g_la_wave[blk][threadIdx.x >> 6] = __builtin_amdgcn_s_memrealtime();
#endif
  // per-model argmin over its candidates: xor-shuffles across the model's lanes inside a
  // wave, then (a model spanning 2 or 4 waves: G*LPM in {128, 256}) across its waves in LDS
  const int span = G * LPM;
  for (int off = (span < 64 ? span : 64) >> 1; off >= LPM; off >>= 1) {
    const double ov = __shfl_xor(bv, off, 64);
    const int64_t oc = __shfl_xor(bc, off, 64);
    if (less_nan_last(ov, oc, bv, bc)) {
      bv = ov;
      bc = oc;
    }
  }
  int par = 0;
  if (span > 64) {                                  // block-uniform
    double* sv = sc.sv + 4 * par;
    int64_t* si = sc.si + 4 * par;
    par ^= 1;
    if ((threadIdx.x & 63) == 0) {
      sv[threadIdx.x >> 6] = bv;
      si[threadIdx.x >> 6] = bc;
    }
    __syncthreads();
    const int w0 = (int)(threadIdx.x / span) * (span / 64);
    bv = sv[w0];
    bc = si[w0];
    for (int k = 1; k < span / 64; ++k) {
      if (less_nan_last(sv[w0 + k], si[w0 + k], bv, bc)) {
        bv = sv[w0 + k];
        bc = si[w0 + k];
      }
    }
  }
  if (live && g == 0 && sub == 0) {
    if (a.poll) {                       // tagged words only (SoA: coalesced rows).  All three at C = 1
      // too, where the candidate is 0: leaving the third out (and final_poll not waiting for it) did not
      // make the tick faster (DESIGN.md §3 "Round 13")
      st_wt(&a.la_tag[n], tag_word(a.seq, (uint32_t)(__double_as_longlong(bv) >> 32)));
      st_wt(&a.la_tag[a.n + n], tag_word(a.seq, (uint32_t)__double_as_longlong(bv)));
      st_wt(&a.la_tag[2 * a.n + n], tag_word(a.seq, (uint32_t)(int32_t)bc));
    } else {
      st_wt(&a.best_cand[n], (int32_t)bc);
      st_wt(&a.best_cost[n], bv);
    }
  }
  // per-block argmin over (model, candidate) in flattened order (goff+n)*C + c
  const int64_t key = (live && bc != kNoIndex && g == 0 && sub == 0) ? (a.goff + n) * C + bc : kNoIndex;
  la_publish(a, blk, sc, par, (key == kNoIndex) ? __builtin_nan("") : bv, key, nf);
  LA_STAMP(blk, 3);
}

}  // namespace llampc

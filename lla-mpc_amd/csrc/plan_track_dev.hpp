// plan_track_dev.hpp — the track tick's block roles (plan_kernel_track, instantiated in plan_track_rk4.hip):
// the corridor block, the look-ahead block that polls the tick's half-planes, the completing block's
// re-run of the chosen rollout (the next tick's path) and the kernel's role frame.  The look-ahead
// block restates lookahead_block<RK4, STAGE, LPM, 0, 0, CORR> (lookahead_dev.hpp) statement for
// statement, with the poll of the tagged half-plane words where that one loads ghp: shared through
// one function the corridor launch's code objects moved.  Included by plan_track_rk4.hip only.
#pragma once
#include "corridor_block_dev.hpp"
#include "ctl_door_dev.hpp"
#include "plan_dev.hpp"

namespace llampc {

#ifdef LLAMPC_STAMPS
// Diagnostic build only: s_memrealtime (100 MHz) per block (by grid index, the first 1024) and phase of
// the last track tick (tools/diag/track_phases.py; the reader, llampc_debug_track_ph, is in
// plan_track_rk4.hip).  Corridor blocks: 0 entry, 1 row published.  Look-ahead blocks: 0 entry, 1 inputs
// staged, 2 half-planes polled, 3 rolled out, 4 published.  The completing block: 5 completion entered,
// 6 record (and host tag) stored, 7 path written.
static __device__ unsigned long long g_trk_ph[1024][8];
#define TRK_STAMP(slot)                                                                              \
  do {                                                                                               \
    if (threadIdx.x == 0 && blockIdx.x < 1024) g_trk_ph[blockIdx.x][slot] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define TRK_STAMP(slot) LLAMPC_NO_STAMP
#endif

// Corridor block k (1..H): the track's half-planes at path point P_k, published as the tagged words
// hp_tag[12 (k - 1)..] (ctl_corr.hip ctl_corridor_block), with plain copies of P, the row and theta for
// the read-back.  `valid` is launch-uniform: the host's half and the flag stored with the path.
__device__ __forceinline__ void track_corridor_block(const PlanTrack& k, int kk, unsigned char* smem) {
  TRK_STAMP(0);
  const bool valid = k.path_ok != 0 && *k.valid_rd != 0;
  const double nan = __builtin_nan("");
  double px = nan, py = nan, p0x = nan, p0y = nan;
  if (valid) {
    px = k.path_rd[kk];
    py = k.path_rd[kPlanPathStride + kk];
    if (kk == 1) {                      // P_0, which no row reads: for the read-back alone
      p0x = k.path_rd[0];
      p0y = k.path_rd[kPlanPathStride];
    }
  }
  auto emit = [&](const double* row, double theta) {   // thread 0
    uint64_t* w = k.hp_tag + 12 * (size_t)(kk - 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const uint64_t b = (uint64_t)__double_as_longlong(row[i]);
      st_wt(&w[2 * i], tag_word(k.seq, (uint32_t)(b >> 32)));
      st_wt(&w[2 * i + 1], tag_word(k.seq, (uint32_t)b));
    }
    // the read-back (llampc_bank_track_corridor): plain stores, read after the stream has drained
    double* d = k.dbg;
    d[kk] = px;
    d[kPlanPathStride + kk] = py;
    if (kk == 1) {
      d[0] = p0x;
      d[kPlanPathStride] = p0y;
      *k.dbg_valid = valid;
    }
    double* dh = d + 2 * kPlanPathStride + 6 * (size_t)(kk - 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) dh[i] = row[i];
    d[2 * kPlanPathStride + 6 * LLAMPC_HMAX + (kk - 1)] = theta;
    TRK_STAMP(1);
  };
  if (valid) {
    corridor_block(k.trk, smem, px, py, k.hw, emit);
  } else if (threadIdx.x == 0) {
    const double inf = __builtin_inf();
    const double row[6] = {0.0, 0.0, inf, 0.0, 0.0, inf};   // constraints.disabled's row
    emit(row, nan);
  }
}

// The tick's half-planes into LDS (shp [H][6]): each thread polls its share of the 12 H tagged halves
// (word 2 i the high half of value i, 2 i + 1 the low one) under the track tick's bound
// (ctl_lookahead<LPM, true>).  A word that never comes leaves a zero; returns whether one did not.
__device__ __forceinline__ int track_poll_hp(const PlanTrack& k, int H, double* shp) {
  uint32_t* hp32 = reinterpret_cast<uint32_t*>(shp);
  int any = 0;
  for (int e = threadIdx.x; e < 12 * H; e += kBlock) {
    int late = 0;
    const uint32_t v = poll_tag(k.hp_tag, e, k.seq, k.poll, late);
    hp32[(e & ~1) | ((e & 1) ^ 1)] = late ? 0u : v;
    any |= late;
  }
  return any;
}

// The staged record of (candidate c, step k) at `o` (lookahead_block's stage_write, RK4): the fused
// stages' input terms (F0, F1, h/m sin d, h/m cos d, h lf/Iz cos d, delta), the input-rate cost term
// and the feasibility.  (ua, dl): the candidate's input at step k, (p0, p1): the input before it.
__device__ __forceinline__ void track_stage_write(const LookaheadLaunch& a, double* o, double ua, double dl, double sd,
                                                  double cd, double p0, double p1, const FusedK& fq0) {
  const double d0 = ua - p0, d1 = dl - p1;
  const FusedIn fi = fused_in(fq0, Input{ua, dl, sd, cd});
  o[0] = fi.F0;
  o[1] = fi.F1;
  o[2] = fi.hmsd;
  o[3] = fi.hmcd;
  o[4] = fi.c5a;
  o[5] = dl;
  o[6] = act_term(a.cost, d0, d1);
  o[7] = (!a.cost.enforce || input_feasible(a.cost, ua, dl, d0, d1)) ? 1.0 : 0.0;
}

// The rollouts' uniform constants in VGPRs (lookahead_block's pin_consts).
__device__ __forceinline__ void track_pin_consts(CostK& q, VehK& veh, double& Ts) {
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
}

// A lane's model constants (lookahead_block's model_setup, fused RK4): its stage constants, the quad's
// zero-operand chains in lanes 2 / 3, the fused constants.
template <int LPM>
__device__ __forceinline__ void track_model_setup(const VehK& veh, const Tire& t, int sub, double Ts, StageK& sk,
                                                  FusedK& fq) {
  constexpr bool kScaled = scaled_yaw(LPM);
  sk = make_stage<LPM>(veh, t, sub, Ts, Ts * veh.inv_mass);
  if (kScaled) sk.ch[0].lw = sk.ch[0].lw / Ts;
  if (kScaled && LPM == 1) sk.ch[1].lw = sk.ch[1].lw / Ts;
  if (kScaled && LPM == 4 && sub >= 2) {
    sk.ch[0].lw = 0.0;
    sk.ch[0].sg = 0.0;
    sk.ch[0].B = 0.0;
    sk.ch[0].nsB = 0.0;
    sk.Bfw = 0.0;
  }
  fq = make_fused(veh, sk, Ts, kScaled, LPM == 4);
}

// A look-ahead block of the track tick: lookahead_block<RK4, STAGE, LPM, 0, 0, CORR>'s batched prologue,
// rollouts, cost and publication, with hp polled from the corridor blocks' tagged words (blocks of lower
// index, which wait for nothing) instead of loaded from global memory.  A word that never came: the
// tick's late word, stored and drained before anything of this block is published.
template <bool STAGE, int LPM>
__device__ __forceinline__ void track_lookahead_block(const LookaheadLaunch& a, int blk, int G, int cpl,
                                                      unsigned char* smem, const Scratch& sc, const PlanTrack& trk) {
  LA_STAMP(blk, 0);
  TRK_STAMP(0);
  constexpr int BT = kBlock;
  double* sx = reinterpret_cast<double*>(smem + kScratchBytes);
  double* su = sx + 2 * (a.H + 1);
  const int H = a.H, C = a.C;
  double* shp = su + (STAGE ? kStageW * C * H : 0);   // hp [H][6] after the staged inputs (16-B aligned rows)
  const int sub = threadIdx.x % LPM;
  const int cl = threadIdx.x / LPM;
  const int g = cl & (G - 1);
  const int64_t n = (int64_t)blk * (kBlock / (G * LPM)) + cl / G;
  const bool live = n < a.n;
  Tire t{};
  if (live) t = load_tire(a.params, a.n, n);
  double x0[6];
  CostK q = a.cost;
  VehK veh = a.veh;
  double Ts = a.Ts;
  StageK sk;
  FusedK fq;
  fm::FmK K0;
  double up0, up1;
  {
    // every input of the prologue in ONE memory round trip (lookahead_block kBatch)
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
    auto stage_load = [&](int e, double& ua, double& dl, double& p0, double& p1) {
      const int ec = e < CH ? e : CH - 1, ep = ec > 0 ? ec - 1 : 0;
      ua = a.U[2 * ec];
      dl = a.U[2 * ec + 1];
      p0 = a.U[2 * ep];
      p1 = a.U[2 * ep + 1];
    };
    double sua = 0.0, sdl = 0.0, sp0 = 0.0, sp1 = 0.0;
    if (STAGE) stage_load(tid, sua, sdl, sp0, sp1);
    // under the loads' latency: the polynomial constants, the pins, this lane's model
    K0 = load_la_consts<0, LPM>();
    track_pin_consts(q, veh, Ts);
    track_model_setup<LPM>(veh, t, sub, Ts, sk, fq);
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
        track_stage_write(a, su + kStageW * (k * C + c), ua, dl, sd, cd, k ? p0 : uv0, k ? p1 : uv1, fq0);
      };
      if (tid < CH) stage_elem(tid, sua, sdl, sp0, sp1);
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
    asm volatile("" ::"v"(xr0), "v"(xr1), "v"(sua), "v"(sdl), "v"(sp0), "v"(sp1));
    TRK_STAMP(1);
    // the tick's half-planes, last: the corridor blocks run beside this prologue
    if (track_poll_hp(trk, H, shp)) {
      st_wt(trk.late, trk.seq);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    TRK_STAMP(2);
    __syncthreads();
  }

  double bv = __builtin_nan("");
  int64_t bc = kNoIndex;
  int nf = 0;
  LA_STAMP(blk, 1);
  constexpr unsigned kRF = STAGE ? kRStage : 0u;
  const double cw = trk.weight;
  if (live) {
    const fm::FmK K = K0;
    for (int j = 0; j < cpl; ++j) {
      const int c = g + j * G;
      if (c >= C) break;
      bool bad = false;
      double J = rollout<0, LPM, kRF | kRFast | kRCorr>(a, c, n, x0, sx, su, veh, t, sk, q, Ts, up0, up1, K, fq, bad,
                                                        nullptr, nullptr, nullptr, 0, nullptr, shp, cw);
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
        if (bad) J = rollout<0, LPM, kRF | kRCorr>(a, c, n, x0, sx, su, veh, t, sk, q, Ts, up0, up1, K, fq, unused,
                                                   nullptr, nullptr, nullptr, 0, nullptr, shp, cw);
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
  TRK_STAMP(3);
  // per-model argmin over its candidates, then the block's partial (lookahead_block)
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
    if (a.poll) {
      st_wt(&a.la_tag[n], tag_word(a.seq, (uint32_t)(__double_as_longlong(bv) >> 32)));
      st_wt(&a.la_tag[a.n + n], tag_word(a.seq, (uint32_t)__double_as_longlong(bv)));
      st_wt(&a.la_tag[2 * a.n + n], tag_word(a.seq, (uint32_t)(int32_t)bc));
    } else {
      st_wt(&a.best_cand[n], (int32_t)bc);
      st_wt(&a.best_cost[n], bv);
    }
  }
  const int64_t key = (live && bc != kNoIndex && g == 0 && sub == 0) ? (a.goff + n) * C + bc : kNoIndex;
  la_publish(a, blk, sc, par, (key == kNoIndex) ? __builtin_nan("") : bv, key, nf);
  LA_STAMP(blk, 3);
  TRK_STAMP(4);
}

// The completing block, once the record is out (and, with host completion, its tag stored): the chosen
// (sel_model, sel_cand) rollout again with its positions stored — the look-ahead's own instantiation and
// operands (kRF | kRFast | kRCorr, the slow path when the fast one flags `bad`), with kRPos: the same
// evaluation with the stores (rollout_dev.hpp) — then P_j = X[ctl_path_index(j, H)], the cost and the
// valid flag into the path state's write copy.  The block has none of a look-ahead block's LDS (it may
// be a look-back block), so it builds what ONE rollout reads: xref, the chosen candidate's staged
// records as candidate 0 of 1 (the same expressions on the same operands), hp from the tagged words —
// every one published long ago — and x_t.  LDS from kScratchBytes (launch_shape.hpp track_rerun_lds_bytes).
template <bool STAGE, int LPM>
__device__ __forceinline__ void track_path_update(const LookaheadLaunch& a, const FinalLaunch& f, const PlanTrack& trk,
                                                  unsigned char* smem) {
  const int tid = threadIdx.x, H = a.H;
  double* sx = reinterpret_cast<double*>(smem + kScratchBytes);
  double* su = sx + 2 * (H + 1);                       // [H][kStageW]
  double* shp = su + kStageW * H;
  double* ppos = shp + 6 * H;                          // X | Y, [2][H + 1]
  double* sx0 = ppos + 2 * (H + 1);                    // x_t [6]
  double* pcost = sx0 + 6;                             // the re-run's cost
  int64_t* psel = reinterpret_cast<int64_t*>(pcost + 1);   // the record's sel_model
  int* pint = reinterpret_cast<int*>(psel + 1);        // sel_cand, sel_owned, the cost is finite
  __syncthreads();                                     // the completion's LDS reads are over
  if (tid == 0) {                                      // the record this thread stored (final_write)
    psel[0] = ld_wt(&f.out->sel_model);
    pint[0] = ld_wt(&f.out->sel_cand);
    pint[1] = ld_wt(&f.out->sel_owned);
    pint[2] = 0;
    *pcost = __builtin_nan("");
  }
  __syncthreads();
  const int64_t sel = psel[0];
  const int cand = pint[0];
  const bool can = pint[1] == 1 && cand >= 0 && cand < a.C && sel >= a.goff && sel < a.goff + a.n;
  if (!can) {                                          // block-uniform: no path from this tick
    if (tid == 0) {
      *trk.cost_wr = __builtin_nan("");
      *trk.valid_wr = 0;
    }
    return;
  }
  // one candidate of one: the rollout indexes a.U and the staged records by (c H + k) and (k C + c)
  LookaheadLaunch a1 = a;
  a1.C = 1;
  a1.U = a.U + 2 * (size_t)cand * H;
  const fm::FmK K0 = load_la_consts<0, LPM>();
  for (int e = tid; e <= H; e += kBlock) {
    sx[2 * e] = a.xref[e];
    sx[2 * e + 1] = a.xref[(H + 1) + e];
  }
  if (tid < 6) sx0[tid] = a.x0[tid];
  const double uv0 = a.uprev[0], uv1 = a.uprev[1];
  if (STAGE) {
    const FusedK fq0 = make_fused(a.veh, make_stage<1>(a.veh, Tire{}, 0), a.Ts, scaled_yaw(LPM));
    for (int k = tid; k < H; k += kBlock) {
      const double ua = a1.U[2 * k], dl = a1.U[2 * k + 1];
      const double p0 = k ? a1.U[2 * k - 2] : uv0, p1 = k ? a1.U[2 * k - 1] : uv1;
      double sd, cd;
      if (fm::sincos_fast_ok(dl)) fm::sincos_fast(dl, &sd, &cd, K0);
      else LL_SINCOS(dl, &sd, &cd);
      track_stage_write(a, su + kStageW * k, ua, dl, sd, cd, p0, p1, fq0);
    }
  }
  (void)track_poll_hp(trk, H, shp);
  __syncthreads();
  if (tid < LPM) {
    const int sub = tid;
    const Tire t = load_tire(a.params, a.n, sel - a.goff);
    CostK q = a.cost;
    VehK veh = a.veh;
    double Ts = a.Ts;
    track_pin_consts(q, veh, Ts);
    StageK sk;
    FusedK fq;
    track_model_setup<LPM>(veh, t, sub, Ts, sk, fq);
    double x0[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) x0[m] = sx0[m];
    constexpr unsigned kRF = STAGE ? kRStage : 0u;
    double* dp = sub == 0 ? ppos : nullptr;
    bool bad = false, unused = false;
    double Jw = rollout<0, LPM, kRF | kRFast | kRCorr | kRPos>(a1, 0, sel - a.goff, x0, sx, su, veh, t, sk, q, Ts, uv0, uv1,
                                                               K0, fq, bad, nullptr, nullptr, dp, H + 1, nullptr, shp,
                                                               trk.weight);
    merge_bad<LPM>(bad);
    if (bad)
      Jw = rollout<0, LPM, kRF | kRCorr | kRPos>(a1, 0, sel - a.goff, x0, sx, su, veh, t, sk, q, Ts, uv0, uv1, K0, fq,
                                                 unused, nullptr, nullptr, dp, H + 1, nullptr, shp, trk.weight);
    if (sub == 0) {
      *pcost = Jw;
      pint[2] = (int)(fabs(Jw) <= __DBL_MAX__);
    }
  }
  __syncthreads();
  if (tid < 64) {
    bool ok = pint[2] != 0;
    for (int e = tid; e < 2 * (H + 1); e += 64) {
      const int row = e / (H + 1), j = e - row * (H + 1);
      const double v = ppos[row * (H + 1) + ctl_path_index(j, H)];   // X_1 .. X_H: X_0 is in no path
      ok = ok && fabs(v) <= __DBL_MAX__;
      trk.path_wr[row * kPlanPathStride + j] = v;
    }
    const int all = __all(ok);
    if (tid == 0) {
      *trk.cost_wr = *pcost;
      *trk.valid_wr = all;
    }
  }
  TRK_STAMP(7);
}

// The record's end, which final_write left to this launch (its FinalLaunch copy carries no host tag): a
// look-ahead block's wait that ran out turns the status, then — host completion — every record store is
// performed and the tag stored (final_write's own order).
__device__ __forceinline__ void track_finish(const FinalLaunch& f, const PlanTrack& trk) {
  if (threadIdx.x == 0 && ld_wt(trk.late) == trk.seq) st_wt(&f.out->status, (int32_t)kPollTimeoutStatus);
  if (f.host_tag) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(f.host_tag, f.host_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// plan_body's role frame with the corridor blocks between the look-back's and the look-ahead's, and the
// path update behind both completions.
template <bool STAGE, int LPM>
__device__ __forceinline__ void plan_track_body(const LookbackLaunch& lb, const LookaheadLaunch& la,
                                                const FinalLaunch& fin, int G, int cpl, const PlanTrack& trk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Scratch sc(smem);
  int* flag = reinterpret_cast<int*>(smem + kFlagOff);
  const int blk = (int)blockIdx.x, H = la.H;
  if (blk >= fin.nb_lb && blk < fin.nb_lb + H) {
    track_corridor_block(trk, blk - fin.nb_lb + 1, smem);
    return;
  }
  FinalLaunch fq = fin;                  // the completion without the host tag: track_finish stores it
  fq.host_tag = nullptr;
  const bool is_lb = blk < fin.nb_lb;
  if (is_lb) {
    lookback_block(lb, blk, sc);
    if (!ticket_last(&fin.tickets[0], (unsigned)fin.nb_lb, flag)) return;
    if (fin.full) {
      lb_final(fin, smem);
      if (fin.host_tag) __threadfence_system();
    }
    if (fin.poll) {                     // the look-back winner completes the tick
      __syncthreads();
      TRK_STAMP(5);
      final_poll(fq, sc);
      track_finish(fin, trk);
      TRK_STAMP(6);
      track_path_update<STAGE, LPM>(la, fin, trk, smem);
      return;
    }
  } else {
    track_lookahead_block<STAGE, LPM>(la, blk - fin.nb_lb - H, G, cpl, smem, sc, trk);
    if (fin.poll) return;                // published tagged records; no ticket
  }
  const unsigned expected = (unsigned)fin.nb_la + (fin.nb_lb > 0 ? 1u : 0u);
  if (!ticket_last(&fin.tickets[1], expected, flag)) return;
  TRK_STAMP(5);
  final_select(fq, sc);
  track_finish(fin, trk);
  TRK_STAMP(6);
  track_path_update<STAGE, LPM>(la, fin, trk, smem);
}

constexpr int kArgTrack = kPlanArgBytes;
static_assert(kPlanArgBytes % alignof(PlanTrack) == 0, "the PlanTrack lies right behind (G, cpl)");

template <bool STAGE, int LPM>
__global__ __launch_bounds__(kBlock) void plan_kernel_track(LookbackLaunch, LookaheadLaunch, FinalLaunch, int, int,
                                                            PlanTrack) {
  const KernargPtr kp = touch_kernargs<kPlanArgBytes>();
  plan_track_body<STAGE, LPM>(kernarg_at<LookbackLaunch>(kp, 0), kernarg_at<LookaheadLaunch>(kp, kArgLa),
                              kernarg_at<FinalLaunch>(kp, kArgFin), kernarg_at<int>(kp, kArgG),
                              kernarg_at<int>(kp, kArgG + 4), kernarg_at<PlanTrack>(kp, kArgTrack));
}

template <bool STAGE, int LPM>
static void launch_plan_track_t(const LookbackLaunch& lb, const LookaheadLaunch& la, const FinalLaunch& f, int G,
                                int cpl, size_t lds, hipStream_t s, const PlanTrack& trk) {
  allow_lds(plan_kernel_track<STAGE, LPM>);
  hipLaunchKernelGGL((plan_kernel_track<STAGE, LPM>), dim3(f.nb_lb + la.H + f.nb_la), dim3(kBlock), lds, s, lb, la, f,
                     G, cpl, trk);
}

}  // namespace llampc

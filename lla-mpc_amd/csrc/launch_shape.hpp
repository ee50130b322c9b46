// launch_shape.hpp — the shape of a plan launch (plan_shape): the kernel family and variant a tick
// takes, its block counts, its LDS request and what it refuses, with the sizing functions and LDS
// layout constants the rule is made of.  The one statement of that rule: launch_plan (kernels.hip)
// and the C ABI's variant entries, inline-pack decision and mode refusals (capi_plan.hip) take
// it from here.  No HIP runtime call: tests/native/capi_host.cpp runs it on a machine with no GPU.
// Included by dev_wave.hpp (the constants the device code lays its LDS out by) and capi_host.hpp.
#pragma once
#include <stdlib.h>

#include <algorithm>

#include "kernels.hpp"

namespace llampc {

// Dynamic LDS carve shared by every block role (dev_wave.hpp Scratch): the role-specific region
// starts at kScratchBytes.
constexpr int kScratchBytes = 192;
constexpr int kStageW = 8;              // doubles per staged (step, candidate) input
constexpr int kRankBytes = 64 * 8 + 64 * 4 + 256;   // wave_topk_rank: keys + ids per wave (+pad)
constexpr int kWaves = kBlock / 64;     // look-back lists per block (one per wave)
constexpr int kListsPerLane = 8;        // lb_final: lists per lane of the merging wave

// A top-K entry of lb_final's merge (final_dev.hpp).
struct Ent {
  double v;
  int64_t i;
};
// A top-K entry of the cross-shard merge with its position in the gathered lists (peer_dev.hpp).
struct EntS {
  double v;
  int64_t i;
  int32_t src;
  int32_t pad;
};
// A top-K entry in LDS: its key, its local model index (ids from kNoModelId up mark lanes
// without a model: unique per slot, above every real index since n <= INT32_MAX) and value
// (lookback_dev.hpp).
struct BEnt {
  uint64_t key;
  uint32_t id;
  uint32_t pos;
  double v;
};
constexpr int kBlockMergeBytes = kWaves * LLAMPC_KMAX * (int)sizeof(BEnt);

// Staged inputs per (step, candidate): RK4 the fused stages' input terms and delta, else pwm,
// delta, sin delta, cos delta; then the input-rate cost term and the feasibility (1/0) —
// kStageW doubles.  One block per CU (the launch's LDS request), so the staging may use most of
// the CU's 160 KiB.
constexpr size_t kStageLimit = 128 * 1024;
// Every plan launch requests more than half of the CU's 160 KiB of LDS, so each block has
// its CU — and each wave its SIMD — to itself.  (Letting LPM-1 launches pack two blocks per
// CU measured no gain at C = 64: 567-574 vs 568-569 us.)  Every cross-block hand-off is an
// agent-scope atomic (sc1: L1-bypassing, st_wt / ld_wt).
constexpr size_t kOneBlockPerCuLds = 82 * 1024;
// The most a raceline launch asks for: its speed window takes what the rest leaves of this.
constexpr size_t kPlanLdsMax = 160 * 1024 - 1024;

inline int lookback_blocks(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

// Lanes (candidate slots) per model: the power of two >= C, at most one block (256); a
// model's candidates beyond G run sequentially in its lanes (cpl = ceil(C / G)).
inline int lookahead_group(int32_t C) {
  int G = 1;
  while (G < C && G < kBlock) G <<= 1;
  return G;
}

// Lanes per rollout while the launch has fewer waves than the chip has SIMDs (latency-
// bound: a wave's time is its instruction stream): a quad (LPM = 4: front chain, rear
// chain, sin psi, cos psi in one stream) up to 16k rollouts, a lane pair (front / rear
// chain) up to 32k; one lane per rollout once the chip fills (fewest instructions per
// rollout).
// share: the number of banks the caller ticks concurrently on the device (llampc_bank_set_
// concurrency): each launch is sized for 1/share of the SIMDs (BASELINE config 5, two tracks
// at N = 10^4, H = 40: LPM 2 instead of 4, so both launches are resident together — 111 ->
// 86 us per paced step, profiles/r04/config5_lpm.log).
inline int lookahead_lpm(int64_t n, int32_t C, int32_t integrator, int32_t share = 1) {
  if (integrator == LLAMPC_RK6) return 1;
  const int G = lookahead_group(C);
  if (const char* e = getenv("LLAMPC_LPM")) {     // benchmarking override, read on every call
    const int v = atoi(e);
    if (v == 1 || ((v == 2 || v == 4) && v * G <= kBlock)) return v;
  }
  const int64_t lanes = n * G * std::max(share, 1);
  if (lanes <= 16384 && 4 * G <= kBlock) return 4;
  return (lanes <= 32768 && 2 * G <= kBlock) ? 2 : 1;
}

inline int lookahead_blocks(int64_t n, int32_t C, int lpm) {
  const int mpb = kBlock / (lookahead_group(C) * lpm);
  return (int)((n + mpb - 1) / mpb);
}

// knots [n] + the +inf pad [kKnotPad] + xy [8(n-1)] + mus [M] (padded to 16 B) (the speed
// window on top: plan_shape)
inline size_t raceline_lds_bytes(int32_t n, int32_t M) {
  return 8 * (size_t)(n + kKnotPad) + 64 * (size_t)(n - 1) + 8 * (size_t)((M + 1) & ~1);
}

// A look-ahead block's LDS: the scratch, xref [H+1][2], `extra` bytes behind it (the corridor
// launch's hp [H][6]: 48 H) and the staged inputs when all of it stays within kStageLimit —
// *stage_u says whether; a shape whose inputs no longer fit goes unstaged.
inline size_t lookahead_lds_bytes(int32_t C, int32_t H, bool* stage_u, size_t extra = 0) {
  const size_t base = kScratchBytes + 16 * (size_t)(H + 1) + extra;
  const size_t ub = 8 * kStageW * (size_t)C * H;
  *stage_u = base + ub <= kStageLimit;
  return *stage_u ? base + ub : base;
}

// Models per look-back lane: lb_final holds blocks * kWaves * K entries in LDS and merges at
// most 64 * kListsPerLane lists; R grows once blocks * K would pass 640 (40 KB of LDS) or the
// blocks 64 * kListsPerLane / kWaves.
inline int lookback_r(int64_t n, int32_t K) {
  const int64_t blocks = std::min<int64_t>(640 / std::max(1, K), 64 * kListsPerLane / kWaves);
  const int64_t per = (int64_t)kBlock * std::max<int64_t>(1, blocks);   // models per R step
  return (int)std::max<int64_t>(1, (n + per - 1) / per);
}

inline int lookback_blocks_r(int64_t n, int R) { return (int)((n + (int64_t)kBlock * R - 1) / ((int64_t)kBlock * R)); }

// A look-back block's LDS once the window is full: the larger of lb_final's region (layout
// there; the plan launch's and the controller launch's) and the waves' ranking lists.
inline size_t lb_final_lds_bytes(int nb_lb, int32_t K) {
  const size_t M = (size_t)nb_lb * K, L = nb_lb;
  return std::max(kScratchBytes + 8 * (3 * M + L) + sizeof(Ent) * L * kWaves + 4 * (3 * M + L + LLAMPC_KMAX + 2) + 8 + 16,
                  kScratchBytes + (size_t)kWaves * kRankBytes + kBlockMergeBytes);
}

// The track tick's LDS besides the look-ahead's: a corridor block's two reduction rows and the centre
// line's three tables (corridor_block_dev.hpp), and the completing block's re-run of the chosen rollout
// (plan_track_dev.hpp): xref [H+1][2] | one candidate's staged inputs [H][kStageW] | hp [H][6] | the
// positions [2][H+1] | x_t [6] | the cost, its flag and the record's selection (64 B).
inline size_t track_block_lds_bytes(int32_t track_n) { return 64 + 24 * (size_t)track_n; }
inline size_t track_rerun_lds_bytes(int32_t H) {
  return kScratchBytes + 16 * (size_t)(H + 1) + 8 * kStageW * (size_t)H + 48 * (size_t)H + 16 * (size_t)(H + 1) + 48 + 64;
}

// What a plan launch is asked for (launch_plan builds it from its arguments, cus from the device).
struct PlanShapeIn {
  int64_t n;                             // the bank's models
  int32_t K;
  bool lb, full;                         // a look-back; its window full (lb_final runs)
  bool la;                               // a look-ahead of C candidates over H steps
  int32_t C, H, integrator, xref_mode;
  int32_t rl_n, rl_M;                    // the raceline's knots and frictions (LLAMPC_XREF_RACELINE)
  int32_t share;                         // banks ticked concurrently (lookahead_lpm)
  int32_t px_G;                          // the fused peer exchange's world (0: none)
  bool pack, corridor;                   // the inputs come as an InlinePack; a PlanCorridor rides along
  bool wq_counter;                       // the bank has a work-queue unit counter
  int32_t track_n;                       // the track tick: the centre line's points (0: none); a PlanTrack rides along
};

// The plan kernels by their trailing argument (plan_dev.hpp): plan_kernel, plan_kernel_inl (the
// InlinePack), plan_kernel_corr (the PlanCorridor), plan_kernel_track (the PlanTrack; plan_track_dev.hpp).
enum PlanFamily { kPlanPlain = 0, kPlanInline = 1, kPlanCorridor = 2, kPlanTrack = 3 };

// Why plan_shape refuses a launch (PlanShape::refuse points at one of these).  The corridor's
// three mode refusals are the C ABI's messages (capi_host.hpp corridor_mode_refused).
inline constexpr char kNoCorridorLookahead[] = "the corridor belongs to the look-ahead: do_lookahead is 0";
inline constexpr char kNoCorridorRk6[] = "the corridor look-ahead has no RK6 rollout";
inline constexpr char kNoCorridorRaceline[] =
    "the corridor look-ahead takes the given xref only (not LLAMPC_XREF_RACELINE)";
inline constexpr char kNoCorridorInputs[] = "the corridor launch takes device inputs and no fused peer exchange";
// The track tick's refusals (capi_host.hpp track_tick_refused passes the mode ones on).
inline constexpr char kNoTrackLookahead[] = "the track tick's corridor belongs to the look-ahead: do_lookahead is 0";
inline constexpr char kNoTrackRk6[] = "the track tick has no RK6 rollout";
inline constexpr char kNoTrackEuler[] = "the track tick has no NLP-Euler rollout (llampc_plan_corridor takes host-built rows)";
inline constexpr char kNoTrackRaceline[] = "the track tick takes the given xref only (not LLAMPC_XREF_RACELINE)";
inline constexpr char kNoTrackPack[] = "the track tick takes device inputs (no inline pack)";
inline constexpr char kNoTrackPeer[] = "the track tick has no fused peer exchange";
inline constexpr char kNoTrackCorridor[] = "the track tick builds its own corridor (no PlanCorridor beside it)";
inline constexpr char kNoIntegrator[] = "unknown integrator";
inline constexpr char kNoWork[] = "nothing to launch: no look-back and no look-ahead block";
inline constexpr char kNoPeer[] = "the fused peer exchange: RK4, the given xref, device inputs, at most kPeerFuseMax ranks";
inline constexpr char kNoPack[] = "the inline pack: an RK4 look-ahead on the given xref, staged, within kInlineDoubles";

// The shape of a plan launch.  refuse != null: the launch is invalid (nothing is enqueued) and
// no other field means anything.
struct PlanShape {
  PlanFamily family;
  int integ, lpm, G, cpl;                // the look-ahead's integrator, lanes per rollout, lanes per
  bool stage;                            //   model, candidates per lane; its inputs staged in LDS
  int wq;                                // work-queue layout (kernels.hpp wq_threads): 0, 1 or 2
  bool px, xm;                           // the fused peer exchange; the per-model raceline reference
  int R, nb_lb, nb_la, threads;          // models per look-back lane, the block counts, threads per block
  int nb_cor;                            // the track tick's corridor blocks (H), between the look-back's and the look-ahead's
  size_t lds;                            // the launch's dynamic LDS, every floor applied
  int32_t wcap;                          // the raceline's speed window, in segments
  const char* refuse;
};

// cus: the device's compute units.  The environment's A/B knobs: LLAMPC_LPM (lookahead_lpm),
// LLAMPC_NO_WQ and LLAMPC_WQ_WAVES are read on every call, LLAMPC_LB_R once per process.
inline PlanShape plan_shape(const PlanShapeIn& in, int cus) {
  PlanShape s{};
  s.family = in.track_n > 0 ? kPlanTrack : in.corridor ? kPlanCorridor : in.pack ? kPlanInline : kPlanPlain;
  s.integ = in.la ? in.integrator : LLAMPC_RK4;
  s.lpm = s.G = s.cpl = 1;
  s.threads = kBlock;
  s.px = in.px_G != 0;
  s.xm = in.la && in.xref_mode == LLAMPC_XREF_RACELINE;
  const auto no = [&s](const char* why) {
    s.refuse = why;
    return s;
  };
  // what the modes refuse, before any size is worked out.  The corridor launch: RK4 or NLP-Euler
  // on the shared xref, device inputs, no peer exchange
  if (in.track_n > 0) {
    if (!in.la) return no(kNoTrackLookahead);
    if (in.integrator == LLAMPC_RK6) return no(kNoTrackRk6);
    if (in.integrator == LLAMPC_EULER_NLP) return no(kNoTrackEuler);
    if (in.xref_mode != LLAMPC_XREF_GIVEN) return no(kNoTrackRaceline);
    if (in.pack) return no(kNoTrackPack);
    if (in.px_G) return no(kNoTrackPeer);
    if (in.corridor) return no(kNoTrackCorridor);
  }
  if (in.corridor) {
    if (!in.la) return no(kNoCorridorLookahead);
    if (in.integrator == LLAMPC_RK6) return no(kNoCorridorRk6);
    if (in.xref_mode != LLAMPC_XREF_GIVEN) return no(kNoCorridorRaceline);
    if (in.pack || in.px_G) return no(kNoCorridorInputs);
  }
  if (in.px_G && (in.pack || s.integ != LLAMPC_RK4 || s.xm || in.px_G > kPeerFuseMax)) return no(kNoPeer);
  if (in.pack && (!in.la || s.integ != LLAMPC_RK4 || in.xref_mode != LLAMPC_XREF_GIVEN || in.C < 1 || in.H < 1))
    return no(kNoPack);
  if (s.integ < LLAMPC_RK4 || s.integ > LLAMPC_RK6) return no(kNoIntegrator);
  size_t lds = kScratchBytes;
  if (in.lb) {
    // A/B knob: at least LLAMPC_LB_R models per look-back lane (fewer look-back blocks)
    static const int r_min = getenv("LLAMPC_LB_R") ? std::max(1, atoi(getenv("LLAMPC_LB_R"))) : 1;
    s.R = std::max(lookback_r(in.n, std::max(1, in.K)), r_min);
    s.nb_lb = lookback_blocks_r(in.n, s.R);
    if (in.full) lds = std::max(lds, lb_final_lds_bytes(s.nb_lb, in.K));
  }
  if (in.la) {
    s.G = lookahead_group(in.C);
    s.cpl = (in.C + s.G - 1) / s.G;
    s.lpm = lookahead_lpm(in.n, in.C, s.integ, in.share);
    s.nb_la = lookahead_blocks(in.n, in.C, s.lpm);
    if (s.xm) {
      // knots + x/y rows in LDS, the staged inputs when they fit beside them, and the rest
      // of the CU's LDS (up to the whole track) for the speed-profile window
      const size_t rl = raceline_lds_bytes(in.rl_n, in.rl_M);
      size_t base = lookahead_lds_bytes(in.C, in.H, &s.stage);
      if (base + rl > kPlanLdsMax) {
        s.stage = false;
        base = kScratchBytes + 16 * (size_t)(in.H + 1);
      }
      const size_t per_seg = 32 * (size_t)std::max(1, in.rl_M);
      const size_t room = base + rl < kPlanLdsMax ? kPlanLdsMax - base - rl : 0;
      s.wcap = (int32_t)std::min<size_t>(room / per_seg, (size_t)(in.rl_n - 1));
      lds = std::max(lds, base + rl + per_seg * (size_t)s.wcap);
    } else {
      lds = std::max(lds, lookahead_lds_bytes(in.C, in.H, &s.stage, in.corridor || in.track_n > 0 ? 48 * (size_t)in.H : 0));
    }
  }
  if (s.nb_lb + s.nb_la == 0) return no(kNoWork);
  // The track tick: H corridor blocks, each with the centre line's tables in LDS (corridor_block_dev.hpp),
  // and the completing block's re-run of the chosen rollout (plan_track_dev.hpp track_rerun_lds_bytes)
  if (in.track_n > 0) {
    s.nb_cor = in.H;
    lds = std::max(lds, std::max(track_block_lds_bytes(in.track_n), track_rerun_lds_bytes(in.H)));
  }
  // Work queue (the throughput regime): LPM 1 with a model inside one wave (G <= 64), RK4 on
  // the shared xref, device inputs, at least 1.75 rounds of look-ahead blocks per CU — then one
  // block per CU (minus the completing look-back block's) takes units of models from the
  // bank's counter: 8 waves per block (two rollout waves per SIMD) from 4 units per wave
  // slot of the 4-wave layout on, else 4 waves.  C = 64 N-sweep on one box (static / 4-wave /
  // 8-wave, us per tick; profiles/r03/v31/c64_sweep.txt): N = 1500: 92.0 / 99.5 / 106.9;
  // 2000: 128.1 / 106.5 / 155.8; 3000: 163.9 / 137.7 / 164.4; 5000: 239.4 / 206.3 / 209.5;
  // 10^4: 468.7 / 391.2 / 372.6; 2 10^4: 899.7 / 732.2 / 681.4 — the 8-wave layout's second
  // wave of a SIMD only fills the first one's bubbles, so with few units per wave the launch
  // waits for those slow units.  LLAMPC_NO_WQ=1 keeps the block-per-models layout,
  // LLAMPC_WQ_WAVES=4|8 forces a work-queue block size (A/B runs).
  if (in.la && in.wq_counter && s.lpm == 1 && s.G <= 64 && s.integ == LLAMPC_RK4 &&
      in.xref_mode == LLAMPC_XREF_GIVEN && !in.pack && !in.corridor && in.track_n <= 0 &&
      getenv("LLAMPC_NO_WQ") == nullptr) {
    const int nw = std::max(1, cus - 1);
    const char* force = getenv("LLAMPC_WQ_WAVES");
    const int forced = force ? atoi(force) : 0;
    if ((int64_t)s.nb_la * 4 >= (int64_t)nw * 7 || (forced && s.nb_la > nw)) {
      const int64_t mpw = 64 / s.G;
      const int64_t units = (in.n + mpw - 1) / mpw;
      s.nb_la = nw;
      s.wq = (s.stage && (forced ? forced == 8 : units >= 4 * (int64_t)nw * kWaves)) ? 2 : 1;
      s.threads = wq_threads(s.wq);
    }
  }
  if (in.px_G)                           // the peers' records and lists in the completing block
    lds = std::max(lds, 256 + (size_t)in.px_G * (sizeof(llampc_plan_out) + 2 * LLAMPC_KMAX * sizeof(EntS)) +
                            kWaves * sizeof(int));
  if (in.pack && (!s.stage || 16 + 2 * ((int64_t)in.H + 1) + 2 * (int64_t)in.C * in.H > kInlineDoubles))
    return no(kNoPack);
  s.lds = std::max(lds, kOneBlockPerCuLds);
  return s;
}

}  // namespace llampc

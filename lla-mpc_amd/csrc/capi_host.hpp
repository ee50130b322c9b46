// capi_host.hpp — the C ABI's host arithmetic (capi*.hip): sequence numbers, poll bounds, the
// input pack, the window unroll, the launch-argument fields that come from the bank, the plan tick's
// prepare / commit, its track state's layout and its entries' refusals, the controller launch's shape
// (the plan launch's: launch_shape.hpp), and the controller tick's prepare / commit, its speculative
// look-ahead's decision, its corridor state's layout, its doorbell's words and its entries' refusals.
// Pure: no HIP runtime call, so
// tests/native/capi_host.cpp runs all of it on a machine with no GPU.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctl.hpp"
#include "ctl_lds.hpp"
#include "kernels.hpp"
#include "launch_shape.hpp"
#include "nlp.hpp"

struct llampc_mailbox;                   // capi_common.hpp

namespace llampc {

// The two types plan_launch (capi_common.hpp) is called with across translation units, so outside the
// unnamed namespace.  A track tick's own arguments beside the plan input:
struct TrackTick {
  double weight, margin;
};

// What a tick takes beside the bank and the plan input; every field null or 0 unless named.
// out: the record (device, or the device alias of the pinned host record); err [n], wmean [n], cost
// [n][C]: device, or null.  host_tag / host_seq: host completion.  pk: the inputs as kernel arguments.
// px: the fused peer exchange, merging into px_merged.  cor: the look-ahead's corridor (device
// half-planes and weight; never with pk or px).  tt: the track tick (the corridor built in the launch
// from the bank's track and path state; never with pk, px or cor).
struct PlanTick {
  llampc_plan_out* out = nullptr;
  double* err = nullptr;
  double* wmean = nullptr;
  double* cost = nullptr;
  hipStream_t stream = nullptr;
  uint64_t* host_tag = nullptr;
  uint64_t host_seq = 0;
  const InlinePack* pk = nullptr;
  llampc_mailbox* px = nullptr;
  llampc_plan_out* px_merged = nullptr;
  const PlanCorridor* cor = nullptr;
  const TrackTick* tt = nullptr;
};

namespace {

inline VehK make_veh(const llampc_vehicle& v) {
  VehK k;
  k.lf = v.lf;
  k.lr = v.lr;
  k.mass = v.mass;
  k.inv_mass = 1 / v.mass;  // the reference's `1/self.mass` scalar (dynamic.py:111-112)
  k.inv_Iz = 1 / v.Iz;      // `1/self.Iz` (dynamic.py:113)
  k.Cm1 = v.Cm1;
  k.Cm2 = v.Cm2;
  k.Cr0 = v.Cr0;
  k.Cr2 = v.Cr2;
  k.input_acc = v.input_acc;
  k.approx = v.approx;
  return k;
}

// The constants an integrator sees: the NLP transcription (Dynamic.casadi + Euler,
// dynamic.py:214-218, nmpc.py:58-60) always uses the pwm motor model and the Pacejka tires,
// so input_acc / approx apply to the batch (RK4 / RK6) forms only.
inline VehK integrator_veh(VehK k, int32_t integrator) {
  if (integrator == LLAMPC_EULER_NLP) {
    k.input_acc = 0;
    k.approx = 0;
  }
  return k;
}

inline CostK make_cost(const llampc_cost& c, double Ts) {
  CostK k;
  for (int i = 0; i < 4; ++i) {
    k.Q[i] = c.Q[i];
    k.R[i] = c.R[i];
    k.P[i] = c.P[i];
  }
  for (int i = 0; i < 2; ++i) {
    k.umin[i] = c.umin[i];
    k.umax[i] = c.umax[i];
    // nmpc.py:104-105, tested with a relative tolerance of 1e-9: a sequence rate-clipped to the
    // bound (u_k = u_{k-1} + rate Ts, the candidate samplers) can exceed it by one rounding
    // of u_k - u_{k-1}; IPOPT itself accepts violations up to constr_viol_tol (1e-4)
    k.dmax[i] = c.rate_max[i] < 0 ? -1.0 : c.rate_max[i] * Ts * (1.0 + 1e-9);
  }
  k.enforce = c.enforce_bounds;
  k.pad = 0;
  return k;
}

// A track's centre line as llampc_nlp_set_track and llampc_ctl_set_track accept it: finite points
// centre [2][n], arc lengths theta [n] from 0 strictly increasing, a closed length beyond the last and
// long enough for the tangent's two points, a positive width.  Null if valid, else what is wrong (in buf).
inline const char* track_tables_invalid(const double* centre, const double* theta, int32_t n, double track_length,
                                        double track_width, char* buf, size_t nbuf) {
  if (n < 2 || n > kTrackMaxPoints) return (std::snprintf(buf, nbuf, "n=%d outside [2, %d]", n, kTrackMaxPoints), buf);
  for (int64_t i = 0; i < 2 * (int64_t)n; ++i)
    if (!std::isfinite(centre[i])) return (std::snprintf(buf, nbuf, "centre line: entry %lld is not finite", (long long)i), buf);
  if (!std::isfinite(track_length) || !std::isfinite(track_width)) return (std::snprintf(buf, nbuf, "length / width not finite"), buf);
  if (theta[0] != 0.0) return (std::snprintf(buf, nbuf, "theta[0] must be 0"), buf);
  for (int32_t i = 1; i < n; ++i)
    if (!std::isfinite(theta[i]) || !(theta[i] > theta[i - 1]))
      return (std::snprintf(buf, nbuf, "theta must be finite and strictly increasing (entry %d)", i), buf);
  if (!(track_length > theta[n - 1])) return (std::snprintf(buf, nbuf, "track_length must exceed theta[n-1]"), buf);
  // the tangent's points lie 2 kTangentEps apart: a shorter lap would meet itself
  if (!(track_length > 4 * kTangentEps)) return (std::snprintf(buf, nbuf, "track_length must exceed %g", 4 * kTangentEps), buf);
  if (!(track_width > 0)) return (std::snprintf(buf, nbuf, "track_width must be > 0"), buf);
  return nullptr;
}

// The host's half of the track tick's path rule (llampc_plan_track; kernels.hpp PlanTrack): the path
// state on the device is offered to a track tick only when its horizon is the tick's, and it was
// written by the bank's immediately preceding launch, itself a track tick, or seeded by
// llampc_bank_set_path since.  Any other launch on the bank, llampc_bank_reset, llampc_bank_set_track
// and llampc_bank_set_path(NULL) clear it.  H = 0: nothing on offer.
struct TrackPathState {
  int32_t H;
};
enum TrackPathEvent {
  kPathTrackTick,                        // a track tick of horizon H was enqueued: it writes the next path
  kPathSeed,                             // llampc_bank_set_path(P, H)
  kPathOtherLaunch,                      // any other plan launch on the bank
  kPathClear,                            // llampc_bank_reset, llampc_bank_set_track, llampc_bank_set_path(NULL)
};
inline TrackPathState track_path_next(TrackPathState, TrackPathEvent ev, int32_t H = 0) {
  return TrackPathState{(ev == kPathTrackTick || ev == kPathSeed) ? H : 0};
}
inline bool track_path_offered(TrackPathState s, int32_t H) { return s.H != 0 && s.H == H; }

// The track tick's weight and margin as llampc_plan_track accepts them: null if valid.
inline const char* track_tick_invalid(double weight, double margin, double track_width) {
  if (!(weight >= 0) || !std::isfinite(weight)) return "weight must be finite and >= 0";
  if (!std::isfinite(margin) || !(track_width / 2 - margin > 0)) return "margin must be finite and below track_width / 2";
  return nullptr;
}

// A corridor hp [H][6] (llampc_nlp_solve_corridor: per step (a0, a1, b, c0, c1, d), a.p <= b and
// c.p <= d) and its weight as the solve accepts them: finite normals, offsets finite or +inf (the
// disabled half-plane's), a finite weight >= 0.  Null if valid, else what is wrong.
inline const char* corridor_invalid(const double* hp, int32_t H, double weight) {
  if (!(weight >= 0) || !std::isfinite(weight)) return "weight must be finite and >= 0";
  for (int64_t k = 0; k < H; ++k) {
    const double* r = hp + 6 * k;
    if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[3]) || !std::isfinite(r[4]))
      return "a normal component is not finite";
    for (const double off : {r[2], r[5]})
      if (std::isnan(off) || off == -HUGE_VAL) return "an offset is NaN or -inf (+inf disables a half-plane)";
  }
  return nullptr;
}

// The largest slack max_k max(s1, s2) of a trajectory xmpc [H+1][6] on the corridor: row k of hp
// against the position after k + 1 steps, s = max(a.p - b, 0) in the device's order (rollout_dev.hpp
// corridor_slack2), every product and sum rounded on its own.
inline double corridor_max_slack(const double* hp, const double* xmpc, int32_t H) {
#pragma clang fp contract(off)
  double m = 0.0;
  for (int64_t k = 0; k < H; ++k) {
    const double* r = hp + 6 * k;
    const double X = xmpc[6 * (k + 1)], Y = xmpc[6 * (k + 1) + 1];
    const double g1 = (r[0] * X + r[1] * Y) - r[2];
    const double g2 = (r[3] * X + r[4] * Y) - r[5];
    if (g1 > m) m = g1;
    if (g2 > m) m = g2;
  }
  return m;
}

// What a launch of the NLP search takes from the solver's cfg and its bank (params [6][n], the
// vehicle), the same for every solve of a solver and every problem of a batch.
inline void nlp_launch_cfg(NlpLaunch& a, const llampc_nlp_cfg& k, const VehK& veh, const double* params, int64_t n) {
  a.la.params = params;
  a.la.n = n;
  a.la.veh = integrator_veh(veh, LLAMPC_EULER_NLP);
  a.la.C = 64;
  a.la.H = k.H;
  a.la.integrator = LLAMPC_EULER_NLP;
  a.la.Ts = k.Ts;
  a.la.cost = make_cost(k.cost, k.Ts);
  a.umin0 = k.cost.umin[0];
  a.umin1 = k.cost.umin[1];
  a.umax0 = k.cost.umax[0];
  a.umax1 = k.cost.umax[1];
  a.rlo0 = k.rate_lo[0];
  a.rlo1 = k.rate_lo[1];
  a.rhi0 = k.rate_hi[0];
  a.rhi1 = k.rate_hi[1];
  a.std_floor = k.std_floor;
  a.sig0 = k.sigma0[0];
  a.sig1 = k.sigma0[1];
  a.H = k.H;
  a.samples = k.samples;
  a.elite = k.elite;
  a.iters = k.iters;                    // the last round's completion writes xmpc (nmpc.py:58-60)
}

// The batched NLP solve's buffers (llampc_nlp_batch_*; nlp.hpp NlpBatch): per problem one input
// record in the pinned mapped buffer, 64-bit words x0 [6] | xref [2][H+1] | the first mean [H][2] |
// uprev [2] at up_off | the Philox seed | model index (low half), has_hold (high), padded to whole
// 64-byte lines so that no two problems share one; one region of tagged list words [2][3][samples],
// of candidate rows [2][samples][H][2], of mean / std words [2][4 HMAX]; one NlpState, one
// NlpResult and one line of host-tag words.  Problem p's part of each starts p strides in.
struct NlpBatchLayout {
  size_t rec_words, up_off;              // the record's stride and its uprev offset, in words
  size_t list_words, cand_doubles, ms_words, tag_words;
};
inline NlpBatchLayout nlp_batch_layout(int32_t H, int32_t samples) {
  NlpBatchLayout l;
  l.up_off = 6 + 2 * ((size_t)H + 1) + 2 * (size_t)H;
  l.rec_words = (l.up_off + 4 + 7) / 8 * 8;
  l.list_words = 6 * (size_t)samples;
  l.cand_doubles = 4 * (size_t)samples * (size_t)H;
  l.ms_words = 8 * (size_t)LLAMPC_HMAX;
  l.tag_words = 8;
  return l;
}
inline NlpBatch nlp_batch_arg(const NlpBatchLayout& l, const uint64_t* in, int32_t samples) {
  NlpBatch b{};
  b.in = in;
  b.cand_doubles = l.cand_doubles;
  b.rec_words = (uint32_t)l.rec_words;
  b.up_off = (uint32_t)l.up_off;
  b.list_words = (uint32_t)l.list_words;
  b.ms_words = (uint32_t)l.ms_words;
  b.tag_words = (uint32_t)l.tag_words;
  for (int nl = samples / 64; nl > 1; nl >>= 1) b.nl_log2++;
  return b;
}

// One problem's record (rec_words words at `rec`): base [H][2] or null = uprev held.
inline void nlp_batch_pack(const NlpBatchLayout& l, int32_t H, uint64_t* rec, const double* x0, const double* xref,
                           const double* uprev, const double* base, uint64_t seed, int64_t model, int32_t has_hold) {
  double* d = reinterpret_cast<double*>(rec);
  std::memcpy(d, x0, 6 * sizeof(double));
  std::memcpy(d + 6, xref, 2 * ((size_t)H + 1) * sizeof(double));
  double* m0 = d + 6 + 2 * ((size_t)H + 1);
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < 2; ++j) m0[2 * i + j] = base ? base[2 * i + j] : uprev[j];
  d[l.up_off] = uprev[0];
  d[l.up_off + 1] = uprev[1];
  rec[l.up_off + 2] = seed;
  rec[l.up_off + 3] = (uint64_t)(uint32_t)model | ((uint64_t)(uint32_t)has_hold << 32);
}

// What llampc_nlp_batch_create refuses beyond llampc_nlp_create's cfg checks: null if valid.  The
// problems' blocks wait for each other's rounds, so all of a full batch's must be resident at once
// (one block per CU by its LDS request).
inline const char* nlp_batch_create_invalid(int64_t n, int32_t samples, int32_t max_batch, int32_t cus) {
  if (n < 1) return "the bank holds no model";
  if (n > 0xFFFFFFFFll) return "the bank holds more models than a record's index word";
  if (max_batch < 1) return "max_batch must be >= 1";
  if ((int64_t)max_batch * (samples / 64) > cus) return "max_batch x samples / 64 blocks exceed the device's CUs";
  return nullptr;
}

// What llampc_nlp_batch_solve refuses before anything is written or launched: null if valid.
inline const char* nlp_batch_args_invalid(int32_t B, int32_t max_batch, const int64_t* model_idx, int64_t n,
                                          const void* x0, const void* xref, const void* uprev, const void* has_hold,
                                          const void* umpc, const void* fval, const void* xmpc, const void* status) {
  if (!model_idx || !x0 || !xref || !uprev || !has_hold || !umpc || !fval || !xmpc || !status) return "NULL argument";
  if (B < 1 || B > max_batch) return "B outside [1, max_batch]";
  for (int32_t p = 0; p < B; ++p)
    if (model_idx[p] < 0 || model_idx[p] >= n) return "a model index outside [0, n)";
  return nullptr;
}

// The batched corridor solve's buffers (llampc_nlp_batch_solve_corridor / _solve_track; nlp.hpp
// NlpBatchCorridor): per problem one part of the pinned mapped corridor buffer, doubles hp [HMAX][6]
// (rows 0..H-1 used) | theta [HMAX] at theta_off (the device builder's) | the problem's weight at
// w_off, padded to whole 64-byte lines; and one path [2][H+1] of the pinned mapped path buffer,
// padded likewise.  The problems' records (nlp_batch_layout) are untouched.
struct NlpBatchCorLayout {
  size_t cor_doubles, theta_off, w_off, path_doubles;
};
inline NlpBatchCorLayout nlp_batch_cor_layout() {
  NlpBatchCorLayout c;
  c.theta_off = 6 * (size_t)LLAMPC_HMAX;
  c.w_off = c.theta_off + (size_t)LLAMPC_HMAX;
  c.cor_doubles = (c.w_off + 1 + 7) / 8 * 8;
  c.path_doubles = (2 * ((size_t)LLAMPC_HMAX + 1) + 7) / 8 * 8;
  return c;
}
inline NlpBatchCorridor nlp_batch_cor_arg(const NlpBatch& bt, const NlpBatchCorLayout& c, const double* cor) {
  NlpBatchCorridor a{};
  a.bt = bt;
  a.cor = cor;
  a.cor_doubles = (uint32_t)c.cor_doubles;
  a.w_off = (uint32_t)c.w_off;
  return a;
}

// One problem's part (cor_doubles doubles at `part`): its weight, and its half-planes hp [H][6] — or,
// hp null, NaN in the rows and theta entries the device builder is about to write, so that a row it
// did not write fails corridor_invalid afterwards.
inline void nlp_batch_cor_pack(const NlpBatchCorLayout& c, int32_t H, double* part, const double* hp, double weight) {
  if (hp) {
    std::memcpy(part, hp, 6 * (size_t)H * sizeof(double));
  } else {
    for (int i = 0; i < 6 * H; ++i) part[i] = __builtin_nan("");
    for (int i = 0; i < H; ++i) part[c.theta_off + i] = __builtin_nan("");
  }
  part[c.w_off] = weight;
}

// What the batched corridor entries refuse, per problem, before anything is written or launched:
// null if valid, else what is wrong with the first bad problem, its index included (in buf).
// hp [B][H][6] or null (the device-built corridor: the weights alone), weight [B].
inline const char* nlp_batch_corridor_invalid(int32_t B, int32_t H, const double* hp, const double* weight, char* buf,
                                              size_t nbuf) {
  if (!weight) return "weight is NULL";
  for (int32_t q = 0; q < B; ++q) {
    const double one[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (const char* why = hp ? corridor_invalid(hp + 6 * (size_t)H * q, H, weight[q]) : corridor_invalid(one, 1, weight[q]))
      return (std::snprintf(buf, nbuf, "problem %d: %s", q, why), buf);
  }
  return nullptr;
}

// A path [2][H+1] as the track entries accept it: the first entry that is not finite, or -1; and the
// single-path entries' message for it (null if valid, else in buf).
inline int path_nonfinite(const double* path, int32_t H) {
  for (int i = 0; i < 2 * (H + 1); ++i)
    if (!std::isfinite(path[i])) return i;
  return -1;
}
inline const char* path_invalid(const double* path, int32_t H, char* buf, size_t nbuf) {
  const int i = path_nonfinite(path, H);
  return i < 0 ? nullptr : (std::snprintf(buf, nbuf, "path: entry %d is not finite", i), buf);
}
// The paths [B][2][H+1] of a device-built batch: finite.  Null if valid (else in buf, with the problem).
inline const char* nlp_batch_paths_invalid(int32_t B, int32_t H, const double* path, char* buf, size_t nbuf) {
  for (int32_t q = 0; q < B; ++q) {
    const int i = path_nonfinite(path + 2 * (size_t)(H + 1) * q, H);
    if (i >= 0) return (std::snprintf(buf, nbuf, "problem %d: path entry %d is not finite", q, i), buf);
  }
  return nullptr;
}
// A corridor margin on a track of this width, as every entry that takes one accepts it: null if valid.
inline const char* track_margin_refused(double margin, double track_width, char* buf, size_t nbuf) {
  if (std::isfinite(margin) && track_width / 2 - margin > 0) return nullptr;
  return (std::snprintf(buf, nbuf, "margin %g leaves no corridor (track width %g)", margin, track_width), buf);
}

// A problem's max_slack: corridor_max_slack of its returned trajectory; 0 for a problem whose tag
// did not arrive or that found no finite objective (its trajectory is not a solution's).
inline double nlp_batch_slack(bool arrived, int32_t best_it, const double* hp, const double* traj, int32_t H) {
  return arrived && best_it >= 0 ? corridor_max_slack(hp, traj, H) : 0.0;
}

// ---- the NLP solve's host path (capi_nlp.hip nlp_solve, capi_nlp_batch.hip nlp_batch_run) --------
// Both solves are the same six steps: guard, refuse, pack, enqueue, wait, unpack.  The call number
// (`calls`: the tag sequence host_seq = calls + 1 and the Philox counter word) advances once a solve's
// launches were enqueued, whatever its wait returned, so that none of its tagged words matches a later
// round's tag; a call refused before its enqueue leaves it alone.
//
// llampc_nlp_create's and llampc_nlp_batch_create's checks of a cfg: null if valid (else in buf).
inline const char* nlp_cfg_invalid(const llampc_nlp_cfg& k, char* buf, size_t nbuf) {
  if (k.H < 1 || k.H > LLAMPC_HMAX) return (std::snprintf(buf, nbuf, "H=%d outside [1, %d]", k.H, LLAMPC_HMAX), buf);
  if (k.samples < 64 || k.samples > 4096 || (k.samples & (k.samples - 1)))
    return (std::snprintf(buf, nbuf, "samples=%d: a power of two in [64, 4096]", k.samples), buf);
  if (k.elite < 1 || k.elite > 64 || k.elite > k.samples || k.iters < 1 || k.iters > kNlpMaxIters)
    return (std::snprintf(buf, nbuf, "elite=%d (1..64, <= samples) iters=%d (1..%d)", k.elite, k.iters, kNlpMaxIters), buf);
  if (!(k.Ts > 0) || !std::isfinite(k.Ts)) return "Ts must be finite > 0";
  if (nlp_lds_bytes(k.H, k.samples, k.elite) > kNlpLdsMax) return "H x elite too large for LDS";
  return nullptr;
}
// What a corridor solve refuses of a cfg that passed nlp_cfg_invalid: null if valid.
inline const char* nlp_corridor_cfg_invalid(const llampc_nlp_cfg& k) {
  return nlp_corridor_lds_bytes(k.H, k.samples, k.elite) > kNlpLdsMax ? "H x elite too large for LDS with a corridor" : nullptr;
}

// NlpLaunch.ltraj of a solver's plain and corridor solves (the corridor's LDS holds the half-planes
// too).  rerun: LLAMPC_NLP_RERUN_TRAJ=1 at create — always the re-run trajectory (tests).
struct NlpLtraj {
  bool plain, corridor;
};
inline NlpLtraj nlp_ltraj_flags(const llampc_nlp_cfg& k, bool rerun) {
  return {!rerun && nlp_ltraj_fits(k.H, k.samples, k.elite), !rerun && nlp_corridor_ltraj_fits(k.H, k.samples, k.elite)};
}

// What a solve's launch takes from its solver beside nlp_launch_cfg: problem 0's buffers, the call
// number, and which kernel (corridor) and how many rounds the launch is for.
struct NlpCallView {
  NlpState* st;  uint64_t* list_tag;  double* cand;  uint64_t* ms_tag;
  NlpResult* res;  uint64_t* host_tag;   // device aliases of the pinned result and tag
  uint64_t calls;
  bool corridor;
  NlpLtraj ltraj;
  int32_t rounds;                        // from round 0 on (a launch per round: the caller advances a.it)
};
inline void nlp_launch_args(NlpLaunch& a, const NlpCallView& v) {
  a.st = v.st;
  a.list_tag = v.list_tag;
  a.cand = v.cand;
  a.ms_tag = v.ms_tag;
  a.res = v.res;
  a.host_tag = v.host_tag;
  a.host_seq = v.calls + 1;
  a.call = v.calls;
  a.ltraj = v.corridor ? v.ltraj.corridor : v.ltraj.plain;
  a.it = 0;
  a.rounds = v.rounds;
}

// The single solve's inputs as kernel arguments: x0 [6] | xref [2][H+1] | the first mean [H][2] (base,
// or null = uprev held); the rest of pk is not touched.  nlp_batch_pack's counterpart.
inline void nlp_inline_pack(NlpInline& pk, int32_t H, const double* x0, const double* xref, const double* uprev,
                            const double* base) {
  std::memcpy(pk.v, x0, 6 * sizeof(double));
  std::memcpy(pk.v + 6, xref, 2 * ((size_t)H + 1) * sizeof(double));
  double* m0 = pk.v + 6 + 2 * ((size_t)H + 1);
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < 2; ++j) m0[2 * i + j] = base ? base[2 * i + j] : uprev[j];
}

// A result whose tag arrived, into umpc [H][2], fval and xmpc [H+1][6] (either may be null): its status.
inline int32_t nlp_result_unpack(const NlpResult& r, int32_t H, double* umpc, double* fval, double* xmpc) {
  std::memcpy(umpc, &r.best_u[0][0], 2 * (size_t)H * sizeof(double));
  if (fval) *fval = r.best_j;
  if (xmpc) std::memcpy(xmpc, &r.traj[0][0], 6 * ((size_t)H + 1) * sizeof(double));
  return r.best_it >= 0 ? LLAMPC_NLP_OK : LLAMPC_NLP_NO_FINITE;
}
// A batch's problem: as above if it solved; else umpc zeros and fval +inf, xmpc the trajectory if the
// tag arrived (no finite objective) and zeros if it did not.
inline int32_t nlp_batch_unpack(const NlpResult& r, bool arrived, int32_t H, double* umpc, double* fval, double* xmpc) {
  if (arrived && r.best_it >= 0) return nlp_result_unpack(r, H, umpc, fval, xmpc);
  std::memset(umpc, 0, 2 * (size_t)H * sizeof(double));
  *fval = HUGE_VAL;
  if (arrived) std::memcpy(xmpc, &r.traj[0][0], 6 * ((size_t)H + 1) * sizeof(double));
  else std::memset(xmpc, 0, 6 * ((size_t)H + 1) * sizeof(double));
  return arrived ? LLAMPC_NLP_NO_FINITE : LLAMPC_NLP_NO_TAG;
}

// The device-built half-planes of a track solve, once the stream has drained past their kernel: out of
// the mapped buffer (`mapped` [H][6]), copied to hp_out (or null), checked, and the slack of traj on them
// (solved: nlp_batch_slack's rule; slack may be null).  Null, or corridor_invalid's word on them.
inline const char* nlp_built_corridor(const double* mapped, int32_t H, double weight, double* hp_out, bool solved,
                                      const double* traj, double* slack) {
  double built[6 * LLAMPC_HMAX];
  std::memcpy(built, mapped, 6 * (size_t)H * sizeof(double));
  if (hp_out) std::memcpy(hp_out, built, 6 * (size_t)H * sizeof(double));
  if (const char* why = corridor_invalid(built, H, weight)) return why;
  if (slack) *slack = solved ? corridor_max_slack(built, traj, H) : 0.0;
  return nullptr;
}

// What a corridor solve adds to a solve of B problems (the single solver: B = 1), by mode.  given: the
// caller's half-planes src = hp [B][H][6], checked by the caller; track: the track's along src = path
// [B][2][H+1], built on the device ahead of the search, margin inside the track's edge (hp_out [B][H][6]
// or null: what the kernel built).  weight [B], max_slack [B] (the single solver's may be null).
enum class NlpCorridorMode { none, given, track };
struct NlpCorridorArgs {
  NlpCorridorMode mode = NlpCorridorMode::none;
  const double *src = nullptr, *weight = nullptr;
  double* max_slack = nullptr;
  double margin = 0.0;
  double* hp_out = nullptr;
};

// The polled completion's wait bound in s_memrealtime ticks (100 MHz): a 2 s floor plus
// 40 ns per look-ahead rollout step of the launch (a rate floor of 2.5e7 steps/s, ~10^3
// below the fast path's, so the general-path re-runs, the raceline walker and launches
// sharing the chip all fit).  A valid long tick (n = 1e7, C = 64, H = 40: ~4 s) therefore
// never reads as a timeout; only a poll that could never finish does.
// LLAMPC_POLL_BOUND_S overrides the floor and LLAMPC_POLL_STEP_NS the per-step term (tests).
inline uint64_t poll_bound_ticks(int64_t n, int32_t C, int32_t H) {
  double floor_s = 2.0, step_ns = 40.0;
  if (const char* e = getenv("LLAMPC_POLL_BOUND_S")) floor_s = std::max(0.0, atof(e));
  if (const char* e = getenv("LLAMPC_POLL_STEP_NS")) step_ns = std::max(0.0, atof(e));
  const double steps = (double)n * (double)C * (double)H;    // <= 2^57 (check_plan_in)
  const double ticks = 1e8 * floor_s + 0.1 * step_ns * steps;
  return ticks >= 1.8e19 ? ~0ull : (uint64_t)ticks;
}

// A bound of s_memrealtime ticks in the kernels' units of 2^16 ticks: rounded up, at least one,
// at most `max` (the width of the launch field that takes it).  The sum wraps in 64 bits: the
// last 0xFFFF tick values, poll_bound_ticks' ~0ull among them, give one unit.
inline uint64_t poll_units(uint64_t ticks, uint64_t max) {
  return std::min(std::max<uint64_t>((ticks + 0xFFFF) >> 16, 1), max);
}

// Next tick number of a tag sequence: never 0 (the zeroed buffers' tag), and the parity
// alternates across the 32-bit wrap (0xFFFFFFFF -> 2), so consecutive ticks of a peer
// mailbox always use different slots (seq & 1).  Callers commit it only after the launch
// that uses it was enqueued: a failed launch must not leave this rank a tick ahead.
inline uint32_t next_seq(uint32_t s) { return s == 0xFFFFFFFFu ? 2u : s + 1u; }

// Doubles of the packed inputs: x_prev[6] u_prev[2] x_now[6] uprev[2] xref[2][H+1] U[C][H][2].
inline size_t pack_len(const llampc_plan_in* in) {
  const int64_t H = in->do_lookahead ? in->H : 0, C = in->do_lookahead ? in->C : 0;
  return 16 + 2 * (H + 1) + 2 * C * H;
}

inline void pack_into(const llampc_plan_in* in, double* h) {
  const int64_t H = in->do_lookahead ? in->H : 0, C = in->do_lookahead ? in->C : 0;
  std::memset(h, 0, 16 * sizeof(double));
  if (in->x_prev) std::memcpy(h + 0, in->x_prev, 6 * sizeof(double));
  if (in->u_prev) std::memcpy(h + 6, in->u_prev, 2 * sizeof(double));
  if (in->x_now) std::memcpy(h + 8, in->x_now, 6 * sizeof(double));
  if (in->uprev) std::memcpy(h + 14, in->uprev, 2 * sizeof(double));
  if (in->do_lookahead) {
    if (in->xref_mode == LLAMPC_XREF_RACELINE) {       // {s0, v0, scale, 0} (<= 2(H+1) slots)
      std::memset(h + 16, 0, 2 * (H + 1) * sizeof(double));
      std::memcpy(h + 16, in->xref, 3 * sizeof(double));
    } else {
      std::memcpy(h + 16, in->xref, 2 * (H + 1) * sizeof(double));
    }
    std::memcpy(h + 16 + 2 * (H + 1), in->U, 2 * C * H * sizeof(double));
  }
}

// The look-back ring [W][n] (slot-major; `slot` is the next row to write, `count` rows filled)
// in the rt.py layout [n][W]: newest in column W-1, unfilled (oldest) columns zero.
inline void window_unroll(const double* raw, int64_t n, int32_t W, int32_t count, int32_t slot, double* ring) {
  for (int64_t i = 0; i < n; ++i) {
    for (int c = 0; c < W; ++c) {
      const int age = W - 1 - c;                   // 0 = newest
      double v = 0.0;
      if (age < count) {
        const int s = ((slot - 1 - age) % W + W) % W;
        v = raw[(size_t)s * n + i];
      }
      ring[(size_t)i * W + c] = v;
    }
  }
}

// What the launches take from a bank: its device buffers by address and its sizes
// (bank_view builds one per tick, on the stack).
struct BankView {
  const double* params;                  // [6][n]
  int64_t n, goff;
  VehK veh;
  double* ring;                          // [W][n]
  int32_t W, slot;
  double* wmean;                         // [n]
  double* am_val;  int64_t* am_idx;
  double* tk_val;  int64_t* tk_idx;
  const double* rl;                      // raceline table: knots | xy | speed | mus (or null)
  int32_t rl_n, rl_M;
  double rl_hmin, rl_vmax;
};

// The raceline table's sections (llampc_bank_set_raceline's layout).  wcap = 0: the plan launch
// sets it from the LDS it leaves; the controller's launch holds the whole lap.
inline RacelineK raceline_view(const BankView& b) {
  const size_t m = (size_t)b.rl_n - 1;
  RacelineK r;
  r.knots = b.rl;
  r.xy = b.rl + b.rl_n;
  r.speed = r.xy + 8 * m;
  r.mus = r.speed + 4 * m * b.rl_M;
  r.n = b.rl_n;
  r.M = b.rl_M;
  r.wcap = 0;
  r.hmin = b.rl_hmin;
  r.vmax = b.rl_vmax;
  return r;
}

// The bank's part of a tick's launch arguments, the same for a plan tick and a controller tick.
inline void bank_lookback(const BankView& b, LookbackLaunch& l) {
  l.params = b.params;
  l.n = b.n;
  l.goff = b.goff;
  l.veh = b.veh;
  l.ring = b.ring;
  l.W = b.W;
  l.slot = b.slot;
  l.wm_buf = b.wmean;
  l.am_val = b.am_val;
  l.am_idx = b.am_idx;
  l.tk_val = b.tk_val;
  l.tk_idx = b.tk_idx;
}

inline void bank_lookahead(const BankView& b, int32_t integrator, LookaheadLaunch& l) {
  l.params = b.params;
  l.n = b.n;
  l.goff = b.goff;
  l.veh = integrator_veh(b.veh, integrator);
  l.integrator = integrator;
}

inline void bank_final(const BankView& b, FinalLaunch& f) {
  f.n = b.n;
  f.goff = b.goff;
  f.params = b.params;
  f.am_val = b.am_val;
  f.am_idx = b.am_idx;
  f.tk_val = b.tk_val;
  f.tk_idx = b.tk_idx;
}

// ---- the plan tick (capi_plan.hip plan_launch) ---------------------------------------------------
// The track tick's device state (kernels.hpp PlanTrack), in the order it is allocated:
//   d_trk        path copy 0 | path copy 1 (each [2][kPlanPathStride]) | cost 0, cost 1 | the read-back:
//                path [2][kPlanPathStride] | hp [HMAX][6] | theta [HMAX] (kPlanTrackDbgDoubles in all)
//   d_trk_flags  valid 0, valid 1 | the read-back's valid | the late word
//   d_hp_tag     [12 HMAX] tagged half-plane words
// The one statement of it: the allocation, the launch arguments, the seed and the read-back take it here.
struct PlanTrackLayout {
  size_t row = kPlanPathStride;          // a path's x row, then its y row
  size_t path_doubles = 2 * row;         // one path copy
  size_t rb_path = 2 * path_doubles + 2, rb_hp = rb_path + path_doubles, rb_theta = rb_hp + 6 * LLAMPC_HMAX;
  size_t trk_doubles = rb_path + kPlanTrackDbgDoubles;
  int flag_rb_valid = 2, flag_late = 3, flags = 4;
  size_t hp_tag_words = 12 * (size_t)LLAMPC_HMAX;
  constexpr size_t path(int r) const { return path_doubles * (size_t)r; }
  constexpr size_t cost(int r) const { return 2 * path_doubles + (size_t)r; }
  constexpr int valid(int r) const { return r; }
};
constexpr PlanTrackLayout plan_track_layout() { return {}; }

// What a plan tick takes from a bank beside the BankView: the completion buffers, the track tables and
// the track tick's state by address, and, of a fused exchange, the mailbox's table and sizes
// (capi_common.hpp plan_view builds one per tick, on the stack).
struct PlanView {
  BankView bank;
  int32_t* best_cand;  double* best_cost;            // [n]
  double* pv;  int64_t* pidx;  int32_t* pnf;         // [blocks]
  uint64_t* la_tag;  uint64_t* blk_tag;  uint64_t* wq;
  unsigned* tickets;
  double* xref_pm;                       // [n][H][2], reserved by the raceline tick
  const double* track;                   // cx | cy | tt, [3][tr_n]
  int32_t tr_n;
  double tr_L, tr_width;
  double* trk;  int32_t* trk_flags;  uint64_t* hp_tag;   // plan_track_layout
  uint64_t* const* px_box;               // the mailbox (null: none)
  int32_t px_G, px_rank;
  uint64_t px_bound;
};

// The host state a tick reads and, once its launch was enqueued, advances.
struct PlanTickState {
  int32_t count, slot, W;                // the window: rows filled, the row written next
  uint32_t seq, tseq;                    // the launch tag's sequence, the half-plane words'
  int32_t trk_cur;                       // the path copy that holds the newest path
  TrackPathState trk_path;
  int32_t trk_last_H;
  uint32_t px_seq;                       // the mailbox's sequence (ticks with px)
};
// A bank's (and, px not null, its mailbox's) state, and a prepared tick's next state applied to them.
// Templates only so that the host harness runs them on plain structs of the same field names.
template <class Bank, class Mailbox>
inline PlanTickState plan_tick_state(const Bank& b, const Mailbox* px) {
  return {b.count, b.slot, b.W, b.seq, b.tseq, b.trk_cur, b.trk_path, b.trk_last_H, px ? px->seq : 0};
}
template <class Bank, class Mailbox>
inline void plan_tick_commit(Bank& b, Mailbox* px, const PlanTickState& next) {
  b.count = next.count;
  b.slot = next.slot;
  b.seq = next.seq;
  b.tseq = next.tseq;
  b.trk_cur = next.trk_cur;
  b.trk_path = next.trk_path;
  b.trk_last_H = next.trk_last_H;
  if (px) px->seq = next.px_seq;
}

// A tick's launch arguments (lbl / lal / trk: only where lb / la / tt say so) and the state after it.
struct PlanPrep {
  bool lb, la, tt;
  LookbackLaunch lbl;
  LookaheadLaunch lal;
  FinalLaunch f;
  PlanTrack trk;
  PlanTickState next;
};

// One tick's arguments from the view, the state and what the caller asks for.  launch_plan sets the
// shape's own fields (f.nb_* / f.do_*, the look-back's R, the raceline's wcap).
inline PlanPrep plan_tick_prepare(const PlanView& v, const PlanTickState& st, const llampc_plan_in& in, const PlanTick& t) {
  const BankView& bv = v.bank;
  PlanPrep p{};
  p.lb = in.do_lookback != 0;
  p.la = in.do_lookahead != 0;
  p.tt = t.tt != nullptr;
  PlanTickState& nx = p.next = st;
  if (p.lb) {
    nx.count = std::min(st.count + 1, st.W);         // rt.py:354
    nx.slot = (st.slot + 1) % st.W;
  }
  const int32_t full = nx.count >= st.W;             // rt.py:357
  // polled completion whenever look-back blocks exist to host the poller (LLAMPC_NO_POLL=1:
  // the ticket + last-block path, for A/B runs)
  const int32_t poll = (p.lb && p.la && getenv("LLAMPC_NO_POLL") == nullptr) ? 1 : 0;
  if (poll) nx.seq = next_seq(st.seq);
  if (p.lb) {
    LookbackLaunch& l = p.lbl;
    bank_lookback(bv, l);
    l.slot = st.slot;
    l.x_prev = in.x_prev;
    l.u_prev = in.u_prev;
    l.x_now = in.x_now;
    l.Ts = in.Ts;
    l.full = full;
    l.K = in.K;
    l.nan_first = in.nan_policy == LLAMPC_NAN_FIRST;
    l.err_out = t.err;
    if (t.wmean) l.wm_buf = t.wmean;
    l.wm_keep = t.wmean != nullptr;                  // else only the R > 1 second pass reads it
  }
  if (p.la) {
    LookaheadLaunch& l = p.lal;
    bank_lookahead(bv, in.integrator, l);
    l.x0 = in.x_now;
    l.U = in.U;
    l.xref = in.xref;
    l.uprev = in.uprev;
    l.C = in.C;
    l.H = in.H;
    l.Ts = in.Ts;
    l.cost = make_cost(in.cost, in.Ts);
    l.cost_out = t.cost;
    l.best_cand = v.best_cand;
    l.best_cost = v.best_cost;
    l.pv = v.pv;
    l.pidx = v.pidx;
    l.pnf = v.pnf;
    l.xref_mode = in.xref_mode;
    if (in.xref_mode == LLAMPC_XREF_RACELINE) {
      l.rl = raceline_view(bv);          // wcap: set by launch_plan from the LDS it leaves
      l.xref_pm = v.xref_pm;
    }
    l.la_tag = v.la_tag;
    l.blk_tag = v.blk_tag;
    l.seq = nx.seq;
    l.poll = poll;
    l.wq = v.wq;
  }
  FinalLaunch& f = p.f;
  bank_final(bv, f);
  f.out = t.out;
  f.tickets = v.tickets;
  f.full = full;
  f.window_count = nx.count;
  f.K = p.lb ? in.K : 0;
  f.nan_first = in.nan_policy == LLAMPC_NAN_FIRST;
  f.C = p.la ? in.C : 1;
  f.current_model = in.current_model;
  f.best_cand = v.best_cand;
  f.best_cost = v.best_cost;
  f.pv = v.pv;
  f.pidx = v.pidx;
  f.pnf = v.pnf;
  f.la_tag = v.la_tag;
  f.blk_tag = v.blk_tag;
  f.seq = nx.seq;
  f.poll = poll ? (int32_t)poll_units(poll_bound_ticks(bv.n, in.C, in.H), INT32_MAX) : 0;
  f.host_tag = t.host_tag;
  f.host_seq = t.host_seq;
  if (t.px) {                            // fused peer exchange (llampc_plan_exchange)
    nx.px_seq = next_seq(st.px_seq);
    f.px_box = v.px_box;
    f.px_merged = t.px_merged;
    f.px_G = v.px_G;
    f.px_rank = v.px_rank;
    f.px_seq = nx.px_seq;
    f.px_bound = (uint32_t)poll_units(v.px_bound, UINT32_MAX);
  }
  f.wq = v.wq;
  // the track tick: the read copy is the one the launch before wrote (or llampc_bank_set_path), the
  // write copy the other; the half-plane words' own sequence
  if (t.tt) {
    constexpr PlanTrackLayout L = plan_track_layout();
    const size_t tn = (size_t)v.tr_n;
    const int rd = st.trk_cur, wr = rd ^ 1;
    PlanTrack& k = p.trk;
    nx.tseq = next_seq(st.tseq);
    nx.trk_cur = wr;
    k.trk = TrackK{v.track, v.track + tn, v.track + 2 * tn, v.tr_n, 0, v.tr_L};
    k.hw = v.tr_width / 2 - t.tt->margin;
    k.weight = t.tt->weight;
    k.hp_tag = v.hp_tag;
    k.path_rd = v.trk + L.path(rd);
    k.path_wr = v.trk + L.path(wr);
    k.valid_rd = v.trk_flags + L.valid(rd);
    k.valid_wr = v.trk_flags + L.valid(wr);
    k.cost_wr = v.trk + L.cost(wr);
    k.dbg = v.trk + L.rb_path;
    k.dbg_valid = v.trk_flags + L.flag_rb_valid;
    k.late = reinterpret_cast<uint32_t*>(v.trk_flags + L.flag_late);
    k.seq = nx.tseq;
    k.poll = (uint32_t)poll_units(poll_bound_ticks(bv.n, in.C, in.H), INT32_MAX);
    k.path_ok = track_path_offered(st.trk_path, in.H) ? 1 : 0;
  }
  nx.trk_path = track_path_next(st.trk_path, t.tt ? kPathTrackTick : kPathOtherLaunch, in.H);
  nx.trk_last_H = t.tt ? in.H : 0;
  return p;
}

// plan_shape of a look-ahead alone, for what no bank decides: of n models (they matter to the LPM
// only; a plan input's own questions take n = 1), with the inline pack or a corridor offered.
inline PlanShape lookahead_shape(int64_t n, bool la, int32_t C, int32_t H, int32_t integrator, int32_t xref_mode,
                                 int32_t share, bool pack, bool corridor, int32_t track_n = 0) {
  PlanShapeIn s{};
  s.n = n;
  s.la = la;
  s.C = C;
  s.H = H;
  s.integrator = integrator;
  s.xref_mode = xref_mode;
  s.share = share;
  s.pack = pack;
  s.corridor = corridor;
  s.track_n = track_n;
  return plan_shape(s, 0);
}

// ---- what the tick entries refuse before anything is enqueued ------------------------------------
// Each returns LLAMPC_OK, or the code with the message in buf.  The bank facts they are decided by:
struct PlanBankFacts {
  int64_t n;
  bool raceline;                         // llampc_bank_set_raceline was called
  int32_t tr_n;                          // 0: no track set
  double tr_width;
  bool async_pending;
};
#define LLAMPC_REFUSE(code, ...) return (std::snprintf(buf, nbuf, __VA_ARGS__), (code))

inline int plan_in_refused(const PlanBankFacts& b, const llampc_plan_in* in, char* buf, size_t nbuf) {
  if (!in) LLAMPC_REFUSE(LLAMPC_E_ARG, "plan input is NULL");
  if (in->do_lookback && (in->K < 1 || in->K > LLAMPC_KMAX))
    LLAMPC_REFUSE(LLAMPC_E_ARG, "K=%d outside [1, %d]", in->K, LLAMPC_KMAX);
  if (in->do_lookback && (!in->x_prev || !in->u_prev || !in->x_now))
    LLAMPC_REFUSE(LLAMPC_E_ARG, "look-back needs x_prev, u_prev and x_now");
  if (in->do_lookahead) {
    if (in->C < 1 || in->H < 1) LLAMPC_REFUSE(LLAMPC_E_ARG, "C=%d H=%d must be >= 1", in->C, in->H);
    if ((int64_t)in->C * in->H > (1 << 26)) LLAMPC_REFUSE(LLAMPC_E_ARG, "C*H too large");
    if (!in->x_now || !in->U || !in->xref || !in->uprev)
      LLAMPC_REFUSE(LLAMPC_E_ARG, "look-ahead needs x_now, U, xref and uprev");
    if (in->integrator < LLAMPC_RK4 || in->integrator > LLAMPC_RK6)
      LLAMPC_REFUSE(LLAMPC_E_ARG, "unknown integrator %d", in->integrator);
    if (in->xref_mode != LLAMPC_XREF_GIVEN && in->xref_mode != LLAMPC_XREF_RACELINE)
      LLAMPC_REFUSE(LLAMPC_E_ARG, "unknown xref_mode %d", in->xref_mode);
    if (in->xref_mode == LLAMPC_XREF_RACELINE && !b.raceline)
      LLAMPC_REFUSE(LLAMPC_E_STATE, "xref_mode RACELINE needs llampc_bank_set_raceline first");
    if ((b.n + 1) * (int64_t)in->C <= 0 || b.n > INT64_MAX / std::max(1, in->C) - 1)
      LLAMPC_REFUSE(LLAMPC_E_ARG, "n*C overflows");
  }
  if (!in->do_lookback && !in->do_lookahead) LLAMPC_REFUSE(LLAMPC_E_ARG, "nothing to do: look-back and look-ahead both off");
  if (!(in->Ts > 0) || !std::isfinite(in->Ts)) LLAMPC_REFUSE(LLAMPC_E_ARG, "Ts must be finite > 0");
  return LLAMPC_OK;
}

// A corridor tick (llampc_plan_corridor, llampc_lookahead_corridor): no look-ahead, RK6, the per-model
// raceline reference — plan_shape's refusals of the corridor's modes, in its words (the rest of the
// input is plan_in_refused's to judge).
inline int corridor_mode_refused(const llampc_plan_in* in, char* buf, size_t nbuf) {
  const char* why =
      lookahead_shape(1, in->do_lookahead != 0, in->C, in->H, in->integrator, in->xref_mode, 1, false, true).refuse;
  if (why == kNoCorridorLookahead || why == kNoCorridorRk6 || why == kNoCorridorRaceline) LLAMPC_REFUSE(LLAMPC_E_ARG, "%s", why);
  return LLAMPC_OK;
}

// A track tick (llampc_plan_track, llampc_plan_track_async): no track, an async tick outstanding
// (LLAMPC_E_STATE), then plan_shape's refusals of the track tick's modes, in its words, and a weight or
// margin track_tick_invalid names.
inline int track_tick_refused(const PlanBankFacts& b, const llampc_plan_in* in, const TrackTick& tt, char* buf, size_t nbuf) {
  if (!b.tr_n) LLAMPC_REFUSE(LLAMPC_E_STATE, "no track set: call llampc_bank_set_track first");
  if (b.async_pending) LLAMPC_REFUSE(LLAMPC_E_STATE, "an async tick is outstanding: call llampc_plan_wait");
  if (in) {
    const char* why = lookahead_shape(1, in->do_lookahead != 0, in->C, in->H, in->integrator, in->xref_mode, 1, false,
                                      false, b.tr_n).refuse;
    if (why == kNoTrackLookahead || why == kNoTrackRk6 || why == kNoTrackEuler || why == kNoTrackRaceline)
      LLAMPC_REFUSE(LLAMPC_E_ARG, "%s", why);
  }
  if (const char* why = track_tick_invalid(tt.weight, tt.margin, b.tr_width)) LLAMPC_REFUSE(LLAMPC_E_ARG, "track tick: %s", why);
  return LLAMPC_OK;
}

// A host-pointer tick entry's refusals up to the point where it disarms the bank, in the entry's one
// order: hp (llampc_plan_corridor) the corridor's modes first — LLAMPC_E_ARG whatever else the bank
// lacks; tt (the track entries) the track tick's, in their table's order; the plan input; the track
// tick's horizon; the corridor's rows and weight (H is valid by then).  An outstanding async tick is
// refused by the track tick's table here, by every other entry after the disarm.
inline int plan_entry_refused(const PlanBankFacts& b, const llampc_plan_in* in, const double* hp, double weight,
                              const TrackTick* tt, char* buf, size_t nbuf) {
  int rc;
  if (hp && in && (rc = corridor_mode_refused(in, buf, nbuf))) return rc;
  if (tt && (rc = track_tick_refused(b, in, *tt, buf, nbuf))) return rc;
  if ((rc = plan_in_refused(b, in, buf, nbuf))) return rc;
  if (tt && in->H > LLAMPC_HMAX) LLAMPC_REFUSE(LLAMPC_E_ARG, "H=%d above %d (the path state's horizon)", in->H, LLAMPC_HMAX);
  if (hp)
    if (const char* why = corridor_invalid(hp, in->H, weight)) LLAMPC_REFUSE(LLAMPC_E_ARG, "corridor: %s", why);
  return LLAMPC_OK;
}

// The launch shape of a controller tick (ctl.hip ctl_kernel<lpm, *>): the look-ahead's lanes per
// rollout, lane group, candidates per lane and models per block, whether its input terms are
// staged (s4: the staged layout fits the CU's 160 KiB and LLAMPC_CTL_NO_STAGE is off) and its
// variates pre-drawn (zfit), the look-back's models per lane and the block counts, with the
// launch's LDS bytes and the completing block's area offset.  The one statement of the rule: the
// launch (ctl_tick_prepare below) and llampc_ctl_variant both take it from here.
struct CtlShape {
  int lpm, G, cpl, mpb, s4, zfit, R, nb_lb, nb_la, nslots;
  size_t lds, poll_off;
  int nb_cor;                            // corridor blocks, between the look-back's and the look-ahead's
};
constexpr size_t kCtlLdsMax = 160 * 1024;
// cor_n > 0: a corridor tick (ctl_corr.hip ctl_kernel_corr) on a centre line of cor_n points — never
// staged (the corridor rollout is unstaged and unsplit), H corridor blocks, and the LDS the largest
// of the roles': the look-ahead layout with the half-planes behind it, a corridor block's tables.
inline CtlShape ctl_shape(int64_t n, int32_t C, int32_t H, int32_t K, int32_t rl_n, bool warm, bool do_lb,
                          bool no_stage, int px_G, int32_t cor_n = 0) {
  CtlShape s{};
  s.R = lookback_r(n, K);
  s.nb_lb = do_lb ? lookback_blocks_r(n, s.R) : 1;
  s.nslots = warm ? 1 : K + 1;
  s.G = lookahead_group(C);
  s.cpl = (C + s.G - 1) / s.G;
  s.lpm = 4 * s.G <= kBlock ? 4 : (2 * s.G <= kBlock ? 2 : 1);
  s.mpb = kBlock / (s.G * s.lpm);
  s.nb_la = (s.nslots + s.mpb - 1) / s.mpb;
  s.zfit = ctl_zfit(C, H) ? 1 : 0;
  if (cor_n > 0) {
    s.nb_cor = H;
    s.lds = ctl_lds_bytes(H, C, rl_n, s.nb_lb, K, &s.poll_off, false, px_G, 0, ctl_corr_extra(H),
                          ctl_corridor_block_lds(cor_n));
    return s;
  }
  // the look-ahead blocks stage every (candidate, step)'s input terms when they fit in LDS
  // (CtlLaunch.s4; LLAMPC_CTL_NO_STAGE=1 at create: never, for A/B runs)
  size_t poll_s4 = 0;
  const size_t lds_s4 = ctl_lds_bytes(H, C, rl_n, s.nb_lb, K, &poll_s4, true, px_G);
  s.s4 = (!no_stage && lds_s4 <= kCtlLdsMax) ? 1 : 0;
  if (s.s4) {
    s.lds = lds_s4;
    s.poll_off = poll_s4;
  } else {
    s.lds = ctl_lds_bytes(H, C, rl_n, s.nb_lb, K, &s.poll_off, false, px_G);
  }
  return s;
}

// ---- the controller tick (capi_ctl.hip llampc_ctl_tick_async, ctl_arm) ----------------------------
// The corridor tick's device state (ctl.hpp CtlCorridor), in the order it is allocated:
//   d_cor       path copy 0 | path copy 1 (each [2][kCtlPathStride]) | read-back copy 0 | read-back copy 1,
//               each path [2][kCtlPathStride] | hp [HMAX][6] | theta [HMAX] (kCtlCorDbgDoubles in all)
//   d_cor_flag  valid 0, valid 1 | the read-backs' valid 0, valid 1
//   d_hp_tag    [12 HMAX] tagged half-plane words
// The one statement of it: the allocation, the launch arguments and the read-back take it here.
struct CtlCorLayout {
  size_t row = kCtlPathStride;           // a path's x row, then its y row
  size_t path_doubles = 2 * row;         // one path copy
  size_t rb_doubles = kCtlCorDbgDoubles; // one read-back copy: the path rows at 0, then
  size_t rb_hp = path_doubles, rb_theta = rb_hp + 6 * LLAMPC_HMAX;
  size_t cor_doubles = 2 * path_doubles + 2 * rb_doubles;
  int flags = 4;
  size_t hp_tag_words = 12 * (size_t)LLAMPC_HMAX;
  constexpr size_t path(int r) const { return path_doubles * (size_t)r; }
  constexpr size_t rb(int r) const { return 2 * path_doubles + rb_doubles * (size_t)r; }
  constexpr int valid(int r) const { return r; }
  constexpr int rb_valid(int r) const { return 2 + r; }
};
constexpr CtlCorLayout ctl_cor_layout() { return {}; }

// An armed launch waits at most kArmBoundS for its doorbell; the host fires it only while it is
// younger than kArmFreshS (else cancels it and launches the tick normally), so the launch cannot
// expire between the host's check and its store short of a ~1 s stall of that thread.
constexpr double kArmBoundS = 2.0;
constexpr double kArmFreshS = 0.5;

// What a tick takes from the controller, its bank and its transport, by address and constant
// (capi_ctl.hpp ctl_view builds one per tick, on the stack).  mailbox false, xg_world 0, cor_w 0: no peer
// exchange, no gather transport, no corridor — their fields are then not read.
struct CtlView {
  BankView bank;
  const llampc_ctl_cfg* cfg;
  CtlState* st;
  llampc_ctl_out* out;                   // the device alias of the pinned record
  uint64_t* host_tag;
  uint64_t* sel_tag;  uint64_t* slot_tag;  unsigned* tickets;
  double* dbg;  double* znoise;  uint64_t* ztag;
  const double* pts;  const double* prefix;  int32_t np;
  const uint64_t* door;  uint64_t* door_dev;
  double* spec_val;  int64_t* spec_idx;  uint64_t* spec_tag;  uint64_t* spec_res;  uint64_t* xref_tag;
  int32_t spec_nb, spec_cap;
  bool no_spec, no_stage;
  int32_t cus, share;                    // the bank's CU count (0: unknown) and concurrency
  const double* rl_mus;                  // host: the raceline's mus [bank.rl_M]
  const double* gparams;  int64_t n_global;          // the replicated global table (sharded)
  bool mailbox;                          // the peer mailboxes: their table, world, rank and bound
  uint64_t* const* px_box;
  int32_t px_world, px_rank;
  uint64_t px_bound;
  int32_t xg_world, xg_rank;             // the gather transport and its two buffers
  uint64_t* xsend;  const uint64_t* xgath;
  const double* track;                   // cx | cy | tt, [3][tr_n]
  int32_t tr_n;
  double tr_L, tr_width;
  double cor_w, cor_margin;              // the corridor's weight (0: off) and margin
  double* cor;  int32_t* cor_flag;  uint64_t* hp_tag;   // ctl_cor_layout
  double* cor_cost;
};

// The host state a tick reads and, once its launch was enqueued (or its armed launch rung), advances.
struct CtlTickState {
  int64_t t;                             // the tick's number
  uint64_t hseq;                         // the completion tag's sequence
  uint32_t seq, door_ctr;                // the launch tag's, the doorbell's (an armed prepare spends one)
  int32_t hint_p0;                       // the state's projidx / mu-hat as the last record left them
  double hint_mu;
  bool cor_prev;                         // the last tick enqueued was a corridor tick
  int32_t cor_nslots;
  int32_t count, slot, W;                // the bank's window: rows filled, the row written next
  uint32_t px_seq;                       // the transport's sequence: the mailbox's, or the gather's
  bool px;                               // (a prepared next state) the tick exchanges: px_seq is committed
};
// A controller's, its bank's and (mb not null) its mailbox's state, and a prepared tick's next state
// applied to them — all but door_ctr, which ctl_arm stores before its launch call: the number is spent
// even if that call fails, and independently of the commit at the doorbell.  Templates only so that
// the host harness runs them on plain structs of the same field names.
template <class Ctl, class Bank, class Mailbox>
inline CtlTickState ctl_tick_state(const Ctl& c, const Bank& b, const Mailbox* mb) {
  return {c.t,      c.hseq,  c.seq, c.door_ctr, c.hint_p0, c.hint_mu, c.cor_prev, c.cor_nslots,
          b.count,  b.slot,  b.W,   mb ? mb->seq : c.xg_seq, false};
}
template <class Ctl, class Bank, class Mailbox>
inline void ctl_tick_commit(Ctl& c, Bank& b, Mailbox* mb, const CtlTickState& next) {
  c.t = next.t;
  c.hseq = next.hseq;
  c.seq = next.seq;
  c.cor_prev = next.cor_prev;
  c.cor_nslots = next.cor_nslots;
  b.count = next.count;
  b.slot = next.slot;
  if (next.px) {                         // committed after the launch was enqueued (next_seq)
    if (mb) mb->seq = next.px_seq;
    else c.xg_seq = next.px_seq;
  }
}

// A prepared tick: its launch (ctl_kernel_corr with `cor` if corr, else ctl_kernel) and the state after it.
struct CtlPrep {
  bool corr = false;
  CtlCorridor cor{};
  CtlLaunch L{};
  int lpm = 4;
  size_t lds = 0;
  CtlTickState next{};
};

// The speculative look-ahead's decision (CtlLaunch.n_spec): how many models an armed tick rolls out
// before its doorbell, 0 for none.  Armed ticks past the warm-up whose rollouts are one model per block
// in fused quads with diagonal Q / P (the spec blocks' layout), never with a gather transport; with the
// peer mailboxes the ranks' lists are exchanged too (ctl.hip ctl_spec_exchange), in the slot after the
// selection record's words, so they must fit there.  The armed footprint: every block of an armed
// launch holds a CU from the end of the tick before to its doorbell, and all launches of the banks
// ticked together (llampc_bank_set_concurrency) must be resident at once — the exchange's peers and the
// tick's own look-back wait on each other — so the spec blocks take what is left of the banks' share of
// the CUs (INTEGRATION.md "What armed launches cost").  lds / poll_off: the spec layout's, when > 0.
struct CtlSpecIn {
  bool armed, no_spec, warm, full, diag, mailbox;
  int32_t R, s4, lpm, cpl, G, C, H, K, rl_n;
  int32_t xg_world, px_G;
  int32_t nb_lb, nb_la, spec_nb, spec_cap;
  int32_t cus, share;
  int64_t n;                             // the models the look-ahead can name: n_global with a mailbox
};
inline int32_t ctl_spec_models(const CtlSpecIn& s, size_t* lds, size_t* poll_off) {
  const int cus = s.cus >= 1 ? s.cus : 256;
  const int room = cus / std::max(1, s.share) - (s.nb_lb + s.nb_la);
  const int ns = (int)std::min<int64_t>(std::min<int64_t>(s.spec_cap, room), s.n);
  const bool px_fits = !s.mailbox || (s.px_G && ctl_rec_words(s.K) + 4 * ns <= kRecWords);
  if (!(s.armed && !s.no_spec && !s.warm && s.full && s.R == 1 && s.s4 && s.lpm == 4 && s.cpl == 1 && s.G == s.C &&
        s.diag && !s.xg_world && px_fits && ns >= 4 && s.nb_lb <= s.spec_nb))
    return 0;
  size_t poll_sp = 0;
  const size_t lds_sp = ctl_lds_bytes(s.H, s.C, s.rl_n, s.nb_lb, s.K, &poll_sp, true, s.px_G, ns);
  if (lds_sp > 160 * 1024) return 0;
  *lds = lds_sp;
  *poll_off = poll_sp;
  return ns;
}

// The launch of tick st.t (x_t null: armed — the doorbell carries x_t) and the state after it, from the
// view and the host's copy of the state (after ctl_refresh).  It refuses, with the message in buf, a
// window that is not full after the warm-up and a launch above the CU's LDS.  An armed prepare takes
// the next doorbell number: P.next.door_ctr holds it whatever is returned (st's own if the window was
// refused), and ctl_arm stores it at once.
inline int ctl_tick_prepare(const CtlView& v, const CtlTickState& st, const double* x_t, CtlPrep& P, char* buf,
                            size_t nbuf) {
  const BankView& bv = v.bank;
  const llampc_ctl_cfg& k = *v.cfg;
  const int64_t t = st.t;
  const int32_t W = st.W;
  const bool do_lb = t >= 2;             // rt.py:347 (the transition idt -> idt+1 from idt >= 1)
  const bool warm = t <= W;              // rt.py:300-301
  int32_t count = st.count;
  if (do_lb) count = std::min(count + 1, W);
  const bool full = do_lb && count >= W;
  CtlTickState& nx = P.next = st;
  if (!warm && !full)
    LLAMPC_REFUSE(LLAMPC_E_STATE, "tick %lld: the look-back window is not full after the warm-up (was the bank reset?)",
                  (long long)t);
  CtlLaunch L{};
  const int R = lookback_r(bv.n, k.K);
  // look-back (rt.py:347-366 on the bank's ring)
  bank_lookback(bv, L.lb);
  L.lb.x_prev = v.st->x_prev;
  L.lb.u_prev = v.st->u_prev;
  L.lb.Ts = k.Ts;
  L.lb.full = full;
  L.lb.K = k.K;
  L.lb.nan_first = k.nan_policy == LLAMPC_NAN_FIRST;
  L.lb.R = R;
  L.lb.wm_keep = 0;
  // look-ahead constants (RK4 on the bank's vehicle, the NLP objective)
  bank_lookahead(bv, LLAMPC_RK4, L.la);
  L.la.C = k.C;
  L.la.H = k.H;
  L.la.Ts = k.Ts;
  L.la.cost = make_cost(k.cost, k.Ts);
  L.la.xref_mode = LLAMPC_XREF_GIVEN;
  L.la.rl = raceline_view(bv);
  L.la.rl.wcap = bv.rl_n - 1;
  // lb_final's view
  bank_final(bv, L.fin);
  L.fin.out = &v.out->plan;
  L.fin.do_lb = do_lb;
  L.fin.do_la = 1;
  L.fin.full = full;
  L.fin.window_count = do_lb ? count : st.count;
  L.fin.K = k.K;
  L.fin.nan_first = k.nan_policy == LLAMPC_NAN_FIRST;
  L.fin.nb_lb = do_lb ? lookback_blocks_r(bv.n, R) : 1;
  L.fin.C = k.C;
  // controller
  nx.t = t + 1;
  nx.hseq = st.hseq + 1;
  nx.seq = next_seq(st.seq);
  if (do_lb) {
    nx.count = count;
    nx.slot = (st.slot + 1) % W;
  }
  L.st = v.st;
  L.out = v.out;
  L.host_tag = v.host_tag;
  L.host_seq = nx.hseq;
  L.sel_tag = v.sel_tag;
  L.slot_tag = v.slot_tag;
  L.tickets = v.tickets;
  L.dbg = v.dbg;
  L.znoise = v.znoise;
  L.ztag = v.ztag;
  L.pts = v.pts;
  L.prefix = v.prefix;
  L.tick = (uint64_t)t;
  L.seed = k.seed;
  for (int j = 0; j < 6; ++j) {
    L.x_t[j] = x_t ? x_t[j] : 0.0;      // armed (x_t null): the doorbell carries it
    L.nominal[j] = k.nominal[j];
  }
  const double sqrt3 = std::sqrt(3.0);
  for (int j = 0; j < 2; ++j) {
    L.nscale[j] = sqrt3 * k.sigma[j];    // sqrt(3) sigma_j, one rounding (ctl.hpp ctl_cand_one)
    L.rate[j] = k.cost.rate_max[j] < 0 ? -1.0 : k.cost.rate_max[j] * k.Ts;
    L.umin[j] = k.cost.umin[j];
    L.umax[j] = k.cost.umax[j];
  }
  L.mu_fixed = 1.0;                      // ConstantSpeed's defaults (rt.py:282)
  L.scale_fixed = 1.0;
  L.v_factor = k.v_factor;
  L.mu_init = k.mu_init;
  L.seq = nx.seq;
  L.poll = (uint32_t)poll_units(poll_bound_ticks(bv.n, k.C, k.H), UINT32_MAX);
  L.np = v.np;
  L.lap_projidx = k.lap_projidx;
  L.do_lb = do_lb;
  L.warm = warm;
  L.use_mu = t > W + 1;                  // rt.py:278
  L.door_dev = v.door_dev;               // every launch: its x_t time (kCtlTimeWord)
  if (!x_t) {                            // armed: the launch reads projidx / mu-hat from the state
    L.door = v.door;
    nx.door_ctr = st.door_ctr == 0xFFFFFFFFu ? 1u : st.door_ctr + 1u;   // never reused, never 0
    L.door_seq = nx.door_ctr;
    L.door_bound = (uint32_t)(kArmBoundS * 1e8 / 65536.0) + 1;
  } else {                               // the last record's (ctl_refresh after a failed wait)
    L.p0_walk = st.hint_p0;
    L.br_walk = mu_bracket(v.rl_mus, bv.rl_M, L.use_mu ? st.hint_mu : L.mu_fixed);   // rt.py:278-282
  }
  L.full = full;
  L.S = k.S;
  L.K = k.K;
  // sharded: the exchange runs on every tick whose window is full (the same ticks on every
  // rank); the selection is global, the look-ahead reads the replicated global table
  L.sel_goff = bv.goff;
  if (v.mailbox || v.xg_world) {
    L.la.params = v.gparams;
    L.la.n = v.n_global;
    L.la.goff = 0;
    L.sel_goff = 0;
  }
  if (v.mailbox) {
    if (full) {
      nx.px = true;
      nx.px_seq = next_seq(st.px_seq);
      L.px_box = v.px_box;
      L.px_G = v.px_world;
      L.px_rank = v.px_rank;
      L.px_seq = nx.px_seq;
      L.px_bound = (uint32_t)poll_units(v.px_bound, UINT32_MAX);
      L.poll = std::max(L.poll, L.px_bound);   // the look-ahead blocks wait for the merged selection
    }
  } else if (v.xg_world && full) {       // gather transport: two launches (CtlLaunch.px_phase; ctl_gather_split)
    nx.px = true;
    nx.px_seq = next_seq(st.px_seq);
    L.px_G = v.xg_world;
    L.px_rank = v.xg_rank;
    L.px_seq = nx.px_seq;
    L.px_phase = 1;
    L.px_send = v.xsend;
    L.px_gath = v.xgath;
    L.px_bound = 16;                     // ~10 ms: the records are there when the launch starts
  }
  // the launch's shape (ctl_shape: the lane split, the staging, the block counts).  A corridor tick
  // (llampc_ctl_set_corridor, weight > 0): ctl_kernel_corr — never staged, H corridor blocks, no
  // speculative blocks (L.s4 = 0 rules them out)
  const bool corr = v.cor_w > 0;
  const CtlShape V = ctl_shape(bv.n, k.C, k.H, k.K, bv.rl_n, warm, do_lb, v.no_stage, L.px_G, corr ? v.tr_n : 0);
  L.nslots = V.nslots;
  L.G = V.G;
  L.cpl = V.cpl;
  L.mpb = V.mpb;
  L.nb_lb = V.nb_lb;
  L.nb_la = V.nb_la;
  L.s4 = V.s4;
  L.poll_off = V.poll_off;
  size_t lds = V.lds;
  if (lds > kCtlLdsMax) LLAMPC_REFUSE(LLAMPC_E_ARG, "controller tick needs %zu B of LDS (> 160 KiB)", lds);
  {
    const llampc_cost& cq = k.cost;
    CtlSpecIn s{};
    s.armed = !x_t, s.no_spec = v.no_spec, s.warm = warm, s.full = full, s.mailbox = v.mailbox;
    s.diag = cq.Q[1] == 0.0 && cq.Q[2] == 0.0 && cq.P[1] == 0.0 && cq.P[2] == 0.0;
    s.R = R, s.s4 = L.s4, s.lpm = V.lpm, s.cpl = L.cpl, s.G = L.G, s.C = k.C, s.H = k.H, s.K = k.K, s.rl_n = bv.rl_n;
    s.xg_world = v.xg_world, s.px_G = L.px_G;
    s.nb_lb = L.nb_lb, s.nb_la = L.nb_la, s.spec_nb = v.spec_nb, s.spec_cap = v.spec_cap;
    s.cus = v.cus, s.share = v.share;
    s.n = v.mailbox ? v.n_global : bv.n;
    if (const int32_t ns = ctl_spec_models(s, &lds, &L.poll_off)) {
      L.px_spec_off = ctl_rec_words(k.K);
      L.px_spec_wait = 20000;            // 200 us: the ranks arm within microseconds of each other
      L.n_spec = ns;
      L.spec_val = v.spec_val;
      L.spec_idx = v.spec_idx;
      L.spec_tag = v.spec_tag;
      L.spec_res = v.spec_res;
      L.xref_tag = v.xref_tag;
    }
  }
  lds = std::max<size_t>(lds, 82 * 1024); // one block per CU, as the plan launch (sc1 hand-offs)
  P.corr = corr;
  if (corr) {
    // the path state and the read-back by tick parity (ctl.hpp CtlCorridor): tick t reads what tick
    // t - 1 wrote and writes its own copy
    constexpr CtlCorLayout Y = ctl_cor_layout();
    CtlCorridor& q = P.cor;
    const size_t tn = (size_t)v.tr_n;
    const int wr = (int)(t & 1), rd = wr ^ 1;
    q = CtlCorridor{};
    q.trk = TrackK{v.track, v.track + tn, v.track + 2 * tn, v.tr_n, 0, v.tr_L};
    q.hw = v.tr_width / 2 - v.cor_margin;
    q.weight = v.cor_w;
    q.hp_tag = v.hp_tag;
    q.path_rd = v.cor + Y.path(rd);
    q.path_wr = v.cor + Y.path(wr);
    q.valid_rd = v.cor_flag + Y.valid(rd);
    q.valid_wr = v.cor_flag + Y.valid(wr);
    q.dbg = v.cor + Y.rb(wr);
    q.dbg_valid = v.cor_flag + Y.rb_valid(wr);
    q.path_ok = st.cor_prev ? 1 : 0;
    q.dbg_cost = v.cor_cost;
  }
  nx.cor_prev = corr;
  nx.cor_nslots = corr ? L.nslots : 0;
  P.L = L;
  P.lpm = V.lpm;
  P.lds = lds;
  return LLAMPC_OK;
}

// The gather transport's two launches from one prepared tick (CtlLaunch.px_phase 1): first the look-back
// blocks alone, which leave this shard's record; after the gather, block 0 merges and completes beside
// the look-ahead blocks.
inline void ctl_gather_split(const CtlPrep& P, CtlPrep& first, CtlPrep& second) {
  first = P;
  first.L.nb_la = 0;
  first.L.n_spec = 0;
  second = P;
  second.L.px_phase = 2;
  second.L.nb_lb = 1;
}

// Whether an armed launch is rung (else cancelled, and the tick launched normally): it is fresh, it was
// armed for this tick, and with the peer exchange its tick number is still the mailbox's next.
inline bool ctl_arm_fires(double age_s, int64_t arm_t, int64_t t, int32_t arm_px_G, bool has_mailbox, uint32_t arm_px_seq,
                          uint32_t mailbox_seq) {
  const bool px_ok = !arm_px_G || !has_mailbox || arm_px_seq == next_seq(mailbox_seq);
  return age_s < kArmFreshS && arm_t == t && px_ok;
}

// The doorbell's words (CtlLaunch.door): every word tagged door_seq in its high half — x_t as twelve
// 32-bit halves (high, low), then the status.  Block 0 polls until all carry the tag, so the stores need
// no order among themselves; the caller stores the last with release.
inline void ctl_door_words(const double* x_t, uint32_t door_seq, uint64_t w[kCtlDoorWords]) {
  const uint64_t tg = (uint64_t)door_seq << 32;
  for (int j = 0; j < 6; ++j) {
    uint64_t b;
    std::memcpy(&b, &x_t[j], 8);
    w[2 * j] = tg | (b >> 32);
    w[2 * j + 1] = tg | (b & 0xFFFFFFFFull);
  }
  w[kCtlDoorWords - 1] = tg | kCtlDoorFire;
}
inline uint64_t ctl_door_cancel_word(uint32_t door_seq) { return ((uint64_t)door_seq << 32) | kCtlDoorCancel; }

// ---- what the controller's entries refuse: LLAMPC_OK, or the code with the message in buf ---------
// llampc_ctl_create (the lock-free part): the pointers, the cfg, the polyline, the bank's raceline and
// the launch's LDS, in that order.
inline int ctl_create_refused(bool out_null, bool arg_null, const llampc_ctl_cfg* cfg, int32_t np, int64_t n,
                              bool raceline, int32_t rl_n, char* buf, size_t nbuf) {
  if (out_null) LLAMPC_REFUSE(LLAMPC_E_ARG, "out is NULL");
  if (arg_null || !cfg) LLAMPC_REFUSE(LLAMPC_E_ARG, "NULL argument");
  const llampc_ctl_cfg& k = *cfg;
  if (k.C < 1 || k.H < 1 || k.H > LLAMPC_HMAX || k.K < 1 || k.K > LLAMPC_KMAX)
    LLAMPC_REFUSE(LLAMPC_E_ARG, "C=%d H=%d (1..%d) K=%d (1..%d)", k.C, k.H, LLAMPC_HMAX, k.K, LLAMPC_KMAX);
  if (k.S < 1 || k.S > kCtlSMax) LLAMPC_REFUSE(LLAMPC_E_ARG, "S=%d outside [1, %d]", k.S, kCtlSMax);
  if (!(k.Ts > 0) || !std::isfinite(k.Ts)) LLAMPC_REFUSE(LLAMPC_E_ARG, "Ts must be finite > 0");
  if (np < 2) LLAMPC_REFUSE(LLAMPC_E_ARG, "np=%d < 2", np);
  if (k.nan_policy != LLAMPC_NAN_FIRST && k.nan_policy != LLAMPC_NAN_IGNORE) LLAMPC_REFUSE(LLAMPC_E_ARG, "nan_policy");
  if (!raceline) LLAMPC_REFUSE(LLAMPC_E_STATE, "the controller needs the bank's raceline (llampc_bank_set_raceline)");
  size_t poll_off = 0;
  const size_t lds = ctl_lds_bytes(k.H, k.C, rl_n, lookback_blocks_r(n, lookback_r(n, k.K)), k.K, &poll_off);
  if (lds > 160 * 1024)
    LLAMPC_REFUSE(LLAMPC_E_ARG, "controller tick needs %zu B of LDS (> 160 KiB): C*H=%d too large for this track", lds,
                  k.C * k.H);
  return LLAMPC_OK;
}

// llampc_ctl_set_corridor, after it cancelled an armed launch: the controller's state, then the weight
// and margin, then (weight > 0) a corridor tick's LDS on the bank's shape.
struct CtlCorridorFacts {
  bool pending, sharded, no_stage;
  int32_t tr_n;                          // 0: no track set
  double tr_width;
  int64_t n;
  int32_t C, H, K, rl_n;
};
inline int ctl_corridor_refused(const CtlCorridorFacts& f, double weight, double margin, char* buf, size_t nbuf) {
  if (f.pending) LLAMPC_REFUSE(LLAMPC_E_STATE, "a controller tick is outstanding");
  if (!f.tr_n) LLAMPC_REFUSE(LLAMPC_E_STATE, "no track set: call llampc_ctl_set_track first");
  if (f.sharded) LLAMPC_REFUSE(LLAMPC_E_STATE, "a sharded controller has no corridor ticks");
  if (!(weight >= 0) || !std::isfinite(weight)) LLAMPC_REFUSE(LLAMPC_E_ARG, "weight must be finite and >= 0");
  if (track_margin_refused(margin, f.tr_width, buf, nbuf)) return LLAMPC_E_ARG;
  if (weight > 0) {
    const CtlShape V = ctl_shape(f.n, f.C, f.H, f.K, f.rl_n, false, true, f.no_stage, 0, f.tr_n);
    if (V.lds > kCtlLdsMax) LLAMPC_REFUSE(LLAMPC_E_ARG, "a corridor tick needs %zu B of LDS (> 160 KiB)", V.lds);
  }
  return LLAMPC_OK;
}

// llampc_ctl_variant (track_n null) and llampc_ctl_variant_corridor: the shape of a tick past the
// warm-up (unsharded) into V, or why it has none.  C beyond kCtlVariantCMax: the candidates alone
// (16 B each per step) exceed the CU's LDS, and the int products C * H stay far from overflow.
constexpr int32_t kCtlVariantCMax = 1 << 16;
inline int ctl_variant_refused(bool out_null, int64_t n, int32_t C, int32_t H, int32_t K, int32_t rl_n,
                               const int32_t* track_n, bool no_stage, CtlShape& V, char* buf, size_t nbuf) {
  if (out_null) LLAMPC_REFUSE(LLAMPC_E_ARG, "NULL argument");
  const bool bad = n < 1 || C < 1 || C > kCtlVariantCMax || H < 1 || H > LLAMPC_HMAX || K < 1 || K > LLAMPC_KMAX || rl_n < 2;
  if (!track_n) {
    if (bad)
      LLAMPC_REFUSE(LLAMPC_E_ARG, "n=%lld C=%d (1..%d) H=%d (1..%d) K=%d (1..%d) rl_n=%d", (long long)n, C, kCtlVariantCMax,
                    H, LLAMPC_HMAX, K, LLAMPC_KMAX, rl_n);
    V = ctl_shape(n, C, H, K, rl_n, false, true, no_stage, 0);
    if (V.lds > kCtlLdsMax)              // llampc_ctl_create refuses the shape
      LLAMPC_REFUSE(LLAMPC_E_ARG, "controller tick needs %zu B of LDS (> 160 KiB): C*H=%d too large for this track", V.lds,
                    C * H);
    return LLAMPC_OK;
  }
  if (bad || *track_n < 2 || *track_n > kTrackMaxPoints)
    LLAMPC_REFUSE(LLAMPC_E_ARG, "n=%lld C=%d (1..%d) H=%d (1..%d) K=%d (1..%d) rl_n=%d track_n=%d (2..%d)", (long long)n, C,
                  kCtlVariantCMax, H, LLAMPC_HMAX, K, LLAMPC_KMAX, rl_n, *track_n, kTrackMaxPoints);
  V = ctl_shape(n, C, H, K, rl_n, false, true, false, 0, *track_n);
  if (V.lds > kCtlLdsMax) LLAMPC_REFUSE(LLAMPC_E_ARG, "a corridor tick needs %zu B of LDS (> 160 KiB)", V.lds);
  return LLAMPC_OK;
}
#undef LLAMPC_REFUSE

// Spins until *tag == want (acquire): 0.  A tag that `stop` accepts ends the spin with
// kSpinStopped.  After `bound`, on_timeout() runs once (it synchronises the stream, so a HIP
// error is the one reported: its non-zero return, an LLAMPC_E_* code, is passed on as it is); a
// tag still missing then gives kSpinTimeout.  Both outcomes are > 0, which no LLAMPC_* code is.
constexpr int kSpinStopped = 1, kSpinTimeout = 2;
template <class OnTimeout, class Stop = bool (*)(uint64_t)>
inline int spin_for_tag(const uint64_t* tag, uint64_t want, OnTimeout on_timeout,
                        Stop stop = [](uint64_t) { return false; },
                        std::chrono::nanoseconds bound = std::chrono::seconds(10)) {
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t spins = 0;
  uint64_t v;
  while ((v = __atomic_load_n(tag, __ATOMIC_ACQUIRE)) != want) {
    __builtin_ia32_pause();
    if (stop(v)) return kSpinStopped;
    if ((++spins & 0xFFF) == 0 && std::chrono::steady_clock::now() - t0 > bound) {
      if (int rc = on_timeout()) return rc;
      return __atomic_load_n(tag, __ATOMIC_ACQUIRE) == want ? 0 : kSpinTimeout;
    }
  }
  return 0;
}

// spin_for_tag for the B tags tag[p stride] of one launch under ONE bound: arrived[p] says whether
// tag p carries `want` (acquire).  After `bound`, on_timeout() runs once (its non-zero return is
// passed on) and the tags still missing are read one last time without waiting.
template <class OnTimeout>
inline int spin_for_tags(const uint64_t* tag, size_t stride, int32_t B, uint64_t want, bool* arrived,
                         OnTimeout on_timeout, std::chrono::nanoseconds bound = std::chrono::seconds(10)) {
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t spins = 0;
  bool expired = false;
  for (int32_t p = 0; p < B; ++p) {
    const uint64_t* t = tag + (size_t)p * stride;
    while (!(arrived[p] = __atomic_load_n(t, __ATOMIC_ACQUIRE) == want) && !expired) {
      __builtin_ia32_pause();
      if ((++spins & 0xFFF) == 0 && std::chrono::steady_clock::now() - t0 > bound) {
        if (int rc = on_timeout()) return rc;
        expired = true;
      }
    }
  }
  return 0;
}

}  // namespace
}  // namespace llampc

// nlp.hpp — the setupNLP.solve drop-in's launch interface (nlp.hip, nlp_batch.hip; llampc_nlp_* in
// capi_nlp.hip, llampc_nlp_batch_* in capi_nlp_batch.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctl.hpp"
#include "kernels.hpp"
#include "llampc.h"

namespace llampc {

// The solver's device state (one per solver handle): the sampling distribution of the
// current iteration and the best sequence so far.
struct NlpState {
  double mean[LLAMPC_HMAX][2];
  double std_[LLAMPC_HMAX][2];
  double best_u[LLAMPC_HMAX][2];
  double best_j;                 // +inf until a finite objective is seen
  int32_t best_it;
  int32_t best_s;                // the best sequence's sample index (in round best_it)
};

// A launch of CEM rounds [it, it + rounds): samples / 64 sample blocks, each of which also
// completes every round (nlp.hip).  Every round of the solve in one launch when the blocks are
// few enough to be co-resident (nlp_persistent), else one launch per round.  Blocks exchange a
// round by tagged words (tag nlp_seq(host_seq, round), so no drain, flag or ticket sits between
// a store and its reader): each block's sorted list (list_tag) to every block; across launches
// the next round's mean / std (ms_tag, block 0).  Scalars only (no arrays): the kernel never
// takes the address of its argument (which would copy it to scratch).
// The solve's result as the last round's completion writes it into pinned host memory (then
// a system-scope fence and the host tag): no D2H copy, no stream synchronisation.
struct NlpResult {
  double best_u[LLAMPC_HMAX][2];
  double traj[LLAMPC_HMAX + 1][6];     // xmpc: the NLP's Euler trajectory of best_u
  double best_j;
  int32_t best_it, pad;
};

struct NlpLaunch {
  LookaheadLaunch la;            // params [6][1], veh (NLP form), cost, H, Ts, integrator EULER_NLP
  NlpState* st;
  double* cand;                  // [2][samples][H][2] the round's sequences after the rate clip
                                 //   (by round parity: nlp.hip nlp_cand)
  NlpResult* res;                // the last round: the result, in pinned host memory (device alias)
  uint64_t* host_tag;            //   then this solve's number (host alias spun on by the caller)
  uint64_t host_seq;
  uint64_t* list_tag;            // [2][3][samples]: by round parity, each sample block's sorted
                                 //   list (samples / 64 x len entries) as tagged words: key high
                                 //   halves, key low halves, sample indices
  uint64_t* ms_tag;              // [2][4 H]: the mean [H][2] then std [H][2] of a launch's first
                                 //   round r >= 1, each double as tagged halves (low, high)
  uint64_t seed, call;           // Philox key; counter word 1 = the solve call number
  double up0, up1;               // uprev (du_0, nmpc.py:65-66)
  double umin0, umin1, umax0, umax1;
  double rlo0, rlo1, rhi0, rhi1; // per-step rate bounds (x Ts); lo > hi: none
  double std_floor;
  double sig0, sig1;             // the first round's std (llampc_nlp_cfg.sigma0)
  int32_t it, rounds, iters;     // the launch's first round, its round count, the solve's
  int32_t H, samples, elite, has_hold;
  int32_t ltraj;                 // the last round's sample rollouts keep their states in LDS and
                                 //   a best from that round is copied from there (else re-run)
};

// The solve's inputs in the kernarg segment (the plan kernel's InlinePack idea): x0 [6] | xref
// [2][H+1] | the first round's mean [H][2] — the launch carries them, so a solve needs no H2D
// copy (it cost ~8 us of a 212 us solve).  The state (best so far, NlpState) starts in registers.
constexpr int kNlpInlineDoubles = 6 + 2 * (LLAMPC_HMAX + 1) + 2 * LLAMPC_HMAX;
struct NlpInline {
  double v[kNlpInlineDoubles];
};

// every round in one launch: the sample blocks (one per CU: the LDS request) must all be
// resident at once, since each waits for the others' rounds
constexpr int kNlpPersistentBlocks = 64;
// the round tags' sequence: the solve's number x kNlpMaxIters + the round (llampc_nlp_create
// bounds iters by it), 32 bits — never a stale word's
constexpr int kNlpMaxIters = 1024;
__host__ __device__ __forceinline__ uint32_t nlp_seq(uint64_t host_seq, int it) {
  return (uint32_t)host_seq * (uint32_t)kNlpMaxIters + (uint32_t)it;
}
__host__ __device__ __forceinline__ bool nlp_persistent(int samples) { return samples / 64 <= kNlpPersistentBlocks; }

// the length of each sample block's sorted list: next power of two >= elite (elite <= 64)
__host__ __device__ __forceinline__ int nlp_list_len(int elite) {
  int l = 1;
  while (l < elite) l <<= 1;
  return l;
}
constexpr size_t kNlpLdsMax = 160 * 1024;   // a launch's LDS: the CU's
size_t nlp_lds_bytes(int H, int samples, int elite, bool ltraj = false);
bool nlp_ltraj_fits(int H, int samples, int elite);
hipError_t launch_nlp(const NlpLaunch& a, const NlpInline& pk, hipStream_t s);

// The corridor solve's own argument (llampc_nlp_solve_corridor): the unconstrained kernels'
// arguments stay as they are.  hp [H][6]: per step k = 1..H the half-planes (a0, a1, b, c0, c1, d),
// a.p_k <= b and c.p_k <= d on the position after k Euler steps (rollout_dev.hpp
// corridor_slack2); the device alias of the solver's pinned mapped buffer — 48 H bytes do not fit
// the kernarg segment beside NlpInline — which each block copies once per launch into its LDS
// (after the region nlp_traj_off starts, before the kept states).  weight: J + weight x pen.
struct NlpCorridor {
  const double* hp;
  double weight;
};
size_t nlp_corridor_lds_bytes(int H, int samples, int elite, bool ltraj = false);
bool nlp_corridor_ltraj_fits(int H, int samples, int elite);   // else the re-run trajectory
hipError_t launch_nlp_corridor(const NlpLaunch& a, const NlpInline& pk, const NlpCorridor& cor, hipStream_t s);

// The batched solve's own argument (llampc_nlp_batch_solve; nlp_batch.hip): B independent
// problems in one launch of B x nl blocks (nl = samples / 64, a power of two), block g being
// block g % nl of problem p = g / nl.  NlpLaunch carries problem 0's pointers and what the batch
// shares (the bank's params [6][n] and vehicle, the cost, the bounds, the shape, host_seq, call);
// problem p's words lie p strides on: st[p], res[p], host_tag[p tag_words], list_tag + p
// list_words, ms_tag + p ms_words, cand + p cand_doubles.  Its inputs are record p of `in` (the
// device alias of a pinned mapped buffer the host writes before the launch; B of them do not fit
// the kernarg segment), 64-bit words: x0 [6] | xref [2][H+1] | the first mean [H][2] (NlpInline's
// layout) | at up_off: uprev [2] | the Philox seed | model index (low half), has_hold (high).
// The strides and offsets are capi_host.hpp nlp_batch_layout's.
struct NlpBatch {
  const uint64_t* in;
  uint64_t cand_doubles;
  uint32_t rec_words, up_off, list_words, ms_words, tag_words;
  int32_t nl_log2;
};
static_assert(sizeof(NlpBatch) == 40 && alignof(NlpBatch) == 8, "NlpBatch layout (a kernel argument)");
// B x nl blocks, all co-resident (the caller has checked B nl against the CU count)
hipError_t launch_nlp_batch(const NlpLaunch& a, const NlpBatch& bt, int B, hipStream_t s);

// The batched corridor solve's own argument (llampc_nlp_batch_solve_corridor / _solve_track;
// nlp_batch_corr.hip): the batch's, unchanged, and the problems' corridors in a buffer of their own
// (the device alias of a pinned mapped buffer, as NlpCorridor.hp): problem p's half-planes hp [H][6]
// start at cor + p cor_doubles, its own weight is the double at w_off of its part (after the
// half-planes, then the device builder's theta: capi_host.hpp nlp_batch_cor_layout).  Each block
// copies its problem's half-planes once into its LDS and takes the weight, block-uniform, into
// scalar registers.
struct NlpBatchCorridor {
  NlpBatch bt;
  const double* cor;
  uint32_t cor_doubles, w_off;
};
static_assert(sizeof(NlpBatchCorridor) == 56 && alignof(NlpBatchCorridor) == 8, "NlpBatchCorridor layout (a kernel argument)");
// B x nl blocks, all co-resident, as launch_nlp_batch; LDS as the corridor solve's
hipError_t launch_nlp_batch_corridor(const NlpLaunch& a, const NlpBatchCorridor& bc, int B, hipStream_t s);

// The track corridor along B paths (track_corridor_batch_kernel, corridor_batch.hip): B x H blocks,
// block (p, k) writes row k - 1 of problem p's half-planes at cor + p cor_doubles and theta_k at
// theta_off of that part, along path + p path_doubles ([2][H+1]; the device alias of a pinned mapped
// buffer, as cor is).
hipError_t launch_track_corridor_batch(const TrackK& t, const double* path, uint32_t path_doubles, int32_t B, int32_t H,
                                       double hw, double* cor, uint32_t cor_doubles, uint32_t theta_off, hipStream_t s);

}  // namespace llampc

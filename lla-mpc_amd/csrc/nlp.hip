// nlp.hip — the setupNLP.solve drop-in (llampc_nlp_*, include/llampc.h): the selected model's
// NMPC (nmpc.py:14-203: Euler transcription of Dynamic.casadi, nmpc.py:58-60; the objective
// nmpc.py:44-111; input bounds and the steering-rate bound nmpc.py:102-105) solved on the
// device by the cross-entropy method — no IPOPT here (casadi is absent; its optimum is parity
// unpinned).  Every round in one launch (or one launch per round, nlp.hpp), then the Euler
// trajectory of the best sequence and the result into pinned host memory:
//
//   sample blocks   each draws 64 sequences from the round's (mean, std) — Philox noise
//                   (ctl.hpp), the bounds, the rate chain in order over the horizon; sample 0 is
//                   the mean itself, sample 1 of the first round holds uprev — and rolls them out
//                   (the plan kernel's rollout, NLP-Euler, four lanes per rollout, candidates in
//                   LDS), writing each sample's objective (+inf if infeasible).  Each block then
//                   sorts its 64 (objective, index) keys in one wave (a bitonic network of
//                   shuffle exchanges: NaN last, ties to the lower index) and publishes its best
//                   len = next_pow2(E) sorted, as tagged words;
//   every block     then completes the round itself (round 6; until then one completion block
//                   did and handed the next mean / std back through tagged words, ~1.5 us a
//                   round), in registers where it can (E <= 32, nlp_complete32): waves 0-3 each
//                   poll four blocks' lists straight into registers and merge them two levels
//                   in the wave — the lower len of two sorted lists is min(a_i, b_(len-1-i)),
//                   bitonic, then one half-cleaner network of lane exchanges per level — and
//                   hand wave 0 the result through LDS (a counter, no block barrier), which
//                   merges those the same way to the E best overall in order, loads the E elite
//                   sequences (32 loads in flight per lane) and sets the next mean / std as
//                   their mean / standard deviation (NumPy's axis-0 order).  Every block
//                   computes the same values in the same order, so all hold the same next
//                   distribution.  Block 0 keeps the state (the best sequence so far) and
//                   writes the result.  The lists and the sequences are double-buffered by
//                   round parity: a block can be a round ahead of another, never two.  The next
//                   round's Philox variates (they do not depend on the mean / std) are drawn by
//                   helper waves 5-7 while waves 0-3 complete the round.  (A bitonic sort
//                   of all samples in LDS took 36 us of the 62 us round: 55 barrier-separated
//                   passes; the barrier-separated merge tree of round 6's first version 2.5 us.)
//
// The corridor solve (llampc_nlp_solve_corridor) is the same kernel with one more argument
// (NlpCorridor): per-step position half-planes in LDS, their squared slacks added to every
// sample's objective in the rollout (rollout_dev.hpp kRCorr); nothing else of the search changes.
#include "dev_wave.hpp"
#include "nlp.hpp"
#include "rollout_dev.hpp"

namespace llampc {

#ifdef LLAMPC_STAMPS
// Diagnostic build only: s_memrealtime per block and phase of the last launch
// (tools/diag/nlp_phases.py): 0 round start, 10 mean / std in, 1 samples formed, 2 rate-clipped,
// 9 staged, 3 wave 0's rollouts done, 12 every wave's, 11 list published; the completion (wave
// 0): 4 its four lists in and merged, 13 every group in, 5 merged, 6 elite loads issued, 14 the
// elite mean, 8 next mean / std.
static __device__ unsigned long long g_nlp_ph[32][16];
#define NLP_STAMP(slot)                                                                               \
  do {                                                                                                \
    if (threadIdx.x == 0 && blockIdx.x < 32) g_nlp_ph[blockIdx.x][slot] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
extern "C" int llampc_debug_nlp_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nlp_ph), sizeof(g_nlp_ph)) == hipSuccess ? 0 : -2;
}
#endif

namespace {
// nlp_dev.hpp's hooks: one problem per launch, the grid's blocks are the problem's and the solver's
// bank holds the one model
__device__ __forceinline__ int nlp_blk(const NlpLaunch&) { return (int)blockIdx.x; }
__device__ __forceinline__ Tire nlp_tire(const NlpLaunch& a) { return load_tire(a.la.params, 1, 0); }
}  // namespace

}  // namespace llampc

#include "nlp_dev.hpp"

namespace llampc {

size_t nlp_lds_bytes(int H, int samples, int elite, bool ltraj) {
  return nlp_traj_off(H, samples / 64, elite) + (ltraj ? 48 * 64 * (size_t)H : 0);
}
bool nlp_ltraj_fits(int H, int samples, int elite) {
  return H <= kNlpStageH && nlp_lds_bytes(H, samples, elite, true) <= kNlpLdsMax;
}

hipError_t launch_nlp(const NlpLaunch& a, const NlpInline& pk, hipStream_t s) {
  const size_t lds = std::max<size_t>(nlp_lds_bytes(a.H, a.samples, a.elite, a.ltraj != 0), 82 * 1024);
  const dim3 grid(a.samples / 64);      // the sample blocks (each completes every round)
  if (a.H <= kNlpStageH) {
    allow_lds(nlp_kernel<true, 2 * kBlock>);
    hipLaunchKernelGGL((nlp_kernel<true, 2 * kBlock>), grid, dim3(2 * kBlock), lds, s, a, pk);
  } else {
    allow_lds(nlp_kernel<false, kBlock>);
    hipLaunchKernelGGL((nlp_kernel<false, kBlock>), grid, dim3(kBlock), lds, s, a, pk);
  }
  return hipGetLastError();
}

// The corridor solve sizes its own LDS: the unconstrained layout with the half-planes [H][6]
// before the kept states, which it drops (the re-run trajectory) when they no longer fit.
size_t nlp_corridor_lds_bytes(int H, int samples, int elite, bool ltraj) {
  return nlp_lds_bytes(H, samples, elite, ltraj) + 48 * (size_t)H;
}
bool nlp_corridor_ltraj_fits(int H, int samples, int elite) {
  return H <= kNlpStageH && nlp_corridor_lds_bytes(H, samples, elite, true) <= kNlpLdsMax;
}

hipError_t launch_nlp_corridor(const NlpLaunch& a, const NlpInline& pk, const NlpCorridor& cor, hipStream_t s) {
  const size_t lds = std::max<size_t>(nlp_corridor_lds_bytes(a.H, a.samples, a.elite, a.ltraj != 0), 82 * 1024);
  const dim3 grid(a.samples / 64);      // as launch_nlp
  if (a.H <= kNlpStageH) {
    allow_lds(nlp_kernel<true, 2 * kBlock, NlpCorridor>);
    hipLaunchKernelGGL((nlp_kernel<true, 2 * kBlock, NlpCorridor>), grid, dim3(2 * kBlock), lds, s, a, pk, cor);
  } else {
    allow_lds(nlp_kernel<false, kBlock, NlpCorridor>);
    hipLaunchKernelGGL((nlp_kernel<false, kBlock, NlpCorridor>), grid, dim3(kBlock), lds, s, a, pk, cor);
  }
  return hipGetLastError();
}

}  // namespace llampc
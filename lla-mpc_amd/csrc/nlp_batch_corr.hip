// nlp_batch_corr.hip — the batched search with a soft track corridor per problem
// (llampc_nlp_batch_solve_corridor, llampc_nlp_batch_solve_track; include/llampc.h): nlp_batch.hip's
// launch of B x nl blocks, every problem with its OWN half-planes hp [H][6] and its OWN weight.
// A translation unit of its own, as plan_corr_*.hip and ctl_corr.hip are: the unconstrained batch's
// and the single solver's code objects stay what they were.
//
// The kernel is nlp_dev.hpp's nlp_kernel with Ext = NlpBatchCorridor, for which both COR and BATCH
// hold: a block takes its problem's words and record as the batch's blocks do, and its problem's
// corridor from the corridor buffer (nlp.hpp NlpBatchCorridor: a pinned mapped buffer the host
// writes, or track_corridor_batch_kernel ahead of this launch on the same stream) — the half-planes
// once into LDS at nlp_traj_off, the loads in flight while the first variates are drawn; the weight,
// block-uniform, into scalar registers.  From there on it is the single corridor solve's text: the
// rollouts' objective with the corridor term (rollout_dev.hpp kRCorr), the kept states after the
// half-planes.  A problem reads no other problem's corridor, so its result is that of the single
// corridor solve on that bank column with that seed, half-planes and weight.  The blocks of a
// problem wait for each other only on nlp_dev.hpp's bounded polls (kNlpRoundWait).
#include "dev_wave.hpp"
#include "nlp.hpp"
#include "rollout_dev.hpp"

namespace llampc {
namespace {
// nlp_dev.hpp's hooks, as nlp_batch.hip's
__device__ __forceinline__ int nlp_blk(const NlpLaunch& a) { return (int)blockIdx.x & (a.samples / 64 - 1); }
__device__ __forceinline__ Tire nlp_tire(const NlpLaunch& a) { return load_tire(a.la.params, a.la.n, a.la.goff); }
}  // namespace
}  // namespace llampc

#include "nlp_dev.hpp"

namespace llampc {

hipError_t launch_nlp_batch_corridor(const NlpLaunch& a, const NlpBatchCorridor& bc, int B, hipStream_t s) {
  const size_t lds = std::max<size_t>(nlp_corridor_lds_bytes(a.H, a.samples, a.elite, a.ltraj != 0), 82 * 1024);
  const dim3 grid((unsigned)B * (unsigned)(a.samples / 64));
  const NlpInline none{};               // the single solve's inputs: unused (the problems' records)
  if (a.H <= kNlpStageH) {
    allow_lds(nlp_kernel<true, 2 * kBlock, NlpBatchCorridor>);
    hipLaunchKernelGGL((nlp_kernel<true, 2 * kBlock, NlpBatchCorridor>), grid, dim3(2 * kBlock), lds, s, a, none, bc);
  } else {
    allow_lds(nlp_kernel<false, kBlock, NlpBatchCorridor>);
    hipLaunchKernelGGL((nlp_kernel<false, kBlock, NlpBatchCorridor>), grid, dim3(kBlock), lds, s, a, none, bc);
  }
  return hipGetLastError();
}

}  // namespace llampc

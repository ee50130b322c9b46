// nlp_batch.hip — the batched instantiation of the cross-entropy NMPC search (llampc_nlp_batch_*,
// include/llampc.h): B independent problems in ONE launch, each on its own nl = samples / 64
// blocks, each with its own bank model (by index into the bank's [6][n] table), state, reference,
// previous input, warm start and Philox seed (nlp.hpp NlpBatch).  The reference builds one
// setupNLP per bank model and solves with the selected one (rt.py:195-202, 305); a single solve
// fills nl of the chip's CUs, so the problems of a tick (the selected model's and the top-K's, or
// two tracks') run side by side instead of in series.
//
// The kernel is nlp.hip's (nlp_dev.hpp nlp_kernel, Ext = NlpBatch): a block takes its problem's
// words and inputs at entry and then runs the single solve's rounds as block g % nl of nl.  A
// problem reads no other problem's words, so the arithmetic, and with it every result bit, is
// that of the single solver created on that bank column with that seed.  The blocks of one
// problem wait for each other's rounds (bounded: kNlpRoundWait, then the block's verdict ends
// it), so all B x nl blocks must be resident at once: the host refuses a launch beyond the CU
// count.  A problem that times out leaves its host tag unwritten and stops no other problem.
#include "dev_wave.hpp"
#include "nlp.hpp"
#include "rollout_dev.hpp"

namespace llampc {
namespace {
// nlp_dev.hpp's hooks: the block within its problem's group of nl (a power of two), and the
// problem's column of the bank's table (la.n models; la.goff: the model index nlp_kernel took
// from the problem's record)
__device__ __forceinline__ int nlp_blk(const NlpLaunch& a) { return (int)blockIdx.x & (a.samples / 64 - 1); }
__device__ __forceinline__ Tire nlp_tire(const NlpLaunch& a) { return load_tire(a.la.params, a.la.n, a.la.goff); }
}  // namespace
}  // namespace llampc

#include "nlp_dev.hpp"

namespace llampc {

hipError_t launch_nlp_batch(const NlpLaunch& a, const NlpBatch& bt, int B, hipStream_t s) {
  const size_t lds = std::max<size_t>(nlp_lds_bytes(a.H, a.samples, a.elite, a.ltraj != 0), 82 * 1024);
  const dim3 grid((unsigned)B * (unsigned)(a.samples / 64));
  const NlpInline none{};               // the single solve's inputs: unused (the problems' records)
  if (a.H <= kNlpStageH) {
    allow_lds(nlp_kernel<true, 2 * kBlock, NlpBatch>);
    hipLaunchKernelGGL((nlp_kernel<true, 2 * kBlock, NlpBatch>), grid, dim3(2 * kBlock), lds, s, a, none, bt);
  } else {
    allow_lds(nlp_kernel<false, kBlock, NlpBatch>);
    hipLaunchKernelGGL((nlp_kernel<false, kBlock, NlpBatch>), grid, dim3(kBlock), lds, s, a, none, bt);
  }
  return hipGetLastError();
}

}  // namespace llampc

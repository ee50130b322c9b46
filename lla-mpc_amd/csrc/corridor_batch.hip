// corridor_batch.hip — the track corridor along B paths in one launch (track_corridor_batch_kernel;
// llampc_nlp_batch_track_corridor and, ahead of the batched corridor search on the same stream,
// llampc_nlp_batch_solve_track).  A grid of B x H blocks: block (p, k) builds row k - 1 of problem
// p's half-planes hp [H][6], and theta_k, at the point k of problem p's path [2][H+1].  The block
// is corridor_block() (corridor_block_dev.hpp), the controller's corridor blocks' too: tables to
// LDS, the nearest-segment scan over the block, the three look-ups in lanes 0-2.  The paths are
// read from a pinned mapped buffer (B of them do not fit the kernarg segment); the rows go into
// the batched solver's corridor buffer (nlp.hpp NlpBatchCorridor), pinned and mapped as well, with
// plain vector stores and a system-scope fence before the kernel ends.  No block waits on anything.
// A translation unit of its own: kernels.hip, and track_corridor_kernel in it, keep their code
// object.
#include "corridor_block_dev.hpp"
#include "dev_wave.hpp"
#include "nlp.hpp"

namespace llampc {

__global__ __launch_bounds__(kBlock) void track_corridor_batch_kernel(TrackK g, const double* path, uint32_t path_doubles,
                                                                      int32_t H, double hw, double* cor,
                                                                      uint32_t cor_doubles, uint32_t theta_off) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const unsigned p = blockIdx.x / (unsigned)H;
  const int k = (int)(blockIdx.x - p * (unsigned)H) + 1;
  const double* pp = path + (size_t)p * path_doubles;
  const double px = pp[k], py = pp[H + 1 + k];
  double* part = cor + (size_t)p * cor_doubles;
  auto emit = [&](const double* row, double theta) {   // thread 0
    double* out = part + 6 * (size_t)(k - 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = row[i];
    part[theta_off + (k - 1)] = theta;
    __threadfence_system();
  };
  corridor_block(g, smem, px, py, hw, emit);
}

hipError_t launch_track_corridor_batch(const TrackK& t, const double* path, uint32_t path_doubles, int32_t B, int32_t H,
                                       double hw, double* cor, uint32_t cor_doubles, uint32_t theta_off, hipStream_t s) {
  if (B < 1 || H < 1 || H > LLAMPC_HMAX || t.n < 2 || t.n > kTrackMaxPoints || !t.cx || !t.cy || !t.tt || !path || !cor ||
      path_doubles < 2 * (uint32_t)(H + 1) || theta_off < 6 * (uint32_t)H || cor_doubles < theta_off + (uint32_t)H)
    return hipErrorInvalidValue;
  allow_lds(track_corridor_batch_kernel);   // 96 KB of tables at the largest centre line
  hipLaunchKernelGGL(track_corridor_batch_kernel, dim3((unsigned)B * (unsigned)H), dim3(kBlock),
                     ctl_corridor_block_lds(t.n), s, t, path, path_doubles, H, hw, cor, cor_doubles, theta_off);
  return hipGetLastError();
}

}  // namespace llampc

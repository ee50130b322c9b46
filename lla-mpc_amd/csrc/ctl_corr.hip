// ctl_corr.hip — the controller tick with the soft track corridor (llampc_ctl_set_corridor; ctl.hpp
// CtlCorridor): ctl_kernel's launch plus H corridor blocks, still one launch per tick, unsharded only.
// Roles by block index:
//
//   look-back blocks [0, nb_lb)          as ctl_kernel's (ctl_back_dev.hpp): the look-back, the
//                                        published selection, the tick's completion
//   corridor blocks  [nb_lb, nb_lb + H)  block k = 1..H: the track's half-planes at path point P_k
//                                        (track_corridor_kernel's block, corridor_block_dev.hpp: tables
//                                        to LDS, split scan, record), published as the tagged
//                                        words hp_tag[12 (k - 1) ..]; with no valid path the disabled
//                                        row.  P = the previous tick's chosen rollout shifted one step
//                                        (ctl_path_index): state the PREVIOUS launch wrote
//   look-ahead blocks after those        ctl_lookahead<LPM, true>: the reference, the candidates, then
//                                        the wait for the selection AND the 12 H half-plane words, the
//                                        unsplit rollouts with the corridor term, and in the selection
//                                        slot's block the path state for the next tick
//
// Waiting (ctl.hip's rule, whole): a corridor block waits for nothing — not the doorbell, not another
// block — so on an armed launch it runs during the prologue and leaves.  A look-ahead block waits
// for the look-back ticket winner (index < nb_lb) and for the corridor blocks (indices < its own);
// neither ever waits on a look-ahead block before it publishes.  The completion waits only for
// look-ahead blocks, which then never wait again.  Workgroups are dispatched in index order, so
// whatever a block waits for has been dispatched; every wait is bounded by the launch's poll bound
// (LLAMPC_STATUS_POLL_TIMEOUT, never expected).  No speculative blocks (the deferred cost holds one
// position component per lane), no staged input terms, no split quad.
#include "corridor_block_dev.hpp"
#include "cs_dev.hpp"
#include "ctl.hpp"
#include "ctl_back_dev.hpp"
#include "ctl_lds.hpp"
#include "ctl_lookahead_dev.hpp"
#include "dev_wave.hpp"
#include "rollout_dev.hpp"

namespace llampc {

// Corridor block k (1..H).  `valid` is launch-uniform: the host's half (the tick before was a
// corridor tick) and the flag its selection block stored with the path.
__device__ __forceinline__ void ctl_corridor_block(const CtlLaunch& c, const CtlCorridor& k, int kk,
                                                   unsigned char* smem) {
  const int H = c.la.H;
  const bool valid = k.path_ok != 0 && *k.valid_rd != 0;
  const double nan = __builtin_nan("");
  double px = nan, py = nan, p0x = nan, p0y = nan;
  if (valid) {
    const int j = ctl_path_index(kk, H);
    px = k.path_rd[j];
    py = k.path_rd[kCtlPathStride + j];
    if (kk == 1) {                      // P_0, which no row reads: for the read-back alone
      p0x = k.path_rd[ctl_path_index(0, H)];
      p0y = k.path_rd[kCtlPathStride + ctl_path_index(0, H)];
    }
  }
  auto emit = [&](const double* row, double theta) {   // thread 0
    uint64_t* w = k.hp_tag + 12 * (size_t)(kk - 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const uint64_t b = (uint64_t)__double_as_longlong(row[i]);
      st_wt(&w[2 * i], tag_word(c.seq, (uint32_t)(b >> 32)));
      st_wt(&w[2 * i + 1], tag_word(c.seq, (uint32_t)b));
    }
    // the read-back (llampc_ctl_corridor): plain stores, read after the stream has drained
    double* d = k.dbg;
    d[kk] = px;
    d[kCtlPathStride + kk] = py;
    if (kk == 1) {
      d[0] = p0x;
      d[kCtlPathStride] = p0y;
      *k.dbg_valid = valid;
    }
    double* dh = d + 2 * kCtlPathStride + 6 * (size_t)(kk - 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) dh[i] = row[i];
    d[2 * kCtlPathStride + 6 * LLAMPC_HMAX + (kk - 1)] = theta;
  };
  if (valid) {
    corridor_block(k.trk, smem, px, py, k.hw, emit);
  } else if (threadIdx.x == 0) {
    const double inf = __builtin_inf();
    const double row[6] = {0.0, 0.0, inf, 0.0, 0.0, inf};   // constraints.disabled's row
    emit(row, nan);
  }
}

constexpr size_t kCtlCorArgOff = (sizeof(CtlLaunch) + alignof(CtlCorridor) - 1) & ~(alignof(CtlCorridor) - 1);

template <int LPM>
__global__ __launch_bounds__(kBlock) void ctl_kernel_corr(CtlLaunch arg, CtlCorridor cor) {
  // both arguments read in place from the kernarg segment (ctl_kernel's reason)
  (void)arg;
  (void)cor;
  const unsigned char* kp = (const unsigned char*)__builtin_amdgcn_kernarg_segment_ptr();
  const CtlLaunch& c = *(const CtlLaunch*)kp;
  const CtlCorridor& k = *(const CtlCorridor*)(kp + kCtlCorArgOff);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Scratch sc(smem);
  int* flag = reinterpret_cast<int*>(smem + kFlagOff);
  const int blk = (int)blockIdx.x;
  if (blk == 0 && threadIdx.x == 0 && !c.door)
    st_wt(&c.door_dev[kCtlTimeWord], (uint64_t)__builtin_amdgcn_s_memrealtime());
  const int H = c.la.H;
  if (blk >= c.nb_lb + H) {
    ctl_lookahead<LPM, true>(c, blk - c.nb_lb - H, smem, sc, &k);
    return;
  }
  if (blk >= c.nb_lb) {
    ctl_corridor_block(c, k, blk - c.nb_lb + 1, smem);
    return;
  }
  ctl_lookback_role(c, blk, smem, sc, flag);
}

hipError_t launch_ctl_corr(const CtlLaunch& c, const CtlCorridor& cor, int lpm, size_t lds, hipStream_t s) {
  const dim3 grid(c.nb_lb + c.la.H + c.nb_la), block(kBlock);
  if (lpm == 4) {
    allow_lds(ctl_kernel_corr<4>);
    hipLaunchKernelGGL((ctl_kernel_corr<4>), grid, block, lds, s, c, cor);
  } else if (lpm == 2) {
    allow_lds(ctl_kernel_corr<2>);
    hipLaunchKernelGGL((ctl_kernel_corr<2>), grid, block, lds, s, c, cor);
  } else {
    allow_lds(ctl_kernel_corr<1>);
    hipLaunchKernelGGL((ctl_kernel_corr<1>), grid, block, lds, s, c, cor);
  }
  return hipGetLastError();
}

}  // namespace llampc

// plan_dev.hpp — the plan launch: the tick's block roles (plan_body), the plan kernels and their
// host launchers, over the device code of the role headers below.  The plan-kernel
// instantiations are spread over plan_*.hip (one TU per integrator / lanes-per-rollout group,
// compiled in parallel); kernels.hip holds the dispatcher and the other kernels.
#pragma once
#include "final_dev.hpp"
#include "lookahead_dev.hpp"
#include "lookback_dev.hpp"
#include "peer_dev.hpp"

namespace llampc {

// ------------------------------------------------------------------------------------
// The tick: ONE launch.  Blocks [0, nb_lb) run the look-back, blocks [nb_lb, nb_lb+nb_la)
// the look-ahead (the halves are independent: x_{t-1} -> x_t vs. rollouts from x_t).
// Look-back blocks come first in dispatch order; the last of them merges the look-back
// (lb_final) while look-ahead blocks still run; the last block overall completes the
// llampc_plan_out record (final_select).
// ------------------------------------------------------------------------------------
template <int INTEG, bool STAGE, int LPM, int XM, bool PX = false, int WQ = 0, bool CORR = false>
__device__ __forceinline__ void plan_body(const LookbackLaunch& lb, const LookaheadLaunch& la,
                                          const FinalLaunch& fin, int G, int cpl,
                                          const double* hp = nullptr, double cw = 0.0) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Scratch sc(smem);
  int* flag = reinterpret_cast<int*>(smem + kFlagOff);
  // WQ launches run kBlockWQ threads per block: every role but the work-queue look-ahead is
  // written for kBlock and its surplus waves leave at once (s_barrier waits for the waves
  // that have not ended)
  // block roles: look-back blocks first in the grid (dispatch order; the look-ahead blocks
  // first measured 26.82-26.92 -> 27.67-27.75 us per tick)
  const bool is_lb = (int)blockIdx.x < fin.nb_lb;
  const int lb_blk = (int)blockIdx.x, la_blk = (int)blockIdx.x - fin.nb_lb;
  if constexpr (wq_threads(WQ) > kBlock) {
    if (is_lb && threadIdx.x >= kBlock) return;
  }
  if (is_lb) {
    lookback_block(lb, lb_blk, sc);
    if (!ticket_last(&fin.tickets[0], (unsigned)fin.nb_lb, flag)) return;
    if (fin.full) {
      lb_final(fin, smem);
      // host completion: lb_final's record stores are performed before any later hand-off
      // (the final block, possibly another one, publishes the host tag after them)
      if (fin.host_tag) __threadfence_system();
    }
    if (fin.poll) {                   // the look-back winner completes the tick
      __syncthreads();
      final_poll(fin, sc);
      if constexpr (PX) peer_finish(fin, smem);
      return;
    }
  } else {
    if constexpr (CORR) lookahead_block<INTEG, STAGE, LPM, XM, WQ, true>(la, la_blk, G, cpl, smem, sc, hp, cw);
    else lookahead_block<INTEG, STAGE, LPM, XM, WQ>(la, la_blk, G, cpl, smem, sc);
    if (fin.poll) return;                // published tagged records; no ticket
    if constexpr (wq_threads(WQ) > kBlock) {
      if (threadIdx.x >= kBlock) return;
    }
  }
  const unsigned expected = (unsigned)fin.nb_la + (fin.nb_lb > 0 ? 1u : 0u);
  if (!ticket_last(&fin.tickets[1], expected, flag)) return;
  final_select(fin, sc);
  if constexpr (PX) peer_finish(fin, smem);
}

// The plan kernels' arguments ahead of the inline pack: three launch structs and (G, cpl), each
// a multiple of its successor's alignment, so they lie back to back from the segment's start.
constexpr int kArgLa = sizeof(LookbackLaunch), kArgFin = kArgLa + sizeof(LookaheadLaunch);
constexpr int kArgG = kArgFin + sizeof(FinalLaunch), kPlanArgBytes = kArgG + 2 * sizeof(int);
static_assert(sizeof(LookbackLaunch) % 8 == 0 && sizeof(LookaheadLaunch) % 8 == 0 && sizeof(FinalLaunch) % 8 == 0,
              "plan kernel arguments: no padding between the launch structs");

// PX: the sharded tick's fused peer exchange (a separate instantiation, so the plain tick's
// code is unchanged: inlining it into every variant cost the headline tick 0.5 us)
// The shared-xref variants read their arguments behind touch_kernargs (dev_wave.hpp), through
// the pointer it returns; the by-value parameters only give the segment its layout.  The
// raceline variants keep the by-value reads (the touch ahead of those cost their unstaged
// instantiation 36 bytes of scratch per lane), and so does the work-queue layout (its tick
// was slower with the touch and the batched prologue, lookahead_dev.hpp kBatch).
template <int INTEG, bool STAGE, int LPM, int XM, bool PX = false, int WQ = 0>
__global__ __launch_bounds__(wq_threads(WQ)) void plan_kernel(LookbackLaunch lb, LookaheadLaunch la,
                                                      FinalLaunch fin, int G, int cpl) {
  if constexpr (XM || WQ) {
    plan_body<INTEG, STAGE, LPM, XM, PX, WQ>(lb, la, fin, G, cpl);
  } else {
    const KernargPtr kp = touch_kernargs<kPlanArgBytes>();
    plan_body<INTEG, STAGE, LPM, XM, PX, WQ>(kernarg_at<LookbackLaunch>(kp, 0), kernarg_at<LookaheadLaunch>(kp, kArgLa),
                                             kernarg_at<FinalLaunch>(kp, kArgFin), kernarg_at<int>(kp, kArgG),
                                             kernarg_at<int>(kp, kArgG + 4));
  }
}

// The same tick with its inputs in the kernarg segment (InlinePack): the pointers are set to
// the pack's fields, read by flat loads like any other input (no H2D copy on the host path).
template <int LPM>
__global__ __launch_bounds__(kBlock) void plan_kernel_inl(LookbackLaunch, LookaheadLaunch, FinalLaunch, int, int,
                                                          InlinePack pk) {
  const KernargPtr kp = touch_kernargs<kPlanArgBytes>();   // the pack is not touched: flat loads
  LookbackLaunch lb = kernarg_at<LookbackLaunch>(kp, 0);
  LookaheadLaunch la = kernarg_at<LookaheadLaunch>(kp, kArgLa);
  const double* v = pk.v;
  lb.x_prev = v;
  lb.u_prev = v + 6;
  lb.x_now = v + 8;
  la.x0 = v + 8;
  la.uprev = v + 14;
  la.xref = v + 16;
  la.U = v + 16 + 2 * (la.H + 1);
  plan_body<0, true, LPM, 0>(lb, la, kernarg_at<FinalLaunch>(kp, kArgFin), kernarg_at<int>(kp, kArgG),
                             kernarg_at<int>(kp, kArgG + 4));
}

// The corridor tick (llampc_plan_corridor, llampc_lookahead_corridor): the same launch with the
// corridor as its own trailing argument (PlanCorridor, kernels.hpp), so the three launch structs and
// every other plan kernel keep their layout and code.  Shared xref, block per models, no peer
// exchange; the look-ahead blocks take the unsplit rollouts with the corridor term
// (lookahead_block CORR).  The corridor is read by value: two scalar loads behind the touch.
template <int INTEG, bool STAGE, int LPM>
__global__ __launch_bounds__(kBlock) void plan_kernel_corr(LookbackLaunch, LookaheadLaunch, FinalLaunch, int, int,
                                                           PlanCorridor cor) {
  const KernargPtr kp = touch_kernargs<kPlanArgBytes>();
  plan_body<INTEG, STAGE, LPM, 0, false, 0, true>(kernarg_at<LookbackLaunch>(kp, 0), kernarg_at<LookaheadLaunch>(kp, kArgLa),
                                                  kernarg_at<FinalLaunch>(kp, kArgFin), kernarg_at<int>(kp, kArgG),
                                                  kernarg_at<int>(kp, kArgG + 4), cor.hp, cor.weight);
}

// The launchers: lds is plan_shape's request (launch_shape.hpp), the one-block-per-CU floor included.
template <int INTEG, bool STAGE, int PX, int WQ>
static void launch_plan_wq(const LookbackLaunch& lb, const LookaheadLaunch& la, const FinalLaunch& f,
                           int G, int cpl, size_t lds, hipStream_t s) {
  allow_lds(plan_kernel<INTEG, STAGE, 1, 0, PX, WQ>);
  hipLaunchKernelGGL((plan_kernel<INTEG, STAGE, 1, 0, PX, WQ>), dim3(f.nb_lb + f.nb_la), dim3(wq_threads(WQ)),
                     lds, s, lb, la, f, G, cpl);
}

template <int INTEG, bool STAGE, int LPM>
static void launch_plan_t(const LookbackLaunch& lb, const LookaheadLaunch& la, const FinalLaunch& f,
                          int G, int cpl, size_t lds, hipStream_t s, int wq = 0) {
  if constexpr (INTEG == LLAMPC_RK4 && LPM == 1) {
    if (wq) {                            // work queue: given xref only (plan_shape checks)
      if constexpr (STAGE) {
        if (wq == 2) {
          if (f.px_G) launch_plan_wq<INTEG, STAGE, 1, 2>(lb, la, f, G, cpl, lds, s);
          else launch_plan_wq<INTEG, STAGE, 0, 2>(lb, la, f, G, cpl, lds, s);
          return;
        }
      }
      if (f.px_G) launch_plan_wq<INTEG, STAGE, 1, 1>(lb, la, f, G, cpl, lds, s);
      else launch_plan_wq<INTEG, STAGE, 0, 1>(lb, la, f, G, cpl, lds, s);
      return;
    }
  }
  if constexpr (INTEG == LLAMPC_RK4) {
    if (f.px_G) {                        // given xref only (plan_shape checks)
      allow_lds(plan_kernel<INTEG, STAGE, LPM, 0, true>);
      hipLaunchKernelGGL((plan_kernel<INTEG, STAGE, LPM, 0, true>), dim3(f.nb_lb + f.nb_la), dim3(kBlock), lds,
                         s, lb, la, f, G, cpl);
      return;
    }
  }
  if (la.xref_mode == LLAMPC_XREF_RACELINE) {
    allow_lds(plan_kernel<INTEG, STAGE, LPM, 1>);
    hipLaunchKernelGGL((plan_kernel<INTEG, STAGE, LPM, 1>), dim3(f.nb_lb + f.nb_la), dim3(kBlock), lds, s,
                       lb, la, f, G, cpl);
  } else {
    allow_lds(plan_kernel<INTEG, STAGE, LPM, 0>);
    hipLaunchKernelGGL((plan_kernel<INTEG, STAGE, LPM, 0>), dim3(f.nb_lb + f.nb_la), dim3(kBlock), lds, s,
                       lb, la, f, G, cpl);
  }
}

template <int LPM>
static void launch_plan_inl(const LookbackLaunch& lb, const LookaheadLaunch& la, const FinalLaunch& f,
                            int G, int cpl, size_t lds, hipStream_t s, const InlinePack& pk) {
  allow_lds(plan_kernel_inl<LPM>);
  hipLaunchKernelGGL((plan_kernel_inl<LPM>), dim3(f.nb_lb + f.nb_la), dim3(kBlock), lds, s, lb, la, f,
                     G, cpl, pk);
}

// One variant group of the plan launch: (integrator, lanes per rollout), staged or not;
// explicitly instantiated in plan_*.hip (declared extern in kernels.hpp).
template <int INTEG, int LPM>
void launch_plan_group(const LookbackLaunch& lb, const LookaheadLaunch& la, const FinalLaunch& f, int G,
                       int cpl, bool stage, size_t lds, hipStream_t s, int wq) {
  if (stage) launch_plan_t<INTEG, true, LPM>(lb, la, f, G, cpl, lds, s, wq);
  else launch_plan_t<INTEG, false, LPM>(lb, la, f, G, cpl, lds, s, wq);
}

template <int LPM>
void launch_plan_inline_group(const LookbackLaunch& lb, const LookaheadLaunch& la, const FinalLaunch& f,
                              int G, int cpl, size_t lds, hipStream_t s, const InlinePack& pk) {
  launch_plan_inl<LPM>(lb, la, f, G, cpl, lds, s, pk);
}

template <int INTEG, bool STAGE, int LPM>
static void launch_plan_corr(const LookbackLaunch& lb, const LookaheadLaunch& la, const FinalLaunch& f, int G,
                             int cpl, size_t lds, hipStream_t s, const PlanCorridor& cor) {
  allow_lds(plan_kernel_corr<INTEG, STAGE, LPM>);
  hipLaunchKernelGGL((plan_kernel_corr<INTEG, STAGE, LPM>), dim3(f.nb_lb + f.nb_la), dim3(kBlock), lds, s, lb, la, f,
                     G, cpl, cor);
}

// The corridor launch's variant group: (integrator, lanes per rollout), staged or not; explicitly
// instantiated in plan_corr_*.hip (declared extern in kernels.hpp).
template <int INTEG, int LPM>
void launch_plan_corridor_group(const LookbackLaunch& lb, const LookaheadLaunch& la, const FinalLaunch& f, int G,
                                int cpl, bool stage, size_t lds, hipStream_t s, const PlanCorridor& cor) {
  if (stage) launch_plan_corr<INTEG, true, LPM>(lb, la, f, G, cpl, lds, s, cor);
  else launch_plan_corr<INTEG, false, LPM>(lb, la, f, G, cpl, lds, s, cor);
}

}  // namespace llampc

// ctl_back_dev.hpp — the look-back blocks of an UNSHARDED controller tick without speculative blocks
// (blocks [0, nb_lb) of ctl_kernel_corr, ctl_corr.hip): x_t (the kernel argument or an armed launch's
// doorbell), the look-back's step, ring and lists, and in the ticket winner the merge, the published
// selection and the tick's completion; block 0 alone completes a tick without a look-back.
// This restates ctl_kernel<LPM, false>'s look-back branch with c.n_spec = 0 (ctl.hip keeps its own
// text: routing it through this function changed the register allocation of ctl.hip's code object).
#pragma once
#include "ctl_complete_dev.hpp"
#include "ctl_door_dev.hpp"
#include "ctl_lds.hpp"
#include "final_dev.hpp"
#include "lookback_dev.hpp"

namespace llampc {

__device__ __forceinline__ void ctl_lookback_role(const CtlLaunch& c, int blk, unsigned char* smem, const Scratch& sc,
                                                  int* flag) {
  unsigned char* pl = smem + c.poll_off;
  CtlSel cs{c.sel_tag, c.seq, reinterpret_cast<uint32_t*>(pl + 2048), reinterpret_cast<double*>(pl + 2304),
            reinterpret_cast<double*>(pl + 2624), reinterpret_cast<double*>(pl + 3200),
            reinterpret_cast<int32_t*>(pl + 3520)};
  if (threadIdx.x == 0) *cs.xlate = 0;
  // x_t through LDS (ctl_kernel's reason): the kernel argument, or an armed launch's doorbell — after
  // the look-back's step, which needs only the state (lookback_block<ARMED>)
  double* xl = reinterpret_cast<double*>(pl + 3072);
  auto door = [&](double, bool, int64_t) -> const double* {
    if (c.door) {
      const int r = ctl_door(c, xl, reinterpret_cast<int*>(pl + 3584));
      if (r != (int)kCtlDoorFire) {     // cancelled or expired: nothing touched
        if (r == (int)kCtlDoorExpired && blk == 0 && threadIdx.x == 0)
          __hip_atomic_store(c.host_tag, c.host_seq | kCtlTagExpired, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return nullptr;
      }
    } else {
      if (threadIdx.x < 6) xl[threadIdx.x] = ctl_xt(c, (int)threadIdx.x);
      __syncthreads();
    }
    return xl;
  };
  if (c.do_lb) {
    LookbackLaunch lb = c.lb;           // x_prev / u_prev: the state
    CTL_STAMP(blk, 0);
    if (!lookback_block<true>(lb, blk, sc, door)) return;
    CTL_STAMP(blk, 6);
    if (!ticket_last(&c.tickets[0], (unsigned)c.nb_lb, flag)) return;
    if (c.full) {
      lb_final<1>(c.fin, smem, &cs);
      __threadfence_system();           // the record's look-back half (pinned host memory)
    }
    CTL_STAMP(blk, 7);
    __syncthreads();
  } else if (!door(0.0, false, 0)) {    // ticks without a look-back: block 0 only completes
    return;
  }
  ctl_complete(c, smem, cs, xl);
}

}  // namespace llampc

// ctl.hip — the controller tick: one launch per LLA-MPC control step (ctl.hpp has the map to
// the reference).  Roles by block index (look-back blocks first in dispatch order):
//
//   look-back blocks [0, nb_lb)   the plan launch's look-back (lookback_block: RK4 step of
//                                 every model from the state's (x_{t-1}, u_{t-1}), error, ring,
//                                 window mean, wave/block top-K lists); the last one (ticket)
//                                 merges them (lb_final<SEL>), PUBLISHES the selection
//                                 (top-K + argmin, tagged words) and completes the tick
//                                 (ctl_complete).  Without a look-back (ticks 0, 1) block 0
//                                 only completes.
//   look-ahead blocks [nb_lb, ..) each: the raceline tables to LDS; the projection of x_t and
//                                 ConstantSpeed with mu-hat (one lane walks, planner.py:
//                                 24-65); the C candidates (Philox, every lane); then it WAITS
//                                 for the selection (or, while the window fills, takes the
//                                 nominal model) and rolls out its slots' models x C candidates
//                                 (the plan kernel's fused RK4 rollout, candidates read from
//                                 LDS) and publishes each slot's best candidate.
//
// Waiting: a look-ahead block waits only for the look-back ticket winner, a block of LOWER
// index; workgroups are dispatched in index order (per XCD), so that block has been dispatched
// and never waits on a look-ahead block before it publishes (the selection comes before its
// own poll).  The completion waits only for look-ahead blocks, which then never wait again.
// Every wait has a bound (status LLAMPC_STATUS_POLL_TIMEOUT, never expected).
//
// The device code by role: ctl_lds.hpp (the LDS layouts), ctl_door_dev.hpp (x_t, the doorbell,
// the tagged-word waits and a slot's result words), ctl_cand_dev.hpp (the candidates),
// cs_dev.hpp (ConstantSpeed), ctl_lookahead_dev.hpp (a look-ahead block), ctl_spec_dev.hpp (the
// speculative look-ahead: spec blocks, last in the grid) and ctl_complete_dev.hpp (the sharded
// exchange and the completion).  Here: the kernels and their launchers.
#include "ctl.hpp"
#include "cs_dev.hpp"
#include "ctl_complete_dev.hpp"
#include "ctl_lds.hpp"
#include "ctl_lookahead_dev.hpp"
#include "ctl_spec_dev.hpp"
#include "dev_wave.hpp"
#include "final_dev.hpp"
#include "lookback_dev.hpp"
#include "rollout_dev.hpp"

namespace llampc {

#ifdef LLAMPC_STAMPS
extern "C" int llampc_debug_ctl_stamps(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ctl_ph), sizeof(g_ctl_ph)) == hipSuccess ? 0 : -2;
}
#endif

// PX: the sharded controller (ctl_exchange after the shard's lb_final) — its own
// instantiation, so the unsharded tick's code is unchanged
template <int LPM, bool PX>
__global__ __launch_bounds__(kBlock) void ctl_kernel(CtlLaunch arg) {
  // the argument read in place from the kernarg segment (it is the launch's first and only
  // explicit argument): referencing the by-value parameter itself made the compiler copy all
  // 1.4 KB of it to scratch once the kernel grew
  (void)arg;
  const CtlLaunch& c = *(const CtlLaunch*)__builtin_amdgcn_kernarg_segment_ptr();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Scratch sc(smem);
  int* flag = reinterpret_cast<int*>(smem + kFlagOff);
  const int blk = (int)blockIdx.x;
  // x_t in the argument: the device time starts here (a gathered tick's: at its first launch)
  if (blk == 0 && threadIdx.x == 0 && !c.door && !(PX && c.px_phase == 2))
    st_wt(&c.door_dev[kCtlTimeWord], (uint64_t)__builtin_amdgcn_s_memrealtime());
  if (blk >= c.nb_lb + c.nb_la) {       // spec blocks (CtlLaunch.n_spec), last in the grid
    ctl_spec<LPM>(c, blk - c.nb_lb - c.nb_la, smem, sc);
    return;
  }
  if (blk >= c.nb_lb) {
    ctl_lookahead<LPM>(c, blk - c.nb_lb, smem, sc);
    return;
  }
  unsigned char* pl = smem + c.poll_off;
  CtlSel cs{c.sel_tag, c.seq, reinterpret_cast<uint32_t*>(pl + 2048), reinterpret_cast<double*>(pl + 2304),
            reinterpret_cast<double*>(pl + 2624), reinterpret_cast<double*>(pl + 3200),
            reinterpret_cast<int32_t*>(pl + 3520)};
  if (threadIdx.x == 0) *cs.xlate = 0;
  // x_t through LDS (pointing into the kernel argument itself would make the compiler copy the
  // whole argument to scratch): the kernel argument, or an armed launch's doorbell — after the
  // look-back's step, which needs only the state (lookback_block<ARMED>)
  double* xl = reinterpret_cast<double*>(pl + 3072);
  auto door = [&](double pred, bool pvalid, int64_t pn) -> const double* {
    // the speculative look-ahead's ranking first: it needs only the window (before x_t)
    if (c.n_spec) ctl_spec_lists<PX>(c, blk, pred, pvalid, pn, smem, flag);
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
  if (PX && c.px_phase == 2) {         // a gathered tick's second launch: block 0 merges, completes
    if (!door(0.0, false, 0)) return;
    ctl_exchange(c, smem, cs);
    __threadfence_system();             // the record's look-back half (pinned host memory)
    __syncthreads();
  } else if (c.do_lb) {
    LookbackLaunch lb = c.lb;           // x_prev / u_prev: the state
    CTL_STAMP(blk, 0);
    if (!lookback_block<true>(lb, blk, sc, door)) return;
    CTL_STAMP(blk, 6);
    if (!ticket_last(&c.tickets[0], (unsigned)c.nb_lb, flag)) return;
    if (c.full) {
      if constexpr (PX) {
        lb_final<2>(c.fin, smem, &cs);  // this shard's lists, then the exchange and the merge
        if (c.px_phase == 1) {          // gathered: the record out, the rest in the second launch
          ctl_px_send(c, cs);
          return;
        }
        ctl_exchange(c, smem, cs);
      } else {
        lb_final<1>(c.fin, smem, &cs);
      }
      __threadfence_system();           // the record's look-back half (pinned host memory)
    }
    CTL_STAMP(blk, 7);
    __syncthreads();
  } else if (!door(0.0, false, 0)) {    // ticks without a look-back: block 0 only completes
    return;
  }
  ctl_complete(c, smem, cs, xl);
}

// llampc_ctl_reference: ConstantSpeed alone (one block), into out = xref [2][H+1], projidx,
// vr.  LDS: xref | knots | two profiles | dists (the controller's layout with C = 0).
__global__ __launch_bounds__(kBlock) void cs_kernel(CsLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const CtlLds L = ctl_lds(a.H, 0, a.rl.n);
  double* sx = reinterpret_cast<double*>(smem + L.sx);
  double* kn = reinterpret_cast<double*>(smem + L.kn);
  double* spd = reinterpret_cast<double*>(smem + L.spd);
  double* dist = reinterpret_cast<double*>(smem + L.misc);
  const MuBracket br = mu_bracket(a.rl.mus, a.rl.M, a.mu);
  cs_stage(a.rl, br, kn, spd);
  const int segs = cs_project(a.pts, a.np, a.p0, a.x0, a.y0, dist);
  __syncthreads();
  if (threadIdx.x < 64) {                // wave 0 walks (the controller tick's walker)
    double vr = 0.0;
    const int pj = cs_walk_wave(a.rl, br, kn, spd, a.prefix, dist, segs, a.p0, a.x0, a.y0, a.v0, a.scale, a.Ts,
                                a.H, sx, &vr);
    if (threadIdx.x == 0) {
      a.out[2 * (a.H + 1)] = (double)pj;
      a.out[2 * (a.H + 1) + 1] = vr;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * (a.H + 1); e += kBlock) {
    const int row = e / (a.H + 1), k = e - row * (a.H + 1);
    a.out[e] = sx[2 * k + row];
  }
}

hipError_t launch_constant_speed(const CsLaunch& a, hipStream_t s) {
  const CtlLds L = ctl_lds(a.H, 0, a.rl.n);
  allow_lds(cs_kernel);
  hipLaunchKernelGGL(cs_kernel, dim3(1), dim3(kBlock), L.end, s, a);
  return hipGetLastError();
}

template <bool PX>
static void launch_ctl_px(const CtlLaunch& c, int lpm, size_t lds, hipStream_t s) {
  const dim3 grid(c.nb_lb + c.nb_la + c.n_spec), block(kBlock);
  if (lpm == 4) {
    allow_lds(ctl_kernel<4, PX>);
    hipLaunchKernelGGL((ctl_kernel<4, PX>), grid, block, lds, s, c);
  } else if (lpm == 2) {
    allow_lds(ctl_kernel<2, PX>);
    hipLaunchKernelGGL((ctl_kernel<2, PX>), grid, block, lds, s, c);
  } else {
    allow_lds(ctl_kernel<1, PX>);
    hipLaunchKernelGGL((ctl_kernel<1, PX>), grid, block, lds, s, c);
  }
}

hipError_t launch_ctl(const CtlLaunch& c, int lpm, size_t lds, hipStream_t s) {
  if (c.px_G) launch_ctl_px<true>(c, lpm, lds, s);
  else launch_ctl_px<false>(c, lpm, lds, s);
  return hipGetLastError();
}

}  // namespace llampc

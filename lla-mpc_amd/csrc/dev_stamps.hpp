// dev_stamps.hpp — the diagnostic stamps of the device code: the LLAMPC_STAMPS globals and the
// STAMP / LA_STAMP / LB_STAMP / RL_STAMP / STEP_STAMP / WQ_STAMP / CTL_STAMP macros, which
// expand to nothing in the product build.  Included by every device header that stamps a phase;
// the llampc_debug_* readers of the globals are in plan_rk4_l4.hip, plan_rk4_l1.hip and ctl.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace llampc {

#ifdef LLAMPC_STAMPS
// Diagnostic build only (-DLLAMPC_STAMPS, libllampc_hip_stamps.so): tid-0 stamps of
// s_memtime (shader clock) and s_memrealtime (100 MHz) at phase boundaries of the select
// kernel; never compiled into the product library.
static __device__ unsigned long long g_stamps[64][8][2];
static __device__ unsigned int g_stamp_launch;
static __device__ unsigned long long g_la_stamps[8][8][2];   // first 8 look-ahead blocks, last launch
static __device__ unsigned long long g_lb_stamps[8][8][2];   // first 8 look-back blocks, last launch
#define LB_STAMP(blk, slot)                                                              \
  do {                                                                                   \
    if (threadIdx.x == 0 && (blk) < 8) {                                                 \
      g_lb_stamps[blk][slot][0] = __builtin_amdgcn_s_memtime();                          \
      g_lb_stamps[blk][slot][1] = __builtin_amdgcn_s_memrealtime();                      \
    }                                                                                    \
  } while (0)
static __device__ unsigned long long g_la_all[1024][4][2];    // every look-ahead block, last launch
static __device__ unsigned long long g_la_wave[1024][4];      // rollout end of every look-ahead wave
static __device__ double g_rl_dbg[8];                          // raceline window decision (block 0)
static __device__ unsigned long long g_rl_ph[1024][4];         // raceline prologue phases per block
#define RL_STAMP(blk, slot)                                                              \
  do {                                                                                   \
    if (threadIdx.x == 0 && (blk) < 1024) g_rl_ph[blk][slot] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define LA_STAMP(blk, slot)                                                              \
  do {                                                                                   \
    if (threadIdx.x == 0) {                                                              \
      const unsigned long long c_ = __builtin_amdgcn_s_memtime();                        \
      const unsigned long long r_ = __builtin_amdgcn_s_memrealtime();                    \
      if ((blk) < 8) {                                                                   \
        g_la_stamps[blk][slot][0] = c_;                                                  \
        g_la_stamps[blk][slot][1] = r_;                                                  \
      }                                                                                  \
      if ((blk) < 1024) {                                                                \
        g_la_all[blk][slot][0] = c_;                                                     \
        g_la_all[blk][slot][1] = r_;                                                     \
      }                                                                                  \
    }                                                                                    \
  } while (0)
// per rollout step (FAST rollouts, thread 0 of every block < 1024): s_memtime before step k
// (k < 24) and at the loop's end (slot 24) — the first step's cold code fetch against the rest
static __device__ unsigned long long g_la_step[1024][25];
#define STEP_STAMP(k)                                                                    \
  do {                                                                                   \
    if (threadIdx.x == 0 && blockIdx.x < 1024 && (k) <= 24)                              \
      g_la_step[blockIdx.x][k] = __builtin_amdgcn_s_memtime();                           \
  } while (0)
#define STAMP(slot)                                                                      \
  do {                                                                                   \
    if (threadIdx.x == 0) {                                                              \
      const unsigned l = g_stamp_launch & 63;                                            \
      g_stamps[l][slot][0] = __builtin_amdgcn_s_memtime();                               \
      g_stamps[l][slot][1] = __builtin_amdgcn_s_memrealtime();                           \
    }                                                                                    \
  } while (0)
// work-queue layout: per wave, per unit j < 16, (s_memtime, s_memrealtime) at [0] the unit
// taken, [1] its Pacejka row loaded, [2] rolled out, [3] done (the tagged stores issued)
static __device__ unsigned long long g_wq_unit[256][8][16][4][2];
#define WQ_STAMP(blk, j, slot)                                                           \
  do {                                                                                   \
    if ((threadIdx.x & 63) == 0 && (blk) < 256 && (j) < 16) {                            \
      g_wq_unit[blk][threadIdx.x >> 6][j][slot][0] = __builtin_amdgcn_s_memtime();       \
      g_wq_unit[blk][threadIdx.x >> 6][j][slot][1] = __builtin_amdgcn_s_memrealtime();   \
    }                                                                                    \
  } while (0)
// The controller tick (ctl.hip): s_memrealtime (100 MHz) per block and phase of the last launch
// (tools/diag/ctl_phases.py; the reader, llampc_debug_ctl_stamps, is in ctl.hip).  Look-ahead
// blocks: 0 entry, 1 staged, 10 walk done, 2 walk
// barrier, 3 selection, 4 rolled out, 5 published; look-back blocks: 0 entry, 6 scored,
// 7 lb_final done (ticket winner), 8 slots polled, 12 top-K / sequence stores issued, 13 the
// record words computed, 11 record stores issued, 9 record written; look-ahead prologue: 14 the
// mu bracket known, 15 the tables' LDS stores issued; 16 an armed launch's doorbell seen; the
// walk (cs_walk_wave): 17 its loop entered, 18 its loop done (then x/y).
static __device__ unsigned long long g_ctl_ph[64][24];
#define CTL_STAMP(blk, slot)                                                                   \
  do {                                                                                         \
    if (threadIdx.x == 0 && (blk) < 64) g_ctl_ph[blk][slot] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define LLAMPC_NO_STAMP \
  do {                  \
  } while (0)
#define STEP_STAMP(k) LLAMPC_NO_STAMP
#define WQ_STAMP(blk, j, slot) LLAMPC_NO_STAMP
#define STAMP(slot) LLAMPC_NO_STAMP
#define LA_STAMP(blk, slot) LLAMPC_NO_STAMP
#define RL_STAMP(blk, slot) LLAMPC_NO_STAMP
#define LB_STAMP(blk, slot) LLAMPC_NO_STAMP
#define CTL_STAMP(blk, slot) LLAMPC_NO_STAMP
#endif

}  // namespace llampc

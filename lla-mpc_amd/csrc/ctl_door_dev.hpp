// ctl_door_dev.hpp — how the blocks of a controller tick wait for one another and for the host:
// x_t from the kernel argument or an armed launch's doorbell (every block), the bounded poll of
// one tagged word (look-ahead, spec and completing blocks), the batched poll of a mailbox
// (the look-back ticket winner's exchanges) and a slot's four result words (written by the
// look-ahead and spec blocks, read by the completing block).  Included by ctl.hip's headers only.
#pragma once
#include "ctl.hpp"
#include "dev_stamps.hpp"
#include "dev_wave.hpp"

namespace llampc {

// x_t[i] of the kernel argument by constant indices (a dynamic index into the argument's array
// makes the compiler copy the whole argument to scratch)
__device__ __forceinline__ double ctl_xt(const CtlLaunch& c, int i) {
  double v = c.x_t[0];
#pragma unroll
  for (int j = 1; j < 6; ++j) v = i == j ? c.x_t[j] : v;
  return v;
}

__device__ __forceinline__ bool ctl_late(uint64_t t0, uint32_t poll) {
  return __builtin_amdgcn_s_memrealtime() - t0 > ((uint64_t)poll << 16);
}

// The tagged word tags[i] polled until it carries seq: its payload, or after mult * bound
// (ctl_late's unit) kNoLocal with late set.  tags, seq and bound are references into the kernel
// argument, as in read_slot below: their loads stay behind the clock read and off the hit path.
__device__ __forceinline__ uint32_t poll_tag(uint64_t* const& tags, int i, const uint32_t& seq, const uint32_t& bound,
                                             int& late, uint32_t mult = 1) {
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  uint32_t v = kNoLocal;
  for (;;) {
    const uint64_t w = ld_wt(&tags[i]);
    if (tag_ok(w, seq)) {
      v = (uint32_t)w;
      break;
    }
    if (ctl_late(t0, mult * bound)) {
      late = 1;
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  return v;
}

// A slot's result (CtlLaunch.slot_tag, spec_res), four words tagged seq: the best candidate's
// cost (hi, lo), the candidate, and the slot's non-finite count with bit 31 set when the
// publisher's own wait for the selection ran out.  One lane publishes; the completing block's
// lane reads all four each round (no sleep: it is the tick's tail) and returns late — after
// `bound`, or bit 31 — with cost NaN, candidate -1 and count 0.
__device__ __forceinline__ void publish_slot(uint64_t* w, uint32_t seq, double cost, int64_t cand, uint32_t nf_word) {
  const uint64_t vb = (uint64_t)__double_as_longlong(cost);
  st_wt(&w[0], tag_word(seq, (uint32_t)(vb >> 32)));
  st_wt(&w[1], tag_word(seq, (uint32_t)vb));
  st_wt(&w[2], tag_word(seq, (uint32_t)(int32_t)cand));
  st_wt(&w[3], tag_word(seq, nf_word));
}
__device__ __forceinline__ void read_slot(const uint64_t* src, const uint32_t& seq, const uint32_t& bound, int& late,
                                          double* cost, int32_t* cand, int32_t* nf, int i) {
  uint64_t w[4];
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  for (;;) {
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = ld_wt(&src[q]);
    if ((int)tag_ok(w[0], seq) & (int)tag_ok(w[1], seq) & (int)tag_ok(w[2], seq) & (int)tag_ok(w[3], seq)) break;
    if (ctl_late(t0, bound)) {
      late = 1;
      break;
    }
  }
  const uint32_t nfw = (uint32_t)w[3];
  late |= (int)(nfw >> 31);
  cost[i] = late ? __builtin_nan("") : __longlong_as_double((long long)join_words(w[0], w[1]));
  cand[i] = late ? -1 : (int32_t)(uint32_t)w[2];
  nf[i] = late ? 0 : (int32_t)(nfw & 0x7FFFFFFFu);
}

// An armed launch's doorbell (CtlLaunch.door): thread 0 of block 0 polls the pinned host copy
// (system-scope loads, all 13 words a round), every other block the device copy block 0 makes:
// its STATUS word alone, and once that carries door_seq the 12 x_t halves (block 0 drains their
// stores before it stores the status); every word's tag is checked.  One word per round on the
// device side: 13 words a round from 64 blocks made the relay 2.9 us instead of 1.1
// (tools/diag/doorbell_lat.hip, mode 3).  Returns, block-uniform after
// the barrier: kCtlDoorFire (x_t in xl), kCtlDoorCancel, kCtlDoorExpired.
__device__ __forceinline__ int ctl_door(const CtlLaunch& c, double* xl, int* res) {
  if (threadIdx.x == 0) {
    const bool host = blockIdx.x == 0;
    auto ld = [&](int q) {
      return host ? __hip_atomic_load(&c.door[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : ld_wt(&c.door_dev[q]);
    };
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint64_t w[kCtlDoorWords];
    int r;
    for (;;) {
      // block 0 reads every word each round (the PCIe reads overlap; a second round trip for
      // the x_t halves after the status would add ~1 us), the others the status word first
      if (host) {
#pragma unroll
        for (int q = 0; q < kCtlDoorWords - 1; ++q) w[q] = ld(q);
      }
      const uint64_t sw = ld(kCtlDoorWords - 1);
      if (tag_ok(sw, c.door_seq)) {
        w[kCtlDoorWords - 1] = sw;
        r = (int)(uint32_t)sw;
        if (r != (int)kCtlDoorFire) break;
        if (!host) {
#pragma unroll
          for (int q = 0; q < kCtlDoorWords - 1; ++q) w[q] = ld(q);
        }
        int all = 1;
#pragma unroll
        for (int q = 0; q < kCtlDoorWords - 1; ++q) all &= (int)tag_ok(w[q], c.door_seq);
        if (all) break;
      }
      // block 0 gives up at the bound; the others wait twice as long for its verdict
      if (ctl_late(t0, host ? c.door_bound : 2 * c.door_bound)) {
        r = (int)kCtlDoorExpired;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (host) {                         // the verdict for the other blocks: x_t, drained, then the status
      if (r == (int)kCtlDoorFire) {
        st_wt(&c.door_dev[kCtlTimeWord], (uint64_t)__builtin_amdgcn_s_memrealtime());
#pragma unroll
        for (int q = 0; q < kCtlDoorWords - 1; ++q) st_wt(&c.door_dev[q], w[q]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      st_wt(&c.door_dev[kCtlDoorWords - 1], r == (int)kCtlDoorExpired ? tag_word(c.door_seq, kCtlDoorExpired)
                                                                       : w[kCtlDoorWords - 1]);
    }
    if (r == (int)kCtlDoorFire) {
#pragma unroll
      for (int j = 0; j < 6; ++j) xl[j] = __longlong_as_double((long long)join_words(w[2 * j], w[2 * j + 1]));
    }
    *res = r;
  }
  CTL_STAMP(blockIdx.x, 16);
  __syncthreads();
  return *res;
}

// Polls this rank's mailbox words own[g stride + w] (w < nw, every g != rank) until each carries
// the tag seq — every thread issues all of its loads of a round before checking any (one memory
// round trip per round; a load under a per-word condition waits its own) — into rec32[g nw + w].
// Gives up after `bound` s_memrealtime ticks; returns this thread's late flag.
template <int kPer>
__device__ __forceinline__ int ctl_poll_words(const uint64_t* own, size_t stride, int G, int nw, int rank,
                                              uint32_t seq, uint64_t bound, uint32_t* rec32) {
  const int tid = threadIdx.x, total = G * nw;
  uint64_t need = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int e = tid + j * kBlock;
    if (e < total && e / nw != rank) need |= 1ull << j;
  }
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  while (need) {
    uint64_t v[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int e = ((need >> j) & 1) ? tid + j * kBlock : rank * nw;   // idle: own slot (never read back)
      const int g = e / nw, w = e - g * nw;
      v[j] = __hip_atomic_load(own + (size_t)g * stride + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (((need >> j) & 1) && tag_ok(v[j], seq)) {
        rec32[tid + j * kBlock] = (uint32_t)v[j];
        need &= ~(1ull << j);
      }
    }
    if (!need) break;
    if (__builtin_amdgcn_s_memrealtime() - t0 > bound) return 1;
    __builtin_amdgcn_s_sleep(1);
  }
  return 0;
}

}  // namespace llampc

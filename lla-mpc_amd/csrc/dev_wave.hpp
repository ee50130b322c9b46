// dev_wave.hpp — primitives under every kernel of the library: wave-wide DPP / readlane
// reductions and ordered picks, the write-through (sc1) hand-off loads and stores, tagged
// words, pin_vgpr, the dynamic-LDS scratch every block role starts with (Scratch, block_min1)
// and the in-launch completion ticket.  Included by the other *_dev.hpp headers and by
// ctl.hip, nlp.hip and kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch_shape.hpp"

namespace llampc {

// split_key's arithmetic (below), callable from the host: key = m C + c with 0 <= c < C for
// 0 <= key < 2^63, 1 <= C < 2^31.  The fp64 quotient of the key is within 2^11 of m (the key's
// rounding to 53 bits over C >= 1), the quotient of that step's exact remainder within 1 of the
// rest, and one fix-up step makes the split exact (tests/test_split_key.py checks it against / and %).
__host__ __device__ __forceinline__ void split_key_hd(int64_t key, int32_t C, int64_t& m, int32_t& c) {
  const double dc = (double)C;
  int64_t q = (int64_t)((double)key / dc);
  q += (int64_t)((double)(key - q * C) / dc);
  int64_t r = key - q * C;
  if (r < 0) {
    q -= 1;
    r += C;
  } else if (r >= C) {
    q += 1;
    r -= C;
  }
  m = q;
  c = (int32_t)r;
}

namespace {

template <int NAN_FIRST>
__device__ __forceinline__ bool kless(double av, int64_t ai, double bv, int64_t bi) {
  return NAN_FIRST ? less_nan_first(av, ai, bv, bi) : less_nan_last(av, ai, bv, bi);
}

// Cross-lane moves within rows of 16 lanes (DPP; a disabled source lane returns the lane's
// own value).  xor 1 / xor 2 = quad_perm [1,0,3,2] / [2,3,0,1]; rotate by 4 / 8 in a row.
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppRor4 = 0x124, kDppRor8 = 0x128;
template <int CTRL>
__device__ __forceinline__ int dpp_i(int x) {
  return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  return __hiloint2double(dpp_i<CTRL>(__double2hiint(v)), dpp_i<CTRL>(__double2loint(v)));
}
template <int CTRL>
__device__ __forceinline__ int64_t dpp_l(int64_t v) {
  const uint64_t u = (uint64_t)v;
  const uint64_t lo = (uint32_t)dpp_i<CTRL>((int)(uint32_t)u), hi = (uint32_t)dpp_i<CTRL>((int)(u >> 32));
  return (int64_t)(lo | (hi << 32));
}
__device__ __forceinline__ double readlane_d(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double readfirstlane_d(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                          __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ int64_t readlane_l(int64_t v, int l) {
  const uint64_t u = (uint64_t)v;
  const uint64_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l);
  const uint64_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(u >> 32), l);
  return (int64_t)(lo | (hi << 32));
}

template <int NAN_FIRST, int CTRL>
__device__ __forceinline__ void min_step(double& v, int64_t& i) {
  const double ov = dpp_d<CTRL>(v);
  const int64_t oi = dpp_l<CTRL>(i);
  if (kless<NAN_FIRST>(ov, oi, v, i)) {
    v = ov;
    i = oi;
  }
}

// Wave-wide min of (v, i) under kless<NAN_FIRST>, the result in every lane.  ALL 64 lanes
// must be active (converged code).  DPP butterfly inside each row of 16 lanes, then the four
// row results combined from readlanes — no LDS round trips (the __shfl_xor form cost ~4k
// cycles per block reduction, SQ stamps).
template <int NAN_FIRST>
__device__ __forceinline__ void wave_min(double& v, int64_t& i) {
  min_step<NAN_FIRST, kDppXor1>(v, i);
  min_step<NAN_FIRST, kDppXor2>(v, i);
  min_step<NAN_FIRST, kDppRor4>(v, i);
  min_step<NAN_FIRST, kDppRor8>(v, i);
  double bv = readlane_d(v, 0);
  int64_t bi = readlane_l(i, 0);
#pragma unroll
  for (int r = 16; r < 64; r += 16) {
    const double rv = readlane_d(v, r);
    const int64_t ri = readlane_l(i, r);
    if (kless<NAN_FIRST>(rv, ri, bv, bi)) {
      bv = rv;
      bi = ri;
    }
  }
  v = bv;
  i = bi;
}

// Branch-free ordered picks over a wave (all 64 lanes active).  A lane's candidate is
// (v, li) with li a local model index (order = global index order); a lane without one holds
// li = kNoLocal (and v = NaN, or +inf under NaN-first).  The value min runs on v_min_f64
// (IEEE minNum: NaN only when every lane is NaN), the tie-break on u32 mins — no compare of
// (value, index) pairs and no divergent branch.
constexpr uint32_t kNoLocal = 0xFFFFFFFFu;
__device__ __forceinline__ double wave_min_f64(double v) {
  v = fmin(v, dpp_d<kDppXor1>(v));
  v = fmin(v, dpp_d<kDppXor2>(v));
  v = fmin(v, dpp_d<kDppRor4>(v));
  v = fmin(v, dpp_d<kDppRor8>(v));
  return fmin(fmin(readlane_d(v, 0), readlane_d(v, 16)), fmin(readlane_d(v, 32), readlane_d(v, 48)));
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
  x = min(x, (uint32_t)dpp_i<kDppXor1>((int)x));
  x = min(x, (uint32_t)dpp_i<kDppXor2>((int)x));
  x = min(x, (uint32_t)dpp_i<kDppRor4>((int)x));
  x = min(x, (uint32_t)dpp_i<kDppRor8>((int)x));
  const uint32_t a = min((uint32_t)__builtin_amdgcn_readlane((int)x, 0), (uint32_t)__builtin_amdgcn_readlane((int)x, 16));
  const uint32_t b = min((uint32_t)__builtin_amdgcn_readlane((int)x, 32), (uint32_t)__builtin_amdgcn_readlane((int)x, 48));
  return min(a, b);
}
// NaN-last order (argsort): the smallest value, ties (and all-NaN) -> the lowest li.
__device__ __forceinline__ void wave_pick_nl(double& v, uint32_t& li) {
  const double m = wave_min_f64(v);
  const int c = (int)(li != kNoLocal) & ((int)(v == m) | ((int)(m != m) & (int)(v != v)));
  li = wave_min_u32(c ? li : kNoLocal);
  v = m;
}
// NaN-first order (np.argmin): the lowest li holding NaN if there is one.
__device__ __forceinline__ void wave_pick_nf(double& v, uint32_t& li) {
  const int isn = (int)(li != kNoLocal) & (int)(v != v);
  if (__any(isn)) {                     // wave-uniform
    li = wave_min_u32(isn ? li : kNoLocal);
    v = __builtin_nan("");
  } else {
    wave_pick_nl(v, li);
  }
}

// As wave_pick_nl with an int64 key (kNoIndex = none): u32 mins over the key's high word,
// then over the low word of the lanes holding that high word.
__device__ __forceinline__ void wave_pick_nl64(double& v, int64_t& key) {
  const double m = wave_min_f64(v);
  const int c = (int)(key != kNoIndex) & ((int)(v == m) | ((int)(m != m) & (int)(v != v)));
  const uint32_t hi = (uint32_t)((uint64_t)key >> 32), lo = (uint32_t)key;
  const uint32_t mh = wave_min_u32(c ? hi : kNoLocal);
  const uint32_t ml = wave_min_u32((c & (int)(hi == mh)) ? lo : kNoLocal);
  key = (mh == kNoLocal && ml == kNoLocal) ? kNoIndex : (int64_t)(((uint64_t)mh << 32) | ml);
  v = m;
}

// Cross-workgroup hand-offs inside the plan launch use write-through (sc1) stores and sc1
// loads with a relaxed agent-scope ticket (MI355X_MICROARCH.md, "Valid forms", first table
// row: every handed-off byte stored sc1 by a wave that drains vmcnt(0) before its block's
// barrier and the one-lane ticket add; the last adder's block loads them sc1; one workgroup
// per CU, guaranteed by the launch's LDS request).  No buffer_wbl2 / buffer_inv.
template <typename T>
__device__ __forceinline__ void st_wt(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ T ld_wt(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// key = m C + c (0 <= c < C, 0 <= key < 2^63) split without the 64-bit integer division's
// ~150-instruction software sequence (the controller record's and the plan record's look-ahead
// best): split_key_hd above.
__device__ __forceinline__ void split_key(int64_t key, int32_t C, int64_t& m, int32_t& c) {
  split_key_hd(key, C, m, c);
}

// Tagged 64-bit words of the polled completion: launch tag in the high half, payload low.
__device__ __forceinline__ uint64_t tag_word(uint32_t seq, uint32_t payload) {
  return ((uint64_t)seq << 32) | payload;
}
__device__ __forceinline__ bool tag_ok(uint64_t w, uint32_t seq) { return (uint32_t)(w >> 32) == seq; }
__device__ __forceinline__ uint64_t join_words(uint64_t hi, uint64_t lo) {
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

__device__ __forceinline__ int wave_sum(int x) {
  x += dpp_i<kDppXor1>(x);
  x += dpp_i<kDppXor2>(x);
  x += dpp_i<kDppRor4>(x);
  x += dpp_i<kDppRor8>(x);
  return __builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) +
         __builtin_amdgcn_readlane(x, 32) + __builtin_amdgcn_readlane(x, 48);
}

// Keep a wave-uniform value in a VGPR: the rollout loop needs ~25 uniform vehicle/cost
// constants; left in SGPRs they overflow the 102-SGPR budget together with the
// polynomial constants and get spilled to VGPR lanes (v_readlane reloads in the loop).
__device__ __forceinline__ void pin_vgpr(double& x) { asm volatile("" : "+v"(x)); }

// The plan kernels' first instructions: one scalar load from every 64-byte line of the
// explicit kernel arguments, all in flight together, then one wait.  The scalar cache is cold
// at every launch and the compiler reads the arguments where it needs them, in groups that
// each wait for their own miss (the look-ahead path: four groups in series before its first
// input load); after this touch those reads hit.  BYTES: the arguments' size.  The segment's
// base is only 8-byte aligned, so the arguments span kArgLines lines or one more: the extra
// load reads the last argument word.  The loads and their wait are one statement and the
// dummy destinations early-clobber, so no destination is reused while its load is in flight.
// Returns the segment's base as the statement's own output: argument loads are invariant, so
// the compiler places those of the by-value parameters above any statement of the kernel;
// the kernels read their arguments through this pointer instead (kernarg_at), plain scalar
// loads as before, which therefore follow the touch.
typedef const __attribute__((address_space(4))) unsigned char* KernargPtr;
constexpr int kArgLines = 15;
template <int BYTES>
__device__ __forceinline__ KernargPtr touch_kernargs() {
  static_assert((BYTES + 63) / 64 == kArgLines, "touch_kernargs: one load per line of the arguments");
  constexpr int kLast = BYTES - 4;
  static_assert(kLast >= 64 * (kArgLines - 1) && kLast % 4 == 0, "the last word lies in the last line");
  uint64_t base = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
  uint32_t d0, d1, d2, d3, d4, d5, d6, d7, d8, d9, d10, d11, d12, d13, d14, d15;
  asm volatile(
      "s_load_dword %0, %16, 0x0\n\t"
      "s_load_dword %1, %16, 0x40\n\t"
      "s_load_dword %2, %16, 0x80\n\t"
      "s_load_dword %3, %16, 0xc0\n\t"
      "s_load_dword %4, %16, 0x100\n\t"
      "s_load_dword %5, %16, 0x140\n\t"
      "s_load_dword %6, %16, 0x180\n\t"
      "s_load_dword %7, %16, 0x1c0\n\t"
      "s_load_dword %8, %16, 0x200\n\t"
      "s_load_dword %9, %16, 0x240\n\t"
      "s_load_dword %10, %16, 0x280\n\t"
      "s_load_dword %11, %16, 0x2c0\n\t"
      "s_load_dword %12, %16, 0x300\n\t"
      "s_load_dword %13, %16, 0x340\n\t"
      "s_load_dword %14, %16, 0x380\n\t"
      "s_load_dword %15, %16, %17\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&s"(d0), "=&s"(d1), "=&s"(d2), "=&s"(d3), "=&s"(d4), "=&s"(d5), "=&s"(d6), "=&s"(d7), "=&s"(d8),
        "=&s"(d9), "=&s"(d10), "=&s"(d11), "=&s"(d12), "=&s"(d13), "=&s"(d14), "=&s"(d15), "+s"(base)
      : "i"(kLast)
      : "memory");
  return (KernargPtr)base;
}
// The argument of type T at byte offset `off` of the segment.
template <typename T>
__device__ __forceinline__ const T& kernarg_at(KernargPtr p, int off) {
  return *(const T*)reinterpret_cast<const __attribute__((address_space(4))) T*>(p + off);
}

}  // namespace

// Dynamic LDS carve shared by every role (16-B aligned offsets, cdna_hip_programming.md
// G17): [0,64) sv[2][4] double | [64,128) si[2][4] int64 | [128,160) sn[8] int32 (the
// 8-wave work-queue block's la_publish uses all 8) | [160,164) the ticket flag (kFlagOff) |
// [168,176) the poller's per-wave late flags (kLateOff) | pad to 192 | role-specific region
// from 192 (kScratchBytes, with the other sizes the launch's LDS request is made of:
// launch_shape.hpp).
constexpr int kFlagOff = 160;
constexpr int kLateOff = 168;

struct Scratch {
  double* sv;
  int64_t* si;
  int32_t* sn;
  __device__ explicit Scratch(unsigned char* smem)
      : sv(reinterpret_cast<double*>(smem)),
        si(reinterpret_cast<int64_t*>(smem + 64)),
        sn(reinterpret_cast<int32_t*>(smem + 128)) {}
};

// Block min with ONE barrier: consecutive calls alternate between two scratch buffers, so
// a buffer is rewritten only after the next call's barrier has retired all its readers.
template <int NAN_FIRST>
__device__ __forceinline__ void block_min1(double& v, int64_t& i, const Scratch& s, int& par) {
  wave_min<NAN_FIRST>(v, i);
  double* sv = s.sv + 4 * par;
  int64_t* si = s.si + 4 * par;
  par ^= 1;
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = v;
    si[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  v = sv[0];
  i = si[0];
#pragma unroll
  for (int k = 1; k < kBlock / 64; ++k) {
    if (kless<NAN_FIRST>(sv[k], si[k], v, i)) {
      v = sv[k];
      i = si[k];
    }
  }
}

// ------------------------------------------------------------------------------------
// In-launch completion tickets (wait-free): every storing wave drains its (sc1) stores, the
// block barriers, lane 0 bumps the ticket (relaxed, agent scope); the block that draws the
// last ticket continues and reads the handed-off data with sc1 loads (st_wt / ld_wt above).
// No block ever waits on another, so residency/dispatch order cannot deadlock.  Tickets are
// reset by the final block (and zeroed when a bank is created or reset).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ bool ticket_last(unsigned* t, unsigned expected, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = old == expected - 1;
  }
  __syncthreads();
  return *flag != 0;
}

}  // namespace llampc

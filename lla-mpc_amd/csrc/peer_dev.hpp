// peer_dev.hpp — the cross-shard merge over records staged in LDS (merge_staged) and the peer
// mailbox exchange around it: poll_mailbox, the timeout record, and peer_finish, the exchange
// fused into the plan launch.  Included by plan_dev.hpp and by kernels.hip (merge_kernel,
// peer_exchange_kernel).
#pragma once
#include "dev_wave.hpp"
#include "final_dev.hpp"

namespace llampc {

// Cross-shard merge after the all-gather: one wave.  Scalars by lane-parallel reads and
// shuffles; the shards' sorted top-K lists by the LDS tree merge.  merge.hpp holds the
// same semantics as straight-line host code (llampc_merge); the tests check both agree.
// An entry of those lists: EntS (launch_shape.hpp).

// The merge proper over G records already staged in LDS at `rec` (their sorted top-K lists
// are ranked in `lists`, 2 G KMAX EntS); thread 0 writes the scalars, threads < KMAX the
// top-K.  `late` (the peer exchange gave up waiting) is or-ed into the status.
__device__ __forceinline__ void merge_staged(const llampc_plan_out* rec, int32_t G, int32_t nan_first,
                                             llampc_plan_out* m, EntS* lists, int32_t late) {
  const int tid = threadIdx.x;
  const int K = rec[0].K;
  const int M = G * K;
  EntS* buf0 = lists;
  EntS* buf1 = buf0 + M;
  for (int e = tid; e < M; e += kBlock) {
    const int g = e / K, j = e - g * K;
    const int64_t id = rec[g].topk[j] < 0 ? kNoIndex : rec[g].topk[j];
    buf0[e] = EntS{id == kNoIndex ? __builtin_nan("") : rec[g].topk_val[j], id, e, 0};
  }
  // wave 0: look-back argmin over the shards' local argmins; look-ahead best; counts; owners
  // — DPP wave reductions over lanes g < G (no LDS shuffles)
  double bv = nan_first ? __builtin_inf() : __builtin_nan("");
  int64_t bi = kNoIndex;
  double av = __builtin_nan("");
  int64_t akey = kNoIndex;              // (model << 24 | candidate): la_less's order
  int nf = 0;
  uint32_t owner_lb = kNoLocal, owner_sel = kNoLocal;
  if (tid < 64) {
    const int lane = tid;
    for (int g = lane; g < G; g += 64) {
      const llampc_plan_out& p = rec[g];
      if (p.lb_best >= 0 && key_less(nan_first, p.lb_best_val, p.lb_best, bv, bi)) {
        bv = p.lb_best_val;
        bi = p.lb_best;
      }
      nf += p.n_nonfinite;
      const int64_t k2 = p.la_best_model >= 0 ? ((int64_t)p.la_best_model << 24) | (uint32_t)p.la_best_cand : kNoIndex;
      if (k2 != kNoIndex && less_nan_last(p.la_best_cost, k2, av, akey)) {
        av = p.la_best_cost;
        akey = k2;
      }
    }
    if (nan_first) wave_min<1>(bv, bi);
    else wave_min<0>(bv, bi);
    wave_min<0>(av, akey);
    nf = wave_sum(nf);
    uint32_t ol = kNoLocal, os = kNoLocal;
    for (int g = lane; g < G; g += 64) {
      if (bi != kNoIndex && rec[g].lb_best == bi) ol = min(ol, (uint32_t)g);
      if (rec[g].sel_owned) os = min(os, (uint32_t)g);
    }
    owner_lb = wave_min_u32(ol);
    owner_sel = wave_min_u32(os);
  }
  const int64_t am = akey == kNoIndex ? kNoIndex : (akey >> 24);
  const int32_t ac = akey == kNoIndex ? INT32_MAX : (int32_t)(akey & 0xFFFFFF);
  __syncthreads();
  const EntS* r = tree_merge(buf0, buf1, G, K);
  if (tid < LLAMPC_KMAX) {
    const int k = tid;
    const bool have = k < K && r[k].i != kNoIndex;
    if (have) {                          // the merged entry carries its gathered position
      const int src = r[k].src, g = src / K, j = src - g * K;
      m->topk[k] = r[k].i;
      m->topk_val[k] = r[k].v;
      m->topk_Df[k] = rec[g].topk_Df[j];
      m->topk_Dr[k] = rec[g].topk_Dr[j];
      m->topk_cand[k] = rec[g].topk_cand[j];
      m->topk_cost[k] = rec[g].topk_cost[j];
    } else {
      m->topk[k] = -1;
      m->topk_val[k] = m->topk_Df[k] = m->topk_Dr[k] = m->topk_cost[k] =
          k < K ? __builtin_nan("") : 0.0;
      m->topk_cand[k] = -1;
    }
  }
  if (tid != 0) return;
  const llampc_plan_out& p0 = rec[0];
  m->window_count = p0.window_count;
  m->window_full = p0.window_full;
  m->K = K;
  int32_t st = late ? kPollTimeoutStatus : 0;
  for (int g = 0; g < G; ++g) st |= rec[g].status;
  m->status = st;
  m->lb_best = bi == kNoIndex ? -1 : bi;
  m->lb_best_val = bi == kNoIndex ? __builtin_nan("") : bv;
  if (m->window_full && owner_lb != kNoLocal) {
    m->sel_model = bi;
    m->sel_owned = rec[owner_lb].sel_owned;
    m->sel_cand = rec[owner_lb].sel_cand;
    m->sel_cost = rec[owner_lb].sel_cost;
  } else {                               // the first shard owning sel (merge.hpp)
    m->sel_model = p0.sel_model;
    m->sel_owned = owner_sel != kNoLocal;
    m->sel_cand = owner_sel != kNoLocal ? rec[owner_sel].sel_cand : -1;
    m->sel_cost = owner_sel != kNoLocal ? rec[owner_sel].sel_cost : __builtin_nan("");
  }
  m->la_best_model = am == kNoIndex ? -1 : am;
  m->la_best_cand = am == kNoIndex ? -1 : ac;
  m->la_best_cost = av;
  m->n_nonfinite = nf;
}

// Poll this rank's mailbox slots [G][kRecWords] (tick parity already applied) for the G-1 peer
// records of tick `seq`, unpacking the payloads into rec32 (LDS).  Every round issues ALL of a
// thread's loads before it checks any (unconditional loads — a load under a per-word
// condition gets its own branch and vmcnt(0) wait, i.e. one memory round trip per word: ~11
// sequential round trips per thread at G = 8); words already valid, past the end or in this
// rank's own slot (never read back) reload a harmless address in that own slot.  Returns 1 if
// `bound` s_memrealtime ticks pass first.
// A peer exchange that gave up waiting (a missing rank): the merged record is this rank's own
// record with status LLAMPC_STATUS_POLL_TIMEOUT (the missing slots hold no record to merge).
__device__ __forceinline__ void peer_timeout_record(const uint32_t* rec32, int rank, llampc_plan_out* m) {
  const uint32_t* mine = rec32 + (size_t)rank * kRecWords;
  uint32_t* dst = reinterpret_cast<uint32_t*>(m);
  constexpr int kStatus = (int)(offsetof(llampc_plan_out, status) / 4);
  for (int w = threadIdx.x; w < kRecWords; w += kBlock)
    dst[w] = w == kStatus ? (uint32_t)LLAMPC_STATUS_POLL_TIMEOUT : mine[w];
}

template <int kPer>
__device__ __forceinline__ int poll_mailbox(const uint64_t* own, int G, int rank, uint32_t seq,
                                            uint64_t bound, uint32_t* rec32) {
  static_assert(kPer <= 64, "one need bit per word");
  const int tid = threadIdx.x;
  const int total = G * kRecWords, skip0 = rank * kRecWords, skip1 = skip0 + kRecWords;
  const int idle = skip0 + tid % kRecWords;      // this thread's harmless address
  uint64_t need = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int e = tid + j * kBlock;
    if (e < total && (e < skip0 || e >= skip1)) need |= 1ull << j;
  }
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  while (need) {
    uint64_t v[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int e = ((need >> j) & 1) ? tid + j * kBlock : idle;
      v[j] = __hip_atomic_load(own + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
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

// Fused peer exchange, run by the block that completed this rank's record (after final_poll /
// final_select): the record's words are read back, pushed as tagged words into slot [seq & 1][rank] of every mailbox, and the
// px_G slots of this rank's mailbox are polled into LDS and merged (peer_exchange_kernel's
// protocol and merge; its comment has the slot-reuse argument).
__device__ __forceinline__ void peer_finish(const FinalLaunch& f, unsigned char* smem) {
  const int tid = threadIdx.x;
  const int G = f.px_G;
  constexpr int kW2 = kRecWords / 2;            // the record as 64-bit loads
  static_assert(kRecWords % 2 == 0, "record of whole 64-bit words");
  // The record is read back with sc1 loads after the block barrier.  This block wrote part
  // of it (final_write); on the ticket path lb_final wrote the rest in ANOTHER block, which
  // can sit on another XCD: every lb_final field is stored sc1 and every load here is sc1,
  // so the ticket hand-off is the "sc1 stores and loads both sides" form and no stale L2
  // line of last tick's record can be merged.  No agent-scope fence: on MI355X that is an
  // L2 writeback of the XCD (measured ~3 us per tick here).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const size_t slot0 = (size_t)(f.px_seq & 1) * G * kRecWords;
  const size_t mine = slot0 + (size_t)f.px_rank * kRecWords;
  const uint64_t* src = reinterpret_cast<const uint64_t*>(f.out);
  unsigned char* base = smem + 256;             // past the scratch the completion used
  uint32_t* rec32 = reinterpret_cast<uint32_t*>(base);
  uint64_t* rec_mine = reinterpret_cast<uint64_t*>(base + (size_t)f.px_rank * sizeof(llampc_plan_out));
  for (int w = tid; w < kW2; w += kBlock) {
    const uint64_t v = ld_wt(&src[w]);
    rec_mine[w] = v;                            // this rank's record: straight to LDS
    const uint64_t lo = tag_word(f.px_seq, (uint32_t)v), hi = tag_word(f.px_seq, (uint32_t)(v >> 32));
    for (int g = 0; g < G; ++g) {
      if (g == f.px_rank) continue;
      uint64_t* d = f.px_box[g] + mine + 2 * w;
      __hip_atomic_store(d, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(d + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  const uint64_t* own = f.px_box[f.px_rank] + slot0;
  constexpr int kPerF = (kPeerFuseMax * kRecWords + kBlock - 1) / kBlock;
  int late = poll_mailbox<kPerF>(own, G, f.px_rank, f.px_seq, (uint64_t)f.px_bound << 16, rec32);
  EntS* lists = reinterpret_cast<EntS*>(base + (size_t)G * sizeof(llampc_plan_out));
  int* wave_late = reinterpret_cast<int*>(lists + 2 * (size_t)G * LLAMPC_KMAX);
  const int wl = __any(late);
  if ((tid & 63) == 0) wave_late[tid >> 6] = wl;
  __syncthreads();
  late = 0;
  for (int w = 0; w < kWaves; ++w) late |= wave_late[w];
  if (late) {                                   // block-uniform
    peer_timeout_record(rec32, f.px_rank, f.px_merged);
    return;
  }
  merge_staged(reinterpret_cast<const llampc_plan_out*>(base), G, f.nan_first, f.px_merged, lists, 0);
}

}  // namespace llampc

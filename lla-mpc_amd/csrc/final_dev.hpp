// final_dev.hpp — the completion stages run by ticket winners inside a launch: the LDS merge
// path / tree merge, lb_final (the look-back blocks' lists into the selection) and the record's
// completion from the look-ahead results (final_select by ticket, final_poll by tagged words).
// Included by peer_dev.hpp, plan_dev.hpp and ctl.hip.
#pragma once
#include "dev_stamps.hpp"
#include "dev_wave.hpp"
#include "lookback_dev.hpp"

namespace llampc {

__device__ __forceinline__ bool ent_less(const Ent& x, const Ent& y) {
  return less_nan_last(x.v, x.i, y.v, y.i);
}

// Element k (0-based) of merge(A, B), |A| = |B| = K, both sorted with sentinel padding:
// co-rank binary search (merge path), ~log2(K) dependent LDS reads.  E has fields v, i.
template <typename E>
__device__ __forceinline__ E merge_path_at(const E* A, const E* B, int K, int k) {
  int lo = 0, hi = k;                       // i = elements taken from A before output k
  while (lo < hi) {
    const int i = (lo + hi) >> 1;
    if (less_nan_last(A[i].v, A[i].i, B[k - i - 1].v, B[k - i - 1].i)) lo = i + 1;
    else hi = i;
  }
  const int i = lo, j = k - lo;
  return (less_nan_last(A[i].v, A[i].i, B[j].v, B[j].i)) ? A[i] : B[j];
}

// Tree-merge L sorted K-lists in LDS (the cross-shard merge_kernel) (buf0 holds them; buf1
// same size); every output element of a level is computed by its own thread.  Returns the
// buffer holding the merged list (first K entries).
template <typename E>
__device__ __forceinline__ E* tree_merge(E* buf0, E* buf1, int L, int K) {
  E* src = buf0;
  E* dst = buf1;
  while (L > 1) {
    const int P = (L + 1) >> 1;
    for (int t = threadIdx.x; t < P * K; t += blockDim.x) {
      const int p = t / K, k = t - p * K;
      const E* A = src + (size_t)(2 * p) * K;
      dst[t] = (2 * p + 1 < L) ? merge_path_at(A, A + K, K, k) : A[k];
    }
    __syncthreads();
    E* tmp = src;
    src = dst;
    dst = tmp;
    L = P;
  }
  return src;
}

// ------------------------------------------------------------------------------------
// Completion stages run by ticket winners inside the plan launch.
// lb_final  (last look-back block): argmin over the blocks' argmins; tree merge of the
//           blocks' sorted top-K lists in LDS; writes the look-back fields of the record.
//           It runs while look-ahead blocks are still rolling out, off the critical path.
// final     (last block overall): look-ahead best over the block partials, the selected
//           model's choice, each top-K model's best candidate; completes the record.
// ------------------------------------------------------------------------------------
// The controller tick's use of lb_final (SEL = true, ctl.hip): the selection is also published
// for the look-ahead blocks waiting on it — tagged words [K + 1] (local model index of top-K
// entry k, kNoLocal = none; entry K: the argmin) — and kept in LDS for the completion.
// SEL = 2 (the sharded controller, ctl_complete_dev.hpp ctl_exchange): nothing is published and no record
// field written — the shard's top-K and argmin (local index, value) go to ids / xv for the
// exchange, which publishes the MERGED selection.
struct CtlSel {
  uint64_t* tag;
  uint32_t seq;
  uint32_t* ids;         // LDS [K + 1]
  double* dr;            // LDS [K]: bank Dr / Df of the top-K (NaN: none)
  double* df;
  double* xv;            // LDS [K + 1]: SEL = 2, the entries' window means
  int32_t* xlate;        // LDS [1]: the exchange gave up waiting for a peer (status)
};

template <int SEL = 0>
__device__ __forceinline__ void lb_final(const FinalLaunch& f, unsigned char* smem, const CtlSel* cs = nullptr) {
  STAMP(0);
  const int tid = threadIdx.x;
  const int L = f.nb_lb;                   // one sorted K-list per look-back block
  const int La = f.nb_lb * kWaves;         // one argmin per look-back wave
  const int K = f.K, M = L * K;
  // LDS (SoA, contiguous scans): thr[2] | key[M] | val[M] | hk[L] | ck[M] | am[La] | id[M] |
  // hid[L] | cid[M] | ce[M] | top[KMAX] | cnt.  Missing entries
  // take ids above every model's, unique per position, so (key, id) is a total order.
  uint64_t* thr = reinterpret_cast<uint64_t*>(smem + kScratchBytes);   // T: key, id
  uint64_t* key = thr + 2;
  double* val = reinterpret_cast<double*>(key + M);
  uint64_t* hk = reinterpret_cast<uint64_t*>(val + M);
  uint64_t* ck = hk + L;
  Ent* am = reinterpret_cast<Ent*>(ck + M);    // the waves' argmins, same round trip
  uint32_t* id = reinterpret_cast<uint32_t*>(am + La);
  uint32_t* hid = id + M;
  uint32_t* cid = hid + L;
  int* ce = reinterpret_cast<int*>(cid + M);
  int* top = ce + M;                           // [K] entry of each output rank
  int* cnt = top + LLAMPC_KMAX;
  auto local = [&](int64_t gi) { return gi == kNoIndex ? kNoLocal : (uint32_t)(gi - f.goff); };
  for (int e = tid; e < M; e += kBlock) {
    const double v = ld_wt(&f.tk_val[e]);
    const uint32_t l = local(ld_wt(&f.tk_idx[e]));
    const uint64_t k = l == kNoLocal ? ~0ull : order_key(v);
    // e >= 512 (M up to 640): the id wraps past 2^32 to e - 512.  It stays unique among the missing
    // entries (M < 2^32) and never reaches the output: only missing entries carry key ~0 (a NaN's
    // key is below it) and M > 512 takes L >= 17 blocks, so more than 4096 >= K models: the K
    // entries top[] names are real ones, which rank below every missing one under (key, id), and the
    // `id >= kNoModelId` test below is never asked about a wrapped id
    // (tests/test_lookback_matrix_gpu.py, the n4869-k32 rows: M = 640, 27 missing entries at e >= 613).
    const uint32_t i = l == kNoLocal ? kNoModelId + (uint32_t)e : l;
    key[e] = k;
    val[e] = v;
    id[e] = i;
    if (e % K == 0) {
      hk[e / K] = k;
      hid[e / K] = i;
    }
  }
  for (int b = tid; b < La; b += kBlock) am[b] = Ent{ld_wt(&f.am_val[b]), ld_wt(&f.am_idx[b])};
  if (tid == 0) {
    *cnt = 0;
    thr[0] = ~0ull;                          // L < K: every entry is a candidate
    thr[1] = 0xFFFFFFFFull;
  }
  __syncthreads();
  STAMP(1);
  // top-K of the L sorted lists without serial rounds (a wave pick per output rank cost
  // ~1 us per rank): T = the K-th smallest list head bounds the K-th smallest entry (the K
  // smallest heads are K entries <= T), so the top-K lies in {entries <= T} — K to a few K
  // entries on real banks — and each candidate's rank among the candidates is its output
  // rank.  The scans read contiguous LDS (broadcast), unrolled so loads overlap.
  auto lt = [](uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    return (int)(ka < kb) | ((int)(ka == kb) & (int)(ia < ib));
  };
  if (L >= K) {
    for (int h = tid; h < L; h += kBlock) {
      const uint64_t mk = hk[h];
      const uint32_t mi = hid[h];
      int r = 0;
#pragma unroll 8
      for (int j = 0; j < L; ++j) r += lt(hk[j], hid[j], mk, mi);
      if (r == K - 1) {
        thr[0] = mk;
        thr[1] = mi;
      }
    }
    __syncthreads();
  }
  STAMP(6);
  const uint64_t tk = thr[0];
  const uint32_t ti = (uint32_t)thr[1];
  for (int e = tid; e < M; e += kBlock) {
    const uint64_t k = key[e];
    const uint32_t i = id[e];
    if (!lt(tk, ti, k, i)) {
      const int slot = atomicAdd(cnt, 1);
      ck[slot] = k;
      cid[slot] = i;
      ce[slot] = e;
    }
  }
  __syncthreads();
  STAMP(7);
  const int c = *cnt;                      // >= K (the K smallest heads, or all M >= K)
  for (int q = tid; q < c; q += kBlock) {
    const uint64_t mk = ck[q];
    const uint32_t mi = cid[q];
    int r = 0;
#pragma unroll 8
    for (int j = 0; j < c; ++j) r += lt(ck[j], cid[j], mk, mi);
    if (r < K) top[r] = ce[q];
  }
  __syncthreads();
  if (tid >= 64) return;                   // one wave finishes; the caller re-converges
  const int lane = tid;
  // argmin over the waves' argmins (rt.py:359)
  double v = f.nan_first ? __builtin_inf() : __builtin_nan("");
  uint32_t li = kNoLocal;
  for (int b = lane; b < La; b += 64) {
    const double bv = am[b].v;
    const uint32_t bl = local(am[b].i);
    const bool t = (int)(bl != kNoLocal) &
                   (int)(f.nan_first ? less_bf<1>(bv, bl, v, li) : less_bf<0>(bv, bl, v, li));
    v = t ? bv : v;
    li = t ? bl : li;
  }
  if (f.nan_first) wave_pick_nf(v, li);
  else wave_pick_nl(v, li);
  double kv = __builtin_nan("");
  uint32_t kl = kNoLocal;
  if (lane < K) {
    const int e = top[lane];
    kl = id[e] >= kNoModelId ? kNoLocal : id[e];
    kv = val[e];
  }
  STAMP(2);
  if constexpr (SEL == 2) {                // the sharded controller: the shard's lists only
    if (lane < K) {
      cs->ids[lane] = kl;
      cs->xv[lane] = kv;
    }
    if (lane == 0) {
      cs->ids[K] = li;
      cs->xv[K] = v;
    }
    return;
  }
  if constexpr (SEL == 1) {                // the controller's selection first: the look-ahead
    if (lane < K) {                        // blocks wait on it (the record's stores below wait
      cs->ids[lane] = kl;                  // on the Pacejka loads of the top-K rows)
      st_wt(&cs->tag[lane], tag_word(cs->seq, kl));
    }
    if (lane == 0) {
      cs->ids[K] = li;
      st_wt(&cs->tag[K], tag_word(cs->seq, li));
    }
  }
  // Every record field is stored write-through (sc1): on the ticket path another block —
  // possibly on another XCD — completes the record, and peer_finish reads all of it back
  // with sc1 loads (MI355X_MICROARCH.md "Valid forms": sc1 stores AND sc1 loads).
  llampc_plan_out* o = f.out;
  if (lane < LLAMPC_KMAX) {
    const int k = lane;
    if (k < K && kl != kNoLocal) {
      st_wt(&o->topk[k], f.goff + (int64_t)kl);      // read by final_select
      st_wt(&o->topk_val[k], kv);
      st_wt(&o->topk_Df[k], f.params[2 * f.n + kl]);
      st_wt(&o->topk_Dr[k], f.params[5 * f.n + kl]);
    } else {
      const double nan = __builtin_nan("");
      st_wt(&o->topk[k], (int64_t)-1);
      st_wt(&o->topk_val[k], nan);
      st_wt(&o->topk_Df[k], nan);
      st_wt(&o->topk_Dr[k], nan);
    }
  }
  if (lane == 0) {
    st_wt(&o->lb_best, li == kNoLocal ? (int64_t)-1 : f.goff + (int64_t)li);
    st_wt(&o->lb_best_val, li == kNoLocal ? __builtin_nan("") : v);
  }
  if constexpr (SEL == 1) {
    if (lane < K) {
      const bool have = kl != kNoLocal;
      cs->dr[lane] = have ? f.params[5 * f.n + kl] : __builtin_nan("");
      cs->df[lane] = have ? f.params[2 * f.n + kl] : __builtin_nan("");
    }
  }
}

// Completes the record from the gathered look-ahead results (final_select / final_poll).
__device__ __forceinline__ void final_write(const FinalLaunch& f, bool lb, int64_t sel, bool owned,
                                            int32_t kcand, double kcost, int32_t scand,
                                            double scost, double lav, int64_t lai, int nf,
                                            int status = 0) {
  const int tid = threadIdx.x;
  llampc_plan_out* o = f.out;
  const double nan = __builtin_nan("");
  // The look-ahead best's (model, candidate) from its key (goff + n) C + c, ahead of the stores (none
  // of them waits for it): at C = 1 the key is the model; else split_key, not the 64-bit / and %, whose
  // ~150-instruction software sequence is one lane's dependent chain between the poll and the record.
  // No look-ahead best (-1, -1, NaN) without a look-ahead, without a key, and when the best cost is NaN:
  // the picks order NaN last, so lav is NaN only if every (model, candidate) cost of the tick is.  (+inf
  // is a cost: every pair infeasible still gives (0, 0, +inf), llampc.h.)
  const bool la_ok = f.do_la && lai != kNoIndex && lav == lav;
  int64_t lam = -1;
  int32_t lac = -1;
  if (la_ok) {
    if (f.C == 1) {
      lam = lai;
      lac = 0;
    } else {
      split_key(lai, f.C, lam, lac);
    }
  }
  // sc1 stores like lb_final's: the fused peer exchange reads the whole record back sc1
  if (tid < LLAMPC_KMAX) {
    const int k = tid;
    if (!lb) {
      st_wt(&o->topk[k], (int64_t)-1);
      st_wt(&o->topk_val[k], nan);
      st_wt(&o->topk_Df[k], nan);
      st_wt(&o->topk_Dr[k], nan);
    }
    st_wt(&o->topk_cand[k], kcand);
    st_wt(&o->topk_cost[k], kcost);
  }
  if (tid == 0) {
    if (!lb) {
      st_wt(&o->lb_best, (int64_t)-1);
      st_wt(&o->lb_best_val, nan);
    }
    st_wt(&o->window_count, f.window_count);
    st_wt(&o->window_full, f.full);
    st_wt(&o->K, f.K);
    st_wt(&o->n_nonfinite, nf);
    st_wt(&o->status, status);
    st_wt(&o->sel_model, sel);
    st_wt(&o->sel_owned, (int32_t)owned);
    st_wt(&o->sel_cand, scand);
    st_wt(&o->sel_cost, scost);
    st_wt(&o->la_best_model, lam);
    st_wt(&o->la_best_cand, lac);
    st_wt(&o->la_best_cost, la_ok ? lav : nan);
    __hip_atomic_store(&f.tickets[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&f.tickets[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // every look-ahead block has published (polled) or drawn its ticket (ticket path) after
    // its last work-queue take: the next launch starts from unit 0
    if (f.wq) __hip_atomic_store(f.wq, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (f.host_tag) {                     // host completion: every record store performed, then the tag
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(f.host_tag, f.host_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  STAMP(5);
#ifdef LLAMPC_STAMPS
  if (tid == 0) g_stamp_launch++;
#endif
}

__device__ __forceinline__ void final_select(const FinalLaunch& f, const Scratch& sc) {
  STAMP(3);
  const int tid = threadIdx.x;
  llampc_plan_out* o = f.out;
  const bool lb = f.do_lb && f.full;
  // Every load that does not depend on the look-ahead reduction is issued first, so the
  // tail costs two dependent round trips, not three: the look-back result lb_final left in
  // the record (top-K ids, lb_best) and then those models' best candidates.
  const int64_t idk = (lb && tid < LLAMPC_KMAX) ? ld_wt(&o->topk[tid]) : -1;
  const int64_t lbi = (tid == 0 && lb) ? ld_wt(&o->lb_best) : -1;
  const int64_t sel = lbi >= 0 ? lbi : f.current_model;
  const bool owned = sel >= f.goff && sel < f.goff + f.n;
  const bool have = lb && tid < LLAMPC_KMAX && idk >= 0 && f.do_la;
  int32_t kcand = -1, scand = -1;
  double kcost = __builtin_nan(""), scost = __builtin_nan("");
  if (have) {
    kcand = ld_wt(&f.best_cand[idk - f.goff]);
    kcost = ld_wt(&f.best_cost[idk - f.goff]);
  }
  if (tid == 0 && owned && f.do_la) {
    scand = ld_wt(&f.best_cand[sel - f.goff]);
    scost = ld_wt(&f.best_cost[sel - f.goff]);
  }
  double lav = __builtin_nan("");
  int64_t lai = kNoIndex;
  int nf = 0;
  if (f.do_la) {
    for (int b = tid; b < f.nb_la; b += kBlock) {
      nf += ld_wt(&f.pnf[b]);
      const int64_t pi = ld_wt(&f.pidx[b]);
      const double pv = ld_wt(&f.pv[b]);
      const bool t = (int)(pi != kNoIndex) & (int)less_bf<0>(pv, pi, lav, lai);
      lav = t ? pv : lav;
      lai = t ? pi : lai;
    }
    wave_pick_nl64(lav, lai);           // converged: every lane of the block is here
    nf = wave_sum(nf);
    if ((tid & 63) == 0) {
      sc.sv[4 + (tid >> 6)] = lav;
      sc.si[4 + (tid >> 6)] = lai;
      sc.sn[tid >> 6] = nf;
    }
    __syncthreads();
    lav = sc.sv[4];
    lai = sc.si[4];
    nf = sc.sn[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      const bool t = (int)(sc.si[4 + w] != kNoIndex) & (int)less_bf<0>(sc.sv[4 + w], sc.si[4 + w], lav, lai);
      lav = t ? sc.sv[4 + w] : lav;
      lai = t ? sc.si[4 + w] : lai;
      nf += sc.sn[w];
    }
  }
  STAMP(4);
  final_write(f, lb, sel, owned, kcand, kcost, scand, scost, lav, lai, nf);
}

// Polled completion (f.poll): run by the look-back ticket winner after lb_final.  Each thread
// spins on its share of the tagged words — the look-ahead blocks' partials (5 words each),
// the top-K models' and the selected model's results (3 words each) — until every word it
// loads carries this launch's tag; one block barrier then joins them.  The blocks it waits
// for never wait, so it cannot deadlock; a bound (f.poll x 2^16 s_memrealtime ticks, 100 MHz,
// scaled by the host with the launch's rollout steps: poll_bound_ticks in capi.hip) ends a
// poll that could never finish (a bug) with status LLAMPC_STATUS_POLL_TIMEOUT in the record
// instead of a hang.
constexpr int kPollTimeoutStatus = LLAMPC_STATUS_POLL_TIMEOUT;
__device__ __forceinline__ void final_poll(const FinalLaunch& f, const Scratch& sc) {
  STAMP(3);
  const int tid = threadIdx.x;
  llampc_plan_out* o = f.out;
  const bool lb = f.do_lb && f.full;
  const int64_t idk = (lb && tid < LLAMPC_KMAX) ? ld_wt(&o->topk[tid]) : -1;
  const int64_t lbi = (tid == 0 && lb) ? ld_wt(&o->lb_best) : -1;
  const int64_t sel = lbi >= 0 ? lbi : f.current_model;
  const bool owned = sel >= f.goff && sel < f.goff + f.n;
  // this thread's model record: top-K entry tid, or (thread 0's second slot) the selection
  const int64_t mk = (lb && tid < LLAMPC_KMAX && idk >= 0) ? idk - f.goff : -1;
  const int64_t ms = (tid == 0 && owned) ? sel - f.goff : -1;
  const int nbt = (f.nb_la + kBlock - 1) / kBlock;        // block records per thread
  uint64_t kw[3] = {0, 0, 0}, sw[3] = {0, 0, 0};
  double lav = __builtin_nan("");
  int64_t lai = kNoIndex;
  int nf = 0;
  int status = 0;
  // every thread spins on its own words (no block barrier per round: a thread's next loads
  // issue as soon as its previous ones return); one barrier after all are current
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  const uint64_t bound = (uint64_t)(uint32_t)f.poll << 16;
  bool late = false;
  if (mk >= 0) {
    for (;;) {
#pragma unroll
      for (int w = 0; w < 3; ++w) kw[w] = ld_wt(&f.la_tag[w * f.n + mk]);
      if ((int)tag_ok(kw[0], f.seq) & (int)tag_ok(kw[1], f.seq) & (int)tag_ok(kw[2], f.seq)) break;
      if (__builtin_amdgcn_s_memrealtime() - t0 > bound) { late = true; break; }
    }
  }
  if (ms >= 0) {
    for (;;) {
#pragma unroll
      for (int w = 0; w < 3; ++w) sw[w] = ld_wt(&f.la_tag[w * f.n + ms]);
      if ((int)tag_ok(sw[0], f.seq) & (int)tag_ok(sw[1], f.seq) & (int)tag_ok(sw[2], f.seq)) break;
      if (__builtin_amdgcn_s_memrealtime() - t0 > bound) { late = true; break; }
    }
  }
  for (int j = 0; j < nbt; ++j) {
    const int b = tid + j * kBlock;
    if (b < f.nb_la) {
      uint64_t r[5];
      for (;;) {
#pragma unroll
        for (int w = 0; w < 5; ++w) r[w] = ld_wt(&f.blk_tag[5 * (int64_t)b + w]);
        if ((int)tag_ok(r[0], f.seq) & (int)tag_ok(r[1], f.seq) & (int)tag_ok(r[2], f.seq) &
            (int)tag_ok(r[3], f.seq) & (int)tag_ok(r[4], f.seq))
          break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > bound) { late = true; break; }
      }
      const double pv = __longlong_as_double((long long)join_words(r[0], r[1]));
      const int64_t pi = (int64_t)join_words(r[2], r[3]);
      nf += (int)(uint32_t)r[4];
      const bool t = (int)(pi != kNoIndex) & (int)less_bf<0>(pv, pi, lav, lai);
      lav = t ? pv : lav;
      lai = t ? pi : lai;
    }
  }
  // the waves' late flags travel with the block reduction's LDS exchange below (one barrier;
  // no __syncthreads_or: its static LDS would break the launches' full-LDS requests)
  unsigned char* late_w = reinterpret_cast<unsigned char*>(sc.sv) + kLateOff;
  const int wlate = __any((int)late);
  int32_t kcand = -1, scand = -1;
  double kcost = __builtin_nan(""), scost = __builtin_nan("");
  if (mk >= 0 && f.do_la) {
    kcost = __longlong_as_double((long long)join_words(kw[0], kw[1]));
    kcand = (int32_t)(uint32_t)kw[2];
  }
  if (ms >= 0 && f.do_la) {
    scost = __longlong_as_double((long long)join_words(sw[0], sw[1]));
    scand = (int32_t)(uint32_t)sw[2];
  }
  wave_pick_nl64(lav, lai);
  nf = wave_sum(nf);
  if ((tid & 63) == 0) {
    sc.sv[4 + (tid >> 6)] = lav;
    sc.si[4 + (tid >> 6)] = lai;
    sc.sn[tid >> 6] = nf;
    late_w[tid >> 6] = (unsigned char)wlate;
  }
  __syncthreads();
  lav = sc.sv[4];
  lai = sc.si[4];
  nf = sc.sn[0];
  int anyl = late_w[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    const bool t = (int)(sc.si[4 + w] != kNoIndex) & (int)less_bf<0>(sc.sv[4 + w], sc.si[4 + w], lav, lai);
    lav = t ? sc.sv[4 + w] : lav;
    lai = t ? sc.si[4 + w] : lai;
    nf += sc.sn[w];
    anyl |= late_w[w];
  }
  if (anyl) status = kPollTimeoutStatus;
  STAMP(4);
  final_write(f, lb, sel, owned, kcand, kcost, scand, scost, lav, lai, nf, status);
}

}  // namespace llampc

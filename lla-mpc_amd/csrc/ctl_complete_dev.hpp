// ctl_complete_dev.hpp — what the look-back ticket winner runs after lb_final: the sharded
// controller's exchange of the selection (ctl_rec_word, ctl_px_send, ctl_exchange) and the
// tick's completion (ctl_complete: projection, mu-hat, the slots' results, the record and the
// state).  Block 0 alone runs the completion on ticks without a look-back.  Included by ctl.hip only.
#pragma once
#include "ctl_cand_dev.hpp"
#include "ctl_door_dev.hpp"
#include "ctl_lds.hpp"
#include "final_dev.hpp"

namespace llampc {

// ------------------------------------------------------------------------------------
// The completing block (after lb_final<true>, or alone on ticks without a look-back).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void ctl_complete(const CtlLaunch& c, unsigned char* smem, const CtlSel& cs,
                                             const double* xt) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const int H = c.la.H, C = c.la.C;
  unsigned char* pl = smem + c.poll_off;
  double* pdist = reinterpret_cast<double*>(pl);                  // [16]
  double* pcost = reinterpret_cast<double*>(pl + 128);            // [kCtlSlotsMax]
  int32_t* pcand = reinterpret_cast<int32_t*>(pl + 448);          // [kCtlSlotsMax]
  int32_t* pnf = reinterpret_cast<int32_t*>(pl + 608);            // [kCtlSlotsMax]
  double* pmu = reinterpret_cast<double*>(pl + 768);              // dr, df, mu_pred, mu_used
  int32_t* pmisc = reinterpret_cast<int32_t*>(pl + 1792);         // projidx
  double* cu = reinterpret_cast<double*>(smem + kScratchBytes);   // [C][H][2] (lb_final's region, dead)
  unsigned char* late_w = smem + kLateOff;
  CtlState* st = c.st;
  const bool warm = c.warm != 0;
  // the spec list (CtlLaunch.n_spec): a slot whose model is on it reads the spec block's words
  uint32_t* spec_ids = reinterpret_cast<uint32_t*>(pl + 3648);    // [kCtlSpecMax]
  if (tid < c.n_spec) {
    int unused = 0;                     // a list that never comes: no model is on it
    spec_ids[tid] = poll_tag(c.spec_tag, tid, c.seq, c.poll, unused);
  }
  // Before the poll (the look-ahead blocks' rollouts take most of the launch) everything that
  // does not need their results: the projection, mu-hat and every candidate after its rate
  // clip (the look-ahead blocks' generator), so the chosen sequence is a copy after the poll.
  // The state is only read here; it is written after the poll, when no block reads it.
  const int p0 = st->projidx;
  const int segs = ctl_segments(p0, c.np);
  if (tid < kCtlSegs && tid < segs)                                // track.py:155-157
    pdist[tid] = ref_project_dist(xt[0], xt[1], c.pts[p0 + tid], c.pts[c.np + p0 + tid],
                                  c.pts[p0 + tid + 1], c.pts[c.np + p0 + tid + 1]);
  const double up0 = st->u_prev[0], up1 = st->u_prev[1];
  {
    const double* prev_seq = st->has_seq ? &st->useq[0][0] : nullptr;
    ctl_draw(c, prev_seq, up0, up1, cu, tid, kBlock);
  }
  __syncthreads();
  for (int t = tid; t < 2 * C; t += kBlock) {
    const int j = t & 1;
    ctl_rate_chain(cu + 2 * (size_t)(t >> 1) * H + j, H, j ? up1 : up0, j ? c.rate[1] : c.rate[0]);
  }
  if (tid == kBlock - 1) {
    pmisc[0] = segs >= 1 ? p0 + np_argmin(pdist, segs) : p0;      // planner.py:26-27
    // mu-hat (rt.py:326-344): the warm-up split with g = 9.8, else the top-K means
    const double mass = c.la.veh.mass, lf = c.la.veh.lf, lr = c.la.veh.lr;
    double dr, df;
    if (warm) {
      dr = c.mu_init * mass * 9.8 * lr / (lf + lr);
      df = c.mu_init * mass * 9.8 * lf / (lf + lr);
    } else {
      int kk = 0;
      while (kk < c.K && cs.ids[kk] != kNoLocal) ++kk;
      dr = np_pairwise_ring(cs.dr, 0, kk, LLAMPC_KMAX) / kk;
      df = np_pairwise_ring(cs.df, 0, kk, LLAMPC_KMAX) / kk;
    }
    // the histories are read and written by this block only (the look-ahead blocks read
    // mu_pred, which is written after the poll)
    const int cnt = st->hist_count;
    const int S = c.S;
    st->dr_hist[cnt % S] = dr;
    st->df_hist[cnt % S] = df;
    st->hist_count = cnt + 1;
    const int tot = cnt + 1, nl = tot < S ? tot : S, first = (tot - nl) % S;
    const double mu_old = ld_wt(&st->mu_pred);
    double mu_pred = mu_old;
    if (!warm)                                                     // rt.py:341
      mu_pred = (np_pairwise_ring(st->dr_hist, first, nl, S) / nl + np_pairwise_ring(st->df_hist, first, nl, S) / nl) /
                (9.81 * mass);
    pmu[0] = dr;
    pmu[1] = df;
    pmu[2] = mu_pred;
    pmu[3] = c.use_mu ? mu_old : c.mu_fixed;                       // the mu this tick's walk used
  }
  // the current model (this block writes it after the poll): loaded now, off the tail
  const int64_t cur_model = (tid < 64 && warm) ? st->current_model : 0;
  // x_prev: every look-back block has read it (this block holds the last ticket) and the
  // look-ahead blocks never do — stored now, so no load of x_t sits behind the record's host
  // stores after the poll
  if (tid < 6) st->x_prev[tid] = xt[tid];
  // the record's scalar kernel arguments, loaded (and kept) before the poll: the tail used
  // to wait for them one by one after it
  // (readfirstlane: launch-uniform values in SGPRs whatever the argument's copy)
  auto rfl = [](int32_t v) { return (int32_t)__builtin_amdgcn_readfirstlane(v); };
  auto rfl64 = [](int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
  };
  int32_t a_wc = rfl(c.fin.window_count), a_full = rfl(c.fin.full), a_K = rfl(c.K), a_warm = rfl(c.warm),
          a_lap = rfl(c.lap_projidx);
  int64_t a_goff = rfl64(c.sel_goff), a_tick = rfl64((int64_t)c.tick);
  double a_scale = __longlong_as_double((long long)rfl64(__double_as_longlong(c.use_mu ? c.v_factor : c.scale_fixed)));
  asm volatile("" : "+s"(a_wc), "+s"(a_full), "+s"(a_K), "+s"(a_warm), "+s"(a_lap));
  asm volatile("" : "+s"(a_goff), "+s"(a_tick), "+s"(a_scale));
  // waves 1-3 draw the next tick's variates while wave 0 polls (off every critical path)
  if (tid >= 64) ctl_draw_next(c, tid - 64, kBlock - 64);
  // every slot's result (tagged words of the look-ahead blocks)
  int late = 0;
  if (tid < c.nslots) {
    const uint64_t* src = c.slot_tag + 4 * (size_t)tid;
    if (c.n_spec && !warm) {
      const uint32_t id = cs.ids[tid];
      for (int p = 0; p < c.n_spec; ++p)
        if (id != kNoLocal && spec_ids[p] == id) src = c.spec_res + 4 * (size_t)p;
    }
    read_slot(src, c.seq, c.poll, late, pcost, pcand, pnf, tid);
  }
  const int wl = __any(late);
  if ((tid & 63) == 0) late_w[tid >> 6] = (unsigned char)wl;
  __syncthreads();
  CTL_STAMP(blockIdx.x, 8);
  // the record and the state
  const int ss = warm ? 0 : c.K;                                   // the selected model's slot
  const int scand = pcand[ss] >= 0 ? pcand[ss] : 0;
  // (assembling the record in LDS and copying it with 16-B stores made the system fence wait
  // ~2 us for the ~100 wide host stores: +1 us on the tail, profiles/r04/s4/ctl_phases_image.txt)
  llampc_ctl_out* o = c.out;
  llampc_plan_out* po = &o->plan;
  const double nan = __builtin_nan("");
  // the top-K's candidates (wave 1) and the chosen sequence (waves 2-3) while wave 0 forms the
  // record's words: every wave issues its own stores into the pinned record (one wave issuing
  // them all in turn put ~1 us before the words, profiles/r05/spec2/phases_armed.txt)
  if (tid >= 64 && tid < 64 + LLAMPC_KMAX) {
    const int k = tid - 64;
    const bool have = !warm && k < c.K;
    if (warm) {                         // no look-back selection yet (lb_final did not run)
      po->topk[k] = -1;
      po->topk_val[k] = po->topk_Df[k] = po->topk_Dr[k] = nan;
    }
    po->topk_cand[k] = have ? pcand[k] : -1;
    po->topk_cost[k] = have ? pcost[k] : nan;
  }
  if (tid >= 128 && tid < 128 + 2 * H) {   // the chosen sequence: candidate sel_cand
    const int e = tid - 128;
    const double v = cu[2 * (size_t)scand * H + e];
    (&o->u_seq[0][0])[e] = v;
    (&st->useq[0][0])[e] = v;
    if (e < 2) st->u_prev[e] = v;
  }
  CTL_STAMP(blockIdx.x, 12);
  if (tid < 64) {
    // wave 0: the look-ahead best over the rolled-out slots (flattened (model, candidate)
    // order, NaN last, ties to the lower key) as a wave pick, then the record's scalars as
    // one 8-byte word per lane — one store instruction into the pinned host record (thread 0
    // storing the ~25 fields one by one over PCIe took ~4 us, profiles/r04/ctl_record_split.txt)
    const int q = tid;
    const bool slot = q < c.nslots;
    const bool valid = slot && !warm && pcand[q] >= 0 && cs.ids[q] != kNoLocal;
    double lav = valid ? pcost[q] : nan;
    int64_t lai = valid ? (a_goff + (int64_t)cs.ids[q]) * C + pcand[q] : kNoIndex;
    wave_pick_nl64(lav, lai);
    const int nf = wave_sum(slot ? pnf[q] : 0);
    int anyl = *cs.xlate;                // the sharded exchange gave up on a peer
    for (int w = 0; w < kWaves; ++w) anyl |= late_w[w];
    const int64_t sel = warm ? cur_model : a_goff + (int64_t)cs.ids[a_K];
    const double dr = pmu[0], df = pmu[1], mu_pred = pmu[2];
    int pj = pmisc[0];
    if (pj > a_lap) pj = 0;                                        // rt.py:287-296
    int64_t lm;
    int32_t lc;
    split_key(lai == kNoIndex ? 0 : lai, C, lm, lc);
    auto pack = [](int32_t lo, int32_t hi) { return (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32); };
    auto bits = [](double v) { return (uint64_t)__double_as_longlong(v); };
    // llampc_plan_out words 0..9 (lb_best / lb_best_val, words 2 and 3, are lb_final's unless
    // warm), then llampc_ctl_out's words after the plan record (static_asserts below)
    // every word uniform, each lane selects its own (no per-lane branches)
    const uint64_t W[17] = {pack(a_wc, a_full),
                            pack(a_K, 1),                                  // sel_owned
                            (uint64_t)(int64_t)-1,
                            bits(nan),
                            (uint64_t)sel,
                            pack(pcand[ss], nf),
                            bits(pcost[ss]),
                            (uint64_t)(lai == kNoIndex ? (int64_t)-1 : lm),
                            pack(lai == kNoIndex ? -1 : lc, anyl ? kPollTimeoutStatus : 0),
                            bits(lai == kNoIndex ? nan : lav),
                            (uint64_t)a_tick,
                            pack(pj, a_warm),
                            bits(pmu[3]),                                  // mu_used
                            bits(a_scale),
                            bits(mu_pred),
                            bits(dr),
                            bits(df)};
    uint64_t w = W[0];
#pragma unroll
    for (int i = 1; i < 17; ++i) w = q == i ? W[i] : w;
    const bool store = q < 17 && (warm || (q != 2 && q != 3));
    uint64_t* dst = q < 10 ? reinterpret_cast<uint64_t*>(po) + q : reinterpret_cast<uint64_t*>(&o->tick) + (q - 10);
    CTL_STAMP(blockIdx.x, 13);
    if (store) *dst = w;
    if (q == 0) {
      st->mu_pred = mu_pred;
      st->projidx = pj;
      st->has_seq = 1;
      if (!warm) st->current_model = sel;
      __hip_atomic_store(&c.tickets[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  CTL_STAMP(blockIdx.x, 11);
  if (tid == 0)                        // x_t on the device -> the record's stores issued (ctl.hpp)
    __hip_atomic_store(c.host_tag + 1, (uint64_t)__builtin_amdgcn_s_memrealtime() - ld_wt(&c.door_dev[kCtlTimeWord]),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();              // ~0.4 us (a plain vmcnt wait: ~0.3, ctl_record_split.txt)
  __syncthreads();
  CTL_STAMP(blockIdx.x, 9);
  if (tid == 0) __hip_atomic_store(c.host_tag, c.host_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------------------
// The sharded controller's exchange (ctl.hpp "sharded controller"; BASELINE config 5): run by
// the look-back ticket winner after lb_final<2> left this shard's top-K and argmin in cs.ids /
// cs.xv.  (a) The record — K + 1 entries of (window mean, global index) as 32-bit words — goes
// to LDS and, tagged with the mailbox's tick number, into slot [seq & 1][rank] of every peer's
// mailbox (system-scope stores over xGMI; the slot-reuse argument is peer_exchange_kernel's);
// (b) this rank's mailbox is polled for the G - 1 peer records (every thread issues all of its
// loads before checking any); (c) the merge: each top-K entry's rank among the G K gathered
// ones (ctl_merge_rank), the argmin over the G argmins (ctl_merge_argmin); (d) the MERGED
// selection is published for the look-ahead blocks (global indices: they roll the models out
// from the replicated global parameter table) and (e) the record's look-back fields and the
// top-K Dr / Df for mu-hat are written.  A peer that never arrives (past px_bound): this
// shard's own selection is used and the record's status says so.
// ------------------------------------------------------------------------------------
// Word w of this shard's record: entry w / 4 of lb_final<2>'s lists (cs.ids local index / cs.xv
// window mean) as value hi, lo, global index hi, lo (index -1: none).
__device__ __forceinline__ uint32_t ctl_rec_word(const CtlSel& cs, int64_t goff, int w) {
  const int e = w >> 2;
  const uint32_t l = cs.ids[e];
  const uint64_t q = (w & 2) ? (uint64_t)(l == kNoLocal ? (int64_t)-1 : goff + (int64_t)l)
                             : (uint64_t)__double_as_longlong(cs.xv[e]);
  return (w & 1) ? (uint32_t)q : (uint32_t)(q >> 32);
}

// A gather transport's first launch (px_phase 1): the look-back's ticket winner stores this
// shard's record, tagged px_seq, at px_send for the all-gather between the launches, and
// re-arms the look-back ticket (the completion does it on one-launch ticks).
__device__ __forceinline__ void ctl_px_send(const CtlLaunch& c, const CtlSel& cs) {
  __syncthreads();                                       // lb_final's wave 0 wrote cs.ids / xv
  const int nw = ctl_rec_words(c.K);
  for (int w = threadIdx.x; w < nw; w += kBlock) st_wt(&c.px_send[w], tag_word(c.px_seq, ctl_rec_word(cs, c.fin.goff, w)));
  if (threadIdx.x == 0) __hip_atomic_store(&c.tickets[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void ctl_exchange(const CtlLaunch& c, unsigned char* smem, const CtlSel& cs) {
  const int tid = threadIdx.x;
  const int G = c.px_G, rank = c.px_rank, K = c.K, nw = ctl_rec_words(K), M = G * K;
  const int64_t goff = c.fin.goff;
  unsigned char* base = smem + kScratchBytes;            // lb_final's region (dead)
  uint32_t* rec32 = reinterpret_cast<uint32_t*>(base);   // [G][nw]
  uint64_t* ekey = reinterpret_cast<uint64_t*>(base + align16(4 * (size_t)G * nw));
  uint64_t* eid = ekey + M;
  int* top = reinterpret_cast<int*>(eid + M);            // [KMAX] entry of each merged rank
  int* wlate = top + LLAMPC_KMAX;                        // [kWaves]
  const bool gath = c.px_phase == 2;                     // launch-uniform
  if (!gath) __syncthreads();                            // lb_final's wave 0 wrote cs.ids / xv
  // (a) this shard's record: to LDS and, tagged, to every peer (one (peer, word) per thread);
  // gathered: the own record from px_send (the first launch's), the peers' come from px_gath
  const size_t slot0 = gath ? 0 : (size_t)(c.px_seq & 1) * G * kRecWords;
  const size_t mine = slot0 + (size_t)rank * kRecWords;
  if (gath) {
    for (int w = tid; w < nw; w += kBlock) rec32[(size_t)rank * nw + w] = (uint32_t)ld_wt(&c.px_send[w]);
  } else {
    for (int p = tid; p < G * nw; p += kBlock) {
      const int g = p / nw, w = p - g * nw;
      const uint32_t word = ctl_rec_word(cs, goff, w);
      if (g == rank) rec32[(size_t)rank * nw + w] = word;
      else __hip_atomic_store(c.px_box[g] + mine + w, tag_word(c.px_seq, word), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  // (b) the peers' records from this rank's mailbox (gathered: from px_gath, stride nw)
  constexpr int kPer = (kCtlPxMax * ctl_rec_words(LLAMPC_KMAX) + kBlock - 1) / kBlock;
  const uint64_t* own = gath ? c.px_gath : c.px_box[rank] + slot0;
  const size_t stride = gath ? (size_t)nw : (size_t)kRecWords;
  int late = ctl_poll_words<kPer>(own, stride, G, nw, rank, c.px_seq, (uint64_t)c.px_bound << 16, rec32);
  const int wl = __any(late);
  if ((tid & 63) == 0) wlate[tid >> 6] = wl;
  __syncthreads();
  late = 0;
  for (int w = 0; w < kWaves; ++w) late |= wlate[w];
  auto ent_v = [&](int g, int j) {
    const uint32_t* r = rec32 + (size_t)g * nw + 4 * j;
    return __longlong_as_double((long long)join_words(r[0], r[1]));
  };
  auto ent_id = [&](int g, int j) {
    const uint32_t* r = rec32 + (size_t)g * nw + 4 * j;
    return (int64_t)join_words(r[2], r[3]);
  };
  // (c) the merge (block-uniform branch): every top-K entry's merged rank
  if (!late) {
    for (int e = tid; e < M; e += kBlock) {
      const int g = e / K, j = e - g * K;
      ctl_entry_order(ent_v(g, j), ent_id(g, j), e, ekey[e], eid[e]);
    }
    __syncthreads();
    for (int e = tid; e < M; e += kBlock) {
      const int r = ctl_merge_rank([&](int j) { return ekey[j]; }, [&](int j) { return eid[j]; }, M, e);
      if (r < K) top[r] = e;
    }
  } else if (tid < K) {
    top[tid] = rank * K + tid;                           // this shard's own lists
  }
  __syncthreads();
  if (tid >= 64) return;                                 // one wave finishes (the caller re-converges)
  const int lane = tid;
  const int Gm = late ? 1 : G;                           // argmin over every shard, or this one
  double bv;
  int64_t bi;
  ctl_merge_argmin([&](int g, double& v, int64_t& id) {
                     const int gg = late ? rank : g;
                     v = ent_v(gg, K);
                     id = ent_id(gg, K);
                   },
                   Gm, c.fin.nan_first != 0, bv, bi);
  double kv = __builtin_nan("");
  int64_t kid = -1;
  if (lane < K) {
    const int e = top[lane], g = e / K, j = e - g * K;
    kv = ent_v(g, j);
    kid = ent_id(g, j);
  }
  // (d) the merged selection (global indices < 2^32 - 1: llampc_ctl_set_exchange checks)
  const uint32_t kl = kid < 0 ? kNoLocal : (uint32_t)kid;
  const uint32_t al = bi < 0 ? kNoLocal : (uint32_t)bi;
  if (lane < K) {
    cs.ids[lane] = kl;
    st_wt(&cs.tag[lane], tag_word(cs.seq, kl));
  }
  if (lane == 0) {
    cs.ids[K] = al;
    st_wt(&cs.tag[K], tag_word(cs.seq, al));
    *cs.xlate = late;
  }
  // (e) the record's look-back half (pinned host memory, sc1 like lb_final's) and mu-hat's Dr / Df
  const double* gp = c.la.params;                        // the replicated global table [6][n]
  const int64_t gn = c.la.n;
  llampc_plan_out* o = &c.out->plan;
  const double nan = __builtin_nan("");
  if (lane < LLAMPC_KMAX) {
    const bool have = lane < K && kid >= 0;
    const double df = have ? gp[2 * gn + kid] : nan, dr = have ? gp[5 * gn + kid] : nan;
    st_wt(&o->topk[lane], have ? kid : (int64_t)-1);
    st_wt(&o->topk_val[lane], have ? kv : nan);
    st_wt(&o->topk_Df[lane], df);
    st_wt(&o->topk_Dr[lane], dr);
    if (lane < K) {
      cs.dr[lane] = dr;
      cs.df[lane] = df;
    }
  }
  if (lane == 0) {
    st_wt(&o->lb_best, bi);
    st_wt(&o->lb_best_val, bi < 0 ? nan : bv);
  }
}

}  // namespace llampc

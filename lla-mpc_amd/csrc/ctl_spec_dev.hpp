// ctl_spec_dev.hpp — the speculative look-ahead (CtlLaunch.n_spec; ctl.hpp): before the
// doorbell the look-back blocks rank their models by the window mean without x_t
// (ctl_spec_lists), the last of them merges the lists (ctl_spec_merge; sharded:
// ctl_spec_exchange) and the spec blocks, last in the grid, roll the listed models out with the
// tracking cost deferred (ctl_spec, defer_cost).  Included by ctl.hip only.
#pragma once
#include "ctl_cand_dev.hpp"
#include "ctl_door_dev.hpp"
#include "ctl_lds.hpp"
#include "final_dev.hpp"
#include "rollout_dev.hpp"

namespace llampc {

// ---- the speculative look-ahead (CtlLaunch.n_spec; ctl.hpp) --------------------------------
// The n_spec best of the look-back blocks' sorted lists: a tree merge in LDS (the cross-shard
// merge's), published as tagged words (local model index; kNoLocal: none).
// The sharded controller's speculative list (peer transport, armed ticks): this shard's n_spec
// best by the window mean without x_t (value, GLOBAL index) as 4 n_spec tagged words pushed into
// every peer's mailbox slot at px_spec_off (after the selection record's words; the same tick
// number: the exchange of this tick, only earlier), the peers' lists polled, and the n_spec best
// over the ranks published — global indices, which the spec blocks roll out from the replicated
// global table.  All before the doorbell.  A peer whose list does not arrive within
// px_spec_wait (a rank that launched this tick instead of arming it has none) leaves this rank
// with its own list: the speculation only decides which models are rolled out early, never a
// result, so the ranks' records stay equal whatever their lists.
__device__ __forceinline__ void ctl_spec_exchange(const CtlLaunch& c, unsigned char* base, const Ent* top) {
  const int tid = threadIdx.x, G = c.px_G, rank = c.px_rank, M = c.n_spec, nw = 4 * M;
  uint32_t* rec32 = reinterpret_cast<uint32_t*>(base);                          // [G][nw]
  Ent* g0 = reinterpret_cast<Ent*>(base + align16(4 * (size_t)G * nw));
  Ent* g1 = g0 + (size_t)G * M;
  const int64_t goff = c.fin.goff;
  const size_t slot0 = (size_t)(c.px_seq & 1) * G * kRecWords;
  const size_t mine = slot0 + (size_t)rank * kRecWords + c.px_spec_off;
  for (int p = tid; p < G * nw; p += kBlock) {
    const int g = p / nw, w = p - g * nw;
    const Ent& x = top[w >> 2];
    const uint64_t q = (w & 2) ? (uint64_t)(x.i == kNoIndex ? (int64_t)-1 : goff + x.i) : (uint64_t)__double_as_longlong(x.v);
    const uint32_t word = (w & 1) ? (uint32_t)q : (uint32_t)(q >> 32);
    if (g == rank) rec32[(size_t)rank * nw + w] = word;
    else __hip_atomic_store(c.px_box[g] + mine + w, tag_word(c.px_seq, word), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  constexpr int kPer = (kCtlPxMax * 4 * kCtlSpecMax + kBlock - 1) / kBlock;
  const int late = __syncthreads_or(
      ctl_poll_words<kPer>(c.px_box[rank] + slot0 + c.px_spec_off, kRecWords, G, nw, rank, c.px_seq, c.px_spec_wait, rec32));
  const int Gm = late ? 1 : G;
  for (int e = tid; e < Gm * M; e += kBlock) {
    const int g = late ? rank : e / M, j = e - (late ? 0 : g) * M;
    const uint32_t* r = rec32 + (size_t)g * nw + 4 * j;
    const int64_t id = (int64_t)join_words(r[2], r[3]);
    g0[e] = Ent{__longlong_as_double((long long)join_words(r[0], r[1])), id < 0 ? kNoIndex : id};
  }
  __syncthreads();
  const Ent* gtop = tree_merge(g0, g1, Gm, M);
  if (tid < M) {
    const int64_t i = gtop[tid].i;
    st_wt(&c.spec_tag[tid], tag_word(c.seq, i == kNoIndex ? kNoLocal : (uint32_t)i));
  }
}

template <bool PX>
__device__ __forceinline__ void ctl_spec_merge(const CtlLaunch& c, unsigned char* smem) {
  const int L = c.nb_lb, M = c.n_spec, tid = threadIdx.x;
  Ent* b0 = reinterpret_cast<Ent*>(smem + kScratchBytes);
  Ent* b1 = b0 + (size_t)L * M;
  for (int e = tid; e < L * M; e += kBlock) b0[e] = Ent{ld_wt(&c.spec_val[e]), ld_wt(&c.spec_idx[e])};
  __syncthreads();
  const Ent* top = tree_merge(b0, b1, L, M);
  if constexpr (PX) {
    if (c.px_G) {                       // launch-uniform: the lists of every rank
      ctl_spec_exchange(c, smem + kScratchBytes + align16(2 * sizeof(Ent) * (size_t)L * M), top);
      return;
    }
  }
  if (tid < M) {
    const int64_t i = top[tid].i;
    st_wt(&c.spec_tag[tid], tag_word(c.seq, i == kNoIndex ? kNoLocal : (uint32_t)i));
  }
}

// A look-back block's part, before the doorbell: its models ranked by the window mean without
// x_t (pred; NaN last, ties to the lower index — lb_final's order), the n_spec best stored
// sorted; the last block (ticket 1, reset at once: every block has drawn) merges the lists.
template <bool PX>
__device__ __forceinline__ void ctl_spec_lists(const CtlLaunch& c, int blk, double pred, bool valid, int64_t n,
                                               unsigned char* smem, int* flag) {
  const int tid = threadIdx.x, M = c.n_spec;
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem + kScratchBytes);
  uint32_t* ids = reinterpret_cast<uint32_t*>(keys + kBlock);
  const uint64_t key = valid ? order_key(pred) : ~0ull;
  const uint32_t id = valid ? (uint32_t)n : kNoModelId + (uint32_t)tid;
  keys[tid] = key;
  ids[tid] = id;
  __syncthreads();
  int r = 0;
#pragma unroll 16
  for (int j = 0; j < kBlock; ++j) r += (int)(keys[j] < key) | ((int)(keys[j] == key) & (int)(ids[j] < id));
  if (r < M) {
    st_wt(&c.spec_val[(int64_t)blk * M + r], valid ? pred : __builtin_nan(""));
    st_wt(&c.spec_idx[(int64_t)blk * M + r], valid ? n : kNoIndex);
  }
  if (!ticket_last(&c.tickets[1], (unsigned)c.nb_lb, flag)) return;
  if (tid == 0) __hip_atomic_store(&c.tickets[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  ctl_spec_merge<PX>(c, smem);
}

// The deferred tracking cost (rollout with kRDefer): the split rollout's epilogue with the reference
// known — the same terms in the same order, so J equals the undeferred rollout's bitwise.
__device__ __forceinline__ double defer_cost(const double* dpos, int dstride, const double* sx, int H, int pc,
                                             double Qd, double Pd, const DeferOut& d, bool sok, bool& bad) {
  double track = 0.0, xr0 = 0.0;
  for (int k = 0; k < H; ++k) {
    xr0 = sx[2 * (k + 1) + pc];
    const double e = dpos[k * dstride] - xr0;
    track = track + e * (Qd * e);
  }
  const double e = d.xl - xr0;
  const double jl = e * (Pd * e) + track;
  double J = (dpp_bcast<kQuad0>(jl) + dpp_bcast<kQuad1>(jl)) + d.act;
  bad = (int)bad | (int)!sok | (int)!d.dok | (int)!(fabs(J) <= __DBL_MAX__) | (int)(d.feas_s != d.feas_s);
  if (!(d.feas_s != 0.0)) J = __builtin_inf();
  return J;
}

// A spec block: model spec_tag[j] x the C candidates from the doorbell on (ctl.hpp
// CtlLaunch.n_spec).  Before the doorbell: the candidates (the look-ahead blocks' generator, so
// the same sequences), the rate clip, the staged terms, the model.  Then the rollouts with the
// tracking cost deferred (rollout with kRDefer), the reference from the first look-ahead block's walk
// (xref_tag), defer_cost, and the block's best candidate as ctl_lookahead publishes a slot.
// LPM 4 with diagonal Q / P only (the host enables spec blocks for that layout).
template <int LPM>
__device__ __forceinline__ void ctl_spec(const CtlLaunch& c, int j, unsigned char* smem, const Scratch& sc) {
  if constexpr (LPM != 4) {
    return;
  } else {
    const int tid = threadIdx.x;
    const int H = c.la.H, C = c.la.C;
    const SpecLds S = spec_lds(H, C);
    double* sx = reinterpret_cast<double*>(smem + S.sx);
    double* Ul = reinterpret_cast<double*>(smem + S.ul);
    double* s4 = reinterpret_cast<double*>(smem + S.s4);
    double* pos = reinterpret_cast<double*>(smem + S.pos);
    double* junk = reinterpret_cast<double*>(smem + S.junk);
    double* x0 = reinterpret_cast<double*>(smem + S.misc);            // [6]
    int* door_res = reinterpret_cast<int*>(smem + S.misc + 64);
    uint32_t* sid = reinterpret_cast<uint32_t*>(smem + S.misc + 80);
    const CtlState* st = c.st;
    const double* prev_seq = st->has_seq ? &st->useq[0][0] : nullptr;
    const double up0 = st->u_prev[0], up1 = st->u_prev[1];
    ctl_draw(c, prev_seq, up0, up1, Ul, tid, kBlock);
    __syncthreads();
    for (int t = tid; t < 2 * C; t += kBlock) {
      const int jj = t & 1;
      ctl_rate_chain(Ul + 2 * (size_t)(t >> 1) * H + jj, H, jj ? up1 : up0, jj ? c.rate[1] : c.rate[0]);
    }
    __syncthreads();
    if (tid >= 64) ctl_stage(c, Ul, s4, tid - 64, up0, up1);      // waves 1-3, as the look-ahead blocks
    if (tid == 0) {                     // the model (the spec merge publishes before the doorbell)
      int unused = 0;                   // no list in time: this block has no model
      *sid = poll_tag(c.spec_tag, j, c.seq, c.door_bound, unused, 2);
    }
    __syncthreads();
    const uint32_t id = *sid;
    if (id == kNoLocal) return;         // block-uniform: fewer models than spec blocks
    const Tire t = load_tire(c.la.params, c.la.n, id);
    if (ctl_door(c, x0, door_res) != (int)kCtlDoorFire) return;
    CTL_STAMP(blockIdx.x, 19);
    const int G = c.G, cpl = c.cpl;
    const int sub = tid % LPM, cl = tid / LPM, g = cl & (G - 1);
    CostK q = c.la.cost;
    VehK veh = c.la.veh;
    double Ts = c.la.Ts;
    // the pins of ctl_lookahead without the input bounds (umin, umax, dmax stay unpinned here)
    for (int m = 0; m < 4; ++m) {
      pin_vgpr(q.Q[m]);
      pin_vgpr(q.R[m]);
      pin_vgpr(q.P[m]);
    }
    pin_vgpr(veh.lf);
    pin_vgpr(veh.lr);
    pin_vgpr(veh.mass);
    pin_vgpr(veh.inv_mass);
    pin_vgpr(veh.inv_Iz);
    pin_vgpr(veh.Cm1);
    pin_vgpr(veh.Cm2);
    pin_vgpr(veh.Cr0);
    pin_vgpr(veh.Cr2);
    pin_vgpr(Ts);
    constexpr bool kScaled = scaled_yaw(LPM);
    StageK sk = make_stage<LPM>(veh, t, sub, Ts, Ts * veh.inv_mass);   // the quad's rear lane: (h/m) Fry
    if (kScaled) sk.ch[0].lw = sk.ch[0].lw / Ts;
    if (kScaled && sub >= 2) {          // lanes 2/3: zero-operand chains (plan kernel)
      sk.ch[0].lw = 0.0;
      sk.ch[0].sg = 0.0;
      sk.ch[0].B = 0.0;
      sk.ch[0].nsB = 0.0;
      sk.Bfw = 0.0;
    }
    const FusedK fq = make_fused(veh, sk, Ts, kScaled, LPM == 4);
    const fm::FmK K = load_la_consts<0, LPM>();
    const double Qd = sk.pc ? q.Q[3] : q.Q[0], Pd = sk.pc ? q.P[3] : q.P[0];
    // cpl == 1 with G == C (the host's layout for spec blocks): candidate g in quad g
    const int cc = g;
    double* dp = sub < 2 ? pos + (size_t)(2 * cc + sub) * H : junk + (tid & 63);
    const int ds = sub < 2 ? 1 : 0;
    bool bad = false;
    DeferOut d{};
    (void)cpl;
    (void)rollout<0, LPM, kRUlds | kRFast | kRS4 | kRSplit | kRDefer>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K,
                                                                      fq, bad, nullptr, s4, dp, ds, &d);
    CTL_STAMP(blockIdx.x, 20);
    // the reference: the walker's tagged halves (its walk ended long before these rollouts)
    {
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      for (int e = tid; e < 2 * (H + 1); e += kBlock) {
        uint64_t hi, lo;
        for (;;) {
          hi = ld_wt(&c.xref_tag[2 * e]);
          lo = ld_wt(&c.xref_tag[2 * e + 1]);
          if ((int)tag_ok(hi, c.seq) & (int)tag_ok(lo, c.seq)) break;
          if (ctl_late(t0, c.poll)) break;
          __builtin_amdgcn_s_sleep(1);
        }
        sx[e] = __longlong_as_double((long long)join_words(hi, lo));
      }
    }
    __syncthreads();
    double J = defer_cost(dp, ds, sx, H, sk.pc, Qd, Pd, d, sk.sok, bad);
    merge_bad<LPM>(bad);
    if (__builtin_expect(__any(bad), 0)) {
      bool unused = false;
      if (bad)
        J = rollout<0, LPM, kRUlds>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K, fq, unused);
    }
    double bv = __builtin_nan("");
    int64_t bc = kNoIndex;
    int nf = 0;
    if (sub == 0) nf += !isfinite(J);
    if (less_nan_last(J, cc, bv, bc)) {
      bv = J;
      bc = cc;
    }
    // the block's argmin over its C candidates and non-finite count (ctl_lookahead's (g))
    const int span = G * LPM;
    for (int off = (span < 64 ? span : 64) >> 1; off >= LPM; off >>= 1) {
      const double ov = __shfl_xor(bv, off, 64);
      const int64_t oc = __shfl_xor(bc, off, 64);
      nf += __shfl_xor(nf, off, 64);
      if (less_nan_last(ov, oc, bv, bc)) {
        bv = ov;
        bc = oc;
      }
    }
    if (span > 64) {                    // block-uniform
      if ((tid & 63) == 0) {
        sc.sv[tid >> 6] = bv;
        sc.si[tid >> 6] = bc;
        sc.sn[tid >> 6] = nf;
      }
      __syncthreads();
      const int w0 = (tid / span) * (span / 64);
      bv = sc.sv[w0];
      bc = sc.si[w0];
      nf = sc.sn[w0];
      for (int k = 1; k < span / 64; ++k) {
        nf += sc.sn[w0 + k];
        if (less_nan_last(sc.sv[w0 + k], sc.si[w0 + k], bv, bc)) {
          bv = sc.sv[w0 + k];
          bc = sc.si[w0 + k];
        }
      }
    }
    if (tid == 0) publish_slot(c.spec_res + 4 * (size_t)j, c.seq, bv, bc, (uint32_t)nf);
    CTL_STAMP(blockIdx.x, 21);
  }
}

}  // namespace llampc

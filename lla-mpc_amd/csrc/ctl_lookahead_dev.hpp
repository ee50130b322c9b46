// ctl_lookahead_dev.hpp — a look-ahead block of the controller tick (blocks [nb_lb, nb_lb +
// nb_la)): the tick's reference (cs_dev.hpp) and candidates (ctl_cand_dev.hpp), the wait for
// the selection, its slots' rollouts and each slot's best candidate published.  Included by ctl.hip and
// ctl_corr.hip (the corridor tick: CORR).
#pragma once
#include "cs_dev.hpp"
#include "ctl_cand_dev.hpp"
#include "ctl_door_dev.hpp"
#include "ctl_lds.hpp"
#include "rollout_dev.hpp"

namespace llampc {

// ------------------------------------------------------------------------------------
// A look-ahead block: the tick's reference and candidates (redundantly per block: they only
// read the state and the tables), then its slots' rollouts.
// ------------------------------------------------------------------------------------
// Waves 1-3 of a look-ahead block while wave 0 walks: an arrival count in LDS joins them (a
// block barrier would wait for the walk).  Every wave's LDS stores are complete before it
// arrives; the count only grows within a launch (targets 3, 6).
__device__ __forceinline__ void ctl_group_sync(int* arrived, int target) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(arrived, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (__hip_atomic_load(arrived, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < target) {
  }
}

// CORR (ctl_corr.hip, a corridor tick: c.s4 = 0, c.n_spec = 0): next to the wait for the selection the
// block polls the tick's half-planes (cor->hp_tag, published by the corridor blocks, which have lower
// indices and wait for nothing) into LDS, rolls out unsplit with the corridor term, and the selection
// slot's block re-runs its winner with the positions stored: the next tick's path (ctl.hpp CtlCorridor).
template <int LPM, bool CORR = false>
__device__ __forceinline__ void ctl_lookahead(const CtlLaunch& c, int blk, unsigned char* smem, const Scratch& sc,
                                              const CtlCorridor* cor = nullptr) {
  const int tid = threadIdx.x;
  const int H = c.la.H, C = c.la.C;
  const RacelineK rl = c.la.rl;
  const CtlLds L = ctl_lds(H, C, rl.n, c.s4 != 0);
  double* sx = reinterpret_cast<double*>(smem + L.sx);
  double* Ul = reinterpret_cast<double*>(smem + L.ul);
  double* kn = reinterpret_cast<double*>(smem + L.kn);
  double* spd = reinterpret_cast<double*>(smem + L.spd);
  double* dist = reinterpret_cast<double*>(smem + L.misc);              // [16]
  uint32_t* slot_id = reinterpret_cast<uint32_t*>(smem + L.misc + 128);   // [mpb] (<= 64)
  int32_t* sel_late = reinterpret_cast<int32_t*>(smem + L.misc + 384);    // [mpb]
  double* x0 = reinterpret_cast<double*>(smem + L.misc + 640);            // [6] x_t (no kernarg address taken)
  int* arrived = reinterpret_cast<int*>(smem + L.misc + 688);              // waves 1-3 (ctl_group_sync)
  double* s4 = reinterpret_cast<double*>(smem + L.s4);                      // s4: the staged inputs
  int* door_res = reinterpret_cast<int*>(smem + L.misc + 720);
  // CORR only, after the layout (ctl.hpp ctl_corr_extra): hp [H][6] | the winner's X | Y [2][H + 1] |
  // its cost is finite; and in misc whether a half-plane word never came
  struct CorLds {
    double *hp, *pos;
    int *flag, *late;
  };
  auto cor_lds = [&] {
    double* hp = reinterpret_cast<double*>(smem + L.end);
    return CorLds{hp, hp + 6 * H, reinterpret_cast<int*>(hp + 6 * H + 2 * (H + 1)),
                  reinterpret_cast<int*>(smem + L.misc + 724)};
  };
  CTL_STAMP(blockIdx.x, 0);
  const bool armed = c.door != nullptr;
  if (!armed && tid < 6) x0[tid] = ctl_xt(c, tid);
  if (tid == 0) *arrived = 0;
  if constexpr (CORR) {
    if (tid == 0) *cor_lds().late = 0;
  }
  const CtlState* st = c.st;
  const double* prev_seq = st->has_seq ? &st->useq[0][0] : nullptr;
  // rt.py:278-282: projidx and the mu bracket (mu-hat or the fixed mu) come from the host's
  // copy of the state (CtlLaunch.p0_walk / br_walk): the tables' loads follow the kernel
  // arguments directly (profiles/r04/s4/ctl_phases_prologue.txt: 2.5 us to the bracket before).
  // An armed launch reads the state itself: the previous tick ended before it started, and
  // the loads sit before the doorbell.
  // (values, not pointers, are selected — the empty asm keeps the compiler from loading through a
  // select of the state's and the kernel argument's addresses, which copies the whole argument
  // to scratch)
  int p0 = c.p0_walk;
  double mu_k = c.mu_fixed;
  asm volatile("" : "+s"(p0));
  asm volatile("" : "+v"(mu_k));
  if (armed) {
    p0 = st->projidx;
    if (c.use_mu) mu_k = st->mu_pred;
  }
  const double scale = c.use_mu ? c.v_factor : c.scale_fixed;
  const MuBracket br = armed ? mu_bracket(rl.mus, rl.M, mu_k) : c.br_walk;
  CTL_STAMP(blockIdx.x, 14);
  // waves 1-3: this tick's candidate variates (the previous tick's completion drew them) are
  // loaded now, their latency under the tables' (used only when their tag matches: ctl_draw)
  constexpr int kZPre = kCtlZPre;
  const int CH = C * H;
  const bool zfit = c.znoise != nullptr && ctl_zfit(C, H);
  double zr[kZPre][2];
  if (tid >= 64 && zfit) {
    const double* zb = c.znoise + 2 * (size_t)CH * (int)(c.tick & 1);
#pragma unroll
    for (int i = 0; i < kZPre; ++i) {
      const int p = tid - 64 + i * (kBlock - 64);
      const int pc = p < CH ? p : CH - 1;
      zr[i][0] = zb[2 * pc];
      zr[i][1] = zb[2 * pc + 1];
    }
  }
  // (a) tables: knots, x/y rows, the two speed profiles bracketing mu (cs_stage); (b)
  //     project_fast of x_t on raceline[:, p0 : p0 + 10] (track.py:147-160)
  cs_stage(rl, br, kn, spd);
  CTL_STAMP(blockIdx.x, 15);
  double px = 0.0, py = 0.0, pv = 0.0;
  if (armed) {                          // x_t: the doorbell (x0 in LDS after its barrier)
    if (ctl_door(c, x0, door_res) != (int)kCtlDoorFire) return;
    px = x0[0];
    py = x0[1];
    pv = x0[3];
  } else {
    px = c.x_t[0];
    py = c.x_t[1];
    pv = c.x_t[3];
    asm volatile("" : "+v"(px), "+v"(py), "+v"(pv));
  }
  const int segs = cs_project(c.pts, c.np, p0, px, py, dist);
  __syncthreads();
  CTL_STAMP(blockIdx.x, 1);
  // (c) wave 0 walks ConstantSpeed from the projection (planner.py:24-65) while waves 1-3
  //     draw the candidates before the rate clip, every (c, k, j)
  const double up0 = st->u_prev[0], up1 = st->u_prev[1];
  if (tid < 64) {
    double vr;
    (void)cs_walk_wave(rl, br, kn, spd, c.prefix, dist, segs, p0, px, py, pv, scale, c.la.Ts, H, sx, &vr);
    CTL_STAMP(blockIdx.x, 10);
  } else {
    if (zfit && c.ztag[(int)(c.tick & 1)] == c.tick + 1) {          // launch-uniform
      const double up[2] = {up0, up1};
#pragma unroll
      for (int i = 0; i < kZPre; ++i) {
        const int p = tid - 64 + i * (kBlock - 64);
        if (p < CH) {
          const int cc = p / H, k = p - cc * H;
          ctl_cand_pair_z(cc, k, H, prev_seq, up, c.nscale, c.umin, c.umax, zr[i][0], zr[i][1], Ul + 2 * (size_t)p);
        }
      }
    } else {
      ctl_draw(c, prev_seq, up0, up1, Ul, tid - 64, kBlock - 64);
    }
    if (c.s4) {                         // block-uniform: still during the walk, clip and stage
      ctl_group_sync(arrived, kWaves - 1);
      for (int t = tid - 64; t < 2 * C; t += kBlock - 64) {
        const int j = t & 1;
        ctl_rate_chain(Ul + 2 * (size_t)(t >> 1) * H + j, H, j ? up1 : up0, j ? c.rate[1] : c.rate[0]);
      }
      ctl_group_sync(arrived, 2 * (kWaves - 1));
      ctl_stage(c, Ul, s4, tid - 64, up0, up1);
    }
  }
  __syncthreads();
  CTL_STAMP(blockIdx.x, 2);
  // speculative look-ahead (c.n_spec): the first block publishes the reference for the spec
  // blocks' deferred costs, and wave 1 of every block loads the spec list (its models' results
  // come from the spec blocks)
  uint32_t* spec_ids = reinterpret_cast<uint32_t*>(smem + L.misc + 768);   // [kCtlSpecMax]
  if (c.n_spec) {
    if (blk == 0 && tid < 2 * (H + 1)) {
      const uint64_t v = (uint64_t)__double_as_longlong(sx[tid]);
      st_wt(&c.xref_tag[2 * tid], tag_word(c.seq, (uint32_t)(v >> 32)));
      st_wt(&c.xref_tag[2 * tid + 1], tag_word(c.seq, (uint32_t)v));
    }
    if (tid >= 64 && tid < 64 + c.n_spec) {
      int unused = 0;                   // a list that never comes: every slot is rolled out here
      spec_ids[tid - 64] = poll_tag(c.spec_tag, tid - 64, c.seq, c.poll, unused);
    }
  }
  // (d) waves 1-3 clip the candidates' rates; meanwhile (e) wave 0 takes this block's slots:
  //     the selection (tagged words of the look-back ticket winner), or the nominal model
  //     while the window fills
  const int mpb = c.mpb;
  if (!c.s4 && tid >= 64) {
    for (int t = tid - 64; t < 2 * C; t += kBlock - 64) {
      const int j = t & 1;
      ctl_rate_chain(Ul + 2 * (size_t)(t >> 1) * H + j, H, j ? up1 : up0, j ? c.rate[1] : c.rate[0]);
    }
  }
  if (tid < mpb) {                      // wave 0 (mpb <= 64): this block's slots
    const int slot = blk * mpb + tid;
    uint32_t id = kNoLocal;
    int late = 0;
    if (slot < c.nslots) {
      if (c.warm) id = 0;
      else id = poll_tag(c.sel_tag, slot, c.seq, c.poll, late);
    }
    slot_id[tid] = id;
    sel_late[tid] = late;
  }
  if constexpr (CORR) {
    // the tick's half-planes: each thread polls its share of the 12 H tagged halves (word 2 i the
    // high half of value i, 2 i + 1 the low one) under the launch's bound; a word that never comes
    // leaves a zero and the slots' late bit (the record then reads LLAMPC_STATUS_POLL_TIMEOUT)
    const CorLds cl = cor_lds();
    uint32_t* hp32 = reinterpret_cast<uint32_t*>(cl.hp);
    for (int e = tid; e < 12 * H; e += kBlock) {
      int late = 0;
      const uint32_t v = poll_tag(cor->hp_tag, e, c.seq, c.poll, late);
      hp32[(e & ~1) | ((e & 1) ^ 1)] = late ? 0u : v;
      if (late) *cl.late = 1;
    }
  }
  __syncthreads();
  if (c.n_spec) {                       // launch-uniform: a slot whose model a spec block rolls out: bit 1
    if (tid < 64) {
      const int lane = tid;
      for (int q = 0; q < mpb; ++q) {
        const uint32_t sid = slot_id[q];
        const bool hit = __ballot(lane < c.n_spec && sid != kNoLocal && spec_ids[lane] == sid) != 0;
        if (lane == 0 && hit) sel_late[q] |= 2;
      }
    }
    __syncthreads();
  }
  CTL_STAMP(blockIdx.x, 3);
  if (c.dbg && blk == 0) {              // tests: this tick's reference and candidates
    for (int e = tid; e < 2 * (H + 1); e += kBlock) {
      const int row = e / (H + 1), k = e - row * (H + 1);
      c.dbg[e] = sx[2 * k + row];
    }
    for (int e = tid; e < 2 * C * H; e += kBlock) c.dbg[2 * (H + 1) + e] = Ul[e];
  }
  // (f) rollouts: lane layout of the plan kernel's look-ahead (G candidate lanes per model,
  //     LPM lanes per rollout)
  const int G = c.G, cpl = c.cpl;
  const int sub = tid % LPM, cl = tid / LPM, g = cl & (G - 1), si = cl / G;
  const int slot = blk * mpb + si;
  const uint32_t id = si < mpb ? slot_id[si] : kNoLocal;
  const bool spec_hit = si < mpb && (sel_late[si] & 2);
  const bool live = slot < c.nslots && id != kNoLocal && !spec_hit;
  Tire t{};
  if (live) {
    if (c.warm) {
      t.Bf = c.nominal[0];
      t.Cf = c.nominal[1];
      t.Df = c.nominal[2];
      t.Br = c.nominal[3];
      t.Cr = c.nominal[4];
      t.Dr = c.nominal[5];
    } else {
      t = load_tire(c.la.params, c.la.n, id);
    }
  }
  CostK q = c.la.cost;
  VehK veh = c.la.veh;
  double Ts = c.la.Ts;
  for (int m = 0; m < 4; ++m) {
    pin_vgpr(q.Q[m]);
    pin_vgpr(q.R[m]);
    pin_vgpr(q.P[m]);
  }
  for (int m = 0; m < 2; ++m) {
    pin_vgpr(q.umin[m]);
    pin_vgpr(q.umax[m]);
    pin_vgpr(q.dmax[m]);
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
  double bv = __builtin_nan("");
  int64_t bc = kNoIndex;
  int nf = 0;
  constexpr bool kSplit = (LPM == 4);
  constexpr unsigned kRF = kRUlds;                          // the re-run; the fast runs add to it
  constexpr unsigned kRSplitQ = kSplit ? kRSplit : 0u;      // the quad's position split
  const bool diagQP = c.la.cost.Q[1] == 0.0 && c.la.cost.Q[2] == 0.0 && c.la.cost.P[1] == 0.0 && c.la.cost.P[2] == 0.0;
  if (live) {
    constexpr bool kScaled = scaled_yaw(LPM);
    StageK sk = make_stage<LPM>(veh, t, sub, Ts, Ts * veh.inv_mass);   // the quad's rear lane: (h/m) Fry
    if (kScaled) sk.ch[0].lw = sk.ch[0].lw / Ts;
    if (kScaled && LPM == 1) sk.ch[1].lw = sk.ch[1].lw / Ts;
    if (kScaled && LPM == 4 && sub >= 2) {   // lanes 2/3: zero-operand chains (plan kernel)
      sk.ch[0].lw = 0.0;
      sk.ch[0].sg = 0.0;
      sk.ch[0].B = 0.0;
      sk.ch[0].nsB = 0.0;
      sk.Bfw = 0.0;
    }
    const FusedK fq = make_fused(veh, sk, Ts, kScaled, LPM == 4);
    const fm::FmK K = load_la_consts<0, LPM>();
    for (int j = 0; j < cpl; ++j) {
      const int cc = g + j * G;
      if (cc >= C) break;
      bool bad = false;
      double J;
      if constexpr (CORR) {             // unsplit, unstaged, the corridor term (rollout_dev.hpp kRCorr)
        J = rollout<0, LPM, kRF | kRFast | kRCorr | kRPos>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K, fq, bad,
                                                          nullptr, nullptr, nullptr, 0, nullptr, cor_lds().hp, cor->weight);
      } else if (c.s4) {                // block-uniform: the staged input terms
        if (kSplit && diagQP)
          J = rollout<0, LPM, kRF | kRFast | kRS4 | kRSplitQ>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K, fq, bad,
                                                              nullptr, s4);
        else
          J = rollout<0, LPM, kRF | kRFast | kRS4>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K, fq, bad, nullptr, s4);
      } else if (kSplit && diagQP) {
        J = rollout<0, LPM, kRF | kRFast | kRSplitQ>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K, fq, bad);
      } else {
        J = rollout<0, LPM, kRF | kRFast>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K, fq, bad);
      }
      merge_bad<LPM>(bad);
      if (__builtin_expect(__any(bad), 0)) {
        bool unused = false;
        if constexpr (CORR) {
          if (bad)
            J = rollout<0, LPM, kRF | kRCorr | kRPos>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K, fq, unused,
                                                     nullptr, nullptr, nullptr, 0, nullptr, cor_lds().hp, cor->weight);
        } else if (bad) {
          J = rollout<0, LPM, kRF>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K, fq, unused);
        }
      }
      if (sub == 0) nf += !isfinite(J);
      if constexpr (CORR) {             // tests: every rolled-out cost, not the slot's best alone
        if (cor->dbg_cost != nullptr && sub == 0) cor->dbg_cost[(size_t)slot * C + cc] = J;
      }
      if (less_nan_last(J, cc, bv, bc)) {
        bv = J;
        bc = cc;
      }
    }
  }
  if constexpr (CORR) {                 // a slot of the tick that rolls nothing out (no such model): NaN
    if (cor->dbg_cost != nullptr && !live && sub == 0 && si < mpb && slot < c.nslots) {
      for (int j = 0; j < cpl; ++j) {
        const int cc = g + j * G;
        if (cc < C) cor->dbg_cost[(size_t)slot * C + cc] = __builtin_nan("");
      }
    }
  }
  CTL_STAMP(blockIdx.x, 4);
  // (g) per-slot argmin over its candidates and non-finite count: xor shuffles inside a wave,
  //     then across the slot's waves in LDS (a slot of 2 or 4 waves: G LPM in {128, 256})
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
  if (span > 64) {                      // block-uniform
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
  // (h) publish: cost (hi, lo), candidate, non-finite count | late << 31 (tagged words)
  if (g == 0 && sub == 0 && si < mpb && slot < c.nslots && !spec_hit) {
    uint32_t nfw = (uint32_t)nf | ((uint32_t)(sel_late[si] & 1) << 31);
    if constexpr (CORR) nfw |= (uint32_t)(*cor_lds().late != 0) << 31;
    publish_slot(c.slot_tag + 4 * (size_t)slot, c.seq, bv, bc, nfw);
  }
  CTL_STAMP(blockIdx.x, 5);
  if constexpr (CORR) {
    // (i) the path state for the next tick, off the tick's critical path (the slot is published): the
    //     block that holds the selection's slot re-runs its winner — the instantiations and operands
    //     of the published cost, so the same roundings — with the positions stored, and wave 0 copies
    //     them out with the validity flag (ctl.hpp ctl_path_valid)
    const int ss = c.warm ? 0 : c.K;
    const CorLds cl = cor_lds();
    double* ppos = cl.pos;
    int* pflag = cl.flag;
    if (blk == ss / mpb) {              // block-uniform
      const int t0 = (ss - blk * mpb) * G * LPM;
      if (tid >= t0 && tid < t0 + LPM) {
        double Jw = __builtin_nan("");
        double* dp = sub == 0 ? ppos : nullptr;
        if (live && bc >= 0 && bc < C) {
          const int cc = (int)bc;
          StageK sk = make_stage<LPM>(veh, t, sub, Ts, Ts * veh.inv_mass);
          constexpr bool kScaled = scaled_yaw(LPM);
          if (kScaled) sk.ch[0].lw = sk.ch[0].lw / Ts;
          if (kScaled && LPM == 1) sk.ch[1].lw = sk.ch[1].lw / Ts;
          if (kScaled && LPM == 4 && sub >= 2) {
            sk.ch[0].lw = 0.0;
            sk.ch[0].sg = 0.0;
            sk.ch[0].B = 0.0;
            sk.ch[0].nsB = 0.0;
            sk.Bfw = 0.0;
          }
          const FusedK fq = make_fused(veh, sk, Ts, kScaled, LPM == 4);
          const fm::FmK K = load_la_consts<0, LPM>();
          bool bad = false, unused = false;
          Jw = rollout<0, LPM, kRF | kRFast | kRCorr | kRPos>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K, fq, bad,
                                                             nullptr, nullptr, dp, H + 1, nullptr, cl.hp, cor->weight);
          merge_bad<LPM>(bad);
          if (bad)
            Jw = rollout<0, LPM, kRF | kRCorr | kRPos>(c.la, cc, 0, x0, sx, Ul, veh, t, sk, q, Ts, up0, up1, K, fq, unused,
                                                      nullptr, nullptr, dp, H + 1, nullptr, cl.hp, cor->weight);
        }
        if (sub == 0) {
          ppos[0] = x0[0];
          ppos[H + 1] = x0[1];
          *pflag = (int)(fabs(Jw) <= __DBL_MAX__);
        }
      }
      __syncthreads();
      if (tid < 64) {
        bool ok = *pflag != 0;
        for (int e = tid; e < 2 * (H + 1); e += 64) {
          const int row = e / (H + 1), j = e - row * (H + 1);
          const double v = ppos[e];
          ok = ok && fabs(v) <= __DBL_MAX__;
          cor->path_wr[row * kCtlPathStride + j] = v;
        }
        const int all = __all(ok);
        if (tid == 0) *cor->valid_wr = all;
      }
    }
  }
}

}  // namespace llampc

// rollout_dev.hpp — one (model, candidate) rollout over the horizon with its NLP objective, in
// every compile-time variant (the RolloutFlag bits), and what its callers share: load_tire, the
// input-rate term, the input feasibility, the pair / quad merge of `bad` and the batched global -> LDS copy.  Included by
// lookback_dev.hpp, lookahead_dev.hpp, ctl.hip, nlp.hip and kernels.hip.
#pragma once
#include "dev_stamps.hpp"
#include "dev_wave.hpp"

namespace llampc {

namespace {

__device__ __forceinline__ Tire load_tire(const double* p, int64_t ld, int64_t i) {
  Tire t;
  t.Bf = p[i];
  t.Cf = p[ld + i];
  t.Df = p[2 * ld + i];
  t.Br = p[3 * ld + i];
  t.Cr = p[4 * ld + i];
  t.Dr = p[5 * ld + i];
  return t;
}

}  // namespace

// Input-rate term du' R du of one step (nmpc.py:65-68, 111) and the bounds / rate
// feasibility of one input (nmpc.py:102-105; branch-free: |d| <= dmax is false for NaN like
// the two one-sided tests; dmax < 0 disables).
__device__ __forceinline__ double act_term(const CostK& q, double d0, double d1) {
  return d0 * (q.R[0] * d0 + q.R[1] * d1) + d1 * (q.R[2] * d0 + q.R[3] * d1);
}
__device__ __forceinline__ bool input_feasible(const CostK& q, double ua, double ud, double d0,
                                               double d1) {
  return (int)(ua <= q.umax[0]) & (int)(ua >= q.umin[0]) & (int)(ud <= q.umax[1]) &
         (int)(ud >= q.umin[1]) & ((int)(q.dmax[0] < 0) | (int)(fabs(d0) <= q.dmax[0])) &
         ((int)(q.dmax[1] < 0) | (int)(fabs(d1) <= q.dmax[1]));
}

// The pair or quad of one rollout shares it: the lanes' `bad` flags merged by DPP, so that the
// general evaluation re-runs in all of the rollout's lanes or in none (in place; LPM 1: nothing).
template <int LPM>
__device__ __forceinline__ void merge_bad(bool& bad) {
  if (LPM == 2) {
    const int bi = bad;
    bad = __builtin_amdgcn_mov_dpp(bi, kPair0, 0xF, 0xF, false) | __builtin_amdgcn_mov_dpp(bi, kPair1, 0xF, 0xF, false);
  } else if (LPM == 4) {
    int bi = bad;
    bi |= __builtin_amdgcn_mov_dpp(bi, kQuadX1, 0xF, 0xF, false);
    bi |= __builtin_amdgcn_mov_dpp(bi, kQuadX2, 0xF, 0xF, false);
    bad = bi;
  }
}

// The corridor term of one step (CORR): hp = (a0, a1, b, c0, c1, d), the half-planes a.p <= b and
// c.p <= d on the position p = (X, Y) after the step; the squared slacks s1^2 + s2^2, every
// product and sum rounded on its own.  a = 0, b = +inf disables a half-plane (g = -inf, s = 0;
// so does a NaN g: the comparison is false).
__device__ __forceinline__ double corridor_slack2(const double* hp, double X, double Y) {
#pragma clang fp contract(off)
  const double2 r0 = *reinterpret_cast<const double2*>(hp);
  const double2 r1 = *reinterpret_cast<const double2*>(hp + 2);
  const double2 r2 = *reinterpret_cast<const double2*>(hp + 4);
  const double g1 = (r0.x * X + r0.y * Y) - r1.x;
  const double g2 = (r1.y * X + r2.x * Y) - r2.y;
  const double s1 = g1 > 0 ? g1 : 0.0, s2 = g2 > 0 ? g2 : 0.0;
  return s1 * s1 + s2 * s2;
}
__device__ __forceinline__ double corridor_add(double J, double cw, double pen) {
#pragma clang fp contract(off)
  const double wp = cw * pen;
  return J + wp;
}

// The rollout's compile-time variants: the template argument F of rollout is an OR of these.
enum RolloutFlag : unsigned {
  kRStage = 1u << 0,  // STAGE: the inputs staged per block at `su` as [k][c][SW] records (lookahead_block, nlp.hip)
  kRXm = 1u << 1,     // XM: the model's own reference a.xref_pm (the raceline walk) instead of the shared `sx`
  kRFast = 1u << 2,   // FAST: the branch-free stage (dyn.hpp step_fast), `bad` |= an operand outside its domains;
                      //   without it the general evaluation: the re-run of bad lanes, on the lane's own operands only
  kRSplit = 1u << 3,  // SPLIT (fused RK4, LPM 4, diagonal Q and P): a quad lane integrates one position component
                      //   (dyn.hpp k_fused) and its tracking term; J = (J_X + J_Y) + act by two DPP broadcasts
  kRUlds = 1u << 4,   // ULDS (the controller tick, nlp.hip): the raw candidates U [C][H][2] at `su` (LDS) instead of a.U
  kRTraj = 1u << 5,   // TRAJ: the state after every step to `traj` (three 16-B stores; null: none)
  kRS4 = 1u << 6,     // S4 (ctl_cand_dev.hpp ctl_stage, with ULDS and FAST): sin / cos delta and the cost terms read at `s4`
  kRDefer = 1u << 7,  // DEFER (ctl_spec_dev.hpp ctl_spec, with SPLIT and S4): positions to `dpos`, the rest to *dout
  kRCorr = 1u << 8,   // CORR (nlp.hip's corridor solve, the plan kernel's corridor look-ahead): two position half-planes
                      //   per step at `hp` [H][6] (LDS), the squared slacks summed over the horizon, J + cw pen
                      //   (corridor_slack2 above); unsplit rollouts only, fused RK4 or NLP-Euler at any LPM
  kRQuadr = 1u << 9,  // QUADR (with SPLIT; the plan kernel's lookahead_block): the component is a per-step quadrature in
                      //   quad lanes 2 / 3 (dyn.hpp step_fused kPosQuadr), no position broadcast in the stages; lanes 0 / 1
                      //   hold garbage in x[0] and track, J = (J_X + J_Y) + act from lanes 2 and 3
  kRPos = 1u << 10,   // POS (the controller tick's corridor look-ahead, with CORR): where `dpos` is not null, the position
                      //   after step k to dpos[k + 1] (X) and dpos[dstride + k + 1] (Y) — the same evaluation with or
                      //   without the stores, so a winner's re-run returns the published cost's own positions
};
// What DEFER returns in *dout: the reference is not known yet, so the lane stores its position
// component after step k at dpos[k dstride] instead of accumulating the tracking term, and
// returns its last position, the summed input-rate cost, the feasibility and the domain flag
// (J: ctl_spec_dev.hpp defer_cost, the same terms in the same order once the reference is known).
struct DeferOut {
  double xl, act, feas_s;
  bool dok;
};
// One (model, candidate) rollout over H steps and its NLP objective (nmpc.py:44-111); returns
// J (+inf when infeasible).  s4 (S4): [C][H][2] the steering's sin / cos per (candidate, step),
// then at s4 + 2CH [C][2] per candidate the input-rate cost sum and the feasibility (1 / 0; NaN:
// a steering outside sincos_fast's domain, so the rollout re-runs in the general evaluation) —
// the step reads two values instead of forming them, with the same values and roundings.
// SW: doubles per staged record (the plan kernel's kStageW; the NLP kernel's compact 6: the
// Euler record's input-rate term and feasibility then at 4 and 5 instead of 6 and 7).
template <int INTEG, int LPM, unsigned F, int SW = kStageW>
__device__ __forceinline__ double rollout(const LookaheadLaunch& a, int c, int64_t n,
                                          const double* x0, const double* sx, const double* su, const VehK& veh,
                                          const Tire& t, const StageK& sk, const CostK& q,
                                          double Ts, double up0, double up1, const fm::FmK& K,
                                          const FusedK& fq, bool& bad, double* traj = nullptr,
                                          const double* s4 = nullptr, double* dpos = nullptr, int dstride = 0,
                                          DeferOut* dout = nullptr, const double* hp = nullptr,
                                          double cw = 0.0) {
  constexpr bool STAGE = F & kRStage, FAST = F & kRFast, SPLIT = F & kRSplit, ULDS = F & kRUlds;
  constexpr bool TRAJ = F & kRTraj, S4 = F & kRS4, DEFER = F & kRDefer, CORR = F & kRCorr, QUADR = F & kRQuadr;
  constexpr int POS = QUADR ? kPosQuadr : (SPLIT ? kPosSplit : kPosBoth);   // dyn.hpp step_fused
  constexpr int XM = (F & kRXm) ? 1 : 0;
  constexpr bool kYaw1 = !XM;           // the quad's lane 3 carries Psi + 1 (below; dyn.hpp chain_fold)
  static_assert(!DEFER || (SPLIT && S4), "deferred tracking cost: the controller's split, staged rollout");
  static_assert(!TRAJ || (INTEG != 0 && !SPLIT), "trajectory output: unscaled, unsplit state");
  static_assert(!S4 || (ULDS && FAST && !STAGE), "staged sincos / cost terms: the controller's fast rollout");
  static_assert(!SPLIT || (FAST && INTEG == 0 && LPM == 4), "position split: fused RK4 quads only");
  static_assert(!QUADR || (SPLIT && !DEFER), "position quadrature: a split rollout that forms its own tracking term");
  static_assert(!ULDS || !STAGE, "candidates in LDS: unstaged rollout");
  static_assert(!CORR || (!SPLIT && !DEFER), "corridor term: a lane that holds both position components");
  static_assert(!CORR || (INTEG != 2 && !S4 && !XM), "corridor term: the NLP kernel's and the plan kernel's shared-xref rollouts");
  const int H = a.H, C = a.C;
  const double* Ub = ULDS ? su : a.U;
  double x[6];
#pragma unroll
  for (int m = 0; m < 6; ++m) x[m] = x0[m];
  if (SPLIT) x[0] = sk.pc ? x0[1] : x0[0];
  if (FAST && INTEG == 0 && scaled_yaw(LPM)) {   // the scaled yaw and yaw rate (make_fused)
    x[2] = x0[2] * K.two_pi;
    x[5] = x0[5] * Ts;
    // The quad's lane 3 carries Psi + 1, a quarter turn: its fold is then lane 2's and returns
    // cos psi (dyn.hpp chain_fold<SCALED>).  A lane's Psi is read by its own fold and by dm.ps
    // only — the yaw increment is W, the cost takes positions, no variant stores or broadcasts
    // x[2] (TRAJ is unscaled) — so the offset ends there; dm.ps of lane 3 is max |Psi + 1|, one
    // unit early at the fold's range, and the general re-run starts again from x0.
    if (LPM == 4 && kYaw1) x[2] = sk.l3 ? x[2] + 1.0 : x[2];
  }
  const double Qd = sk.pc ? q.Q[3] : q.Q[0], Pd = sk.pc ? q.P[3] : q.P[0];   // SPLIT only
  double track = 0.0, act = 0.0;
  double p0 = up0, p1 = up1;
  bool feas = true;
  double feas_s = 1.0;
  double xr0 = 0.0, xr1 = 0.0;
  [[maybe_unused]] double pen = 0.0;    // CORR: the summed squared slacks
  const double* xpm = XM ? a.xref_pm + n * 2 * H : nullptr;   // this model's reference
  Dom dm;                               // FAST: the operands' running extremes
  dm.init();
  for (int k = 0; k < H; ++k) {
    if (FAST) STEP_STAMP(k < 24 ? k : 24);
    double ua, ud;
    Input u;
    FusedIn fi{};
    if (STAGE) {                        // staged per block (lookahead_block), layouts there
      static_assert(SW == kStageW || (SW == 6 && INTEG != 0), "the compact record: NLP-Euler only");
      constexpr int kAct = SW == kStageW ? 6 : 4, kFeas = kAct + 1;
      const double* o = su + SW * (k * C + c);
      if (INTEG == 0 && FAST) {         // the fused stages' input terms
        fi = FusedIn{o[0], o[1], o[2], o[3], o[4]};
        ua = 0.0;
        ud = o[5];
      } else if (INTEG == 0) {          // the general re-run: the candidate from U itself
        ua = Ub[2 * ((int64_t)c * H + k)];
        ud = Ub[2 * ((int64_t)c * H + k) + 1];
        u = make_input(ua, ud);
      } else {                          // sincos(delta) staged with the fast/general rule
        ua = o[0];
        ud = o[1];
        u.a = ua;
        u.d = ud;
        u.sd = o[2];
        u.cd = o[3];
      }
      act = act + o[kAct];              // the candidate's input-rate term and feasibility
      feas_s = feas_s * o[kFeas];
    } else {
      ua = Ub[2 * ((int64_t)c * H + k)];
      ud = Ub[2 * ((int64_t)c * H + k) + 1];
      if (S4) {
        const double2 sc2 = *reinterpret_cast<const double2*>(s4 + 2 * ((int64_t)c * H + k));
        u.a = ua;
        u.d = ud;
        u.sd = sc2.x;
        u.cd = sc2.y;
      } else if (FAST) {
        u = make_input_fast(ua, ud, K, bad);
      } else {
        u = make_input(ua, ud);
      }
    }
    const double d0 = ua - p0, d1 = ud - p1;          // nmpc.py:65-68
    if (!STAGE && !S4 && q.enforce) feas = (int)feas & (int)input_feasible(q, ua, ud, d0, d1);
    if (FAST && INTEG == 0 && STAGE) step_fused<LPM, POS, kYaw1>(sk, fq, x, fi, ud, K, dm);
    else if (FAST && INTEG == 0) step_fused<LPM, POS, kYaw1>(sk, fq, x, u, K, dm);
    else if (FAST) step_fast<INTEG, LPM>(veh, t, sk, x, u, Ts, K, dm);
    else step<INTEG>(veh, t, x, u, Ts);
    if constexpr (CORR) pen = pen + corridor_slack2(hp + 6 * k, x[0], x[1]);
    if constexpr ((F & kRPos) != 0) {
      static_assert(CORR, "position output: the corridor rollout (both components in the lane, unscaled)");
      if (dpos != nullptr) {
        dpos[k + 1] = x[0];
        dpos[dstride + k + 1] = x[1];
      }
    }
    if (DEFER) {                        // the position component, for defer_cost
      dpos[k * dstride] = x[0];
    } else if (SPLIT) {                 // this lane's component of the reference and term
      xr0 = XM ? xpm[2 * k + sk.pc] : sx[2 * (k + 1) + sk.pc];
      const double e = x[0] - xr0;
      track = track + e * (Qd * e);
    } else if (XM) {
      xr0 = xpm[2 * k];
      xr1 = xpm[2 * k + 1];
    } else {
      xr0 = sx[2 * (k + 1)];
      xr1 = sx[2 * (k + 1) + 1];
    }
    if (!SPLIT) {
      const double e0 = x[0] - xr0, e1 = x[1] - xr1;
      track = track + (e0 * (q.Q[0] * e0 + q.Q[1] * e1) + e1 * (q.Q[2] * e0 + q.Q[3] * e1));
    }
    if (!STAGE && !S4) act = act + act_term(q, d0, d1);
    p0 = ua;
    p1 = ud;
    if (TRAJ && traj != nullptr) {      // the state after step k (every lane of a quad holds it;
#pragma unroll                          // the caller passes traj to one lane): three 16-B stores
      for (int m = 0; m < 6; m += 2) *reinterpret_cast<double2*>(traj + 6 * (k + 1) + m) = double2{x[m], x[m + 1]};
    }
  }
  if (S4) {                             // the candidate's summed input-rate cost, feasibility
    const double2 af = *reinterpret_cast<const double2*>(s4 + 2 * (int64_t)C * H + 2 * c);
    act = af.x;
    feas_s = af.y;
  }
  if constexpr (DEFER) {
    (void)track;
    (void)Qd;
    (void)Pd;
    *dout = DeferOut{x[0], act, feas_s, dm.ok()};
    return 0.0;
  }
  double J;
  if (SPLIT) {                                                    // nmpc.py:48, :111
    const double e = x[0] - xr0;
    const double jl = e * (Pd * e) + track;                       // this component's part
    // X + Y: lanes 0 and 1, or (QUADR) lanes 2 and 3 — there lanes 0/1's jl is garbage (step_fused)
    // and ends here: J, and with it `bad`, the count and the argmin, is the same in the four lanes
    if constexpr (QUADR) J = (dpp_bcast<kQuad2>(jl) + dpp_bcast<kQuad3>(jl)) + act;
    else J = (dpp_bcast<kQuad0>(jl) + dpp_bcast<kQuad1>(jl)) + act;
  } else {
    const double e0 = x[0] - xr0, e1 = x[1] - xr1;                 // nmpc.py:48 (xref_H)
    const double term = e0 * (q.P[0] * e0 + q.P[1] * e1) + e1 * (q.P[2] * e0 + q.P[3] * e1);
    J = (term + track) + act;                                     // nmpc.py:111
  }
  if constexpr (CORR) J = corridor_add(J, cw, pen);
  // the domain, once per rollout: a NaN operand reaches x[0..1] (every chain output feeds
  // the later stages' positions, the last stage's feeds vx, vy, omega only through a NaN
  // state that the position update already carries), so a non-finite J is re-run too
  if (FAST) {
    const bool dok = dm.ok();
    bad = (int)bad | (int)!sk.sok | (int)!dok | (int)!(fabs(J) <= __DBL_MAX__);
    if (S4) bad = (int)bad | (int)(feas_s != feas_s);   // a steering outside sincos_fast's domain
  }
  if (STAGE || S4) feas = feas_s != 0.0;
  if (!feas) J = __builtin_inf();
  return J;
}

// Global -> LDS copy of `count` doubles with B loads in flight per thread: a plain strided
// loop waits one memory round trip per element — ~25 per thread for the ETHZ spline table
// (50 KB per block), which made the raceline prologue ~25 us.  src(e) gives element e; it
// is called for e = threadIdx.x + j kBlock in order, j < B per batch, past count too (with
// e clamped to count - 1: unguarded loads, no branch per element; those are not stored).
template <int B = 16, typename Src>
__device__ __forceinline__ void copy_lds(double* dst, int count, Src src) {
  for (int base = threadIdx.x; base < count; base += B * kBlock) {
    double v[B];
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const int e = base + j * kBlock;
      v[j] = src(e < count ? e : count - 1);
    }
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const int e = base + j * kBlock;
      if (e < count) dst[e] = v[j];
    }
  }
}

}  // namespace llampc

// ctl_cand_dev.hpp — the tick's candidate input sequences, the same in every block that needs
// them: the draw (look-ahead, spec and completing blocks), the next tick's variates (the
// completing block) and the staged look-ahead inputs (look-ahead and spec blocks).  The rate clip
// between draw and staging is a loop over ctl_rate_chain (ctl.hpp) in each of those blocks.
// Included by ctl.hip's headers only.
#pragma once
#include "ctl.hpp"
#include "rollout_dev.hpp"

namespace llampc {

// The raw candidates [C][H][2] (before the rate clip) by threads t0 + i stride, i >= 0: from
// this tick's variates when the previous tick's completion drew them (znoise, tagged), four
// pairs' loads in flight per thread; else one Philox call per pair here.
__device__ __forceinline__ void ctl_draw(const CtlLaunch& c, const double* prev_seq, double up0, double up1,
                                         double* U, int t0, int stride) {
  const int H = c.la.H, C = c.la.C, CH = C * H;
  const double up[2] = {up0, up1};
  const int half = (int)(c.tick & 1);
  if (c.znoise && c.ztag[half] == c.tick + 1) {                     // launch-uniform
    const double* zb = c.znoise + 2 * (size_t)CH * half;
    for (int p0 = t0; p0 < CH; p0 += 4 * stride) {
      double z[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = p0 + i * stride < CH ? p0 + i * stride : CH - 1;
        z[i][0] = zb[2 * p];
        z[i][1] = zb[2 * p + 1];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = p0 + i * stride;
        if (p < CH) {
          const int cc = p / H, k = p - cc * H;
          ctl_cand_pair_z(cc, k, H, prev_seq, up, c.nscale, c.umin, c.umax, z[i][0], z[i][1], U + 2 * (size_t)p);
        }
      }
    }
  } else {
    for (int p = t0; p < CH; p += stride) {
      const int cc = p / H, k = p - cc * H;
      ctl_cand_pair(cc, k, H, prev_seq, up, c.nscale, c.umin, c.umax, c.tick, c.seed, 0, U + 2 * (size_t)p);
    }
  }
}

// The next tick's variates into znoise half (t + 1) & 1 (the completing block's waves 1-3
// while wave 0 polls), then its tag; the next launch reads them after this one has ended.
__device__ __forceinline__ void ctl_draw_next(const CtlLaunch& c, int t0, int stride) {
  if (!c.znoise) return;
  const int H = c.la.H, CH = c.la.C * H;
  const uint64_t nt = c.tick + 1;
  double* zb = c.znoise + 2 * (size_t)CH * (int)(nt & 1);
  for (int p = t0; p < CH; p += stride) {
    double z0 = 0.0, z1 = 0.0;
    if (p >= H) ctl_z2((uint32_t)p, nt, c.seed, 0, z0, z1);           // candidate 0 has none
    *reinterpret_cast<double2*>(zb + 2 * (size_t)p) = double2{z0, z1};
  }
  if (t0 == 0) c.ztag[nt & 1] = nt + 1;
}

// The staged look-ahead inputs (s4; waves 1-3, t in [0, 192), after the rate clip): sin / cos
// delta of every (candidate, step) — make_input_fast's values — and per candidate the
// rollout's input-rate cost sum (act_term over k in order from 0, nmpc.py:65-68, 111) and
// its feasibility (1 / 0, nmpc.py:102-105; NaN: a steering outside sincos_fast's domain, so
// the rollout re-runs in the general evaluation).  The same arithmetic as the unstaged step.
__device__ __forceinline__ void ctl_stage(const CtlLaunch& c, const double* Ul, double* s4, int t, double up0,
                                          double up1) {
  const int H = c.la.H, C = c.la.C;
  constexpr int kThreads = kBlock - 64;
  const int ns = C < kThreads / 2 ? C : kThreads / 2;                 // threads summing per candidate
  if (t < ns) {
    const CostK q = c.la.cost;          // a copy: a reference into the kernel argument made
                                        // the compiler copy the whole argument to scratch
    for (int cc = t; cc < C; cc += ns) {
      const double* u = Ul + 2 * (size_t)cc * H;
      double act = 0.0, p0 = up0, p1 = up1;
      bool feas = true, bad = false;
      for (int k = 0; k < H; ++k) {
        const double ua = u[2 * k], ud = u[2 * k + 1];
        const double d0 = ua - p0, d1 = ud - p1;
        if (q.enforce) feas = (int)feas & (int)input_feasible(q, ua, ud, d0, d1);
        act = act + act_term(q, d0, d1);
        bad = (int)bad | (int)!fm::sincos_fast_ok(ud);
        p0 = ua;
        p1 = ud;
      }
      *reinterpret_cast<double2*>(s4 + 2 * (size_t)C * H + 2 * cc) =
          double2{act, bad ? __builtin_nan("") : (feas ? 1.0 : 0.0)};
    }
  } else {
    const fm::FmK K = fm::FmK::load();
    for (int f = t - ns; f < C * H; f += kThreads - ns) {
      double sd, cd;
      fm::sincos_fast(Ul[2 * f + 1], &sd, &cd, K);
      *reinterpret_cast<double2*>(s4 + 2 * (size_t)f) = double2{sd, cd};
    }
  }
}

}  // namespace llampc

// cs_dev.hpp — the device ConstantSpeed reference walker (planner.py:12-67): the tables to
// LDS, the projection of x_t, one wave's walk.  Run by every look-ahead block of the
// controller tick (ctl_lookahead) and by cs_kernel (llampc_ctl_reference).  Included by ctl.hip only.
#pragma once
#include "ctl.hpp"
#include "dev_stamps.hpp"
#include "dev_wave.hpp"
#include "rollout_dev.hpp"

namespace llampc {

// ------------------------------------------------------------------------------------
// The device ConstantSpeed (planner.py:12-67), shared by the controller's look-ahead blocks
// and llampc_ctl_reference: tables -> LDS, the projection, one lane's walk.
// ------------------------------------------------------------------------------------
// knots (+inf pad, RaceRef::step) and the two speed profiles bracketing mu, interleaved per
// segment [n-1][2][4] (consecutive threads write consecutive LDS words; a wave's loads touch 8
// rows x 8 consecutive segments).  The x/y rows stay in global memory: the walk records each
// step's (segment, dx) and x/y are evaluated once after it, in parallel.
__device__ __forceinline__ void cs_stage(const RacelineK& rl, const MuBracket& br, double* kn, double* spd) {
  const int nseg = rl.n - 1;
  const double* slo = rl.speed + (size_t)br.lo * 4 * nseg;
  const double* shi = rl.speed + (size_t)br.hi * 4 * nseg;
  copy_lds<4>(kn, rl.n, [&](int e) { return rl.knots[e]; });
  copy_lds<24>(spd, 8 * nseg, [&](int e) {
    const int sg = e >> 3, q = e & 3;
    return ((e >> 2) & 1 ? shi : slo)[(size_t)q * nseg + sg];
  });
  if ((int)threadIdx.x < kKnotPad) kn[rl.n + threadIdx.x] = __builtin_inf();
}

// project_fast of (px, py) on points[:, p0 : p0 + 10] (track.py:147-160): threads < segs
// write their segment's distance; returns the segment count
__device__ __forceinline__ int cs_project(const double* pts, int np_, int p0, double px, double py, double* dist) {
  const int segs = ctl_segments(p0, np_);
  const int tid = threadIdx.x;
  if (tid < kCtlSegs && tid < segs)
    dist[tid] = ref_project_dist(px, py, pts[p0 + tid], pts[np_ + p0 + tid], pts[p0 + tid + 1], pts[np_ + p0 + tid + 1]);
  return segs;
}

// x / den rounded as the IEEE division, by den's correctly rounded reciprocal rden = 1 / den:
// q0 = x rden, then one FMA residual step (Markstein; checked against x / den on 10^8 pairs
// of normal operands) — 3 dependent instructions instead of the division's ~10
__device__ __forceinline__ double div_by(double x, double den, double rden) {
  const double q0 = x * rden;
  const double e = __builtin_fma(-q0, den, x);
  return __builtin_fma(e, rden, q0);
}

// One speed profile's cubic at dx from its interleaved coefficients (spline_at's expression,
// so the same roundings): two 16-B LDS reads.
__device__ __forceinline__ double spline4(const double* c, double dx) {
  const double2 ab = *reinterpret_cast<const double2*>(c);
  const double2 cd = *reinterpret_cast<const double2*>(c + 2);
  const double dx2 = dx * dx;
  return ab.x + ab.y * dx + cd.x * dx2 + cd.y * (dx2 * dx);
}

// ConstantSpeed's walk (planner.py:24-65) by ONE WAVE (all 64 lanes call it, uniform control
// flow): projidx = p0 + argmin (:26-27), the start arc length from the prefix table (:29-36),
// then H <= 64 steps of :40-62 into sx [H+1][2]; returns projidx and, in lane 0, vr (:63-64).
// RaceRef::step's walk over a window of 64 consecutive segments held in registers — lane j
// segment w0 + j: its knot (+inf past the last) and the two speed cubics' coefficients — so a
// step reads no memory: every lane evaluates its segment's v at t, the count of knots <= t over
// the kWalkAhead lanes past the current segment (a ballot: RaceRef::step's advance) picks the
// lane whose v holds, and readlane takes v, the knot and dx from it.  The chain of a step is
// the cubic and one division chain.  The window moves (64 lanes' LDS reads) when the
// candidates would leave it — about once per walk; x/y are not on the chain: lane k keeps step
// k's (segment, dx) and evaluates :43 after the walk.  (Before: each step read its candidate
// segments from LDS — one LDS round trip on the chain, ~0.3 us a step; the serial walker
// ~0.7 us.)  v = (v_lo wa) / den + (v_hi wb) / den (:58-60), the divisions by div_by, the cubic
// spline_at's expression (spline4's): the same roundings as before.
constexpr int kWalkAhead = 16;
__device__ __forceinline__ double cubic4(double a, double b, double c, double d, double dx) {
  const double dx2 = dx * dx;
  return a + b * dx + c * dx2 + d * (dx2 * dx);
}
__device__ __forceinline__ int cs_walk_wave(const RacelineK& rl, const MuBracket& br, const double* kn,
                                            const double* spd, const double* prefix, const double* dist, int segs,
                                            int p0, double px, double py, double v0, double scale, double Ts, int H,
                                            double* sx, double* vr) {
  const int lane = (int)threadIdx.x & 63;
  const int m = rl.n - 1;
  const int pj = segs >= 1 ? p0 + np_argmin(dist, segs) : p0;
  const double L = kn[m];
  double s = prefix[pj];
  double v = fmax(v0, 0.01);                                        // planner.py:34
  // the start segment: bisect-right on the knots clamped to [0, m - 1] = the count of
  // knots[i] <= s over i in [1, m - 1] (ascending knots)
  int cnt = 0;
  for (int i = 1 + lane; i <= m - 1; i += 64) cnt += (int)(kn[i] <= s);
  int seg = wave_sum(cnt);
  double kseg = kn[seg];
  // a single profile (mu outside the table) has wa = 1, wb = 0, den = 1: v = v_lo exactly
  // (both rows hold it), so no branch keeps the second cubic's reads behind the first
  const double wa = br.wa, wb = br.wb, den = br.den, rden = 1.0 / den;
  // the register window: lane j <- segment w0 + j (cubics of min(w0 + j, m - 1), as before)
  int w0 = 0;
  double wk, c0, c1, c2, c3, c4, c5, c6, c7;
  auto load_win = [&](int base) {
    w0 = base;
    const int sj = base + lane;
    wk = sj <= m ? kn[sj] : __builtin_inf();
    const int sl = sj < m - 1 ? sj : m - 1;
    const double2* c = reinterpret_cast<const double2*>(spd + 8 * (size_t)sl);
    const double2 q0 = c[0], q1 = c[1], q2 = c[2], q3 = c[3];
    c0 = q0.x;
    c1 = q0.y;
    c2 = q1.x;
    c3 = q1.y;
    c4 = q2.x;
    c5 = q2.y;
    c6 = q3.x;
    c7 = q3.y;
  };
  load_win(seg);
  CTL_STAMP(blockIdx.x, 17);
  int myseg = 0;                                                    // lane k: step k's segment, dx
  double mydx = 0.0, v1 = 0.0;
  for (int k = 0; k < H; ++k) {
    double t = s + scale * v * Ts;                                  // :41
    if (!(t >= 0.0 && t < L)) {                                     // :42 Python float %
      double r = fmod(t, L);
      if (r != 0.0 && r < 0.0) r += L;
      t = (r == 0.0) ? 0.0 : r;
    }
    s = t;
    if (t < kseg) {                                                 // wrapped past the lap end
      seg = 0;
      kseg = kn[0];
    }
    int rel = seg - w0;
    if (rel < 0 || rel + kWalkAhead > 63) {                         // wave-uniform: move the window
      load_win(seg);
      rel = 0;
    }
    double dl = t - wk;
    const double vb = cubic4(c0, c1, c2, c3, dl);
    const double va = cubic4(c4, c5, c6, c7, dl);
    double vl = div_by(vb * wa, den, rden) + div_by(va * wb, den, rden);
    const int adv = __popcll(__ballot(lane > rel && lane <= rel + kWalkAhead && wk <= t));
    double dx;
    if (__builtin_expect(adv < kWalkAhead, 1)) {                    // wave-uniform
      const int ch = rel + adv;
      v = readlane_d(vl, ch);
      kseg = readlane_d(wk, ch);
      dx = readlane_d(dl, ch);
      seg += adv;
    } else {                                                        // past the candidates: serial
      int sg = seg + kWalkAhead;
      while (sg < m - 1 && kn[sg + 1] <= t) ++sg;
      kseg = kn[sg];
      dx = t - kseg;
      const double* c = spd + 8 * (size_t)sg;
      const double b = spline4(c, dx);
      const double a = spline4(c + 4, dx);
      v = div_by(b * wa, den, rden) + div_by(a * wb, den, rden);
      seg = sg;
    }
    if (lane == k) {
      myseg = seg;
      mydx = dx;
    }
    if (k == 0) v1 = v;
  }
  CTL_STAMP(blockIdx.x, 18);
  if (lane == 0) {
    sx[0] = px;                                                     // planner.py:33
    sx[1] = py;
    *vr = v1 * scale;
  }
  if (lane < H) {                                                   // :43 calc_position
    sx[2 * (lane + 1)] = spline_at(rl.xy, m, myseg, mydx);
    sx[2 * (lane + 1) + 1] = spline_at(rl.xy + 4 * (size_t)m, m, myseg, mydx);
  }
  return pj;
}

}  // namespace llampc

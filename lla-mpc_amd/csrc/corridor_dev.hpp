// corridor_dev.hpp — the track corridor of llampc.mpc.constraints.track_corridor in scalar form,
// for the device (kernels.hip track_corridor_kernel; llampc_nlp_track_corridor, llampc_nlp_solve_track)
// and, being __host__ __device__, for a stand-alone host program (tests/native/track_corridor_host.cpp).
//
// One path point p = P_k, k = 1..H, gives row k - 1 of hp [H][6] and theta_k:
//   nearest segment  segments j = 0..n-1 of the CLOSED centre line, A = c_j, B = c_{(j+1) mod n} (n-1
//                    the closing one): len = sqrt(dx^2 + dy^2), u = (B - A) / len, t = (p - A).u; the
//                    foot q = A (t <= 0), B (t >= len), A + u t (else); d2 = |p - q|^2.  The smallest
//                    d2 wins, ties to the lower j (np.argmin over Track.project's order).
//   arc length       r = |q - A| / len; theta = fmod(tt[j] + r (next - tt[j]), L), next = tt[j+1], or
//                    L on the closing segment (Track._xy2param).  tt (theta_track) and L
//                    (track_length) are the Track object's own numbers, handed over as they are.
//   param_to_xy      idt = the first index with tt[idt] > theta, capped at n-1 (binary search), the
//                    point interpolated linearly between idt-1 and idt (Track._param2xy).  The cap
//                    extrapolates the last segment over the closing gap, as the host does: the lookup
//                    is DISCONTINUOUS at vertex 0 (theta = 0 gives c_0, theta just below L a point up
//                    to millimetres away), so a path that touches vertex 0 exactly has a centre and a
//                    tangent that turn on the last rounding of theta — on the host and here alike.
//   record           c = param_to_xy(theta), fwd = param_to_xy(fmod(theta + eps, L)), back =
//                    param_to_xy(theta - eps (+ L if negative)), eps = kTangentEps = 0.05
//                    (constraints.TANGENT_EPS); n = the left normal of fwd - back over sqrt(x^2 + y^2);
//                    hw = track_width / 2 - margin; the row is (n, n.c + hw, -n, -(n.c - hw)).
// The host function differs from this form by rounding only (<= 1e-12 on hp and theta on the
// packaged tracks, tests/test_nlp_track_corridor_cpu.py).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace llampc {

constexpr double kTangentEps = 0.05;     // constraints.TANGENT_EPS
constexpr int kTrackMaxPoints = 4096;    // llampc_nlp_set_track's largest centre line

// A track's centre line as the corridor reads it (device pointers in a launch).
struct TrackK {
  const double* cx;                      // [n]
  const double* cy;                      // [n]
  const double* tt;                      // [n] arc length at every centre point, tt[0] = 0, increasing
  int32_t n;
  int32_t pad;
  double L;                              // closed length, > tt[n-1]
};

// The foot of p on segment j: -> d2 = |p - q|^2; q, the segment's start and length through the
// references.
__host__ __device__ inline double corridor_foot(const TrackK& t, int j, double px, double py, double& qx,
                                                double& qy, double& ax, double& ay, double& len) {
  const int j1 = j + 1 == t.n ? 0 : j + 1;
  ax = t.cx[j];
  ay = t.cy[j];
  const double bx = t.cx[j1], by = t.cy[j1];
  const double dx = bx - ax, dy = by - ay;
  len = sqrt(dx * dx + dy * dy);
  const double ux = dx / len, uy = dy / len;
  const double s = (px - ax) * ux + (py - ay) * uy;
  if (s <= 0.0) {
    qx = ax;
    qy = ay;
  } else if (s >= len) {
    qx = bx;
    qy = by;
  } else {
    qx = ax + ux * s;
    qy = ay + uy * s;
  }
  const double ex = px - qx, ey = py - qy;
  return ex * ex + ey * ey;
}

__host__ __device__ inline double corridor_seg_d2(const TrackK& t, int j, double px, double py) {
  double qx, qy, ax, ay, len;
  return corridor_foot(t, j, px, py, qx, qy, ax, ay, len);
}

// Whether (d2, j) comes before (bd2, bj): the smaller distance, ties to the lower segment.
__host__ __device__ inline bool corridor_before(double d2, int j, double bd2, int bj) {
  return d2 < bd2 || (d2 == bd2 && j < bj);
}

// The nearest segment by a scan in order (the host program; the kernel splits the scan over a block).
__host__ __device__ inline int corridor_nearest(const TrackK& t, double px, double py) {
  int bj = 0;
  double bd2 = corridor_seg_d2(t, 0, px, py);
  for (int j = 1; j < t.n; ++j) {
    const double d2 = corridor_seg_d2(t, j, px, py);
    if (d2 < bd2) {
      bd2 = d2;
      bj = j;
    }
  }
  return bj;
}

// The arc length of p's foot on segment j.
__host__ __device__ inline double corridor_theta(const TrackK& t, int j, double px, double py) {
  double qx, qy, ax, ay, len;
  (void)corridor_foot(t, j, px, py, qx, qy, ax, ay, len);
  const double fx = qx - ax, fy = qy - ay;
  const double r = sqrt(fx * fx + fy * fy) / len;
  const double t0 = t.tt[j];
  const double next = j + 1 == t.n ? t.L : t.tt[j + 1];
  return fmod(t0 + r * (next - t0), t.L);
}

// Track._param2xy: the first idt with tt[idt] > theta, capped at n-1, by bisection; idt >= 1 as
// tt[0] = 0 <= theta (the clamp keeps a theta that is not, a NaN's included, inside the tables).
__host__ __device__ inline void corridor_param_to_xy(const TrackK& t, double theta, double& x, double& y) {
  int lo = 0, hi = t.n;                  // tt[i] <= theta for i < lo, tt[i] > theta for i >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t.tt[mid] > theta) hi = mid;
    else lo = mid + 1;
  }
  int idt = lo < t.n - 1 ? lo : t.n - 1;
  if (idt < 1) idt = 1;
  const double ta = t.tt[idt - 1], tb = t.tt[idt];
  const double d = (theta - ta) / (tb - ta);
  const double xa = t.cx[idt - 1], ya = t.cy[idt - 1];
  x = xa + d * (t.cx[idt] - xa);
  y = ya + d * (t.cy[idt] - ya);
}

// The three arc lengths a record looks up: the centre's, the tangent's forward and backward ones.
__host__ __device__ inline double corridor_lookup_theta(double theta, double L, int which) {
  if (which == 1) return fmod(theta + kTangentEps, L);
  if (which == 2) {
    const double b = theta - kTangentEps;
    return b < 0.0 ? b + L : b;
  }
  return theta;
}

// The row (n, n.c + hw, -n, -(n.c - hw)) from the centre c and the tangent's two points.
__host__ __device__ inline void corridor_row(double cx, double cy, double fx, double fy, double bx, double by,
                                             double hw, double* row) {
  const double tx = fx - bx, ty = fy - by;
  const double nx0 = -ty, ny0 = tx;
  const double nn = sqrt(nx0 * nx0 + ny0 * ny0);
  const double nx = nx0 / nn, ny = ny0 / nn;
  const double nc = nx * cx + ny * cy;
  row[0] = nx;
  row[1] = ny;
  row[2] = nc + hw;
  row[3] = -nx;
  row[4] = -ny;
  row[5] = -(nc - hw);
}

// One record in one thread (the host program): row [6] and the arc length of p = (px, py).
__host__ __device__ inline double corridor_record(const TrackK& t, double px, double py, double hw, double* row) {
  const double theta = corridor_theta(t, corridor_nearest(t, px, py), px, py);
  double c[3][2];
  for (int w = 0; w < 3; ++w) corridor_param_to_xy(t, corridor_lookup_theta(theta, t.L, w), c[w][0], c[w][1]);
  corridor_row(c[0][0], c[0][1], c[1][0], c[1][1], c[2][0], c[2][1], hw, row);
  return theta;
}

}  // namespace llampc

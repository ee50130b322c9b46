// corridor_block_dev.hpp — one block's share of the track corridor (corridor_dev.hpp): the record of ONE
// path point, the nearest-segment scan split over the block, for the controller tick's corridor blocks
// (ctl_corr.hip).  The geometry is corridor_dev.hpp's; the block's frame — tables to LDS, the scan by
// thread, the wave and block reduction, the three look-ups in lanes 0-2 — is track_corridor_kernel's
// (kernels.hip), statement for statement.  That kernel keeps its own text: called through this
// function its code object came out with another register allocation.  Device only.
#pragma once
#include "corridor_dev.hpp"
#include "dev_wave.hpp"

namespace llampc {

// The record of p = (px, py).  The block first copies the track's three tables into its LDS (24 n
// bytes: independent loads, one memory round trip), and everything after reads them there.  Each
// thread takes the segments j = tid (mod 256) in ascending order, the (d2, j) pairs are reduced over
// the wave (DPP) and over the four waves (LDS) with ties to the lower j; wave 0 then looks up the
// centre and the tangent's two points in lanes 0, 1, 2 and thread 0 calls emit(row [6], theta).
// Waits for nothing.  Dynamic LDS: sv [4] | si [4] | cx [n] | cy [n] | tt [n].
constexpr size_t kCorridorBlockScratch = 64;
template <typename Emit>
__device__ __forceinline__ void corridor_block(const TrackK g, unsigned char* smem, double px, double py, double hw,
                                               Emit emit) {
  double* sv = reinterpret_cast<double*>(smem);
  int64_t* si = reinterpret_cast<int64_t*>(smem + 32);
  double* lx = reinterpret_cast<double*>(smem + kCorridorBlockScratch);
  double* ly = lx + g.n;
  double* lt = ly + g.n;
  const int tid = threadIdx.x;
#pragma unroll 4
  for (int j = tid; j < g.n; j += kBlock) {
    lx[j] = g.cx[j];
    ly[j] = g.cy[j];
    lt[j] = g.tt[j];
  }
  __syncthreads();
  const TrackK t{lx, ly, lt, g.n, 0, g.L};
  // a lane with no segment holds (NaN, kNoIndex): last under the NaN-last order
  double bd2 = __builtin_nan("");
  int64_t bj = kNoIndex;
  for (int j = tid; j < t.n; j += kBlock) {
    const double d2 = corridor_seg_d2(t, j, px, py);
    if (bj == kNoIndex || d2 < bd2) {
      bd2 = d2;
      bj = j;
    }
  }
  wave_min<0>(bd2, bj);
  if ((tid & 63) == 0) {
    sv[tid >> 6] = bd2;
    si[tid >> 6] = bj;
  }
  __syncthreads();
  if (tid >= 64) return;
  bd2 = sv[0];
  bj = si[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; ++w) {
    if (less_nan_last(sv[w], si[w], bd2, bj)) {
      bd2 = sv[w];
      bj = si[w];
    }
  }
  const int j = (int)(bj < 0 ? 0 : (bj > t.n - 1 ? t.n - 1 : bj));   // inside the tables whatever the path
  const double theta = corridor_theta(t, j, px, py);
  double x, y;
  corridor_param_to_xy(t, corridor_lookup_theta(theta, t.L, tid < 3 ? tid : 0), x, y);
  const double fx = readlane_d(x, 1), fy = readlane_d(y, 1);
  const double bx = readlane_d(x, 2), by = readlane_d(y, 2);
  if (tid == 0) {
    double row[6];
    corridor_row(x, y, fx, fy, bx, by, hw, row);
    emit(row, theta);
  }
}

}  // namespace llampc

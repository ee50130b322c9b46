// Host harness for csrc/corridor_dev.hpp (test infrastructure): the device corridor's own
// __host__ __device__ functions run on the CPU on a track and a path read from a file, so
// tests/test_nlp_track_corridor_cpu.py compares them with constraints.track_corridor and
// Track.xy_to_param before any GPU is involved — built with AddressSanitizer and UBSan (host
// code only), every table a heap block of exactly the size the functions may touch.
//   track_corridor_host FILE
// FILE: float64 words — n, H, track_length, hw, then cx [n], cy [n], theta_track [n], path [2][H+1].
// Output: H lines "theta a0 a1 b c0 c1 d" (%.17g) by corridor_record (the scan in one thread), then
// H lines the same by the kernel's split: the nearest segment as the minimum over 256 strided
// partial scans under corridor_before, the three lookups one by one, corridor_row.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "corridor_dev.hpp"

using namespace llampc;

static std::unique_ptr<double[]> take(FILE* f, size_t n) {
  std::unique_ptr<double[]> v(new double[n]);
  if (std::fread(v.get(), sizeof(double), n, f) != n) std::exit(3);
  return v;
}

static void print(double theta, const double* row) {
  std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", theta, row[0], row[1], row[2], row[3], row[4], row[5]);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const auto head = take(f, 4);
  const int n = (int)head[0], H = (int)head[1];
  if (n < 2 || n > kTrackMaxPoints || H < 1 || H > 64) return 2;
  const auto cx = take(f, (size_t)n), cy = take(f, (size_t)n), tt = take(f, (size_t)n);
  const auto path = take(f, 2 * (size_t)(H + 1));
  std::fclose(f);
  const TrackK t{cx.get(), cy.get(), tt.get(), n, 0, head[2]};
  const double hw = head[3];
  double row[6];
  for (int k = 1; k <= H; ++k) {
    const double theta = corridor_record(t, path[k], path[H + 1 + k], hw, row);
    print(theta, row);
  }
  constexpr int kLanes = 256;
  for (int k = 1; k <= H; ++k) {
    const double px = path[k], py = path[H + 1 + k];
    int bj = -1;
    double bd2 = 0.0;
    for (int lane = kLanes - 1; lane >= 0; --lane) {     // any order of the partial results
      int lj = -1;
      double ld2 = 0.0;
      for (int j = lane; j < n; j += kLanes) {
        const double d2 = corridor_seg_d2(t, j, px, py);
        if (lj < 0 || d2 < ld2) {
          ld2 = d2;
          lj = j;
        }
      }
      if (lj >= 0 && (bj < 0 || corridor_before(ld2, lj, bd2, bj))) {
        bd2 = ld2;
        bj = lj;
      }
    }
    const double theta = corridor_theta(t, bj, px, py);
    double c[3][2];
    for (int w = 0; w < 3; ++w) corridor_param_to_xy(t, corridor_lookup_theta(theta, t.L, w), c[w][0], c[w][1]);
    corridor_row(c[0][0], c[0][1], c[1][0], c[1][1], c[2][0], c[2][1], hw, row);
    print(theta, row);
  }
  return 0;
}

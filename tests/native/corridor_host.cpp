// Host harness for the corridor helpers of csrc/capi_host.hpp (test infrastructure):
// corridor_max_slack and corridor_invalid run on the CPU on the numbers of the command line and
// print what they return, so tests/test_nlp_corridor_cpu.py compares them with hand-computed
// values — built with AddressSanitizer and UBSan (host code only), every buffer a heap block of
// exactly the size the helper may touch.
//   corridor_host slack H hp[6 H] xmpc[6 (H + 1)]   -> the largest slack, %.17g
//   corridor_host valid H weight hp[6 H]            -> "ok", or what is wrong
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "capi_host.hpp"

using namespace llampc;

static std::unique_ptr<double[]> take(char** argv, size_t n) {
  std::unique_ptr<double[]> v(new double[n]);
  for (size_t i = 0; i < n; ++i) v[i] = std::strtod(argv[i], nullptr);   // "inf", "-inf", "nan" too
  return v;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int H = std::atoi(argv[2]);
  if (H < 1) return 2;
  if (!std::strcmp(argv[1], "slack")) {
    if (argc != 3 + 6 * H + 6 * (H + 1)) return 2;
    const auto hp = take(argv + 3, 6 * (size_t)H);
    const auto xm = take(argv + 3 + 6 * H, 6 * (size_t)(H + 1));
    std::printf("%.17g\n", corridor_max_slack(hp.get(), xm.get(), H));
    return 0;
  }
  if (!std::strcmp(argv[1], "valid")) {
    if (argc != 4 + 6 * H) return 2;
    const double w = std::strtod(argv[3], nullptr);
    const auto hp = take(argv + 4, 6 * (size_t)H);
    const char* why = corridor_invalid(hp.get(), H, w);
    std::printf("%s\n", why ? why : "ok");
    return 0;
  }
  return 2;
}

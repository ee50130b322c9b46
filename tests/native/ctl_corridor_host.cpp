// Host harness for the corridor tick's host-checkable parts (test infrastructure), built with
// AddressSanitizer and UBSan (host code only) by tests/test_ctl_corridor_cpu.py:
//   ctl_corridor_host path FILE
//     FILE: float64 words — H, the chosen cost, X [H+1], Y [H+1] (heap blocks of exactly that size).
//     Output: "valid V" by ctl_path_valid, then H + 1 lines "Px Py" (%.17g): the path P_j = X[ctl_path_index(j, H)]
//     (csrc/ctl.hpp: constraints.default_path's prev_xmpc rule, as the corridor blocks read it).
//   ctl_corridor_host shape n C H K rl_n warm do_lb track_n
//     ctl_shape (csrc/capi_host.hpp) with the corridor input, every field by name.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "capi_host.hpp"

using namespace llampc;

static std::unique_ptr<double[]> take(FILE* f, size_t n) {
  std::unique_ptr<double[]> v(new double[n]);
  if (std::fread(v.get(), sizeof(double), n, f) != n) std::exit(3);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "path" && argc == 3) {
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    const auto head = take(f, 2);
    const int H = (int)head[0];
    if (H < 1 || H > LLAMPC_HMAX) return 2;
    const auto X = take(f, (size_t)H + 1), Y = take(f, (size_t)H + 1);
    std::fclose(f);
    std::printf("valid %d\n", (int)ctl_path_valid(head[1], X.get(), Y.get(), H));
    for (int j = 0; j <= H; ++j) std::printf("%.17g %.17g\n", X[ctl_path_index(j, H)], Y[ctl_path_index(j, H)]);
    return 0;
  }
  if (mode == "shape" && argc == 10) {
    auto arg = [&](int i) { return std::atoll(argv[i]); };
    const CtlShape s = ctl_shape(arg(2), (int32_t)arg(3), (int32_t)arg(4), (int32_t)arg(5), (int32_t)arg(6), arg(7) != 0,
                                 arg(8) != 0, false, 0, (int32_t)arg(9));
    std::printf("lpm %d\nG %d\ncpl %d\nmpb %d\ns4 %d\nzfit %d\nR %d\nnb_lb %d\nnb_la %d\nnslots %d\nnb_cor %d\nlds %zu\n"
                "poll_off %zu\n",
                s.lpm, s.G, s.cpl, s.mpb, s.s4, s.zfit, s.R, s.nb_lb, s.nb_la, s.nslots, s.nb_cor, s.lds, s.poll_off);
    return 0;
  }
  return 2;
}

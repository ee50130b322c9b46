// Host harness for the track tick's host-checkable parts (test infrastructure): plan_shape with a
// track (csrc/launch_shape.hpp), the path rule's index (csrc/ctl.hpp ctl_path_index) and the host's
// half of the path's validity (csrc/capi_host.hpp track_path_next / track_path_offered), run on the
// CPU and printed for tests/test_plan_track_cpu.py.  Built with AddressSanitizer and UBSan (host code
// only).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_host.hpp"

using namespace llampc;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "shape")) {
    // n C H K lb full la integrator xref_mode pack px_G corridor track_n
    if (argc != 15) return 2;
    PlanShapeIn in{};
    in.n = std::atoll(argv[2]);
    in.C = std::atoi(argv[3]);
    in.H = std::atoi(argv[4]);
    in.K = std::atoi(argv[5]);
    in.lb = std::atoi(argv[6]) != 0;
    in.full = std::atoi(argv[7]) != 0;
    in.la = std::atoi(argv[8]) != 0;
    in.integrator = std::atoi(argv[9]);
    in.xref_mode = std::atoi(argv[10]);
    in.pack = std::atoi(argv[11]) != 0;
    in.px_G = std::atoi(argv[12]);
    in.corridor = std::atoi(argv[13]) != 0;
    in.track_n = std::atoi(argv[14]);
    in.share = 1;
    in.wq_counter = true;
    const PlanShape s = plan_shape(in, 256);
    if (s.refuse) {
      std::printf("refuse %s\n", s.refuse);
      return 0;
    }
    std::printf("family %d\nlpm %d\nG %d\ncpl %d\nstage %d\nwq %d\nnb_lb %d\nnb_cor %d\nnb_la %d\ngrid %d\nlds %zu\n",
                (int)s.family, s.lpm, s.G, s.cpl, (int)s.stage, s.wq, s.nb_lb, s.nb_cor, s.nb_la,
                s.nb_lb + s.nb_cor + s.nb_la, s.lds);
  } else if (!std::strcmp(argv[1], "index")) {
    // H: ctl_path_index(j, H) for j = 0..H
    if (argc != 3) return 2;
    const int H = std::atoi(argv[2]);
    for (int j = 0; j <= H; ++j) std::printf("%d\n", ctl_path_index(j, H));
  } else if (!std::strcmp(argv[1], "state")) {
    // events: tick:H | plain | seed:H | clear | offer:H (prints 0 / 1)
    TrackPathState st{0};
    for (int i = 2; i < argc; ++i) {
      const char* a = argv[i];
      const char* c = std::strchr(a, ':');
      const int H = c ? std::atoi(c + 1) : 0;
      if (!std::strncmp(a, "tick", 4)) st = track_path_next(st, kPathTrackTick, H);
      else if (!std::strncmp(a, "plain", 5)) st = track_path_next(st, kPathOtherLaunch);
      else if (!std::strncmp(a, "seed", 4)) st = track_path_next(st, kPathSeed, H);
      else if (!std::strncmp(a, "clear", 5)) st = track_path_next(st, kPathClear);
      else if (!std::strncmp(a, "offer", 5)) std::printf("%d\n", (int)track_path_offered(st, H));
      else return 2;
    }
  } else if (!std::strcmp(argv[1], "tick")) {
    // weight margin track_width: track_tick_invalid's message or "ok"
    if (argc != 5) return 2;
    const char* why = track_tick_invalid(std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4]));
    std::printf("%s\n", why ? why : "ok");
  } else {
    return 2;
  }
  return 0;
}

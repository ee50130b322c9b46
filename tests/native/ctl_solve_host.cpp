// Host harness for the fused control step's pure helpers in csrc/ctl_solve.hpp (test infrastructure):
// the record writer the build kernel runs, held BITWISE to capi_host.hpp nlp_batch_pack (the record
// the batched search was written for), the parameter table's entries, and the refusals' predicates —
// on the CPU, built with AddressSanitizer (host code only), every buffer a heap block of exactly the
// size the layout claims.
//   ctl_solve_host record H warm stride     the two records compared word by word; the p6 table
//   ctl_solve_host state attached pending prelaunch exchange gather cor_w
//   ctl_solve_host cfg H Ts samples ctl_H ctl_Ts cus
//   ctl_solve_host blocks attached setter on
//   ctl_solve_host applied H bad            bad: -1 none, 0..1 u0[bad] = NaN, 2.. useq[bad - 2] = inf
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "capi_host.hpp"
#include "ctl_solve.hpp"

using namespace llampc;

static int record(int H, int warm, int stride) {
  const NlpBatchLayout l = nlp_batch_layout(H, 64);
  const int64_t n = 7, col = 4;
  std::unique_ptr<uint64_t[]> want(new uint64_t[l.rec_words]), got(new uint64_t[l.rec_words]);
  for (size_t i = 0; i < l.rec_words; ++i) want[i] = got[i] = 0xA5A5A5A5A5A5A5A5ull;
  std::unique_ptr<double[]> x0(new double[6]), xref(new double[2 * (H + 1)]), up(new double[2]), mean(new double[2 * H]),
      nominal(new double[6]), params(new double[6 * n]);
  for (int i = 0; i < 6; ++i) x0[i] = 0.1 + i / 3.0;
  x0[2] = -0.0;                                   // a signed zero travels as its bits
  for (int i = 0; i < 2 * (H + 1); ++i) xref[i] = 1.0 / (i + 1) - 0.25;
  for (int i = 0; i < 2 * H; ++i) mean[i] = (i % 2 ? -1.0 : 1.0) / (i + 3.0);
  up[0] = 0.3;
  up[1] = __builtin_nan("");                      // so does a NaN
  for (int i = 0; i < 6; ++i) nominal[i] = 10.0 + i;
  for (int i = 0; i < 6 * n; ++i) params[i] = 100.0 + i;
  const uint64_t seed = 0x123456789ABCDEFull;
  nlp_batch_pack(l, H, want.get(), x0.get(), xref.get(), up.get(), mean.get(), seed, 0, 1);
  // as the build kernel's threads do: thread `first` of `stride` writes its words
  for (int first = 0; first < stride; ++first)
    ctl_solve_record(got.get(), H, (uint32_t)l.up_off, x0.get(), xref.get(), mean.get(), up.get(), seed, first, stride);
  int bad = 0;
  for (size_t i = 0; i < l.rec_words; ++i) bad += want[i] != got[i];
  std::printf("%zu %zu %d\n", l.rec_words, l.up_off, bad);
  // the table: the nominal model while warm, else the bank's column; NaN for a column it does not hold
  for (int j = 0; j < 6; ++j) {
    const double v = ctl_solve_p6(j, warm != 0, nominal.get(), params.get(), n, col);
    const double w = warm ? nominal[j] : params[j * n + col];
    const double o1 = ctl_solve_p6(j, false, nominal.get(), params.get(), n, n), o2 = ctl_solve_p6(j, false, nominal.get(), params.get(), n, -1);
    std::printf("%d %d %d\n", j, (int)(std::memcmp(&v, &w, 8) == 0), (int)(o1 != o1 && o2 != o2));
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  auto I = [&](int i) { return std::atoll(argv[i]); };
  auto D = [&](int i) { return std::atof(argv[i]); };
  auto say = [](const char* why) { std::printf("%s\n", why ? why : "ok"); };
  if (mode == "record" && argc == 5) return record((int)I(2), (int)I(3), (int)I(4));
  if (mode == "state" && argc == 8) {
    say(ctl_solver_state_refused({I(2) != 0, I(3) != 0, I(4) != 0, I(5) != 0, I(6) != 0, D(7)}));
    return 0;
  }
  if (mode == "cfg" && argc == 8) {
    say(ctl_solver_cfg_refused((int32_t)I(2), D(3), (int32_t)I(4), (int32_t)I(5), D(6), (int32_t)I(7)));
    return 0;
  }
  if (mode == "blocks" && argc == 5) {
    say(ctl_solver_blocks(I(2) != 0, (CtlSetter)I(3), I(4) != 0));
    return 0;
  }
  if (mode == "applied" && argc == 4) {
    const int H = (int)I(2), bad = (int)I(3);
    std::unique_ptr<double[]> u0(new double[2]), useq(new double[2 * H]);
    u0[0] = u0[1] = 0.5;
    for (int i = 0; i < 2 * H; ++i) useq[i] = 0.25;
    if (bad >= 0 && bad < 2) u0[bad] = __builtin_nan("");
    if (bad >= 2) useq[bad - 2] = __builtin_inf();
    std::printf("%d %d\n", (int)ctl_applied_finite(u0.get(), useq.get(), H), (int)ctl_applied_finite(u0.get(), nullptr, H));
    return 0;
  }
  return 2;
}

// Host harness for the batched corridor solve's pure host helpers in csrc/capi_host.hpp (test
// infrastructure): the corridor buffer's layout and pack, the per-problem argument checks and the
// per-problem slack, run on the CPU — built with AddressSanitizer and UBSan (host code only), every
// buffer a heap block of exactly the size the layout claims, so a write past a problem's part or
// past the buffer's end is an error here before any GPU is involved.
//   nlp_batch_corridor_host layout H B       the layout, then per problem the count of wrong words
//   nlp_batch_corridor_host check B H bad_problem what     what: ok | normal | nan_off | ninf_off |
//                                            pinf_off | neg_w | nan_w | inf_w | null_w | nohp_neg_w
//   nlp_batch_corridor_host paths B H bad_problem entry    entry < 0: all finite
//   nlp_batch_corridor_host slack H                        arrived / failed / no tag, and the value
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "capi_host.hpp"

using namespace llampc;

static_assert(sizeof(NlpBatch) == 40, "NlpBatch layout: unchanged by the corridor");
static_assert(sizeof(NlpBatchCorridor) == 56, "NlpBatchCorridor layout");

static int layout(int H, int B) {
  const NlpBatchCorLayout c = nlp_batch_cor_layout();
  const NlpBatch bt = nlp_batch_arg(nlp_batch_layout(H, 64), nullptr, 64);
  std::unique_ptr<double[]> buf(new double[(size_t)B * c.cor_doubles]);
  const NlpBatchCorridor a = nlp_batch_cor_arg(bt, c, buf.get());
  std::printf("%zu %zu %zu %zu %u %u\n", c.cor_doubles, c.theta_off, c.w_off, c.path_doubles, a.cor_doubles, a.w_off);
  if (a.cor != buf.get() || a.bt.rec_words != bt.rec_words || a.bt.nl_log2 != bt.nl_log2) return 4;
  const double mark = -12345.0;
  for (size_t i = 0; i < (size_t)B * c.cor_doubles; ++i) buf[i] = mark;
  auto val = [](int p, int i) { return 1000.0 * p + i; };
  // packed last problem first, from an hp of exactly H rows; odd problems as the device builder's
  for (int p = B - 1; p >= 0; --p) {
    std::unique_ptr<double[]> hp(new double[6 * (size_t)H]);
    for (int i = 0; i < 6 * H; ++i) hp[i] = val(p, i);
    nlp_batch_cor_pack(c, H, buf.get() + p * c.cor_doubles, p % 2 ? nullptr : hp.get(), 0.5 + p);
  }
  for (int p = 0; p < B; ++p) {
    const double* d = buf.get() + p * c.cor_doubles;
    int bad = 0;
    for (size_t i = 0; i < c.cor_doubles; ++i) {
      const bool row = i < 6 * (size_t)H, th = i >= c.theta_off && i < c.theta_off + (size_t)H;
      if (i == c.w_off) bad += d[i] != 0.5 + p;
      else if (p % 2) bad += (row || th) ? !std::isnan(d[i]) : d[i] != mark;
      else bad += row ? d[i] != val(p, (int)i) : d[i] != mark;
    }
    std::printf("%d %d\n", p, bad);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  auto I = [&](int i) { return std::atoll(argv[i]); };
  if (mode == "layout" && argc == 4) return layout((int)I(2), (int)I(3));
  if (mode == "check" && argc == 6) {
    const int B = (int)I(2), H = (int)I(3), badp = (int)I(4);
    const std::string what = argv[5];
    std::vector<double> hp(6 * (size_t)H * B), w(B, 2.0);
    for (int q = 0; q < B; ++q)
      for (int k = 0; k < H; ++k) {
        double* r = hp.data() + 6 * ((size_t)H * q + k);
        r[0] = 1.0, r[1] = 0.5, r[2] = 3.0 + k, r[3] = -1.0, r[4] = -0.5, r[5] = HUGE_VAL;   // +inf: disabled, valid
      }
    double* r = hp.data() + 6 * ((size_t)H * badp + (H - 1));
    if (what == "normal") r[4] = HUGE_VAL;
    else if (what == "nan_off") r[2] = std::nan("");
    else if (what == "ninf_off") r[5] = -HUGE_VAL;
    else if (what == "pinf_off") r[2] = HUGE_VAL;
    else if (what == "neg_w" || what == "nohp_neg_w") w[badp] = -1.0;
    else if (what == "nan_w") w[badp] = std::nan("");
    else if (what == "inf_w") w[badp] = HUGE_VAL;
    char buf[160];
    const char* why = nlp_batch_corridor_invalid(B, H, what == "nohp_neg_w" ? nullptr : hp.data(),
                                                 what == "null_w" ? nullptr : w.data(), buf, sizeof buf);
    std::printf("%s\n", why ? why : "ok");
    return 0;
  }
  if (mode == "paths" && argc == 6) {
    const int B = (int)I(2), H = (int)I(3), badp = (int)I(4), entry = (int)I(5);
    std::vector<double> path(2 * (size_t)(H + 1) * B, 0.25);
    if (entry >= 0) path[2 * (size_t)(H + 1) * badp + entry] = entry % 2 ? std::nan("") : HUGE_VAL;
    char buf[96];
    const char* why = nlp_batch_paths_invalid(B, H, path.data(), buf, sizeof buf);
    std::printf("%s\n", why ? why : "ok");
    return 0;
  }
  if (mode == "slack" && argc == 3) {
    const int H = (int)I(2);
    std::vector<double> hp(6 * (size_t)H), traj(6 * (size_t)(H + 1), 0.0);
    for (int k = 0; k < H; ++k) {
      double* r = hp.data() + 6 * (size_t)k;
      r[0] = 1.0, r[1] = 0.0, r[2] = 1.0, r[3] = 0.0, r[4] = -1.0, r[5] = HUGE_VAL;      // X <= 1
      traj[6 * (size_t)(k + 1)] = 0.5 + 0.125 * k;                                         // X_k+1
    }
    const double want = std::max(0.0, (0.5 + 0.125 * (H - 1)) - 1.0);
    std::vector<double> nan_traj(traj.size(), std::nan(""));
    std::printf("%.17g %.17g %.17g %.17g %.17g\n", want, nlp_batch_slack(true, 0, hp.data(), traj.data(), H),
                nlp_batch_slack(true, -1, hp.data(), nan_traj.data(), H),
                nlp_batch_slack(false, 3, hp.data(), traj.data(), H), corridor_max_slack(hp.data(), traj.data(), H));
    return 0;
  }
  return 2;
}

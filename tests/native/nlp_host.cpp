// Host harness for the NLP solve's pure host section of csrc/capi_host.hpp (test infrastructure): the
// inline pack, the two result unpackers, the launch arguments, the built-corridor step and the refusals,
// run on the CPU — built with AddressSanitizer and UBSan (host code only), every buffer a heap block of
// exactly the size its user claims.  Words are printed as 64-bit hex so that the test compares bits.
// nlp.hip's LDS sizes are not linked here: the four functions below stand in for them, set per run.
//   nlp_host pack H with_base
//   nlp_host unpack single|batch arrived best_it H fval_null xmpc_null
//   nlp_host launch calls corridor ltraj_plain ltraj_corridor rounds
//   nlp_host built H weight solved bad_row      (bad_row >= 0: that row's first normal is NaN)
//   nlp_host margin margin width | path H bad value | bpath B H problem bad value
//   nlp_host cfg H samples elite iters Ts lds | ltraj fits_plain fits_corridor rerun
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "capi_host.hpp"

namespace llampc {
static size_t g_lds = 0;
static bool g_fits = false, g_fits_cor = false;
size_t nlp_lds_bytes(int, int, int, bool) { return g_lds; }
size_t nlp_corridor_lds_bytes(int H, int, int, bool) { return g_lds + 48 * (size_t)H; }
bool nlp_ltraj_fits(int, int, int) { return g_fits; }
bool nlp_corridor_ltraj_fits(int, int, int) { return g_fits_cor; }
}  // namespace llampc

using namespace llampc;

static const uint64_t kSentinel = 0xFFF8DEADBEEF0000ull;   // a NaN no helper writes
static uint64_t bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, sizeof u);
  return u;
}
static std::unique_ptr<double[]> block(size_t n) {
  std::unique_ptr<double[]> p(new double[n]);
  for (size_t i = 0; i < n; ++i) std::memcpy(&p[i], &kSentinel, sizeof kSentinel);
  return p;
}
static void dump(const char* name, const double* p, size_t n) {
  std::printf("%s", name);
  for (size_t i = 0; i < n; ++i) std::printf(" %016" PRIx64, bits(p[i]));
  std::printf("\n");
}
static double val(int field, int i) { return 100.0 * field + i + 0.25; }

static int pack(int H, bool with_base) {
  auto x0 = block(6), xref = block(2 * (H + 1)), up = block(2), base = block(2 * H);
  for (int i = 0; i < 6; ++i) x0[i] = val(0, i);
  for (int i = 0; i < 2 * (H + 1); ++i) xref[i] = val(1, i);
  for (int i = 0; i < 2; ++i) up[i] = val(2, i);
  for (int i = 0; i < 2 * H; ++i) base[i] = val(3, i);
  static_assert(sizeof(NlpInline) == kNlpInlineDoubles * sizeof(double), "NlpInline is its doubles");
  auto mem = block(kNlpInlineDoubles);
  nlp_inline_pack(*reinterpret_cast<NlpInline*>(mem.get()), H, x0.get(), xref.get(), up.get(), with_base ? base.get() : nullptr);
  dump("pk", mem.get(), kNlpInlineDoubles);
  return 0;
}

static int unpack(bool batch, bool arrived, int best_it, int H, bool fval_null, bool xmpc_null) {
  std::unique_ptr<NlpResult> r(new NlpResult());
  for (int i = 0; i < 2 * LLAMPC_HMAX; ++i) (&r->best_u[0][0])[i] = val(4, i);
  for (int i = 0; i < 6 * (LLAMPC_HMAX + 1); ++i) (&r->traj[0][0])[i] = val(5, i);
  r->best_j = val(6, 0);
  r->best_it = best_it;
  auto umpc = block(2 * H), fval = block(1), xmpc = block(6 * (H + 1));
  const int32_t st = batch ? nlp_batch_unpack(*r, arrived, H, umpc.get(), fval.get(), xmpc.get())
                           : nlp_result_unpack(*r, H, umpc.get(), fval_null ? nullptr : fval.get(), xmpc_null ? nullptr : xmpc.get());
  std::printf("status %d\n", st);
  dump("umpc", umpc.get(), 2 * H);
  dump("fval", fval.get(), 1);
  dump("xmpc", xmpc.get(), 6 * (H + 1));
  return 0;
}

static int launch(uint64_t calls, bool corridor, bool lp, bool lc, int rounds) {
  auto at = [](uintptr_t v) { return reinterpret_cast<void*>(v); };
  NlpLaunch a{};
  a.it = 77;
  nlp_launch_args(a, {(NlpState*)at(0x1000), (uint64_t*)at(0x2000), (double*)at(0x3000), (uint64_t*)at(0x4000),
                      (NlpResult*)at(0x5000), (uint64_t*)at(0x6000), calls, corridor, NlpLtraj{lp, lc}, rounds});
  std::printf("st=%p list_tag=%p cand=%p ms_tag=%p res=%p host_tag=%p host_seq=%" PRIu64 " call=%" PRIu64 " ltraj=%d it=%d rounds=%d\n",
              (void*)a.st, (void*)a.list_tag, (void*)a.cand, (void*)a.ms_tag, (void*)a.res, (void*)a.host_tag, a.host_seq,
              a.call, a.ltraj, a.it, a.rounds);
  // nothing else of the launch is touched
  NlpLaunch z{};
  z.st = a.st, z.list_tag = a.list_tag, z.cand = a.cand, z.ms_tag = a.ms_tag, z.res = a.res, z.host_tag = a.host_tag;
  z.host_seq = a.host_seq, z.call = a.call, z.ltraj = a.ltraj, z.it = a.it, z.rounds = a.rounds;
  std::printf("rest %d\n", std::memcmp(&a, &z, sizeof a));
  return 0;
}

static int built(int H, double weight, bool solved, int bad_row) {
  auto mapped = block(6 * H), out = block(6 * H), traj = block(6 * (H + 1)), slack = block(1);
  for (int k = 0; k < H; ++k) {
    const double row[6] = {1.0, 0.0, 0.5 + k, 0.0, -1.0, HUGE_VAL};
    std::memcpy(&mapped[6 * k], row, sizeof row);
  }
  if (bad_row >= 0) mapped[6 * bad_row] = __builtin_nan("");
  for (int i = 0; i < 6 * (H + 1); ++i) traj[i] = 0.75 * i;
  const char* why = nlp_built_corridor(mapped.get(), H, weight, out.get(), solved, traj.get(), slack.get());
  std::printf("why %s\n", why ? why : "ok");
  dump("hp_out", out.get(), 6 * H);
  dump("slack", slack.get(), 1);
  const double want = corridor_max_slack(mapped.get(), traj.get(), H);
  dump("want", &want, 1);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  auto I = [&](int i) { return std::atoll(argv[i]); };
  auto D = [&](int i) { return std::strtod(argv[i], nullptr); };
  char buf[160];
  auto say = [](const char* why) { return std::printf("%s\n", why ? why : "ok"), 0; };
  if (mode == "pack" && argc == 4) return pack((int)I(2), I(3) != 0);
  if (mode == "unpack" && argc == 8)
    return unpack(std::string(argv[2]) == "batch", I(3) != 0, (int)I(4), (int)I(5), I(6) != 0, I(7) != 0);
  if (mode == "launch" && argc == 7) return launch((uint64_t)I(2), I(3) != 0, I(4) != 0, I(5) != 0, (int)I(6));
  if (mode == "built" && argc == 6) return built((int)I(2), D(3), I(4) != 0, (int)I(5));
  if (mode == "margin" && argc == 4) return say(track_margin_refused(D(2), D(3), buf, sizeof buf));
  if ((mode == "path" && argc == 5) || (mode == "bpath" && argc == 7)) {
    const bool b = mode == "bpath";
    const int B = b ? (int)I(2) : 1, H = (int)I(b ? 3 : 2), q = b ? (int)I(4) : 0, bad = (int)I(b ? 5 : 3);
    auto path = block(2 * (size_t)(H + 1) * B);
    for (int i = 0; i < 2 * (H + 1) * B; ++i) path[i] = 0.5 * i;
    if (bad >= 0) path[2 * (H + 1) * q + bad] = D(b ? 6 : 4);
    return say(b ? nlp_batch_paths_invalid(B, H, path.get(), buf, sizeof buf) : path_invalid(path.get(), H, buf, sizeof buf));
  }
  if (mode == "cfg" && argc == 8) {
    llampc_nlp_cfg k{};
    k.H = (int32_t)I(2), k.samples = (int32_t)I(3), k.elite = (int32_t)I(4), k.iters = (int32_t)I(5), k.Ts = D(6);
    g_lds = (size_t)I(7);
    const char* why = nlp_cfg_invalid(k, buf, sizeof buf);
    const char* cor = nlp_corridor_cfg_invalid(k);
    return std::printf("%s\n%s\n", why ? why : "ok", cor ? cor : "ok"), 0;
  }
  if (mode == "ltraj" && argc == 5) {
    g_fits = I(2) != 0, g_fits_cor = I(3) != 0;
    const NlpLtraj f = nlp_ltraj_flags(llampc_nlp_cfg{}, I(4) != 0);
    return std::printf("%d %d\n", (int)f.plain, (int)f.corridor), 0;
  }
  return 2;
}

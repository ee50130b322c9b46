// Host harness for csrc/capi_host.hpp (test infrastructure): runs the C ABI's pure host helpers
// on the CPU and prints what they return, so tests/test_capi_native.py compares the values with
// its own arithmetic — built with AddressSanitizer and UBSan (host code only), every buffer a
// heap block of exactly the size the helper may touch.
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "capi_host.hpp"

using namespace llampc;

// Fake, distinct, never dereferenced device addresses.
template <class T>
static T* fake(uintptr_t a) { return reinterpret_cast<T*>(a); }
static unsigned long long addr(const void* p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }

static std::unique_ptr<double[]> ramp(size_t n, double base) {
  std::unique_ptr<double[]> v(new double[n]);
  for (size_t i = 0; i < n; ++i) v[i] = base + (double)i;
  return v;
}

static BankView fake_bank() {
  BankView b{};
  b.params = fake<double>(0x1000);
  b.n = 5;
  b.goff = 70;
  b.veh.lf = 0.5;
  b.veh.mass = 0.25;
  b.veh.input_acc = 1;
  b.veh.approx = 1;
  b.ring = fake<double>(0x2000);
  b.W = 3;
  b.slot = 2;
  b.wmean = fake<double>(0x3000);
  b.am_val = fake<double>(0x4000);
  b.am_idx = fake<int64_t>(0x5000);
  b.tk_val = fake<double>(0x6000);
  b.tk_idx = fake<int64_t>(0x7000);
  b.rl = fake<double>(0x80000);
  b.rl_n = 5;
  b.rl_M = 2;
  b.rl_hmin = 0.25;
  b.rl_vmax = 3.5;
  return b;
}

static void print_builders(const char* who, const BankView& b, int32_t integrator) {
  LookbackLaunch lb{};
  LookaheadLaunch la{};
  FinalLaunch f{};
  bank_lookback(b, lb);
  bank_lookahead(b, integrator, la);
  bank_final(b, f);
  std::printf("%s lb %llx %lld %lld %.17g %.17g %llx %d %d %llx %llx %llx %llx %llx\n", who, addr(lb.params),
              (long long)lb.n, (long long)lb.goff, lb.veh.lf, lb.veh.mass, addr(lb.ring), lb.W, lb.slot, addr(lb.wm_buf),
              addr(lb.am_val), addr(lb.am_idx), addr(lb.tk_val), addr(lb.tk_idx));
  std::printf("%s la %llx %lld %lld %.17g %.17g %d %d %d\n", who, addr(la.params), (long long)la.n, (long long)la.goff,
              la.veh.lf, la.veh.mass, la.veh.input_acc, la.veh.approx, la.integrator);
  std::printf("%s fin %llx %lld %lld %llx %llx %llx %llx\n", who, addr(f.params), (long long)f.n, (long long)f.goff,
              addr(f.am_val), addr(f.am_idx), addr(f.tk_val), addr(f.tk_idx));
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  auto arg = [&](int i) { return std::strtoll(argv[i], nullptr, 0); };
  auto uarg = [&](int i) { return std::strtoull(argv[i], nullptr, 0); };
  if (mode == "seq") {                   // seq s steps: the chain s -> next_seq(s) -> ...
    uint32_t s = (uint32_t)uarg(2);
    for (int i = 0; i < arg(3); ++i) std::printf("%u\n", s = next_seq(s));
  } else if (mode == "poll") {           // poll n C H: ticks, then the units under both clamps
    const uint64_t t = poll_bound_ticks(arg(2), (int32_t)arg(3), (int32_t)arg(4));
    std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", t, poll_units(t, INT32_MAX), poll_units(t, UINT32_MAX));
  } else if (mode == "units") {          // units ticks max
    std::printf("%" PRIu64 "\n", poll_units(uarg(2), uarg(3)));
  } else if (mode == "pack") {           // pack C H xref_mode do_lookahead with_prev
    llampc_plan_in in{};
    in.C = (int32_t)arg(2);
    in.H = (int32_t)arg(3);
    in.xref_mode = (int32_t)arg(4);
    in.do_lookahead = (int32_t)arg(5);
    in.do_lookback = 1;
    const bool prev = arg(6) != 0;
    const size_t nx = in.xref_mode == LLAMPC_XREF_RACELINE ? 3 : 2 * (size_t)(in.H + 1);
    const auto xp = ramp(6, 100), up = ramp(2, 200), xn = ramp(6, 300), upv = ramp(2, 400), xr = ramp(nx, 500),
               U = ramp(2 * (size_t)in.C * in.H, 1000);
    if (prev) in.x_prev = xp.get(), in.u_prev = up.get();
    in.x_now = xn.get();
    in.uprev = upv.get();
    in.xref = xr.get();
    in.U = U.get();
    const size_t len = pack_len(&in);
    std::unique_ptr<double[]> h(new double[len]);
    for (size_t i = 0; i < len; ++i) h[i] = -7.0;   // every slot must be written
    pack_into(&in, h.get());
    std::printf("%zu\n", len);
    for (size_t i = 0; i < len; ++i) std::printf("%.17g\n", h[i]);
  } else if (mode == "window") {         // window W n: every (count, slot); raw[s][i] = 10 s + i + 1
    const int32_t W = (int32_t)arg(2);
    const int64_t n = arg(3);
    std::unique_ptr<double[]> raw(new double[(size_t)W * n]), ring(new double[(size_t)W * n]);
    for (int s = 0; s < W; ++s)
      for (int64_t i = 0; i < n; ++i) raw[(size_t)s * n + i] = 10.0 * s + (double)i + 1.0;
    for (int32_t count = 0; count <= W; ++count)
      for (int32_t slot = 0; slot < W; ++slot) {
        for (size_t i = 0; i < (size_t)W * n; ++i) ring[i] = -7.0;
        window_unroll(raw.get(), n, W, count, slot, ring.get());
        for (size_t i = 0; i < (size_t)W * n; ++i) std::printf("%.17g ", ring[i]);
        std::printf("\n");
      }
  } else if (mode == "raceline") {       // the sections' offsets from knots, in doubles
    const BankView b = fake_bank();
    const RacelineK r = raceline_view(b);
    std::printf("%llx %lld %lld %lld %d %d %d %.17g %.17g\n", addr(r.knots), (long long)((addr(r.xy) - addr(r.knots)) / 8),
                (long long)((addr(r.speed) - addr(r.knots)) / 8), (long long)((addr(r.mus) - addr(r.knots)) / 8), r.n, r.M,
                r.wcap, r.hmin, r.vmax);
  } else if (mode == "builders") {       // a plan tick's (any integrator) and a controller tick's (RK4)
    const BankView b = fake_bank();
    print_builders("plan", b, (int32_t)arg(2));
    print_builders("ctl", b, LLAMPC_RK4);
  } else if (mode == "shape") {          // shape cus field=value ...: plan_shape of the named PlanShapeIn fields
    PlanShapeIn in{};
    in.share = 1;
    for (int i = 3; i < argc; ++i) {
      const std::string a = argv[i];
      const size_t eq = a.find('=');
      if (eq == std::string::npos) return 2;
      const std::string k = a.substr(0, eq);
      const long long v = std::strtoll(a.c_str() + eq + 1, nullptr, 0);
      if (k == "n") in.n = v;
      else if (k == "K") in.K = (int32_t)v;
      else if (k == "lb") in.lb = v != 0;
      else if (k == "full") in.full = v != 0;
      else if (k == "la") in.la = v != 0;
      else if (k == "C") in.C = (int32_t)v;
      else if (k == "H") in.H = (int32_t)v;
      else if (k == "integrator") in.integrator = (int32_t)v;
      else if (k == "xref_mode") in.xref_mode = (int32_t)v;
      else if (k == "rl_n") in.rl_n = (int32_t)v;
      else if (k == "rl_M") in.rl_M = (int32_t)v;
      else if (k == "share") in.share = (int32_t)v;
      else if (k == "px_G") in.px_G = (int32_t)v;
      else if (k == "pack") in.pack = v != 0;
      else if (k == "corridor") in.corridor = v != 0;
      else if (k == "wq_counter") in.wq_counter = v != 0;
      else return 2;
    }
    const PlanShape s = plan_shape(in, (int)arg(2));
    std::printf("family %d\ninteg %d\nlpm %d\nG %d\ncpl %d\nstage %d\nwq %d\npx %d\nxm %d\nR %d\nnb_lb %d\nnb_la %d\n"
                "threads %d\nlds %zu\nwcap %d\nrefuse %s\n",
                (int)s.family, s.integ, s.lpm, s.G, s.cpl, (int)s.stage, s.wq, (int)s.px, (int)s.xm, s.R, s.nb_lb,
                s.nb_la, s.threads, s.lds, s.wcap, s.refuse ? s.refuse : "-");
  } else if (mode == "ctl_shape") {      // ctl_shape n C H K rl_n warm do_lb no_stage px_G
    const CtlShape s = ctl_shape(arg(2), (int32_t)arg(3), (int32_t)arg(4), (int32_t)arg(5), (int32_t)arg(6),
                                 arg(7) != 0, arg(8) != 0, arg(9) != 0, (int)arg(10));
    std::printf("lpm %d\nG %d\ncpl %d\nmpb %d\ns4 %d\nzfit %d\nR %d\nnb_lb %d\nnb_la %d\nnslots %d\nlds %zu\n"
                "poll_off %zu\n",
                s.lpm, s.G, s.cpl, s.mpb, s.s4, s.zfit, s.R, s.nb_lb, s.nb_la, s.nslots, s.lds, s.poll_off);
  } else if (mode == "spin") {          // spin code: a tag that never comes, 1 ms bound, on_timeout returns code
    uint64_t tag = 41;
    int timeouts = 0;
    const auto never = [](uint64_t) { return false; };
    const auto ms = std::chrono::milliseconds(1);
    // the tag already there; a tag the predicate stops on: on_timeout never runs
    const int a = spin_for_tag(&tag, 41, [&] { return ++timeouts; });
    const int b = spin_for_tag(&tag, 42, [&] { return ++timeouts; }, [](uint64_t v) { return v == 41; });
    std::printf("%d %d %d\n", a, b, timeouts);
    // the bound runs out: on_timeout's code is passed on as it is; 0 and no tag: the timeout;
    // 0 and the tag arrived meanwhile: success
    const int code = (int)arg(2);
    const int c = spin_for_tag(&tag, 42, [&] { return ++timeouts, code; }, never, ms);
    const int d = spin_for_tag(&tag, 42, [&] { return ++timeouts, 0; }, never, ms);
    const int e = spin_for_tag(&tag, 42, [&] { return ++timeouts, tag = 42, 0; }, never, ms);
    std::printf("%d %d %d %d\n", c, d, e, timeouts);
    std::printf("%d %d %d %d\n", kSpinStopped, kSpinTimeout, (int)LLAMPC_E_ARG, (int)LLAMPC_E_HIP);
  } else {
    return 2;
  }
  return 0;
}

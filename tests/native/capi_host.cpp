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

// field=value arguments from argv[from] on; a field not named reads as its default.
struct Fields {
  int argc;
  char** argv;
  int from;
  const char* find(const char* k) const {
    const size_t n = std::strlen(k);
    for (int i = from; i < argc; ++i)
      if (!std::strncmp(argv[i], k, n) && argv[i][n] == '=') return argv[i] + n + 1;
    return nullptr;
  }
  long long i(const char* k, long long dflt = 0) const {
    const char* v = find(k);
    return v ? std::strtoll(v, nullptr, 0) : dflt;
  }
  unsigned long long u(const char* k, unsigned long long dflt = 0) const {
    const char* v = find(k);
    return v ? std::strtoull(v, nullptr, 0) : dflt;
  }
  double d(const char* k, double dflt) const {
    const char* v = find(k);
    return v ? std::strtod(v, nullptr) : dflt;
  }
};

// What a plan tick takes from a bank, at fake addresses (fake_bank's and 0x9000 on).
static PlanView fake_plan_view(bool px) {
  PlanView v{};
  v.bank = fake_bank();
  v.best_cand = fake<int32_t>(0x9000);
  v.best_cost = fake<double>(0xA000);
  v.pv = fake<double>(0xB000);
  v.pidx = fake<int64_t>(0xC000);
  v.pnf = fake<int32_t>(0xD000);
  v.la_tag = fake<uint64_t>(0xE000);
  v.blk_tag = fake<uint64_t>(0xF000);
  v.wq = fake<uint64_t>(0x10000);
  v.tickets = fake<unsigned>(0x11000);
  v.xref_pm = fake<double>(0x12000);
  v.track = fake<double>(0x20000);
  v.tr_n = 4;
  v.tr_L = 8.0;
  v.tr_width = 2.4;
  v.trk = fake<double>(0x30000);
  v.trk_flags = fake<int32_t>(0x40000);
  v.hp_tag = fake<uint64_t>(0x50000);
  if (px) {
    v.px_box = fake<uint64_t*>(0x60000);
    v.px_G = 2;
    v.px_rank = 1;
    v.px_bound = 1000000000ull;
  }
  return v;
}

// The host state of a bank and of a mailbox, as plan_tick_state / plan_tick_commit name their fields.
struct FakeBankState {
  int32_t count, slot, W;
  uint32_t seq, tseq;
  int32_t trk_cur;
  TrackPathState trk_path;
  int32_t trk_last_H;
};
struct FakeBox {
  uint32_t seq;
};

static void pp(int t, const char* k, const void* p) { std::printf("t%d.%s %llx\n", t, k, addr(p)); }
static void pi(int t, const char* k, long long v) { std::printf("t%d.%s %lld\n", t, k, v); }
static void pd(int t, const char* k, double v) { std::printf("t%d.%s %.17g\n", t, k, v); }

static void print_prep(int t, const PlanPrep& p) {
  pi(t, "has.lb", p.lb), pi(t, "has.la", p.la), pi(t, "has.tt", p.tt);
  if (p.lb) {
    const LookbackLaunch& l = p.lbl;
    pp(t, "lb.params", l.params), pi(t, "lb.n", l.n), pi(t, "lb.goff", l.goff), pd(t, "lb.veh.lf", l.veh.lf);
    pd(t, "lb.veh.mass", l.veh.mass), pp(t, "lb.x_prev", l.x_prev), pp(t, "lb.u_prev", l.u_prev), pp(t, "lb.x_now", l.x_now);
    pd(t, "lb.Ts", l.Ts), pp(t, "lb.ring", l.ring), pi(t, "lb.W", l.W), pi(t, "lb.slot", l.slot), pi(t, "lb.full", l.full);
    pi(t, "lb.K", l.K), pi(t, "lb.nan_first", l.nan_first), pi(t, "lb.R", l.R), pi(t, "lb.wm_keep", l.wm_keep);
    pp(t, "lb.err_out", l.err_out), pp(t, "lb.wm_buf", l.wm_buf), pp(t, "lb.am_val", l.am_val), pp(t, "lb.am_idx", l.am_idx);
    pp(t, "lb.tk_val", l.tk_val), pp(t, "lb.tk_idx", l.tk_idx);
  }
  if (p.la) {
    const LookaheadLaunch& l = p.lal;
    pp(t, "la.params", l.params), pi(t, "la.n", l.n), pi(t, "la.goff", l.goff), pd(t, "la.veh.lf", l.veh.lf);
    pd(t, "la.veh.mass", l.veh.mass), pi(t, "la.veh.input_acc", l.veh.input_acc), pi(t, "la.veh.approx", l.veh.approx);
    pp(t, "la.x0", l.x0), pp(t, "la.U", l.U), pp(t, "la.xref", l.xref), pp(t, "la.uprev", l.uprev);
    pi(t, "la.C", l.C), pi(t, "la.H", l.H), pi(t, "la.integrator", l.integrator), pd(t, "la.Ts", l.Ts);
    for (int i = 0; i < 4; ++i) {
      char k[32];
      std::snprintf(k, sizeof k, "la.cost.Q%d", i), pd(t, k, l.cost.Q[i]);
      std::snprintf(k, sizeof k, "la.cost.R%d", i), pd(t, k, l.cost.R[i]);
      std::snprintf(k, sizeof k, "la.cost.P%d", i), pd(t, k, l.cost.P[i]);
    }
    for (int i = 0; i < 2; ++i) {
      char k[32];
      std::snprintf(k, sizeof k, "la.cost.umin%d", i), pd(t, k, l.cost.umin[i]);
      std::snprintf(k, sizeof k, "la.cost.umax%d", i), pd(t, k, l.cost.umax[i]);
      std::snprintf(k, sizeof k, "la.cost.dmax%d", i), pd(t, k, l.cost.dmax[i]);
    }
    pi(t, "la.cost.enforce", l.cost.enforce), pi(t, "la.cost.pad", l.cost.pad);
    pp(t, "la.cost_out", l.cost_out), pp(t, "la.best_cand", l.best_cand), pp(t, "la.best_cost", l.best_cost);
    pp(t, "la.pv", l.pv), pp(t, "la.pidx", l.pidx), pp(t, "la.pnf", l.pnf), pi(t, "la.xref_mode", l.xref_mode);
    pp(t, "la.rl.knots", l.rl.knots), pp(t, "la.rl.xy", l.rl.xy), pp(t, "la.rl.speed", l.rl.speed), pp(t, "la.rl.mus", l.rl.mus);
    pi(t, "la.rl.n", l.rl.n), pi(t, "la.rl.M", l.rl.M), pi(t, "la.rl.wcap", l.rl.wcap), pd(t, "la.rl.hmin", l.rl.hmin);
    pd(t, "la.rl.vmax", l.rl.vmax), pp(t, "la.xref_pm", l.xref_pm), pp(t, "la.la_tag", l.la_tag), pp(t, "la.blk_tag", l.blk_tag);
    pi(t, "la.seq", l.seq), pi(t, "la.poll", l.poll), pp(t, "la.wq", l.wq);
  }
  const FinalLaunch& f = p.f;
  pp(t, "f.out", f.out), pp(t, "f.tickets", f.tickets), pi(t, "f.do_lb", f.do_lb), pi(t, "f.do_la", f.do_la);
  pi(t, "f.full", f.full), pi(t, "f.window_count", f.window_count), pi(t, "f.K", f.K), pi(t, "f.nan_first", f.nan_first);
  pi(t, "f.nb_lb", f.nb_lb), pi(t, "f.nb_la", f.nb_la), pi(t, "f.C", f.C), pi(t, "f.current_model", f.current_model);
  pi(t, "f.n", f.n), pi(t, "f.goff", f.goff), pp(t, "f.params", f.params), pp(t, "f.best_cand", f.best_cand);
  pp(t, "f.best_cost", f.best_cost), pp(t, "f.am_val", f.am_val), pp(t, "f.am_idx", f.am_idx), pp(t, "f.tk_val", f.tk_val);
  pp(t, "f.tk_idx", f.tk_idx), pp(t, "f.pv", f.pv), pp(t, "f.pidx", f.pidx), pp(t, "f.pnf", f.pnf);
  pp(t, "f.la_tag", f.la_tag), pp(t, "f.blk_tag", f.blk_tag), pi(t, "f.seq", f.seq), pi(t, "f.poll", f.poll);
  pp(t, "f.host_tag", f.host_tag), pi(t, "f.host_seq", (long long)f.host_seq), pp(t, "f.px_box", f.px_box);
  pp(t, "f.px_merged", f.px_merged), pi(t, "f.px_G", f.px_G), pi(t, "f.px_rank", f.px_rank), pi(t, "f.px_seq", f.px_seq);
  pi(t, "f.px_bound", f.px_bound), pp(t, "f.wq", f.wq);
  if (p.tt) {
    const PlanTrack& k = p.trk;
    pp(t, "trk.cx", k.trk.cx), pp(t, "trk.cy", k.trk.cy), pp(t, "trk.tt", k.trk.tt), pi(t, "trk.n", k.trk.n);
    pi(t, "trk.npad", k.trk.pad), pd(t, "trk.L", k.trk.L), pd(t, "trk.hw", k.hw), pd(t, "trk.weight", k.weight);
    pp(t, "trk.hp_tag", k.hp_tag), pp(t, "trk.path_rd", k.path_rd), pp(t, "trk.path_wr", k.path_wr);
    pp(t, "trk.valid_rd", k.valid_rd), pp(t, "trk.valid_wr", k.valid_wr), pp(t, "trk.cost_wr", k.cost_wr);
    pp(t, "trk.dbg", k.dbg), pp(t, "trk.dbg_valid", k.dbg_valid), pp(t, "trk.late", k.late), pi(t, "trk.seq", k.seq);
    pi(t, "trk.poll", k.poll), pi(t, "trk.path_ok", k.path_ok), pi(t, "trk.pad", k.pad);
  }
  const PlanTickState& n = p.next;
  pi(t, "next.count", n.count), pi(t, "next.slot", n.slot), pi(t, "next.W", n.W), pi(t, "next.seq", n.seq);
  pi(t, "next.tseq", n.tseq), pi(t, "next.trk_cur", n.trk_cur), pi(t, "next.trk_path", n.trk_path.H);
  pi(t, "next.trk_last_H", n.trk_last_H), pi(t, "next.px_seq", n.px_seq);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  auto arg = [&](int i) { return std::strtoll(argv[i], nullptr, 0); };
  auto uarg = [&](int i) { return std::strtoull(argv[i], nullptr, 0); };
  if (mode == "prep") {
    // prep field=value ...: `ticks` plan ticks of one kind chained through plan_tick_commit on a fake bank
    // (and mailbox): lb la xref_mode integrator C H K Ts nan_policy current_model | err wmean cost host px tt
    // | the state count slot W seq tseq trk_cur path_H px_seq.  pk and cor are always set: prepare reads neither.
    const Fields a{argc, argv, 2};
    llampc_plan_in in{};
    in.x_prev = fake<double>(0x100000);
    in.u_prev = fake<double>(0x100100);
    in.x_now = fake<double>(0x100200);
    in.U = fake<double>(0x100300);
    in.xref = fake<double>(0x100400);
    in.uprev = fake<double>(0x100500);
    in.do_lookback = (int32_t)a.i("lb", 1);
    in.do_lookahead = (int32_t)a.i("la", 1);
    in.xref_mode = (int32_t)a.i("xref_mode", LLAMPC_XREF_GIVEN);
    in.integrator = (int32_t)a.i("integrator", LLAMPC_RK4);
    in.C = (int32_t)a.i("C", 2);
    in.H = (int32_t)a.i("H", 3);
    in.K = (int32_t)a.i("K", 4);
    in.Ts = a.d("Ts", 0.02);
    in.nan_policy = (int32_t)a.i("nan_policy", LLAMPC_NAN_FIRST);
    in.current_model = a.i("current_model", 3);
    for (int i = 0; i < 4; ++i) in.cost.Q[i] = 1 + i, in.cost.R[i] = 10 + i, in.cost.P[i] = 20 + i;
    in.cost.umin[0] = -0.1, in.cost.umin[1] = -0.35, in.cost.umax[0] = 1.0, in.cost.umax[1] = 0.35;
    in.cost.rate_max[0] = -1.0, in.cost.rate_max[1] = 2.0;
    in.cost.enforce_bounds = 1;
    static const InlinePack pk{};
    const PlanCorridor cor{fake<double>(0x206000), 7.0};
    const TrackTick tt{a.d("tw", 1e4), a.d("margin", 0.05)};
    PlanTick t;
    t.out = fake<llampc_plan_out>(0x200000);
    if (a.i("err")) t.err = fake<double>(0x201000);
    if (a.i("wmean")) t.wmean = fake<double>(0x202000);
    if (a.i("cost")) t.cost = fake<double>(0x203000);
    if (a.i("host")) t.host_tag = fake<uint64_t>(0x204000), t.host_seq = 9;
    if (a.i("pk")) t.pk = &pk;
    if (a.i("cor")) t.cor = &cor;
    if (a.i("px")) t.px = fake<llampc_mailbox>(0x300000), t.px_merged = fake<llampc_plan_out>(0x205000);
    if (a.i("tt")) t.tt = &tt;
    FakeBankState bank{(int32_t)a.i("count", 1), (int32_t)a.i("slot", 2), (int32_t)a.i("W", 3), (uint32_t)a.u("seq", 7),
                       (uint32_t)a.u("tseq", 11), (int32_t)a.i("trk_cur", 0), TrackPathState{(int32_t)a.i("path_H", 0)},
                       (int32_t)a.i("last_H", 0)};
    FakeBox box{(uint32_t)a.u("px_seq", 5)};
    FakeBox* px = t.px ? &box : nullptr;
    const PlanView v = fake_plan_view(t.px != nullptr);
    for (int k = 0; k < a.i("ticks", 1); ++k) {
      const PlanPrep p = plan_tick_prepare(v, plan_tick_state(bank, px), in, t);
      print_prep(k, p);
      plan_tick_commit(bank, px, p.next);
      pi(k, "bank.count", bank.count), pi(k, "bank.slot", bank.slot), pi(k, "bank.W", bank.W), pi(k, "bank.seq", bank.seq);
      pi(k, "bank.tseq", bank.tseq), pi(k, "bank.trk_cur", bank.trk_cur), pi(k, "bank.trk_path", bank.trk_path.H);
      pi(k, "bank.trk_last_H", bank.trk_last_H), pi(k, "box.seq", box.seq);
    }
    return 0;
  }
  if (mode == "track_layout") {
    constexpr PlanTrackLayout L = plan_track_layout();
    std::printf("row %zu\npath_doubles %zu\nrb_path %zu\nrb_hp %zu\nrb_theta %zu\ntrk_doubles %zu\nflag_rb_valid %d\n"
                "flag_late %d\nflags %d\nhp_tag_words %zu\npath0 %zu\npath1 %zu\ncost0 %zu\ncost1 %zu\nvalid0 %d\nvalid1 %d\n"
                "kPlanPathStride %d\nkPlanTrackDbgDoubles %d\nHMAX %d\n",
                L.row, L.path_doubles, L.rb_path, L.rb_hp, L.rb_theta, L.trk_doubles, L.flag_rb_valid, L.flag_late, L.flags,
                L.hp_tag_words, L.path(0), L.path(1), L.cost(0), L.cost(1), L.valid(0), L.valid(1), kPlanPathStride,
                kPlanTrackDbgDoubles, LLAMPC_HMAX);
    return 0;
  }
  if (mode == "refuse") {
    // refuse field=value ...: plan_entry_refused of one entry: `code message` (0 and nothing when accepted).
    // The bank: n raceline tr_n tr_width async.  The input: null_in lb la K C H integrator xref_mode Ts and
    // no_prev / no_now / no_U (null pointers).  hp=1: a corridor entry (weight, hp_bad: a NaN normal in row
    // H - 1); tt=1: a track entry (tw, margin).
    const Fields a{argc, argv, 2};
    const PlanBankFacts b{a.i("n", 70), a.i("raceline") != 0, (int32_t)a.i("tr_n", 4), a.d("tr_width", 2.4), a.i("async") != 0};
    const auto x = ramp(6, 0);
    llampc_plan_in in{};
    in.do_lookback = (int32_t)a.i("lb", 1);
    in.do_lookahead = (int32_t)a.i("la", 1);
    in.K = (int32_t)a.i("K", 2);
    in.C = (int32_t)a.i("C", 2);
    in.H = (int32_t)a.i("H", 3);
    in.integrator = (int32_t)a.i("integrator", LLAMPC_RK4);
    in.xref_mode = (int32_t)a.i("xref_mode", LLAMPC_XREF_GIVEN);
    in.Ts = a.d("Ts", 0.02);
    if (!a.i("no_prev")) in.x_prev = in.u_prev = x.get();
    if (!a.i("no_now")) in.x_now = x.get();
    if (!a.i("no_U")) in.U = in.xref = in.uprev = x.get();   // never read: only tested for null
    std::unique_ptr<double[]> hp;
    if (a.i("hp")) {
      const size_t rows = in.H > 0 && in.H <= LLAMPC_HMAX ? (size_t)in.H : 1;   // exactly what corridor_invalid may read
      hp.reset(new double[6 * rows]);
      for (size_t i = 0; i < 6 * rows; ++i) hp[i] = 0.5;
      if (a.i("hp_bad")) hp[6 * (rows - 1) + 1] = __builtin_nan("");
    }
    const TrackTick tt{a.d("tw", 1e4), a.d("margin", 0.05)};
    char why[256] = "";
    const int rc = plan_entry_refused(b, a.i("null_in") ? nullptr : &in, hp.get(), a.d("weight", 1e4),
                                      a.i("tt") ? &tt : nullptr, why, sizeof why);
    std::printf("%d %s\n", rc, why);
    return 0;
  }
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

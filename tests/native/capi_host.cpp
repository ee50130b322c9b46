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

static const char* g_pfx = "";           // between the tick and the field's name (ctl_prep: the split's halves)
static void pp(int t, const char* k, const void* p) { std::printf("t%d.%s%s %llx\n", t, g_pfx, k, addr(p)); }
static void pi(int t, const char* k, long long v) { std::printf("t%d.%s%s %lld\n", t, g_pfx, k, v); }
static void pd(int t, const char* k, double v) { std::printf("t%d.%s%s %.17g\n", t, g_pfx, k, v); }

static void print_lookback(int t, const LookbackLaunch& l) {
    pp(t, "lb.params", l.params), pi(t, "lb.n", l.n), pi(t, "lb.goff", l.goff), pd(t, "lb.veh.lf", l.veh.lf);
    pd(t, "lb.veh.mass", l.veh.mass), pp(t, "lb.x_prev", l.x_prev), pp(t, "lb.u_prev", l.u_prev), pp(t, "lb.x_now", l.x_now);
    pd(t, "lb.Ts", l.Ts), pp(t, "lb.ring", l.ring), pi(t, "lb.W", l.W), pi(t, "lb.slot", l.slot), pi(t, "lb.full", l.full);
    pi(t, "lb.K", l.K), pi(t, "lb.nan_first", l.nan_first), pi(t, "lb.R", l.R), pi(t, "lb.wm_keep", l.wm_keep);
    pp(t, "lb.err_out", l.err_out), pp(t, "lb.wm_buf", l.wm_buf), pp(t, "lb.am_val", l.am_val), pp(t, "lb.am_idx", l.am_idx);
    pp(t, "lb.tk_val", l.tk_val), pp(t, "lb.tk_idx", l.tk_idx);
}

static void print_lookahead(int t, const LookaheadLaunch& l) {
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

static void print_final(int t, const FinalLaunch& f) {
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
}

static void print_prep(int t, const PlanPrep& p) {
  pi(t, "has.lb", p.lb), pi(t, "has.la", p.la), pi(t, "has.tt", p.tt);
  if (p.lb) print_lookback(t, p.lbl);
  if (p.la) print_lookahead(t, p.lal);
  print_final(t, p.f);
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

// The host state of a controller, as ctl_tick_state / ctl_tick_commit name its fields (its bank's:
// FakeBankState, its mailbox's: FakeBox).
struct FakeCtl {
  int64_t t;
  uint64_t hseq;
  uint32_t seq, door_ctr;
  int32_t hint_p0;
  double hint_mu;
  bool cor_prev;
  int32_t cor_nslots;
  uint32_t xg_seq;
};

// What a controller tick takes, at fake addresses (fake_bank's and 0x400000 on); cfg and mus: the caller's.
static CtlView fake_ctl_view(const llampc_ctl_cfg* cfg, const double* mus, const Fields& a) {
  CtlView v{};
  v.bank = fake_bank();
  v.cfg = cfg;
  v.st = fake<CtlState>(0x400000);
  v.out = fake<llampc_ctl_out>(0x401000);
  v.host_tag = fake<uint64_t>(0x402000);
  v.sel_tag = fake<uint64_t>(0x403000);
  v.slot_tag = fake<uint64_t>(0x404000);
  v.tickets = fake<unsigned>(0x405000);
  v.dbg = fake<double>(0x406000);
  v.znoise = fake<double>(0x407000);
  v.ztag = fake<uint64_t>(0x408000);
  v.pts = fake<double>(0x409000);
  v.prefix = fake<double>(0x409800);
  v.np = 9;
  v.door = fake<uint64_t>(0x40A000);
  v.door_dev = fake<uint64_t>(0x40B000);
  v.spec_val = fake<double>(0x40C000);
  v.spec_idx = fake<int64_t>(0x40D000);
  v.spec_tag = fake<uint64_t>(0x40E000);
  v.spec_res = fake<uint64_t>(0x40F000);
  v.xref_tag = fake<uint64_t>(0x410000);
  v.spec_nb = (int32_t)a.i("spec_nb", 1);
  v.spec_cap = (int32_t)a.i("spec_cap", 32);
  v.no_spec = a.i("no_spec") != 0;
  v.no_stage = a.i("no_stage") != 0;
  v.cus = (int32_t)a.i("cus", 256);
  v.share = (int32_t)a.i("share", 1);
  v.rl_mus = mus;
  const std::string tr = a.find("transport") ? a.find("transport") : "none";
  if (tr != "none") {
    v.gparams = fake<double>(0x411000);
    v.n_global = a.i("n_global", 12);
  }
  if (tr == "mailbox") {
    v.mailbox = true;
    v.px_box = fake<uint64_t*>(0x412000);
    v.px_world = 2;
    v.px_rank = 1;
    v.px_bound = 1000000000ull;
  } else if (tr == "gather") {
    v.xg_world = 3;
    v.xg_rank = 2;
    v.xsend = fake<uint64_t>(0x413000);
    v.xgath = fake<uint64_t>(0x414000);
  }
  v.track = fake<double>(0x420000);
  v.tr_n = 4;
  v.tr_L = 8.0;
  v.tr_width = 2.4;
  v.cor_w = a.d("cor_w", 0.0);
  v.cor_margin = a.d("cor_margin", 0.05);
  v.cor = fake<double>(0x430000);
  v.cor_flag = fake<int32_t>(0x440000);
  v.hp_tag = fake<uint64_t>(0x450000);
  v.cor_cost = fake<double>(0x460000);
  return v;
}

static void print_ctl_launch(int t, const CtlLaunch& L, int lpm, size_t lds) {
  char k[32];
  print_lookback(t, L.lb), print_lookahead(t, L.la), print_final(t, L.fin);
  pp(t, "L.st", L.st), pp(t, "L.out", L.out), pp(t, "L.host_tag", L.host_tag), pi(t, "L.host_seq", (long long)L.host_seq);
  pp(t, "L.sel_tag", L.sel_tag), pp(t, "L.slot_tag", L.slot_tag), pp(t, "L.tickets", L.tickets), pp(t, "L.dbg", L.dbg);
  pp(t, "L.znoise", L.znoise), pp(t, "L.ztag", L.ztag), pp(t, "L.pts", L.pts), pp(t, "L.prefix", L.prefix);
  pi(t, "L.tick", (long long)L.tick), pi(t, "L.seed", (long long)L.seed);
  for (int j = 0; j < 6; ++j) {
    std::snprintf(k, sizeof k, "L.x_t%d", j), pd(t, k, L.x_t[j]);
    std::snprintf(k, sizeof k, "L.nominal%d", j), pd(t, k, L.nominal[j]);
  }
  for (int j = 0; j < 2; ++j) {
    std::snprintf(k, sizeof k, "L.nscale%d", j), pd(t, k, L.nscale[j]);
    std::snprintf(k, sizeof k, "L.rate%d", j), pd(t, k, L.rate[j]);
    std::snprintf(k, sizeof k, "L.umin%d", j), pd(t, k, L.umin[j]);
    std::snprintf(k, sizeof k, "L.umax%d", j), pd(t, k, L.umax[j]);
  }
  pd(t, "L.mu_fixed", L.mu_fixed), pd(t, "L.scale_fixed", L.scale_fixed), pd(t, "L.v_factor", L.v_factor);
  pd(t, "L.mu_init", L.mu_init), pi(t, "L.poll_off", (long long)L.poll_off), pi(t, "L.seq", L.seq), pi(t, "L.poll", L.poll);
  pi(t, "L.np", L.np), pi(t, "L.lap_projidx", L.lap_projidx), pi(t, "L.do_lb", L.do_lb), pi(t, "L.warm", L.warm);
  pi(t, "L.use_mu", L.use_mu), pi(t, "L.full", L.full), pi(t, "L.nslots", L.nslots), pi(t, "L.mpb", L.mpb), pi(t, "L.G", L.G);
  pi(t, "L.cpl", L.cpl), pi(t, "L.S", L.S), pi(t, "L.K", L.K), pi(t, "L.nb_lb", L.nb_lb), pi(t, "L.nb_la", L.nb_la);
  pi(t, "L.s4", L.s4), pi(t, "L.p0_walk", L.p0_walk), pi(t, "L.br.lo", L.br_walk.lo), pi(t, "L.br.hi", L.br_walk.hi);
  pi(t, "L.br.single", L.br_walk.single), pd(t, "L.br.wa", L.br_walk.wa), pd(t, "L.br.wb", L.br_walk.wb);
  pd(t, "L.br.den", L.br_walk.den), pi(t, "L.sel_goff", L.sel_goff), pp(t, "L.px_box", L.px_box), pi(t, "L.px_G", L.px_G);
  pi(t, "L.px_rank", L.px_rank), pi(t, "L.px_seq", L.px_seq), pi(t, "L.px_bound", L.px_bound), pi(t, "L.px_phase", L.px_phase);
  pp(t, "L.px_send", L.px_send), pp(t, "L.px_gath", L.px_gath), pi(t, "L.px_spec_off", L.px_spec_off);
  pi(t, "L.px_spec_wait", L.px_spec_wait), pp(t, "L.door", L.door), pp(t, "L.door_dev", L.door_dev);
  pi(t, "L.door_seq", L.door_seq), pi(t, "L.door_bound", L.door_bound), pi(t, "L.n_spec", L.n_spec);
  pp(t, "L.spec_val", L.spec_val), pp(t, "L.spec_idx", L.spec_idx), pp(t, "L.spec_tag", L.spec_tag);
  pp(t, "L.spec_res", L.spec_res), pp(t, "L.xref_tag", L.xref_tag);
  pi(t, "lpm", lpm), pi(t, "lds", (long long)lds);
}

static void print_ctl_prep(int t, const CtlPrep& P) {
  print_ctl_launch(t, P.L, P.lpm, P.lds);
  pi(t, "corr", P.corr);
  if (P.corr) {
    const CtlCorridor& q = P.cor;
    pp(t, "cor.cx", q.trk.cx), pp(t, "cor.cy", q.trk.cy), pp(t, "cor.tt", q.trk.tt), pi(t, "cor.n", q.trk.n);
    pi(t, "cor.npad", q.trk.pad), pd(t, "cor.L", q.trk.L), pd(t, "cor.hw", q.hw), pd(t, "cor.weight", q.weight);
    pp(t, "cor.hp_tag", q.hp_tag), pp(t, "cor.path_rd", q.path_rd), pp(t, "cor.path_wr", q.path_wr);
    pp(t, "cor.valid_rd", q.valid_rd), pp(t, "cor.valid_wr", q.valid_wr), pp(t, "cor.dbg", q.dbg);
    pp(t, "cor.dbg_valid", q.dbg_valid), pi(t, "cor.path_ok", q.path_ok), pi(t, "cor.pad", q.pad), pp(t, "cor.dbg_cost", q.dbg_cost);
  }
  if (P.L.px_phase == 1) {               // the gather transport's two launches
    CtlPrep a, b;
    ctl_gather_split(P, a, b);
    g_pfx = "s1.", print_ctl_launch(t, a.L, a.lpm, a.lds);
    g_pfx = "s2.", print_ctl_launch(t, b.L, b.lpm, b.lds);
    g_pfx = "";
  }
  const CtlTickState& n = P.next;
  pi(t, "next.t", n.t), pi(t, "next.hseq", (long long)n.hseq), pi(t, "next.seq", n.seq), pi(t, "next.door_ctr", n.door_ctr);
  pi(t, "next.hint_p0", n.hint_p0), pd(t, "next.hint_mu", n.hint_mu), pi(t, "next.cor_prev", n.cor_prev);
  pi(t, "next.cor_nslots", n.cor_nslots), pi(t, "next.count", n.count), pi(t, "next.slot", n.slot), pi(t, "next.W", n.W);
  pi(t, "next.px_seq", n.px_seq), pi(t, "next.px", n.px);
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
  if (mode == "ctl_prep") {
    // ctl_prep field=value ...: controller ticks on a fake controller, bank and mailbox, one per letter of
    // `kinds`: l launched, a armed and rung (ctl_arm stores the doorbell number, the fire commits), f armed
    // but its launch call failed (the number is stored and nothing else).  A refused prepare prints its code
    // and message and commits nothing.  The cfg: C H K Ts nan_policy q1 (an off-diagonal Q); the view:
    // transport=none|mailbox|gather n_global cor_w cor_margin spec_nb spec_cap no_spec no_stage cus share;
    // the state: t hseq seq door_ctr hint_p0 hint_mu cor_prev count slot px_seq; reset=k: the window is
    // emptied before step k (llampc_bank_reset).
    const Fields a{argc, argv, 2};
    llampc_ctl_cfg cfg{};
    cfg.C = (int32_t)a.i("C", 2), cfg.H = (int32_t)a.i("H", 3), cfg.K = (int32_t)a.i("K", 2);
    cfg.nan_policy = (int32_t)a.i("nan_policy", LLAMPC_NAN_FIRST);
    cfg.Ts = a.d("Ts", 0.02), cfg.v_factor = 0.9, cfg.mu_init = 0.8, cfg.S = 20, cfg.lap_projidx = 7;
    cfg.sigma[0] = 0.1, cfg.sigma[1] = 0.05, cfg.seed = 77;
    for (int i = 0; i < 6; ++i) cfg.nominal[i] = 1.5 + i;
    for (int i = 0; i < 4; ++i) cfg.cost.Q[i] = (i == 0 || i == 3) ? 1 + i : 0, cfg.cost.R[i] = 10 + i, cfg.cost.P[i] = (i == 0 || i == 3) ? 20 + i : 0;
    cfg.cost.Q[1] = a.d("q1", 0.0);
    cfg.cost.umin[0] = -0.1, cfg.cost.umin[1] = -0.35, cfg.cost.umax[0] = 1.0, cfg.cost.umax[1] = 0.35;
    cfg.cost.rate_max[0] = -1.0, cfg.cost.rate_max[1] = 2.0;
    cfg.cost.enforce_bounds = 1;
    const auto mus = ramp(2, 0.5);       // exactly rl_M entries: 0.5, 1.5
    const auto x_t = ramp(6, 0.25);
    CtlView v = fake_ctl_view(&cfg, mus.get(), a);
    FakeCtl c{a.i("t", 0), a.u("hseq", 40), (uint32_t)a.u("seq", 7), (uint32_t)a.u("door_ctr", 3), (int32_t)a.i("hint_p0", 5),
              a.d("hint_mu", 0.75), a.i("cor_prev") != 0, 0, (uint32_t)a.u("px_seq", 5)};
    FakeBankState bank{(int32_t)a.i("count", 0), (int32_t)a.i("slot", 0), v.bank.W, 0, 0, 0, TrackPathState{0}, 0};
    FakeBox box{(uint32_t)a.u("px_seq", 5)};
    FakeBox* mb = v.mailbox ? &box : nullptr;
    const std::string kinds = a.find("kinds") ? a.find("kinds") : "l";
    const long long reset = a.i("reset", -1);
    for (int s = 0; s < (int)kinds.size(); ++s) {
      if (s == reset) bank.count = bank.slot = 0;
      v.bank.slot = bank.slot;           // bank_view's
      const bool armed = kinds[s] != 'l';
      CtlPrep P;
      char why[256] = "";
      const int rc = ctl_tick_prepare(v, ctl_tick_state(c, bank, mb), armed ? nullptr : x_t.get(), P, why, sizeof why);
      if (armed) c.door_ctr = P.next.door_ctr;
      pi(s, "rc", rc);
      if (rc) {
        std::printf("t%d.why %s\n", s, why);
      } else {
        print_ctl_prep(s, P);
        if (kinds[s] != 'f') ctl_tick_commit(c, bank, mb, P.next);
      }
      pi(s, "ctl.t", c.t), pi(s, "ctl.hseq", (long long)c.hseq), pi(s, "ctl.seq", c.seq), pi(s, "ctl.door_ctr", c.door_ctr);
      pi(s, "ctl.cor_prev", c.cor_prev), pi(s, "ctl.cor_nslots", c.cor_nslots), pi(s, "ctl.xg_seq", c.xg_seq);
      pi(s, "bank.count", bank.count), pi(s, "bank.slot", bank.slot), pi(s, "box.seq", box.seq);
    }
    return 0;
  }
  if (mode == "ctl_spec") {
    // ctl_spec field=value ...: ctl_spec_models of the named CtlSpecIn fields: `n_spec lds poll_off`
    // (lds and poll_off as they were given, -1, when none).
    const Fields a{argc, argv, 2};
    CtlSpecIn s{};
    s.armed = a.i("armed", 1) != 0, s.no_spec = a.i("no_spec") != 0, s.warm = a.i("warm") != 0, s.full = a.i("full", 1) != 0;
    s.diag = a.i("diag", 1) != 0, s.mailbox = a.i("mailbox") != 0;
    s.R = (int32_t)a.i("R", 1), s.s4 = (int32_t)a.i("s4", 1), s.lpm = (int32_t)a.i("lpm", 4), s.cpl = (int32_t)a.i("cpl", 1);
    s.G = (int32_t)a.i("G", 2), s.C = (int32_t)a.i("C", 2), s.H = (int32_t)a.i("H", 3), s.K = (int32_t)a.i("K", 2);
    s.rl_n = (int32_t)a.i("rl_n", 5), s.xg_world = (int32_t)a.i("xg_world"), s.px_G = (int32_t)a.i("px_G");
    s.nb_lb = (int32_t)a.i("nb_lb", 1), s.nb_la = (int32_t)a.i("nb_la", 3), s.spec_nb = (int32_t)a.i("spec_nb", 1);
    s.spec_cap = (int32_t)a.i("spec_cap", 32), s.cus = (int32_t)a.i("cus", 256), s.share = (int32_t)a.i("share", 1);
    s.n = a.i("n", 5);
    size_t lds = (size_t)-1, poll_off = (size_t)-1;
    const int32_t ns = ctl_spec_models(s, &lds, &poll_off);
    std::printf("%d %lld %lld\n", ns, (long long)lds, (long long)poll_off);
    return 0;
  }
  if (mode == "ctl_cor_layout") {
    constexpr CtlCorLayout L = ctl_cor_layout();
    std::printf("row %zu\npath_doubles %zu\nrb_doubles %zu\nrb_hp %zu\nrb_theta %zu\ncor_doubles %zu\nflags %d\nhp_tag_words %zu\n"
                "path0 %zu\npath1 %zu\nrb0 %zu\nrb1 %zu\nvalid0 %d\nvalid1 %d\nrb_valid0 %d\nrb_valid1 %d\n"
                "kCtlPathStride %d\nkCtlCorDbgDoubles %d\nHMAX %d\n",
                L.row, L.path_doubles, L.rb_doubles, L.rb_hp, L.rb_theta, L.cor_doubles, L.flags, L.hp_tag_words, L.path(0),
                L.path(1), L.rb(0), L.rb(1), L.valid(0), L.valid(1), L.rb_valid(0), L.rb_valid(1), kCtlPathStride,
                kCtlCorDbgDoubles, LLAMPC_HMAX);
    return 0;
  }
  if (mode == "ctl_door") {
    // ctl_door door_seq x0 .. x5 (each a double's 64 bits, hex): the kCtlDoorWords words, the cancel word,
    // then kCtlDoorFire kCtlDoorCancel kArmFreshS kArmBoundS
    std::unique_ptr<double[]> x(new double[6]);
    for (int j = 0; j < 6; ++j) {
      const uint64_t b = uarg(3 + j);
      std::memcpy(&x[j], &b, 8);
    }
    std::unique_ptr<uint64_t[]> w(new uint64_t[kCtlDoorWords]);
    ctl_door_words(x.get(), (uint32_t)uarg(2), w.get());
    for (int j = 0; j < kCtlDoorWords; ++j) std::printf("%" PRIx64 "\n", w[j]);
    std::printf("%" PRIx64 "\n%u %u %.17g %.17g\n", ctl_door_cancel_word((uint32_t)uarg(2)), kCtlDoorFire, kCtlDoorCancel,
                kArmFreshS, kArmBoundS);
    return 0;
  }
  if (mode == "ctl_fires") {             // ctl_fires age arm_t t arm_px_G has_mailbox arm_px_seq mailbox_seq
    std::printf("%d\n", (int)ctl_arm_fires(std::strtod(argv[2], nullptr), arg(3), arg(4), (int32_t)arg(5), arg(6) != 0,
                                           (uint32_t)uarg(7), (uint32_t)uarg(8)));
    return 0;
  }
  if (mode == "ctl_refuse") {
    // ctl_refuse entry field=value ...: `code message` of ctl_create_refused (entry create: out_null arg_null
    // null_cfg C H K S Ts np nan_policy n raceline rl_n), ctl_corridor_refused (corridor: pending tr_n sharded
    // weight margin tr_width n C H K rl_n no_stage) or ctl_variant_refused (variant: out_null n C H K rl_n
    // and, a corridor tick's, track_n).
    const std::string entry = argc > 2 ? argv[2] : "";
    const Fields a{argc, argv, 3};
    char why[256] = "";
    int rc = 0;
    if (entry == "create") {
      llampc_ctl_cfg cfg{};
      cfg.C = (int32_t)a.i("C", 2), cfg.H = (int32_t)a.i("H", 3), cfg.K = (int32_t)a.i("K", 2), cfg.S = (int32_t)a.i("S", 20);
      cfg.Ts = a.d("Ts", 0.02), cfg.nan_policy = (int32_t)a.i("nan_policy", LLAMPC_NAN_FIRST);
      rc = ctl_create_refused(a.i("out_null") != 0, a.i("arg_null") != 0, a.i("null_cfg") ? nullptr : &cfg, (int32_t)a.i("np", 9),
                              a.i("n", 5), a.i("raceline", 1) != 0, (int32_t)a.i("rl_n", 5), why, sizeof why);
    } else if (entry == "corridor") {
      const CtlCorridorFacts f{a.i("pending") != 0, a.i("sharded") != 0, a.i("no_stage") != 0, (int32_t)a.i("tr_n", 4),
                               a.d("tr_width", 2.4), a.i("n", 5), (int32_t)a.i("C", 2), (int32_t)a.i("H", 3), (int32_t)a.i("K", 2),
                               (int32_t)a.i("rl_n", 5)};
      rc = ctl_corridor_refused(f, a.d("weight", 1e4), a.d("margin", 0.05), why, sizeof why);
    } else if (entry == "variant") {
      const int32_t track_n = (int32_t)a.i("track_n", 0);
      CtlShape V{};
      rc = ctl_variant_refused(a.i("out_null") != 0, a.i("n", 5), (int32_t)a.i("C", 2), (int32_t)a.i("H", 3), (int32_t)a.i("K", 2),
                               (int32_t)a.i("rl_n", 5), a.find("track_n") ? &track_n : nullptr, a.i("no_stage") != 0, V, why,
                               sizeof why);
      if (!rc) std::snprintf(why, sizeof why, "lpm=%d nb_cor=%d", V.lpm, V.nb_cor);
    } else {
      return 2;
    }
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

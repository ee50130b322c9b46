// capi_plan.hip — extern "C" boundary (include/llampc.h): the plan tick on a bank.  plan_launch (one
// launch from a prepared tick: capi_host.hpp plan_tick_prepare / plan_tick_commit), the host-pointer
// tick, every llampc_plan* / llampc_lookback / llampc_lookahead* entry, the track tick's entries and
// the llampc_plan_variant* questions.
#include "capi_common.hpp"

using namespace llampc;

// The tick on device pointers (capi_common.hpp).
int plan_launch(llampc_bank* b, const llampc_plan_in& in, const PlanTick& t) {
  if (in.do_lookahead && in.xref_mode == LLAMPC_XREF_RACELINE)   // per-model references [n][H][2]
    if (int rc = b->d_xref_pm.reserve((size_t)b->n * 2 * in.H)) return rc;
  const PlanView v = plan_view(*b, t.px);
  const PlanPrep p = plan_tick_prepare(v, plan_tick_state(*b, t.px), in, t);
  {
    TimedLaunch tl(b, 0, t.stream);
    HIP_TRY(launch_plan(p.lb ? &p.lbl : nullptr, p.la ? &p.lal : nullptr, p.f, t.stream, t.pk, b->share, t.cor,
                        p.tt ? &p.trk : nullptr));
  }
  plan_tick_commit(*b, t.px, p.next);    // only now: a failed launch leaves the bank where it was
  b->launches++;
  return LLAMPC_OK;
}

namespace {

PlanBankFacts bank_facts(const llampc_bank* b) {
  return {b->n, static_cast<bool>(b->d_rl), b->track.n, b->track.width, b->async_pending};
}

// plan_entry_refused of the bank (the caller holds b->mu), reported through fail().
int refuse_entry(const llampc_bank* b, const llampc_plan_in* in, const double* hp, double weight, const TrackTick* tt) {
  char why[256];
  const int rc = plan_entry_refused(bank_facts(b), in, hp, weight, tt, why, sizeof why);
  return rc ? fail(rc, "%s", why) : LLAMPC_OK;
}

int refuse_async_pending(const llampc_bank* b) {
  // an outstanding async tick shares the tickets, tags, ring slot and window count
  return b->async_pending ? fail(LLAMPC_E_STATE, "an async tick is outstanding: call llampc_plan_wait") : LLAMPC_OK;
}

// Host ticks whose inputs travel as kernel arguments (InlinePack): no H2D copy — every tick whose
// launch plan_shape accepts with the pack.  LLAMPC_NO_INLINE=1 keeps the copy (A/B runs).
bool inline_inputs(const llampc_plan_in* in) {
  return !lookahead_shape(1, in->do_lookahead != 0, in->C, in->H, in->integrator, in->xref_mode, 1, true, false).refuse &&
         getenv("LLAMPC_NO_INLINE") == nullptr;
}

// Pack a host plan input into the pinned buffer; return a device-pointer copy of `in`.  hp (the
// corridor tick): the half-planes [H][6] ride behind the pack in the same copy, *d_hp their device
// address.
int stage_inputs(llampc_bank* b, const llampc_plan_in* in, llampc_plan_in* dev_in, hipStream_t s, const double* hp,
                 const double** d_hp) {
  const size_t len = pack_len(in);
  const int64_t H = in->do_lookahead ? in->H : 0;
  const size_t total = len + (hp ? 6 * (size_t)H : 0);
  int rc;
  if ((rc = b->h_in.reserve(total, 1024, "input pack", LLAMPC_E_HIP)) || (rc = b->d_in.reserve(total, 1024))) return rc;
  pack_into(in, b->h_in.get());
  double* d = b->d_in.get();
  if (hp) {
    std::memcpy(b->h_in.get() + len, hp, 6 * (size_t)H * sizeof(double));
    *d_hp = d + len;
  }
  HIP_TRY(hipMemcpyAsync(d, b->h_in.get(), total * sizeof(double), hipMemcpyHostToDevice, s));
  *dev_in = *in;
  dev_in->x_prev = d;
  dev_in->u_prev = d + 6;
  dev_in->x_now = d + 8;
  dev_in->uprev = d + 14;
  dev_in->xref = d + 16;
  dev_in->U = d + 16 + 2 * (H + 1);
  return LLAMPC_OK;
}

// Host completion is the default for host-pointer ticks that return only the record;
// LLAMPC_SYNC_COMPLETION=1 selects the D2H copy + hipStreamSynchronize path (A/B runs).
bool host_completion() { return getenv("LLAMPC_SYNC_COMPLETION") == nullptr; }

// The host-pointer tick, enqueued on the bank's stream (the caller holds b->mu; the bank's device is
// current).  hp: the corridor tick; tt: the track tick.  Either
//   the host-completion launch (the record alone is asked for): the inputs inline or — the corridor
//   rides with them, the track launch takes device inputs — staged, the record into pinned host
//   memory, then the tick's number into the tag: *wait is that number (wait_host_tag); or
//   the copy path: the inputs staged, the record to d_out and its D2H copy, the copies of whichever
//   of err / wmean / cost are asked for: *wait is 0 (the stream's end is the tick's).
int host_tick(llampc_bank* b, const llampc_plan_in* in, const double* hp, double weight, const TrackTick* tt,
              double* err_out, double* wmean_out, double* cost_out, uint64_t* wait) {
  hipStream_t s = b->stream;
  llampc_plan_in din = *in;
  InlinePack pk;
  PlanCorridor cor{nullptr, weight};
  PlanTick t;
  t.stream = s;
  t.tt = tt;
  if (hp) t.cor = &cor;
  int rc;
  *wait = 0;
  if (!err_out && !wmean_out && !cost_out && host_completion()) {
    if (!hp && !tt && inline_inputs(in)) {
      pack_into(in, pk.v);
      t.pk = &pk;
    } else if ((rc = stage_inputs(b, in, &din, s, hp, &cor.hp))) {
      return rc;
    }
    t.out = b->host.rec.dev();
    t.host_tag = b->host.tag.dev();
    t.host_seq = *wait = ++b->hseq;
    return plan_launch(b, din, t);
  }
  if (cost_out && in->do_lookahead) {
    if ((rc = b->d_cost.reserve((size_t)b->n * in->C))) return rc;
    t.cost = b->d_cost.get();
  }
  if ((rc = stage_inputs(b, in, &din, s, hp, &cor.hp))) return rc;
  t.out = b->d_out.get();
  if (err_out) t.err = b->d_err.get();
  if (wmean_out) t.wmean = b->d_wmean.get();
  if ((rc = plan_launch(b, din, t))) return rc;
  HIP_TRY(hipMemcpyAsync(b->h_out.get(), b->d_out.get(), sizeof(llampc_plan_out), hipMemcpyDeviceToHost, s));
  if (err_out && in->do_lookback)
    HIP_TRY(hipMemcpyAsync(err_out, b->d_err.get(), b->n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (wmean_out && in->do_lookback && b->count >= b->W)
    HIP_TRY(hipMemcpyAsync(wmean_out, b->d_wmean.get(), b->n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (t.cost)
    HIP_TRY(hipMemcpyAsync(cost_out, t.cost, (size_t)b->n * in->C * sizeof(double), hipMemcpyDeviceToHost, s));
  return LLAMPC_OK;
}

// After a tick whose record reports a device-side status (an in-launch wait gave up) or whose
// completion never arrived: once the stream has drained, every in-launch counter is zeroed —
// the work-queue counter (straggler blocks may have taken units after final_write reset it)
// and the tickets — so the next launch starts from a clean hand-off state.
int recover_counters(llampc_bank* b) {
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemsetAsync(b->d_wq.get(), 0, sizeof(uint64_t), b->stream));
  HIP_TRY(hipMemsetAsync(b->d_tickets.get(), 0, 2 * sizeof(unsigned), b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return LLAMPC_OK;
}

// Spin until the plan kernel has published tick `seq` in the tag, then copy the record out.
// A tag that never arrives (a device fault) ends the spin after 10 s: the stream is then
// synchronised so the HIP error, if any, is the one reported.
int wait_host_tag(llampc_bank* b, uint64_t seq, llampc_plan_out* out) {
  const int rc = spin_for_tag(b->host.tag.get(), seq, [&]() -> int {
    HIP_TRY(hipStreamSynchronize(b->stream));
    return LLAMPC_OK;
  });
  if (rc == kSpinTimeout) {
    (void)recover_counters(b);
    return fail(LLAMPC_E_DEVICE, "tick %llu: completion tag never arrived", (unsigned long long)seq);
  }
  if (rc) return rc;
  std::memcpy(out, const_cast<const llampc_plan_out*>(b->host.rec.get()), sizeof(llampc_plan_out));
  return LLAMPC_OK;
}

// The record of the host_tick that returned `wait`, once it is there; a device-side status in it is
// LLAMPC_E_DEVICE.
int host_tick_result(llampc_bank* b, uint64_t wait, llampc_plan_out* out) {
  if (wait) {
    if (int rc = wait_host_tag(b, wait, out)) return rc;
  } else {
    HIP_TRY(hipStreamSynchronize(b->stream));
    *out = *b->h_out.get();
  }
  if (out->status) {
    (void)recover_counters(b);
    return fail(LLAMPC_E_DEVICE, "tick record status %d (in-launch completion timed out)", out->status);
  }
  return LLAMPC_OK;
}

// llampc_plan (hp null), llampc_plan_corridor and (tt) llampc_plan_track: the blocking host-pointer tick.
// The refusals are decided under the lock the launch is made under: the track, the raceline and the
// outstanding async tick they depend on cannot change in between.
int plan_blocking(llampc_bank* b, const llampc_plan_in* in, const double* hp, double weight, llampc_plan_out* out,
                  double* err_out, double* wmean_out, double* cost_out, const TrackTick* tt = nullptr) {
  if (!b || !out) return fail(LLAMPC_E_ARG, "bank/out is NULL");
  std::lock_guard<std::mutex> lk(b->mu);
  int rc;
  if ((rc = refuse_entry(b, in, hp, weight, tt))) return rc;
  bank_disarm(b);
  if ((rc = refuse_async_pending(b))) return rc;
  DeviceGuard g(b->device);
  uint64_t wait;
  if ((rc = host_tick(b, in, hp, weight, tt, err_out, wmean_out, cost_out, &wait))) return rc;
  return host_tick_result(b, wait, out);
}

// llampc_plan_async (tt null) and llampc_plan_track_async.
int plan_async(llampc_bank* b, const llampc_plan_in* in, const TrackTick* tt) {
  if (!b) return fail(LLAMPC_E_ARG, "bank is NULL");
  std::lock_guard<std::mutex> lk(b->mu);
  int rc;
  if ((rc = refuse_entry(b, in, nullptr, 0.0, tt))) return rc;
  bank_disarm(b);
  if ((rc = refuse_async_pending(b))) return rc;
  DeviceGuard g(b->device);
  uint64_t wait;
  if ((rc = host_tick(b, in, nullptr, 0.0, tt, nullptr, nullptr, nullptr, &wait))) return rc;
  b->async_seq = wait;
  b->async_pending = true;
  return LLAMPC_OK;
}

// llampc_lookahead (hp null) and llampc_lookahead_corridor.
int lookahead_blocking(llampc_bank* b, const double* x0, const double* U, int32_t C, int32_t H, const double* xref,
                       const double* uprev, const llampc_cost* cost, double Ts, int32_t integrator, const double* hp,
                       double weight, double* cost_out, int32_t* best_cand_out, int64_t* best_model, int32_t* best_cand,
                       double* best_cost) {
  if (!cost) return fail(LLAMPC_E_ARG, "cost is NULL");
  llampc_plan_in in{};
  in.x_now = x0;
  in.U = U;
  in.C = C;
  in.H = H;
  in.xref = xref;
  in.uprev = uprev;
  in.K = 1;
  in.integrator = integrator;
  in.do_lookback = 0;
  in.do_lookahead = 1;
  in.current_model = -1;
  in.Ts = Ts;
  in.cost = *cost;
  llampc_plan_out o;
  int rc = plan_blocking(b, &in, hp, weight, &o, nullptr, nullptr, cost_out);
  if (rc) return rc;
  if (best_cand_out) {
    DeviceGuard g(b->device);
    HIP_TRY(hipMemcpy(best_cand_out, b->d_best_cand.get(), b->n * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  if (best_model) *best_model = o.la_best_model;
  if (best_cand) *best_cand = o.la_best_cand;
  if (best_cost) *best_cost = o.la_best_cost;
  return LLAMPC_OK;
}

// The track tick's device state (capi_host.hpp plan_track_layout), allocated with the first track or
// path (the caller holds b->mu, the bank's device is current).
int track_state(llampc_bank* b) {
  if (b->d_trk) return LLAMPC_OK;
  constexpr PlanTrackLayout L = plan_track_layout();
  int rc;
  if ((rc = b->d_trk.zalloc(L.trk_doubles, "track tick path state")) ||
      (rc = b->d_trk_flags.zalloc(L.flags, "track tick flags")) ||
      (rc = b->d_hp_tag.zalloc(L.hp_tag_words, "track tick half-plane words")))
    return rc;
  return LLAMPC_OK;
}

// The variant a given-xref look-ahead of these sizes takes, without or with a corridor: the
// launch's own plan_shape.
void plan_variant(int64_t n, int32_t C, int32_t H, int32_t integrator, int32_t share, bool corridor, int32_t out[4]) {
  const PlanShape s = lookahead_shape(n, true, C, H, integrator, LLAMPC_XREF_GIVEN, share, false, corridor);
  out[0] = s.lpm;
  out[1] = s.G;
  out[2] = s.cpl;
  out[3] = s.stage ? 1 : 0;
}

}  // namespace

int check_plan_in(const llampc_bank* b, const llampc_plan_in* in) {
  char why[256];
  const int rc = plan_in_refused(bank_facts(b), in, why, sizeof why);
  return rc ? fail(rc, "%s", why) : LLAMPC_OK;
}

extern "C" {

int llampc_plan(llampc_bank* b, const llampc_plan_in* in, llampc_plan_out* out, double* err_out,
                double* wmean_out, double* cost_out) {
  return plan_blocking(b, in, nullptr, 0.0, out, err_out, wmean_out, cost_out);
}

int llampc_plan_corridor(llampc_bank* b, const llampc_plan_in* in, const double* hp, double weight,
                         llampc_plan_out* out, double* err_out, double* wmean_out, double* cost_out) {
  if (!hp) return fail(LLAMPC_E_ARG, "hp is NULL (llampc_plan is the tick without a corridor)");
  return plan_blocking(b, in, hp, weight, out, err_out, wmean_out, cost_out);
}

int llampc_plan_track(llampc_bank* b, const llampc_plan_in* in, double weight, double margin, llampc_plan_out* out,
                      double* err_out, double* wmean_out, double* cost_out) {
  const TrackTick tt{weight, margin};
  return plan_blocking(b, in, nullptr, 0.0, out, err_out, wmean_out, cost_out, &tt);
}

int llampc_plan_async(llampc_bank* b, const llampc_plan_in* in) { return plan_async(b, in, nullptr); }

int llampc_plan_track_async(llampc_bank* b, const llampc_plan_in* in, double weight, double margin) {
  const TrackTick tt{weight, margin};
  return plan_async(b, in, &tt);
}

int llampc_plan_wait(llampc_bank* b, llampc_plan_out* out) {
  if (!b || !out) return fail(LLAMPC_E_ARG, "bank/out is NULL");
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->async_pending) return fail(LLAMPC_E_STATE, "no async tick outstanding");
  DeviceGuard g(b->device);
  b->async_pending = false;
  return host_tick_result(b, b->async_seq, out);
}

int llampc_plan_device(llampc_bank* b, const llampc_plan_in* in, void* d_out, double* d_err,
                       double* d_wmean, double* d_cost, void* stream) {
  if (!b || !d_out) return fail(LLAMPC_E_ARG, "bank/d_out is NULL");
  std::lock_guard<std::mutex> lk(b->mu);
  int rc;
  if ((rc = check_plan_in(b, in))) return rc;
  bank_disarm(b);
  if ((rc = refuse_async_pending(b))) return rc;
  DeviceGuard g(b->device);
  PlanTick t;
  t.out = (llampc_plan_out*)d_out;
  t.err = d_err;
  t.wmean = d_wmean;
  t.cost = d_cost;
  t.stream = pick_stream(b, stream);
  return plan_launch(b, *in, t);
}

int llampc_lookback(llampc_bank* b, const double* x_prev, const double* u_prev, const double* x_now,
                    double Ts, int32_t K, int32_t nan_policy, double* err_out, double* wmean_out,
                    int64_t* best, int64_t* topk, double* topk_val, int32_t* window_count) {
  llampc_plan_in in{};
  in.x_prev = x_prev;
  in.u_prev = u_prev;
  in.x_now = x_now;
  in.K = K;
  in.do_lookback = 1;
  in.do_lookahead = 0;
  in.nan_policy = nan_policy;
  in.current_model = -1;
  in.Ts = Ts;
  llampc_plan_out o;
  int rc = llampc_plan(b, &in, &o, err_out, wmean_out, nullptr);
  if (rc) return rc;
  if (best) *best = o.window_full ? o.lb_best : -1;
  for (int k = 0; k < K; ++k) {
    if (topk) topk[k] = o.topk[k];
    if (topk_val) topk_val[k] = o.topk_val[k];
  }
  if (window_count) *window_count = o.window_count;
  return LLAMPC_OK;
}

int llampc_lookahead(llampc_bank* b, const double* x0, const double* U, int32_t C, int32_t H,
                     const double* xref, const double* uprev, const llampc_cost* cost, double Ts,
                     int32_t integrator, double* cost_out, int32_t* best_cand_out,
                     int64_t* best_model, int32_t* best_cand, double* best_cost) {
  return lookahead_blocking(b, x0, U, C, H, xref, uprev, cost, Ts, integrator, nullptr, 0.0, cost_out, best_cand_out,
                            best_model, best_cand, best_cost);
}

int llampc_lookahead_corridor(llampc_bank* b, const double* x0, const double* U, int32_t C, int32_t H,
                              const double* xref, const double* uprev, const llampc_cost* cost, double Ts,
                              int32_t integrator, double* cost_out, int32_t* best_cand_out,
                              int64_t* best_model, int32_t* best_cand, double* best_cost, const double* hp,
                              double weight) {
  if (!hp) return fail(LLAMPC_E_ARG, "hp is NULL (llampc_lookahead is the look-ahead without a corridor)");
  return lookahead_blocking(b, x0, U, C, H, xref, uprev, cost, Ts, integrator, hp, weight, cost_out, best_cand_out,
                            best_model, best_cand, best_cost);
}

int llampc_bank_set_track(llampc_bank* b, const double* centre, const double* theta, int32_t n, double track_length,
                          double track_width) {
  if (!b || !centre || !theta) return fail(LLAMPC_E_ARG, "NULL argument");
  char why[128];
  if (track_tables_invalid(centre, theta, n, track_length, track_width, why, sizeof why)) return fail(LLAMPC_E_ARG, "%s", why);
  BankIdle idle(b);
  if (idle.rc) return idle.rc;
  b->trk_path = track_path_next(b->trk_path, kPathClear);
  b->trk_last_H = 0;
  if (int rc = track_state(b)) return rc;
  return b->track.upload(b->stream, centre, theta, n, track_length, track_width);
}

int llampc_bank_set_path(llampc_bank* b, const double* path, int32_t H) {
  if (!b) return fail(LLAMPC_E_ARG, "bank is NULL");
  if (path) {
    if (H < 1 || H > LLAMPC_HMAX) return fail(LLAMPC_E_ARG, "H=%d outside [1, %d]", H, LLAMPC_HMAX);
    char why[64];
    if (path_invalid(path, H, why, sizeof why)) return fail(LLAMPC_E_ARG, "%s", why);
  }
  BankIdle idle(b);
  if (idle.rc) return idle.rc;
  if (!path) {
    b->trk_path = track_path_next(b->trk_path, kPathClear);
    return LLAMPC_OK;
  }
  HIP_TRY(hipStreamSynchronize(b->stream));      // no launch reads or writes the copy being seeded
  if (int rc = track_state(b)) return rc;
  constexpr PlanTrackLayout L = plan_track_layout();
  std::vector<double> h(L.path_doubles, 0.0);
  for (int r = 0; r < 2; ++r) std::memcpy(h.data() + r * L.row, path + (size_t)r * (H + 1), (H + 1) * sizeof(double));
  const int32_t one = 1;
  HIP_TRY(hipMemcpy(b->d_trk.get() + L.path(b->trk_cur), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_trk_flags.get() + L.valid(b->trk_cur), &one, sizeof one, hipMemcpyHostToDevice));
  b->trk_path = track_path_next(b->trk_path, kPathSeed, H);
  return LLAMPC_OK;
}

int llampc_bank_track_corridor(llampc_bank* b, double* path, double* hp, double* theta, int32_t* valid,
                               double* next_path, int32_t* next_valid, double* next_cost) {
  if (!b || !path || !hp || !theta || !valid || !next_path || !next_valid || !next_cost)
    return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->trk_last_H) return fail(LLAMPC_E_STATE, "the bank's last launch was not a track tick");
  DeviceGuard g(b->device);
  HIP_TRY(hipStreamSynchronize(b->stream));      // the launch's end: the path update follows the record
  const int H = b->trk_last_H;
  constexpr PlanTrackLayout L = plan_track_layout();
  std::vector<double> h(L.trk_doubles);
  int32_t fl[L.flags];
  HIP_TRY(hipMemcpy(h.data(), b->d_trk.get(), h.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(fl, b->d_trk_flags.get(), sizeof fl, hipMemcpyDeviceToHost));
  const int cur = b->trk_cur;            // the copy the tick wrote
  for (int r = 0; r < 2; ++r) {
    std::memcpy(path + (size_t)r * (H + 1), h.data() + L.rb_path + r * L.row, (H + 1) * sizeof(double));
    std::memcpy(next_path + (size_t)r * (H + 1), h.data() + L.path(cur) + r * L.row, (H + 1) * sizeof(double));
  }
  std::memcpy(hp, h.data() + L.rb_hp, 6 * (size_t)H * sizeof(double));
  std::memcpy(theta, h.data() + L.rb_theta, (size_t)H * sizeof(double));
  *valid = fl[L.flag_rb_valid];
  *next_valid = fl[L.valid(cur)];
  *next_cost = h[L.cost(cur)];
  return LLAMPC_OK;
}

int llampc_plan_variant(int64_t n, int32_t C, int32_t H, int32_t integrator, int32_t share, int32_t out[4]) {
  if (!out) return fail(LLAMPC_E_ARG, "NULL argument");
  if (n < 1 || C < 1 || H < 1 || integrator < LLAMPC_RK4 || integrator > LLAMPC_RK6)
    return fail(LLAMPC_E_ARG, "n %lld, C %d, H %d, integrator %d", (long long)n, C, H, integrator);
  plan_variant(n, C, H, integrator, share, false, out);
  return LLAMPC_OK;
}

int llampc_plan_variant_corridor(int64_t n, int32_t C, int32_t H, int32_t integrator, int32_t share, int32_t out[4]) {
  if (!out) return fail(LLAMPC_E_ARG, "NULL argument");
  if (n < 1 || C < 1 || H < 1 || (integrator != LLAMPC_RK4 && integrator != LLAMPC_EULER_NLP))
    return fail(LLAMPC_E_ARG, "n %lld, C %d, H %d, integrator %d (the corridor look-ahead: RK4 or NLP-Euler)",
                (long long)n, C, H, integrator);
  plan_variant(n, C, H, integrator, share, true, out);
  return LLAMPC_OK;
}

int llampc_plan_variant_track(int64_t n, int32_t C, int32_t H, int32_t share, int32_t track_n, int32_t out[5]) {
  if (!out) return fail(LLAMPC_E_ARG, "NULL argument");
  if (n < 1 || C < 1 || H < 1 || H > LLAMPC_HMAX || track_n < 2 || track_n > kTrackMaxPoints)
    return fail(LLAMPC_E_ARG, "n %lld, C %d, H %d (<= %d), track_n %d (2..%d)", (long long)n, C, H, LLAMPC_HMAX, track_n,
                kTrackMaxPoints);
  const PlanShape s = lookahead_shape(n, true, C, H, LLAMPC_RK4, LLAMPC_XREF_GIVEN, share, false, false, track_n);
  out[0] = s.lpm;
  out[1] = s.G;
  out[2] = s.cpl;
  out[3] = s.stage ? 1 : 0;
  out[4] = s.nb_cor;
  return LLAMPC_OK;
}

}  // extern "C"

// capi.hip — extern "C" boundary (include/llampc.h): the device-resident model-bank
// handle, host<->device staging and the per-tick launch sequence.
//
// A bank owns, on its device: params SoA [6][n] (48 B/model, read coalesced by lane),
// the look-back ring [W][n] (slot-major, so each tick writes one contiguous row — the
// reference's np.roll copy of N*W doubles per tick, rt.py:352, is gone), per-block
// reduction partials, the per-model look-ahead result, and pinned host staging so one
// host-pointer tick = 1 H2D copy + 1 kernel on one stream, the record coming back through
// pinned host memory with a completion tag (llampc_plan / llampc_plan_wait).
#include <cstdarg>
#include <cstdio>

#include "capi_common.hpp"
#include "merge.hpp"

using namespace llampc;

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int check_plan_in(const llampc_bank* b, const llampc_plan_in* in) {
  if (!in) return fail(LLAMPC_E_ARG, "plan input is NULL");
  if (in->do_lookback && (in->K < 1 || in->K > LLAMPC_KMAX))
    return fail(LLAMPC_E_ARG, "K=%d outside [1, %d]", in->K, LLAMPC_KMAX);
  if (in->do_lookback && (!in->x_prev || !in->u_prev || !in->x_now))
    return fail(LLAMPC_E_ARG, "look-back needs x_prev, u_prev and x_now");
  if (in->do_lookahead) {
    if (in->C < 1 || in->H < 1) return fail(LLAMPC_E_ARG, "C=%d H=%d must be >= 1", in->C, in->H);
    if ((int64_t)in->C * in->H > (1 << 26)) return fail(LLAMPC_E_ARG, "C*H too large");
    if (!in->x_now || !in->U || !in->xref || !in->uprev)
      return fail(LLAMPC_E_ARG, "look-ahead needs x_now, U, xref and uprev");
    if (in->integrator < LLAMPC_RK4 || in->integrator > LLAMPC_RK6)
      return fail(LLAMPC_E_ARG, "unknown integrator %d", in->integrator);
    if (in->xref_mode != LLAMPC_XREF_GIVEN && in->xref_mode != LLAMPC_XREF_RACELINE)
      return fail(LLAMPC_E_ARG, "unknown xref_mode %d", in->xref_mode);
    if (in->xref_mode == LLAMPC_XREF_RACELINE && !b->d_rl)
      return fail(LLAMPC_E_STATE, "xref_mode RACELINE needs llampc_bank_set_raceline first");
    if ((b->n + 1) * (int64_t)in->C <= 0 || b->n > INT64_MAX / std::max(1, in->C) - 1)
      return fail(LLAMPC_E_ARG, "n*C overflows");
  }
  if (!in->do_lookback && !in->do_lookahead) return fail(LLAMPC_E_ARG, "nothing to do: look-back and look-ahead both off");
  if (!(in->Ts > 0) || !std::isfinite(in->Ts)) return fail(LLAMPC_E_ARG, "Ts must be finite > 0");
  return LLAMPC_OK;
}

static void timing_free(llampc_bank* b) {
  for (auto& v : b->ev) {
    for (hipEvent_t e : v) (void)hipEventDestroy(e);
    v.clear();
  }
  for (size_t& u : b->ev_used) u = 0;
  for (int64_t& u : b->timing_seen) u = 0;
  b->timing = false;
  b->timing_stride = 1;
  b->timing_sample = false;
}

// The tick on device pointers (capi_common.hpp).  Advances the window bookkeeping when a look-back runs.
int plan_launch(llampc_bank* b, const llampc_plan_in& in, llampc_plan_out* d_out, double* d_err, double* d_wmean,
                double* d_cost, hipStream_t s, uint64_t* host_tag, uint64_t host_seq, const InlinePack* pk,
                llampc_mailbox* px, llampc_plan_out* px_merged, const PlanCorridor* cor, const TrackTick* tt) {
  const bool lb = in.do_lookback != 0;
  const bool la = in.do_lookahead != 0;
  const bool raceline = la && in.xref_mode == LLAMPC_XREF_RACELINE;
  if (raceline)                          // per-model references [n][H][2]
    if (int rc = b->d_xref_pm.reserve((size_t)b->n * 2 * in.H)) return rc;
  const BankView bv = bank_view(*b);
  int32_t count = b->count;
  int32_t full = count >= b->W;
  LookbackLaunch lbl{};
  if (lb) {
    count = std::min(count + 1, b->W);             // rt.py:354
    full = count >= b->W;                          // rt.py:357
    bank_lookback(bv, lbl);
    lbl.x_prev = in.x_prev;
    lbl.u_prev = in.u_prev;
    lbl.x_now = in.x_now;
    lbl.Ts = in.Ts;
    lbl.full = full;
    lbl.K = in.K;
    lbl.nan_first = in.nan_policy == LLAMPC_NAN_FIRST;
    lbl.err_out = d_err;
    if (d_wmean) lbl.wm_buf = d_wmean;
    lbl.wm_keep = d_wmean != nullptr;              // else only the R > 1 second pass reads it
  }
  // polled completion whenever look-back blocks exist to host the poller (LLAMPC_NO_POLL=1:
  // the ticket + last-block path, for A/B runs)
  const bool no_poll = getenv("LLAMPC_NO_POLL") != nullptr;
  const int32_t poll = (lb && la && !no_poll) ? 1 : 0;
  const uint32_t seq = poll ? next_seq(b->seq) : b->seq;
  LookaheadLaunch lal{};
  if (la) {
    bank_lookahead(bv, in.integrator, lal);
    lal.x0 = in.x_now;
    lal.U = in.U;
    lal.xref = in.xref;
    lal.uprev = in.uprev;
    lal.C = in.C;
    lal.H = in.H;
    lal.Ts = in.Ts;
    lal.cost = make_cost(in.cost, in.Ts);
    lal.cost_out = d_cost;
    lal.best_cand = b->d_best_cand.get();
    lal.best_cost = b->d_best_cost.get();
    lal.pv = b->d_pv.get();
    lal.pidx = b->d_pidx.get();
    lal.pnf = b->d_pnf.get();
    lal.xref_mode = in.xref_mode;
    if (raceline) {
      lal.rl = raceline_view(bv);       // wcap: set by launch_plan from the LDS it leaves
      lal.xref_pm = b->d_xref_pm.get();
    }
    lal.la_tag = b->d_la_tag.get();
    lal.blk_tag = b->d_blk_tag.get();
    lal.seq = seq;
    lal.poll = poll;
    lal.wq = b->d_wq.get();
  }
  FinalLaunch f{};
  bank_final(bv, f);
  f.out = d_out;
  f.tickets = b->d_tickets.get();
  f.full = full;
  f.window_count = count;
  f.K = lb ? in.K : 0;
  f.nan_first = in.nan_policy == LLAMPC_NAN_FIRST;
  f.C = la ? in.C : 1;
  f.current_model = in.current_model;
  f.best_cand = b->d_best_cand.get();
  f.best_cost = b->d_best_cost.get();
  f.pv = b->d_pv.get();
  f.pidx = b->d_pidx.get();
  f.pnf = b->d_pnf.get();
  f.la_tag = b->d_la_tag.get();
  f.blk_tag = b->d_blk_tag.get();
  f.seq = seq;
  f.poll = poll ? (int32_t)poll_units(poll_bound_ticks(b->n, in.C, in.H), INT32_MAX) : 0;
  f.host_tag = host_tag;
  f.host_seq = host_seq;
  const uint32_t px_seq = px ? next_seq(px->seq) : 0;
  if (px) {                             // fused peer exchange (llampc_plan_exchange)
    f.px_box = px->d_box.get();
    f.px_merged = px_merged;
    f.px_G = px->world;
    f.px_rank = px->rank;
    f.px_seq = px_seq;
    f.px_bound = (uint32_t)poll_units(px->bound, UINT32_MAX);
  }
  f.wq = b->d_wq.get();
  // the track tick: the read copy is the one the launch before wrote (or llampc_bank_set_path), the
  // write copy the other; the half-plane words' own sequence
  PlanTrack trk{};
  const uint32_t tseq = tt ? next_seq(b->tseq) : b->tseq;
  if (tt) {
    const size_t tn = (size_t)b->tr_n, ps = 2 * (size_t)kPlanPathStride;
    const double* d = b->d_track.get();
    const int rd = b->trk_cur, wr = rd ^ 1;
    double* st = b->d_trk.get();
    int32_t* fl = b->d_trk_flags.get();
    trk.trk = TrackK{d, d + tn, d + 2 * tn, b->tr_n, 0, b->tr_L};
    trk.hw = b->tr_width / 2 - tt->margin;
    trk.weight = tt->weight;
    trk.hp_tag = b->d_hp_tag.get();
    trk.path_rd = st + ps * rd;
    trk.path_wr = st + ps * wr;
    trk.valid_rd = fl + rd;
    trk.valid_wr = fl + wr;
    trk.cost_wr = st + 2 * ps + wr;
    trk.dbg = st + 2 * ps + 2;
    trk.dbg_valid = fl + 2;
    trk.late = reinterpret_cast<uint32_t*>(fl + 3);
    trk.seq = tseq;
    trk.poll = (uint32_t)poll_units(poll_bound_ticks(b->n, in.C, in.H), INT32_MAX);
    trk.path_ok = track_path_offered(b->trk_path, in.H) ? 1 : 0;
  }
  {
    TimedLaunch tl(b, 0, s);
    HIP_TRY(launch_plan(lb ? &lbl : nullptr, la ? &lal : nullptr, f, s, pk, b->share, cor, tt ? &trk : nullptr));
  }
  b->seq = seq;
  b->tseq = tseq;
  if (tt) b->trk_cur ^= 1;
  b->trk_path = track_path_next(b->trk_path, tt ? kPathTrackTick : kPathOtherLaunch, in.H);
  b->trk_last_H = tt ? in.H : 0;
  if (px) px->seq = px_seq;
  b->launches++;
  if (lb) {
    b->slot = (b->slot + 1) % b->W;
    b->count = count;
  }
  return LLAMPC_OK;
}

namespace {

// plan_shape of a look-ahead alone, for what no bank decides: of n models (they matter to the LPM
// only; a plan input's own questions take n = 1), with the inline pack or a corridor offered.
PlanShape lookahead_shape(int64_t n, bool la, int32_t C, int32_t H, int32_t integrator, int32_t xref_mode,
                          int32_t share, bool pack, bool corridor, int32_t track_n = 0) {
  PlanShapeIn s{};
  s.n = n;
  s.la = la;
  s.C = C;
  s.H = H;
  s.integrator = integrator;
  s.xref_mode = xref_mode;
  s.share = share;
  s.pack = pack;
  s.corridor = corridor;
  s.track_n = track_n;
  return plan_shape(s, 0);
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
int stage_inputs(llampc_bank* b, const llampc_plan_in* in, llampc_plan_in* dev_in, hipStream_t s,
                 const double* hp = nullptr, const double** d_hp = nullptr) {
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

// The host-completion tick: the inputs inline or staged, the record into pinned host memory,
// then tick number *seq into the tag (wait_host_tag).
// hp: the corridor tick, whose inputs are always staged (the corridor rides with them).  tt: the track
// tick, staged too (its launch takes device inputs).
int plan_launch_host(llampc_bank* b, const llampc_plan_in* in, hipStream_t s, uint64_t* seq,
                     const double* hp = nullptr, double weight = 0.0, const TrackTick* tt = nullptr) {
  llampc_plan_in din = *in;
  InlinePack pk;
  PlanCorridor cor{nullptr, weight};
  const bool inl = !hp && !tt && inline_inputs(in);
  if (inl) pack_into(in, pk.v);
  else if (int rc = stage_inputs(b, in, &din, s, hp, &cor.hp)) return rc;
  *seq = ++b->hseq;
  return plan_launch(b, din, b->host.rec.dev(), nullptr, nullptr, nullptr, s, b->host.tag.dev(), *seq,
                     inl ? &pk : nullptr, nullptr, nullptr, hp ? &cor : nullptr, tt);
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

int status_fail(llampc_bank* b, int32_t status) {
  (void)recover_counters(b);
  return fail(LLAMPC_E_DEVICE, "tick record status %d (in-launch completion timed out)", status);
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

// A bank's stream.  HIP maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by
// default, least-used first), so two banks ticked concurrently — the two controllers of
// config 5 — can land on one queue and run one after the other: the two-track controller
// step measured 172 us instead of 98 us whenever two other streams were in use first
// (tools/diag/bench_extra.py).  A stream with a CU mask gets a hardware queue of its own;
// the mask holds every CU, so nothing else changes.  LLAMPC_SHARED_QUEUES=1 keeps the plain
// stream; the plain stream is also the fallback.  Only banks ticked concurrently get one
// (llampc_bank_set_concurrency(> 1), or LLAMPC_DEDICATED_QUEUE=1 at create): every other bank
// — a setupNLP's one-model bank, a host-mode nominal bank — keeps a plain non-blocking stream,
// so a process never opens more hardware queues than it has concurrent banks.
hipError_t bank_stream(int cus, bool dedicated, hipStream_t* s) {
  if (dedicated && !std::getenv("LLAMPC_SHARED_QUEUES") && cus > 0) {
    std::vector<uint32_t> mask((cus + 31) / 32, 0xFFFFFFFFu);
    if (cus % 32) mask.back() = (1u << (cus % 32)) - 1;
    if (hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data()) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
  }
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

}  // namespace

extern "C" {

int32_t llampc_abi_version(void) { return LLAMPC_ABI_VERSION; }

const char* llampc_last_error(void) { return g_err.c_str(); }

int llampc_device_count(int32_t* count) {
  if (!count) return fail(LLAMPC_E_ARG, "count is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    return fail(LLAMPC_E_NODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = c;
  return LLAMPC_OK;
}

int llampc_bank_create(const double* params, int64_t n, int64_t global_offset,
                       const llampc_vehicle* veh, int32_t W, int32_t device, llampc_bank** out) {
  if (!out) return fail(LLAMPC_E_ARG, "out is NULL");
  *out = nullptr;
  if (!params || !veh) return fail(LLAMPC_E_ARG, "params/veh is NULL");
  if (n < 1 || n > INT32_MAX)   // the kernels rank models by a 32-bit local index
    return fail(LLAMPC_E_ARG, "n=%lld must be in [1, 2^31-1]", (long long)n);
  if (W < 1 || W > LLAMPC_WMAX) return fail(LLAMPC_E_ARG, "W=%d outside [1, %d]", W, LLAMPC_WMAX);
  if (global_offset < 0) return fail(LLAMPC_E_ARG, "global_offset < 0");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(LLAMPC_E_NODEV, "no HIP device visible (the HIP path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(LLAMPC_E_ARG, "device %d of %d", device, ndev);
  DeviceGuard g(device);
  if (!g.ok) return fail(LLAMPC_E_HIP, "hipSetDevice(%d) failed", device);

  Building<llampc_bank> b(new llampc_bank(), llampc_bank_destroy);
  b->device = device;
  b->n = n;
  b->goff = global_offset;
  b->W = W;
  b->veh = make_veh(*veh);
  if (hipDeviceGetAttribute(&b->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) b->cus = 0;
  if (const char* e = std::getenv("LLAMPC_DEDICATED_QUEUE")) b->dedicated = e[0] == '1';
  if (bank_stream(b->cus, b->dedicated, &b->stream) != hipSuccess) return fail(LLAMPC_E_HIP, "hipStreamCreate failed");
  b->own_stream = true;
  const size_t lbl = (size_t)lookback_blocks(n) * (kBlock / 64);   // look-back lists (waves)
  const size_t lab = n;                  // worst case: one model per block (wave-role, G=64)
  int rc;
  if ((rc = b->d_params.alloc(6 * (size_t)n)) || (rc = b->d_ring.zalloc((size_t)W * n)) ||
      (rc = b->d_am_val.alloc(lbl)) || (rc = b->d_am_idx.alloc(lbl)) ||
      (rc = b->d_tk_val.alloc(lbl * LLAMPC_KMAX)) || (rc = b->d_tk_idx.alloc(lbl * LLAMPC_KMAX)) ||
      (rc = b->d_pv.alloc(lab)) || (rc = b->d_pidx.alloc(lab)) || (rc = b->d_pnf.alloc(lab)) ||
      (rc = b->d_best_cand.alloc(n)) || (rc = b->d_best_cost.alloc(n)) || (rc = b->d_err.alloc(n)) ||
      (rc = b->d_wmean.alloc(n)) || (rc = b->d_out.alloc(1)) || (rc = b->d_tickets.zalloc(2)) ||
      (rc = b->d_la_tag.zalloc(3 * (size_t)n)) || (rc = b->d_blk_tag.zalloc(5 * lab)) || (rc = b->d_wq.zalloc(1)) ||
      (rc = b->h_out.alloc(1, "out")) || (rc = b->host.alloc("host completion record")))
    return rc;
  if (hipMemcpy(b->d_params.get(), params, 6 * n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess)
    return fail(LLAMPC_E_HIP, "bank upload failed");
  *out = b.release();
  return LLAMPC_OK;
}

int llampc_bank_destroy(llampc_bank* b) {
  if (!b) return LLAMPC_OK;
  bank_disarm(b);
  DeviceGuard g(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  hipStream_t own = b->own_stream ? b->stream : nullptr;
  timing_free(b);
  delete b;                              // its buffers, on its device, ahead of its stream
  if (own) (void)hipStreamDestroy(own);
  return LLAMPC_OK;
}

int llampc_bank_info(const llampc_bank* b, int64_t* n, int64_t* goff, int32_t* W,
                     int32_t* window_count, int32_t* device) {
  if (!b) return fail(LLAMPC_E_ARG, "bank is NULL");
  if (n) *n = b->n;
  if (goff) *goff = b->goff;
  if (W) *W = b->W;
  if (window_count) *window_count = b->count;
  if (device) *device = b->device;
  return LLAMPC_OK;
}

int llampc_bank_launches(const llampc_bank* b, int64_t* launches) {
  if (!b || !launches) return fail(LLAMPC_E_ARG, "bank/launches is NULL");
  *launches = b->launches;
  return LLAMPC_OK;
}

int llampc_bank_reset(llampc_bank* b) {
  if (!b) return fail(LLAMPC_E_ARG, "bank is NULL");
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  DeviceGuard g(b->device);
  HIP_TRY(hipMemsetAsync(b->d_ring.get(), 0, (size_t)b->W * b->n * sizeof(double), b->stream));
  HIP_TRY(hipMemsetAsync(b->d_tickets.get(), 0, 2 * sizeof(unsigned), b->stream));
  HIP_TRY(hipMemsetAsync(b->d_wq.get(), 0, sizeof(uint64_t), b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->count = 0;
  b->slot = 0;
  b->trk_path = track_path_next(b->trk_path, kPathClear);
  return LLAMPC_OK;
}

int llampc_bank_window(llampc_bank* b, double* ring, int32_t* window_count) {
  if (!b || !ring) return fail(LLAMPC_E_ARG, "bank/ring is NULL");
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  DeviceGuard g(b->device);
  std::vector<double> raw((size_t)b->W * b->n);
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(raw.data(), b->d_ring.get(), raw.size() * sizeof(double), hipMemcpyDeviceToHost));
  window_unroll(raw.data(), b->n, b->W, b->count, b->slot, ring);
  if (window_count) *window_count = b->count;
  return LLAMPC_OK;
}

int llampc_bank_stream(const llampc_bank* b, void** stream) {
  if (!b || !stream) return fail(LLAMPC_E_ARG, "NULL argument");
  *stream = (void*)b->stream;
  return LLAMPC_OK;
}

}  // extern "C"

// A stream from bank_stream replaces the bank's plain one.
int bank_dedicate(llampc_bank* b) {
  if (b->dedicated) return LLAMPC_OK;
  b->dedicated = true;
  if (b->own_stream) {
    DeviceGuard g(b->device);
    HIP_TRY(hipStreamSynchronize(b->stream));
    hipStream_t s = nullptr;
    HIP_TRY(bank_stream(b->cus, true, &s));
    (void)hipStreamDestroy(b->stream);
    b->stream = s;
  }
  return LLAMPC_OK;
}

extern "C" {

int llampc_bank_set_concurrency(llampc_bank* b, int32_t banks) {
  if (!b) return fail(LLAMPC_E_ARG, "bank is NULL");
  if (banks < 1 || banks > 64) return fail(LLAMPC_E_ARG, "banks=%d outside [1, 64]", banks);
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  b->share = banks;
  if (banks > 1) return bank_dedicate(b);   // concurrent banks: a hardware queue of its own
  return LLAMPC_OK;
}

int llampc_bank_set_stream(llampc_bank* b, void* stream) {
  if (!b) return fail(LLAMPC_E_ARG, "bank is NULL");
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  DeviceGuard g(b->device);
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (b->own_stream) (void)hipStreamDestroy(b->stream);
  if (stream) {
    b->stream = (hipStream_t)stream;
    b->own_stream = false;
  } else {
    HIP_TRY(bank_stream(b->cus, b->dedicated, &b->stream));
    b->own_stream = true;
  }
  return LLAMPC_OK;
}

int llampc_bank_timing(llampc_bank* b, int32_t enable, int32_t max_launches) {
  if (!b) return fail(LLAMPC_E_ARG, "bank is NULL");
  std::lock_guard<std::mutex> lk(b->mu);
  DeviceGuard g(b->device);
  HIP_TRY(hipStreamSynchronize(b->stream));
  timing_free(b);
  if (!enable) return LLAMPC_OK;
  if (enable == INT32_MIN) return fail(LLAMPC_E_ARG, "bad enable");
  if (max_launches < 1) return fail(LLAMPC_E_ARG, "max_launches must be >= 1");
  for (auto& v : b->ev) {
    v.resize(2 * (size_t)max_launches, nullptr);
    for (hipEvent_t& e : v) HIP_TRY(hipEventCreate(&e));
  }
  b->timing = true;
  b->timing_stride = enable < 0 ? -(int64_t)enable : enable;
  b->timing_sample = enable < 0;
  return LLAMPC_OK;
}

int llampc_bank_timing_read(llampc_bank* b, double* avg_ms, int64_t* count) {
  if (!b || !avg_ms || !count) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(b->mu);
  DeviceGuard g(b->device);
  for (int k = 0; k < 3; ++k) {
    double tot = 0.0;
    for (size_t i = 0; i < b->ev_used[k]; ++i) {
      HIP_TRY(hipEventSynchronize(b->ev[k][2 * i + 1]));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, b->ev[k][2 * i], b->ev[k][2 * i + 1]));
      tot += ms;
    }
    const int64_t per = b->timing_sample ? 1 : b->timing_stride;   // launches per pair
    count[k] = (int64_t)b->ev_used[k] * per;
    avg_ms[k] = b->ev_used[k] ? tot / ((double)b->ev_used[k] * per) : 0.0;
    b->ev_used[k] = 0;
    b->timing_seen[k] = 0;
  }
  return LLAMPC_OK;
}

}  // extern "C"

// What a corridor tick refuses before anything is enqueued (llampc_plan_corridor,
// llampc_lookahead_corridor): no look-ahead, RK6, the per-model raceline reference — plan_shape's
// refusals of the corridor's modes, in its words (the rest of the input is check_plan_in's to
// judge) — then a corridor or weight corridor_invalid names.
static int check_corridor_mode(const llampc_plan_in* in) {
  const char* why =
      lookahead_shape(1, in->do_lookahead != 0, in->C, in->H, in->integrator, in->xref_mode, 1, false, true).refuse;
  if (why == kNoCorridorLookahead || why == kNoCorridorRk6 || why == kNoCorridorRaceline)
    return fail(LLAMPC_E_ARG, "%s", why);
  return LLAMPC_OK;
}

// What a track tick refuses before anything is enqueued (llampc_plan_track, llampc_plan_track_async; the
// caller holds b->mu): no track, an async tick outstanding (LLAMPC_E_STATE), then plan_shape's refusals
// of the track tick's modes, in its words, and a weight or margin track_tick_invalid names.
static int check_track_tick(const llampc_bank* b, const llampc_plan_in* in, const TrackTick& tt) {
  if (!b->tr_n) return fail(LLAMPC_E_STATE, "no track set: call llampc_bank_set_track first");
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding: call llampc_plan_wait");
  if (in) {
    const char* why = lookahead_shape(1, in->do_lookahead != 0, in->C, in->H, in->integrator, in->xref_mode, 1, false,
                                      false, b->tr_n).refuse;
    if (why == kNoTrackLookahead || why == kNoTrackRk6 || why == kNoTrackEuler || why == kNoTrackRaceline)
      return fail(LLAMPC_E_ARG, "%s", why);
  }
  if (const char* why = track_tick_invalid(tt.weight, tt.margin, b->tr_width)) return fail(LLAMPC_E_ARG, "track tick: %s", why);
  return LLAMPC_OK;
}

// llampc_plan (hp null), llampc_plan_corridor and (tt) llampc_plan_track: the blocking host-pointer tick.
static int plan_blocking(llampc_bank* b, const llampc_plan_in* in, const double* hp, double weight,
                         llampc_plan_out* out, double* err_out, double* wmean_out, double* cost_out,
                         const TrackTick* tt = nullptr) {
  if (!b || !out) return fail(LLAMPC_E_ARG, "bank/out is NULL");
  int rc;
  if (hp && in && (rc = check_corridor_mode(in))) return rc;   // E_ARG whatever else the bank lacks
  // the track tick's refusals first, in their table's order, under the lock the launch is made under: the
  // track and the outstanding async tick they are decided by cannot change in between
  std::unique_lock<std::mutex> lk(b->mu, std::defer_lock);
  if (tt) {
    lk.lock();
    if ((rc = check_track_tick(b, in, *tt))) return rc;
  }
  if ((rc = check_plan_in(b, in))) return rc;
  if (tt && in->H > LLAMPC_HMAX) return fail(LLAMPC_E_ARG, "H=%d above %d (the path state's horizon)", in->H, LLAMPC_HMAX);
  if (hp)                                // H is valid from here on
    if (const char* why = corridor_invalid(hp, in->H, weight)) return fail(LLAMPC_E_ARG, "corridor: %s", why);
  if (!lk.owns_lock()) lk.lock();
  bank_disarm(b);
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding: call llampc_plan_wait");
  DeviceGuard g(b->device);
  hipStream_t s = b->stream;
  if (!err_out && !wmean_out && !cost_out && host_completion()) {
    // the record only: the kernel writes it to pinned host memory and publishes a tag
    uint64_t seq;
    if ((rc = plan_launch_host(b, in, s, &seq, hp, weight, tt)) || (rc = wait_host_tag(b, seq, out))) return rc;
    if (out->status) return status_fail(b, out->status);
    return LLAMPC_OK;
  }
  double* d_cost = nullptr;
  if (cost_out && in->do_lookahead) {
    if ((rc = b->d_cost.reserve((size_t)b->n * in->C))) return rc;
    d_cost = b->d_cost.get();
  }
  llampc_plan_in din;
  PlanCorridor cor{nullptr, weight};
  if ((rc = stage_inputs(b, in, &din, s, hp, &cor.hp))) return rc;
  if ((rc = plan_launch(b, din, b->d_out.get(), err_out ? b->d_err.get() : nullptr,
                        wmean_out ? b->d_wmean.get() : nullptr, d_cost, s, nullptr, 0, nullptr, nullptr, nullptr,
                        hp ? &cor : nullptr, tt)))
    return rc;
  HIP_TRY(hipMemcpyAsync(b->h_out.get(), b->d_out.get(), sizeof(llampc_plan_out), hipMemcpyDeviceToHost, s));
  if (err_out && in->do_lookback)
    HIP_TRY(hipMemcpyAsync(err_out, b->d_err.get(), b->n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (wmean_out && in->do_lookback && b->count >= b->W)
    HIP_TRY(hipMemcpyAsync(wmean_out, b->d_wmean.get(), b->n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (d_cost)
    HIP_TRY(hipMemcpyAsync(cost_out, d_cost, (size_t)b->n * in->C * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *out = *b->h_out.get();
  if (out->status) return status_fail(b, out->status);
  return LLAMPC_OK;
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

}  // extern "C"

// The track tick's device state, allocated with the first track or path (the caller holds b->mu, the
// bank's device is current): the path copies, their costs and the read-back, the flags, the tagged words.
static int track_state(llampc_bank* b) {
  if (b->d_trk) return LLAMPC_OK;
  int rc;
  if ((rc = b->d_trk.zalloc(4 * (size_t)kPlanPathStride + 2 + (size_t)kPlanTrackDbgDoubles, "track tick path state")) ||
      (rc = b->d_trk_flags.zalloc(4, "track tick flags")) ||
      (rc = b->d_hp_tag.zalloc(12 * (size_t)LLAMPC_HMAX, "track tick half-plane words")))
    return rc;
  return LLAMPC_OK;
}

extern "C" {

int llampc_bank_set_track(llampc_bank* b, const double* centre, const double* theta, int32_t n, double track_length,
                          double track_width) {
  if (!b || !centre || !theta) return fail(LLAMPC_E_ARG, "NULL argument");
  char why[128];
  if (track_tables_invalid(centre, theta, n, track_length, track_width, why, sizeof why)) return fail(LLAMPC_E_ARG, "%s", why);
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding on the bank");
  DeviceGuard g(b->device);
  HIP_TRY(hipStreamSynchronize(b->stream));      // no launch reads the tables being replaced
  b->tr_n = 0;
  b->trk_path = track_path_next(b->trk_path, kPathClear);
  b->trk_last_H = 0;
  int rc;
  if ((rc = track_state(b)) || (rc = b->d_track.reserve(3 * (size_t)n, 0, "track tables"))) return rc;
  std::vector<double> h(3 * (size_t)n);
  std::memcpy(h.data(), centre, 2 * (size_t)n * sizeof(double));
  std::memcpy(h.data() + 2 * (size_t)n, theta, (size_t)n * sizeof(double));
  HIP_TRY(hipMemcpy(b->d_track.get(), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  b->tr_n = n;
  b->tr_L = track_length;
  b->tr_width = track_width;
  return LLAMPC_OK;
}

int llampc_bank_set_path(llampc_bank* b, const double* path, int32_t H) {
  if (!b) return fail(LLAMPC_E_ARG, "bank is NULL");
  if (path) {
    if (H < 1 || H > LLAMPC_HMAX) return fail(LLAMPC_E_ARG, "H=%d outside [1, %d]", H, LLAMPC_HMAX);
    for (int i = 0; i < 2 * (H + 1); ++i)
      if (!std::isfinite(path[i])) return fail(LLAMPC_E_ARG, "path: entry %d is not finite", i);
  }
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding on the bank");
  if (!path) {
    b->trk_path = track_path_next(b->trk_path, kPathClear);
    return LLAMPC_OK;
  }
  DeviceGuard g(b->device);
  HIP_TRY(hipStreamSynchronize(b->stream));      // no launch reads or writes the copy being seeded
  if (int rc = track_state(b)) return rc;
  std::vector<double> h(2 * (size_t)kPlanPathStride, 0.0);
  for (int r = 0; r < 2; ++r) std::memcpy(h.data() + (size_t)r * kPlanPathStride, path + (size_t)r * (H + 1), (H + 1) * sizeof(double));
  const int32_t one = 1;
  HIP_TRY(hipMemcpy(b->d_trk.get() + 2 * (size_t)kPlanPathStride * b->trk_cur, h.data(), h.size() * sizeof(double),
                    hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_trk_flags.get() + b->trk_cur, &one, sizeof one, hipMemcpyHostToDevice));
  b->trk_path = track_path_next(b->trk_path, kPathSeed, H);
  return LLAMPC_OK;
}

int llampc_plan_track_async(llampc_bank* b, const llampc_plan_in* in, double weight, double margin) {
  if (!b) return fail(LLAMPC_E_ARG, "bank is NULL");
  const TrackTick tt{weight, margin};
  std::lock_guard<std::mutex> lk(b->mu);
  int rc;
  if ((rc = check_track_tick(b, in, tt)) || (rc = check_plan_in(b, in))) return rc;
  if (in->H > LLAMPC_HMAX) return fail(LLAMPC_E_ARG, "H=%d above %d (the path state's horizon)", in->H, LLAMPC_HMAX);
  bank_disarm(b);
  DeviceGuard g(b->device);
  hipStream_t s = b->stream;
  if (host_completion()) {
    uint64_t seq;
    if ((rc = plan_launch_host(b, in, s, &seq, nullptr, 0.0, &tt))) return rc;
    b->async_seq = seq;
  } else {
    llampc_plan_in din;
    if ((rc = stage_inputs(b, in, &din, s))) return rc;
    b->async_seq = 0;
    if ((rc = plan_launch(b, din, b->d_out.get(), nullptr, nullptr, nullptr, s, nullptr, 0, nullptr, nullptr, nullptr,
                          nullptr, &tt)))
      return rc;
    HIP_TRY(hipMemcpyAsync(b->h_out.get(), b->d_out.get(), sizeof(llampc_plan_out), hipMemcpyDeviceToHost, s));
  }
  b->async_pending = true;
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
  const size_t ps = 2 * (size_t)kPlanPathStride;
  std::vector<double> h(2 * ps + 2 + (size_t)kPlanTrackDbgDoubles);
  int32_t fl[4];
  HIP_TRY(hipMemcpy(h.data(), b->d_trk.get(), h.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(fl, b->d_trk_flags.get(), sizeof fl, hipMemcpyDeviceToHost));
  const int cur = b->trk_cur;            // the copy the tick wrote
  const double* dbg = h.data() + 2 * ps + 2;
  for (int r = 0; r < 2; ++r) {
    std::memcpy(path + (size_t)r * (H + 1), dbg + (size_t)r * kPlanPathStride, (H + 1) * sizeof(double));
    std::memcpy(next_path + (size_t)r * (H + 1), h.data() + ps * cur + (size_t)r * kPlanPathStride, (H + 1) * sizeof(double));
  }
  std::memcpy(hp, dbg + ps, 6 * (size_t)H * sizeof(double));
  std::memcpy(theta, dbg + ps + 6 * LLAMPC_HMAX, (size_t)H * sizeof(double));
  *valid = fl[2];
  *next_valid = fl[cur];
  *next_cost = h[2 * ps + cur];
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

int llampc_bank_set_raceline(llampc_bank* b, const double* knots, int32_t n, const double* xy,
                             const double* speed, const double* mus, int32_t M) {
  if (!b || !knots || !xy || !speed || !mus) return fail(LLAMPC_E_ARG, "NULL argument");
  if (n < 2 || M < 1 || M > 64) return fail(LLAMPC_E_ARG, "n=%d (>= 2) M=%d (1..64)", n, M);
  if (raceline_lds_bytes(n, M) > 60 * 1024)
    return fail(LLAMPC_E_ARG, "raceline of %d knots exceeds the 60 KB LDS stage", n);
  for (int32_t i = 1; i < n; ++i)
    if (!(knots[i] > knots[i - 1])) return fail(LLAMPC_E_ARG, "knots must increase (at %d)", i);
  for (int32_t i = 1; i < M; ++i)
    if (!(mus[i] >= mus[i - 1])) return fail(LLAMPC_E_ARG, "mus must be ascending (at %d)", i);
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  DeviceGuard g(b->device);
  HIP_TRY(hipStreamSynchronize(b->stream));
  const size_t m = (size_t)n - 1;
  const size_t total = (size_t)n + 8 * m + 4 * m * M + M;
  b->rl_n = b->rl_M = 0;
  if (int rc = b->d_rl.alloc(total)) return rc;
  double* d = b->d_rl.get();
  HIP_TRY(hipMemcpy(d, knots, n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d + n, xy, 8 * m * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d + n + 8 * m, speed, 4 * m * M * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d + n + 8 * m + 4 * m * M, mus, M * sizeof(double), hipMemcpyHostToDevice));
  b->rl_n = n;
  b->rl_M = M;
  b->rl_mus.assign(mus, mus + M);
  double hmin = knots[1] - knots[0];
  for (int32_t i = 2; i < n; ++i) hmin = std::min(hmin, knots[i] - knots[i - 1]);
  b->rl_hmin = hmin;
  b->rl_vmax = speed_bound(knots, speed, n, M);
  return LLAMPC_OK;
}

int llampc_plan_async(llampc_bank* b, const llampc_plan_in* in) {
  if (!b) return fail(LLAMPC_E_ARG, "bank is NULL");
  int rc = check_plan_in(b, in);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding: call llampc_plan_wait");
  DeviceGuard g(b->device);
  hipStream_t s = b->stream;
  if (host_completion()) {
    uint64_t seq;
    if ((rc = plan_launch_host(b, in, s, &seq))) return rc;
    b->async_seq = seq;
  } else {
    llampc_plan_in din;
    if ((rc = stage_inputs(b, in, &din, s))) return rc;
    b->async_seq = 0;
    if ((rc = plan_launch(b, din, b->d_out.get(), nullptr, nullptr, nullptr, s))) return rc;
    HIP_TRY(hipMemcpyAsync(b->h_out.get(), b->d_out.get(), sizeof(llampc_plan_out), hipMemcpyDeviceToHost, s));
  }
  b->async_pending = true;
  return LLAMPC_OK;
}

int llampc_plan_wait(llampc_bank* b, llampc_plan_out* out) {
  if (!b || !out) return fail(LLAMPC_E_ARG, "bank/out is NULL");
  std::lock_guard<std::mutex> lk(b->mu);
  if (!b->async_pending) return fail(LLAMPC_E_STATE, "no async tick outstanding");
  DeviceGuard g(b->device);
  b->async_pending = false;
  if (b->async_seq) {
    if (int rc = wait_host_tag(b, b->async_seq, out)) return rc;
  } else {
    HIP_TRY(hipStreamSynchronize(b->stream));
    *out = *b->h_out.get();
  }
  if (out->status) return status_fail(b, out->status);
  return LLAMPC_OK;
}

int llampc_plan_device(llampc_bank* b, const llampc_plan_in* in, void* d_out, double* d_err,
                       double* d_wmean, double* d_cost, void* stream) {
  if (!b || !d_out) return fail(LLAMPC_E_ARG, "bank/d_out is NULL");
  int rc = check_plan_in(b, in);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  // an outstanding async tick shares the tickets, tags, ring slot and window count
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding: call llampc_plan_wait");
  DeviceGuard g(b->device);
  return plan_launch(b, *in, (llampc_plan_out*)d_out, d_err, d_wmean, d_cost, pick_stream(b, stream));
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

}  // extern "C"

// llampc_lookahead (hp null) and llampc_lookahead_corridor.
static int lookahead_blocking(llampc_bank* b, const double* x0, const double* U, int32_t C, int32_t H,
                              const double* xref, const double* uprev, const llampc_cost* cost, double Ts,
                              int32_t integrator, const double* hp, double weight, double* cost_out,
                              int32_t* best_cand_out, int64_t* best_model, int32_t* best_cand, double* best_cost) {
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

extern "C" {

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

int llampc_merge(const llampc_plan_out* parts, int32_t G, int32_t nan_policy, llampc_plan_out* merged) {
  if (!parts || !merged || G < 1) return fail(LLAMPC_E_ARG, "bad merge arguments");
  for (int g = 1; g < G; ++g)
    if (parts[g].K != parts[0].K || parts[g].window_count != parts[0].window_count)
      return fail(LLAMPC_E_STATE, "shard %d disagrees on K/window (K %d vs %d, count %d vs %d)", g,
                  parts[g].K, parts[0].K, parts[g].window_count, parts[0].window_count);
  merge_plan_parts(parts, G, nan_policy == LLAMPC_NAN_FIRST, merged);
  return LLAMPC_OK;
}

int llampc_merge_device(const void* d_parts, int32_t G, int32_t nan_policy, void* d_merged,
                        int32_t device, void* stream) {
  if (!d_parts || !d_merged || G < 1) return fail(LLAMPC_E_ARG, "bad merge arguments");
  DeviceGuard g(device);
  if (!g.ok) return fail(LLAMPC_E_HIP, "hipSetDevice(%d) failed", device);
  HIP_TRY(launch_merge((const llampc_plan_out*)d_parts, G, nan_policy == LLAMPC_NAN_FIRST,
                       (llampc_plan_out*)d_merged, (hipStream_t)stream));
  return LLAMPC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// Raw batched dynamics: per-device cached workspace + stream
// ------------------------------------------------------------------------------------
namespace {

struct Workspace {
  std::mutex mu;
  DevBuf<char> d;
  hipStream_t stream = nullptr;
};
Workspace* const g_ws = new Workspace[64];   // never deleted: nothing is freed at process exit

int ws_get(int device, size_t bytes, Workspace** out) {
  if (device < 0 || device >= 64) return fail(LLAMPC_E_ARG, "device %d", device);
  Workspace& w = g_ws[device];
  if (!w.stream) HIP_TRY(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
  if (int rc = w.d.reserve(bytes, 1 << 20)) return rc;
  *out = &w;
  return LLAMPC_OK;
}

int resolve_device(int32_t device, int* out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(LLAMPC_E_NODEV, "no HIP device visible (the HIP path has no CPU fallback)");
  int d = device;
  if (d < 0 && hipGetDevice(&d) != hipSuccess) d = 0;
  if (d >= ndev) return fail(LLAMPC_E_ARG, "device %d of %d", d, ndev);
  *out = d;
  return LLAMPC_OK;
}

size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

extern "C" int llampc_dynamics_batch(int32_t op, const double* x, const double* u,
                                     const double* params, int64_t P, const llampc_vehicle* veh,
                                     int64_t n, double* out, int32_t device, int32_t device_ptrs,
                                     void* stream) {
  if (!x || !u || !params || !veh || !out) return fail(LLAMPC_E_ARG, "NULL argument");
  if (op != LLAMPC_OP_FORCES && op != LLAMPC_OP_DERIV) return fail(LLAMPC_E_ARG, "op %d", op);
  if (n < 0 || !(P == 1 || P == n)) return fail(LLAMPC_E_ARG, "P=%lld must be 1 or n=%lld", (long long)P, (long long)n);
  if (n == 0) return LLAMPC_OK;
  int dev, rc;
  if ((rc = resolve_device(device, &dev))) return rc;
  DeviceGuard g(dev);
  const VehK vk = make_veh(*veh);
  const size_t out_n = (op == LLAMPC_OP_FORCES ? 5 : 6) * (size_t)n;
  if (device_ptrs) {
    HIP_TRY(launch_dynamics(op, x, u, params, P, vk, n, out, (hipStream_t)stream));
    return LLAMPC_OK;
  }
  const size_t bx = align_up(6 * n * 8), bu = align_up(2 * n * 8), bp = align_up(6 * P * 8),
               bo = align_up(out_n * 8);
  Workspace* w;
  std::lock_guard<std::mutex> lk(g_ws[dev].mu);
  if ((rc = ws_get(dev, bx + bu + bp + bo, &w))) return rc;
  char* base = w->d.get();
  double *dx = (double*)base, *du = (double*)(base + bx), *dp = (double*)(base + bx + bu),
         *dout = (double*)(base + bx + bu + bp);
  HIP_TRY(hipMemcpyAsync(dx, x, 6 * n * 8, hipMemcpyHostToDevice, w->stream));
  HIP_TRY(hipMemcpyAsync(du, u, 2 * n * 8, hipMemcpyHostToDevice, w->stream));
  HIP_TRY(hipMemcpyAsync(dp, params, 6 * P * 8, hipMemcpyHostToDevice, w->stream));
  HIP_TRY(launch_dynamics(op, dx, du, dp, P, vk, n, dout, w->stream));
  HIP_TRY(hipMemcpyAsync(out, dout, out_n * 8, hipMemcpyDeviceToHost, w->stream));
  HIP_TRY(hipStreamSynchronize(w->stream));
  return LLAMPC_OK;
}

extern "C" int llampc_integrate_batch(const double* x0, const double* u, int64_t u_stride_lane,
                                      const double* h, int32_t S, const double* params, int64_t P,
                                      const llampc_vehicle* veh, int64_t n, int32_t integrator,
                                      double* traj_out, int32_t final_only, int32_t device,
                                      int32_t device_ptrs, void* stream) {
  if (!x0 || !u || !h || !params || !veh || !traj_out) return fail(LLAMPC_E_ARG, "NULL argument");
  if (S < 1) return fail(LLAMPC_E_ARG, "S=%d must be >= 1", S);
  if (n < 0 || !(P == 1 || P == n)) return fail(LLAMPC_E_ARG, "P must be 1 or n");
  if (!(u_stride_lane == 0 || u_stride_lane == 2 * (int64_t)S))
    return fail(LLAMPC_E_ARG, "u_stride_lane must be 0 or 2*S");
  if (integrator < LLAMPC_RK4 || integrator > LLAMPC_RK6) return fail(LLAMPC_E_ARG, "integrator %d", integrator);
  if (n == 0) return LLAMPC_OK;
  int dev, rc;
  if ((rc = resolve_device(device, &dev))) return rc;
  DeviceGuard g(dev);
  const VehK vk = integrator_veh(make_veh(*veh), integrator);
  const size_t out_n = (final_only ? 1 : (size_t)(S + 1)) * n * 6;
  if (device_ptrs) {
    HIP_TRY(launch_integrate(x0, u, u_stride_lane, h, S, params, P, vk, n, integrator, traj_out,
                             final_only, (hipStream_t)stream));
    return LLAMPC_OK;
  }
  const size_t un = (u_stride_lane ? (size_t)n : 1) * 2 * S;
  const size_t bx = align_up(6 * n * 8), bu = align_up(un * 8), bh = align_up(S * 8),
               bp = align_up(6 * P * 8), bo = align_up(out_n * 8);
  Workspace* w;
  std::lock_guard<std::mutex> lk(g_ws[dev].mu);
  if ((rc = ws_get(dev, bx + bu + bh + bp + bo, &w))) return rc;
  char* base = w->d.get();
  double *dx = (double*)base, *du = (double*)(base + bx), *dh = (double*)(base + bx + bu),
         *dp = (double*)(base + bx + bu + bh), *dout = (double*)(base + bx + bu + bh + bp);
  HIP_TRY(hipMemcpyAsync(dx, x0, 6 * n * 8, hipMemcpyHostToDevice, w->stream));
  HIP_TRY(hipMemcpyAsync(du, u, un * 8, hipMemcpyHostToDevice, w->stream));
  HIP_TRY(hipMemcpyAsync(dh, h, S * 8, hipMemcpyHostToDevice, w->stream));
  HIP_TRY(hipMemcpyAsync(dp, params, 6 * P * 8, hipMemcpyHostToDevice, w->stream));
  HIP_TRY(launch_integrate(dx, du, u_stride_lane, dh, S, dp, P, vk, n, integrator, dout, final_only,
                           w->stream));
  HIP_TRY(hipMemcpyAsync(traj_out, dout, out_n * 8, hipMemcpyDeviceToHost, w->stream));
  HIP_TRY(hipStreamSynchronize(w->stream));
  return LLAMPC_OK;
}

// The variant a given-xref look-ahead of these sizes takes, without or with a corridor: the
// launch's own plan_shape.
static void plan_variant(int64_t n, int32_t C, int32_t H, int32_t integrator, int32_t share, bool corridor,
                         int32_t out[4]) {
  const PlanShape s = lookahead_shape(n, true, C, H, integrator, LLAMPC_XREF_GIVEN, share, false, corridor);
  out[0] = s.lpm;
  out[1] = s.G;
  out[2] = s.cpl;
  out[3] = s.stage ? 1 : 0;
}

extern "C" int llampc_plan_variant(int64_t n, int32_t C, int32_t H, int32_t integrator, int32_t share,
                                   int32_t out[4]) {
  if (!out) return fail(LLAMPC_E_ARG, "NULL argument");
  if (n < 1 || C < 1 || H < 1 || integrator < LLAMPC_RK4 || integrator > LLAMPC_RK6)
    return fail(LLAMPC_E_ARG, "n %lld, C %d, H %d, integrator %d", (long long)n, C, H, integrator);
  plan_variant(n, C, H, integrator, share, false, out);
  return LLAMPC_OK;
}

extern "C" int llampc_plan_variant_corridor(int64_t n, int32_t C, int32_t H, int32_t integrator, int32_t share,
                                            int32_t out[4]) {
  if (!out) return fail(LLAMPC_E_ARG, "NULL argument");
  if (n < 1 || C < 1 || H < 1 || (integrator != LLAMPC_RK4 && integrator != LLAMPC_EULER_NLP))
    return fail(LLAMPC_E_ARG, "n %lld, C %d, H %d, integrator %d (the corridor look-ahead: RK4 or NLP-Euler)",
                (long long)n, C, H, integrator);
  plan_variant(n, C, H, integrator, share, true, out);
  return LLAMPC_OK;
}

extern "C" int llampc_math_batch(int32_t fn, const double* a, const double* b, int64_t n,
                                 double* out, int32_t device) {
  if (!a || !out || ((fn == LLAMPC_MATH_ATAN2_XPOS || fn == LLAMPC_MATH_ATAN2_FAST ||
                      fn == LLAMPC_MATH_ATAN2_LEAN || fn == LLAMPC_MATH_ATAN2_PAIR) && !b))
    return fail(LLAMPC_E_ARG, "NULL argument");
  if (fn < LLAMPC_MATH_ATAN2_XPOS || fn > LLAMPC_MATH_ATAN_PAIR) return fail(LLAMPC_E_ARG, "fn %d", fn);
  if (n <= 0) return LLAMPC_OK;
  int dev, rc;
  if ((rc = resolve_device(device, &dev))) return rc;
  DeviceGuard g(dev);
  const size_t bn = align_up(n * 8);
  Workspace* w;
  std::lock_guard<std::mutex> lk(g_ws[dev].mu);
  if ((rc = ws_get(dev, 3 * bn, &w))) return rc;
  char* base = w->d.get();
  double *da = (double*)base, *db = (double*)(base + bn), *dout = (double*)(base + 2 * bn);
  HIP_TRY(hipMemcpyAsync(da, a, n * 8, hipMemcpyHostToDevice, w->stream));
  if (b) HIP_TRY(hipMemcpyAsync(db, b, n * 8, hipMemcpyHostToDevice, w->stream));
  HIP_TRY(launch_math(fn, da, db, n, dout, w->stream));
  HIP_TRY(hipMemcpyAsync(out, dout, n * 8, hipMemcpyDeviceToHost, w->stream));
  HIP_TRY(hipStreamSynchronize(w->stream));
  return LLAMPC_OK;
}

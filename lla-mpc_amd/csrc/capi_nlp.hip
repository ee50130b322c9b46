// capi_nlp.hip — the setupNLP.solve drop-in's host side (llampc_nlp_*, include/llampc.h;
// nlp.hip): CEM iterations enqueued back to back on the bank's stream, the Euler trajectory of
// the best sequence, the result through pinned host memory.  The corridor solve
// (llampc_nlp_solve_corridor) is the same solve with the half-planes handed over in a pinned mapped
// buffer and the largest slack of the returned trajectory computed here on the host.  With a track
// set (llampc_nlp_set_track: the centre line's tables, uploaded once) llampc_nlp_solve_track builds
// those half-planes on the device instead: track_corridor_kernel (kernels.hip, corridor_dev.hpp)
// writes them into the same buffer, enqueued ahead of the corridor solve on the same stream with no
// host synchronisation between the two; llampc_nlp_track_corridor is that kernel alone.
#include "capi_common.hpp"

using namespace llampc;

static_assert(sizeof(llampc_nlp_cfg) == 16 + 8 + 16 + 8 + 8 + sizeof(llampc_cost) + 32, "llampc_nlp_cfg layout");

struct __attribute__((visibility("hidden"))) llampc_nlp {
  llampc_bank* b = nullptr;
  llampc_nlp_cfg cfg{};
  DevBuf<NlpState> d_st;                 // the best so far across a solve's launches (device);
                                         // the inputs travel as kernel arguments (NlpInline)
  DevBuf<double> d_cost;                 // the sample blocks' sorted lists as tagged words
                                         // [2][3][samples], then the rounds' rate-clipped
                                         // sequences [2][samples][H][2] (NlpLaunch.list_tag, cand;
                                         // by round parity)
  DevBuf<uint64_t> d_ms_tag;             // [2][4 HMAX]: a round's mean / std (NlpLaunch.ms_tag)
  bool per_round = false;                // one launch per round (LLAMPC_NLP_ROUND_LAUNCHES=1: A/B)
  bool ltraj = false;                    // the last round keeps its states in LDS (NlpLaunch.ltraj;
                                         // LLAMPC_NLP_RERUN_TRAJ=1 at create: always re-run, tests)
  MappedRecord<NlpResult> host;          // the last round writes the result, then the solve's number
  Mapped<double> hp;                     // the corridor solve's half-planes [HMAX][6] (NlpCorridor.hp):
                                         // pinned and mapped, written by the host before the launch
                                         // or by track_corridor_kernel ahead of it, read once per
                                         // block and launch (no H2D copy); then that kernel's
                                         // theta [HMAX]
  DevBuf<double> d_track;                // llampc_nlp_set_track: cx | cy | tt, [3][tr_n]
  int32_t tr_n = 0;                      // 0: no track set
  double tr_L = 0.0, tr_width = 0.0;
  bool ltraj_cor = false;                // ltraj of a corridor solve (its LDS holds the half-planes too)
  uint64_t calls = 0;
  std::mutex mu;
};

// The cfg checks of llampc_nlp_create and llampc_nlp_batch_create.
int nlp_check_cfg(const llampc_nlp_cfg& k) {
  if (k.H < 1 || k.H > LLAMPC_HMAX) return fail(LLAMPC_E_ARG, "H=%d outside [1, %d]", k.H, LLAMPC_HMAX);
  if (k.samples < 64 || k.samples > 4096 || (k.samples & (k.samples - 1)))
    return fail(LLAMPC_E_ARG, "samples=%d: a power of two in [64, 4096]", k.samples);
  if (k.elite < 1 || k.elite > 64 || k.elite > k.samples || k.iters < 1 || k.iters > kNlpMaxIters)
    return fail(LLAMPC_E_ARG, "elite=%d (1..64, <= samples) iters=%d (1..%d)", k.elite, k.iters, kNlpMaxIters);
  if (!(k.Ts > 0) || !std::isfinite(k.Ts)) return fail(LLAMPC_E_ARG, "Ts must be finite > 0");
  if (nlp_lds_bytes(k.H, k.samples, k.elite) > 160 * 1024) return fail(LLAMPC_E_ARG, "H x elite too large for LDS");
  return LLAMPC_OK;
}

extern "C" {

int llampc_nlp_destroy(llampc_nlp* p) {
  if (!p) return LLAMPC_OK;
  DeviceGuard g(p->b->device);
  if (p->b->stream) (void)hipStreamSynchronize(p->b->stream);
  delete p;
  return LLAMPC_OK;
}

int llampc_nlp_create(llampc_bank* b, const llampc_nlp_cfg* cfg, llampc_nlp** out) {
  if (!out) return fail(LLAMPC_E_ARG, "out is NULL");
  *out = nullptr;
  if (!b || !cfg) return fail(LLAMPC_E_ARG, "NULL argument");
  const llampc_nlp_cfg& k = *cfg;
  if (b->n != 1) return fail(LLAMPC_E_ARG, "the NLP solver's bank holds one model (n=%lld)", (long long)b->n);
  if (int rc = nlp_check_cfg(k)) return rc;
  DeviceGuard g(b->device);
  Building<llampc_nlp> p(new llampc_nlp(), llampc_nlp_destroy);
  p->b = b;
  p->cfg = k;
  const size_t H = (size_t)k.H;
  int rc;
  // the lists: 3 words per entry, samples / 64 x len <= samples entries; both by round parity.
  // Tagged words start at tag 0, which no solve uses (nlp_seq of a solve number >= 1)
  if ((rc = p->d_st.zalloc(1)) || (rc = p->d_cost.zalloc((size_t)k.samples * (6 + 4 * H))) ||
      (rc = p->d_ms_tag.zalloc(8 * (size_t)LLAMPC_HMAX)) || (rc = p->host.alloc("NLP result")) ||
      (rc = p->hp.alloc(7 * (size_t)LLAMPC_HMAX, "NLP corridor")))
    return rc;
  {
    // every round in one launch needs all samples / 64 blocks resident together (each waits for
    // the others' rounds; one block per CU by its LDS request): not on a device, or a partition
    // of one, with fewer CUs than blocks — then one launch per round
    const char* e = std::getenv("LLAMPC_NLP_ROUND_LAUNCHES");
    const bool resident = k.samples / 64 <= b->cus;
    p->per_round = !nlp_persistent(k.samples) || !resident || (e && e[0] == '1');
    const char* rt = std::getenv("LLAMPC_NLP_RERUN_TRAJ");
    p->ltraj = nlp_ltraj_fits(k.H, k.samples, k.elite) && !(rt && rt[0] == '1');
    p->ltraj_cor = nlp_corridor_ltraj_fits(k.H, k.samples, k.elite) && !(rt && rt[0] == '1');
  }
  if (hipDeviceSynchronize() != hipSuccess)
    return fail(LLAMPC_E_HIP, "NLP solver upload failed");
  *out = p.release();
  return LLAMPC_OK;
}

int llampc_nlp_set_track(llampc_nlp* p, const double* centre, const double* theta, int32_t n, double track_length,
                         double track_width) {
  if (!p || !centre || !theta) return fail(LLAMPC_E_ARG, "NULL argument");
  char why[128];
  if (track_tables_invalid(centre, theta, n, track_length, track_width, why, sizeof why)) return fail(LLAMPC_E_ARG, "%s", why);
  std::lock_guard<std::mutex> lp(p->mu);
  llampc_bank* b = p->b;
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding on the bank");
  DeviceGuard g(b->device);
  HIP_TRY(hipStreamSynchronize(b->stream));      // no launch reads the tables being replaced
  p->tr_n = 0;
  if (int rc = p->d_track.reserve(3 * (size_t)n, 0, "track tables")) return rc;
  std::vector<double> h(3 * (size_t)n);
  std::memcpy(h.data(), centre, 2 * (size_t)n * sizeof(double));
  std::memcpy(h.data() + 2 * (size_t)n, theta, (size_t)n * sizeof(double));
  HIP_TRY(hipMemcpy(p->d_track.get(), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  p->tr_n = n;
  p->tr_L = track_length;
  p->tr_width = track_width;
  return LLAMPC_OK;
}

}  // extern "C"

// What the device corridor needs before anything is launched (the caller holds p->mu): a track, a
// finite path [2][H+1] and a margin that leaves a corridor.
static int track_corridor_args(const llampc_nlp* p, const double* path, double margin) {
  if (!p->tr_n) return fail(LLAMPC_E_STATE, "no track set: call llampc_nlp_set_track first");
  for (int i = 0; i < 2 * (p->cfg.H + 1); ++i)
    if (!std::isfinite(path[i])) return fail(LLAMPC_E_ARG, "path: entry %d is not finite", i);
  if (!std::isfinite(margin) || !(p->tr_width / 2 - margin > 0))
    return fail(LLAMPC_E_ARG, "margin %g leaves no corridor (track width %g)", margin, p->tr_width);
  return LLAMPC_OK;
}

// Enqueues track_corridor_kernel on s: the half-planes along `path` into the solver's pinned
// buffer (hp [H][6], then theta [H] from 6 HMAX on), which starts as NaN so that a row the kernel
// did not write fails corridor_invalid afterwards.
static int enqueue_track_corridor(llampc_nlp* p, const double* path, double margin, hipStream_t s) {
  const int H = p->cfg.H;
  const size_t n = (size_t)p->tr_n;
  CorridorPath cp{};
  std::memcpy(cp.v, path, 2 * (size_t)(H + 1) * sizeof(double));
  for (int i = 0; i < 6 * H; ++i) p->hp.get()[i] = __builtin_nan("");
  for (int i = 0; i < H; ++i) p->hp.get()[6 * LLAMPC_HMAX + i] = __builtin_nan("");
  const double* d = p->d_track.get();
  const TrackK t{d, d + n, d + 2 * n, p->tr_n, 0, p->tr_L};
  TimedLaunch tl(p->b, 1, s);              // llampc_bank_timing's kernel 1: the corridor kernel alone
  HIP_TRY(launch_track_corridor(t, cp, H, p->tr_width / 2 - margin, p->hp.dev(), p->hp.dev() + 6 * LLAMPC_HMAX, s));
  p->b->launches++;
  return LLAMPC_OK;
}

// One solve: the unconstrained search (hp and path null: llampc_nlp_solve), the corridor's with the
// caller's half-planes (hp [H][6] and the weight, checked by the caller: llampc_nlp_solve_corridor)
// or with the track's along `path` [2][H+1], built on the device ahead of the search
// (llampc_nlp_solve_track; hp_out [H][6] or null: what the kernel built).
static int nlp_solve(llampc_nlp* p, const double* x0, const double* xref, const double* uprev, const double* base,
                     int32_t has_hold, const double* hp, double weight, double* umpc, double* fval, double* xmpc,
                     double* max_slack, const double* path = nullptr, double margin = 0.0, double* hp_out = nullptr) {
  std::lock_guard<std::mutex> lp(p->mu);
  llampc_bank* b = p->b;
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding on the bank");
  DeviceGuard g(b->device);
  const llampc_nlp_cfg& k = p->cfg;
  const int H = k.H;
  hipStream_t s = b->stream;
  NlpCorridor cor{};
  const bool corridor = hp || path;
  if (corridor) {
    if (nlp_corridor_lds_bytes(H, k.samples, k.elite) > 160 * 1024)
      return fail(LLAMPC_E_ARG, "H x elite too large for LDS with a corridor");
    cor.hp = p->hp.dev();
    cor.weight = weight;
  }
  if (hp) std::memcpy(p->hp.get(), hp, 6 * (size_t)H * sizeof(double));
  if (path) {
    if (int rc = track_corridor_args(p, path, margin)) return rc;
    if (int rc = enqueue_track_corridor(p, path, margin, s)) return rc;
  }
  auto launch = [&](const NlpLaunch& a, const NlpInline& pk) {
    return corridor ? launch_nlp_corridor(a, pk, cor, s) : launch_nlp(a, pk, s);
  };
  // the launch's inputs (NlpInline): x0, xref, the first mean (base or uprev held); the first
  // std is sigma0, the best so far starts at +inf (the kernel's round 0)
  NlpInline pk;
  std::memcpy(pk.v, x0, 6 * sizeof(double));
  std::memcpy(pk.v + 6, xref, 2 * (size_t)(H + 1) * sizeof(double));
  double* m0 = pk.v + 6 + 2 * (H + 1);
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < 2; ++j) m0[2 * i + j] = base ? base[2 * i + j] : uprev[j];
  NlpLaunch a{};
  nlp_launch_cfg(a, k, b->veh, b->d_params.get(), 1);
  a.st = p->d_st.get();
  a.list_tag = reinterpret_cast<uint64_t*>(p->d_cost.get());
  a.cand = p->d_cost.get() + 6 * (size_t)k.samples;
  a.res = p->host.rec.dev();
  a.host_tag = p->host.tag.dev();
  a.host_seq = p->calls + 1;
  a.ms_tag = p->d_ms_tag.get();
  a.ltraj = corridor ? p->ltraj_cor : p->ltraj;
  a.seed = k.seed;
  a.call = p->calls;
  a.up0 = uprev[0];
  a.up1 = uprev[1];
  a.has_hold = has_hold;
  if (p->per_round) {
    a.rounds = 1;
    for (int it = 0; it < k.iters; ++it) {
      a.it = it;
      TimedLaunch tl(b, 0, s);           // llampc_bank_timing on the solver's bank: per round
      HIP_TRY(launch(a, pk));
    }
  } else {                              // every round in one launch (nlp.hpp nlp_persistent)
    a.it = 0;
    a.rounds = k.iters;
    TimedLaunch tl(b, 0, s);             // llampc_bank_timing on the solver's bank: per solve
    HIP_TRY(launch(a, pk));
  }
  // the last round's completion writes the result into pinned memory and then the tag
  const uint64_t want = p->calls + 1;
  const int rc = spin_for_tag(p->host.tag.get(), want, [&]() -> int {
    HIP_TRY(hipStreamSynchronize(s));
    return LLAMPC_OK;
  });
  if (rc == kSpinTimeout) {
    // the launch has ended (its blocks give up a round wait after kNlpRoundWait): the next
    // solve must not meet this one's state — a new call number, so none of this solve's
    // tagged words (lists, mean / std) matches a later round's tag
    p->calls++;
    return fail(LLAMPC_E_DEVICE, "NLP solve %llu: completion tag never arrived", (unsigned long long)want);
  }
  if (rc) return rc;
  p->calls++;
  b->launches += p->per_round ? k.iters : 1;
  const NlpResult* r = const_cast<const NlpResult*>(p->host.rec.get());
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < 2; ++j) umpc[2 * i + j] = r->best_u[i][j];
  if (fval) *fval = r->best_j;
  if (xmpc) std::memcpy(xmpc, &r->traj[0][0], 6 * (size_t)(H + 1) * sizeof(double));
  if (hp && max_slack) *max_slack = corridor_max_slack(hp, &r->traj[0][0], H);
  if (path) {
    // the corridor kernel ended before the search began, whose completion tag has arrived
    double built[6 * LLAMPC_HMAX];
    std::memcpy(built, p->hp.get(), 6 * (size_t)H * sizeof(double));
    if (hp_out) std::memcpy(hp_out, built, 6 * (size_t)H * sizeof(double));
    if (const char* why = corridor_invalid(built, H, weight))
      return fail(LLAMPC_E_DEVICE, "the device-built corridor: %s", why);
    if (max_slack) *max_slack = corridor_max_slack(built, &r->traj[0][0], H);
  }
  if (r->best_it < 0) return fail(LLAMPC_E_DEVICE, "no finite objective in %d rounds of %d samples", k.iters, k.samples);
  return LLAMPC_OK;
}

extern "C" {

int llampc_nlp_solve(llampc_nlp* p, const double* x0, const double* xref, const double* uprev, const double* base,
                     int32_t has_hold, double* umpc, double* fval, double* xmpc) {
  if (!p || !x0 || !xref || !uprev || !umpc) return fail(LLAMPC_E_ARG, "NULL argument");
  return nlp_solve(p, x0, xref, uprev, base, has_hold, nullptr, 0.0, umpc, fval, xmpc, nullptr);
}

int llampc_nlp_solve_corridor(llampc_nlp* p, const double* x0, const double* xref, const double* uprev,
                              const double* base, int32_t has_hold, const double* hp, double weight, double* umpc,
                              double* fval, double* xmpc, double* max_slack) {
  if (!p || !x0 || !xref || !uprev || !umpc) return fail(LLAMPC_E_ARG, "NULL argument");
  if (!hp) return fail(LLAMPC_E_ARG, "hp is NULL (llampc_nlp_solve is the unconstrained solve)");
  if (const char* why = corridor_invalid(hp, p->cfg.H, weight)) return fail(LLAMPC_E_ARG, "corridor: %s", why);
  return nlp_solve(p, x0, xref, uprev, base, has_hold, hp, weight, umpc, fval, xmpc, max_slack);
}

int llampc_nlp_solve_track(llampc_nlp* p, const double* x0, const double* xref, const double* uprev,
                           const double* base, int32_t has_hold, const double* path, double margin, double weight,
                           double* umpc, double* fval, double* xmpc, double* max_slack, double* hp_out) {
  if (!p || !x0 || !xref || !uprev || !umpc) return fail(LLAMPC_E_ARG, "NULL argument");
  if (!path) return fail(LLAMPC_E_ARG, "path is NULL");
  if (!(weight >= 0) || !std::isfinite(weight)) return fail(LLAMPC_E_ARG, "corridor: weight must be finite and >= 0");
  return nlp_solve(p, x0, xref, uprev, base, has_hold, nullptr, weight, umpc, fval, xmpc, max_slack, path, margin,
                   hp_out);
}

int llampc_nlp_track_corridor(llampc_nlp* p, const double* path, double margin, double* hp, double* theta) {
  if (!p || !path || !hp) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lp(p->mu);
  llampc_bank* b = p->b;
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding on the bank");
  DeviceGuard g(b->device);
  const int H = p->cfg.H;
  if (int rc = track_corridor_args(p, path, margin)) return rc;
  if (int rc = enqueue_track_corridor(p, path, margin, b->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(b->stream));
  std::memcpy(hp, p->hp.get(), 6 * (size_t)H * sizeof(double));
  if (theta) std::memcpy(theta, p->hp.get() + 6 * LLAMPC_HMAX, (size_t)H * sizeof(double));
  if (const char* why = corridor_invalid(hp, H, 0.0)) return fail(LLAMPC_E_DEVICE, "the device-built corridor: %s", why);
  return LLAMPC_OK;
}

}  // extern "C"

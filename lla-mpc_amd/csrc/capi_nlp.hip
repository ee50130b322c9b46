// capi_nlp.hip — the setupNLP.solve drop-in's host side (llampc_nlp_*, include/llampc.h;
// nlp.hip): CEM iterations enqueued back to back on the bank's stream, the Euler trajectory of
// the best sequence, the result through pinned host memory.  The corridor solve
// (llampc_nlp_solve_corridor) is the same solve with the half-planes handed over in a pinned mapped
// buffer and the largest slack of the returned trajectory computed here on the host.  With a track
// set (llampc_nlp_set_track: the centre line's tables, uploaded once) llampc_nlp_solve_track builds
// those half-planes on the device instead: track_corridor_kernel (kernels.hip, corridor_dev.hpp)
// writes them into the same buffer, enqueued ahead of the corridor solve on the same stream with no
// host synchronisation between the two; llampc_nlp_track_corridor is that kernel alone.  The packing,
// the launch arguments, the unpacking and the refusals' words are capi_host.hpp's (pure).
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
  NlpLtraj ltraj{};                      // the last round keeps its states in LDS (NlpLaunch.ltraj)
  MappedRecord<NlpResult> host;          // the last round writes the result, then the solve's number
  Mapped<double> hp;                     // the corridor solve's half-planes [HMAX][6] (NlpCorridor.hp):
                                         // pinned and mapped, written by the host before the launch
                                         // or by track_corridor_kernel ahead of it, read once per
                                         // block and launch (no H2D copy); then that kernel's
                                         // theta [HMAX]
  TrackTables track;                     // llampc_nlp_set_track
  uint64_t calls = 0;
  std::mutex mu;
};

int nlp_check_cfg(const llampc_nlp_cfg& k) {
  char buf[96];
  const char* why = nlp_cfg_invalid(k, buf, sizeof buf);
  return why ? fail(LLAMPC_E_ARG, "%s", why) : LLAMPC_OK;
}

// What the device corridor needs before anything is launched (the caller holds p->mu): a track, a
// finite path [2][H+1] and a margin that leaves a corridor.
static int track_corridor_args(const llampc_nlp* p, const double* path, double margin) {
  char why[96];
  if (!p->track.n) return fail(LLAMPC_E_STATE, "no track set: call llampc_nlp_set_track first");
  if (path_invalid(path, p->cfg.H, why, sizeof why) || track_margin_refused(margin, p->track.width, why, sizeof why))
    return fail(LLAMPC_E_ARG, "%s", why);
  return LLAMPC_OK;
}

// Enqueues track_corridor_kernel on s: the half-planes along `path` into the solver's pinned
// buffer (hp [H][6], then theta [H] from 6 HMAX on), which starts as NaN so that a row the kernel
// did not write fails corridor_invalid afterwards.
static int enqueue_track_corridor(llampc_nlp* p, const double* path, double margin, hipStream_t s) {
  const int H = p->cfg.H;
  CorridorPath cp{};
  std::memcpy(cp.v, path, 2 * (size_t)(H + 1) * sizeof(double));
  for (int i = 0; i < 6 * H; ++i) p->hp.get()[i] = __builtin_nan("");
  for (int i = 0; i < H; ++i) p->hp.get()[6 * LLAMPC_HMAX + i] = __builtin_nan("");
  TimedLaunch tl(p->b, 1, s);              // llampc_bank_timing's kernel 1: the corridor kernel alone
  HIP_TRY(launch_track_corridor(p->track.view(), cp, H, p->track.width / 2 - margin, p->hp.dev(),
                                p->hp.dev() + 6 * LLAMPC_HMAX, s));
  p->b->launches++;
  return LLAMPC_OK;
}

// One solve's inputs and outputs (fval, xmpc: or null), and the corridor's with B = 1: none
// (llampc_nlp_solve), the caller's half-planes (llampc_nlp_solve_corridor) or the track's, built on
// the device ahead of the search (llampc_nlp_solve_track).
struct NlpSolveArgs {
  const double *x0, *xref, *uprev, *base;
  int32_t has_hold;
  double *umpc, *fval, *xmpc;
  NlpCorridorArgs cor;
};

static int nlp_solve(llampc_nlp* p, const NlpSolveArgs& q) {
  BankIdle idle(p->b, &p->mu);
  if (idle.rc) return idle.rc;
  llampc_bank* b = p->b;
  const llampc_nlp_cfg& k = p->cfg;
  const NlpCorridorArgs& cr = q.cor;
  const bool corridor = cr.mode != NlpCorridorMode::none, track = cr.mode == NlpCorridorMode::track;
  const int H = k.H;
  hipStream_t s = b->stream;
  if (const char* why = corridor ? nlp_corridor_cfg_invalid(k) : nullptr) return fail(LLAMPC_E_ARG, "%s", why);
  if (int rc = track ? track_corridor_args(p, cr.src, cr.margin) : 0) return rc;
  // the launch's inputs (NlpInline); the first std is sigma0, the best so far starts at +inf (round 0)
  NlpInline pk;
  nlp_inline_pack(pk, H, q.x0, q.xref, q.uprev, q.base);
  if (cr.mode == NlpCorridorMode::given) std::memcpy(p->hp.get(), cr.src, 6 * (size_t)H * sizeof(double));
  if (int rc = track ? enqueue_track_corridor(p, cr.src, cr.margin, s) : 0) return rc;
  const NlpCorridor cor{p->hp.dev(), corridor ? cr.weight[0] : 0.0};
  NlpLaunch a{};
  nlp_launch_cfg(a, k, b->veh, b->d_params.get(), 1);
  // the lists, then the sequences, in the one buffer
  nlp_launch_args(a, {p->d_st.get(), reinterpret_cast<uint64_t*>(p->d_cost.get()), p->d_cost.get() + 6 * (size_t)k.samples,
                      p->d_ms_tag.get(), p->host.rec.dev(), p->host.tag.dev(), p->calls, corridor, p->ltraj,
                      p->per_round ? 1 : k.iters});
  a.seed = k.seed;
  a.up0 = q.uprev[0];
  a.up1 = q.uprev[1];
  a.has_hold = q.has_hold;
  // every round in one launch (nlp.hpp nlp_persistent) or one per round, each in llampc_bank_timing's bracket
  for (a.it = 0; a.it < k.iters; a.it += a.rounds) {
    TimedLaunch tl(b, 0, s);
    HIP_TRY(corridor ? launch_nlp_corridor(a, pk, cor, s) : launch_nlp(a, pk, s));
  }
  // the last round's completion writes the result into pinned memory and then the tag
  const uint64_t want = p->calls + 1;
  const int rc = spin_for_tag(p->host.tag.get(), want, [&]() -> int {
    HIP_TRY(hipStreamSynchronize(s));
    return LLAMPC_OK;
  });
  p->calls++;                            // capi_host.hpp: whatever the wait returned
  if (rc == kSpinTimeout)                // the launch has ended: its blocks give up a round wait after kNlpRoundWait
    return fail(LLAMPC_E_DEVICE, "NLP solve %llu: completion tag never arrived", (unsigned long long)want);
  if (rc) return rc;
  b->launches += p->per_round ? k.iters : 1;
  const NlpResult& r = *const_cast<const NlpResult*>(p->host.rec.get());
  const int32_t status = nlp_result_unpack(r, H, q.umpc, q.fval, q.xmpc);
  if (cr.mode == NlpCorridorMode::given && cr.max_slack) *cr.max_slack = corridor_max_slack(cr.src, &r.traj[0][0], H);
  if (track)                             // the corridor kernel ended before the search began, whose tag has arrived
    if (const char* why = nlp_built_corridor(p->hp.get(), H, cr.weight[0], cr.hp_out, true, &r.traj[0][0], cr.max_slack))
      return fail(LLAMPC_E_DEVICE, "the device-built corridor: %s", why);
  if (status != LLAMPC_NLP_OK) return fail(LLAMPC_E_DEVICE, "no finite objective in %d rounds of %d samples", k.iters, k.samples);
  return LLAMPC_OK;
}

extern "C" {

int llampc_nlp_destroy(llampc_nlp* p) { return solver_destroy(p); }

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
  // every round in one launch needs all samples / 64 blocks resident together (each waits for
  // the others' rounds; one block per CU by its LDS request): not on a device, or a partition
  // of one, with fewer CUs than blocks — then one launch per round
  const char* e = std::getenv("LLAMPC_NLP_ROUND_LAUNCHES");
  const bool resident = k.samples / 64 <= b->cus;
  p->per_round = !nlp_persistent(k.samples) || !resident || (e && e[0] == '1');
  p->ltraj = nlp_create_ltraj(k);
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
  BankIdle idle(p->b, &p->mu);
  if (idle.rc) return idle.rc;
  return p->track.upload(p->b->stream, centre, theta, n, track_length, track_width);
}

int llampc_nlp_solve(llampc_nlp* p, const double* x0, const double* xref, const double* uprev, const double* base,
                     int32_t has_hold, double* umpc, double* fval, double* xmpc) {
  if (!p || !x0 || !xref || !uprev || !umpc) return fail(LLAMPC_E_ARG, "NULL argument");
  return nlp_solve(p, {x0, xref, uprev, base, has_hold, umpc, fval, xmpc, {}});
}

int llampc_nlp_solve_corridor(llampc_nlp* p, const double* x0, const double* xref, const double* uprev,
                              const double* base, int32_t has_hold, const double* hp, double weight, double* umpc,
                              double* fval, double* xmpc, double* max_slack) {
  if (!p || !x0 || !xref || !uprev || !umpc) return fail(LLAMPC_E_ARG, "NULL argument");
  if (!hp) return fail(LLAMPC_E_ARG, "hp is NULL (llampc_nlp_solve is the unconstrained solve)");
  if (const char* why = corridor_invalid(hp, p->cfg.H, weight)) return fail(LLAMPC_E_ARG, "corridor: %s", why);
  const NlpCorridorArgs cr{NlpCorridorMode::given, hp, &weight, max_slack};
  return nlp_solve(p, {x0, xref, uprev, base, has_hold, umpc, fval, xmpc, cr});
}

int llampc_nlp_solve_track(llampc_nlp* p, const double* x0, const double* xref, const double* uprev,
                           const double* base, int32_t has_hold, const double* path, double margin, double weight,
                           double* umpc, double* fval, double* xmpc, double* max_slack, double* hp_out) {
  if (!p || !x0 || !xref || !uprev || !umpc) return fail(LLAMPC_E_ARG, "NULL argument");
  if (!path) return fail(LLAMPC_E_ARG, "path is NULL");
  if (!(weight >= 0) || !std::isfinite(weight)) return fail(LLAMPC_E_ARG, "corridor: weight must be finite and >= 0");
  const NlpCorridorArgs cr{NlpCorridorMode::track, path, &weight, max_slack, margin, hp_out};
  return nlp_solve(p, {x0, xref, uprev, base, has_hold, umpc, fval, xmpc, cr});
}

int llampc_nlp_track_corridor(llampc_nlp* p, const double* path, double margin, double* hp, double* theta) {
  if (!p || !path || !hp) return fail(LLAMPC_E_ARG, "NULL argument");
  BankIdle idle(p->b, &p->mu);
  if (idle.rc) return idle.rc;
  const int H = p->cfg.H;
  hipStream_t s = p->b->stream;
  if (int rc = track_corridor_args(p, path, margin)) return rc;
  if (int rc = enqueue_track_corridor(p, path, margin, s)) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  if (theta) std::memcpy(theta, p->hp.get() + 6 * LLAMPC_HMAX, (size_t)H * sizeof(double));
  if (const char* why = nlp_built_corridor(p->hp.get(), H, 0.0, hp, false, nullptr, nullptr))
    return fail(LLAMPC_E_DEVICE, "the device-built corridor: %s", why);
  return LLAMPC_OK;
}

}  // extern "C"

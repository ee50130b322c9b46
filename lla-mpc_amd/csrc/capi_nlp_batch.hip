// capi_nlp_batch.hip — the batched setupNLP.solve's host side (llampc_nlp_batch_*,
// include/llampc.h; nlp_batch.hip): one solver bound to a whole bank, B problems per call in one
// launch on the bank's stream.  The problems' inputs go into a pinned mapped buffer (a record
// each, capi_host.hpp nlp_batch_layout) that the blocks read once; every problem's last round
// writes its own result and then its own tag into pinned host memory, and the host waits for the
// B tags with one bound.  Locking, the armed-launch cancel, the async refusal and the timing
// bracket are llampc_nlp_solve's (capi_nlp.hip).
//
// The corridor solves (llampc_nlp_batch_solve_corridor, llampc_nlp_batch_solve_track) are the same
// call (nlp_batch_run below: one statement of the locking, the launch bracket, the B-tag wait and
// the call number) with nlp_batch_corr.hip's kernel: every problem's half-planes and weight in a
// pinned mapped buffer of their own (capi_host.hpp nlp_batch_cor_layout), written by the host, or,
// with a track set (llampc_nlp_batch_set_track), by track_corridor_batch_kernel (corridor_batch.hip)
// along the problems' paths, enqueued ahead of the search on the same stream with no host
// synchronisation between the two; llampc_nlp_batch_track_corridor is that kernel alone.  One track
// per solver.  The largest slack of each returned trajectory is computed here on the host.
#include "capi_common.hpp"

using namespace llampc;

struct __attribute__((visibility("hidden"))) llampc_nlp_batch {
  llampc_bank* b = nullptr;              // borrowed
  llampc_nlp_cfg cfg{};
  int32_t max_batch = 0;
  NlpBatchLayout lay{};
  DevBuf<NlpState> d_st;                 // [max_batch]
  DevBuf<uint64_t> d_list;               // [max_batch][2][3][samples] tagged list words
  DevBuf<double> d_cand;                 // [max_batch][2][samples][H][2]
  DevBuf<uint64_t> d_ms_tag;             // [max_batch][2][4 HMAX]
  Mapped<uint64_t> in;                   // [max_batch][rec_words] the problems' records
  Mapped<NlpResult> res;                 // [max_batch]
  Mapped<uint64_t> tag;                  // [max_batch][tag_words]: word 0 the problem's tag
  NlpLtraj ltraj{};                      // as llampc_nlp
  NlpBatchCorLayout cl{};
  Mapped<double> cor;                    // [max_batch][cor_doubles]: hp | theta | weight per problem
  Mapped<double> path;                   // [max_batch][path_doubles]: the device builder's paths
  TrackTables track;                     // llampc_nlp_batch_set_track
  uint64_t calls = 0;                    // one solve number per call, every problem's
  std::mutex mu;
};

namespace {

// What the device corridor needs before anything is launched (the caller holds p->mu): a track, finite
// paths and a margin that leaves a corridor (llampc_nlp_solve_track's checks, per problem).
int batch_track_args(const llampc_nlp_batch* p, int32_t B, const double* path, double margin) {
  char why[96];
  if (!p->track.n) return fail(LLAMPC_E_STATE, "no track set: call llampc_nlp_batch_set_track first");
  if (nlp_batch_paths_invalid(B, p->cfg.H, path, why, sizeof why) || track_margin_refused(margin, p->track.width, why, sizeof why))
    return fail(LLAMPC_E_ARG, "%s", why);
  return LLAMPC_OK;
}

// Enqueues track_corridor_batch_kernel on s: the half-planes along the B paths into the problems'
// parts of the corridor buffer, which start as NaN (nlp_batch_cor_pack) so that a row the kernel did
// not write fails corridor_invalid afterwards.  weight: [B] or null (the builder alone).
int enqueue_batch_track_corridor(llampc_nlp_batch* p, int32_t B, const double* path, double margin,
                                 const double* weight, hipStream_t s) {
  const int H = p->cfg.H;
  const NlpBatchCorLayout& c = p->cl;
  for (int32_t q = 0; q < B; ++q) {
    std::memcpy(p->path.get() + q * c.path_doubles, path + 2 * (size_t)(H + 1) * q, 2 * (size_t)(H + 1) * sizeof(double));
    nlp_batch_cor_pack(c, H, p->cor.get() + q * c.cor_doubles, nullptr, weight ? weight[q] : 0.0);
  }
  TimedLaunch tl(p->b, 1, s);              // llampc_bank_timing's kernel 1: the corridor kernel alone
  HIP_TRY(launch_track_corridor_batch(p->track.view(), p->path.dev(), (uint32_t)c.path_doubles, B, H,
                                      p->track.width / 2 - margin, p->cor.dev(), (uint32_t)c.cor_doubles,
                                      (uint32_t)c.theta_off, s));
  p->b->launches++;
  return LLAMPC_OK;
}

// One batched solve's inputs and outputs, [B] of llampc_nlp_solve's each, and the corridor's.
struct NlpBatchArgs {
  int32_t B;
  const int64_t* model_idx;
  const uint64_t* seed;
  const double *x0, *xref, *uprev, *base;
  const int32_t* has_hold;
  double *umpc, *fval, *xmpc;
  int32_t* status;
  NlpCorridorArgs cor;
};

int nlp_batch_run(llampc_nlp_batch* p, const NlpBatchArgs& q) {
  std::lock_guard<std::mutex> lp(p->mu);
  llampc_bank* b = p->b;
  const int32_t B = q.B;
  if (const char* why = nlp_batch_args_invalid(B, p->max_batch, q.model_idx, b->n, q.x0, q.xref, q.uprev, q.has_hold, q.umpc,
                                               q.fval, q.xmpc, q.status))
    return fail(LLAMPC_E_ARG, "NLP batch solve: %s (B=%d, max_batch=%d, n=%lld)", why, B, p->max_batch, (long long)b->n);
  const llampc_nlp_cfg& k = p->cfg;
  const NlpCorridorArgs& cr = q.cor;
  const bool corridor = cr.mode != NlpCorridorMode::none, track = cr.mode == NlpCorridorMode::track;
  if (corridor) {
    char why[160];
    if (!cr.max_slack) return fail(LLAMPC_E_ARG, "NLP batch solve: max_slack is NULL");
    if (nlp_batch_corridor_invalid(B, k.H, track ? nullptr : cr.src, cr.weight, why, sizeof why))
      return fail(LLAMPC_E_ARG, "NLP batch corridor: %s", why);
    if (const char* lds = nlp_corridor_cfg_invalid(k)) return fail(LLAMPC_E_ARG, "%s", lds);
  }
  BankIdle idle(b);
  if (idle.rc) return idle.rc;
  const NlpBatchLayout& l = p->lay;
  const NlpBatchCorLayout& c = p->cl;
  const size_t H = (size_t)k.H;
  hipStream_t s = b->stream;
  // all B x nl blocks resident at once: checked at create for max_batch, and B <= max_batch
  if ((int64_t)B * (k.samples / 64) > b->cus) return fail(LLAMPC_E_ARG, "NLP batch solve: B x samples / 64 exceeds the CUs");
  if (int rc = track ? batch_track_args(p, B, cr.src, cr.margin) : 0) return rc;
  for (int32_t i = 0; i < B; ++i) {
    const int32_t hold = q.has_hold[i] != 0;
    nlp_batch_pack(l, k.H, p->in.get() + i * l.rec_words, q.x0 + 6 * i, q.xref + 2 * (H + 1) * i, q.uprev + 2 * i,
                   q.base && hold ? q.base + 2 * H * i : nullptr, q.seed ? q.seed[i] : k.seed, q.model_idx[i], hold);
    if (cr.mode == NlpCorridorMode::given)
      nlp_batch_cor_pack(c, k.H, p->cor.get() + i * c.cor_doubles, cr.src + 6 * H * i, cr.weight[i]);
  }
  if (int rc = track ? enqueue_batch_track_corridor(p, B, cr.src, cr.margin, cr.weight, s) : 0) return rc;
  NlpLaunch a{};
  nlp_launch_cfg(a, k, b->veh, b->d_params.get(), b->n);
  // always every round in one launch
  nlp_launch_args(a, {p->d_st.get(), p->d_list.get(), p->d_cand.get(), p->d_ms_tag.get(), p->res.dev(), p->tag.dev(),
                      p->calls, corridor, p->ltraj, k.iters});
  const NlpBatch bt = nlp_batch_arg(l, p->in.dev(), k.samples);
  {
    TimedLaunch tl(b, 0, s);             // llampc_bank_timing on the bank: per batched solve
    HIP_TRY(corridor ? launch_nlp_batch_corridor(a, nlp_batch_cor_arg(bt, c, p->cor.dev()), B, s)
                     : launch_nlp_batch(a, bt, B, s));
  }
  const uint64_t want = p->calls + 1;
  const std::unique_ptr<bool[]> arrived(new bool[B]());
  const int rc = spin_for_tags(p->tag.get(), l.tag_words, B, want, arrived.get(), [&]() -> int {
    HIP_TRY(hipStreamSynchronize(s));
    return LLAMPC_OK;
  });
  p->calls++;                            // capi_host.hpp: whatever the wait returned
  if (rc) return rc;
  b->launches++;
  const NlpResult* r = const_cast<const NlpResult*>(p->res.get());
  for (int32_t i = 0; i < B; ++i)
    q.status[i] = nlp_batch_unpack(r[i], arrived[i], k.H, q.umpc + 2 * H * i, q.fval + i, q.xmpc + 6 * (H + 1) * i);
  // a device-built corridor: the stream has drained past its kernel if any problem's tag arrived; if
  // none did, spin_for_tags' timeout handler synchronised it
  for (int32_t i = 0; corridor && i < B; ++i) {
    const double* traj = &r[i].traj[0][0];
    if (!track) {
      cr.max_slack[i] = nlp_batch_slack(arrived[i], r[i].best_it, cr.src + 6 * H * i, traj, k.H);
    } else if (const char* why = nlp_built_corridor(p->cor.get() + i * c.cor_doubles, k.H, cr.weight[i],
                                                    cr.hp_out ? cr.hp_out + 6 * H * i : nullptr,
                                                    q.status[i] == LLAMPC_NLP_OK, traj, cr.max_slack + i)) {
      return fail(LLAMPC_E_DEVICE, "the device-built corridor of problem %d: %s", i, why);
    }
  }
  return LLAMPC_OK;
}

}  // namespace

extern "C" {

int llampc_nlp_batch_destroy(llampc_nlp_batch* p) { return solver_destroy(p); }

int llampc_nlp_batch_create(llampc_bank* b, const llampc_nlp_cfg* cfg, int32_t max_batch, llampc_nlp_batch** out) {
  if (!out) return fail(LLAMPC_E_ARG, "out is NULL");
  *out = nullptr;
  if (!b || !cfg) return fail(LLAMPC_E_ARG, "NULL argument");
  const llampc_nlp_cfg& k = *cfg;
  if (int rc = nlp_check_cfg(k)) return rc;
  if (const char* why = nlp_batch_create_invalid(b->n, k.samples, max_batch, b->cus))
    return fail(LLAMPC_E_ARG, "NLP batch: %s (n=%lld, max_batch=%d, samples=%d, CUs=%d)", why, (long long)b->n,
                max_batch, k.samples, b->cus);
  DeviceGuard g(b->device);
  Building<llampc_nlp_batch> p(new llampc_nlp_batch(), llampc_nlp_batch_destroy);
  p->b = b;
  p->cfg = k;
  p->max_batch = max_batch;
  p->lay = nlp_batch_layout(k.H, k.samples);
  const NlpBatchLayout& l = p->lay;
  const size_t mb = (size_t)max_batch;
  int rc;
  // tagged words start at tag 0, which no solve uses (nlp_seq of a solve number >= 1)
  if ((rc = p->d_st.zalloc(mb)) || (rc = p->d_list.zalloc(mb * l.list_words)) ||
      (rc = p->d_cand.zalloc(mb * l.cand_doubles)) || (rc = p->d_ms_tag.zalloc(mb * l.ms_words)) ||
      (rc = p->in.alloc(mb * l.rec_words, "NLP batch inputs")) || (rc = p->res.alloc(mb, "NLP batch results")) ||
      (rc = p->tag.alloc(mb * l.tag_words, "NLP batch tags")))
    return rc;
  p->cl = nlp_batch_cor_layout();
  if ((rc = p->cor.alloc(mb * p->cl.cor_doubles, "NLP batch corridors")) ||
      (rc = p->path.alloc(mb * p->cl.path_doubles, "NLP batch corridor paths")))
    return rc;
  p->ltraj = nlp_create_ltraj(k);
  if (hipDeviceSynchronize() != hipSuccess) return fail(LLAMPC_E_HIP, "NLP batch solver upload failed");
  *out = p.release();
  return LLAMPC_OK;
}

int llampc_nlp_batch_info(const llampc_nlp_batch* p, int32_t* max_batch, int32_t* cus) {
  if (!p) return fail(LLAMPC_E_ARG, "NULL argument");
  if (max_batch) *max_batch = p->max_batch;
  if (cus) *cus = p->b->cus;
  return LLAMPC_OK;
}

int llampc_nlp_batch_solve(llampc_nlp_batch* p, int32_t B, const int64_t* model_idx, const uint64_t* seed,
                           const double* x0, const double* xref, const double* uprev, const double* base,
                           const int32_t* has_hold, double* umpc, double* fval, double* xmpc, int32_t* status) {
  if (!p) return fail(LLAMPC_E_ARG, "NULL argument");
  return nlp_batch_run(p, {B, model_idx, seed, x0, xref, uprev, base, has_hold, umpc, fval, xmpc, status, {}});
}

int llampc_nlp_batch_solve_corridor(llampc_nlp_batch* p, int32_t B, const int64_t* model_idx, const uint64_t* seed,
                                    const double* x0, const double* xref, const double* uprev, const double* base,
                                    const int32_t* has_hold, const double* hp, const double* weight, double* umpc,
                                    double* fval, double* xmpc, int32_t* status, double* max_slack) {
  if (!p) return fail(LLAMPC_E_ARG, "NULL argument");
  if (!hp) return fail(LLAMPC_E_ARG, "hp is NULL (llampc_nlp_batch_solve is the unconstrained solve)");
  const NlpCorridorArgs cr{NlpCorridorMode::given, hp, weight, max_slack};
  return nlp_batch_run(p, {B, model_idx, seed, x0, xref, uprev, base, has_hold, umpc, fval, xmpc, status, cr});
}

int llampc_nlp_batch_set_track(llampc_nlp_batch* p, const double* centre, const double* theta, int32_t n,
                               double track_length, double track_width) {
  if (!p || !centre || !theta) return fail(LLAMPC_E_ARG, "NULL argument");
  char why[128];
  if (track_tables_invalid(centre, theta, n, track_length, track_width, why, sizeof why)) return fail(LLAMPC_E_ARG, "%s", why);
  BankIdle idle(p->b, &p->mu);
  if (idle.rc) return idle.rc;
  return p->track.upload(p->b->stream, centre, theta, n, track_length, track_width);
}

int llampc_nlp_batch_solve_track(llampc_nlp_batch* p, int32_t B, const int64_t* model_idx, const uint64_t* seed,
                                 const double* x0, const double* xref, const double* uprev, const double* base,
                                 const int32_t* has_hold, const double* path, double margin, const double* weight,
                                 double* umpc, double* fval, double* xmpc, int32_t* status, double* max_slack,
                                 double* hp_out) {
  if (!p) return fail(LLAMPC_E_ARG, "NULL argument");
  if (!path) return fail(LLAMPC_E_ARG, "path is NULL");
  const NlpCorridorArgs cr{NlpCorridorMode::track, path, weight, max_slack, margin, hp_out};
  return nlp_batch_run(p, {B, model_idx, seed, x0, xref, uprev, base, has_hold, umpc, fval, xmpc, status, cr});
}

int llampc_nlp_batch_track_corridor(llampc_nlp_batch* p, int32_t B, const double* path, double margin, double* hp,
                                    double* theta) {
  if (!p || !path || !hp) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lp(p->mu);
  if (B < 1 || B > p->max_batch) return fail(LLAMPC_E_ARG, "B=%d outside [1, max_batch=%d]", B, p->max_batch);
  BankIdle idle(p->b);
  if (idle.rc) return idle.rc;
  const size_t H = (size_t)p->cfg.H;
  const NlpBatchCorLayout& c = p->cl;
  hipStream_t s = p->b->stream;
  if (int rc = batch_track_args(p, B, path, margin)) return rc;
  if (int rc = enqueue_batch_track_corridor(p, B, path, margin, nullptr, s)) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  for (int32_t q = 0; q < B; ++q) {
    const double* part = p->cor.get() + q * c.cor_doubles;
    if (theta) std::memcpy(theta + H * q, part + c.theta_off, H * sizeof(double));
    if (const char* why = nlp_built_corridor(part, (int32_t)H, 0.0, hp + 6 * H * q, false, nullptr, nullptr))
      return fail(LLAMPC_E_DEVICE, "the device-built corridor of problem %d: %s", q, why);
  }
  return LLAMPC_OK;
}

}  // extern "C"

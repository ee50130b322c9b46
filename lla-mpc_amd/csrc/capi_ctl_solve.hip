// capi_ctl_solve.hip — the fused control step's host side (llampc_ctl_solver_*, llampc_ctl_step,
// include/llampc.h; ctl_solve.hpp): the controller tick's launch and the NLP search of the model it
// selects as ONE chain on the bank's stream — snapshot, the tick (llampc_ctl_tick_async's prepare,
// launch and commit: capi_ctl.hpp), build, the batched search with B = 1 (nlp_batch.hip, unmodified;
// its record, result and tag in device memory, its parameter table the build kernel's p6 [6][1]),
// commit — and then the tick's wait (llampc_ctl_wait) and one bounded wait for the commit's tag.  The
// solver borrows the controller; what it rules out is refused there while it is attached
// (ctl_solve_refuse.hpp ctl_solver_blocks).
#include <optional>

#include "capi_ctl.hpp"
#include "ctl_solve.hpp"

using namespace llampc;

static_assert(sizeof(llampc_ctl_solve_out) == 16 * LLAMPC_HMAX + 48 * (LLAMPC_HMAX + 1) + 8 + 16 + 8 + 8,
              "llampc_ctl_solve_out layout (llampc/_native.py CtlSolveOut)");

struct __attribute__((visibility("hidden"))) llampc_ctl_solver {
  llampc_ctl* c = nullptr;               // borrowed, and through it the bank
  llampc_bank* b = nullptr;              //   (solver_destroy's name for it)
  llampc_nlp_cfg cfg{};
  NlpBatchLayout lay{};
  DevBuf<NlpState> d_st;                 // the search's buffers, one problem's (capi_nlp_batch.hip)
  DevBuf<uint64_t> d_list;
  DevBuf<double> d_cand;
  DevBuf<uint64_t> d_ms_tag;
  DevBuf<uint64_t> d_rec;                // [rec_words] the problem's record: written by the build kernel
  DevBuf<NlpResult> d_res;               // the search's result and tag line: read by the commit kernel
  DevBuf<uint64_t> d_tag;
  DevBuf<double> d_p6;                   // [6][1] the search's parameter table
  DevBuf<double> d_uprev;                // [2] the snapshot
  MappedRecord<llampc_ctl_solve_out> host;
  NlpLtraj ltraj{};
  uint64_t steps = 0;                    // steps run: the search's call word, the tags' sequence
  std::mutex mu;
};

namespace {
// What ctl_tick_launched runs between the tick's prepare and its launch: the prepared tick's warm flag
// into the glue kernels' arguments, the timing bracket opened, the snapshot enqueued.
struct StepBefore {
  llampc_ctl_solver* s;
  CtlSolveBuild* bd;
  CtlSolveCommit* cm;
  std::optional<TimedLaunch>* tl;
};
int step_before(void* arg, int32_t warm) {
  const StepBefore& q = *static_cast<StepBefore*>(arg);
  q.bd->warm = q.cm->warm = warm;
  q.tl->emplace(q.s->b, 0, q.s->b->stream);
  HIP_TRY(launch_ctl_solve_snapshot(q.s->c->d_st.get(), q.s->d_uprev.get(), q.s->b->stream));
  return LLAMPC_OK;
}
}  // namespace

extern "C" {

int llampc_ctl_solver_destroy(llampc_ctl_solver* s) {
  if (!s) return LLAMPC_OK;
  if (llampc_ctl* c = s->c) {
    std::lock_guard<std::mutex> lc(c->mu);
    DeviceGuard g(s->b->device);
    if (s->b->stream) (void)hipStreamSynchronize(s->b->stream);
    c->solver_attached = false;
    if (c->dbg_by_solver) {              // no tick in flight reads it: the stream has drained
      c->d_dbg.reset();
      c->dbg_by_solver = false;
    }
  }
  return solver_destroy(s);
}

int llampc_ctl_solver_create(llampc_ctl* c, const llampc_nlp_cfg* cfg, llampc_ctl_solver** out) {
  if (out) *out = nullptr;
  if (!c || !cfg || !out) return fail(LLAMPC_E_ARG, "NULL argument");
  const llampc_nlp_cfg& k = *cfg;
  if (int rc = nlp_check_cfg(k)) return rc;
  std::lock_guard<std::mutex> lc(c->mu);
  llampc_bank* b = c->b;
  if (const char* why = ctl_solver_state_refused({c->solver_attached, c->pending, c->prelaunch || c->armed, c->mb != nullptr,
                                                  c->xg_world != 0, c->cor_w}))
    return fail(LLAMPC_E_STATE, "%s", why);
  if (const char* why = ctl_solver_cfg_refused(k.H, k.Ts, k.samples, c->cfg.H, c->cfg.Ts, b->cus))
    return fail(LLAMPC_E_ARG, "fused step: %s (H=%d Ts=%g samples=%d; controller H=%d Ts=%g, CUs=%d)", why, k.H, k.Ts,
                k.samples, c->cfg.H, c->cfg.Ts, b->cus);
  BankIdle idle(b);
  if (idle.rc) return idle.rc;
  Building<llampc_ctl_solver> s(new llampc_ctl_solver(), llampc_ctl_solver_destroy);
  s->b = b;
  s->cfg = k;
  s->lay = nlp_batch_layout(k.H, k.samples);
  const NlpBatchLayout& l = s->lay;
  int rc;
  // tagged words start at tag 0, which no solve uses (nlp_seq of a solve number >= 1)
  if ((rc = s->d_st.zalloc(1)) || (rc = s->d_list.zalloc(l.list_words)) || (rc = s->d_cand.zalloc(l.cand_doubles)) ||
      (rc = s->d_ms_tag.zalloc(l.ms_words)) || (rc = s->d_rec.zalloc(l.rec_words)) || (rc = s->d_res.zalloc(1)) ||
      (rc = s->d_tag.zalloc(l.tag_words)) || (rc = s->d_p6.zalloc(6)) || (rc = s->d_uprev.zalloc(2)) ||
      (rc = s->host.alloc("fused step record")))
    return rc;
  s->ltraj = nlp_create_ltraj(k);
  // the tick publishes its reference to device memory (CtlLaunch.dbg) for the build kernel
  if (!c->d_dbg) {
    HIP_TRY(hipStreamSynchronize(b->stream));
    if ((rc = c->d_dbg.alloc(2 * (size_t)(c->cfg.H + 1) + 2 * (size_t)c->cfg.C * c->cfg.H))) return rc;
    c->dbg_by_solver = true;
  }
  if (hipDeviceSynchronize() != hipSuccess) {
    if (c->dbg_by_solver) {              // no solver after all: the controller ticks without the copy
      c->d_dbg.reset();
      c->dbg_by_solver = false;
    }
    return fail(LLAMPC_E_HIP, "fused step solver upload failed");
  }
  s->c = c;                              // from here on destroy detaches it
  c->solver_attached = true;
  *out = s.release();
  return LLAMPC_OK;
}

int llampc_ctl_step(llampc_ctl_solver* s, const double* x_t, llampc_ctl_out* out, llampc_ctl_solve_out* sol) {
  if (!s || !x_t || !out || !sol) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> ls(s->mu);
  llampc_ctl* c = s->c;
  llampc_bank* b = s->b;
  const llampc_nlp_cfg& k = s->cfg;
  const uint64_t want = s->steps + 1;
  hipError_t chain = hipSuccess;         // the launches behind the tick's
  {
    std::lock_guard<std::mutex> lc(c->mu);
    if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding: call llampc_ctl_wait");
    // attached: no armed launch, no exchange, no corridor (their setters refuse)
    BankIdle idle(b);
    if (idle.rc) return idle.rc;
    hipStream_t st = b->stream;
    CtlSolveBuild bd{};
    bd.st = c->d_st.get();
    bd.dbg = c->d_dbg.get();
    bd.uprev = s->d_uprev.get();
    bd.rec = s->d_rec.get();
    bd.p6 = s->d_p6.get();
    bd.params = b->d_params.get();
    bd.n = b->n;
    bd.goff = b->goff;
    for (int j = 0; j < 6; ++j) {
      bd.x_t[j] = x_t[j];
      bd.nominal[j] = c->cfg.nominal[j];
    }
    bd.seed = k.seed;
    bd.up_off = (uint32_t)s->lay.up_off;
    bd.H = k.H;
    NlpLaunch a{};
    nlp_launch_cfg(a, k, b->veh, s->d_p6.get(), 1);
    nlp_launch_args(a, {s->d_st.get(), s->d_list.get(), s->d_cand.get(), s->d_ms_tag.get(), s->d_res.get(), s->d_tag.get(),
                        s->steps, false, s->ltraj, k.iters});
    const NlpBatch bt = nlp_batch_arg(s->lay, s->d_rec.get(), k.samples);
    CtlSolveCommit cm{c->d_st.get(), s->d_res.get(),       s->d_tag.get(), want, s->d_uprev.get(),
                      s->host.rec.dev(), s->host.tag.dev(), want,          k.H,  0};
    std::optional<TimedLaunch> tl;         // llampc_bank_timing: the chain as one group
    // the tick's launch exactly as llampc_ctl_tick_async issues it, the snapshot ahead of it
    StepBefore before{s, &bd, &cm, &tl};
    if (int rc = ctl_tick_launched(c, x_t, step_before, &before)) return rc;
    // the tick is enqueued (and counted: ctl_commit): its wait below, whatever follows
    chain = launch_ctl_solve_build(bd, st);
    if (chain == hipSuccess && (chain = launch_nlp_batch(a, bt, 1, st)) == hipSuccess)
      b->launches++;                       // the search's, where it is enqueued, as the tick's is
    if (chain == hipSuccess) chain = launch_ctl_solve_commit(cm, st);
    s->steps++;                            // capi_host.hpp: once enqueued, whatever the waits return
  }
  if (int rc = llampc_ctl_wait(c, out)) return rc;
  if (chain != hipSuccess) return fail(LLAMPC_E_HIP, "fused step: enqueueing the solve failed: %s", hipGetErrorString(chain));
  bool arrived = false;
  const int rc = spin_for_tags(s->host.tag.get(), 8, 1, want, &arrived, [&]() -> int {
    HIP_TRY(hipStreamSynchronize(b->stream));
    return LLAMPC_OK;
  });
  if (rc) return rc;
  if (!arrived) return fail(LLAMPC_E_DEVICE, "fused step %llu: the commit's tag never arrived", (unsigned long long)want);
  std::memcpy(sol, const_cast<const llampc_ctl_solve_out*>(s->host.rec.get()), sizeof *sol);
  return LLAMPC_OK;
}

}  // extern "C"

// capi_nlp_batch.hip — the batched setupNLP.solve's host side (llampc_nlp_batch_*,
// include/llampc.h; nlp_batch.hip): one solver bound to a whole bank, B problems per call in one
// launch on the bank's stream.  The problems' inputs go into a pinned mapped buffer (a record
// each, capi_host.hpp nlp_batch_layout) that the blocks read once; every problem's last round
// writes its own result and then its own tag into pinned host memory, and the host waits for the
// B tags with one bound.  Locking, the armed-launch cancel, the async refusal and the timing
// bracket are llampc_nlp_solve's (capi_nlp.hip).
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
  bool ltraj = false;                    // as llampc_nlp (LLAMPC_NLP_RERUN_TRAJ=1 at create: re-run)
  uint64_t calls = 0;                    // one solve number per call, every problem's
  std::mutex mu;
};

extern "C" {

int llampc_nlp_batch_destroy(llampc_nlp_batch* p) {
  if (!p) return LLAMPC_OK;
  DeviceGuard g(p->b->device);
  if (p->b->stream) (void)hipStreamSynchronize(p->b->stream);
  delete p;
  return LLAMPC_OK;
}

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
  const char* rt = std::getenv("LLAMPC_NLP_RERUN_TRAJ");
  p->ltraj = nlp_ltraj_fits(k.H, k.samples, k.elite) && !(rt && rt[0] == '1');
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
  std::lock_guard<std::mutex> lp(p->mu);
  llampc_bank* b = p->b;
  if (const char* why = nlp_batch_args_invalid(B, p->max_batch, model_idx, b->n, x0, xref, uprev, has_hold, umpc, fval,
                                               xmpc, status))
    return fail(LLAMPC_E_ARG, "NLP batch solve: %s (B=%d, max_batch=%d, n=%lld)", why, B, p->max_batch, (long long)b->n);
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding on the bank");
  DeviceGuard g(b->device);
  const llampc_nlp_cfg& k = p->cfg;
  const NlpBatchLayout& l = p->lay;
  const size_t H = (size_t)k.H;
  hipStream_t s = b->stream;
  // all B x nl blocks resident at once: checked at create for max_batch, and B <= max_batch
  if ((int64_t)B * (k.samples / 64) > b->cus) return fail(LLAMPC_E_ARG, "NLP batch solve: B x samples / 64 exceeds the CUs");
  for (int32_t q = 0; q < B; ++q) {
    const int32_t hold = has_hold[q] != 0;
    nlp_batch_pack(l, k.H, p->in.get() + q * l.rec_words, x0 + 6 * q, xref + 2 * (H + 1) * q, uprev + 2 * q,
                   base && hold ? base + 2 * H * q : nullptr, seed ? seed[q] : k.seed, model_idx[q], hold);
  }
  NlpLaunch a{};
  nlp_launch_cfg(a, k, b->veh, b->d_params.get(), b->n);
  a.st = p->d_st.get();
  a.list_tag = p->d_list.get();
  a.cand = p->d_cand.get();
  a.ms_tag = p->d_ms_tag.get();
  a.res = p->res.dev();
  a.host_tag = p->tag.dev();
  a.host_seq = p->calls + 1;
  a.call = p->calls;
  a.ltraj = p->ltraj;
  a.it = 0;                             // always every round in one launch
  a.rounds = k.iters;
  const NlpBatch bt = nlp_batch_arg(l, p->in.dev(), k.samples);
  {
    TimedLaunch tl(b, 0, s);             // llampc_bank_timing on the bank: per batched solve
    HIP_TRY(launch_nlp_batch(a, bt, B, s));
  }
  const uint64_t want = p->calls + 1;
  const std::unique_ptr<bool[]> arrived(new bool[B]());
  const int rc = spin_for_tags(p->tag.get(), l.tag_words, B, want, arrived.get(), [&]() -> int {
    HIP_TRY(hipStreamSynchronize(s));
    return LLAMPC_OK;
  });
  // a new call number whatever happened: none of this solve's tagged words matches a later round's
  p->calls++;
  if (rc) return rc;
  b->launches++;
  const NlpResult* r = const_cast<const NlpResult*>(p->res.get());
  for (int32_t q = 0; q < B; ++q) {
    const bool ok = arrived[q] && r[q].best_it >= 0;
    status[q] = !arrived[q] ? LLAMPC_NLP_NO_TAG : (ok ? LLAMPC_NLP_OK : LLAMPC_NLP_NO_FINITE);
    for (size_t i = 0; i < 2 * H; ++i) umpc[2 * H * q + i] = ok ? (&r[q].best_u[0][0])[i] : 0.0;
    fval[q] = ok ? r[q].best_j : HUGE_VAL;
    if (arrived[q]) std::memcpy(xmpc + 6 * (H + 1) * q, &r[q].traj[0][0], 6 * (H + 1) * sizeof(double));
    else std::memset(xmpc + 6 * (H + 1) * q, 0, 6 * (H + 1) * sizeof(double));
  }
  return LLAMPC_OK;
}

}  // extern "C"

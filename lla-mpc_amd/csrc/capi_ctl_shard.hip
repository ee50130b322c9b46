// capi_ctl_shard.hip — the sharded controller's transports (llampc_ctl_set_exchange: the peers'
// mailboxes; llampc_ctl_set_gather: RCCL, or the caller carries the records between the two launches
// with llampc_ctl_shard_record / llampc_ctl_resume) and the host restatement of the merge.
#include "capi_ctl.hpp"

using namespace llampc;

// What llampc_ctl_set_exchange and llampc_ctl_set_gather share: the check of n_global ...
static int ctl_check_global(const llampc_bank* b, int64_t n_global) {
  if (n_global < b->goff + b->n || n_global >= (int64_t)0xFFFFFFFFll)
    return fail(LLAMPC_E_ARG, "n_global=%lld: must hold this shard [%lld, %lld) and be < 2^32 - 1", (long long)n_global,
                (long long)b->goff, (long long)(b->goff + b->n));
  return LLAMPC_OK;
}
// ... and (the caller holds c->mu, the bank's device is current) the state's checks (`other`: the
// other transport, if the controller already has it), then the replicated global table uploaded
// into `gp`: the controller itself is not touched beyond cancelling an armed launch.
static int ctl_upload_global(llampc_ctl* c, const char* other, const double* gparams, int64_t n_global,
                             DevBuf<double>& gp) {
  if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding");
  if (c->cor_w > 0) return fail(LLAMPC_E_STATE, "a corridor controller is unsharded (llampc_ctl_set_corridor)");
  if (c->t != 0) return fail(LLAMPC_E_STATE, "set the exchange before the first tick");
  if (other) return fail(LLAMPC_E_STATE, "the controller already exchanges over %s", other);
  ctl_cancel(c);                         // no armed launches with an exchange
  if (int rc = gp.alloc(6 * (size_t)n_global, "global parameter table")) return rc;
  if (hipMemcpy(gp.get(), gparams, 6 * (size_t)n_global * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    return fail(LLAMPC_E_HIP, "global parameter table upload failed");
  return LLAMPC_OK;
}

extern "C" {

int llampc_ctl_set_exchange(llampc_ctl* c, llampc_mailbox* mb, const double* gparams, int64_t n_global) {
  if (!c || !mb || !gparams) return fail(LLAMPC_E_ARG, "NULL argument");
  llampc_bank* b = c->b;
  if (mb->device != b->device) return fail(LLAMPC_E_ARG, "mailbox on device %d, bank on %d", mb->device, b->device);
  if (mb->world > kCtlPxMax) return fail(LLAMPC_E_ARG, "world %d > %d (the exchange's LDS)", mb->world, kCtlPxMax);
  if (int rc = ctl_check_global(b, n_global)) return rc;
  for (int g = 0; g < mb->world; ++g)
    if (!mb->box[g]) return fail(LLAMPC_E_STATE, "mailbox of peer %d not open", g);
  std::lock_guard<std::mutex> lc(c->mu);
  if (const char* why = ctl_solver_blocks(c->solver_attached, CtlSetter::exchange, true)) return fail(LLAMPC_E_STATE, "%s", why);
  DeviceGuard g(b->device);
  DevBuf<double> gp;
  if (int rc = ctl_upload_global(c, c->xg_world ? "a gather transport" : nullptr, gparams, n_global, gp)) return rc;
  c->prelaunch = false;
  c->d_gparams = std::move(gp);
  c->n_global = n_global;
  c->mb = mb;
  return LLAMPC_OK;
}

int32_t llampc_ctl_record_words(int32_t K) { return (K < 1 || K > LLAMPC_KMAX) ? 0 : ctl_rec_words(K); }

int llampc_ctl_set_gather(llampc_ctl* c, int32_t world, int32_t rank, llampc_comm* comm, const double* gparams,
                          int64_t n_global) {
  if (!c || !gparams) return fail(LLAMPC_E_ARG, "NULL argument");
  llampc_bank* b = c->b;
  if (world < 1 || world > kCtlPxMax || rank < 0 || rank >= world)
    return fail(LLAMPC_E_ARG, "world=%d rank=%d (world 1..%d)", world, rank, kCtlPxMax);
  if (comm && (comm->world != world || comm->rank != rank || comm->device != b->device))
    return fail(LLAMPC_E_ARG, "the communicator is rank %d of %d on device %d, the controller rank %d of %d on %d",
                comm->rank, comm->world, comm->device, rank, world, b->device);
  if (int rc = ctl_check_global(b, n_global)) return rc;
  std::lock_guard<std::mutex> lc(c->mu);
  if (const char* why = ctl_solver_blocks(c->solver_attached, CtlSetter::gather, true)) return fail(LLAMPC_E_STATE, "%s", why);
  DeviceGuard g(b->device);
  // everything into locals: a failed call leaves the controller as it was
  DevBuf<double> gp;
  DevBuf<uint64_t> xsend, xgath;
  PinnedBuf<uint64_t> xstage;
  const size_t nw = ctl_rec_words(c->cfg.K), ng = (size_t)kCtlPxMax * nw;
  int rc;
  if ((rc = ctl_upload_global(c, c->mb ? "peer mailboxes" : nullptr, gparams, n_global, gp))) return rc;
  if (!c->d_xsend) {
    if ((rc = xsend.zalloc(nw, "gather record")) || (rc = xgath.zalloc(ng, "gathered records")) ||
        (rc = xstage.alloc(ng, "gather staging")))
      return rc;
    c->d_xsend = std::move(xsend);
    c->d_xgath = std::move(xgath);
    c->h_xstage = std::move(xstage);
  }
  c->prelaunch = false;
  c->d_gparams = std::move(gp);
  c->n_global = n_global;
  c->xg_nw = (int32_t)nw;
  c->xg_world = world;
  c->xg_rank = rank;
  c->xg_comm = comm;
  return LLAMPC_OK;
}

int llampc_ctl_shard_record(llampc_ctl* c, uint64_t* words, int32_t* nw) {
  if (!c || !words || !nw) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lc(c->mu);
  *nw = 0;
  if (!c->xg_wait) return LLAMPC_OK;     // no exchange on this tick (or RCCL carries it)
  DeviceGuard g(c->b->device);
  const size_t bytes = (size_t)c->xg_nw * sizeof(uint64_t);
  HIP_TRY(hipMemcpyAsync(c->h_xstage.get(), c->d_xsend.get(), bytes, hipMemcpyDeviceToHost, c->b->stream));
  HIP_TRY(hipStreamSynchronize(c->b->stream));
  std::memcpy(words, c->h_xstage.get(), bytes);
  c->xg_read = true;
  *nw = c->xg_nw;
  return LLAMPC_OK;
}

int llampc_ctl_resume(llampc_ctl* c, const uint64_t* all_words) {
  if (!c || !all_words) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lc(c->mu);
  if (!c->xg_wait || !c->xg_read)
    return fail(LLAMPC_E_STATE, "no tick awaits its gathered records (llampc_ctl_shard_record first)");
  llampc_bank* b = c->b;
  std::lock_guard<std::mutex> lk(b->mu);
  DeviceGuard g(b->device);
  const size_t bytes = (size_t)c->xg_world * c->xg_nw * sizeof(uint64_t);
  std::memcpy(c->h_xstage.get(), all_words, bytes);
  HIP_TRY(hipMemcpyAsync(c->d_xgath.get(), c->h_xstage.get(), bytes, hipMemcpyHostToDevice, b->stream));
  const CtlPrep& P2 = c->xg_second;      // ctl_gather_split's second launch
  HIP_TRY(launch_ctl(P2.L, P2.lpm, P2.lds, b->stream));
  c->xg_wait = false;
  c->xg_read = false;
  return LLAMPC_OK;
}

int llampc_ctl_merge(const double* vals, const int64_t* gids, int32_t G, int32_t K, int32_t nan_policy,
                     int64_t* topk, double* topk_val, int64_t* best, double* best_val) {
  if (!vals || !gids || !topk || !topk_val || !best || !best_val) return fail(LLAMPC_E_ARG, "NULL argument");
  if (G < 1 || G > kCtlPxMax || K < 1 || K > LLAMPC_KMAX) return fail(LLAMPC_E_ARG, "G=%d (1..%d) K=%d", G, kCtlPxMax, K);
  const int M = G * K;
  std::vector<uint64_t> key(M), id(M);
  for (int e = 0; e < M; ++e) {
    const int g = e / K, j = e - g * K;
    ctl_entry_order(vals[g * (K + 1) + j], gids[g * (K + 1) + j], e, key[e], id[e]);
  }
  for (int k = 0; k < K; ++k) {
    topk[k] = -1;
    topk_val[k] = std::nan("");
  }
  for (int e = 0; e < M; ++e) {
    const int r = ctl_merge_rank([&](int j) { return key[j]; }, [&](int j) { return id[j]; }, M, e);
    if (r < K) {
      const int g = e / K, j = e - g * K;
      const int64_t gid = gids[g * (K + 1) + j];
      topk[r] = gid < 0 ? -1 : gid;
      topk_val[r] = gid < 0 ? std::nan("") : vals[g * (K + 1) + j];
    }
  }
  ctl_merge_argmin([&](int g, double& v, int64_t& i) {
                     v = vals[g * (K + 1) + K];
                     i = gids[g * (K + 1) + K];
                   },
                   G, nan_policy == LLAMPC_NAN_FIRST, *best_val, *best);
  return LLAMPC_OK;
}

}  // extern "C"

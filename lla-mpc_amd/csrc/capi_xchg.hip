// capi_xchg.hip — the sharded tick's exchanges (include/llampc.h): the library's own RCCL
// communicator, the xGMI peer mailboxes and the two exchange entry points.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include "capi_common.hpp"

using namespace llampc;

// ---- RCCL: the library's own communicator (rccl.h) ----------------------------------
// RCCL is resolved at first use, not linked: the librccl.so.1 the process already holds
// (torch's bundled RCCL carries that soname: one RCCL per process, whatever the import order
// of torch and this library), else the system's.  A process that never exchanges over RCCL
// never loads it.
namespace {
struct Rccl {
  decltype(&ncclGetUniqueId) get_id = nullptr;
  decltype(&ncclCommInitRank) init_rank = nullptr;
  decltype(&ncclCommDestroy) destroy = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclGetErrorString) err_str = nullptr;
  bool ok = false;
  std::string why;
};
const Rccl& rccl() {
  static Rccl r = [] {
    Rccl x;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) {
      const char* e = dlerror();
      x.why = e ? e : "librccl.so.1 not found";
      return x;
    }
    x.get_id = reinterpret_cast<decltype(x.get_id)>(dlsym(h, "ncclGetUniqueId"));
    x.init_rank = reinterpret_cast<decltype(x.init_rank)>(dlsym(h, "ncclCommInitRank"));
    x.destroy = reinterpret_cast<decltype(x.destroy)>(dlsym(h, "ncclCommDestroy"));
    x.all_gather = reinterpret_cast<decltype(x.all_gather)>(dlsym(h, "ncclAllGather"));
    x.err_str = reinterpret_cast<decltype(x.err_str)>(dlsym(h, "ncclGetErrorString"));
    x.ok = x.get_id && x.init_rank && x.destroy && x.all_gather && x.err_str;
    if (!x.ok) x.why = "librccl.so.1 lacks an ncclGetUniqueId/ncclCommInitRank/ncclAllGather symbol";
    return x;
  }();
  return r;
}
static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes (llampc_comm_unique_id)");
}  // namespace

#define RCCL_TRY(expr)                                                                         \
  do {                                                                                         \
    const ncclResult_t r_ = (expr);                                                            \
    if (r_ != ncclSuccess) return fail(LLAMPC_E_HIP, "%s failed: %s", #expr, rccl().err_str(r_)); \
  } while (0)

int comm_all_gather(llampc_comm* c, const void* send, void* recv, size_t count, bool words, hipStream_t s) {
  RCCL_TRY(rccl().all_gather(send, recv, count, words ? ncclUint64 : ncclUint8, c->comm, s));
  return LLAMPC_OK;
}

int mailbox_sync(llampc_mailbox* mb) {
  if (mb->box_synced) return LLAMPC_OK;
  HIP_TRY(hipMemcpy(mb->d_box.get(), mb->box, kPeerMax * sizeof(uint64_t*), hipMemcpyHostToDevice));
  mb->box_synced = true;
  return LLAMPC_OK;
}

extern "C" {

int llampc_comm_unique_id(void* id) {
  if (!id) return fail(LLAMPC_E_ARG, "id is NULL");
  if (!rccl().ok) return fail(LLAMPC_E_STATE, "RCCL unavailable: %s", rccl().why.c_str());
  ncclUniqueId u;
  RCCL_TRY(rccl().get_id(&u));
  std::memcpy(id, &u, sizeof u);
  return LLAMPC_OK;
}

int llampc_comm_create(const void* id, int32_t world, int32_t rank, int32_t device, llampc_comm** out) {
  if (!out) return fail(LLAMPC_E_ARG, "out is NULL");
  *out = nullptr;
  if (!id || world < 1 || rank < 0 || rank >= world) return fail(LLAMPC_E_ARG, "bad comm arguments (world=%d rank=%d)", world, rank);
  if (!rccl().ok) return fail(LLAMPC_E_STATE, "RCCL unavailable: %s", rccl().why.c_str());
  DeviceGuard g(device);
  if (!g.ok) return fail(LLAMPC_E_HIP, "hipSetDevice(%d) failed", device);
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  ncclComm_t comm = nullptr;
  RCCL_TRY(rccl().init_rank(&comm, world, u, rank));
  auto* c = new llampc_comm();
  c->comm = comm;
  c->world = world;
  c->rank = rank;
  c->device = device;
  *out = c;
  return LLAMPC_OK;
}

int llampc_comm_destroy(llampc_comm* c) {
  if (!c) return LLAMPC_OK;
  if (c->comm && rccl().ok) {
    DeviceGuard g(c->device);
    (void)rccl().destroy(c->comm);
  }
  delete c;
  return LLAMPC_OK;
}

int llampc_exchange_rccl(llampc_comm* comm, const void* d_local, void* d_all, void* d_merged, int32_t nan_policy,
                         void* stream) {
  if (!comm || !d_local || !d_all || !d_merged || comm->world > 32)
    return fail(LLAMPC_E_ARG, "bad exchange arguments (world 1..32)");
  DeviceGuard g(comm->device);
  if (!g.ok) return fail(LLAMPC_E_HIP, "hipSetDevice(%d) failed", comm->device);
  if (int rc = comm_all_gather(comm, d_local, d_all, sizeof(llampc_plan_out), false, (hipStream_t)stream)) return rc;
  HIP_TRY(launch_merge((const llampc_plan_out*)d_all, comm->world, nan_policy == LLAMPC_NAN_FIRST,
                       (llampc_plan_out*)d_merged, (hipStream_t)stream));
  return LLAMPC_OK;
}

int llampc_mailbox_create(int32_t world, int32_t rank, int32_t device, llampc_mailbox** out) {
  if (out) *out = nullptr;
  if (!out || world < 1 || world > kPeerMax || rank < 0 || rank >= world)
    return fail(LLAMPC_E_ARG, "bad mailbox arguments (world=%d rank=%d, world 1..%d)", world, rank, kPeerMax);
  DeviceGuard g(device);
  if (!g.ok) return fail(LLAMPC_E_HIP, "hipSetDevice(%d) failed", device);
  Building<llampc_mailbox> mb(new llampc_mailbox(), llampc_mailbox_destroy);
  mb->world = world;
  mb->rank = rank;
  mb->device = device;
  const size_t words = (size_t)2 * world * kRecWords;
  int rc;
  if ((rc = mb->own.zalloc(words, "mailbox", LLAMPC_E_HIP)) ||
      (rc = mb->d_box.alloc(kPeerMax, "mailbox table", LLAMPC_E_HIP)))
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  mb->box[rank] = mb->own.get();
  *out = mb.release();
  return LLAMPC_OK;
}

int llampc_mailbox_ipc_handle(llampc_mailbox* mb, void* handle) {
  if (!mb || !handle) return fail(LLAMPC_E_ARG, "null mailbox/handle");
  DeviceGuard g(mb->device);
  hipIpcMemHandle_t h;
  HIP_TRY(hipIpcGetMemHandle(&h, mb->own.get()));
  memcpy(handle, &h, sizeof(h));
  return LLAMPC_OK;
}

int llampc_mailbox_open_peer(llampc_mailbox* mb, int32_t peer, const void* handle) {
  if (!mb || !handle || peer < 0 || peer >= mb->world || peer == mb->rank || mb->box[peer])
    return fail(LLAMPC_E_ARG, "bad peer %d (world %d, rank %d, or already open)", mb ? peer : -1,
                mb ? mb->world : 0, mb ? mb->rank : 0);
  DeviceGuard g(mb->device);
  std::lock_guard<std::mutex> lm(mb->mu);
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof(h));
  void* p = nullptr;
  HIP_TRY(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
  mb->box[peer] = (uint64_t*)p;
  mb->opened[peer] = true;
  mb->box_synced = false;
  return LLAMPC_OK;
}

int llampc_mailbox_link(llampc_mailbox* mb, int32_t peer, const llampc_mailbox* other) {
  if (!mb || !other || peer < 0 || peer >= mb->world || peer == mb->rank || mb->box[peer] ||
      other->world != mb->world || other->rank != peer || other->device != mb->device)
    return fail(LLAMPC_E_ARG, "bad mailbox link (peer %d)", peer);
  std::lock_guard<std::mutex> lm(mb->mu);
  mb->box[peer] = other->own.get();
  mb->box_synced = false;
  return LLAMPC_OK;
}

int llampc_mailbox_set_bound(llampc_mailbox* mb, double seconds) {
  if (!mb || !(seconds > 0) || seconds > 1e6) return fail(LLAMPC_E_ARG, "bad poll bound");
  mb->bound = (uint64_t)(seconds * 1e8);
  return LLAMPC_OK;
}

int llampc_exchange_peer(llampc_mailbox* mb, const void* d_local, void* d_merged, int32_t nan_policy,
                         void* stream) {
  if (!mb || !d_local || !d_merged) return fail(LLAMPC_E_ARG, "bad exchange arguments");
  for (int g = 0; g < mb->world; ++g)
    if (!mb->box[g]) return fail(LLAMPC_E_STATE, "mailbox of peer %d not open", g);
  DeviceGuard g(mb->device);
  if (!g.ok) return fail(LLAMPC_E_HIP, "hipSetDevice(%d) failed", mb->device);
  std::lock_guard<std::mutex> lm(mb->mu);
  const uint32_t seq = next_seq(mb->seq);
  PeerLaunch a{};
  a.local = (const llampc_plan_out*)d_local;
  for (int r = 0; r < mb->world; ++r) a.box[r] = mb->box[r];
  a.merged = (llampc_plan_out*)d_merged;
  a.bound = mb->bound;
  a.G = mb->world;
  a.rank = mb->rank;
  a.nan_first = nan_policy == LLAMPC_NAN_FIRST;
  a.seq = seq;
  HIP_TRY(launch_peer_exchange(a, (hipStream_t)stream));
  mb->seq = seq;
  return LLAMPC_OK;
}

int llampc_plan_exchange(llampc_bank* b, const llampc_plan_in* in, void* d_local, void* d_merged,
                         llampc_mailbox* mb, void* stream) {
  if (!b || !d_local || !d_merged || !mb) return fail(LLAMPC_E_ARG, "bank/d_local/d_merged/mailbox is NULL");
  if (mb->device != b->device) return fail(LLAMPC_E_ARG, "mailbox on device %d, bank on %d", mb->device, b->device);
  for (int g = 0; g < mb->world; ++g)
    if (!mb->box[g]) return fail(LLAMPC_E_STATE, "mailbox of peer %d not open", g);
  int rc = check_plan_in(b, in);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async tick is outstanding: call llampc_plan_wait");
  DeviceGuard g(b->device);
  hipStream_t s = pick_stream(b, stream);
  std::unique_lock<std::mutex> lm(mb->mu);
  if ((rc = mailbox_sync(mb))) return rc;   // the peers are open: publish the table once
  const bool split = getenv("LLAMPC_PEER_SPLIT") != nullptr;   // A/B: separate kernel
  const bool fusable = !in->do_lookahead || (in->integrator == LLAMPC_RK4 && in->xref_mode == LLAMPC_XREF_GIVEN);
  PlanTick t;
  t.out = (llampc_plan_out*)d_local;
  t.stream = s;
  if (!split && fusable && mb->world <= kPeerFuseMax) {
    t.px = mb;
    t.px_merged = (llampc_plan_out*)d_merged;
    return plan_launch(b, *in, t);
  }
  rc = plan_launch(b, *in, t);
  if (rc) return rc;
  lm.unlock();                           // llampc_exchange_peer takes it
  return llampc_exchange_peer(mb, d_local, d_merged, in->nan_policy, s);
}

int llampc_mailbox_destroy(llampc_mailbox* mb) {
  if (!mb) return LLAMPC_OK;
  DeviceGuard g(mb->device);
  (void)hipDeviceSynchronize();
  for (int r = 0; r < mb->world; ++r)
    if (mb->opened[r]) (void)hipIpcCloseMemHandle(mb->box[r]);
  delete mb;
  return LLAMPC_OK;
}

}  // extern "C"

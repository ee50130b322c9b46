// capi_common.hpp — what the C ABI's translation units share (capi.hip: errors, the bank's lifecycle,
// the raceline upload; capi_plan.hip: the plan tick and its entries, the track entries; capi_batch.hip:
// the raw batch calls and the merge; capi_xchg.hip: RCCL, mailboxes, exchange; capi_ctl.hip,
// capi_ctl_shard.hip and capi_ctl_corr.hip over capi_ctl.hpp: the controller; capi_nlp.hip: the NLP
// solver; capi_nlp_batch.hip: the batched NLP solver): error reporting, the owners of device and pinned
// memory, the handle structs (the controller's: capi_ctl.hpp) and the few functions one file calls in
// another.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "capi_host.hpp"

#pragma GCC visibility push(hidden)

// Records the calling thread's message (llampc_last_error) and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(LLAMPC_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                  __FILE__, __LINE__);                                                    \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Move-only owner of `cap()` elements of T from Acquire, given back to Release.  It frees in
// its destructor, so a handle is deleted with its device current, after its stream was
// synchronised and before that stream is destroyed.
template <class T, hipError_t (*Acquire)(void**, size_t), hipError_t (*Release)(void*)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept { *this = std::move(o); }
  Owned& operator=(Owned&& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
    return *this;
  }
  ~Owned() { reset(); }
  void reset() {
    if (p_) (void)Release(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // `count` elements (at least one), replacing what was held.
  int alloc(size_t count, const char* what = "buffer", int code = LLAMPC_E_OOM) {
    reset();
    count = std::max<size_t>(count, 1);
    const hipError_t e = Acquire(reinterpret_cast<void**>(&p_), count * sizeof(T));
    if (e != hipSuccess) {
      p_ = nullptr;
      return fail(code, "allocating the %s (%zu B) failed: %s", what, count * sizeof(T), hipGetErrorString(e));
    }
    cap_ = count;
    return LLAMPC_OK;
  }
  // ... all zero (device memory: in stream order on the null stream, as hipMemset).
  int zalloc(size_t count, const char* what = "buffer", int code = LLAMPC_E_OOM) {
    if (int rc = alloc(count, what, code)) return rc;
    HIP_TRY(hipMemset(p_, 0, cap_ * sizeof(T)));
    return LLAMPC_OK;
  }
  // Grows to at least `count` elements (a new allocation of max(count, floor); contents are lost).
  int reserve(size_t count, size_t floor = 0, const char* what = "buffer", int code = LLAMPC_E_OOM) {
    return count <= cap_ ? LLAMPC_OK : alloc(std::max(count, floor), what, code);
  }
  T* get() const { return p_; }
  size_t cap() const { return cap_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};
inline hipError_t acquire_uncached(void** p, size_t n) { return hipExtMallocWithFlags(p, n, hipDeviceMallocUncached); }
inline hipError_t acquire_pinned(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
inline hipError_t acquire_mapped(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocCoherent | hipHostMallocMapped); }
template <class T> using DevBuf = Owned<T, hipMalloc, hipFree>;
template <class T> using UncachedBuf = Owned<T, acquire_uncached, hipFree>;   // fine-grained (the peers' mailboxes)
template <class T> using PinnedBuf = Owned<T, acquire_pinned, hipHostFree>;
// Pinned, coherent and mapped, zeroed: get() for the host, dev() its device alias.
template <class T>
class Mapped {
 public:
  int alloc(size_t count, const char* what) {
    d_ = nullptr;
    if (int rc = h_.alloc(count, what)) return rc;
    std::memset(h_.get(), 0, h_.cap() * sizeof(T));
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&d_), h_.get(), 0) != hipSuccess)
      return fail(LLAMPC_E_HIP, "hipHostGetDevicePointer(%s) failed", what);
    return LLAMPC_OK;
  }
  T* get() const { return h_.get(); }
  T* dev() const { return d_; }

 private:
  Owned<T, acquire_mapped, hipHostFree> h_;
  T* d_ = nullptr;
};
// A launch's record in host memory and the completion tag the host spins on (spin_for_tag):
// the kernel writes the record, then stores the launch's number into tag[0].
template <class T>
struct MappedRecord {
  Mapped<T> rec;
  Mapped<uint64_t> tag;                  // 64 B: [0] the tag, [1] the controller's device time
  int alloc(const char* what) {
    const int rc = rec.alloc(1, what);
    return rc ? rc : tag.alloc(8, what);
  }
};

// A track's centre-line tables on the device, cx | cy | tt, [3][n], with its closed length and width
// (llampc_*_set_track): the bank's, the controller's and the two NLP solvers' each own one.
struct TrackTables {
  DevBuf<double> d;
  int32_t n = 0;                         // 0: no track set
  double L = 0.0, width = 0.0;
  // Replaces the tables with ones track_tables_invalid accepts, once `s` has drained (no launch reads the
  // tables being replaced); the caller holds the owner's locks, its device current.  A failure leaves no track.
  int upload(hipStream_t s, const double* centre, const double* theta, int32_t n_, double L_, double width_) {
    HIP_TRY(hipStreamSynchronize(s));
    n = 0;
    if (int rc = d.reserve(3 * (size_t)n_, 0, "track tables")) return rc;
    std::vector<double> h(3 * (size_t)n_);
    std::memcpy(h.data(), centre, 2 * (size_t)n_ * sizeof(double));
    std::memcpy(h.data() + 2 * (size_t)n_, theta, (size_t)n_ * sizeof(double));
    HIP_TRY(hipMemcpy(d.get(), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    n = n_;
    L = L_;
    width = width_;
    return LLAMPC_OK;
  }
  llampc::TrackK view() const { return {d.get(), d.get() + n, d.get() + 2 * (size_t)n, n, 0, L}; }
};

// ---- peer exchange (xGMI mailboxes; capi_xchg.hip) -------------------------------------
struct llampc_mailbox {
  int32_t world = 0, rank = 0, device = 0;
  UncachedBuf<uint64_t> own;             // [2][world][kRecWords], uncached device memory
  uint64_t* box[llampc::kPeerMax] = {};  // every rank's mailbox as mapped in this process
  bool opened[llampc::kPeerMax] = {};    // box[g] came from hipIpcOpenMemHandle
  uint32_t seq = 0;
  uint64_t bound = 1000000000ull;        // 10 s of s_memrealtime (100 MHz): ranks may drift apart
                                         // by host-side pauses; only a missing rank should time out
  DevBuf<uint64_t*> d_box;               // device copy of box[] (the fused exchange reads it)
  bool box_synced = false;
  std::mutex mu;                         // serialises the tick sequence (seq) and the table
};
// Publishes box[] to d_box once the peers are open (the caller holds mb->mu).
int mailbox_sync(llampc_mailbox* mb);

struct ncclComm;
struct llampc_comm {
  ncclComm* comm = nullptr;
  int32_t world = 0, rank = 0, device = 0;
};
// ncclAllGather of `count` elements per rank, bytes or (words) 64-bit words, on `s` (the caller
// has the comm's device current).
int comm_all_gather(llampc_comm* c, const void* send, void* recv, size_t count, bool words, hipStream_t s);

// ---- the bank (capi.hip; its ticks: capi_plan.hip) ------------------------------------------------------------
struct llampc_bank {
  int device = 0;
  int cus = 0;                           // the device's CU count, read at create (0: unknown)
  int64_t n = 0, goff = 0;
  int32_t W = 0, count = 0, slot = 0;
  llampc::VehK veh{};
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool dedicated = false;                // its own stream has a hardware queue of its own (bank_stream)
  int32_t share = 1;                     // banks ticked concurrently (llampc_bank_set_concurrency)
  DevBuf<double> d_params, d_ring;
  DevBuf<double> d_am_val, d_tk_val, d_pv, d_best_cost;
  DevBuf<int64_t> d_am_idx, d_tk_idx, d_pidx;
  DevBuf<int32_t> d_pnf, d_best_cand;
  PinnedBuf<double> h_in;                // pinned input pack
  DevBuf<double> d_in;
  PinnedBuf<llampc_plan_out> h_out;
  DevBuf<llampc_plan_out> d_out;
  DevBuf<double> d_err, d_wmean;         // [n]
  DevBuf<double> d_cost;                 // [n*C]
  DevBuf<unsigned> d_tickets;            // [2] in-launch completion tickets
  std::mutex mu;
  // optional per-kernel event timing: [kernel][2*i] start, [kernel][2*i+1] stop
  std::vector<hipEvent_t> ev[3];
  size_t ev_used[3] = {0, 0, 0};
  bool timing = false;
  int64_t timing_stride = 1;             // group of stride launches per pair (or sampling period)
  bool timing_sample = false;            // pair around one launch of every stride
  bool async_pending = false;            // llampc_plan_async issued, llampc_plan_wait not yet
  DevBuf<double> d_rl;                   // raceline table: knots | xy | speed | mus
  int32_t rl_n = 0, rl_M = 0;
  double rl_hmin = 1.0, rl_vmax = 0.0;   // the walkers' speed-window bounds (raceline.hpp)
  std::vector<double> rl_mus;            // the profiles' mu values (host copy: the controller's bracket)
  DevBuf<double> d_xref_pm;              // per-model references [n][H][2] (RACELINE ticks)
  int64_t timing_seen[3] = {0, 0, 0};
  DevBuf<uint64_t> d_la_tag;             // polled completion: [3][n] tagged per-model results
  DevBuf<uint64_t> d_blk_tag;            // [blocks][5] tagged look-ahead block partials
  uint32_t seq = 0;                      // launch tag (1, 2, ...; never 0 = the zeroed buffers)
  // host completion (llampc_plan, llampc_plan_async/wait): the plan kernel writes the record
  // straight into pinned host memory and then stores the tick's number into the tag; the host
  // spins on it (no D2H copy, no stream synchronisation on the path)
  MappedRecord<llampc_plan_out> host;
  uint64_t hseq = 0;
  uint64_t async_seq = 0;                // the outstanding llampc_plan_async tick's tag (0: copy path)
  int64_t launches = 0;                  // plan-kernel launches enqueued on this bank (llampc_bank_launches)
  DevBuf<uint64_t> d_wq;                 // work-queue unit counter (0 between launches; launch_plan's WQ layout)
  // the controller whose armed launch waits on this bank's stream (llampc_ctl_set_prelaunch):
  // every other call that enqueues on the stream cancels it first (bank_disarm)
  llampc_ctl* armed = nullptr;
  // the track tick (llampc_plan_track; kernels.hpp PlanTrack)
  TrackTables track;                     // llampc_bank_set_track
  DevBuf<double> d_trk;                  // the path copies [2][2][HMAX + 1] | their costs [2] | the read-back
  DevBuf<int32_t> d_trk_flags;           // the copies' valid flags [2] | the read-back's | the late word
  DevBuf<uint64_t> d_hp_tag;             // [12 HMAX] tagged half-plane words
  uint32_t tseq = 0;                     // the half-plane words' own sequence: every track tick advances it
  int32_t trk_cur = 0;                   // the copy that holds (or will hold, once the stream drains) the newest path
  llampc::TrackPathState trk_path{0};    // the host's half of the path rule
  int32_t trk_last_H = 0;                // the horizon of the last launch if it was a track tick, else 0
};
static inline llampc::BankView bank_view(const llampc_bank& b) {
  return {b.d_params.get(), b.n, b.goff, b.veh, b.d_ring.get(), b.W, b.slot, b.d_wmean.get(),
          b.d_am_val.get(), b.d_am_idx.get(), b.d_tk_val.get(), b.d_tk_idx.get(),
          b.d_rl.get(), b.rl_n, b.rl_M, b.rl_hmin, b.rl_vmax};
}
// ... and what a plan tick takes beside it (px: the fused exchange's mailbox, or null).
static inline llampc::PlanView plan_view(const llampc_bank& b, const llampc_mailbox* px) {
  return {bank_view(b), b.d_best_cand.get(), b.d_best_cost.get(), b.d_pv.get(), b.d_pidx.get(), b.d_pnf.get(),
          b.d_la_tag.get(), b.d_blk_tag.get(), b.d_wq.get(), b.d_tickets.get(), b.d_xref_pm.get(),
          b.track.d.get(), b.track.n, b.track.L, b.track.width, b.d_trk.get(), b.d_trk_flags.get(), b.d_hp_tag.get(),
          px ? px->d_box.get() : nullptr, px ? px->world : 0, px ? px->rank : 0, px ? px->bound : 0};
}

// Cancels the armed controller launch waiting on the bank's stream, if any (capi_ctl.hip): the
// launch exits without touching anything, and work enqueued after it runs once it has.
void bank_disarm(llampc_bank* b);
// "This call needs the bank idle": the solver's mutex (or none), then b->mu; the armed launch cancelled;
// rc, reported through fail(), if an async tick is outstanding; the bank's device current.  An entry
// with checks of its own between the two locks takes its solver's mutex itself.
struct BankIdle {
  std::unique_lock<std::mutex> ls, lk;
  int rc;
  DeviceGuard g;
  explicit BankIdle(llampc_bank* b, std::mutex* solver = nullptr)
      : ls(solver ? std::unique_lock<std::mutex>(*solver) : std::unique_lock<std::mutex>()), lk(b->mu),
        rc((bank_disarm(b), b->async_pending) ? fail(LLAMPC_E_STATE, "an async tick is outstanding on the bank") : LLAMPC_OK),
        g(b->device) {}
};
// The bank's own stream on a hardware queue of its own (the caller holds b->mu; nothing armed).
int bank_dedicate(llampc_bank* b);
// plan_in_refused of the bank's facts, reported through fail() (capi_plan.hip; the caller holds b->mu
// or reads a bank nothing else configures).
int check_plan_in(const llampc_bank* b, const llampc_plan_in* in);
// The tick on device pointers (capi_plan.hip): ONE launch (look-back + look-ahead + completion) of what
// `tick` names (capi_host.hpp PlanTick).  The bank's host state advances only once the launch was enqueued.
int plan_launch(llampc_bank* b, const llampc_plan_in& in, const llampc::PlanTick& tick);
inline hipStream_t pick_stream(llampc_bank* b, void* s) { return s ? (hipStream_t)s : b->stream; }

// llampc_nlp_create's and llampc_nlp_batch_create's: nlp_cfg_invalid reported through fail()
// (capi_nlp.hip), and nlp_ltraj_flags of the environment (LLAMPC_NLP_RERUN_TRAJ, read here alone).
int nlp_check_cfg(const llampc_nlp_cfg& k);
inline llampc::NlpLtraj nlp_create_ltraj(const llampc_nlp_cfg& k) {
  const char* rt = std::getenv("LLAMPC_NLP_RERUN_TRAJ");
  return llampc::nlp_ltraj_flags(k, rt && rt[0] == '1');
}

// Event pair around a GROUP of timing_stride consecutive launches of kernel `k` (0 the plan
// kernel; 1, 2 reserved): start before the group's first launch, stop after its last, so a
// launch's mean duration is elapsed / group — the events' own cost (~2 us per record on
// this stack) is spread over the group instead of inflating every bracketed launch.
struct TimedLaunch {
  llampc_bank* b;
  int k;
  hipStream_t s;
  hipEvent_t stop = nullptr;
  TimedLaunch(llampc_bank* b_, int k_, hipStream_t s_) : b(b_), k(k_), s(s_) {
    if (!b->timing || 2 * (b->ev_used[k] + 1) > b->ev[k].size()) return;
    const int64_t pos = b->timing_seen[k]++ % b->timing_stride;
    const size_t i = b->ev_used[k];
    if (pos == 0) (void)hipEventRecord(b->ev[k][2 * i], s);
    // sampling: the pair brackets the period's first launch alone
    if (pos == (b->timing_sample ? 0 : b->timing_stride - 1)) stop = b->ev[k][2 * i + 1];
  }
  ~TimedLaunch() {
    if (stop) {
      (void)hipEventRecord(stop, s);
      b->ev_used[k]++;
    }
  }
};

// Deletes a solver bound to a bank (p->b) once the bank's stream has drained.
template <class S>
int solver_destroy(S* p) {
  if (!p) return LLAMPC_OK;
  DeviceGuard g(p->b->device);
  if (p->b->stream) (void)hipStreamSynchronize(p->b->stream);
  delete p;
  return LLAMPC_OK;
}

// A handle under construction: a create that fails part-way destroys it (llampc_*_destroy).
template <class H> using Building = std::unique_ptr<H, int (*)(H*)>;

#pragma GCC visibility pop

// capi.hip — extern "C" boundary (include/llampc.h): error reporting and the device-resident
// model-bank handle's lifecycle.  (The ticks on a bank: capi_plan.hip; the calls that take no bank:
// capi_batch.hip.)
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

namespace {

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

}  // extern "C"

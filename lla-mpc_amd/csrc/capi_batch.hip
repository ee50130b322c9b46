// capi_batch.hip — the extern "C" calls that take no bank (include/llampc.h): the merge of the
// shards' records and the raw batched dynamics / integration / math calls with their per-device
// workspace.
#include "capi_common.hpp"
#include "merge.hpp"

using namespace llampc;

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

extern "C" {

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

int llampc_dynamics_batch(int32_t op, const double* x, const double* u,
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

int llampc_integrate_batch(const double* x0, const double* u, int64_t u_stride_lane,
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

int llampc_math_batch(int32_t fn, const double* a, const double* b, int64_t n,
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

}  // extern "C"

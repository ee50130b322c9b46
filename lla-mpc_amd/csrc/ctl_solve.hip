// ctl_solve.hip — the fused control step's glue kernels (ctl_solve.hpp; llampc_ctl_step,
// capi_ctl_solve.hip): one block each, enqueued around the tick's launch and the batched NLP search on
// the bank's stream.  They wait for nothing but stream order: the tick's launch has completed (its
// state and its debug copy of the reference are in device memory) before the build kernel starts, the
// search (its result and tag in device memory) before the commit kernel does.
#include "ctl_solve.hpp"

namespace llampc {
namespace {

// CtlState.u_prev as the tick is about to read it: zeros before the first tick.
__global__ __launch_bounds__(64) void ctl_solve_snapshot_kernel(const CtlState* st, double* uprev) {
  if (threadIdx.x < 2) uprev[threadIdx.x] = st->u_prev[threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void ctl_solve_build_kernel(CtlSolveBuild a) {
  __shared__ double lx[6], lnom[6], lup[2];
  const int tid = threadIdx.x;
  // x_t and the nominal model from the kernel arguments by constant index (no copy of the
  // argument to scratch)
#pragma unroll
  for (int j = 0; j < 6; ++j)
    if (tid == j) {
      lx[j] = a.x_t[j];
      lnom[j] = a.nominal[j];
    }
  if (tid < 2) lup[tid] = a.uprev[tid];
  __syncthreads();
  if (tid >= 64 && tid < 70) {
    const bool warm = a.warm != 0;
    a.p6[tid - 64] = ctl_solve_p6(tid - 64, warm, lnom, a.params, a.n, warm ? 0 : a.st->current_model - a.goff);
  }
  ctl_solve_record(a.rec, a.H, a.up_off, lx, a.dbg, &a.st->useq[0][0], lup, a.seed, tid, (int)blockDim.x);
}

__global__ __launch_bounds__(kBlock) void ctl_solve_commit_kernel(CtlSolveCommit a) {
  const int tid = threadIdx.x, H = a.H;
  const NlpResult* r = a.res;
  const bool arrived = __hip_atomic_load(a.tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.want;
  const bool ok = arrived && r->best_it >= 0;
  llampc_ctl_solve_out* o = a.out;
  CtlState* st = a.st;
  // a solve without a finite objective (or whose tag never came): umpc zeros, fval +inf, and the
  // state as the tick left it (nlp_batch_unpack's contract)
  for (int e = tid; e < 2 * H; e += (int)blockDim.x) {
    const double v = ok ? (&r->best_u[0][0])[e] : 0.0;
    (&o->umpc[0][0])[e] = v;
    if (ok) {
      (&st->useq[0][0])[e] = v;
      if (e < 2) st->u_prev[e] = v;
    }
  }
  for (int e = tid; e < 6 * (H + 1); e += (int)blockDim.x) (&o->xmpc[0][0])[e] = arrived ? (&r->traj[0][0])[e] : 0.0;
  if (tid == 0) {
    o->fval = ok ? r->best_j : __builtin_inf();
    o->uprev[0] = a.uprev[0];
    o->uprev[1] = a.uprev[1];
    o->model = a.warm ? -1 : st->current_model;
    o->status = ok ? LLAMPC_NLP_OK : arrived ? LLAMPC_NLP_NO_FINITE : LLAMPC_NLP_NO_TAG;
    o->committed = ok ? 1 : 0;
  }
  __threadfence_system();               // the record's host-memory stores, then the tag
  __syncthreads();
  if (tid == 0) __hip_atomic_store(a.host_tag, a.host_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

hipError_t launch_ctl_solve_snapshot(const CtlState* st, double* uprev, hipStream_t s) {
  hipLaunchKernelGGL(ctl_solve_snapshot_kernel, dim3(1), dim3(64), 0, s, st, uprev);
  return hipGetLastError();
}
hipError_t launch_ctl_solve_build(const CtlSolveBuild& a, hipStream_t s) {
  hipLaunchKernelGGL(ctl_solve_build_kernel, dim3(1), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_ctl_solve_commit(const CtlSolveCommit& a, hipStream_t s) {
  hipLaunchKernelGGL(ctl_solve_commit_kernel, dim3(1), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace llampc

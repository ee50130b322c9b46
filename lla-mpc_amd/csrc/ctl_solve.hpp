// ctl_solve.hpp — the fused control step's glue (llampc_ctl_step, include/llampc.h; ctl_solve.hip;
// capi_ctl_solve.hip): what joins the controller tick's launch to the batched NLP search of the model
// that tick selected, on the bank's stream with no host in between.
//   snapshot   CtlState.u_prev -> d_uprev [2] before the tick overwrites it (du_0's reference)
//   build      after the tick: problem 0's record in nlp_batch_layout's format into DEVICE memory
//              (x0 = x_t | the tick's xref from its debug copy | the first mean = the tick's chosen
//              sequence, not shifted | uprev = d_uprev | the seed | model 0, has_hold 1) and the
//              search's private parameter table p6 [6][1]: the nominal model while warm, else the
//              bank column the tick selected
//   (the solve: nlp_kernel<.., NlpBatch>, B = 1, unmodified; its result and tag in device memory)
//   commit     a solve that found a finite objective becomes the controller's applied sequence
//              (CtlState.u_prev <- best_u[0], CtlState.useq <- best_u); the result goes to the pinned
//              llampc_ctl_solve_out, then a system-scope fence and the host tag
// Neither kernel polls: stream order is their only wait.  The record's words and the table's entries
// are __host__ __device__ functions, so that a host harness holds them bitwise to nlp_batch_pack
// (tests/native/ctl_solve_host.cpp); the refusals' predicates are pure too (the cfg's here, the
// controller state's and its setters' in ctl_solve_refuse.hpp).
#pragma once
#include "ctl_solve_refuse.hpp"
#include "nlp.hpp"

namespace llampc {

// Word e of problem 0's record, e in [0, up_off + 4): nlp_batch_pack's words for model 0 with
// has_hold = 1 and base = mean0 [H][2].  up_off = 6 + 2 (H + 1) + 2 H (nlp_batch_layout).
__host__ __device__ __forceinline__ uint64_t ctl_solve_rec_word(int e, int H, uint32_t up_off, const double* x0,
                                                                const double* xref, const double* mean0,
                                                                const double* uprev, uint64_t seed) {
  const int nx = 6 + 2 * (H + 1), up = (int)up_off;
  if (e == up + 2) return seed;
  if (e == up + 3) return (uint64_t)1 << 32;          // model 0 | has_hold 1 << 32
  const double v = e < 6 ? x0[e] : e < nx ? xref[e - 6] : e < up ? mean0[e - nx] : uprev[e - up];
  return __builtin_bit_cast(uint64_t, v);
}
// The record's words first, first + stride, ... (the host: 0 and 1; a block: its thread and size).
// The pad after word up_off + 3 is not touched, as nlp_batch_pack leaves it.
__host__ __device__ __forceinline__ void ctl_solve_record(uint64_t* rec, int H, uint32_t up_off, const double* x0,
                                                          const double* xref, const double* mean0, const double* uprev,
                                                          uint64_t seed, int first, int stride) {
  for (int e = first; e < (int)up_off + 4; e += stride) rec[e] = ctl_solve_rec_word(e, H, up_off, x0, xref, mean0, uprev, seed);
}
// Entry j of the search's parameter table [6][1]: the nominal model's while the tick was warm, else
// the bank's column `col` of params [6][n] — NaN for a column the bank does not hold, so that the
// solve finds no finite objective and nothing is committed.
__host__ __device__ __forceinline__ double ctl_solve_p6(int j, bool warm, const double* nominal, const double* params,
                                                        int64_t n, int64_t col) {
  if (warm) return nominal[j];
  return col >= 0 && col < n ? params[(size_t)j * (size_t)n + (size_t)col] : __builtin_nan("");
}

// ---- the refusals (pure; the state's and the setters': ctl_solve_refuse.hpp) ---------------------
// llampc_ctl_solver_create with a cfg that passed nlp_cfg_invalid: LLAMPC_E_ARG's message, or null.
inline const char* ctl_solver_cfg_refused(int32_t H, double Ts, int32_t samples, int32_t ctl_H, double ctl_Ts, int32_t cus) {
  if (H != ctl_H) return "H must equal the controller's";
  if (Ts != ctl_Ts) return "Ts must equal the controller's";
  if (!nlp_persistent(samples)) return "samples: every round in one launch only (samples / 64 <= 64)";
  if (samples / 64 > cus) return "samples / 64 blocks exceed the device's CUs";
  return nullptr;
}

// ---- the glue kernels' arguments (ctl_solve.hip) --------------------------------------------------
struct CtlSolveBuild {
  const CtlState* st;         // as the tick left it
  const double* dbg;          // the tick's xref [2][H+1] (CtlLaunch.dbg)
  const double* uprev;        // d_uprev [2] (the snapshot)
  uint64_t* rec;              // problem 0's record (device memory)
  double* p6;                 // [6][1]
  const double* params;       // the bank's [6][n]
  int64_t n, goff;
  double x_t[6], nominal[6];
  uint64_t seed;
  uint32_t up_off;
  int32_t H, warm;
};
struct CtlSolveCommit {
  CtlState* st;
  const NlpResult* res;       // the solve's result and tag (device memory)
  const uint64_t* tag;
  uint64_t want;              // this step's solve number
  const double* uprev;        // d_uprev [2]
  llampc_ctl_solve_out* out;  // device alias of the pinned record
  uint64_t* host_tag;
  uint64_t host_seq;
  int32_t H, warm;
};
hipError_t launch_ctl_solve_snapshot(const CtlState* st, double* uprev, hipStream_t s);
hipError_t launch_ctl_solve_build(const CtlSolveBuild& a, hipStream_t s);
hipError_t launch_ctl_solve_commit(const CtlSolveCommit& a, hipStream_t s);

}  // namespace llampc

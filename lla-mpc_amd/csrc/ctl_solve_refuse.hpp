// ctl_solve_refuse.hpp — what the controller's host units need of the fused step (ctl_solve.hpp) and
// of llampc_ctl_set_applied: the pure predicates of their refusals, nothing of the NLP search.
// Included by capi_ctl.hpp and ctl_solve.hpp; run on the CPU by tests/native/ctl_solve_host.cpp.
#pragma once
#include <stdint.h>

namespace llampc {

// llampc_ctl_solver_create on a controller in this state: LLAMPC_E_STATE's message, or null.
struct CtlSolveFacts {
  bool attached, pending, prelaunch, exchange, gather;
  double cor_w;
};
inline const char* ctl_solver_state_refused(const CtlSolveFacts& f) {
  if (f.attached) return "the controller already has a solver";
  if (f.pending) return "a controller tick is outstanding";
  if (f.prelaunch) return "the fused step has no armed launches: switch prelaunch off first";
  if (f.exchange || f.gather) return "the fused step is unsharded (the controller exchanges its selection)";
  if (f.cor_w > 0) return "the fused step has no corridor ticks: switch the corridor off first";
  return nullptr;
}
// What a controller with a solver attached refuses of its setters (LLAMPC_E_STATE), or null:
// prelaunch on, a corridor weight > 0, an exchange or a gather transport.
enum class CtlSetter { prelaunch, corridor, exchange, gather };
inline const char* ctl_solver_blocks(bool attached, CtlSetter what, bool on) {
  if (!attached || !on) return nullptr;
  switch (what) {
    case CtlSetter::prelaunch: return "a solver is attached: the fused step has no armed launches";
    case CtlSetter::corridor: return "a solver is attached: the fused step has no corridor ticks";
    case CtlSetter::exchange: return "a solver is attached: the fused step is unsharded (set_exchange)";
    case CtlSetter::gather: return "a solver is attached: the fused step is unsharded (set_gather)";
  }
  return nullptr;
}
// llampc_ctl_set_applied's values: u0 [2] and useq [H][2] (or null) finite.
inline bool ctl_applied_finite(const double* u0, const double* useq, int32_t H) {
  bool ok = __builtin_isfinite(u0[0]) && __builtin_isfinite(u0[1]);
  for (int i = 0; useq && i < 2 * H; ++i) ok = ok && __builtin_isfinite(useq[i]);
  return ok;
}

}  // namespace llampc

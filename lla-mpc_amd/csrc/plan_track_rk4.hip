// plan_track_rk4.hip — the track tick (llampc_plan_track; kernels.hpp PlanTrack): llampc_plan_corridor's
// tick whose corridor H blocks of the same launch build from the bank's track, along the path the
// tick before left on the device.  Fused RK4, the shared xref, device inputs, every lane split; still
// one launch per tick.  Roles by block index (plan_track_dev.hpp):
//
//   look-back blocks [0, nb_lb)          plan_body's: the look-back, lb_final, and — a polled tick — the
//                                        completion (final_poll)
//   corridor blocks  [nb_lb, nb_lb + H)  block k = 1..H: the track's half-planes at path point P_k
//                                        (corridor_block_dev.hpp), published as the tagged words
//                                        hp_tag[12 (k - 1) ..]; with no valid path the disabled row.  P is
//                                        state the PREVIOUS launch wrote (or llampc_bank_set_path)
//   look-ahead blocks after those        lookahead_block<RK4, STAGE, LPM, 0, 0, CORR>'s rollouts and cost,
//                                        hp polled from the 12 H words into LDS
//
// Waiting: a corridor block waits for nothing.  A look-ahead block waits only for the corridor blocks,
// whose indices are below its own; it never waits on a look-back or a look-ahead block.  The completion
// (the look-back ticket winner's poll, or the last ticket's block) waits only for look-ahead blocks,
// which by then never wait again.  Workgroups are dispatched in index order, so whatever a block waits
// for has been dispatched; every wait is bounded (LLAMPC_STATUS_POLL_TIMEOUT in the record, never
// expected).  With do_lookback = 0 there is no look-back block and the corridor blocks come first.
//
// The half-plane words carry a sequence of their own (PlanTrack::seq) that advances on every track
// tick: the launch's tag advances on polled ticks only.  Once the record is complete — and, with host
// completion, its tag stored — the completing block re-runs the chosen rollout with its positions
// stored and writes the next tick's path (track_path_update), in both completion paths.
#include "plan_track_dev.hpp"

namespace llampc {

void launch_plan_track(const LookbackLaunch& lb, const LookaheadLaunch& la, const FinalLaunch& f, int G, int cpl,
                       bool stage, int lpm, size_t lds, hipStream_t s, const PlanTrack& trk) {
  const auto with_stage = [&](auto L) {
    constexpr int kL = decltype(L)::value;
    if (stage) launch_plan_track_t<true, kL>(lb, la, f, G, cpl, lds, s, trk);
    else launch_plan_track_t<false, kL>(lb, la, f, G, cpl, lds, s, trk);
  };
  if (lpm == 4) with_stage(std::integral_constant<int, 4>{});
  else if (lpm == 2) with_stage(std::integral_constant<int, 2>{});
  else with_stage(std::integral_constant<int, 1>{});
}

#ifdef LLAMPC_STAMPS
// diagnostic reader of this TU's phase stamps (plan_track_dev.hpp g_trk_ph [1024][8])
extern "C" int llampc_debug_track_ph(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_trk_ph), sizeof(g_trk_ph)) == hipSuccess ? 0 : -2;
}
#endif

}  // namespace llampc

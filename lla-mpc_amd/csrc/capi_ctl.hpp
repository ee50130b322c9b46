// capi_ctl.hpp — what the controller's host units share (capi_ctl.hip: lifecycle, tick, wait, arming;
// capi_ctl_shard.hip: the sharding transports; capi_ctl_corr.hip: the track and the corridor): the
// handle, the view a tick takes of it (capi_host.hpp CtlView) and the cancel of its armed launch.
// Included by those three units and by the fused step's (capi_ctl_solve.hip), which enqueues the tick's
// launch through ctl_tick_launched, declared at the end.
#pragma once
#include "capi_common.hpp"
#include "ctl_solve_refuse.hpp"

#pragma GCC visibility push(hidden)

struct llampc_ctl {
  llampc_bank* b = nullptr;
  llampc_ctl_cfg cfg{};
  bool no_stage = false;                 // LLAMPC_CTL_NO_STAGE=1: unstaged look-ahead inputs (A/B)
  // the state's projidx / mu-hat as the last record left them (the look-ahead prologue's
  // projection and mu bracket come as kernel arguments); hint_ok = false after a failed wait:
  // the next tick reads them from the device first
  bool hint_ok = true;
  int32_t hint_p0 = 0;
  double hint_mu = std::nan("");
  DevBuf<llampc::CtlState> d_st;
  DevBuf<double> d_pts;                  // points [2][np] | prefix [np - 1]
  int32_t np = 0;
  MappedRecord<llampc_ctl_out> host;     // the tick's record and its completion tag
  uint64_t hseq = 0;
  DevBuf<uint64_t> d_sel_tag;            // [kCtlSlotsMax]
  DevBuf<uint64_t> d_slot_tag;           // [kCtlSlotsMax][4]
  DevBuf<unsigned> d_tickets;            // [1]
  DevBuf<double> d_dbg;                  // xref [2][H+1] | U [C][H][2] (debug_inputs)
  DevBuf<double> d_znoise;               // [2][C H][2] the candidates' variates (CtlLaunch.znoise)
  DevBuf<uint64_t> d_ztag;               // [2]
  uint32_t seq = 0;
  int64_t t = 0;
  bool pending = false;
  uint64_t pend_seq = 0;
  // sharded (llampc_ctl_set_exchange): the peers' mailboxes and the replicated global table
  llampc_mailbox* mb = nullptr;
  DevBuf<double> d_gparams;              // [6][n_global]
  int64_t n_global = 0;
  // sharded over a gather transport (llampc_ctl_set_gather; CtlLaunch.px_phase): RCCL, or the
  // caller carries the records (xg_comm null) between the two launches of a full-window tick
  int32_t xg_world = 0, xg_rank = 0;
  llampc_comm* xg_comm = nullptr;
  DevBuf<uint64_t> d_xsend;              // [nw] this shard's record (the first launch writes it)
  DevBuf<uint64_t> d_xgath;              // [G][nw] the gathered records
  PinnedBuf<uint64_t> h_xstage;          // pinned [G][nw] (the host transport's staging)
  uint32_t xg_seq = 0;
  bool xg_wait = false;                  // the host transport's second launch awaits llampc_ctl_resume
  bool xg_read = false;                  //   and this rank's record has been read
  int32_t xg_nw = 0;
  // armed launches (llampc_ctl_set_prelaunch): the next tick's launch is enqueued behind this
  // one and waits for x_t on the doorbell (CtlLaunch.door)
  bool prelaunch = false;
  bool armed = false;
  bool arm_next = false;                 // arm the next tick in llampc_ctl_wait (before its spin)
  Mapped<uint64_t> door;                 // pinned: kCtlDoorWords tagged words (CtlLaunch.door)
  DevBuf<uint64_t> d_door_dev;           // block 0's device copy (CtlLaunch.door_dev)
  // the speculative look-ahead of armed ticks (CtlLaunch.n_spec; LLAMPC_CTL_NO_SPEC=1: never)
  bool no_spec = false;
  // spec models per armed tick: 32 (LLAMPC_CTL_SPEC_N, <= kCtlSpecMax).  The paced two-track step
  // measured p50 56.1 / 55.9 us with 32, 57.8 / 58.0 with 64, 57.9 with 96 (profiles/r05/specn/):
  // fewer busy CUs outweigh the 2-3 % more misses (profiles/r05/spec_topm.json)
  int32_t spec_cap = 32;
  int32_t spec_nb = 0;                   // look-back blocks the lists were sized for
  DevBuf<double> d_spec_val;             // [spec_nb][kCtlSpecMax]
  DevBuf<int64_t> d_spec_idx;
  DevBuf<uint64_t> d_spec_tag;           // [kCtlSpecMax]
  DevBuf<uint64_t> d_spec_res;           // [kCtlSpecMax][4]
  DevBuf<uint64_t> d_xref_tag;           // [2 (HMAX + 1)][2]
  uint32_t door_ctr = 0;                 // never reused: a cancelled word cannot match a later launch
  uint64_t dev_ticks = 0;                // the last completed tick's device time (llampc_ctl_device_us)
  std::chrono::steady_clock::time_point arm_t{};
  // the soft track corridor (llampc_ctl_set_track / llampc_ctl_set_corridor; ctl.hpp CtlCorridor)
  TrackTables track;
  double cor_w = 0.0, cor_margin = 0.0;  // weight 0: off (the tick launches ctl_kernel)
  bool cor_prev = false;                 // the last tick enqueued was a corridor tick (CtlCorridor.path_ok)
  DevBuf<double> d_cor;                  // the path copies and the read-back copies (capi_host.hpp ctl_cor_layout)
  DevBuf<uint64_t> d_hp_tag;
  DevBuf<int32_t> d_cor_flag;
  DevBuf<double> d_cor_cost;             // debug_inputs: every rolled-out cost of the last corridor tick [kCtlSlotsMax][C]
  int32_t cor_nslots = 0;                //   and how many slots it rolled out
  // prepared ticks (capi_host.hpp CtlPrep): the armed launch, and the host transport's pending second launch
  llampc::CtlPrep arm, xg_second;
  // a fused-step solver borrows this controller (llampc_ctl_solver_create; capi_ctl_solve.hip): the
  // setters it rules out refuse while it is attached (ctl_solve_refuse.hpp ctl_solver_blocks)
  bool solver_attached = false;
  bool dbg_by_solver = false;            // d_dbg was allocated for the solver (freed when it goes)
  std::mutex mu;
};

// What a tick takes from the controller (the caller holds c.mu, c.b->mu and, with a peer exchange,
// c.mb->mu): built per tick, on the stack.
static inline llampc::CtlView ctl_view(const llampc_ctl& c) {
  const llampc_bank& b = *c.b;
  const llampc_mailbox* mb = c.mb;
  return {bank_view(b), &c.cfg, c.d_st.get(), c.host.rec.dev(), c.host.tag.dev(),
          c.d_sel_tag.get(), c.d_slot_tag.get(), c.d_tickets.get(),
          c.d_dbg.get(), c.d_znoise.get(), c.d_ztag.get(),
          c.d_pts.get(), c.d_pts.get() + 2 * (size_t)c.np, c.np,
          c.door.dev(), c.d_door_dev.get(),
          c.d_spec_val.get(), c.d_spec_idx.get(), c.d_spec_tag.get(), c.d_spec_res.get(), c.d_xref_tag.get(),
          c.spec_nb, c.spec_cap, c.no_spec, c.no_stage,
          b.cus, b.share, b.rl_mus.data(),
          c.d_gparams.get(), c.n_global,
          mb != nullptr, mb ? mb->d_box.get() : nullptr, mb ? mb->world : 0, mb ? mb->rank : 0, mb ? mb->bound : 0,
          c.xg_world, c.xg_rank, c.d_xsend.get(), c.d_xgath.get(),
          c.track.d.get(), c.track.n, c.track.L, c.track.width, c.cor_w, c.cor_margin,
          c.d_cor.get(), c.d_cor_flag.get(), c.d_hp_tag.get(), c.d_cor_cost.get()};
}

// Cancels the controller's armed launch, if any: the launch exits without touching anything.
static inline void ctl_cancel(llampc_ctl* c) {
  if (!c || !c->armed) return;
  __atomic_store_n(&c->door.get()[llampc::kCtlDoorWords - 1], llampc::ctl_door_cancel_word(c->arm.L.door_seq),
                   __ATOMIC_RELEASE);
  // its completion number is spent: a launch that expired before the cancel has stored it
  // (with kCtlTagExpired) into the tag the next tick's wait reads.  So is its selection tag: the
  // cancelled launch may have published spec_tag words tagged arm.seq before its doorbell, which
  // a relaunch with the same tag would read as its own
  c->hseq = c->arm.next.hseq;
  c->seq = c->arm.next.seq;
  c->armed = false;
  if (c->b && c->b->armed == c) c->b->armed = nullptr;
}

// A launched tick's steps as llampc_ctl_tick_async runs them (capi_ctl.hip), for the fused step, which
// enqueues kernels of its own around the launch: refresh and prepare; then before(arg, warm) — the
// prepared tick's warm flag; a non-zero return ends the call with nothing of the tick enqueued — then
// the tick's one launch and its commit (the tick is then outstanding: llampc_ctl_wait).  The caller holds
// c->mu and c->b->mu; the controller has no armed launch, exchange or gather transport.
int ctl_tick_launched(llampc_ctl* c, const double* x_t, int (*before)(void* arg, int32_t warm), void* arg);

#pragma GCC visibility pop

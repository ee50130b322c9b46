// capi_ctl.hip — the controller tick's host side (llampc_ctl_*, include/llampc.h; ctl.hip):
// the control loop body rt.py:278-366 as ONE launch per step, the controller state resident on
// the device between steps.
#include "capi_common.hpp"

using namespace llampc;

static_assert(sizeof(llampc_ctl_cfg) == 280, "llampc_ctl_cfg layout (llampc/_native.py CtlCfg)");
static_assert(sizeof(llampc_ctl_out) == sizeof(llampc_plan_out) + 56 + 16 * LLAMPC_HMAX, "llampc_ctl_out layout");

struct __attribute__((visibility("hidden"))) llampc_ctl {
  llampc_bank* b = nullptr;
  llampc_ctl_cfg cfg{};
  bool no_stage = false;                 // LLAMPC_CTL_NO_STAGE=1: unstaged look-ahead inputs (A/B)
  // the state's projidx / mu-hat as the last record left them (the look-ahead prologue's
  // projection and mu bracket come as kernel arguments); hint_ok = false after a failed wait:
  // the next tick reads them from the device first
  bool hint_ok = true;
  int32_t hint_p0 = 0;
  double hint_mu = std::nan("");
  DevBuf<CtlState> d_st;
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
  DevBuf<double> d_track;                // cx | cy | tt, [3][tr_n]
  int32_t tr_n = 0;                      // 0: no track set
  double tr_L = 0.0, tr_width = 0.0;
  double cor_w = 0.0, cor_margin = 0.0;  // weight 0: off (the tick launches ctl_kernel)
  bool cor_prev = false;                 // the last tick enqueued was a corridor tick (CtlCorridor.path_ok)
  DevBuf<double> d_cor;                  // path state [2][2][HMAX + 1], then the read-back copies [2][kCtlCorDbgDoubles]
  DevBuf<uint64_t> d_hp_tag;             // [12 HMAX]
  DevBuf<int32_t> d_cor_flag;            // the paths' valid flags [2], the read-back's [2]
  DevBuf<double> d_cor_cost;             // debug_inputs: every rolled-out cost of the last corridor tick [kCtlSlotsMax][C]
  int32_t cor_nslots = 0;                //   and how many slots it rolled out
  struct Prep {                          // a prepared tick: its launch and what it commits
    bool corr = false;                   // a corridor tick: ctl_kernel_corr with `cor`
    CtlCorridor cor{};
    CtlLaunch L{};
    int lpm = 4;
    size_t lds = 0;
    uint64_t hs = 0;
    uint32_t seq = 0, px_seq = 0;
    int64_t t = 0;
    bool do_lb = false;
    int32_t count = 0;
  } arm, xg_second;                      // xg_second: the host transport's pending second launch
  std::mutex mu;
};

// An armed launch waits at most kArmBound for its doorbell; the host fires it only while it is
// younger than kArmFresh (else cancels it and launches the tick normally), so the launch
// cannot expire between the host's check and its store short of a ~1 s stall of that thread.
constexpr double kArmBoundS = 2.0;
constexpr double kArmFreshS = 0.5;

static void ctl_cancel(llampc_ctl* c) {
  if (!c || !c->armed) return;
  __atomic_store_n(&c->door.get()[kCtlDoorWords - 1], ((uint64_t)c->arm.L.door_seq << 32) | kCtlDoorCancel,
                   __ATOMIC_RELEASE);
  // its completion number is spent: a launch that expired before the cancel has stored it
  // (with kCtlTagExpired) into the tag the next tick's wait reads.  So is its selection tag: the
  // cancelled launch may have published spec_tag words tagged arm.seq before its doorbell, which
  // a relaunch with the same tag would read as its own
  c->hseq = c->arm.hs;
  c->seq = c->arm.seq;
  c->armed = false;
  if (c->b && c->b->armed == c) c->b->armed = nullptr;
}

void bank_disarm(llampc_bank* b) {
  if (b && b->armed) ctl_cancel(b->armed);
}

// Controllers whose tick was rung and whose next launch is still to be armed (arm_next).  The
// first llampc_ctl_wait of a step arms them ALL before it spins: with two tracks (tick_async on
// both, then wait on both) the second controller's launch call would otherwise sit between the
// first's result and its own (~5 us on the two-track step).  The arming pass holds g_arm_mu
// throughout and only try-locks the controllers it visits; llampc_ctl_destroy removes its
// controller under g_arm_mu before anything is freed, so the pass never holds a controller that
// is being destroyed.
static std::mutex g_arm_mu;
static std::vector<llampc_ctl*> g_arm_list;
static void arm_list_add(llampc_ctl* c) {
  std::lock_guard<std::mutex> g(g_arm_mu);
  g_arm_list.push_back(c);
}
static void arm_list_remove(llampc_ctl* c) {
  std::lock_guard<std::mutex> g(g_arm_mu);
  g_arm_list.erase(std::remove(g_arm_list.begin(), g_arm_list.end(), c), g_arm_list.end());
}

// A failed controller tick (a wait that gave up, or a completion that never arrived): once the
// stream has drained, the look-back ticket is zeroed so the next launch's ticket_last counts
// from 0.  The tick still consumed its step on the device (the window slot, the tick number);
// the Python controller refuses further ticks until it is rebuilt (LLAMPC.tick).
static int ctl_recover(llampc_ctl* c) {
  ctl_cancel(c);                         // an armed launch behind the failed one exits at once
  HIP_TRY(hipStreamSynchronize(c->b->stream));
  HIP_TRY(hipMemsetAsync(c->d_tickets.get(), 0, 2 * sizeof(unsigned), c->b->stream));
  HIP_TRY(hipStreamSynchronize(c->b->stream));
  return LLAMPC_OK;
}

extern "C" {

int llampc_ctl_destroy(llampc_ctl* c) {
  if (!c) return LLAMPC_OK;
  arm_list_remove(c);
  ctl_cancel(c);
  DeviceGuard g(c->b->device);
  if (c->b->stream) (void)hipStreamSynchronize(c->b->stream);
  delete c;
  return LLAMPC_OK;
}

int llampc_ctl_create(llampc_bank* b, const llampc_ctl_cfg* cfg, const double* points, int32_t np,
                      const double* prefix, llampc_ctl** out) {
  if (!out) return fail(LLAMPC_E_ARG, "out is NULL");
  *out = nullptr;
  if (!b || !cfg || !points || !prefix) return fail(LLAMPC_E_ARG, "NULL argument");
  const llampc_ctl_cfg& k = *cfg;
  if (k.C < 1 || k.H < 1 || k.H > LLAMPC_HMAX || k.K < 1 || k.K > LLAMPC_KMAX)
    return fail(LLAMPC_E_ARG, "C=%d H=%d (1..%d) K=%d (1..%d)", k.C, k.H, LLAMPC_HMAX, k.K, LLAMPC_KMAX);
  if (k.S < 1 || k.S > kCtlSMax) return fail(LLAMPC_E_ARG, "S=%d outside [1, %d]", k.S, kCtlSMax);
  if (!(k.Ts > 0) || !std::isfinite(k.Ts)) return fail(LLAMPC_E_ARG, "Ts must be finite > 0");
  if (np < 2) return fail(LLAMPC_E_ARG, "np=%d < 2", np);
  if (k.nan_policy != LLAMPC_NAN_FIRST && k.nan_policy != LLAMPC_NAN_IGNORE) return fail(LLAMPC_E_ARG, "nan_policy");
  if (!b->d_rl) return fail(LLAMPC_E_STATE, "the controller needs the bank's raceline (llampc_bank_set_raceline)");
  const int R = lookback_r(b->n, k.K);
  const int nb_lb = lookback_blocks_r(b->n, R);
  size_t poll_off = 0;
  const size_t lds = ctl_lds_bytes(k.H, k.C, b->rl_n, nb_lb, k.K, &poll_off);
  if (lds > 160 * 1024)
    return fail(LLAMPC_E_ARG, "controller tick needs %zu B of LDS (> 160 KiB): C*H=%d too large for this track", lds,
                k.C * k.H);
  DeviceGuard g(b->device);
  Building<llampc_ctl> c(new llampc_ctl(), llampc_ctl_destroy);
  c->b = b;
  c->cfg = k;
  if (const char* e = std::getenv("LLAMPC_CTL_NO_STAGE")) c->no_stage = e[0] == '1';
  c->np = np;
  const size_t nslots = kCtlSlotsMax, nspec = kCtlSpecMax;
  int rc;
  if ((rc = c->d_st.alloc(1)) || (rc = c->d_pts.alloc(3 * (size_t)np - 1)) || (rc = c->d_sel_tag.zalloc(nslots)) ||
      (rc = c->d_slot_tag.zalloc(4 * nslots)) || (rc = c->d_tickets.zalloc(2)) ||
      (rc = c->d_znoise.alloc(4 * (size_t)k.C * k.H)) || (rc = c->d_ztag.zalloc(2)) || (rc = c->d_door_dev.zalloc(16)) ||
      (rc = c->d_spec_val.alloc((size_t)nb_lb * nspec)) || (rc = c->d_spec_idx.alloc((size_t)nb_lb * nspec)) ||
      (rc = c->d_spec_tag.zalloc(nspec)) || (rc = c->d_spec_res.zalloc(4 * nspec)) ||
      (rc = c->d_xref_tag.zalloc(4 * (size_t)(LLAMPC_HMAX + 1))) ||
      (k.debug_inputs && (rc = c->d_dbg.alloc(2 * (size_t)(k.H + 1) + 2 * (size_t)k.C * k.H))) ||
      (rc = c->host.alloc("controller record")) || (rc = c->door.alloc(16, "controller doorbell")))
    return rc;
  c->spec_nb = nb_lb;
  if (const char* e = std::getenv("LLAMPC_CTL_NO_SPEC")) c->no_spec = e[0] == '1';
  if (const char* e = std::getenv("LLAMPC_CTL_SPEC_N")) c->spec_cap = std::max(1, std::min(kCtlSpecMax, std::atoi(e)));
  CtlState st{};
  st.mu_pred = std::nan("");
  st.current_model = 0;                  // rt.py:264: the nominal model's index
  double* pts = c->d_pts.get();
  if (hipMemcpy(c->d_st.get(), &st, sizeof st, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(pts, points, 2 * (size_t)np * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(pts + 2 * (size_t)np, prefix, ((size_t)np - 1) * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess)
    return fail(LLAMPC_E_HIP, "controller upload failed");
  *out = c.release();
  return LLAMPC_OK;
}

}  // extern "C"

// The host copies a launched tick reads: the peers' mailbox table on the device, and after a
// failed wait the state's projidx / mu-hat.  The caller holds c->b->mu and, with a peer
// exchange, c->mb->mu.
static int ctl_refresh(llampc_ctl* c, bool launched) {
  if (launched && !c->hint_ok) {
    CtlState hs{};
    HIP_TRY(hipStreamSynchronize(c->b->stream));
    HIP_TRY(hipMemcpy(&hs, c->d_st.get(), sizeof hs, hipMemcpyDeviceToHost));
    c->hint_p0 = hs.projidx;
    c->hint_mu = hs.mu_pred;
    c->hint_ok = true;
  }
  return c->mb ? mailbox_sync(c->mb) : LLAMPC_OK;
}

// The launch of tick c->t (x_t null: armed — the doorbell carries x_t) and what it commits
// (ctl_commit), from the host's copy of the controller and bank state (after ctl_refresh): no
// HIP call.  An armed prepare takes the next doorbell number.
static int ctl_prepare(llampc_ctl* c, const double* x_t, llampc_ctl::Prep& P) {
  llampc_bank* b = c->b;
  const llampc_ctl_cfg& k = c->cfg;
  const int64_t t = c->t;
  const int32_t W = b->W;
  const bool do_lb = t >= 2;             // rt.py:347 (the transition idt -> idt+1 from idt >= 1)
  const bool warm = t <= W;              // rt.py:300-301
  int32_t count = b->count;
  if (do_lb) count = std::min(count + 1, W);
  const bool full = do_lb && count >= W;
  if (!warm && !full)
    return fail(LLAMPC_E_STATE, "tick %lld: the look-back window is not full after the warm-up (was the bank reset?)",
                (long long)t);
  CtlLaunch L{};
  const BankView bv = bank_view(*b);
  const int R = lookback_r(b->n, k.K);
  // look-back (rt.py:347-366 on the bank's ring)
  bank_lookback(bv, L.lb);
  L.lb.x_prev = c->d_st.get()->x_prev;
  L.lb.u_prev = c->d_st.get()->u_prev;
  L.lb.Ts = k.Ts;
  L.lb.full = full;
  L.lb.K = k.K;
  L.lb.nan_first = k.nan_policy == LLAMPC_NAN_FIRST;
  L.lb.R = R;
  L.lb.wm_keep = 0;
  // look-ahead constants (RK4 on the bank's vehicle, the NLP objective)
  bank_lookahead(bv, LLAMPC_RK4, L.la);
  L.la.C = k.C;
  L.la.H = k.H;
  L.la.Ts = k.Ts;
  L.la.cost = make_cost(k.cost, k.Ts);
  L.la.xref_mode = LLAMPC_XREF_GIVEN;
  L.la.rl = raceline_view(bv);
  L.la.rl.wcap = b->rl_n - 1;
  // lb_final's view
  bank_final(bv, L.fin);
  L.fin.out = &c->host.rec.dev()->plan;
  L.fin.do_lb = do_lb;
  L.fin.do_la = 1;
  L.fin.full = full;
  L.fin.window_count = do_lb ? count : b->count;
  L.fin.K = k.K;
  L.fin.nan_first = k.nan_policy == LLAMPC_NAN_FIRST;
  L.fin.nb_lb = do_lb ? lookback_blocks_r(b->n, R) : 1;
  L.fin.C = k.C;
  // controller
  const uint64_t hs = c->hseq + 1;
  const uint32_t seq = next_seq(c->seq);
  L.st = c->d_st.get();
  L.out = c->host.rec.dev();
  L.host_tag = c->host.tag.dev();
  L.host_seq = hs;
  L.sel_tag = c->d_sel_tag.get();
  L.slot_tag = c->d_slot_tag.get();
  L.tickets = c->d_tickets.get();
  L.dbg = c->d_dbg.get();
  L.znoise = c->d_znoise.get();
  L.ztag = c->d_ztag.get();
  L.pts = c->d_pts.get();
  L.prefix = c->d_pts.get() + 2 * (size_t)c->np;
  L.tick = (uint64_t)t;
  L.seed = k.seed;
  for (int j = 0; j < 6; ++j) {
    L.x_t[j] = x_t ? x_t[j] : 0.0;      // armed (x_t null): the doorbell carries it
    L.nominal[j] = k.nominal[j];
  }
  const double sqrt3 = std::sqrt(3.0);
  for (int j = 0; j < 2; ++j) {
    L.nscale[j] = sqrt3 * k.sigma[j];    // sqrt(3) sigma_j, one rounding (ctl.hpp ctl_cand_one)
    L.rate[j] = k.cost.rate_max[j] < 0 ? -1.0 : k.cost.rate_max[j] * k.Ts;
    L.umin[j] = k.cost.umin[j];
    L.umax[j] = k.cost.umax[j];
  }
  L.mu_fixed = 1.0;                      // ConstantSpeed's defaults (rt.py:282)
  L.scale_fixed = 1.0;
  L.v_factor = k.v_factor;
  L.mu_init = k.mu_init;
  L.seq = seq;
  L.poll = (uint32_t)poll_units(poll_bound_ticks(b->n, k.C, k.H), UINT32_MAX);
  L.np = c->np;
  L.lap_projidx = k.lap_projidx;
  L.do_lb = do_lb;
  L.warm = warm;
  L.use_mu = t > W + 1;                  // rt.py:278
  L.door_dev = c->d_door_dev.get();      // every launch: its x_t time (kCtlTimeWord)
  if (!x_t) {                            // armed: the launch reads projidx / mu-hat from the state
    L.door = c->door.dev();
    c->door_ctr = c->door_ctr == 0xFFFFFFFFu ? 1u : c->door_ctr + 1u;
    L.door_seq = c->door_ctr;
    L.door_bound = (uint32_t)(kArmBoundS * 1e8 / 65536.0) + 1;
  } else {                               // the last record's (ctl_refresh after a failed wait)
    L.p0_walk = c->hint_p0;
    L.br_walk = mu_bracket(b->rl_mus.data(), b->rl_M, L.use_mu ? c->hint_mu : L.mu_fixed);   // rt.py:278-282
  }
  L.full = full;
  L.S = k.S;
  L.K = k.K;
  // sharded: the exchange runs on every tick whose window is full (the same ticks on every
  // rank); the selection is global, the look-ahead reads the replicated global table
  L.sel_goff = b->goff;
  uint32_t px_seq = 0;
  if (c->mb || c->xg_world) {            // (the caller holds mb->mu)
    L.la.params = c->d_gparams.get();
    L.la.n = c->n_global;
    L.la.goff = 0;
    L.sel_goff = 0;
  }
  if (c->mb) {
    llampc_mailbox* mb = c->mb;
    if (full) {
      px_seq = next_seq(mb->seq);
      L.px_box = mb->d_box.get();
      L.px_G = mb->world;
      L.px_rank = mb->rank;
      L.px_seq = px_seq;
      L.px_bound = (uint32_t)poll_units(mb->bound, UINT32_MAX);
      L.poll = std::max(L.poll, L.px_bound);   // the look-ahead blocks wait for the merged selection
    }
  } else if (c->xg_world && full) {      // gather transport: two launches (CtlLaunch.px_phase)
    px_seq = next_seq(c->xg_seq);
    L.px_G = c->xg_world;
    L.px_rank = c->xg_rank;
    L.px_seq = px_seq;
    L.px_phase = 1;
    L.px_send = c->d_xsend.get();
    L.px_gath = c->d_xgath.get();
    L.px_bound = 16;                     // ~10 ms: the records are there when the launch starts
  }
  // the launch's shape (capi_host.hpp ctl_shape: the lane split, the staging, the block counts)
  // a corridor tick (llampc_ctl_set_corridor, weight > 0): ctl_kernel_corr — never staged, H corridor
  // blocks, no speculative blocks (L.s4 = 0 rules them out below)
  const bool corr = c->cor_w > 0;
  const CtlShape V = ctl_shape(b->n, k.C, k.H, k.K, b->rl_n, warm, do_lb, c->no_stage, L.px_G, corr ? c->tr_n : 0);
  const int lpm = V.lpm;
  L.nslots = V.nslots;
  L.G = V.G;
  L.cpl = V.cpl;
  L.mpb = V.mpb;
  L.nb_lb = V.nb_lb;
  L.nb_la = V.nb_la;
  L.s4 = V.s4;
  L.poll_off = V.poll_off;
  size_t lds = V.lds;
  if (lds > kCtlLdsMax) return fail(LLAMPC_E_ARG, "controller tick needs %zu B of LDS (> 160 KiB)", lds);
  // the speculative look-ahead (CtlLaunch.n_spec): armed ticks past the warm-up whose rollouts
  // are one model per block in fused quads with diagonal Q / P (the spec blocks' layout)
  {
    const llampc_cost& cq = k.cost;
    const bool diag = cq.Q[1] == 0.0 && cq.Q[2] == 0.0 && cq.P[1] == 0.0 && cq.P[2] == 0.0;
    // sharded over the peer mailboxes: the ranks' lists are exchanged too (ctl.hip
    // ctl_spec_exchange), in the slot after the selection record's words
    // the armed footprint: every block of an armed launch holds a CU from the end of the tick
    // before to its doorbell, and all launches of the banks ticked together
    // (llampc_bank_set_concurrency) must be resident at once — the exchange's peers and the
    // tick's own look-back wait on each other — so the spec blocks take what is left of the
    // banks' share of the CUs (INTEGRATION.md "What armed launches cost")
    const int cus = b->cus >= 1 ? b->cus : 256;
    const int room = cus / std::max(1, b->share) - (L.nb_lb + L.nb_la);
    const int ns = (int)std::min<int64_t>(std::min<int64_t>(c->spec_cap, room), c->mb ? c->n_global : b->n);
    const int spec_off = ctl_rec_words(k.K);
    const bool px_fits = !c->mb || (L.px_G && spec_off + 4 * ns <= kRecWords);
    if (!x_t && !c->no_spec && !warm && full && R == 1 && L.s4 && lpm == 4 && L.cpl == 1 && L.G == k.C && diag &&
        !c->xg_world && px_fits && ns >= 4 && L.nb_lb <= c->spec_nb) {
      size_t poll_sp = 0;
      const size_t lds_sp = ctl_lds_bytes(k.H, k.C, b->rl_n, L.nb_lb, k.K, &poll_sp, true, L.px_G, ns);
      if (lds_sp <= 160 * 1024) {
        L.px_spec_off = spec_off;
        L.px_spec_wait = 20000;           // 200 us: the ranks arm within microseconds of each other
        L.n_spec = ns;
        L.spec_val = c->d_spec_val.get();
        L.spec_idx = c->d_spec_idx.get();
        L.spec_tag = c->d_spec_tag.get();
        L.spec_res = c->d_spec_res.get();
        L.xref_tag = c->d_xref_tag.get();
        L.poll_off = poll_sp;
        lds = lds_sp;
      }
    }
  }
  lds = std::max<size_t>(lds, 82 * 1024); // one block per CU, as the plan launch (sc1 hand-offs)
  P.corr = corr;
  if (corr) {
    // the path state and the read-back by tick parity (ctl.hpp CtlCorridor): tick t reads what tick
    // t - 1 wrote and writes its own copy
    CtlCorridor& q = P.cor;
    const double* tr = c->d_track.get();
    const size_t tn = (size_t)c->tr_n, ps = 2 * (size_t)kCtlPathStride;
    const int wr = (int)(t & 1), rd = wr ^ 1;
    q = CtlCorridor{};
    q.trk = TrackK{tr, tr + tn, tr + 2 * tn, c->tr_n, 0, c->tr_L};
    q.hw = c->tr_width / 2 - c->cor_margin;
    q.weight = c->cor_w;
    q.hp_tag = c->d_hp_tag.get();
    q.path_rd = c->d_cor.get() + rd * ps;
    q.path_wr = c->d_cor.get() + wr * ps;
    q.valid_rd = c->d_cor_flag.get() + rd;
    q.valid_wr = c->d_cor_flag.get() + wr;
    q.dbg = c->d_cor.get() + 2 * ps + (size_t)wr * kCtlCorDbgDoubles;
    q.dbg_valid = c->d_cor_flag.get() + 2 + wr;
    q.path_ok = c->cor_prev ? 1 : 0;
    q.dbg_cost = c->d_cor_cost.get();
  }
  P.L = L;
  P.lpm = lpm;
  P.lds = lds;
  P.hs = hs;
  P.seq = seq;
  P.px_seq = px_seq;
  P.t = t;
  P.do_lb = do_lb;
  P.count = count;
  return LLAMPC_OK;
}

// A prepared tick's one launch: the corridor kernel for a corridor tick.
static hipError_t ctl_launch(const llampc_ctl::Prep& P, hipStream_t s) {
  return P.corr ? launch_ctl_corr(P.L, P.cor, P.lpm, P.lds, s) : launch_ctl(P.L, P.lpm, P.lds, s);
}

// The host state after tick P.t was enqueued (or its armed launch fired).
static void ctl_commit(llampc_ctl* c, const llampc_ctl::Prep& P) {
  llampc_bank* b = c->b;
  c->cor_prev = P.corr;
  c->cor_nslots = P.corr ? P.L.nslots : 0;
  c->hseq = P.hs;
  c->seq = P.seq;
  if (P.L.px_G) {                        // committed after the launch was enqueued (next_seq)
    if (c->mb) c->mb->seq = P.px_seq;
    else c->xg_seq = P.px_seq;
  }
  c->t = P.t + 1;
  c->pending = true;
  c->pend_seq = P.hs;
  b->launches++;
  if (P.do_lb) {
    b->slot = (b->slot + 1) % b->W;
    b->count = P.count;
  }
}

// Enqueues tick c->t's launch armed (llampc_ctl_set_prelaunch): it runs behind the tick in
// flight and waits for the doorbell.  The caller holds c->mu, c->b->mu and, with a peer
// exchange, c->mb->mu.  With the peer exchange the armed launch takes the mailbox's next tick
// number (the exchange runs after its doorbell, inside it); the number is committed only when
// the doorbell fires (ctl_commit), so a cancelled armed launch — which exits before the doorbell,
// never pushing — leaves the sequence to its relaunch, and the ranks' sequences stay in step
// whichever of them armed, fired or relaunched.  Not with a gather transport (two launches).
static int ctl_arm(llampc_ctl* c) {
  if (c->armed || c->xg_world) return LLAMPC_OK;
  if (!c->b->own_stream || !c->b->dedicated)   // the stream changed since set_prelaunch
    return fail(LLAMPC_E_STATE, "an armed launch needs the bank's own dedicated-queue stream");
  llampc_ctl::Prep P;
  int rc;
  if ((rc = ctl_refresh(c, false)) || (rc = ctl_prepare(c, nullptr, P))) return rc;
  HIP_TRY(ctl_launch(P, c->b->stream));
  c->arm = P;
  c->armed = true;
  c->arm_t = std::chrono::steady_clock::now();
  c->b->armed = c;
  return LLAMPC_OK;
}

// After a tick was enqueued or rung: its successor is armed by the step's first wait.
static void ctl_arm_later(llampc_ctl* c) {
  c->arm_next = c->prelaunch;
  if (c->arm_next) arm_list_add(c);
}

extern "C" {

int llampc_ctl_tick_async(llampc_ctl* c, const double* x_t) {
  if (!c || !x_t) return fail(LLAMPC_E_ARG, "controller/x_t is NULL");
  std::lock_guard<std::mutex> lc(c->mu);
  if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding: call llampc_ctl_wait");
  llampc_bank* b = c->b;
  std::lock_guard<std::mutex> lk(b->mu);
  if (b->async_pending) return fail(LLAMPC_E_STATE, "an async plan tick is outstanding on the bank");
  DeviceGuard g(b->device);
  std::unique_lock<std::mutex> lm;
  if (c->mb) lm = std::unique_lock<std::mutex>(c->mb->mu);
  if (c->armed) {
    const double age = std::chrono::duration<double>(std::chrono::steady_clock::now() - c->arm_t).count();
    // (with a peer exchange the armed launch's tick number must still be the mailbox's next)
    const bool px_ok = !c->arm.L.px_G || !c->mb || c->arm.px_seq == next_seq(c->mb->seq);
    if (age < kArmFreshS && c->arm.t == c->t && px_ok) {
      // fire: every word tagged (block 0 polls until all carry the tag: no order needed)
      const uint64_t tg = (uint64_t)c->arm.L.door_seq << 32;
      uint64_t* door = c->door.get();
      for (int j = 0; j < 6; ++j) {
        uint64_t w;
        std::memcpy(&w, &x_t[j], 8);
        __atomic_store_n(&door[2 * j], tg | (w >> 32), __ATOMIC_RELAXED);
        __atomic_store_n(&door[2 * j + 1], tg | (w & 0xFFFFFFFFull), __ATOMIC_RELAXED);
      }
      __atomic_store_n(&door[kCtlDoorWords - 1], tg | kCtlDoorFire, __ATOMIC_RELEASE);
      c->armed = false;
      b->armed = nullptr;
      ctl_commit(c, c->arm);
      ctl_arm_later(c);
      return LLAMPC_OK;
    }
    ctl_cancel(c);                       // stale: this tick launches normally
  }
  llampc_ctl::Prep P;
  int rc;
  if ((rc = ctl_refresh(c, true)) || (rc = ctl_prepare(c, x_t, P))) return rc;
  if (P.L.px_phase == 1) {               // gather transport: the look-back launch, the gather, the rest
    llampc_ctl::Prep P2 = P;
    P2.L.px_phase = 2;
    P2.L.nb_lb = 1;                      // block 0 merges and completes
    llampc_ctl::Prep P1 = P;
    P1.L.nb_la = 0;                      // the look-back blocks alone
    P1.L.n_spec = 0;
    {
      TimedLaunch tl(b, 0, b->stream);
      HIP_TRY(launch_ctl(P1.L, P1.lpm, P1.lds, b->stream));
      if (c->xg_comm) {
        if ((rc = comm_all_gather(c->xg_comm, c->d_xsend.get(), c->d_xgath.get(), (size_t)c->xg_nw, true, b->stream)))
          return rc;
        HIP_TRY(launch_ctl(P2.L, P2.lpm, P2.lds, b->stream));
      }
    }
    ctl_commit(c, P);
    if (!c->xg_comm) {                   // the caller carries the records (llampc_ctl_resume)
      c->xg_second = P2;
      c->xg_wait = true;
      c->xg_read = false;
      return LLAMPC_OK;
    }
    ctl_arm_later(c);
    return LLAMPC_OK;
  }
  {
    TimedLaunch tl(b, 0, b->stream);
    HIP_TRY(ctl_launch(P, b->stream));
  }
  ctl_commit(c, P);
  ctl_arm_later(c);
  return LLAMPC_OK;
}

int llampc_ctl_wait(llampc_ctl* c, llampc_ctl_out* out) {
  if (!c || !out) return fail(LLAMPC_E_ARG, "controller/out is NULL");
  std::lock_guard<std::mutex> lc(c->mu);
  if (!c->pending) return fail(LLAMPC_E_STATE, "no controller tick outstanding");
  if (c->xg_wait) return fail(LLAMPC_E_STATE, "the tick's records are not gathered yet: call llampc_ctl_resume");
  c->pending = false;
  c->hint_ok = false;                    // until this tick's record is read
  DeviceGuard g(c->b->device);
  {
    // the next ticks' launches, armed behind the ones in flight — here rather than in
    // tick_async, so that several controllers' ticks (two tracks) are all rung before any
    // launch call, and for every rung controller at once (g_arm_list); the launch calls overlap
    // the device time.  Another controller is armed only if its locks are free (else its own
    // wait arms it).  A failed arm only turns prelaunch off.
    std::lock_guard<std::mutex> ga(g_arm_mu);
    std::vector<llampc_ctl*> keep;
    for (llampc_ctl* x : g_arm_list) {
      const bool self = x == c;
      if (!self && !x->mu.try_lock()) {
        keep.push_back(x);
        continue;
      }
      if (x->arm_next) {
        if (x->b->mu.try_lock()) {
          if (!x->mb || x->mb->mu.try_lock()) {
            x->arm_next = false;
            DeviceGuard gx(x->b->device);
            if (!x->b->async_pending && ctl_arm(x) != LLAMPC_OK) x->prelaunch = false;
            if (x->mb) x->mb->mu.unlock();
          } else {
            keep.push_back(x);
          }
          x->b->mu.unlock();
        } else {
          keep.push_back(x);
        }
      }
      if (!self) x->mu.unlock();
    }
    g_arm_list.swap(keep);
  }
  const uint64_t* tag = c->host.tag.get();
  const int rc = spin_for_tag(
      tag, c->pend_seq,
      [&]() -> int {
        ctl_cancel(c);
        HIP_TRY(hipStreamSynchronize(c->b->stream));
        return LLAMPC_OK;
      },
      [&](uint64_t v) { return v == (c->pend_seq | kCtlTagExpired); });   // an armed launch that never saw its doorbell
  if (rc == kSpinStopped || rc == kSpinTimeout) {
    (void)ctl_recover(c);
    return fail(LLAMPC_E_DEVICE, rc == kSpinStopped ? "controller tick %llu: the armed launch expired before its doorbell"
                                                    : "controller tick %llu: completion tag never arrived",
                (unsigned long long)c->pend_seq);
  }
  if (rc) return rc;
  std::memcpy(out, const_cast<const llampc_ctl_out*>(c->host.rec.get()), sizeof(llampc_ctl_out));
  c->dev_ticks = __atomic_load_n(tag + 1, __ATOMIC_RELAXED);
  if (out->plan.status) {
    (void)ctl_recover(c);
    return fail(LLAMPC_E_DEVICE, "controller tick record status %d (an in-launch wait timed out)", out->plan.status);
  }
  c->hint_p0 = out->projidx;             // the state this tick left (ctl_complete writes both)
  c->hint_mu = out->mu_pred;
  c->hint_ok = true;
  return LLAMPC_OK;
}

int llampc_ctl_device_us(llampc_ctl* c, double* us) {
  if (!c || !us) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lc(c->mu);
  *us = c->dev_ticks ? (double)c->dev_ticks * 1e-2 : std::nan("");   // s_memrealtime: 100 MHz
  return LLAMPC_OK;
}

int llampc_ctl_set_prelaunch(llampc_ctl* c, int32_t on) {
  if (!c) return fail(LLAMPC_E_ARG, "controller is NULL");
  std::lock_guard<std::mutex> lc(c->mu);
  if (on && c->xg_world) return fail(LLAMPC_E_STATE, "prelaunch is not available with a gather transport");
  llampc_bank* b = c->b;
  std::lock_guard<std::mutex> lk(b->mu);
  DeviceGuard g(b->device);
  if (on) {
    if (!b->own_stream)
      return fail(LLAMPC_E_STATE, "prelaunch needs the bank's own stream (the bank launches on a caller's stream)");
    if (!b->dedicated) {                  // an armed launch must not sit on a shared hardware queue
      bank_disarm(b);
      if (int rc = bank_dedicate(b)) return rc;
    }
  }
  c->prelaunch = on != 0;
  c->arm_next = c->prelaunch && c->pending;   // a tick in flight: armed by its wait
  if (c->arm_next) arm_list_add(c);
  if (!c->prelaunch) {
    ctl_cancel(c);
    return LLAMPC_OK;
  }
  if (c->pending || b->async_pending) return LLAMPC_OK;
  bank_disarm(b);                         // another controller's launch on this bank
  std::unique_lock<std::mutex> lm;
  if (c->mb) lm = std::unique_lock<std::mutex>(c->mb->mu);
  return ctl_arm(c);
}

int llampc_ctl_tick(llampc_ctl* c, const double* x_t, llampc_ctl_out* out) {
  if (!out) return fail(LLAMPC_E_ARG, "out is NULL");
  int rc = llampc_ctl_tick_async(c, x_t);
  return rc ? rc : llampc_ctl_wait(c, out);
}

int llampc_ctl_reference(llampc_ctl* c, const double* x0, double v0, int32_t H, int32_t projidx, double curr_mu,
                         double scale, double* xref, int32_t* projidx_out, double* vr) {
  if (!c || !x0 || !xref) return fail(LLAMPC_E_ARG, "NULL argument");
  if (H < 1 || H > LLAMPC_HMAX) return fail(LLAMPC_E_ARG, "H=%d outside [1, %d]", H, LLAMPC_HMAX);
  if (projidx < 0 || projidx > c->np - 2) return fail(LLAMPC_E_ARG, "projidx=%d outside [0, %d]", projidx, c->np - 2);
  std::lock_guard<std::mutex> lc(c->mu);
  llampc_bank* b = c->b;
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  DeviceGuard g(b->device);
  const size_t n = 2 * (size_t)(H + 1) + 2;
  DevBuf<double> d;
  if (int rc = d.alloc(n)) return rc;
  CsLaunch a{};
  a.rl = raceline_view(bank_view(*b));
  a.pts = c->d_pts.get();
  a.prefix = c->d_pts.get() + 2 * (size_t)c->np;
  a.out = d.get();
  a.x0 = x0[0];
  a.y0 = x0[1];
  a.v0 = v0;
  a.mu = curr_mu;
  a.scale = scale;
  a.Ts = c->cfg.Ts;
  a.np = c->np;
  a.p0 = projidx;
  a.H = H;
  std::vector<double> h(n);
  hipError_t e = launch_constant_speed(a, b->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d.get(), n * sizeof(double), hipMemcpyDeviceToHost, b->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  if (e != hipSuccess) return fail(LLAMPC_E_HIP, "llampc_ctl_reference: %s", hipGetErrorString(e));
  std::memcpy(xref, h.data(), 2 * (size_t)(H + 1) * sizeof(double));
  if (projidx_out) *projidx_out = (int32_t)h[2 * (H + 1)];
  if (vr) *vr = h[2 * (H + 1) + 1];
  return LLAMPC_OK;
}

}  // extern "C"

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

// The shape ctl_prepare gives a tick past the warm-up (unsharded), from the same ctl_shape.
int llampc_ctl_variant(int64_t n, int32_t C, int32_t H, int32_t K, int32_t rl_n, int32_t out[9]) {
  if (!out) return fail(LLAMPC_E_ARG, "NULL argument");
  // C beyond kCtlVariantCMax: the candidates alone (16 B each per step) exceed the CU's LDS, and the
  // int products C * H below stay far from overflow
  constexpr int32_t kCtlVariantCMax = 1 << 16;
  if (n < 1 || C < 1 || C > kCtlVariantCMax || H < 1 || H > LLAMPC_HMAX || K < 1 || K > LLAMPC_KMAX || rl_n < 2)
    return fail(LLAMPC_E_ARG, "n=%lld C=%d (1..%d) H=%d (1..%d) K=%d (1..%d) rl_n=%d", (long long)n, C, kCtlVariantCMax,
                H, LLAMPC_HMAX, K, LLAMPC_KMAX, rl_n);
  bool no_stage = false;
  if (const char* e = std::getenv("LLAMPC_CTL_NO_STAGE")) no_stage = e[0] == '1';
  const CtlShape V = ctl_shape(n, C, H, K, rl_n, false, true, no_stage, 0);
  if (V.lds > kCtlLdsMax)                // llampc_ctl_create refuses the shape
    return fail(LLAMPC_E_ARG, "controller tick needs %zu B of LDS (> 160 KiB): C*H=%d too large for this track", V.lds,
                C * H);
  const int32_t v[9] = {V.lpm, V.G, V.cpl, V.mpb, V.s4, V.zfit, V.R, V.nb_lb, V.nb_la};
  std::memcpy(out, v, sizeof v);
  return LLAMPC_OK;
}

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
  const llampc_ctl::Prep& P2 = c->xg_second;
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

int llampc_ctl_set_track(llampc_ctl* c, const double* centre, const double* theta, int32_t n, double track_length,
                         double track_width) {
  if (!c || !centre || !theta) return fail(LLAMPC_E_ARG, "NULL argument");
  char why[128];
  if (track_tables_invalid(centre, theta, n, track_length, track_width, why, sizeof why)) return fail(LLAMPC_E_ARG, "%s", why);
  std::lock_guard<std::mutex> lc(c->mu);
  if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding");
  if (c->cor_w > 0) return fail(LLAMPC_E_STATE, "switch the corridor off before replacing its track");
  llampc_bank* b = c->b;
  std::lock_guard<std::mutex> lk(b->mu);
  bank_disarm(b);
  DeviceGuard g(b->device);
  HIP_TRY(hipStreamSynchronize(b->stream));      // no launch reads the tables being replaced
  c->tr_n = 0;
  if (int rc = c->d_track.reserve(3 * (size_t)n, 0, "track tables")) return rc;
  std::vector<double> h(3 * (size_t)n);
  std::memcpy(h.data(), centre, 2 * (size_t)n * sizeof(double));
  std::memcpy(h.data() + 2 * (size_t)n, theta, (size_t)n * sizeof(double));
  HIP_TRY(hipMemcpy(c->d_track.get(), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  c->tr_n = n;
  c->tr_L = track_length;
  c->tr_width = track_width;
  return LLAMPC_OK;
}

int llampc_ctl_set_corridor(llampc_ctl* c, double weight, double margin) {
  if (!c) return fail(LLAMPC_E_ARG, "controller is NULL");
  std::lock_guard<std::mutex> lc(c->mu);
  ctl_cancel(c);                         // as every other call: the tick after launches normally
  if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding");
  if (!c->tr_n) return fail(LLAMPC_E_STATE, "no track set: call llampc_ctl_set_track first");
  if (c->mb || c->xg_world) return fail(LLAMPC_E_STATE, "a sharded controller has no corridor ticks");
  if (!(weight >= 0) || !std::isfinite(weight)) return fail(LLAMPC_E_ARG, "weight must be finite and >= 0");
  if (!std::isfinite(margin) || !(c->tr_width / 2 - margin > 0))
    return fail(LLAMPC_E_ARG, "margin %g leaves no corridor (track width %g)", margin, c->tr_width);
  if (weight > 0) {
    llampc_bank* b = c->b;
    const llampc_ctl_cfg& k = c->cfg;
    const CtlShape V = ctl_shape(b->n, k.C, k.H, k.K, b->rl_n, false, true, c->no_stage, 0, c->tr_n);
    if (V.lds > kCtlLdsMax) return fail(LLAMPC_E_ARG, "a corridor tick needs %zu B of LDS (> 160 KiB)", V.lds);
    if (!c->d_cor) {
      DeviceGuard g(b->device);
      DevBuf<double> cor;
      DevBuf<uint64_t> tag;
      DevBuf<int32_t> flag;
      int rc;
      if ((rc = cor.zalloc(4 * (size_t)kCtlPathStride + 2 * (size_t)kCtlCorDbgDoubles, "corridor path state")) ||
          (rc = tag.zalloc(12 * (size_t)LLAMPC_HMAX, "corridor words")) || (rc = flag.zalloc(4, "corridor flags")))
        return rc;
      c->d_cor = std::move(cor);
      c->d_hp_tag = std::move(tag);
      c->d_cor_flag = std::move(flag);
    }
    if (k.debug_inputs && !c->d_cor_cost) {
      DeviceGuard g(b->device);
      if (int rc = c->d_cor_cost.zalloc((size_t)kCtlSlotsMax * k.C, "corridor costs")) return rc;
    }
  } else {
    c->cor_prev = false;                 // off: the path state is invalid from here on
  }
  c->cor_w = weight;
  c->cor_margin = margin;
  return LLAMPC_OK;
}

int llampc_ctl_corridor(llampc_ctl* c, double* path, double* hp, double* theta, int32_t* valid) {
  if (!c || !path || !hp || !theta || !valid) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lc(c->mu);
  if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding");
  if (!c->d_cor || !c->cor_prev) return fail(LLAMPC_E_STATE, "the last tick was not a corridor tick");
  DeviceGuard g(c->b->device);
  ctl_cancel(c);                         // an armed launch would hold the stream (re-armed next tick)
  HIP_TRY(hipStreamSynchronize(c->b->stream));
  const int H = c->cfg.H;
  const int cp = (int)((c->t - 1) & 1);  // the last tick's copy
  std::vector<double> h(kCtlCorDbgDoubles);
  int32_t v = 0;
  HIP_TRY(hipMemcpy(h.data(), c->d_cor.get() + 4 * (size_t)kCtlPathStride + (size_t)cp * kCtlCorDbgDoubles,
                    h.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&v, c->d_cor_flag.get() + 2 + cp, sizeof v, hipMemcpyDeviceToHost));
  for (int r = 0; r < 2; ++r) std::memcpy(path + (size_t)r * (H + 1), h.data() + (size_t)r * kCtlPathStride, (H + 1) * sizeof(double));
  std::memcpy(hp, h.data() + 2 * kCtlPathStride, 6 * (size_t)H * sizeof(double));
  std::memcpy(theta, h.data() + 2 * kCtlPathStride + 6 * LLAMPC_HMAX, (size_t)H * sizeof(double));
  *valid = v;
  return LLAMPC_OK;
}

int llampc_ctl_corridor_costs(llampc_ctl* c, double* costs, int32_t* nslots) {
  if (!c || !costs || !nslots) return fail(LLAMPC_E_ARG, "NULL argument");
  std::lock_guard<std::mutex> lc(c->mu);
  if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding");
  if (!c->d_cor_cost) return fail(LLAMPC_E_STATE, "controller created without debug_inputs");
  if (!c->cor_prev) return fail(LLAMPC_E_STATE, "the last tick was not a corridor tick");
  DeviceGuard g(c->b->device);
  ctl_cancel(c);                         // an armed launch would hold the stream (re-armed next tick)
  HIP_TRY(hipStreamSynchronize(c->b->stream));
  HIP_TRY(hipMemcpy(costs, c->d_cor_cost.get(), (size_t)c->cor_nslots * c->cfg.C * sizeof(double), hipMemcpyDeviceToHost));
  *nslots = c->cor_nslots;
  return LLAMPC_OK;
}

// llampc_ctl_variant's fields for a corridor tick on a centre line of track_n points, then the
// corridor block count: from the same ctl_shape.
int llampc_ctl_variant_corridor(int64_t n, int32_t C, int32_t H, int32_t K, int32_t rl_n, int32_t track_n,
                                int32_t out[10]) {
  if (!out) return fail(LLAMPC_E_ARG, "NULL argument");
  constexpr int32_t kCtlVariantCMax = 1 << 16;
  if (n < 1 || C < 1 || C > kCtlVariantCMax || H < 1 || H > LLAMPC_HMAX || K < 1 || K > LLAMPC_KMAX || rl_n < 2 ||
      track_n < 2 || track_n > kTrackMaxPoints)
    return fail(LLAMPC_E_ARG, "n=%lld C=%d (1..%d) H=%d (1..%d) K=%d (1..%d) rl_n=%d track_n=%d (2..%d)", (long long)n, C,
                kCtlVariantCMax, H, LLAMPC_HMAX, K, LLAMPC_KMAX, rl_n, track_n, kTrackMaxPoints);
  const CtlShape V = ctl_shape(n, C, H, K, rl_n, false, true, false, 0, track_n);
  if (V.lds > kCtlLdsMax) return fail(LLAMPC_E_ARG, "a corridor tick needs %zu B of LDS (> 160 KiB)", V.lds);
  const int32_t v[10] = {V.lpm, V.G, V.cpl, V.mpb, V.s4, V.zfit, V.R, V.nb_lb, V.nb_la, V.nb_cor};
  std::memcpy(out, v, sizeof v);
  return LLAMPC_OK;
}

int llampc_ctl_inputs(llampc_ctl* c, double* xref, double* U) {
  if (!c || !xref || !U) return fail(LLAMPC_E_ARG, "NULL argument");
  if (!c->d_dbg) return fail(LLAMPC_E_STATE, "controller created without debug_inputs");
  std::lock_guard<std::mutex> lc(c->mu);
  DeviceGuard g(c->b->device);
  ctl_cancel(c);                         // an armed launch would hold the stream (re-armed next tick)
  HIP_TRY(hipStreamSynchronize(c->b->stream));
  const size_t nx = 2 * (size_t)(c->cfg.H + 1), nu = 2 * (size_t)c->cfg.C * c->cfg.H;
  HIP_TRY(hipMemcpy(xref, c->d_dbg.get(), nx * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(U, c->d_dbg.get() + nx, nu * sizeof(double), hipMemcpyDeviceToHost));
  return LLAMPC_OK;
}

}  // extern "C"

// capi_ctl.hip — the controller tick's host side (llampc_ctl_*, include/llampc.h; ctl.hip): the
// control loop body rt.py:278-366 as ONE launch per step, the controller state resident on the
// device between steps.  Here: the lifecycle, the tick and its wait, the armed launches, the
// reference, the debug inputs, the device time and the variant question.  A tick's arguments and the
// state after it are capi_host.hpp's (ctl_tick_prepare / ctl_tick_commit); the sharding transports
// are capi_ctl_shard.hip's, the track and the corridor capi_ctl_corr.hip's.
#include "capi_ctl.hpp"

using namespace llampc;

static_assert(sizeof(llampc_ctl_cfg) == 280, "llampc_ctl_cfg layout (llampc/_native.py CtlCfg)");
static_assert(sizeof(llampc_ctl_out) == sizeof(llampc_plan_out) + 56 + 16 * LLAMPC_HMAX, "llampc_ctl_out layout");

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

// ctl_tick_prepare of the controller as it stands (after ctl_refresh; the caller's locks as ctl_view's).
static int ctl_prepare(const llampc_ctl* c, const double* x_t, CtlPrep& P) {
  char why[256];
  const int rc = ctl_tick_prepare(ctl_view(*c), ctl_tick_state(*c, *c->b, c->mb), x_t, P, why, sizeof why);
  return rc ? fail(rc, "%s", why) : LLAMPC_OK;
}

// A prepared tick's one launch: the corridor kernel for a corridor tick.
static hipError_t ctl_launch(const CtlPrep& P, hipStream_t s) {
  return P.corr ? launch_ctl_corr(P.L, P.cor, P.lpm, P.lds, s) : launch_ctl(P.L, P.lpm, P.lds, s);
}

// A launched tick's launch.  Over a gather transport (CtlLaunch.px_phase 1) it is two (ctl_gather_split):
// the look-back launch, then with RCCL the gather and the rest; without, the second launch is kept for
// llampc_ctl_resume, once the caller has carried the records.
static int ctl_enqueue(llampc_ctl* c, const CtlPrep& P) {
  llampc_bank* b = c->b;
  TimedLaunch tl(b, 0, b->stream);
  if (P.L.px_phase != 1) {
    HIP_TRY(ctl_launch(P, b->stream));
    return LLAMPC_OK;
  }
  CtlPrep P1, P2;
  ctl_gather_split(P, P1, P2);
  HIP_TRY(launch_ctl(P1.L, P1.lpm, P1.lds, b->stream));
  if (!c->xg_comm) {
    c->xg_second = P2;
    return LLAMPC_OK;
  }
  if (int rc = comm_all_gather(c->xg_comm, c->d_xsend.get(), c->d_xgath.get(), (size_t)c->xg_nw, true, b->stream)) return rc;
  HIP_TRY(launch_ctl(P2.L, P2.lpm, P2.lds, b->stream));
  return LLAMPC_OK;
}

// The host state after P's tick was enqueued (or its armed launch fired).
static void ctl_commit(llampc_ctl* c, const CtlPrep& P) {
  ctl_tick_commit(*c, *c->b, c->mb, P.next);
  c->pending = true;
  c->pend_seq = P.next.hseq;
  c->b->launches++;
}

// A launched tick as the fused step enqueues it (capi_ctl.hpp): llampc_ctl_tick_async's refresh and
// prepare, then `before` (its warm flag; what the caller enqueues ahead of the tick), the tick's one
// launch and its commit.  A refusal of the prepare, or `before` failing, leaves nothing of the tick.
int ctl_tick_launched(llampc_ctl* c, const double* x_t, int (*before)(void* arg, int32_t warm), void* arg) {
  CtlPrep P;
  int rc;
  if ((rc = ctl_refresh(c, true)) || (rc = ctl_prepare(c, x_t, P)) || (rc = before(arg, P.L.warm))) return rc;
  HIP_TRY(ctl_launch(P, c->b->stream));
  ctl_commit(c, P);
  return LLAMPC_OK;
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
  CtlPrep P;
  int rc = ctl_refresh(c, false);
  if (rc) return rc;
  rc = ctl_prepare(c, nullptr, P);
  c->door_ctr = P.next.door_ctr;         // spent here: whether or not the launch call succeeds
  if (rc) return rc;
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

// The armed launch is this tick's, and still fresh (ctl_arm_fires): rings its doorbell with x_t and
// commits it.  False: it is stale, and the caller cancels it.
static bool ctl_ring(llampc_ctl* c, const double* x_t) {
  const double age = std::chrono::duration<double>(std::chrono::steady_clock::now() - c->arm_t).count();
  const CtlLaunch& A = c->arm.L;
  if (!ctl_arm_fires(age, c->arm.next.t - 1, c->t, A.px_G, c->mb != nullptr, A.px_seq, c->mb ? c->mb->seq : 0)) return false;
  uint64_t w[kCtlDoorWords];
  ctl_door_words(x_t, A.door_seq, w);
  uint64_t* door = c->door.get();
  for (int j = 0; j < kCtlDoorWords - 1; ++j) __atomic_store_n(&door[j], w[j], __ATOMIC_RELAXED);
  __atomic_store_n(&door[kCtlDoorWords - 1], w[kCtlDoorWords - 1], __ATOMIC_RELEASE);
  c->armed = false;
  c->b->armed = nullptr;
  ctl_commit(c, c->arm);
  return true;
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
  if (out) *out = nullptr;
  char why[256];
  if (int rc = ctl_create_refused(!out, !b || !cfg || !points || !prefix, cfg, np, b ? b->n : 0, b && b->d_rl,
                                  b ? b->rl_n : 0, why, sizeof why))
    return fail(rc, "%s", why);
  const llampc_ctl_cfg& k = *cfg;
  const int nb_lb = lookback_blocks_r(b->n, lookback_r(b->n, k.K));
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
    if (ctl_ring(c, x_t)) {
      ctl_arm_later(c);
      return LLAMPC_OK;
    }
    ctl_cancel(c);                       // stale: this tick launches normally
  }
  CtlPrep P;
  int rc;
  if ((rc = ctl_refresh(c, true)) || (rc = ctl_prepare(c, x_t, P))) return rc;
  if ((rc = ctl_enqueue(c, P))) return rc;
  ctl_commit(c, P);
  if (P.L.px_phase == 1 && !c->xg_comm) {   // the caller carries the records (llampc_ctl_resume)
    c->xg_wait = true;
    c->xg_read = false;
    return LLAMPC_OK;
  }
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
  if (const char* why = ctl_solver_blocks(c->solver_attached, CtlSetter::prelaunch, on != 0)) return fail(LLAMPC_E_STATE, "%s", why);
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

int llampc_ctl_set_applied(llampc_ctl* c, const double* u0, const double* useq) {
  if (!c || !u0) return fail(LLAMPC_E_ARG, "controller/u0 is NULL");
  const int32_t H = c->cfg.H;
  if (!ctl_applied_finite(u0, useq, H)) return fail(LLAMPC_E_ARG, "the applied input and sequence must be finite");
  std::lock_guard<std::mutex> lc(c->mu);
  if (c->pending) return fail(LLAMPC_E_STATE, "a controller tick is outstanding");
  if (c->t < 1) return fail(LLAMPC_E_STATE, "no tick completed yet: there is no applied input to replace");
  BankIdle idle(c->b);
  if (idle.rc) return idle.rc;
  hipStream_t s = c->b->stream;
  // u_prev [2] and useq [HMAX][2] follow each other in CtlState: u0 | useq (or u0 again, row 0 alone)
  static_assert(offsetof(CtlState, useq) == offsetof(CtlState, u_prev) + 2 * sizeof(double), "CtlState: u_prev, then useq");
  double h[2 + 2 * LLAMPC_HMAX];
  const size_t nd = useq ? 2 + 2 * (size_t)H : 4;
  for (size_t i = 0; i < nd; ++i) h[i] = i < 2 ? u0[i] : useq ? useq[i - 2] : u0[i - 2];
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(reinterpret_cast<char*>(c->d_st.get()) + offsetof(CtlState, u_prev), h, nd * sizeof(double),
                    hipMemcpyHostToDevice));
  return LLAMPC_OK;
}

// The shape ctl_tick_prepare gives a tick past the warm-up (unsharded), from the same ctl_shape.
int llampc_ctl_variant(int64_t n, int32_t C, int32_t H, int32_t K, int32_t rl_n, int32_t out[9]) {
  bool no_stage = false;
  if (const char* e = std::getenv("LLAMPC_CTL_NO_STAGE")) no_stage = e[0] == '1';
  CtlShape V{};
  char why[256];
  if (int rc = ctl_variant_refused(!out, n, C, H, K, rl_n, nullptr, no_stage, V, why, sizeof why)) return fail(rc, "%s", why);
  const int32_t v[9] = {V.lpm, V.G, V.cpl, V.mpb, V.s4, V.zfit, V.R, V.nb_lb, V.nb_la};
  std::memcpy(out, v, sizeof v);
  return LLAMPC_OK;
}

}  // extern "C"

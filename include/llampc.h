/*
 * llampc.h — C ABI of the MI355X-native LLA-MPC model-bank engine (libllampc_hip.so).
 *
 * Drop-in boundary for the reference's hot path (tianhao-stan-wu/LLA-MPC; all
 * citations relative to the reference root).  Plain pointers and sizes only; every
 * array is row-major fp64 unless stated.  All calls return 0 on success or a negative
 * LLAMPC_E_* code; llampc_last_error() gives the thread's last message.
 *
 *  ABI entry point                 replaces (reference)
 *  ------------------------------  -----------------------------------------------------
 *  llampc_bank_create/destroy      the N-object MODEL_BANK + params_pass tuple
 *                                  (llampc/mpc/run_nmpc_orca_llampc_rt.py:161-179) and the
 *                                  error_windows ring (rt.py:83-84)
 *  llampc_lookback                 evaluate_models_vectorized (llampc/mpc/evaluate_models_
 *                                  vectorized.py:4-24) + the inline error / window / argmin
 *                                  / argsort[:K] block (rt.py:347-366)
 *  llampc_lookahead                H x Model._integrate_batch (llampc/models/model.py:32-40)
 *                                  per (model, candidate) + the NLP objective
 *                                  (llampc/mpc/nmpc.py:44-111) + argmin
 *  llampc_plan / llampc_plan_device one LLA-MPC tick: rt.py:300-366 (look-back on the
 *                                  newest transition, selection, look-ahead from x_t)
 *  llampc_plan_corridor,           (new) llampc_plan / llampc_lookahead with soft per-step track
 *  llampc_lookahead_corridor       half-planes on every rollout's positions (the half-planes of
 *                                  llampc_nlp_solve_corridor; rt.py:63 runs TRACK_CONS = False)
 *  llampc_merge / _device          (new) cross-shard merge of per-GPU plan results
 *  llampc_exchange_rccl / _peer    (new) the per-tick gather + merge of the sharded bank
 *                                  (SURVEY.md §8e): RCCL all-gather, or xGMI mailboxes
 *  llampc_nlp_*                    setupNLP / .solve (nmpc.py:14-203), solved by sampling
 *  llampc_nlp_batch_*              (new) the per-model setupNLP bank and the solve with the
 *                                  selected one (rt.py:195-202, 305): B problems of a model
 *                                  bank, by model index, in one launch
 *  llampc_dynamics_batch           Dynamic.calc_forces_batch (llampc/models/dynamic.py:
 *                                  117-154), Dynamic._diffequation_batch (:98-115)
 *  llampc_ctl_*                    the control loop body rt.py:278-366 on the device
 *                                  (ConstantSpeed, selection, look-ahead, mu-hat, state)
 *  llampc_ctl_step / _solver_*     (new) that body with the selected model's NMPC solve
 *                                  (rt.py:303-305) chained behind the tick on the device and its
 *                                  first input committed as the applied one
 *  llampc_ctl_set_applied          (new) tells the controller the input that was really applied
 *  llampc_integrate_batch          Model._integrate_batch (model.py:32-40, RK4),
 *                                  Model._integrate/odeintRK6 (model.py:18-30,
 *                                  llampc/utils/rk6.py:13-28) and the NLP Euler form
 *                                  (nmpc.py:58-60 with Dynamic.casadi, dynamic.py:195-226)
 */
#ifndef LLAMPC_H_
#define LLAMPC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLAMPC_ABI_VERSION 1
#define LLAMPC_KMAX 32          /* max top-K (rt.py:69 uses K=10) */
#define LLAMPC_WMAX 128         /* max look-back window (rt.py:67 uses W=10) */
#define LLAMPC_HMAX 64          /* max horizon of the controller tick (rt.py:52 uses 20) */

enum llampc_status {
  LLAMPC_OK = 0,
  LLAMPC_E_ARG = -1,        /* bad argument / shape                       */
  LLAMPC_E_HIP = -2,        /* HIP runtime error                          */
  LLAMPC_E_NODEV = -3,      /* no HIP device                              */
  LLAMPC_E_STATE = -4,      /* call not valid in the handle's state       */
  LLAMPC_E_OOM = -5,        /* device allocation failed                   */
  LLAMPC_E_DEVICE = -6      /* the tick's record reports a device-side status != 0 */
};

/* Integrators.  RK4 = odeintRK4_batch (rk6.py:50-68) on the |vx| dynamics
 * (dynamic.py:98-154); EULER_NLP = the NLP transcription x+Ts*f (nmpc.py:58-60) on
 * Dynamic.casadi (vmin clamp, atan2(.,vx); dynamic.py:195-226); RK6 = odeintRK6
 * (rk6.py:13-28), the plant integrator (dynamic.py:59-74). */
enum llampc_integrator { LLAMPC_RK4 = 0, LLAMPC_EULER_NLP = 1, LLAMPC_RK6 = 2 };

/* argmin NaN policy for the look-back selection: NAN_FIRST reproduces np.argmin
 * (first NaN wins, rt.py:359); NAN_IGNORE treats NaN as +inf.  top-K always orders
 * NaN last (np.argsort, rt.py:360).  The look-ahead argmin always treats NaN as +inf. */
enum llampc_nan_policy { LLAMPC_NAN_FIRST = 0, LLAMPC_NAN_IGNORE = 1 };

/* llampc_dynamics_batch ops */
enum llampc_dyn_op { LLAMPC_OP_FORCES = 0, LLAMPC_OP_DERIV = 1 };

/* Shared (per-bank) vehicle constants (llampc/params/orca.py:13-27). */
typedef struct llampc_vehicle {
  double lf, lr, mass, Iz;
  double Cm1, Cm2, Cr0, Cr2;
  int32_t input_acc;   /* 1: Frx = mass*u0 (dynamic.py:139-142)                    */
  int32_t approx;      /* 1: linear tires Ffy=2*Cf*af (dynamic.py:126-136); params */
                       /*    rows Cf/Cr are then cornering stiffnesses             */
} llampc_vehicle;

/* Look-ahead objective (nmpc.py:44-111) and candidate feasibility (nmpc.py:102-105). */
typedef struct llampc_cost {
  double Q[4];         /* 2x2 row-major tracking weight   (rt.py:60 diag(1,1))      */
  double R[4];         /* 2x2 row-major input-rate weight (rt.py:62 diag(5e-3,1))   */
  double P[4];         /* 2x2 row-major terminal weight   (rt.py:61 diag(0,0))      */
  double umin[2], umax[2];   /* input bounds (orca.py:31-35)                        */
  double rate_max[2];  /* |u_k - u_{k-1}| <= rate_max*Ts; <0 disables (orca.py:35)  */
  int32_t enforce_bounds;    /* 1: infeasible candidates cost +inf                  */
  int32_t reserved;
} llampc_cost;

/* Look-ahead reference.  GIVEN: one shared xref [2][H+1] (ConstantSpeed with mu-hat,
 * rt.py:280).  RACELINE: every model tracks its own ConstantSpeed
 * reference (planner.py:12-67) with mu_n = (Df_n + Dr_n) / (9.81 mass), evaluated on the
 * device from the table of llampc_bank_set_raceline; xref then points to the shared start
 * {s0 = arc length after the projection (planner.py:25-33), v0, scale, 0}. */
enum llampc_xref_mode { LLAMPC_XREF_GIVEN = 0, LLAMPC_XREF_RACELINE = 1 };

/* One tick's inputs.  Pointers are HOST pointers for llampc_plan and DEVICE pointers
 * for llampc_plan_device. */
typedef struct llampc_plan_in {
  const double* x_prev;   /* [6]  x_{t-1}                                          */
  const double* u_prev;   /* [2]  u_{t-1}                                          */
  const double* x_now;    /* [6]  x_t (look-back target, look-ahead start)          */
  const double* U;        /* [C][H][2] candidate control sequences                 */
  const double* xref;     /* [2][H+1] reference (planner.py:12-67 output); with
                             xref_mode RACELINE: [4] {s0, v0, scale, 0} (see below)  */
  const double* uprev;    /* [2]  last applied input for du_0 (nmpc.py:65-66)      */
  int32_t C, H;
  int32_t K;              /* top-K size, <= LLAMPC_KMAX                            */
  int32_t integrator;     /* look-ahead integrator                                 */
  int32_t do_lookback;    /* 0: skip the look-back (first tick, rt.py:347)         */
  int32_t do_lookahead;   /* 0: skip the look-ahead                                */
  int32_t nan_policy;
  int32_t xref_mode;      /* LLAMPC_XREF_GIVEN (0) or LLAMPC_XREF_RACELINE (1)      */
  int64_t current_model;  /* global index used while the window fills (rt.py:264)  */
  double Ts;
  llampc_cost cost;
} llampc_plan_in;

/* One tick's result (fixed size: also the cross-GPU payload, see llampc_merge). */
#define LLAMPC_STATUS_POLL_TIMEOUT 1
typedef struct llampc_plan_out {
  int32_t window_count;   /* transitions in the window, <= W (rt.py:354)           */
  int32_t window_full;    /* window_count >= W: selection valid (rt.py:357)        */
  int32_t K;
  int32_t sel_owned;      /* this shard owns sel_model                             */
  int64_t lb_best;        /* argmin of the window mean (rt.py:359), -1 if not full */
  double  lb_best_val;
  int64_t sel_model;      /* full ? lb_best : current_model                        */
  int32_t sel_cand;       /* argmin_c cost[sel_model, c]  ("chosen control")       */
  int32_t n_nonfinite;    /* look-ahead rollouts whose cost is not finite          */
  double  sel_cost;
  int64_t la_best_model;  /* argmin over all (model, candidate) costs, NaN as +inf;
                             -1 (with la_best_cand -1, la_best_cost NaN) without a
                             look-ahead and when every cost of the tick is NaN     */
  int32_t la_best_cand;
  int32_t status;         /* 0 ok; LLAMPC_STATUS_POLL_TIMEOUT (1): the in-launch
                             completion (or the peer exchange) gave up waiting (a device
                             fault or a missing rank, never expected) */
  double  la_best_cost;
  int64_t topk[LLAMPC_KMAX];      /* argsort(window mean)[:K] (rt.py:360), -1 pad  */
  double  topk_val[LLAMPC_KMAX];
  double  topk_Df[LLAMPC_KMAX];   /* bank Df/Dr of the top-K (rt.py:336-338)      */
  double  topk_Dr[LLAMPC_KMAX];
  int32_t topk_cand[LLAMPC_KMAX]; /* look-ahead best candidate of each top-K model */
  double  topk_cost[LLAMPC_KMAX];
} llampc_plan_out;

typedef struct llampc_bank llampc_bank;

/* ---- library ---------------------------------------------------------------- */
int32_t     llampc_abi_version(void);
const char* llampc_last_error(void);
int         llampc_device_count(int32_t* count);

/* ---- bank handle -------------------------------------------------------------- */
/* params: [6][n] rows (Bf, Cf, Df, Br, Cr, Dr) = rt.py:179 params_pass order.
 * global_offset: global index of this shard's first model (multi-GPU).  W: window. */
int llampc_bank_create(const double* params, int64_t n, int64_t global_offset,
                       const llampc_vehicle* veh, int32_t W, int32_t device,
                       llampc_bank** out);
int llampc_bank_destroy(llampc_bank* bank);
int llampc_bank_info(const llampc_bank* bank, int64_t* n, int64_t* global_offset,
                     int32_t* W, int32_t* window_count, int32_t* device);
int llampc_bank_reset(llampc_bank* bank);                 /* empty the window       */
/* plan-kernel launches enqueued on this bank so far (every tick entry point is ONE
 * launch; the controller test counts them — replaces nothing in the reference).  On an NLP
 * solver's bank: its solve launches, and every track-corridor kernel (llampc_nlp_solve_track,
 * llampc_nlp_track_corridor, llampc_nlp_batch_solve_track, llampc_nlp_batch_track_corridor) as one
 * more */
int llampc_bank_launches(const llampc_bank* bank, int64_t* launches);
/* ring: [n][W] oldest -> newest (the rt.py error_windows layout, zeros if unfilled) */
int llampc_bank_window(llampc_bank* bank, double* ring, int32_t* window_count);
/* stream the bank launches on (hipStream_t as void*); NULL = its own stream */
int llampc_bank_set_stream(llampc_bank* bank, void* stream);
/* the stream the bank launches on now (its own or the one set above), for callers that
 * enqueue their own work with it.  The bank's OWN stream may be replaced by a dedicated-queue
 * one (llampc_bank_set_concurrency(banks > 1), llampc_ctl_set_prelaunch(on)): a handle read
 * earlier is then destroyed — read it again after either call. */
int llampc_bank_stream(const llampc_bank* bank, void** stream);
/* the number of banks the caller ticks concurrently on this device (default 1; BASELINE
 * config 5 ticks two tracks together: 2).  The look-ahead sizes its launch for 1/banks of the
 * chip (its lane split), so the concurrent launches are resident together, and banks > 1 gives
 * the bank's own stream a hardware queue of its own (a full-CU-mask stream: two banks' launches
 * on one of HIP's shared queues would run one after the other).  Other banks
 * keep a plain non-blocking stream (LLAMPC_DEDICATED_QUEUE=1 at create: a dedicated queue
 * anyway).  Replaces nothing in the reference (one process per track there) */
int llampc_bank_set_concurrency(llampc_bank* bank, int32_t banks);

/* Per-kernel HIP-event timing of the bank's launches, on the stream they run on (for the
 * benchmark's roofline).  enable=k >= 1 arms `max_launches` event pairs; each pair brackets
 * a group of k consecutive launches of the plan kernel (the whole tick: look-back +
 * look-ahead + selection), so the mean launch duration is elapsed / k (k > 1 spreads the
 * events' own cost over the group); enable=-k (k >= 1) brackets ONE launch out of every k
 * (sampling: for ticks whose launches are separated by other work on the stream, e.g. the
 * multi-GPU exchange, with the events' cost on 1/k of the ticks); enable=0 disarms.
 * count = launches timed. */
int llampc_bank_timing(llampc_bank* bank, int32_t enable, int32_t max_launches);
/* Synchronises, returns avg_ms[3] and count[3] for {plan kernel, the NLP solver's track-corridor
 * kernel (llampc_nlp_track_corridor, llampc_nlp_solve_track and their llampc_nlp_batch_* forms),
 * reserved} since the last read, and re-arms the counters. */
int llampc_bank_timing_read(llampc_bank* bank, double* avg_ms, int64_t* count);

/* ---- look-back (host pointers) -------------------------------------------------- */
/* err_out [n] (rt.py:349 errors), wmean_out [n] (rt.py:358 avg_errors, valid when the
 * window is full), topk/topk_val [K] may each be NULL. */
int llampc_lookback(llampc_bank* bank, const double* x_prev, const double* u_prev,
                    const double* x_now, double Ts, int32_t K, int32_t nan_policy,
                    double* err_out, double* wmean_out, int64_t* best, int64_t* topk,
                    double* topk_val, int32_t* window_count);

/* ---- look-ahead (host pointers) ------------------------------------------------- */
/* cost_out [n][C] and best_cand_out [n] may be NULL.  A candidate that is infeasible under
 * cost.enforce_bounds costs +inf; the argmins treat NaN as +inf and break ties towards the
 * lower index, so when every candidate of a model is infeasible its best candidate is 0 with
 * cost +inf, and when every (model, candidate) pair is, best_model = best_cand = 0 and
 * best_cost = +inf (np.argmin over all-inf).  When every cost is NaN there is no best:
 * best_model = best_cand = -1, best_cost = NaN (the record's la_best_*). */
int llampc_lookahead(llampc_bank* bank, const double* x0, const double* U, int32_t C,
                     int32_t H, const double* xref, const double* uprev,
                     const llampc_cost* cost, double Ts, int32_t integrator,
                     double* cost_out, int32_t* best_cand_out, int64_t* best_model,
                     int32_t* best_cand, double* best_cost);

/* The look-ahead kernel variant a launch of n models, C candidates, H steps takes with the
 * shared (GIVEN) xref — host only, no device needed (for tests that mean to run one variant),
 * from the launch's own rule (plan_shape):
 * out = {lpm (lanes per rollout: 4, 2 or 1; honours the LLAMPC_LPM override exactly as the
 * launch does), G (lanes per model), cpl (candidates per lane), stage (1: the candidate
 * inputs are staged in LDS)}.  share = llampc_bank_set_concurrency's banks (1 by default). */
int llampc_plan_variant(int64_t n, int32_t C, int32_t H, int32_t integrator, int32_t share,
                        int32_t out[4]);

/* llampc_lookahead under a soft track corridor (extends llampc_lookahead; the half-planes are
 * llampc_nlp_solve_corridor's): hp [H][6], row k - 1 = (a0, a1, b, c0, c1, d), the half-planes
 * a.p_k <= b and c.p_k <= d on the position p_k = (X, Y) after k steps of the launch's own
 * integrator, k = 1..H (a = (0, 0), b = +inf disables one).  Every (model, candidate) cost becomes
 *   J_c = J + weight x sum_k max(a.p_k - b, 0)^2 + max(c.p_k - d, 0)^2
 * (k ascending, every product and sum rounded on its own, weight x pen added last, after the
 * terminal and input-rate terms); a candidate infeasible under cost.enforce_bounds still costs
 * +inf, and the per-model argmin, the global best, the non-finite count and the tie-breaking are
 * llampc_lookahead's, applied to J_c.  Replaces nothing in the reference (its look-ahead is the
 * NLP solve, whose track constraints constraints.py holds; rt.py:63 runs without them).
 * Integrators: LLAMPC_RK4 and LLAMPC_EULER_NLP.  The launch rolls every pair out with both position
 * components in one lane (at 4 lanes per rollout too, where llampc_lookahead splits them for
 * diagonal Q and P), one block per group of models — never the work-queue layout.
 * LLAMPC_E_ARG, with nothing enqueued and the bank's launch counter unchanged: hp NULL, LLAMPC_RK6,
 * a non-finite normal component, an offset NaN or -inf, a weight negative or non-finite. */
int llampc_lookahead_corridor(llampc_bank* bank, const double* x0, const double* U, int32_t C,
                              int32_t H, const double* xref, const double* uprev,
                              const llampc_cost* cost, double Ts, int32_t integrator,
                              double* cost_out, int32_t* best_cand_out, int64_t* best_model,
                              int32_t* best_cand, double* best_cost,
                              const double* hp /* [H][6] */, double weight);
/* llampc_plan_variant for a corridor launch (llampc_lookahead_corridor, llampc_plan_corridor) —
 * host only, from the same rule with a corridor offered: out = {lpm, G, cpl, stage}; stage counts the
 * corridor's 48 H bytes of LDS, so a shape llampc_plan_variant reports staged may be unstaged
 * here.  LLAMPC_E_ARG also for LLAMPC_RK6. */
int llampc_plan_variant_corridor(int64_t n, int32_t C, int32_t H, int32_t integrator, int32_t share,
                                 int32_t out[4]);

/* Attach (replace) the raceline library used by LLAMPC_XREF_RACELINE: natural cubic
 * splines over the arc length (pycubicspline.py:17-182, track.py:52-83): knots [n]
 * (Spline2D.s, ascending from 0), xy [2][4][n-1] (x(s) then y(s); rows a, b, c, d per
 * segment), speed [M][4][n-1] (one speed profile per friction), mus [M] ascending.
 * 2 <= n <= 850 (knots and x/y rows are staged in 60 KB of LDS), 1 <= M <= 64.  Copied
 * to the device. */
int llampc_bank_set_raceline(llampc_bank* bank, const double* knots, int32_t n, const double* xy,
                             const double* speed, const double* mus, int32_t M);

/* ---- fused tick ------------------------------------------------------------------ */
/* Host pointers; blocking.  err_out [n], wmean_out [n], cost_out [n][C] may be NULL.
 * With all three NULL the kernel writes the record into the bank's pinned host buffer and
 * then a completion tag; the call spins on the tag (no D2H copy, no stream synchronise).
 * LLAMPC_SYNC_COMPLETION=1 in the environment selects the copy + synchronise path. */
int llampc_plan(llampc_bank* bank, const llampc_plan_in* in, llampc_plan_out* out,
                double* err_out, double* wmean_out, double* cost_out);
/* llampc_plan with the look-ahead under a corridor (extends llampc_plan; hp, weight and the cost
 * J_c as llampc_lookahead_corridor): the same blocking tick in ONE launch — the look-back half,
 * the NaN policies, the selection and the record are llampc_plan's, with J_c in the cost's place.
 * Both completion modes: outputs copied back, or (err_out, wmean_out and cost_out all NULL) the
 * record through pinned host memory and its tag.  hp rides behind the other inputs in the bank's
 * staging buffer (one host-to-device copy; a corridor tick's inputs never travel as kernel
 * arguments).  LLAMPC_E_ARG, with nothing enqueued and the launch counter unchanged: hp NULL,
 * do_lookahead 0, LLAMPC_RK6, LLAMPC_XREF_RACELINE, a corridor or weight as above.
 * The corridor built on the device, tick after tick, with an async form: llampc_plan_track below.
 * Not yet under a corridor (the remaining steps): llampc_plan_device,
 * llampc_plan_exchange and the sharded bank, the sharded controller, the work-queue and inline-pack
 * layouts, RK6, the per-model raceline reference. */
int llampc_plan_corridor(llampc_bank* bank, const llampc_plan_in* in, const double* hp /* [H][6] */,
                         double weight, llampc_plan_out* out, double* err_out, double* wmean_out,
                         double* cost_out);

/* ---- track tick: llampc_plan_corridor with the corridor built inside the launch ---------------- */
/* Attach (replace) the track whose corridor llampc_plan_track builds: llampc_nlp_set_track's
 * arguments and refusals (centre [2][n] finite, theta [n] from 0 strictly increasing, track_length
 * beyond theta[n-1], track_width > 0, 2 <= n <= 4096; LLAMPC_E_STATE while an async tick is
 * outstanding).  Copied to the device; invalidates the bank's path.  Replaces nothing in the
 * reference (constraints.py builds the half-planes on the host). */
int llampc_bank_set_track(llampc_bank* bank, const double* centre /* [2][n] */, const double* theta /* [n] */,
                          int32_t n, double track_length, double track_width);
/* Seeds the next track tick's path P [2][H+1] (row k of its corridor is built at P_k, k = 1..H);
 * NULL invalidates the path (the next track tick then runs on the disabled rows).  LLAMPC_E_ARG: a
 * non-finite entry, H outside [1, LLAMPC_HMAX]. */
int llampc_bank_set_path(llampc_bank* bank, const double* path /* [2][H+1] or NULL */, int32_t H);
/* llampc_plan_corridor whose half-planes the launch builds itself (still ONE launch): H corridor blocks
 * compute hp [H][6] from the bank's track (llampc_bank_set_track; half-width track_width / 2 - margin)
 * along the bank's path, the look-ahead blocks roll out under it with llampc_plan_corridor's cost J_c,
 * and once the record is complete the launch re-runs the chosen (sel_model, sel_cand) rollout and keeps
 * its positions on the device as the next tick's path: P_j = X_{j+1} for j < H, P_H = X_H
 * (constraints.default_path's prev_xmpc rule).  The host builds no geometry and moves no path between
 * ticks.  The path is offered to a tick only when its H is the tick's and it was written by the bank's
 * immediately preceding launch, itself a track tick, or seeded by llampc_bank_set_path since; it was
 * written valid only if the chosen cost and positions were finite, sel_owned = 1 and
 * 0 <= sel_cand < C.  Any other launch on the bank, llampc_bank_reset and llampc_bank_set_track clear
 * it.  Without a valid path every row is (0, 0, +inf, 0, 0, +inf): no corridor.
 * LLAMPC_RK4 on the given xref, H <= LLAMPC_HMAX.  Both completion modes, as llampc_plan_corridor.
 * With nothing enqueued and the launch counter unchanged: LLAMPC_E_STATE without a track or while an
 * async tick is outstanding; LLAMPC_E_ARG for do_lookahead 0, LLAMPC_RK6, LLAMPC_EULER_NLP,
 * LLAMPC_XREF_RACELINE, a weight negative or non-finite, a margin non-finite or >= track_width / 2. */
int llampc_plan_track(llampc_bank* bank, const llampc_plan_in* in, double weight, double margin,
                      llampc_plan_out* out, double* err_out, double* wmean_out, double* cost_out);
/* llampc_plan_async for the track tick: completed by llampc_plan_wait. */
int llampc_plan_track_async(llampc_bank* bank, const llampc_plan_in* in, double weight, double margin);
/* The last track tick's read-back (blocking; for tests and logging): the path it used [2][H+1] (NaN
 * without a valid one), the rows it built hp [H][6] and their arc lengths theta [H], whether the path
 * was valid, and what it left for the next tick: next_path [2][H+1], next_valid, and next_cost, the
 * re-run's cost (the record's sel_cost).  LLAMPC_E_STATE unless the bank's last launch was a track tick. */
int llampc_bank_track_corridor(llampc_bank* bank, double* path, double* hp, double* theta, int32_t* valid,
                               double* next_path, int32_t* next_valid, double* next_cost);
/* llampc_plan_variant for a track tick on a centre line of track_n points — host only:
 * out = {lpm, G, cpl, stage, nb_cor (the corridor blocks: H)}. */
int llampc_plan_variant_track(int64_t n, int32_t C, int32_t H, int32_t share, int32_t track_n, int32_t out[5]);
/* Host pointers; asynchronous (SURVEY.md §8b "_async" variant): the inputs are copied
 * into the bank's pinned staging buffer before the call returns (the caller may reuse
 * them), and the H2D copy and the plan kernel are enqueued on the bank's stream; the
 * kernel writes the record to pinned host memory + a completion tag, on which
 * llampc_plan_wait spins before returning the record.
 * At most one outstanding async tick per bank (LLAMPC_E_STATE otherwise); independent
 * banks (e.g. two tracks) overlap on the device. */
int llampc_plan_async(llampc_bank* bank, const llampc_plan_in* in);
int llampc_plan_wait(llampc_bank* bank, llampc_plan_out* out);
/* Device pointers in `in`; d_out is a device llampc_plan_out; asynchronous on
 * `stream` (hipStream_t, NULL = the bank's stream).  d_err/d_wmean/d_cost: device
 * arrays or NULL.  LLAMPC_E_STATE while an llampc_plan_async tick is outstanding (both
 * would share the bank's completion state and window). */
int llampc_plan_device(llampc_bank* bank, const llampc_plan_in* in, void* d_out,
                       double* d_err, double* d_wmean, double* d_cost, void* stream);

/* ---- multi-GPU merge ----------------------------------------------------------- */
/* Merge G shard results (shards ordered by global_offset; G <= 32 on the device) into one, deterministic:
 * lowest value, ties -> lowest global index, NaN first for lb_best under NAN_FIRST.
 * Host version runs the same merge code as the device version. */
int llampc_merge(const llampc_plan_out* parts, int32_t G, int32_t nan_policy,
                 llampc_plan_out* merged);
int llampc_merge_device(const void* d_parts, int32_t G, int32_t nan_policy, void* d_merged,
                        int32_t device, void* stream);
/* ---- RCCL, the library's own communicator (public rccl.h API) ---------------------- */
/* The library resolves RCCL at first use: the librccl.so.1 the process has already loaded
 * (torch's, so one RCCL per process), else the system's.  Setup per rank: rank 0 calls
 * llampc_comm_unique_id (ncclGetUniqueId) and shares the 128-byte id out of band (e.g. a
 * torch.distributed store or all_gather_object); every rank calls llampc_comm_create
 * (ncclCommInitRank on `device`; collective: blocks until all `world` ranks joined).
 * LLAMPC_E_STATE when no RCCL can be loaded. */
typedef struct llampc_comm llampc_comm;
int llampc_comm_unique_id(void* id /* 128 bytes out */);
int llampc_comm_create(const void* id /* 128 bytes */, int32_t world, int32_t rank, int32_t device, llampc_comm** out);
int llampc_comm_destroy(llampc_comm* comm);
/* The per-tick exchange of the sharded bank, enqueued on `stream` (hipStream_t) with no
 * host round trip: ncclAllGather of this rank's record d_local (one llampc_plan_out) into
 * d_all [world] over `comm`, then merge_kernel into d_merged.  Replaces the reference-side
 * gather that SURVEY.md §8e specifies (the reference itself is single-process). */
int llampc_exchange_rccl(llampc_comm* comm, const void* d_local, void* d_all, void* d_merged, int32_t nan_policy,
                         void* stream);

/* Peer exchange: the same per-tick gather + merge with no collective library.  Each rank
 * owns a mailbox (uncached device memory, [2][world] record slots of tagged words) that every
 * peer process maps through HIP IPC; per tick ONE kernel pushes this rank's record into slot
 * [rank] of every mailbox over xGMI (system-scope stores), polls its own mailbox until all
 * `world` records of this tick have arrived and runs merge_kernel's merge — the output equals
 * llampc_exchange_rccl's.  Setup: create, export the IPC handle (64 bytes), share the
 * handles out of band (e.g. a torch.distributed all_gather_object), open every peer's.  All
 * ranks must call llampc_exchange_peer the same number of times (the tick number is the tag).
 * A rank that waits more than the poll bound (default 10 s; set_bound) gets status
 * LLAMPC_STATUS_POLL_TIMEOUT in d_merged.  Replaces the same reference-side gather as
 * llampc_exchange_rccl. */
typedef struct llampc_mailbox llampc_mailbox;
int llampc_mailbox_create(int32_t world, int32_t rank, int32_t device, llampc_mailbox** out);
int llampc_mailbox_ipc_handle(llampc_mailbox* mb, void* handle /* 64 bytes out */);
int llampc_mailbox_open_peer(llampc_mailbox* mb, int32_t peer, const void* handle /* 64 bytes */);
/* Use `other`, a mailbox of rank `peer` created in THIS process on the same device, as that
 * peer's (several ranks driven from one process; tests). */
int llampc_mailbox_link(llampc_mailbox* mb, int32_t peer, const llampc_mailbox* other);
int llampc_mailbox_set_bound(llampc_mailbox* mb, double seconds);
int llampc_exchange_peer(llampc_mailbox* mb, const void* d_local, void* d_merged, int32_t nan_policy,
                         void* stream);
/* The sharded tick in ONE launch per rank: llampc_plan_device's tick on this rank's shard
 * (record -> d_local) whose completing block then runs the peer exchange itself (push, poll,
 * merge -> d_merged), so no second kernel follows the plan (RK4 look-ahead with the given
 * xref; otherwise, for world > 16 (the merge's LDS) or with LLAMPC_PEER_SPLIT=1: the plan
 * launch followed by llampc_exchange_peer).  Same rules as
 * llampc_plan_device (stream, LLAMPC_E_STATE while an async tick is outstanding) and as
 * llampc_exchange_peer (every rank makes the same sequence of exchange calls). */
int llampc_plan_exchange(llampc_bank* bank, const llampc_plan_in* in, void* d_local, void* d_merged,
                         llampc_mailbox* mb, void* stream);
int llampc_mailbox_destroy(llampc_mailbox* mb);

/* ---- controller tick (the whole control step on the device) ------------------------- */
/* One LLA-MPC control step of rt.py:269-366 in ONE kernel launch, the controller state kept
 * on the device between ticks (replaces the host loop body rt.py:278-366: ConstantSpeed with
 * mu-hat, planner.py:12-67 + track.py:147-160; the per-tick solve, nmpc.py:161-203 — here a
 * candidate search; the look-back selection rt.py:347-366; the mu-hat estimator rt.py:326-344):
 *   reference   ConstantSpeed(x_t, projidx, mu-hat, v_factor) once the window has been full
 *               for a tick (rt.py:278-282), ConstantSpeed(x_t, projidx) before; the start arc
 *               length from `prefix` (one entry per projection index, the reference's own sum);
 *               lap wrap projidx > lap_projidx -> 0 (rt.py:287-296)
 *   candidates  C sequences: candidate 0 = the previous chosen sequence shifted one step (or
 *               u_{t-1} held), candidate c >= 1 adds Philox4x32-10 noise (four-word sum, unit
 *               variance) x sigma_j, clipped to cost.umin/umax and, in order over the horizon,
 *               to |du| <= cost.rate_max Ts (oracle/llampc_oracle.py candidates_ctl)
 *   look-back   the transition (x_{t-1}, u_{t-1}) -> x_t from tick 2 on (rt.py:347)
 *   look-ahead  ticks t <= W: the nominal model (nlp_initial, rt.py:300-301); afterwards the
 *               selected model (nlp_bank[current_model_idx], rt.py:303) and the K top-K models,
 *               every candidate, RK4 + the NLP objective (llampc_plan's look-ahead)
 *   mu-hat      warm-up split (rt.py:326-330), then the top-K Dr / Df means (rt.py:331-344)
 * The bank must carry a raceline (llampc_bank_set_raceline) and is driven by the controller
 * from its creation on (its window advances with the ticks). */
typedef struct llampc_ctl_cfg {
  int32_t C, H, K, nan_policy;   /* candidates, horizon (<= LLAMPC_HMAX), top-K, look-back NaN */
  double Ts;
  double v_factor;               /* ConstantSpeed scale once mu-hat is used (rt.py:73: 0.9)  */
  double mu_init;                /* rt.py:327 (1.0)                                          */
  int32_t S;                     /* mu-hat smoothing window (rt.py:68: 20), <= 64            */
  int32_t lap_projidx;           /* rt.py:287 (ETHZ 656, ETHZMobil 440)                      */
  double sigma[2];               /* candidate noise std per input (pwm, steer)              */
  uint64_t seed;
  double nominal[6];             /* warm-up model (Bf, Cf, Df, Br, Cr, Dr), rt.py:207       */
  llampc_cost cost;              /* objective, bounds and rate bound of the look-ahead       */
  int32_t debug_inputs;          /* 1: keep each tick's xref and U (llampc_ctl_inputs)       */
  int32_t reserved;
} llampc_ctl_cfg;

typedef struct llampc_ctl_out {
  llampc_plan_out plan;          /* the tick record (sel_model / sel_cand: the chosen control;
                                    la_best_*: over the rolled-out models only; -1 while warm) */
  int64_t tick;
  int32_t projidx;               /* planner state after this tick (lap wrap applied)         */
  int32_t warm;                  /* 1: planned with the nominal model (tick <= W)            */
  double mu_used, scale_used;    /* curr_mu / scale of this tick's reference                 */
  double mu_pred;                /* mu-hat after this tick (NaN until the first update)      */
  double dr_mean, df_mean;       /* what this tick appended to the Dr / Df histories          */
  double u_seq[LLAMPC_HMAX][2];  /* [H][2]: the chosen control sequence; u_seq[0] is applied  */
} llampc_ctl_out;

typedef struct llampc_ctl llampc_ctl;
/* points [2][np]: the raceline polyline project_fast projects on (track.raceline);
 * prefix [np-1]: prefix[p] = sum of the segment lengths of points 0..p+1 (planner.py:29-36's
 * start arc length for projection index p). */
int llampc_ctl_create(llampc_bank* bank, const llampc_ctl_cfg* cfg, const double* points, int32_t np,
                      const double* prefix, llampc_ctl** out);
/* x_t [6] (host): one control step, blocking; the record comes back through pinned host memory. */
int llampc_ctl_tick(llampc_ctl* ctl, const double* x_t, llampc_ctl_out* out);
/* The same step enqueued (x_t copied into the launch); at most one outstanding per controller;
 * controllers of different banks (e.g. two tracks) overlap on the device. */
int llampc_ctl_tick_async(llampc_ctl* ctl, const double* x_t);
int llampc_ctl_wait(llampc_ctl* ctl, llampc_ctl_out* out);
/* on = 1: every tick also enqueues the NEXT tick's launch behind itself ("armed"): it runs the
 * part of the tick that does not need x_t (the raceline tables, the state, the variates) and
 * then waits on a doorbell in pinned host memory; the next llampc_ctl_tick_async stores x_t and
 * rings it instead of launching, so the launch call and the dispatch leave the control step's
 * latency (rt.py:269-366's step starts when x_t is known).  Results are those of unarmed ticks.
 * While armed, the bank's stream holds that launch: every other call on the bank or the
 * controller cancels it first (it exits untouched; the next tick launches normally and re-arms),
 * as does a tick more than 0.5 s after the arming; an armed launch never rung exits after 2 s.
 * The armed launch must not hold a hardware queue other work shares (a solve or another bank's
 * tick enqueued behind it on that queue would wait for the doorbell): on = 1 gives the bank's
 * own stream a hardware queue of its own (as llampc_bank_set_concurrency(> 1) does) and is
 * refused (LLAMPC_E_STATE) on a bank launching on a caller's stream (llampc_bank_set_stream).
 * With llampc_ctl_set_exchange (peer mailboxes) the armed launch runs the exchange after its
 * doorbell; its mailbox tick number is committed when it fires, so every rank may arm, cancel
 * or launch independently (call set_exchange first).  Not with llampc_ctl_set_gather (two
 * launches per tick; LLAMPC_E_STATE).  on = 0 cancels. */
int llampc_ctl_set_prelaunch(llampc_ctl* ctl, int32_t on);
/* The last completed tick's device time in microseconds: from x_t reaching the device (an armed
 * launch's block 0 seeing the doorbell; else block 0 starting) to the record's stores issued, by
 * the GPU's 100 MHz clock (s_memrealtime).  NaN before the first tick.  Not the step latency:
 * that adds the doorbell / launch and the record's path to the host. */
int llampc_ctl_device_us(llampc_ctl* ctl, double* us);
/* ConstantSpeed (planner.py:12-67) alone on the device with the controller's tables and Ts:
 * x0 [2], v0, horizon H (<= LLAMPC_HMAX), projidx, curr_mu, scale -> xref [2][H+1], the new
 * projidx (no lap wrap) and vr.  Blocking; leaves the controller state alone. */
int llampc_ctl_reference(llampc_ctl* ctl, const double* x0, double v0, int32_t H, int32_t projidx, double curr_mu,
                         double scale, double* xref, int32_t* projidx_out, double* vr);
/* The last tick's reference xref [2][H+1] and candidates U [C][H][2] (cfg.debug_inputs = 1).  A
 * fused-step solver (llampc_ctl_solver_create) needs the tick's reference in device memory and
 * switches the same copy on while it is attached: every tick then also stores its candidates
 * (16 C H bytes, by one block), and this call answers on a controller created without
 * debug_inputs too; both end when the solver is destroyed. */
int llampc_ctl_inputs(llampc_ctl* ctl, double* xref, double* U);
/* The input really applied after the last tick, when it is not the tick's own u_seq[0] (an NMPC
 * solve's, a safety override): u0 [2] -> CtlState.u_prev; useq [H][2] or NULL (keep the chosen
 * sequence, its row 0 replaced by u0) -> CtlState.useq, the next candidates' base.  The next tick's
 * look-back transition, du_0 and candidate base use the new values; the past record's u_seq stays as
 * it was.  Needs a completed tick and none outstanding (LLAMPC_E_STATE).  Values must be finite
 * (LLAMPC_E_ARG).  Takes the bank idle like every other call (cancels an armed launch).  Blocking. */
int llampc_ctl_set_applied(llampc_ctl* ctl, const double* u0, const double* useq);
/* ---- the soft track corridor inside the controller tick ----
 * The reference's constraints.py (Boundary(): the track's boundary lines linearised per step, with
 * slack variables in the NLP of nmpc.py:161-203) as a soft term of the candidate search: every
 * rolled-out (model, candidate) cost becomes J + weight x the summed squared slacks of the rollout's
 * positions on per-step half-planes hp_t [H][6] (llampc_plan_corridor's term).  hp_t is the track's
 * corridor (llampc.mpc.constraints.track_corridor, half width track_width / 2 - margin) along the
 * PREVIOUS tick's chosen rollout shifted one step (constraints.default_path's prev_xmpc rule), built
 * by H corridor blocks inside the tick's one launch; tick 0, the first tick after the corridor is
 * switched on and a tick after a non-finite chosen rollout use constraints.disabled(H).  Nothing in
 * hp_t depends on x_t.  The record, the reference, the candidates, the look-back, the selection and
 * mu-hat are unchanged; corridor ticks run the unstaged, unsplit look-ahead without speculative blocks.
 *
 * llampc_ctl_set_track: the centre line as llampc_nlp_set_track takes it (centre [2][n], theta [n]
 * from 0 strictly increasing, track_length > theta[n-1], track_width > 0; the same refusals,
 * LLAMPC_E_ARG).  LLAMPC_E_STATE with a tick outstanding or the corridor on.  Blocking. */
int llampc_ctl_set_track(llampc_ctl* ctl, const double* centre /* [2][n] */, const double* theta /* [n] */, int32_t n,
                         double track_length, double track_width);
/* weight > 0: the next ticks are corridor ticks; weight 0: off — the path state is invalidated and
 * the controller launches the plain tick again, its records those of a controller that never had a
 * corridor.  Cancels an armed launch first.  LLAMPC_E_STATE: no track set, a tick outstanding, or a
 * sharded controller (llampc_ctl_set_exchange / llampc_ctl_set_gather, which in turn refuse a
 * controller whose corridor is on).  LLAMPC_E_ARG: a weight that is negative or not finite, a margin
 * that is not finite or >= track_width / 2, a shape whose corridor tick exceeds the LDS.  Nothing is
 * enqueued either way. */
int llampc_ctl_set_corridor(llampc_ctl* ctl, double weight, double margin);
/* The last tick's corridor: the path P [2][H+1] it was built along (NaN when invalid), hp [H][6],
 * the path points' arc lengths theta [H] (NaN when invalid) and whether the path was valid.
 * Blocking, as llampc_ctl_inputs; LLAMPC_E_STATE unless the last tick was a corridor tick. */
int llampc_ctl_corridor(llampc_ctl* ctl, double* path, double* hp, double* theta, int32_t* valid);
/* Every rolled-out cost of the last corridor tick (cfg.debug_inputs = 1, for tests: the record carries
 * each slot's best alone): costs [nslots][C] in the record's slot order — while warm the nominal
 * model's one slot, else the top-K's K slots and then the selection's; a slot without a model is NaN.
 * Blocking, as llampc_ctl_inputs; LLAMPC_E_STATE without debug_inputs or a last corridor tick. */
int llampc_ctl_corridor_costs(llampc_ctl* ctl, double* costs /* [K + 1][C] */, int32_t* nslots);
/* llampc_ctl_variant for a corridor tick on a centre line of track_n points (host only): its nine
 * fields (s4 = 0), then the corridor block count (H). */
int llampc_ctl_variant_corridor(int64_t n, int32_t C, int32_t H, int32_t K, int32_t rl_n, int32_t track_n,
                                int32_t out[10]);
/* The controller over a bank SHARDED across ranks (BASELINE config 5: one process per GPU, each
 * rank's controller on its contiguous shard; replaces the single-process loop rt.py:269-366 with
 * its look-back over the whole bank).  Call on every rank before the first tick: `mb` is this
 * rank's mailbox with every peer open (llampc_mailbox_*), `gparams` [6][n_global] the whole
 * bank (rows Bf, Cf, Df, Br, Cr, Dr), copied to the device.  Then on every tick with a full
 * window the look-back's completing block pushes the shard's top-K and argmin (window mean,
 * global index) into every peer's mailbox, merges the `world` records (llampc_ctl_merge's order)
 * and publishes the merged selection: every rank rolls out the same K + 1 models from the global
 * table, so every rank's record and controller state equal the unsharded controller's.  All
 * ranks must tick the same number of times (the mailbox's tick number is the tag); the tick's
 * own launch does the exchange (no second kernel).  world <= 16, n_global < 2^32 - 1. */
int llampc_ctl_set_exchange(llampc_ctl* ctl, llampc_mailbox* mb, const double* gparams, int64_t n_global);
/* The same sharded controller over a GATHER transport (no peer mailbox; world <= 16): every
 * full-window tick is two launches on the bank's stream.  The first runs the look-back and
 * leaves this shard's record — llampc_ctl_record_words(K) words: its top-K and argmin as
 * (window mean, global index) entries, tagged with the exchange's tick number — in device
 * memory; the G records are all-gathered; the second launch merges them (the peer exchange's
 * merge, so the results are the same bitwise) and runs the look-ahead and the completion.
 * comm != NULL: the library issues ncclAllGather between the launches (stream-ordered, no host
 * round trip).  comm == NULL: the caller carries the records — after llampc_ctl_tick_async,
 * llampc_ctl_shard_record(ctl, words, &nw) waits for the first launch and returns this rank's
 * record (nw = 0: this tick has no exchange, e.g. the window is not full; llampc_ctl_wait
 * follows directly), the caller all-gathers the records of ranks 0..world-1 in rank order
 * (any transport) and passes them to llampc_ctl_resume, then llampc_ctl_wait as usual.  A
 * record whose tag does not match (ranks out of step) fails the tick (record status). */
int llampc_ctl_set_gather(llampc_ctl* ctl, int32_t world, int32_t rank, llampc_comm* comm, const double* gparams,
                          int64_t n_global);
int32_t llampc_ctl_record_words(int32_t K);
/* The launch shape of a controller tick past the warm-up with n models, a raceline of rl_n knots
 * and no exchange — host only, no device needed (for tests that mean to run one variant):
 * out = {lpm (look-ahead lanes per rollout: 4, 2 or 1), G (lanes per model), cpl (candidates per
 * lane), mpb (models per look-ahead block), s4 (1: the look-ahead's input terms are staged in LDS;
 * honours LLAMPC_CTL_NO_STAGE as llampc_ctl_create does), zfit (1: the candidates' variates are
 * pre-loaded per thread), R (look-back models per lane), nb_lb, nb_la (look-back / look-ahead
 * blocks)}.  LLAMPC_E_ARG for a shape llampc_ctl_create refuses. */
int llampc_ctl_variant(int64_t n, int32_t C, int32_t H, int32_t K, int32_t rl_n, int32_t out[9]);
int llampc_ctl_shard_record(llampc_ctl* ctl, uint64_t* words /* [llampc_ctl_record_words(K)] */, int32_t* nw);
int llampc_ctl_resume(llampc_ctl* ctl, const uint64_t* all_words /* [world][nw] */);
/* The sharded controller's merge on the host (the device exchange runs the same functions,
 * csrc/ctl.hpp): G records of K + 1 entries each — vals / gids [G][K+1], entries 0..K-1 the
 * shard's sorted top-K (gid -1: none), entry K its argmin — -> the merged top-K (argsort order
 * of rt.py:360: NaN last, ties to the lower global index; -1 padded) and argmin (rt.py:359;
 * NaN-first under LLAMPC_NAN_FIRST; -1 if none). */
int llampc_ctl_merge(const double* vals, const int64_t* gids, int32_t G, int32_t K, int32_t nan_policy,
                     int64_t* topk, double* topk_val, int64_t* best, double* best_val);
int llampc_ctl_destroy(llampc_ctl* ctl);

/* ---- setupNLP.solve drop-in ------------------------------------------------------ */
/* The selected model's NMPC (nmpc.py:14-203) on the device: the NLP's Euler transcription of
 * Dynamic.casadi (nmpc.py:58-60, dynamic.py:195-226), its objective (nmpc.py:44-111), the input
 * bounds and the rate bound (nmpc.py:102-105), minimised by the cross-entropy method: `iters`
 * rounds of `samples` sequences drawn from a per-(step, input) normal-like distribution (Philox
 * noise, clipped to the bounds, rate-clipped in order), the `elite` best setting the next mean
 * and std.  Replaces nlpsol/IPOPT (nmpc.py:146-157, 192), which this platform lacks: the
 * optimum is NOT IPOPT's (parity unpinned).  The bank holds the ONE model (n = 1).  Every
 * round runs in one launch (every block completes every round from the others' tagged lists;
 * LLAMPC_NLP_ROUND_LAUNCHES=1 in the environment at create: one launch per round).  The solve's
 * inputs travel as kernel arguments (no host-to-device copy). */
typedef struct llampc_nlp_cfg {
  int32_t H, samples, iters, elite;  /* samples: power of two in [64, 4096]; 1 <= elite <= 64      */
  double Ts;
  double sigma0[2];                  /* the first iteration's std per input                     */
  double std_floor;                  /* added to every elite std                                 */
  uint64_t seed;
  llampc_cost cost;                  /* Q, R, P, bounds; rate_max: the symmetric feasibility bound */
  double rate_lo[2], rate_hi[2];     /* per-step rate bounds already x Ts (min_rates / max_rates x
                                        Ts); rate_lo > rate_hi: none on that input             */
} llampc_nlp_cfg;
typedef struct llampc_nlp llampc_nlp;
int llampc_nlp_create(llampc_bank* bank, const llampc_nlp_cfg* cfg, llampc_nlp** out);
/* x0 [6], xref [2][H+1], uprev [2], base [H][2] (the first mean: the previous solution shifted,
 * or NULL = uprev held); has_hold = 1 adds the held uprev as a candidate of the first round.
 * -> umpc [H][2], fval, xmpc [H+1][6] (the Euler trajectory of umpc).  Blocking. */
int llampc_nlp_solve(llampc_nlp* nlp, const double* x0, const double* xref, const double* uprev,
                     const double* base, int32_t has_hold, double* umpc, double* fval, double* xmpc);
/* The same solve under a soft corridor: hp [H][6], row k - 1 = (a0, a1, b, c0, c1, d) the two
 * half-planes a.p_k <= b and c.p_k <= d on the position p_k = (X, Y) after k Euler steps, k = 1..H
 * (a = (0, 0), b = +inf disables one).  Every sample's objective becomes J + weight x pen, pen =
 * sum_k max(a.p_k - b, 0)^2 + max(c.p_k - d, 0)^2 (k ascending, every product and sum rounded on
 * its own); the bounds, the rate chain, the ranking and the warm start are llampc_nlp_solve's, and a
 * corridor that no sample touches returns its umpc and fval bitwise.  fval includes the penalty;
 * -> max_slack (may be NULL): the largest max(a.p_k - b, c.p_k - d, 0) along the returned xmpc.
 * LLAMPC_E_ARG, with nothing launched: hp NULL, a non-finite normal component, an offset NaN or
 * -inf, weight negative or non-finite.  hp travels through the solver's pinned mapped buffer.
 * Blocking. */
int llampc_nlp_solve_corridor(llampc_nlp* nlp, const double* x0, const double* xref, const double* uprev,
                              const double* base, int32_t has_hold, const double* hp, double weight,
                              double* umpc, double* fval, double* xmpc, double* max_slack);
/* The track for the device-built corridor: the centre line centre [2][n] (x row, y row), the arc
 * length theta [n] at every centre point and the closed length, as the Track object holds them
 * (center_line, theta_track, track_length: they are NOT recomputed here, NumPy's sums round in
 * their own order), and the track's width.  Copies the tables to the device; a second call replaces
 * the track.  LLAMPC_E_ARG: n outside [2, 4096], a non-finite value, theta[0] != 0 or theta not
 * strictly increasing, track_length <= theta[n-1] or <= 0.2 (four times the tangent's 0.05 m arc
 * step), track_width <= 0.  Blocking. */
int llampc_nlp_set_track(llampc_nlp* nlp, const double* centre /* [2][n] */, const double* theta /* [n] */,
                         int32_t n, double track_length, double track_width);
/* The track's corridor along a path on the device (csrc/corridor_dev.hpp, one small kernel):
 * path [2][H+1] = P_0 .. P_H with the solver's H (P_0 is not read) -> hp [H][6], row k - 1 the two
 * half-planes |n.(p - c)| <= track_width / 2 - margin across the centre line at P_k's nearest point
 * (llampc.mpc.constraints.track_corridor in scalar form: nearest segment of the closed centre line,
 * ties to the lower one; the tangent from the centre line 0.05 m of arc length either side), and
 * theta [H] (may be NULL), that point's arc length.  The centre-line lookup extrapolates the last
 * segment over the closing gap, as Track.param_to_xy does, and is discontinuous at vertex 0.
 * LLAMPC_E_STATE with no track set; LLAMPC_E_ARG, with nothing launched: a non-finite path entry, a
 * margin that is not finite or >= track_width / 2.  Blocking (as llampc_ctl_reference is the
 * controller's reference alone, this is the corridor alone). */
int llampc_nlp_track_corridor(llampc_nlp* nlp, const double* path /* [2][H+1] */, double margin,
                              double* hp /* [H][6] */, double* theta /* [H], may be NULL */);
/* llampc_nlp_solve_corridor with the track's corridor along `path`, built on the device: the
 * corridor kernel, then the corridor solve's launch on the bank's stream, with no host
 * synchronisation between the two and one completion wait, as every solve.  The kernel writes hp
 * into the solver's pinned mapped buffer, where the solve reads it and where the host reads it
 * after the completion tag: -> max_slack (may be NULL) of the returned xmpc on it, hp_out [H][6]
 * (may be NULL) a copy.  LLAMPC_E_STATE and LLAMPC_E_ARG as llampc_nlp_track_corridor, LLAMPC_E_ARG
 * also for a weight negative or non-finite; LLAMPC_E_DEVICE if the read-back corridor is not a
 * valid one.  Blocking. */
int llampc_nlp_solve_track(llampc_nlp* nlp, const double* x0, const double* xref, const double* uprev,
                           const double* base, int32_t has_hold, const double* path /* [2][H+1] */,
                           double margin, double weight, double* umpc, double* fval, double* xmpc,
                           double* max_slack, double* hp_out /* [H][6], may be NULL */);
int llampc_nlp_destroy(llampc_nlp* nlp);

/* ---- batched setupNLP.solve: B problems of a model bank in one launch ---------------- */
/* The reference builds one setupNLP per bank model (rt.py:195-202) and solves each tick with the
 * model the look-back selected (rt.py:305).  One solver handle per model does not scale to a bank
 * of 10^4; this solver is bound to the whole bank (any n >= 1, borrowed: destroy the solver first)
 * and solves B independent problems per call in ONE launch, each with its own bank model (by
 * index: e.g. llampc_plan_out.sel_model and topk), state, reference, previous input, warm start
 * and Philox seed, each on its own samples / 64 blocks (csrc/nlp_batch.hip).  The vehicle
 * constants are the bank's, the cost, bounds, rates and shape the cfg's, shared by the batch.
 * A problem's search is llampc_nlp_solve's, bit for bit: problem p of the handle's c-th call
 * (c = 0, 1, ..: one solve number per call, the Philox call word of every problem of it) draws
 * the noise of the c-th call of a single solver created with seed[p].
 * The problems' blocks wait for each other's rounds, so max_batch x samples / 64 must not exceed
 * the device's CU count (LLAMPC_E_ARG at create), and a batch of B holds B x samples / 64 CUs
 * for the solve's duration.  The cfg checks are llampc_nlp_create's. */
typedef struct llampc_nlp_batch llampc_nlp_batch;
int llampc_nlp_batch_create(llampc_bank* bank, const llampc_nlp_cfg* cfg, int32_t max_batch,
                            llampc_nlp_batch** out);
/* -> max_batch and the CU count read at the bank's create (either may be NULL). */
int llampc_nlp_batch_info(const llampc_nlp_batch* nb, int32_t* max_batch, int32_t* cus);
/* status[p] of a problem */
enum llampc_nlp_status { LLAMPC_NLP_OK = 0,
                         LLAMPC_NLP_NO_FINITE = 1,   /* no finite objective in any round         */
                         LLAMPC_NLP_NO_TAG = 2 };    /* its completion tag never arrived          */
/* model_idx [B] in [0, n); seed [B] or NULL (= cfg.seed for all); x0 [B][6]; xref [B][2][H+1];
 * uprev [B][2]; base [B][H][2] or NULL (every first mean = uprev held; a problem whose has_hold
 * is 0 ignores its row of base and holds uprev too, so warm and cold slots mix in one call);
 * has_hold [B] -> umpc [B][H][2], fval [B], xmpc [B][H+1][6], status [B].  The host writes the
 * inputs into a pinned mapped buffer, launches once and waits for the B completion tags with one
 * bounded wait.  Returns LLAMPC_OK when every problem reported: a problem's failure is its
 * status, with umpc zeros and fval +inf, and stops no other problem.  LLAMPC_E_ARG, with nothing
 * launched and the bank's launch counter unchanged: a NULL pointer (seed and base excepted),
 * B < 1 or B > max_batch, a model index outside [0, n).  Blocking. */
int llampc_nlp_batch_solve(llampc_nlp_batch* nb, int32_t B, const int64_t* model_idx, const uint64_t* seed,
                           const double* x0, const double* xref, const double* uprev, const double* base,
                           const int32_t* has_hold, double* umpc, double* fval, double* xmpc, int32_t* status);
/* llampc_nlp_batch_solve under a soft corridor per problem (csrc/nlp_batch_corr.hip), still ONE
 * launch: hp [B][H][6], problem p's half-planes as llampc_nlp_solve_corridor takes them (a problem
 * that wants none passes rows (0, 0, +inf, 0, 0, +inf)), and weight [B], problem p's own.  Problem
 * p's search is llampc_nlp_solve_corridor's with hp[p] and weight[p], bit for bit; with every
 * half-plane disabled it is llampc_nlp_batch_solve's.  fval includes the penalty.  -> max_slack [B]:
 * the largest slack along problem p's returned xmpc on hp[p], computed on the host; 0 for a problem
 * whose status is not LLAMPC_NLP_OK.  The corridors travel in a pinned mapped buffer of their own;
 * the problems' records are llampc_nlp_batch_solve's.  LLAMPC_E_ARG, with nothing launched and the
 * launch counter unchanged: what llampc_nlp_batch_solve refuses, hp, weight or max_slack NULL, and
 * for any problem (its index is in the message) a non-finite normal component, an offset NaN or
 * -inf, a weight negative or non-finite.  The call number advances as llampc_nlp_batch_solve's
 * does.  Blocking. */
int llampc_nlp_batch_solve_corridor(llampc_nlp_batch* nb, int32_t B, const int64_t* model_idx, const uint64_t* seed,
                                    const double* x0, const double* xref, const double* uprev, const double* base,
                                    const int32_t* has_hold, const double* hp /* [B][H][6] */,
                                    const double* weight /* [B] */, double* umpc, double* fval, double* xmpc,
                                    int32_t* status, double* max_slack /* [B] */);
/* The track for the device-built corridors, as llampc_nlp_set_track takes it (the same checks).
 * One track per solver: two tracks are two solvers, or host-built hp.  Blocking. */
int llampc_nlp_batch_set_track(llampc_nlp_batch* nb, const double* centre /* [2][n] */,
                               const double* theta /* [n] */, int32_t n, double track_length, double track_width);
/* The track's corridors along B paths on the device (csrc/corridor_batch.hip: one kernel of B x H
 * blocks): path [B][2][H+1] -> hp [B][H][6] and theta [B][H] (may be NULL), each problem's as
 * llampc_nlp_track_corridor builds them.  LLAMPC_E_STATE with no track set; LLAMPC_E_ARG, with
 * nothing launched: B < 1 or B > max_batch, a non-finite path entry (the problem is named), a
 * margin that is not finite or >= track_width / 2.  Blocking. */
int llampc_nlp_batch_track_corridor(llampc_nlp_batch* nb, int32_t B, const double* path /* [B][2][H+1] */,
                                    double margin, double* hp /* [B][H][6] */, double* theta /* [B][H] or NULL */);
/* llampc_nlp_batch_solve_corridor with the track's corridors along the problems' paths, built on
 * the device: the corridor kernel, then the search, on the bank's stream with no host
 * synchronisation between the two and one wait for the B tags (two launches).  -> max_slack [B] on
 * the built half-planes, hp_out [B][H][6] (may be NULL) a copy of them.  LLAMPC_E_STATE and
 * LLAMPC_E_ARG as llampc_nlp_batch_track_corridor and llampc_nlp_batch_solve_corridor (weights);
 * LLAMPC_E_DEVICE if a read-back corridor is not a valid one.  Blocking. */
int llampc_nlp_batch_solve_track(llampc_nlp_batch* nb, int32_t B, const int64_t* model_idx, const uint64_t* seed,
                                 const double* x0, const double* xref, const double* uprev, const double* base,
                                 const int32_t* has_hold, const double* path /* [B][2][H+1] */, double margin,
                                 const double* weight /* [B] */, double* umpc, double* fval, double* xmpc,
                                 int32_t* status, double* max_slack /* [B] */, double* hp_out /* [B][H][6] or NULL */);
int llampc_nlp_batch_destroy(llampc_nlp_batch* nb);

/* ---- the fused control step: the tick and the selected model's NMPC solve, one chain ------ */
/* The reference's control step (rt.py:269-366): the look-back selects a model, THAT model's NMPC is
 * solved (nlp_bank[current_model_idx].solve, rt.py:303-305; nlp_initial while the window fills), the
 * solve's first input is applied, and the next look-back scores the bank on the transition under the
 * input that was applied.  llampc_ctl_step enqueues all of it on the bank's stream with no host
 * synchronisation in between and ONE pair of host waits at the end:
 *   0. snapshot  CtlState.u_prev (zeros before the first tick) -> the solve's du_0 reference
 *   1. the tick  exactly llampc_ctl_tick_async's launch (same prepare / commit, same kernel); with a
 *                solver attached it also leaves its reference xref [2][H+1] in device memory
 *   2. build     one block writes the solve's problem in device memory: x0 = x_t, the tick's xref, the
 *                first mean = the tick's chosen sequence (not shifted), uprev = the snapshot, has_hold
 *                = 1; and the model: cfg.nominal of the controller while the tick was warm, else the
 *                bank column the tick selected
 *   3. the solve llampc_nlp_batch_solve's kernel, B = 1, unmodified (its result in device memory)
 *   4. commit    one block: a solve with a finite objective becomes the applied sequence
 *                (CtlState.u_prev <- umpc[0], CtlState.useq <- umpc; committed = 1); otherwise the
 *                state stays as the tick left it and the tick's candidate is the applied input.  Then
 *                the result into the pinned llampc_ctl_solve_out and its tag.
 * The host waits for the tick's tag (llampc_ctl_wait's path), then the commit's.  The solve's Philox
 * call word is the number of steps this solver has run (plain ticks in between do not count); it
 * advances whatever the waits returned.  llampc_bank_timing brackets the whole chain as one launch
 * group; llampc_bank_launches counts the tick and the solve (2 per step), each once it is enqueued.
 *
 * cfg is llampc_nlp_create's, with H and Ts equal to the controller's (LLAMPC_E_ARG), samples / 64 <=
 * 64 and <= the device's CUs (every round in one launch).  The solver borrows the controller and its
 * bank: destroy the solver first.  LLAMPC_E_STATE, with nothing launched and the launch counter
 * unchanged: create on a controller with prelaunch on, with an exchange or a gather transport, with a
 * corridor weight > 0, with a tick outstanding or with a solver already; and, while a solver is
 * attached, llampc_ctl_set_prelaunch(1), llampc_ctl_set_corridor(weight > 0), llampc_ctl_set_exchange
 * and llampc_ctl_set_gather.  A plain llampc_ctl_tick stays allowed: its candidate is then the applied
 * input.  Not part of this interface: armed, sharded or corridor fused steps (refused as above), the
 * top-K's side problems, and an asynchronous step_begin / step_end pair. */
typedef struct llampc_ctl_solver llampc_ctl_solver;
typedef struct llampc_ctl_solve_out {
  double umpc[LLAMPC_HMAX][2];     /* [H][2]; zeros unless status == LLAMPC_NLP_OK               */
  double xmpc[LLAMPC_HMAX + 1][6]; /* [H+1][6] the NLP's Euler trajectory of umpc                */
  double fval;                     /* +inf unless status == LLAMPC_NLP_OK                        */
  double uprev[2];                 /* du_0's reference: the state's u_prev as the tick read it   */
  int64_t model;                   /* global index solved with; -1: the nominal model (warm)     */
  int32_t status;                  /* LLAMPC_NLP_OK / _NO_FINITE / _NO_TAG                       */
  int32_t committed;               /* 1: umpc is now the controller's applied sequence           */
} llampc_ctl_solve_out;
int llampc_ctl_solver_create(llampc_ctl* ctl, const llampc_nlp_cfg* cfg, llampc_ctl_solver** out);
/* x_t [6] -> the tick's record and the solve's.  Blocking. */
int llampc_ctl_step(llampc_ctl_solver* s, const double* x_t, llampc_ctl_out* out, llampc_ctl_solve_out* sol);
int llampc_ctl_solver_destroy(llampc_ctl_solver* s);

/* ---- raw batched dynamics (Dynamic API parity) ---------------------------------- */
/* x [n][6], u [n][2]; params [6][P] with P == 1 (one model broadcast) or P == n.
 * OP_FORCES -> out [5][n] = (Ffy, Frx, Fry, alphaf, alphar)   (dynamic.py:117-154)
 * OP_DERIV  -> out [n][6]                                      (dynamic.py:98-115)
 * device_ptrs: 0 = host arrays (blocking), 1 = device arrays (async on stream). */
int llampc_dynamics_batch(int32_t op, const double* x, const double* u,
                          const double* params, int64_t P, const llampc_vehicle* veh,
                          int64_t n, double* out, int32_t device, int32_t device_ptrs,
                          void* stream);
/* S successive integration steps per lane: x0 [n][6]; u [n][S][2] (u_stride_lane =
 * S*2) or [S][2] broadcast (u_stride_lane = 0); h [S] step sizes; traj_out
 * [S+1][n][6] (full trajectory) or [n][6] (final state only, when final_only=1). */
int llampc_integrate_batch(const double* x0, const double* u, int64_t u_stride_lane,
                           const double* h, int32_t S, const double* params, int64_t P,
                           const llampc_vehicle* veh, int64_t n, int32_t integrator,
                           double* traj_out, int32_t final_only, int32_t device,
                           int32_t device_ptrs, void* stream);

/* ---- model transcendentals (accuracy tests) -------------------------------------- */
/* The fp64 atan2 (x >= 0) / atan / sin / cos the kernels use (csrc/fastmath.hpp),
 * elementwise on host arrays: out[i] = f(a[i][, b[i]]).  0-3: the general versions (any
 * argument); 4-9: the branch-free cores of the rollout stage, defined on their domains only
 * (atan2: |a| + b in [2^-1000, 2^1000], b >= 0; atan: |a| <= 2^1000; sin_wide: |a| <= 3;
 * sincos: |a| <= 2^20 pi/2) — the stage re-does out-of-domain lanes with 0-3; 9 = a / 6. */
enum llampc_math_fn { LLAMPC_MATH_ATAN2_XPOS = 0, LLAMPC_MATH_ATAN = 1, LLAMPC_MATH_SIN = 2,
                      LLAMPC_MATH_COS = 3, LLAMPC_MATH_ATAN2_FAST = 4, LLAMPC_MATH_ATAN_FAST = 5,
                      LLAMPC_MATH_SIN_WIDE = 6, LLAMPC_MATH_SIN_FAST = 7, LLAMPC_MATH_COS_FAST = 8,
                      LLAMPC_MATH_DIV6 = 9,
                      /* the look-ahead's lean cores (fastmath.hpp kAtanRL / kSinWQL) */
                      LLAMPC_MATH_ATAN2_LEAN = 10, LLAMPC_MATH_ATAN_LEAN = 11,
                      LLAMPC_MATH_SIN_WIDE_LEAN = 12,
                      /* the LPM-1 look-ahead lane's paired lean cores (front and rear division
                         through one reciprocal): out[i] = the first result of the pair
                         (a[i], a[n-1-i]) — atan2 with x = b[i], or atan */
                      LLAMPC_MATH_ATAN2_PAIR = 13, LLAMPC_MATH_ATAN_PAIR = 14 };
int llampc_math_batch(int32_t fn, const double* a, const double* b, int64_t n, double* out,
                      int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* LLAMPC_H_ */

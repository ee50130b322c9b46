// kernels.hip — gfx950 (CDNA4) kernels of the LLA-MPC model-bank hot path.
//
//   lookback_kernel    one lane per model: RK4 step from (x_{t-1}, u_{t-1}), 4-state MSE
//                      against x_t, in-place ring write, W-window mean in NumPy's pairwise
//                      order, then per-block argmin + top-K by wave64 shuffles.
//                      Reference: evaluate_models_vectorized.py:4-24, rt.py:347-366.
//   lookahead_kernel   one lane per (model, candidate): H-step rollout (RK4 / NLP-Euler /
//                      RK6) with the MPC objective accumulated in registers; candidates'
//                      controls and xref staged in LDS; group (per-model) argmin over the
//                      candidates by xor-shuffles; per-block argmin.
//                      Reference: model.py:32-40 composed H times + nmpc.py:44-111.
//   select_kernel      one block: merges the per-block partials into llampc_plan_out.
//   merge_kernel       cross-shard merge after the RCCL all-gather (merge.hpp).
//   dynamics_kernel / integrate_kernel   raw batched Dynamic API (dynamic.py:98-154,
//                      model.py:18-40, rk6.py).
//   track_corridor_kernel   one block per horizon step: the track's half-planes along a path
//                      (corridor_dev.hpp; constraints.track_corridor on the device).
//
// This translation unit: the plan-launch dispatcher (launch_plan) and the non-plan kernels.
// The plan kernels are in plan_dev.hpp (their device code in the *_dev.hpp role headers), their
// instantiations in plan_*.hip
// (one TU per variant group, so the library builds in parallel), the controller tick in ctl.hip.
#include <type_traits>

#include "dev_wave.hpp"
#include "final_dev.hpp"
#include "lookback_dev.hpp"
#include "peer_dev.hpp"
#include "rollout_dev.hpp"

namespace llampc {

__global__ __launch_bounds__(kBlock) void merge_kernel(const llampc_plan_out* parts, int32_t G,
                                                       int32_t nan_first, llampc_plan_out* m) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  // the G gathered records -> LDS in ONE round trip of 16-B loads (every later read is LDS)
  llampc_plan_out* rec = reinterpret_cast<llampc_plan_out*>(smem);
  constexpr int kWords = sizeof(llampc_plan_out) / 16;
  static_assert(sizeof(llampc_plan_out) % 16 == 0, "records staged as 16-B words");
  const uint4* srcw = reinterpret_cast<const uint4*>(parts);
  uint4* dstw = reinterpret_cast<uint4*>(rec);
  for (int e = tid; e < G * kWords; e += kBlock) dstw[e] = srcw[e];
  __syncthreads();
  merge_staged(rec, G, nan_first, m, reinterpret_cast<EntS*>(smem + (size_t)G * sizeof(llampc_plan_out)), 0);
}

// Peer exchange (xGMI, no collective library): every rank's mailbox is uncached device
// memory mapped into every peer process (IPC).  One block per rank per tick:
//  1. push — this rank's record as tagged 64-bit words (tick seq << 32 | 32 payload bits)
//     into slot [seq & 1][rank] of every peer's mailbox, system-scope stores that go straight
//     over xGMI into the peer's HBM (its own copy goes straight to LDS);
//  2. poll — every thread spins on its share of the G slots of its own mailbox until each
//     word carries this tick's seq (every word validates itself: no fence pairing across
//     devices), unpacking the payloads into the LDS records;
//  3. merge_staged — the same merge as merge_kernel.
// Two slots by tick parity: a peer can only push tick t+2 after its own exchange of t+1,
// which needs this rank's push of t+1, issued after this rank's exchange of t has finished
// reading slot (t & 1) — so a slot is never overwritten while it is read.  A poll that
// waits longer than `bound` (s_memrealtime ticks) gives status LLAMPC_STATUS_POLL_TIMEOUT.
__global__ __launch_bounds__(kBlock) void peer_exchange_kernel(PeerLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int kW = kRecWords;
  const int tid = threadIdx.x;
  const int G = a.G;
  const size_t slot0 = (size_t)(a.seq & 1) * G * kW;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.local);
  uint32_t* rec32 = reinterpret_cast<uint32_t*>(smem);
  for (int w = tid; w < kW; w += kBlock) {
    const uint32_t x = src[w];
    rec32[a.rank * kW + w] = x;                 // this rank's record: straight to LDS
    const uint64_t v = tag_word(a.seq, x);
    const size_t off = slot0 + (size_t)a.rank * kW + w;
    for (int g = 0; g < G; ++g)
      if (g != a.rank) __hip_atomic_store(a.box[g] + off, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const uint64_t* own = a.box[a.rank] + slot0;
  constexpr int kPerK = (kPeerMax * kRecWords + kBlock - 1) / kBlock;
  int late = poll_mailbox<kPerK>(own, G, a.rank, a.seq, a.bound, rec32);
  // one flag per wave after the lists (no static LDS: the launch asks for all 160 KB)
  EntS* lists = reinterpret_cast<EntS*>(smem + (size_t)G * sizeof(llampc_plan_out));
  int* wave_late = reinterpret_cast<int*>(lists + 2 * (size_t)G * LLAMPC_KMAX);
  const int wl = __any(late);
  if ((tid & 63) == 0) wave_late[tid >> 6] = wl;
  __syncthreads();
  late = 0;
  for (int w = 0; w < kBlock / 64; ++w) late |= wave_late[w];
  if (late) {                                   // block-uniform
    peer_timeout_record(rec32, a.rank, a.merged);
    return;
  }
  merge_staged(reinterpret_cast<const llampc_plan_out*>(smem), G, a.nan_first, a.merged, lists, 0);
}

// ------------------------------------------------------------------------------------
// Raw batched dynamics (Dynamic API)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void dynamics_kernel(int32_t op, const double* x,
                                                          const double* u, const double* params,
                                                          int64_t P, VehK veh, int64_t n,
                                                          double* out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const Tire t = load_tire(params, P, P == 1 ? 0 : i);
  double xi[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) xi[j] = x[6 * i + j];
  if (op == LLAMPC_OP_FORCES) {
    const Forces f = forces<Form::Ref>(veh, t, xi[3], xi[4], xi[5], u[2 * i], u[2 * i + 1]);
    out[i] = f.Ffy;
    out[n + i] = f.Frx;
    out[2 * n + i] = f.Fry;
    out[3 * n + i] = f.af;
    out[4 * n + i] = f.ar;
  } else {
    const Input in = make_input(u[2 * i], u[2 * i + 1]);
    double d[6];
    rhs<Form::Ref>(veh, t, xi, in, d);
#pragma unroll
    for (int j = 0; j < 6; ++j) out[6 * i + j] = d[j];
  }
}

// Elementwise transcendentals of the model (accuracy tests of fastmath.hpp).
__global__ __launch_bounds__(kBlock) void math_kernel(int32_t fn, const double* a, const double* b,
                                                      int64_t n, double* out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double r = 0.0, s, c;
  const fm::FmK K = fm::FmK::load();
  switch (fn) {
    case 0: r = LL_ATAN2P(a[i], b[i]); break;
    case 1: r = LL_ATAN(a[i]); break;
    case 2: LL_SINCOS(a[i], &s, &c); r = s; break;
    case 3: LL_SINCOS(a[i], &s, &c); r = c; break;
    case 4: r = fm::atan2_fast(a[i], b[i], K); break;
    case 5: r = fm::atan_fast(a[i], K); break;
    case 6: r = fm::sin_wide(a[i], K); break;
    case 7: fm::sincos_fast(a[i], &s, &c, K); r = s; break;
    case 8: fm::sincos_fast(a[i], &s, &c, K); r = c; break;
    case 9: r = fm::div6(a[i], K); break;
    case 10: r = fm::atan2_fast<true>(a[i], b[i], fm::FmK::load<true>()); break;
    case 11: r = fm::atan_fast<true>(a[i], fm::FmK::load<true>()); break;
    case 12: r = fm::sin_wide<true>(a[i], fm::FmK::load<true>()); break;
    case 13:   // paired atan2 (dyn.hpp chain_pair): partner element n-1-i, the same x
    case 14: { // paired atan: partner element n-1-i
      const int64_t j = n - 1 - i;
      double af, ar, hf, hr, dp;
      if (fn == 13) fm::atan2_fast_pair(a[i], a[j], b[i], fm::FmK::load<true>(), af, ar, hf, hr, dp);
      else fm::atan_fast_pair(a[i], a[j], fm::FmK::load<true>(), af, ar, dp);
      r = af;
      break;
    }
    default: r = __builtin_nan("");
  }
  out[i] = r;
}

// The track corridor along a path (corridor_dev.hpp; llampc_nlp_track_corridor and, ahead of the
// corridor solve on the same stream, llampc_nlp_solve_track).  One block per step k = 1..H.  The
// block first copies the track's three tables into its LDS (24 n bytes, 16 KB on ETHZ: independent
// loads, one memory round trip), and everything after reads them there — with the tables in global
// memory the bisection's ten dependent loads alone, cold in the block's L2, made the kernel 8.8 us
// long (DESIGN §3 "The corridor").  Each thread takes the segments j = tid (mod 256) in ascending
// order, the (d2, j) pairs are reduced over the wave (DPP) and over the four waves (LDS) with ties
// to the lower j; wave 0 then looks up the centre and the tangent's two points in lanes 0, 1, 2 and
// lane 0 stores row k - 1 and theta_k with plain vector stores.  No block waits on anything.  hp
// is the device alias of pinned host memory in both callers: the system-scope fence orders the row
// before the kernel's end.  Dynamic LDS: sv [4] | si [4] | cx [n] | cy [n] | tt [n].
constexpr size_t kCorridorScratch = 64;
__global__ __launch_bounds__(kBlock) void track_corridor_kernel(TrackK g, CorridorPath path, int32_t H, double hw,
                                                                double* hp, double* theta_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* sv = reinterpret_cast<double*>(smem);
  int64_t* si = reinterpret_cast<int64_t*>(smem + 32);
  double* lx = reinterpret_cast<double*>(smem + kCorridorScratch);
  double* ly = lx + g.n;
  double* lt = ly + g.n;
  const int tid = threadIdx.x;
  const int k = blockIdx.x + 1;
  const double px = path.v[k], py = path.v[H + 1 + k];
#pragma unroll 4
  for (int j = tid; j < g.n; j += kBlock) {
    lx[j] = g.cx[j];
    ly[j] = g.cy[j];
    lt[j] = g.tt[j];
  }
  __syncthreads();
  const TrackK t{lx, ly, lt, g.n, 0, g.L};
  // a lane with no segment holds (NaN, kNoIndex): last under the NaN-last order
  double bd2 = __builtin_nan("");
  int64_t bj = kNoIndex;
  for (int j = tid; j < t.n; j += kBlock) {
    const double d2 = corridor_seg_d2(t, j, px, py);
    if (bj == kNoIndex || d2 < bd2) {
      bd2 = d2;
      bj = j;
    }
  }
  wave_min<0>(bd2, bj);
  if ((tid & 63) == 0) {
    sv[tid >> 6] = bd2;
    si[tid >> 6] = bj;
  }
  __syncthreads();
  if (tid >= 64) return;
  bd2 = sv[0];
  bj = si[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; ++w) {
    if (less_nan_last(sv[w], si[w], bd2, bj)) {
      bd2 = sv[w];
      bj = si[w];
    }
  }
  const int j = (int)(bj < 0 ? 0 : (bj > t.n - 1 ? t.n - 1 : bj));   // inside the tables whatever the path
  const double theta = corridor_theta(t, j, px, py);
  double x, y;
  corridor_param_to_xy(t, corridor_lookup_theta(theta, t.L, tid < 3 ? tid : 0), x, y);
  const double fx = readlane_d(x, 1), fy = readlane_d(y, 1);
  const double bx = readlane_d(x, 2), by = readlane_d(y, 2);
  if (tid == 0) {
    double row[6];
    corridor_row(x, y, fx, fy, bx, by, hw, row);
    double* out = hp + 6 * (size_t)(k - 1);
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = row[i];
    if (theta_out) theta_out[k - 1] = theta;
    __threadfence_system();
  }
}

template <int INTEG>
__global__ __launch_bounds__(kBlock) void integrate_kernel(const double* x0, const double* u,
                                                           int64_t us, const double* h, int32_t S,
                                                           const double* params, int64_t P,
                                                           VehK veh, int64_t n, double* traj,
                                                           int32_t final_only) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const Tire t = load_tire(params, P, P == 1 ? 0 : i);
  double x[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) x[j] = x0[6 * i + j];
  if (!final_only) {
#pragma unroll
    for (int j = 0; j < 6; ++j) traj[6 * i + j] = x[j];
  }
  for (int s = 0; s < S; ++s) {
    const Input in = make_input(u[i * us + 2 * s], u[i * us + 2 * s + 1]);
    step<INTEG>(veh, t, x, in, h[s]);
    if (!final_only) {
#pragma unroll
      for (int j = 0; j < 6; ++j) traj[((int64_t)(s + 1) * n + i) * 6 + j] = x[j];
    }
  }
  if (final_only) {
#pragma unroll
    for (int j = 0; j < 6; ++j) traj[6 * i + j] = x[j];
  }
}

// ------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------
// Compute units of the current device (cached): the work-queue layout launches one
// look-ahead block per CU, minus the one the completing look-back block holds.
static int device_cus() {
  static int cus[64] = {};
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return 256;
  if (!cus[d]) {
    int c = 0;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || c < 2) c = 256;
    cus[d] = c;
  }
  return cus[d];
}

// f(I, L) with the runtime (integrator, lanes per rollout) of an RK4 or NLP-Euler launch as
// std::integral_constants: the instantiated variant groups of kernels.hpp, {0, 1} x {4, 2, 1}.
template <class F>
static void with_variant(int integ, int lpm, F&& f) {
  const auto with_lpm = [&](auto I) {
    if (lpm == 4) f(I, std::integral_constant<int, 4>{});
    else if (lpm == 2) f(I, std::integral_constant<int, 2>{});
    else f(I, std::integral_constant<int, 1>{});
  };
  if (integ == LLAMPC_RK4) with_lpm(std::integral_constant<int, 0>{});
  else with_lpm(std::integral_constant<int, 1>{});
}

hipError_t launch_plan(const LookbackLaunch* lb, const LookaheadLaunch* la, FinalLaunch f,
                       hipStream_t s, const InlinePack* pk, int32_t share, const PlanCorridor* cor,
                       const PlanTrack* trk) {
  if (cor && !cor->hp) return hipErrorInvalidValue;
  if (trk && (trk->trk.n < 2 || trk->trk.n > kTrackMaxPoints || !trk->hp_tag)) return hipErrorInvalidValue;
  // 1. the launch's shape (launch_shape.hpp): the one place that decides it, or refuses
  PlanShapeIn in{};
  in.n = lb ? lb->n : la ? la->n : 0;
  in.lb = lb != nullptr;
  if (lb) {
    in.K = lb->K;
    in.full = lb->full != 0;
  }
  in.la = la != nullptr;
  if (la) {
    in.C = la->C;
    in.H = la->H;
    in.integrator = la->integrator;
    in.xref_mode = la->xref_mode;
    in.rl_n = la->rl.n;
    in.rl_M = la->rl.M;
    in.wq_counter = la->wq != nullptr;
  }
  in.share = share;
  in.px_G = f.px_G;
  in.pack = pk != nullptr;
  in.corridor = cor != nullptr;
  in.track_n = trk ? trk->trk.n : 0;
  const PlanShape sh = plan_shape(in, device_cus());
  if (sh.refuse) return hipErrorInvalidValue;
  // 2. what the kernels read of it
  LookbackLaunch lbv{};
  LookaheadLaunch lav{};
  if (lb) {
    lbv = *lb;
    lbv.R = sh.R;
  }
  if (la) {
    lav = *la;
    lav.rl.wcap = sh.wcap;
  }
  f.nb_lb = sh.nb_lb;
  f.nb_la = sh.nb_la;
  f.do_lb = lb != nullptr;
  f.do_la = la != nullptr;
  // 3. the variant group's launcher
  if (trk) {
    launch_plan_track(lbv, lav, f, sh.G, sh.cpl, sh.stage, sh.lpm, sh.lds, s, *trk);
  } else if (sh.integ == LLAMPC_RK6) {
    launch_plan_group<2, 1>(lbv, lav, f, sh.G, sh.cpl, sh.stage, sh.lds, s, 0);
  } else {
    with_variant(sh.integ, sh.lpm, [&](auto I, auto L) {
      constexpr int kI = decltype(I)::value, kL = decltype(L)::value;
      if (pk) launch_plan_inline_group<kL>(lbv, lav, f, sh.G, sh.cpl, sh.lds, s, *pk);
      else if (cor) launch_plan_corridor_group<kI, kL>(lbv, lav, f, sh.G, sh.cpl, sh.stage, sh.lds, s, *cor);
      else launch_plan_group<kI, kL>(lbv, lav, f, sh.G, sh.cpl, sh.stage, sh.lds, s, sh.wq);
    });
  }
  return hipGetLastError();
}

hipError_t launch_merge(const llampc_plan_out* parts, int32_t G, int32_t nan_first,
                        llampc_plan_out* merged, hipStream_t s) {
  if (G < 1 || G > 32) return hipErrorInvalidValue;   // LDS: 95 KB at G = 32
  const size_t M = (size_t)G * LLAMPC_KMAX;      // K <= KMAX (read on device)
  const size_t lds = (size_t)G * sizeof(llampc_plan_out) + 2 * M * sizeof(EntS);
  allow_lds(merge_kernel);
  hipLaunchKernelGGL(merge_kernel, dim3(1), dim3(kBlock), lds, s, parts, G, nan_first, merged);
  return hipGetLastError();
}

hipError_t launch_peer_exchange(const PeerLaunch& a, hipStream_t s) {
  if (a.G < 1 || a.G > kPeerMax || a.rank < 0 || a.rank >= a.G || a.seq == 0) return hipErrorInvalidValue;
  const size_t lds = (size_t)a.G * sizeof(llampc_plan_out) + 2 * (size_t)a.G * LLAMPC_KMAX * sizeof(EntS) +
                     (kBlock / 64) * sizeof(int);
  allow_lds(peer_exchange_kernel);
  hipLaunchKernelGGL(peer_exchange_kernel, dim3(1), dim3(kBlock), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_track_corridor(const TrackK& t, const CorridorPath& path, int32_t H, double hw, double* hp,
                                 double* theta, hipStream_t s) {
  if (H < 1 || H > LLAMPC_HMAX || t.n < 2 || t.n > kTrackMaxPoints || !t.cx || !t.cy || !t.tt || !hp)
    return hipErrorInvalidValue;
  allow_lds(track_corridor_kernel);      // 96 KB of tables at the largest centre line
  hipLaunchKernelGGL(track_corridor_kernel, dim3(H), dim3(kBlock), kCorridorScratch + 24 * (size_t)t.n, s, t, path, H,
                     hw, hp, theta);
  return hipGetLastError();
}

hipError_t launch_dynamics(int32_t op, const double* x, const double* u, const double* params,
                           int64_t P, VehK veh, int64_t n, double* out, hipStream_t s) {
  const int nb = (int)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(dynamics_kernel, dim3(nb), dim3(kBlock), 0, s, op, x, u, params, P, veh, n, out);
  return hipGetLastError();
}

hipError_t launch_math(int32_t fn, const double* a, const double* b, int64_t n, double* out,
                       hipStream_t s) {
  const int nb = (int)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(math_kernel, dim3(nb), dim3(kBlock), 0, s, fn, a, b, n, out);
  return hipGetLastError();
}

hipError_t launch_integrate(const double* x0, const double* u, int64_t us, const double* h,
                            int32_t S, const double* params, int64_t P, VehK veh, int64_t n,
                            int32_t integrator, double* traj, int32_t final_only, hipStream_t s) {
  const int nb = (int)((n + kBlock - 1) / kBlock);
  switch (integrator) {
    case LLAMPC_RK4:
      hipLaunchKernelGGL(integrate_kernel<0>, dim3(nb), dim3(kBlock), 0, s, x0, u, us, h, S, params, P, veh, n, traj, final_only);
      break;
    case LLAMPC_EULER_NLP:
      hipLaunchKernelGGL(integrate_kernel<1>, dim3(nb), dim3(kBlock), 0, s, x0, u, us, h, S, params, P, veh, n, traj, final_only);
      break;
    case LLAMPC_RK6:
      hipLaunchKernelGGL(integrate_kernel<2>, dim3(nb), dim3(kBlock), 0, s, x0, u, us, h, S, params, P, veh, n, traj, final_only);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace llampc

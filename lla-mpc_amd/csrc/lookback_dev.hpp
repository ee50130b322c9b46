// lookback_dev.hpp — the look-back block: one RK4 step of every model of the bank, the error
// against x_t, the ring write and the window mean in NumPy's pairwise order, then the waves'
// argmins and the block's sorted top-K list.  Included by final_dev.hpp (which merges the
// lists), plan_dev.hpp and ctl.hip.
#pragma once
#include "dev_stamps.hpp"
#include "dev_wave.hpp"
#include "rollout_dev.hpp"

namespace llampc {

namespace {

// np.mean(window, axis=1) for one model (rt.py:358): NumPy's pairwise order (8 partial sums)
// over the ring read oldest -> newest, then / W; W <= LLAMPC_WMAX (one pairwise block).
// Split around the newest value (the ring slot this tick writes): every older
// value is loaded and summed BEFORE the look-back's RK4 step — the loads' latency under the
// step instead of after it — in that exact order, so finishing with the newest error
// (win_finish) gives the mean's bits in that order.  Oldest -> newest is i = 0 .. W-1, the newest i = W-1:
//   W < 8 or W % 8 != 0: the newest is the sequential tail's last add:  s = pre + e
//   W % 8 == 0 (W >= 8):  it is r[7]'s last term (W = 8: r[7] itself), so
//                          s = A + (B + (r6 + r7)),  A = (r0 + r1) + (r2 + r3),  B = r4 + r5
struct WinPre {
  double a, b, c, d;                    // pre | A, B, r6, r7 without the newest
};
__device__ __forceinline__ WinPre win_pre(const double* ring, int64_t ld, int64_t n, int o, int W) {
  auto at = [&](int i) {
    int s = o + i;
    if (s >= W) s -= W;
    return ring[(int64_t)s * ld + n];
  };
  WinPre p{0.0, 0.0, 0.0, 0.0};
  if (W < 8) {
    for (int i = 0; i < W - 1; ++i) p.a += at(i);
    return p;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = j < W - 1 ? at(j) : 0.0;
  int i = 8;
  const int full = W - (W % 8);
  for (; i < full; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i + j < W - 1) r[j] += at(i + j);
  }
  if (W % 8 == 0) {
    p.a = (r[0] + r[1]) + (r[2] + r[3]);
    p.b = r[4] + r[5];
    p.c = r[6];
    p.d = r[7];                         // W = 8: unused (r[7] is the newest itself)
    return p;
  }
  double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < W - 1; ++i) s += at(i);
  p.a = s;
  return p;
}
__device__ __forceinline__ double win_finish(const WinPre& p, double e, int W) {
  double s;
  if (W >= 8 && W % 8 == 0) {
    const double r7 = W == 8 ? e : p.d + e;
    s = p.a + (p.b + (p.c + r7));
  } else {
    s = p.a + e;
  }
  return s / W;
}

}  // namespace

__device__ __forceinline__ double sq_err4(const double* x, const double* xn) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double e = x[j] - xn[j];
    s += e * e;
  }
  return s;
}

// Order-preserving u64 of a window mean for the argsort order (rt.py:360): -0 -> +0 and
// every NaN -> one canonical NaN above +inf.
__device__ __forceinline__ uint64_t order_key(double w) {
  const double wc = (w != w) ? __builtin_nan("") : w + 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(wc);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// A top-K entry in LDS (BEnt, launch_shape.hpp): ids from kNoModelId up mark lanes without a model.
constexpr uint32_t kNoModelId = 0xFFFFFE00u;
// (key, id, pos) order: total, so every rank below is unique.
__device__ __forceinline__ bool bless(const BEnt& a, const BEnt& b) {
  return (int)(a.key < b.key) |
         ((int)(a.key == b.key) & ((int)(a.id < b.id) | ((int)(a.id == b.id) & (int)(a.pos < b.pos))));
}

// The block's sorted top-K from its waves' lists (kWaves x K entries staged in LDS by
// wave_topk_rank or the R > 1 rounds): the first kWaves*K threads rank their entry among
// them and the ones ranked below K store it in the block's list tk_val/tk_idx[blk][K] —
// one list per block for lb_final (its merge cost grows with the lists' count).
__device__ __forceinline__ void block_topk_merge(const LookbackLaunch& a, int blk, const BEnt* e) {
  const int M = kWaves * a.K;
  const int t = threadIdx.x;
  if (t < M) {
    const BEnt me = e[t];
    int rank = 0;
    for (int j = 0; j < M; ++j) rank += (int)bless(e[j], me);
    if (rank < a.K) {
      st_wt(&a.tk_val[(int64_t)blk * a.K + rank], me.v);
      st_wt(&a.tk_idx[(int64_t)blk * a.K + rank], me.id >= kNoModelId ? kNoIndex : a.goff + (int64_t)me.id);
    }
  }
}

// The sorted top-K of one wave's 64 window means (R == 1) by rank: every lane counts the
// lanes whose (value, index) key precedes its own — NaN last, ties to the lower index
// (rt.py:360 argsort order) — and the lanes ranked below K store their entry at that rank.
// Keys as order-preserving u64 (+0 for -0, one canonical NaN above +inf); lanes without a
// model take a key above every model's (kNoIndex entries at the end of a short list).
// The wave's list goes to out[rank] (LDS, block_topk_merge).
__device__ __forceinline__ void wave_topk_rank(const LookbackLaunch& a, double w, int64_t n,
                                               unsigned char* lds, BEnt* out) {
  const int lane = threadIdx.x & 63;
  uint64_t* keys = reinterpret_cast<uint64_t*>(lds + (threadIdx.x >> 6) * kRankBytes);
  uint32_t* ids = reinterpret_cast<uint32_t*>(keys + 64);
  const bool valid = n < a.n;
  const uint64_t key = valid ? order_key(w) : ~0ull;
  const uint32_t id = valid ? (uint32_t)n : kNoModelId + (uint32_t)threadIdx.x;
  keys[lane] = key;
  ids[lane] = id;
  __syncthreads();
  int rank = 0;
#pragma unroll 16
  for (int j = 0; j < 64; ++j) {
    const uint64_t kj = keys[j];
    const uint32_t ij = ids[j];
    rank += (int)(kj < key) | ((int)(kj == key) & (int)(ij < id));
  }
  if (rank < a.K) out[rank] = BEnt{key, id, 0u, valid ? w : __builtin_nan("")};
}

// ------------------------------------------------------------------------------------
// Look-back body: one block = 256*R models (R models per lane, coalesced in r).
// RK4 step from (x_{t-1}, u_{t-1}), 4-state MSE against x_t, in-place ring write, window
// mean in NumPy's pairwise order; then the block's argmin and its SORTED top-K list.
// ------------------------------------------------------------------------------------
// ARMED (the controller, ctl.hip): x_t comes from door(pred, valid, n) — the LDS copy of x_t,
// or null when the launch is cancelled (lookback_block then returns false) — and with one
// model per lane the RK4 step runs BEFORE it: the step needs only the state's (x_{t-1},
// u_{t-1}), x_t enters with the error, so an armed launch has the step done when its doorbell
// rings.  door() also gets the lane's model n (valid: n < N) and its window mean without x_t
// (pred: the W - 1 entries that stay, over W; the speculative look-ahead's ranking).
template <bool ARMED = false, typename Door = int>
__device__ __forceinline__ bool lookback_block(const LookbackLaunch& a, int blk, const Scratch& sc, Door door = 0) {
  LB_STAMP(blk, 0);
  const int64_t base = (int64_t)blk * kBlock * a.R;
  const fm::FmK K = fm::FmK::load();
  bool ubad = false;
  const Input uf = make_input_fast(a.u_prev[0], a.u_prev[1], K, ubad);
  double wm0 = 0.0;                     // R == 1 keeps the window mean in a register
  const double* x_now = a.x_now;
  double xp[4] = {0.0, 0.0, 0.0, 0.0};  // ARMED, R == 1: the step before the doorbell
  Tire tp{};
  WinPre wpp{0.0, 0.0, 0.0, 0.0};
  bool bp = false, pre = false;
  if constexpr (ARMED) {
    double pred = 0.0;
    bool pvalid = false;
    int64_t pn = 0;
    if (a.R == 1) {                     // launch-uniform
      const int64_t n = base + threadIdx.x;
      if (n < a.n) {
        pvalid = true;
        pn = n;
        double x[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) x[j] = a.x_prev[j];
        tp = load_tire(a.params, a.n, n);
        const int o = (a.slot + 1 == a.W) ? 0 : a.slot + 1;
        if (a.full) wpp = win_pre(a.ring, a.n, n, o, a.W);
        const StageK sk = make_stage<1>(a.veh, tp, 0);
        Dom dm;
        dm.init();
        step_fast<0, 1>(a.veh, tp, sk, x, uf, a.Ts, K, dm);
#pragma unroll
        for (int j = 0; j < 4; ++j) xp[j] = x[j];
        bp = (int)ubad | (int)!sk.sok | (int)!dm.ok();
        if (a.full) pred = win_finish(wpp, 0.0, a.W);
      }
      pre = true;
    }
    x_now = door(pred, pvalid, pn);
    if (!x_now) return false;
  }
  for (int r = 0; r < a.R; ++r) {
    const int64_t n = base + (int64_t)r * kBlock + threadIdx.x;
    if (n >= a.n) break;
    double x[6];
    Tire t;
    WinPre wp{0.0, 0.0, 0.0, 0.0};
    bool bad;
    if (ARMED && pre) {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = xp[j];
      t = tp;
      wp = wpp;
      bad = bp;
    } else {
#pragma unroll
      for (int j = 0; j < 6; ++j) x[j] = a.x_prev[j];
      t = load_tire(a.params, a.n, n);
      const int o = (a.slot + 1 == a.W) ? 0 : a.slot + 1;     // the window's oldest slot
      if (a.full) wp = win_pre(a.ring, a.n, n, o, a.W);      // launch-uniform; under the step
      // model.py:32-40, one RK4 step: the fast stage; a lane whose operands leave the fast
      // cores' domains redoes the step with the general functions (as the look-ahead does)
      const StageK sk = make_stage<1>(a.veh, t, 0);
      Dom dm;
      dm.init();
      step_fast<0, 1>(a.veh, t, sk, x, uf, a.Ts, K, dm);
      bad = (int)ubad | (int)!sk.sok | (int)!dm.ok();
    }
    double s = sq_err4(x, x_now);                         // rt.py:349 mean over 4 states
    // the domain once per step; a NaN operand reaches x[0..3] (the stage-4 chains feed x[3])
    bad = (int)bad | (int)!(s <= __DBL_MAX__);
    if (__builtin_expect(__any(bad), 0)) {
      if (bad) {
#pragma unroll
        for (int j = 0; j < 6; ++j) x[j] = a.x_prev[j];
        rk4_step(a.veh, t, x, make_input(a.u_prev[0], a.u_prev[1]), a.Ts);
        s = sq_err4(x, x_now);
      }
    }
    const double err = s / 4;
    if (a.err_out) a.err_out[n] = err;
    a.ring[(int64_t)a.slot * a.n + n] = err;             // rt.py:352-353 without np.roll
    if (a.full) {
      const double wm = win_finish(wp, err, a.W);          // rt.py:358
      if (a.R > 1 || a.wm_keep) a.wm_buf[n] = wm;         // launch-uniform
      if (r == 0) wm0 = wm;
    }
  }
  LB_STAMP(blk, 1);
  if (!a.full) return true;  // launch-uniform

  // per WAVE (a list): the argmin (rt.py:359 semantics) and the sorted top-K (rt.py:360
  // argsort order) of its 64*R models with branch-free wave picks — no LDS round trip, no
  // barrier (a block-wide (value, index) min per round cost ~4k cycles); lb_final merges
  // the kWaves lists of every block.  Local index n < 2^32 (bank size check in the C-ABI).
  const int lane = threadIdx.x & 63;
  const int64_t list = (int64_t)blk * kWaves + (threadIdx.x >> 6);
  double v = a.nan_first ? __builtin_inf() : __builtin_nan("");
  uint32_t li = kNoLocal;
  for (int r = 0; r < a.R; ++r) {
    const int64_t n = base + (int64_t)r * kBlock + threadIdx.x;
    if (n >= a.n) break;
    const double w = (a.R == 1) ? wm0 : a.wm_buf[n];
    const bool t = a.nan_first ? less_bf<1>(w, (uint32_t)n, v, li) : less_bf<0>(w, (uint32_t)n, v, li);
    v = t ? w : v;
    li = t ? (uint32_t)n : li;
  }
  if (a.nan_first) wave_pick_nf(v, li);
  else wave_pick_nl(v, li);
  if (lane == 0) {
    st_wt(&a.am_val[list], v);
    st_wt(&a.am_idx[list], li == kNoLocal ? kNoIndex : a.goff + li);
  }
  LB_STAMP(blk, 2);
  unsigned char* rank_lds = reinterpret_cast<unsigned char*>(sc.sv) + kScratchBytes;
  BEnt* wl = reinterpret_cast<BEnt*>(rank_lds + kWaves * kRankBytes);   // [kWaves][K]
  BEnt* mine = wl + (threadIdx.x >> 6) * a.K;
  if (a.R == 1) {                       // launch-uniform
    wave_topk_rank(a, wm0, base + threadIdx.x, rank_lds, mine);
    __syncthreads();
    block_topk_merge(a, blk, wl);
    LB_STAMP(blk, 3);
    return true;
  }
  // R > 1: K rounds of "next key after the previous pick" (NaN last, ties -> lower index)
  double lv = 0.0;
  uint32_t ll = kNoLocal;
  for (int k = 0; k < a.K; ++k) {
    double cv = __builtin_nan("");
    uint32_t cl = kNoLocal;
    for (int r = 0; r < a.R; ++r) {
      const int64_t n = base + (int64_t)r * kBlock + threadIdx.x;
      if (n >= a.n) break;
      const double w = (a.R == 1) ? wm0 : a.wm_buf[n];
      const uint32_t ln = (uint32_t)n;
      const bool t = (int)(k == 0 || less_bf<0>(lv, ll, w, ln)) & (int)less_bf<0>(w, ln, cv, cl);
      cv = t ? w : cv;
      cl = t ? ln : cl;
    }
    wave_pick_nl(cv, cl);
    if (lane == 0) {
      const bool none = cl == kNoLocal;
      mine[k] = BEnt{none ? ~0ull : order_key(cv), none ? kNoModelId + (uint32_t)((threadIdx.x >> 6) * a.K + k) : cl,
                     0u, none ? __builtin_nan("") : cv};
    }
    lv = cv;
    ll = cl;
  }
  __syncthreads();
  block_topk_merge(a, blk, wl);
  LB_STAMP(blk, 3);
  return true;
}

}  // namespace llampc

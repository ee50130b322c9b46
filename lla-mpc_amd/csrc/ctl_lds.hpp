// ctl_lds.hpp — the controller launch's dynamic-LDS layouts, for the device and for the host's
// size computation (ctl_lds_bytes): a look-ahead block's (CtlLds; cs_kernel's with C = 0),
// a spec block's (SpecLds) and the size of the completing block's area, whose record words are
// checked against the C structs here.  No device code: included by the ctl_*_dev.hpp headers,
// ctl.hip and capi_host.hpp (ctl_shape).
#pragma once
#include <algorithm>
#include <cstddef>

#include "ctl.hpp"
#include "launch_shape.hpp"

namespace llampc {

// LDS layout of the controller launch (byte offsets; 16-B aligned regions).  Look-ahead
// blocks: xref [H+1][2] | U [C][H][2] | knots [n + pad] | the two speed profiles bracketing mu
// interleaved per segment [n-1][2][4] (a, b, c, d of lo, then of hi: one segment's values are
// four 16-B reads) | with s4: sin / cos delta [C][H][2], then per candidate the summed
// input-rate cost and its feasibility flag [C][2] (staged during the walk) | misc.
// The completing block: lb_final's region from kScratchBytes (then the candidates [C][H][2]),
// its own area at poll_off (CtlPollLds).
struct CtlLds {
  size_t sx, ul, kn, spd, s4, misc, end;
};
__host__ __device__ __forceinline__ size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
__host__ __device__ __forceinline__ CtlLds ctl_lds(int H, int C, int n, bool s4 = false) {
  CtlLds L;
  size_t o = kScratchBytes;
  L.sx = o;
  o = align16(o + 16 * (size_t)(H + 1));
  L.ul = o;
  o = align16(o + 16 * (size_t)C * H);
  L.kn = o;
  o = align16(o + 8 * (size_t)(n + kKnotPad));
  L.spd = o;
  o = align16(o + 64 * (size_t)(n - 1));
  L.s4 = o;
  if (s4) o = align16(o + 16 * (size_t)C * H + 16 * (size_t)C);
  L.misc = o;
  L.end = o + 1024;
  return L;
}
// A spec block (ctl_spec): xref [H+1][2] (from the walker) | U [C][H][2] | the staged terms
// (s4) | the deferred positions [C][2][H] (X, Y of each candidate per step) | the quads' unused
// lanes' sink | misc (x_t, the doorbell's verdict, the model).
struct SpecLds {
  size_t sx, ul, s4, pos, junk, misc, end;
};
__host__ __device__ __forceinline__ SpecLds spec_lds(int H, int C) {
  SpecLds L;
  size_t o = kScratchBytes;
  L.sx = o;
  o = align16(o + 16 * (size_t)(H + 1));
  L.ul = o;
  o = align16(o + 16 * (size_t)C * H);
  L.s4 = o;
  o = align16(o + 16 * (size_t)C * H + 16 * (size_t)C);
  L.pos = o;
  o = align16(o + 16 * (size_t)C * H);
  L.junk = o;
  o += 8 * 64;
  L.misc = o;
  L.end = o + 256;
  return L;
}
constexpr size_t kCtlPollBytes = 4096;   // ctl_complete's area (layout there)

// LDS bytes of the controller launch and the completing block's area offset; s4: with the staged
// input terms (CtlLaunch.s4).
// extra: bytes a look-ahead block keeps after its layout, from L.end on (a corridor tick's half-planes
// and winner positions, ctl.hpp ctl_corr_extra); role_min: another block role's whole request (the
// corridor blocks' track tables).
inline size_t ctl_lds_bytes(int H, int C, int n, int nb_lb, int K, size_t* poll_off, bool s4 = false, int px_G = 0,
                            int n_spec = 0, size_t extra = 0, size_t role_min = 0) {
  CtlLds L = ctl_lds(H, C, n, s4);
  L.end = std::max(align16(L.end + extra), role_min);
  const size_t Lb = nb_lb;
  const size_t lbf = lb_final_lds_bytes(nb_lb, K);                      // lb_final's region, the wave lists
  const size_t px = px_G ? kScratchBytes + ctl_px_bytes(px_G, K) : 0;   // ctl_exchange's region
  // the speculative look-ahead: a spec block's layout, the look-back blocks' ranking and the
  // spec merge's two list buffers
  // (sharded: then the ranks' lists, ctl_spec_exchange)
  const size_t spec_px = px_G ? align16(2 * sizeof(Ent) * Lb * n_spec) + align16(16 * (size_t)px_G * n_spec) +
                                    2 * sizeof(Ent) * (size_t)px_G * n_spec
                              : 0;
  const size_t spec = n_spec ? std::max(spec_lds(H, C).end,
                                        kScratchBytes + std::max<size_t>(std::max<size_t>(12 * kBlock, 2 * sizeof(Ent) * Lb * n_spec),
                                                                         spec_px))
                             : 0;
  size_t off = std::max(std::max(std::max(L.end, px), lbf), spec);
  off = align16(off);
  *poll_off = off;
  return off + kCtlPollBytes;
}
// ctl_complete's record words (one 8-byte word per lane of wave 0)
static_assert(offsetof(llampc_plan_out, window_full) == 4 && offsetof(llampc_plan_out, K) == 8 &&
                  offsetof(llampc_plan_out, sel_owned) == 12 && offsetof(llampc_plan_out, lb_best) == 16 &&
                  offsetof(llampc_plan_out, lb_best_val) == 24 && offsetof(llampc_plan_out, sel_model) == 32 &&
                  offsetof(llampc_plan_out, sel_cand) == 40 && offsetof(llampc_plan_out, n_nonfinite) == 44 &&
                  offsetof(llampc_plan_out, sel_cost) == 48 && offsetof(llampc_plan_out, la_best_model) == 56 &&
                  offsetof(llampc_plan_out, la_best_cand) == 64 && offsetof(llampc_plan_out, status) == 68 &&
                  offsetof(llampc_plan_out, la_best_cost) == 72 && offsetof(llampc_plan_out, topk) == 80,
              "llampc_plan_out header words");
static_assert(offsetof(llampc_ctl_out, tick) == sizeof(llampc_plan_out) &&
                  offsetof(llampc_ctl_out, projidx) == offsetof(llampc_ctl_out, tick) + 8 &&
                  offsetof(llampc_ctl_out, warm) == offsetof(llampc_ctl_out, tick) + 12 &&
                  offsetof(llampc_ctl_out, mu_used) == offsetof(llampc_ctl_out, tick) + 16 &&
                  offsetof(llampc_ctl_out, scale_used) == offsetof(llampc_ctl_out, tick) + 24 &&
                  offsetof(llampc_ctl_out, mu_pred) == offsetof(llampc_ctl_out, tick) + 32 &&
                  offsetof(llampc_ctl_out, dr_mean) == offsetof(llampc_ctl_out, tick) + 40 &&
                  offsetof(llampc_ctl_out, df_mean) == offsetof(llampc_ctl_out, tick) + 48,
              "llampc_ctl_out words");

}  // namespace llampc

"""The nine corridor cases the device builder (csrc/corridor_dev.hpp) is held to, shared by
tests/test_nlp_track_corridor_cpu.py (the header's functions on the host) and
tests/test_nlp_track_corridor_gpu.py (the kernel): the smallest shapes at which it can go wrong.

  ethz-H1 / H20 / H40 / H64   ETHZ('optimal', True), the tick-20 ConstantSpeed reference of the
                              test_setupnlp_* tests, margin 0.03; H = 64 is LLAMPC_HMAX.
  ethz-wrap                   ETHZ across the lap wrap: P_k = param_to_xy((L - 0.30 + 0.03 k) mod L)
                              + (0.02, 0.02), k = 0..20, margin 0 — the closing segment and the fmod.
  mobil-vertices              ETHZMobil, the 21 consecutive centre points from index n // 2, margin
                              0.05: every point a vertex (t = 0 and t = len, ties between
                              neighbours).  No run through vertex 0: param_to_xy is discontinuous
                              there (the closing-gap extrapolation; corridor_dev.hpp).
  polygon-5 / 64 / 257        regular polygons, R = 1, width 0.4, as bare Track objects: fewer
                              segments than lanes, a quarter block, one past a block's stride;
                              H = 20, margin 0.02, the path a_k = 2 pi (0.013 + 0.0497 k),
                              r_k = 1 + 0.15 cos 7 a_k, P_k = r_k (cos a_k, sin a_k).

The reference is constraints.track_corridor and Track.xy_to_param, computed once per case.

TOL = 1e-12 absolute on every hp entry and on theta: coordinates and arc lengths are <= 18 in
magnitude (one rounding ~2e-15), a record takes a few dozen operations and one division by a
segment length >= 0.01 multiplied back by it — about 1e-13 in the worst case, FMA contraction
included.  A larger difference means another segment or branch."""
import functools

import numpy as np

from conftest import golden

TOL = 1e-12
TS = 0.02
CASES = ["ethz-H1", "ethz-H20", "ethz-H40", "ethz-H64", "ethz-wrap", "mobil-vertices",
         "polygon-5", "polygon-64", "polygon-257"]


@functools.lru_cache(maxsize=None)
def track(name):
    from llampc.tracks import ETHZ, ETHZMobil, Track
    if name == "ETHZ":
        return ETHZ('optimal', True)
    if name == "ETHZMobil":
        return ETHZMobil('optimal', True)
    n = int(name.split("-")[1])
    a = 2 * np.pi * np.arange(n) / n
    tr = Track()
    tr.x_center, tr.y_center, tr.track_width = np.cos(a), np.sin(a), 0.4
    tr._init_geometry()
    return tr


@functools.lru_cache(maxsize=None)
def tick_inputs(tick, H):
    """(x0, uprev, xref) of DYN-slice tick `tick` as the test_setupnlp_* tests build them."""
    from llampc.mpc.planner import ConstantSpeed
    d = golden("dyn_slice.npz")
    s, u = d["states"], d["inputs"]
    x0, up = s[:, tick].copy(), u[:, tick - 1].copy()
    xref, _, _ = ConstantSpeed(x0[:2], x0[3], track("ETHZ"), H, TS, 0)
    xref = np.ascontiguousarray(xref, dtype=np.float64)
    for a in (x0, up, xref):
        a.setflags(write=False)
    return x0, up, xref


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(track, track_name, path [2, H+1], H, margin, hp [H, 6], theta [H]), read-only."""
    from llampc.mpc import constraints
    if name.startswith("ethz-H"):
        tname, H, margin = "ETHZ", int(name[6:]), 0.03
        path = tick_inputs(20, H)[2][:2]
    elif name == "ethz-wrap":
        tname, H, margin = "ETHZ", 20, 0.0
        tr = track(tname)
        L = float(tr.track_length)
        path = np.array([tr.param_to_xy((L - 0.30 + 0.03 * k) % L) for k in range(H + 1)]).T + 0.02
    elif name == "mobil-vertices":
        tname, H, margin = "ETHZMobil", 20, 0.05
        tr = track(tname)
        n = tr.center_line.shape[1]
        path = tr.center_line[:, n // 2:n // 2 + H + 1]
    else:
        tname, H, margin = name, 20, 0.02
        a = 2 * np.pi * (0.013 + 0.0497 * np.arange(H + 1))
        r = 1 + 0.15 * np.cos(7 * a)
        path = np.stack([r * np.cos(a), r * np.sin(a)])
    tr = track(tname)
    path = np.ascontiguousarray(path, dtype=np.float64)
    assert path.shape == (2, H + 1)
    hp = constraints.track_corridor(tr, path, margin)
    theta = np.array([float(tr.xy_to_param(path[0, k], path[1, k])) for k in range(1, H + 1)])
    out = dict(track=tr, track_name=tname, path=path, H=H, margin=margin, hp=hp, theta=theta)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out

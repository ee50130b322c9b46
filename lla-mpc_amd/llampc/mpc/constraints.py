"""Corridors for ``setupNLP.solve(..., corridor=hp)``: per-step position half-planes.

A corridor is ``hp`` [H, 6] float64.  Row k - 1 (k = 1..H, the state after k Euler steps) is
(a0, a1, b, c0, c1, d): the two half-planes a.p_k <= b and c.p_k <= d on the position
p_k = (X, Y); a = (0, 0), b = +inf disables one.  The device search penalises the squared
slacks max(a.p_k - b, 0)^2 + max(c.p_k - d, 0)^2 (csrc/rollout_dev.hpp corridor_slack2).

``track_corridor`` builds the corridor of a packaged track around a reference, ``strip`` one
around any polyline; ``slacks`` evaluates a trajectory on a corridor in the device's order.
``setupNLP(device_corridor=True)`` builds ``track_corridor``'s half-planes on the device instead
(csrc/corridor_dev.hpp restates the function in scalar form, equal to it to 1e-12) along
``default_path`` or the caller's own path.

The reference's constraints.py (``Boundary()``: the boundary lines linearised per step, with
slack variables in the NLP) is not restated here; this is the same geometry — two parallel
half-planes per step, one per track side — as a soft constraint of the sampling search.
"""
from __future__ import annotations

import numpy as np

# track_corridor's tangent: the centre line at theta -/+ TANGENT_EPS metres of arc length.  The
# packaged centre lines are polylines of 1-3.5 cm segments whose param_to_xy extrapolates the
# last segment over the 3 cm closing gap (up to 2 mm off the first point): 5 cm spans a few
# segments, so a corner of the polyline and that mismatch turn the tangent by a few degrees at
# most, and stays far below the tracks' smallest radius.
TANGENT_EPS = 0.05


def require_track(track, what):
    """The track attributes a device-built corridor reads (``setupNLP(device_corridor=True)``,
    ``LLAMPC(corridor_weight=...)``): raises ValueError naming the missing ones."""
    missing = [k for k in ("center_line", "theta_track", "track_length", "track_width")
               if getattr(track, k, None) is None]
    if track is None or missing:
        raise ValueError(f"{what} needs a track with center_line, theta_track, track_length "
                         f"and track_width (missing: {'the track' if track is None else ', '.join(missing)})")


def require_margin(track, margin):
    """A margin that leaves a corridor on the track (a NaN margin does not)."""
    if not float(margin) < float(track.track_width) / 2:
        raise ValueError(f"corridor_margin {margin} leaves no corridor "
                         f"(track width {track.track_width})")


def track_tables(track):
    """(centre [2, n], theta [n], track_length, track_width) as llampc_nlp_set_track and
    llampc_ctl_set_track take them."""
    centre = np.ascontiguousarray(track.center_line, dtype=np.float64)
    theta = np.ascontiguousarray(track.theta_track, dtype=np.float64)
    if centre.ndim != 2 or centre.shape[0] != 2 or theta.shape != (centre.shape[1],):
        raise ValueError(f"track: center_line {centre.shape} and theta_track {theta.shape} must be "
                         "[2, n] and [n]")
    return centre, theta, float(track.track_length), float(track.track_width)


def _left_normal(t):
    t = np.asarray(t, dtype=np.float64)
    n = np.array([-t[1], t[0]])
    return n / np.hypot(n[0], n[1])


def _record(n, centre, half):
    """(n, n.c + half, -n, -(n.c - half)): |n.p - n.c| <= half as two half-planes."""
    return np.array([n[0], n[1], centre + half, -n[0], -n[1], -(centre - half)])


def track_corridor(track, xref, margin=0.0):
    """The track's corridor along a reference: -> hp [H, 6] for ``xref`` [2, H+1] (or more rows;
    the first two are X, Y).  For k = 1..H: theta = track.xy_to_param(xref[:, k]), the centre
    c = track.param_to_xy(theta), the unit tangent from param_to_xy(theta -/+ TANGENT_EPS)
    (modulo track_length), n its left normal and hw = track.track_width / 2 - margin; the record is
    (n, n.c + hw, -n, -(n.c - hw)): the position stays within hw of the centre line, across it."""
    xref = np.asarray(xref, dtype=np.float64)
    H = xref.shape[1] - 1
    hw = float(track.track_width) / 2 - float(margin)
    if not hw > 0:
        raise ValueError(f"margin {margin} leaves no corridor (track width {track.track_width})")
    L = float(track.track_length)
    hp = np.empty((H, 6))
    for k in range(1, H + 1):
        theta = float(track.xy_to_param(xref[0, k], xref[1, k]))
        c = np.array(track.param_to_xy(theta), dtype=np.float64)
        fwd = np.array(track.param_to_xy((theta + TANGENT_EPS) % L), dtype=np.float64)
        back = np.array(track.param_to_xy((theta - TANGENT_EPS) % L), dtype=np.float64)
        n = _left_normal(fwd - back)
        hp[k - 1] = _record(n, float(n @ c), hw)
    return hp


def default_path(x0, H, Ts, prev_xmpc=None):
    """The path [2, H+1] a ``setupNLP(device_corridor=True)`` solve builds its corridor along when
    the caller gives none.  With the previous solve's ``prev_xmpc`` ([6, H+1], or its first two
    rows): its positions shifted one step, the last one repeated — the warm start's rule, so the
    corridor follows where the search starts.  Without (the first solve): the ray from the car,
    P_k = (X0, Y0) + k Ts max(vx0, 0.05) (cos psi0, sin psi0), 0.05 the NLP's own vmin.  (Not
    ``xref``: ConstantSpeed runs far ahead of the car on the recorded states, and the corridor
    along it leaves the unconstrained optimum 0.2-0.9 m outside the walls.)  At a long horizon
    with a spinning car the ray leaves the track: a caller who knows better passes
    ``corridor_path``."""
    H = int(H)
    out = np.empty((2, H + 1))
    if prev_xmpc is not None:
        P = np.asarray(prev_xmpc, dtype=np.float64)
        if P.ndim != 2 or P.shape[0] < 2 or P.shape[1] != H + 1:
            raise ValueError(f"prev_xmpc must be [6, H+1] = {(6, H + 1)}, got {P.shape}")
        out[:, :-1] = P[:2, 1:]
        out[:, -1] = P[:2, -1]
        return out
    x0 = np.asarray(x0, dtype=np.float64).ravel()
    step = np.arange(H + 1) * (float(Ts) * max(float(x0[3]), 0.05))
    out[0] = x0[0] + step * np.cos(x0[2])
    out[1] = x0[1] + step * np.sin(x0[2])
    return out


def strip(path, half, offset=0.0):
    """A corridor around a polyline: -> hp [H, 6] for ``path`` [H+1, 2] (P_0 .. P_H; [2, H+1] is
    taken too when H != 1).  For k = 1..H the normal n is the left normal of
    P[min(k+1, H)] - P[k-1], the centre n.P[k] + offset_k and the half-width half_k (scalars or
    [H] arrays): the record (n, centre + half, -n, -(centre - half))."""
    P = np.asarray(path, dtype=np.float64)
    if P.ndim != 2 or 2 not in P.shape:
        raise ValueError(f"path must be [H+1, 2], got {P.shape}")
    if P.shape[1] != 2:
        P = P.T
    H = P.shape[0] - 1
    if H < 1:
        raise ValueError("path needs at least two points")
    half = np.broadcast_to(np.asarray(half, dtype=np.float64), (H,))
    offset = np.broadcast_to(np.asarray(offset, dtype=np.float64), (H,))
    hp = np.empty((H, 6))
    for k in range(1, H + 1):
        n = _left_normal(P[min(k + 1, H)] - P[k - 1])
        hp[k - 1] = _record(n, float(n @ P[k]) + offset[k - 1], half[k - 1])
    return hp


def disabled(H):
    """The corridor that constrains nothing: a = c = 0, b = d = +inf at every step."""
    hp = np.zeros((H, 6))
    hp[:, 2] = hp[:, 5] = np.inf
    return hp


def slacks(hp, xy):
    """The slacks [H, 2] = max(a.p_k - b, 0), max(c.p_k - d, 0) of the positions ``xy`` [2, H+1]
    (p_0 .. p_H; row k - 1 of hp meets p_k), each product and sum rounded on its own as the
    device forms them."""
    hp = np.asarray(hp, dtype=np.float64)
    xy = np.asarray(xy, dtype=np.float64)
    X, Y = xy[0, 1:hp.shape[0] + 1], xy[1, 1:hp.shape[0] + 1]
    g1 = (hp[:, 0] * X + hp[:, 1] * Y) - hp[:, 2]
    g2 = (hp[:, 3] * X + hp[:, 4] * Y) - hp[:, 5]
    return np.stack([np.where(g1 > 0, g1, 0.0), np.where(g2 > 0, g2, 0.0)], axis=1)

"""Shared inputs and NumPy restatements for the tests of the look-ahead tire chain's atan cores
(csrc/fastmath.hpp: octant_fix, atan_zones).  No GPU here: test_chain_zones_cpu.py checks these on
the oracle alone, test_chain_selects_gpu.py runs the same inputs on the device."""
import numpy as np

from conftest import golden
from oracle import llampc_oracle as O

TS = 0.02
TP8 = 0.41421356237309503                     # tan(pi/8), fastmath.hpp kTanPi8
CTP8 = 2.414213562373095                      # cot(pi/8) = 1 + sqrt(2), kCotPi8
PIO2, PIO4 = 1.5707963267948966, 0.7853981633974483
ZMAX = 2.0 ** 1000                            # kAtanClamp
# the precise 10-term atan polynomial on |t| <= tan(pi/8) (fastmath.hpp kAtanR, <= 1 ulp)
ATAN_R = [-0.3333333333333325, 0.19999999999898407, -0.1428571426609662, 0.11111109636534361,
          -0.09090852557176049, 0.0769105515839315, -0.06649613695291669, 0.05736332165907643,
          -0.04483334622272886, 0.02275052699336167]
TINY = 5e-324


def _with_neighbours(v):
    return [np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)]


def atan_edges(nonfinite=True):
    """0, +-tiny, +-2^1000, the zone edges tan(pi/8), 1 and 1 + sqrt(2) with their two nextafter
    neighbours, in both signs; +-inf and NaN last when asked for."""
    pos = [TINY, 2.0 ** 1000] + _with_neighbours(TP8) + _with_neighbours(1.0) + _with_neighbours(CTP8)
    z = [0.0, -0.0] + pos + [-v for v in pos]
    if nonfinite:
        z += [np.inf, -np.inf, np.nan]
    return np.array(z, dtype=np.float64)


def atan2_edges():
    """(y, x), x >= 0: every octant boundary of atan2_fast's reduction — y = 0, |y| = tan(pi/8) x
    (the pi/4 split of the ratio), |y| = x (the swap), x = tan(pi/8) |y| (the split of the swapped
    ratio), x = 0 — each with the nextafter neighbours of y, at x = 1, 3 and 2^-20, both signs of
    y; and +-tiny and +-2^999 against 1."""
    ys, xs = [], []
    for x in (1.0, 3.0, 2.0 ** -20):
        for r in (TP8, 1.0, CTP8):
            for y in _with_neighbours(r * x):
                ys += [y, -y]
                xs += [x, x]
        ys += [0.0, -0.0]
        xs += [x, x]
    for y in (TINY, 1.0, 2.0 ** 999):
        ys += [y, -y]
        xs += [1.0, 1.0]
    for y in (1.0, 2.0 ** 999):               # x = 0 (|y| + x >= 2^-1000: the domain)
        ys += [y, -y]
        xs += [0.0, 0.0]
    ys += [1.0, -1.0]
    xs += [2.0 ** 999, 2.0 ** 999]
    return np.array(ys, dtype=np.float64), np.array(xs, dtype=np.float64)


def ulp_err(got, want):
    """Largest |got - want| in ulps of want over the finite entries (0 ulp where both are +-0)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin]) / np.spacing(np.maximum(np.abs(want[fin]), 1e-300))))


def poly10(t):
    s = t * t
    p = np.full_like(s, ATAN_R[-1])
    for c in ATAN_R[-2::-1]:
        p = p * s + c
    return t + (t * s) * p


def atan_three_zone(z, core=np.arctan):
    """atan_zones in NumPy with a true division: a = min(|z|, 2^1000); z2 = |z| > tan(pi/8),
    z3 = !(|z| <= cot(pi/8)); num = q3 a - s2, den = s2 a + q3, t = num / den, result =
    copysign(c1 pi/4 + core(t), z).  core: atan on |t| <= tan(pi/8) — NumPy's own by default (the
    reduction and the reconstruction alone), or poly10 (the precise polynomial, without FMAs)."""
    z = np.asarray(z, dtype=np.float64)
    az = np.abs(z)
    with np.errstate(all="ignore"):
        a = np.fmin(az, ZMAX)                    # v_min: a NaN operand gives the other one
        z2, z3 = az > TP8, ~(az <= CTP8)
        s2 = np.where(z2, 1.0, 0.0)
        q3 = np.where(z3, 0.0, 1.0)
        c1 = np.where(z3, 2.0, s2)
        t = (q3 * a - s2) / (s2 * a + q3)
        return np.copysign(c1 * PIO4 + core(t), z)


def atan_two_way_parts(z):
    """(swap, r) of the two-way atan_fast in NumPy: r = atan(min(|z|, 1) / max(|z|, 1)) with the
    pi/8 split (atan_ratio_k, precise polynomial, true division), swap = |z| > 1."""
    az = np.abs(np.asarray(z, dtype=np.float64))
    with np.errstate(all="ignore"):
        n, d = np.fmin(az, 1.0), np.fmax(az, 1.0)
        sf = np.where(n > TP8 * d, 1.0, 0.0)
        t = (n - sf * d) / (sf * n + d)
        return az > 1.0, sf * PIO4 + poly10(t)


def fixup_select(swap, r, y):
    """The octant fix-up as it was: copysign(swap ? pi/2 - r : r, y)."""
    return np.copysign(np.where(swap, PIO2 - r, r), y)


def fixup_fma(swap, r, y):
    """octant_fix: w = swap ? 1.0 : 0.0, copysign(fma(w, pi/2, -r), y).  w pi/2 is exact for w in
    {0, 1}, so the FMA's single rounding is that of the sum below."""
    w = np.where(swap, 1.0, 0.0)
    return np.copysign(w * PIO2 + (-r), y)


# ---- the rollouts that reach every zone -------------------------------------------------------
NMAX = 65
# two decades of Bf and Br.  (Up to 80 the zones fill as well, but one model's rollout is then
# ill-conditioned in the oracle itself: a one-ulp change of x0 moves its cost by 4e-4; here the
# largest such change is 6e-13, conftest.cost_sensitivity.)
B_LO, B_HI = 0.4, 40.0


def shared():
    p = O.orca_params()
    return {k: p[k] for k in ("lf", "lr", "mass", "Iz", "Cm1", "Cm2", "Cr0", "Cr2")}


def zone_bank(n=NMAX):
    """generate_bank(NMAX, seed 8) with Bf log-spaced over [B_LO, B_HI] up the models and Br down
    them, so that |B slip| of the stage evaluations spreads over the three zones of atan_zones."""
    from llampc.mpc import generate_bank
    p = generate_bank(NMAX, seed=8)
    g = np.geomspace(B_LO, B_HI, NMAX)
    p[0], p[3] = g, g[::-1]
    return p[:, :n].copy()


def start():
    """The recorded state 30 and the input before it."""
    d = golden("dyn_slice.npz")
    return d["states"][:, 30].copy(), d["inputs"][:, 29].copy(), d["inputs"]


def candidates(C, H):
    """The recorded inputs from step 30; candidate 1 steers +0.04 at 0.05 less pwm, candidate 2
    steers -0.04."""
    _, _, u = start()
    U = np.repeat(u[:, 30:30 + H].T[None].copy(), C, axis=0)
    if C > 1:
        U[1, :, 1] += 0.04
        U[1, :, 0] -= 0.05
    if C > 2:
        U[2, :, 1] -= 0.04
    return np.clip(U, [-0.1, -0.35], [1.0, 0.35])


def straight_xref(x0, H):
    v, t = np.hypot(x0[3], x0[4]), np.arange(H + 1) * TS
    return np.vstack([x0[0] + v * np.cos(x0[2]) * t + 0.01, x0[1] + v * np.sin(x0[2]) * t - 0.02])


class _RecordingNumpy:
    """numpy whose arctan also appends |argument| to a list; every other attribute is numpy's."""

    def __init__(self, sink):
        self._sink = sink

    def __getattr__(self, k):
        return getattr(np, k)

    def arctan(self, z):
        self._sink.append(np.abs(np.asarray(z, dtype=np.float64)).ravel().copy())
        return np.arctan(z)


def oracle_rollout_recording_atan(p, x0, U):
    """(traj, |z| of every arctan the oracle's RK4 rollout evaluates): the stage evaluations of
    atan(B slip), front and rear, of every (model, candidate, step, stage)."""
    sink, real = [], O.np
    try:
        O.np = _RecordingNumpy(sink)
        with np.errstate(all="ignore"):
            traj = O.rollout_rk4(shared(), tuple(p), x0, U, TS)
    finally:
        O.np = real
    return traj, np.concatenate(sink)


def zone_fractions(az):
    az = az[np.isfinite(az)]
    return (float(np.mean(az <= TP8)), float(np.mean((az > TP8) & (az <= CTP8))), float(np.mean(az > CTP8)))

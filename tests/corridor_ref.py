"""The look-ahead corridor's reference (no GPU): J_c = O.mpc_cost(traj, ...) + w pen on the oracle's
own rollouts, pen = sum_k max(a_k.p_k - b_k, 0)^2 + max(c_k.p_k - d_k, 0)^2 in NumPy with every
product and sum separate and k ascending (the device's order, csrc/rollout_dev.hpp corridor_slack2 /
corridor_add); the test corridor of the parity matrix (a strip around the reference line whose half
width is the median of the pairs' largest lateral offsets); and the conditioning screen of J_c
(conftest.core_error_bound's construction applied to cost + penalty, and the one-ulp sensitivity).
Shared by test_lookahead_corridor_cpu.py and test_lookahead_corridor_gpu.py."""
import numpy as np

from conftest import CORE_MARGIN, _PerturbedNumpy, lean_core_errors
from oracle import llampc_oracle as O

ROLLOUTS = {"rk4": O.rollout_rk4, "euler_nlp": O.rollout_euler_nlp}


def penalty(hp, traj):
    """pen [L] of traj [H+1, L, 6] on hp [H, 6]: row k - 1 meets the position after k steps."""
    hp = np.asarray(hp, dtype=np.float64)
    H = hp.shape[0]
    assert hp.shape == (H, 6) and traj.shape[0] == H + 1, (hp.shape, traj.shape)
    pen = np.zeros(traj.shape[1])
    with np.errstate(invalid="ignore"):
        for k in range(1, H + 1):
            X, Y = traj[k, :, 0], traj[k, :, 1]
            a0, a1, b, c0, c1, d = hp[k - 1]
            p0 = a0 * X
            p1 = a1 * Y
            g1 = (p0 + p1) - b
            q0 = c0 * X
            q1 = c1 * Y
            g2 = (q0 + q1) - d
            s1 = np.where(g1 > 0, g1, 0.0)
            s2 = np.where(g2 > 0, g2, 0.0)
            t1 = s1 * s1
            t2 = s2 * s2
            pen = pen + (t1 + t2)
    return pen


def corridor_cost(traj, U, xref, uprev, Q, R, P, hp, w):
    """(J_c [L], pen [L]): J + w pen, the product rounded before the sum."""
    pen = penalty(hp, traj)
    wp = w * pen
    return O.mpc_cost(traj, U, xref, uprev, Q, R, P) + wp, pen


def lateral_offsets(traj, xref):
    """[L]: every rollout's largest distance from the reference line, across it — the slacks of
    the zero-width strip around xref."""
    from llampc.mpc import constraints
    hp0 = constraints.strip(np.asarray(xref).T, 0.0)
    off = np.zeros(traj.shape[1])
    for k in range(1, hp0.shape[0] + 1):
        a0, a1, b = hp0[k - 1, :3]
        off = np.maximum(off, np.abs((a0 * traj[k, :, 0] + a1 * traj[k, :, 1]) - b))
    return off


def median_strip(traj, xref, scale=1.0):
    """The matrix's corridor: constraints.strip around the reference line, half width = scale x the
    median over the pairs of lateral_offsets (about half of the pairs leave it)."""
    from llampc.mpc import constraints
    hw = scale * float(np.median(lateral_offsets(traj, xref)))
    assert hw > 0
    return constraints.strip(np.asarray(xref).T, hw)


def core_error_bound_corridor(shared, cols6, x0, U, xref, uprev, Q, R, P, hp, w, Ts=0.02, draws=4, seed=0, eps=None):
    """conftest.core_error_bound on J_c: CORE_MARGIN x the largest relative change of the oracle's
    RK4 cost + penalty when every transcendental result carries its lean core's worst relative
    error (eps: None = measured on the device, lean_core_errors) — all +, all -, `draws` random
    sign patterns."""
    eps = lean_core_errors() if eps is None else eps
    x0 = np.asarray(x0, dtype=np.float64)
    rng = np.random.RandomState(seed)
    real = O.np
    with np.errstate(all="ignore"):
        c0, _ = corridor_cost(O.rollout_rk4(shared, cols6, x0, U, Ts), U, xref, uprev, Q, R, P, hp, w)
        dev = np.zeros_like(c0)
        try:
            for sign in [1.0, -1.0] + [None] * draws:
                O.np = _PerturbedNumpy(eps, sign, rng)
                traj = O.rollout_rk4(shared, cols6, x0, U, Ts)
                O.np = real
                cj, _ = corridor_cost(traj, U, xref, uprev, Q, R, P, hp, w)
                dev = np.maximum(dev, np.abs(cj - c0) / np.abs(c0))
        finally:
            O.np = real
    return CORE_MARGIN * dev


def ulp_sensitivity_corridor(rollout, shared, cols6, x0, U, xref, uprev, Q, R, P, hp, w, Ts=0.02):
    """The largest relative change of J_c when x0 moves by one ulp (every component up, every
    component down, alternating): the NLP-Euler screen's sensitivity (x ULP_FACTOR there)."""
    x0 = np.asarray(x0, dtype=np.float64)

    def cost_of(x):
        with np.errstate(all="ignore"):
            return corridor_cost(rollout(shared, cols6, x, U, Ts), U, xref, uprev, Q, R, P, hp, w)[0]
    c0 = cost_of(x0)
    s = np.zeros_like(c0)
    for sign in (np.ones(6), -np.ones(6), np.array([1.0, -1, 1, -1, 1, -1])):
        xp = np.array([np.nextafter(v, np.inf * sg) for v, sg in zip(x0, sign)])
        s = np.maximum(s, np.abs(cost_of(xp) - c0) / np.abs(c0))
    return float(s.max())

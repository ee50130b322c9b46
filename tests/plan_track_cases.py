"""The track tick's cases (llampc_plan_track; no GPU needed): the closed-loop inputs on the recorded
states of dyn_slice.npz, the oracle's chain — the corridor along the previous chosen rollout shifted
one step, J_c on the oracle's own rollouts, the look-back selection with W = 2 — and the margins and
weights the device tests run under, with the shares they were chosen by.  Shared by
test_plan_track_cpu.py and test_plan_track_gpu.py.

The margins.  On these inputs (test_lookahead_matrix_gpu's builders moved along the record) the
rollouts of a tick lie in a bunch: at (C, H) = (3, 12) the pairs' largest offsets from ETHZ's centre
line span 0.5 mm, while the car itself closes in on the centre line by 14 mm per tick (0.16 m off it
at tick 0, 0.09 m at tick 5; the half width is 0.185 m).  Under ONE margin every tick has either all
of its pairs penalised or none: no constant satisfies "between 10 % and 90 % in two valid ticks"
(scanned from 0 to 0.14 m in steps of 5 mm on the oracle).  llampc_plan_track takes the margin per
tick, so the chain runs under one margin per tick: at tick t the half width is the 0.3 quantile, over
the (model, candidate) pairs, of the oracle rollouts' largest offset from the centre line along that
tick's path — margin_t = track_width / 2 - that, rounded to 1e-6 and frozen in CHAIN below (at the
long horizons the recorded inputs, full brake at full lock, carry most rollouts off the track: those
margins are negative, a corridor wider than the track).  About 70 % of the pairs then pay a penalty
in every valid tick.  The weight: at (3, 12) a slack is below 0.5 mm, and w = 1e4 (penalty 2.5e-3)
moves no argmin of the selected model; w = 1e6 moves it in ticks 2..5.  (64, 40) keeps w = 1e4 (tick 2).
test_plan_track_cpu.py::test_margin_preconditions recomputes the shares and the moved ticks on the
oracle and asserts them against CHAIN; the GPU tests assert them again before the device runs."""
import functools

import numpy as np

import corridor_ref as CR
from conftest import golden
from oracle import llampc_oracle as O

TS = 0.02
W, K = 2, 10
TICKS = 6
T0 = 40                          # the recorded state of tick 0
N = 97
HMAX = 64
UMIN, UMAX = np.array([-0.1, -0.35]), np.array([1.0, 0.35])
# (C, H) of the chain test and the edges
S, UW, H1, HM = (3, 12), (64, 40), (5, 1), (2, HMAX)
# (shape, track) -> weight, the margin of ticks 0..5 (tick 0 has no path: its margin is never used), the
# penalised share of the valid ticks 1..5 to 0.01, the ticks whose selected argmin the corridor moves
CHAIN = {
    (S, "ETHZ"): dict(weight=1e6, margins=(0.0, 0.052571, 0.067051, 0.081225, 0.09482, 0.107878),
                      shares=(0.70, 0.70, 0.70, 0.70, 0.70), moved=(2, 3, 4, 5)),
    (UW, "ETHZ"): dict(weight=1e4, margins=(0.0, -0.222379, -0.232711, -0.210713, -0.220762, -0.238578),
                       shares=(0.70, 0.70, 0.70, 0.70, 0.70), moved=(2,)),
    (H1, "ETHZ"): dict(weight=1e6, margins=(0.0, 0.052335, 0.066566, 0.080742, 0.094505, 0.107682),
                       shares=(0.70, 0.70, 0.70, 0.70, 0.70), moved=(2, 3, 4, 5)),
    (HM, "ETHZ"): dict(weight=1e4, margins=(0.0, -0.573446, -0.588086, -0.536391, -0.519784, -0.83252),
                       shares=(0.70, 0.70, 0.70, 0.70, 0.70), moved=()),
    (S, "square"): dict(weight=1e6, margins=(0.0, 0.197019, 0.211914, 0.22616, 0.239821, 0.252925),
                        shares=(0.70, 0.70, 0.70, 0.70, 0.70), moved=(2, 3, 4, 5)),
}


@functools.lru_cache(maxsize=None)
def track(name="ETHZ"):
    """ETHZ('optimal', True), or `square`: four centre points, a 2 m square whose left side the recorded
    car runs along (most lanes of a corridor block's scan hold no segment), 2.4 m wide."""
    from llampc.tracks import ETHZ, Track
    if name == "ETHZ":
        return ETHZ('optimal', True)
    tr = Track()
    tr.x_center = np.array([0.3, 2.3, 2.3, 0.3])
    tr.y_center = np.array([-0.1, -0.1, 1.9, 1.9])
    tr.track_width = 2.4
    tr._init_geometry()
    return tr


def shared():
    p = O.orca_params()
    return {k: p[k] for k in ("lf", "lr", "mass", "Iz", "Cm1", "Cm2", "Cr0", "Cr2")}


@functools.lru_cache(maxsize=None)
def bank():
    from llampc.mpc import generate_bank
    p = generate_bank(N, seed=97)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def tick_inputs(t, C, H):
    """Tick t of the closed loop, test_lookahead_matrix_gpu.realistic_inputs moved along the record:
    (x_prev, u_prev, x_t, uprev, U [C, H, 2], xref [2, H+1]) — the recorded transition t - 1 -> t, the
    recorded inputs from step t for every candidate with uniform +-0.03 noise on candidates 1..,
    the straight line from x_t at its speed and heading, offset by (+0.01, -0.02)."""
    d = golden("dyn_slice.npz")
    s, u = d["states"], d["inputs"]
    i = T0 + t
    x_prev, u_prev, x_t = s[:, i - 1].copy(), u[:, i - 1].copy(), s[:, i].copy()
    base = u[:, i:i + H].T.copy()
    assert base.shape == (H, 2)
    U = np.repeat(base[None], C, axis=0)
    rng = np.random.RandomState(1000 * C + H + t)
    U[1:] = np.clip(U[1:] + rng.uniform(-0.03, 0.03, (C - 1, H, 2)), UMIN, UMAX)
    v, tt = np.hypot(x_t[3], x_t[4]), np.arange(H + 1) * TS
    xref = np.vstack([x_t[0] + v * np.cos(x_t[2]) * tt + 0.01, x_t[1] + v * np.sin(x_t[2]) * tt - 0.02])
    out = (x_prev, u_prev, x_t, u_prev.copy(), U, xref)
    for a in out:
        a.setflags(write=False)
    return out


def path_index(j, H):
    """csrc/ctl.hpp ctl_path_index: the index of X that path point j reads."""
    return j + 1 if j + 1 < H else H


def shifted(X, H):
    """P [2, H+1] from the chosen rollout's positions X [2, H+1]: P_j = X[path_index(j, H)]."""
    return np.ascontiguousarray(X[:, [path_index(j, H) for j in range(H + 1)]])


@functools.lru_cache(maxsize=None)
def oracle_chain(shape, track_name="ETHZ", ticks=TICKS):
    """The chain on the oracle alone under CHAIN's margins and weight: per tick dict(valid, path, hp,
    plain [N, C], cref [N, C], pen, sel, cand, share, moved).  Tick 0 runs without a look-back (current
    model 0), tick 1 with a window that is not full, ticks 2.. select argmin of the W = 2 window mean."""
    from llampc.mpc import constraints
    C, H = shape
    row = CHAIN[(shape, track_name)]
    tr, sh, p = track(track_name), shared(), tuple(bank())
    Q, R, P = np.eye(2), np.diag([5e-3, 1.0]), np.zeros((2, 2))
    outs, errs, path = [], [], None
    for t in range(ticks):
        x_prev, u_prev, x_t, uprev, U, xref = tick_inputs(t, C, H)
        hp = constraints.disabled(H) if path is None else constraints.track_corridor(tr, path, row["margins"][t])
        with np.errstate(all="ignore"):
            traj = O.rollout_rk4(sh, p, x_t, U, TS)
        jc, pen = CR.corridor_cost(traj, U, xref, uprev, Q, R, P, hp, row["weight"])
        plain = O.mpc_cost(traj, U, xref, uprev, Q, R, P).reshape(N, C)
        cref, pen = jc.reshape(N, C), pen.reshape(N, C)
        sel = 0
        if t >= 1:
            errs.append(O.lookback_errors(O.evaluate_models_vectorized(sh, p, x_prev, u_prev, TS), x_t))
            if len(errs) >= W:
                sel = int(np.argmin((errs[-2] + errs[-1]) / 2))
        cand = int(np.argmin(cref[sel]))
        outs.append(dict(valid=path is not None, path=path, hp=hp, plain=plain, cref=cref, pen=pen, sel=sel, cand=cand,
                         share=float(np.mean(pen > 0)), moved=cand != int(np.argmin(plain[sel]))))
        X = traj[:, sel * C + cand, :2].T
        path = shifted(X, H) if np.isfinite(cref[sel, cand]) and np.isfinite(X).all() else None
    return outs


def chosen_positions(x_t, U, sel, cand):
    """X [2, H+1] of (sel, cand) on the oracle's RK4 rollout from x_t."""
    with np.errstate(all="ignore"):
        traj = O.rollout_rk4(shared(), tuple(bank()[:, sel:sel + 1]), x_t, U[cand:cand + 1], TS)
    return traj[:, 0, :2].T

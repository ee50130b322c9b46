"""The controller tick's soft track corridor (LLAMPC(corridor_weight=...), llampc_ctl_set_corridor,
csrc/ctl_corr.hip): its rows, its oracle and its checker, shared by test_ctl_corridor_cpu.py (the
conditions, on the oracle alone) and test_ctl_corridor_gpu.py (the device against the oracle).

The specification the oracle restates.  A corridor tick t of a controller with a track, a weight
w > 0 and a margin m:
  corridor   hp_t [H, 6] = constraints.track_corridor(track, P, m) along P = constraints.default_path(
             ., H, Ts, prev_xy): the positions X_0..X_H of tick t - 1's chosen rollout (the selected model,
             or the nominal model while warm, on sel_cand; X_0 = x_{t-1}) shifted one step, the last
             repeated — when tick t - 1 was a corridor tick whose chosen cost and H + 1 chosen positions
             were finite; else constraints.disabled(H) (tick 0, the first tick after switching on, a tick
             after a non-finite chosen rollout).  Nothing in hp_t depends on x_t.
  costs      every rolled-out (slot, candidate) cost is J + w pen, pen = corridor_ref.penalty(hp_t,
             rollout) (the plan kernel's corridor look-ahead); infeasible keeps +inf, a NaN rollout NaN.
  the rest   reference, candidates, look-back, selection, mu-hat and the record: ControllerOracle's.

A row is a ctl_matrix.Row plus the corridor's half width (None: margin 0, the full track) and weight.
The rows' claims (TABLE: the share of penalised rolled-out candidates, the ticks with a valid path) are
recomputed by the CPU file; every row keeps ctl_matrix.tick_gaps above GAP_COST on this oracle."""
import contextlib
import ctypes

import numpy as np

import corridor_ref
import ctl_matrix as M
from oracle import llampc_oracle as O

WEIGHT = 100.0
COMMON = dict(W=4, K=10, ticks=14, bank_seed=21)


class Row(M.Row):
    def __init__(self, name, half=None, weight=WEIGHT, **kw):
        super().__init__(name, **{**COMMON, **kw})
        self.half, self.weight = half, weight


ROWS = [
    Row("ethz-c8", half=0.08, N=200, C=8, H=20, track="ETHZ", variant=dict(lpm=4),
        what="every candidate penalised; w pen up to 31 against J ~ 20"),
    Row("ethz-c96", half=0.10, N=100, C=96, H=20, track="ETHZ", variant=dict(lpm=2), what="every candidate penalised"),
    Row("ethz-c200", half=0.10, N=100, C=200, H=20, track="ETHZ", variant=dict(lpm=1), what="every candidate penalised"),
    Row("mobil-wide", half=None, N=200, C=8, H=20, track="ETHZMobil", variant=dict(lpm=4),
        what="no candidate penalised: the costs equal the plain oracle's"),
    Row("mobil-mixed", half=0.15, N=200, C=8, H=20, track="ETHZMobil", variant=dict(lpm=4),
        what="slack on some lanes only"),
    Row("mobil-h40", half=0.15, N=200, C=64, H=40, track="ETHZMobil", variant=dict(lpm=4),
        what="the benchmark's C and H"),
    Row("ethz-nan", half=0.10, N=200, C=8, H=20, track="ETHZ", nan_models=M.NAN_MODELS, nan_first=True,
        variant=dict(lpm=4), what="NaN-first selects the NaN model: the disabled fallback"),
]
BY_NAME = {r.name: r for r in ROWS}
BITES = [r for r in ROWS if r.name != "mobil-wide"]
ARMED = [BY_NAME[n] for n in ("ethz-c8", "ethz-c200", "mobil-h40")]

# name -> (lowest, highest share of the rolled-out (slot, candidate) costs with pen > 0, ticks with a
# valid path of the 14) on this oracle; test_ctl_corridor_cpu.py recomputes them
TABLE = {
    "ethz-c8": (0.99, 1.0, 13),
    "ethz-c96": (0.99, 1.0, 13),
    "ethz-c200": (0.99, 1.0, 13),
    "mobil-wide": (0.0, 0.0, 13),
    "mobil-mixed": (0.03, 0.05, 13),
    "mobil-h40": (0.015, 0.025, 13),
    "ethz-nan": (0.10, 0.20, 5),
}


def margin(row):
    tr, _ = M.tracks(row.track)
    return 0.0 if row.half is None else float(tr.track_width) / 2 - row.half


def track_n(row):
    tr, _ = M.tracks(row.track)
    return int(np.asarray(tr.center_line).shape[1])


class CorridorOracle(O.ControllerOracle):
    """ControllerOracle with the corridor ticks' semantics (module doc).  tick(x_t, hp=None): hp given
    (the device's own corridor of the tick, so that the comparison does not inherit its 1e-12) or
    built by the rule.  The tick's dict gains hp, path (P [2, H+1] or None), path_valid, pen (the
    rolled-out penalties [slots, C]) and chosen_xy (X [2, H+1]) / chosen_valid for the next tick."""

    def __init__(self, *a, weight=WEIGHT, margin=0.0, pkg_track=None, **kw):
        super().__init__(*a, **kw)
        self.weight, self.margin, self.pkg_track = float(weight), float(margin), pkg_track
        self.prev_xy, self.prev_valid = None, False
        self.hp = None
        self._pen = []

    # -- the rule (the mutants override one of these) ----------------------------------------------
    def path(self, x_t):
        from llampc.mpc import constraints
        return constraints.default_path(None, self.H, self.Ts, self.prev_xy)

    def penalty_weight(self):
        return self.weight

    def corridor(self, x_t):
        """(hp [H, 6], path or None, valid) of this tick by the rule."""
        from llampc.mpc import constraints
        if not self.prev_valid:
            return constraints.disabled(self.H), None, False
        P = self.path(x_t)
        return constraints.track_corridor(self.pkg_track, P, self.margin), P, True

    # -- ControllerOracle's hooks --------------------------------------------------------------------
    def costs(self, cols, x_t, U, xref, uprev):
        traj = O.rollout_rk4(self.shared, tuple(cols), x_t, U, self.Ts)
        J = O.mpc_cost(traj, U, xref, uprev, self.Q, self.R, self.P)
        pen = corridor_ref.penalty(self.hp, traj)
        wp = self.penalty_weight() * pen
        cost = J + wp
        ok = O.candidates_feasible(U, uprev, self.umin, self.umax, self.rate_max[1], self.Ts,
                                   rate_max_pwm=self.rate_max[0])
        ncols = cols[0].shape[0]
        self._pen.append(pen.reshape(ncols, self.C))
        return np.where(np.tile(ok, ncols), cost, np.inf).reshape(ncols, self.C)

    def tick(self, x_t, hp=None):
        x_t = np.asarray(x_t, dtype=np.float64)
        own, P, valid = self.corridor(x_t)
        self.hp = own if hp is None else np.asarray(hp, dtype=np.float64)
        self._pen = []
        with np.errstate(all="ignore"):
            o = super().tick(x_t)
            # the chosen rollout: the selected model (the nominal one while warm) on the chosen candidate
            col = self.nominal.reshape(6, 1) if o["warm"] else self.bank[:, [o["best_model"]]]
            c = o["best_cand"]
            traj = O.rollout_rk4(self.shared, tuple(col), x_t, o["U"][c:c + 1], self.Ts)
        xy = traj[:, 0, :2].T.copy()
        ok = bool(np.isfinite(o["cost"]) and np.isfinite(xy).all())
        # super().tick evaluates the selection before the top-K: the device's slot order is the reverse
        pen = np.vstack(self._pen[::-1]) if len(self._pen) > 1 else self._pen[0]
        o.update(hp=self.hp, path=P, path_valid=valid, pen=pen, chosen_xy=xy, chosen_valid=ok)
        self.prev_xy, self.prev_valid = xy, ok
        return o


class AlongXref(CorridorOracle):
    """Mutant: the corridor along the tick's own ConstantSpeed reference."""

    def path(self, x_t):
        return self.reference(x_t)[0]


class NotShifted(CorridorOracle):
    """Mutant: the previous chosen rollout as it is, not shifted one step."""

    def path(self, x_t):
        return self.prev_xy.copy()


class NoPenalty(CorridorOracle):
    """Mutant: the penalty dropped."""

    def penalty_weight(self):
        return 0.0


MUTANTS = (AlongXref, NotShifted, NoPenalty)


def oracle_for(row, cls=CorridorOracle):
    tr, ref = M.tracks(row.track)
    return cls(M.shared(), M.bank(row), ref, tr.lap_projidx, H=row.H, C=row.C, K=row.K, W=row.W, Ts=row.Ts,
               v_factor=row.v_factor, mu_init=row.mu_init, S=row.S, sigma=row.sigma, seed=row.seed, Q=row.Q, R=row.R,
               P=row.P, umin=row.umin, umax=row.umax, rate_max=row.rate_max, nan_first=row.nan_first,
               weight=row.weight, margin=margin(row), pkg_track=tr)


def plant_step(row, plant, x, o):
    """ctl_matrix.reference's plant: RK6, Df / Dr dropping 1/260 per tick, the chosen first input."""
    plant.Df *= 1 - 1 / 260.0
    plant.Dr *= 1 - 1 / 260.0
    xn, _ = O.sim_continuous(plant, x, np.asarray(o["u_seq"])[:, 0].reshape(2, 1), [0, row.Ts])
    return xn[:, -1]


_CACHE = {}


def reference(row, cls=CorridorOracle):
    """The oracle's closed loop of the row (ticks, states), computed once per (row, class), read-only."""
    key = (row.name, cls.__name__)
    if key not in _CACHE:
        orc = oracle_for(row, cls)
        plant = O.Vehicle.from_params(O.orca_params())
        x = M.start_state(row)
        outs, xs = [], []
        for _ in range(row.ticks):
            o = orc.tick(x)
            for v in o.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            outs.append(o)
            xs.append(x.copy())
            x = plant_step(row, plant, x, o)
        _CACHE[key] = (outs, xs)
    return _CACHE[key]


# ---- the checker: ctl_matrix.check_tick with the corridor cost's own core-error bound --------------------
def pair_bounds(row, o, x, pairs, eps=None):
    """ctl_matrix.pair_bounds for J + w pen (corridor_ref.core_error_bound_corridor)."""
    nom = M.nominal6()
    return [corridor_ref.core_error_bound_corridor(M.shared(), M._cols(row, nom, [m]), x, o["U"][c:c + 1], o["xref"],
                                                   o["uprev"], row.Q, row.R, row.P, o["hp"], row.weight, Ts=row.Ts,
                                                   eps=eps)[0] for m, c in pairs]


@contextlib.contextmanager
def _corridor_bounds(eps):
    real = M.pair_bounds
    M.pair_bounds = lambda row, o, x, pairs: pair_bounds(row, o, x, pairs, eps)
    try:
        yield
    finally:
        M.pair_bounds = real


PATH_ATOL = 1e-6        # the look-ahead rows' state tolerance (test_lookahead_*): the path against the oracle's
HP_ATOL = 1e-12         # corridor_dev.hpp against constraints.track_corridor (test_nlp_track_corridor_gpu.py)


def check_tick(row, t, o, x, res, xref, U, projidx_in, counts, cor, costs, eps=None):
    """One tick's record (res: a CtlResult) and corridor (cor: LLAMPC.corridor()'s (path, hp, theta,
    valid)) against the corridor oracle's tick o.  The corridor first: valid equals the oracle's; with a
    valid path, the path within PATH_ATOL of the oracle's shifted chosen rollout and hp within HP_ATOL of
    constraints.track_corridor(track, that device path, margin); without, hp bitwise
    constraints.disabled(H).  Then ctl_matrix.check_tick — its tolerances (RTOL_ROLL, exact indices), its
    counts for the BOUND_SHARE_MAX cap — with the bounds of the corridor cost, and every rolled-out cost
    (costs: LLAMPC.corridor_costs(); check_slot_costs).  eps: the lean cores' relative errors (None:
    measured on the device)."""
    from llampc.mpc import constraints
    tr, _ = M.tracks(row.track)
    path, hp, _, valid = cor
    tag = f"{row.name} tick {t}"
    assert bool(valid) == bool(o["path_valid"]), tag
    if valid:
        np.testing.assert_allclose(path, o["path"], rtol=0, atol=PATH_ATOL, err_msg=tag)
        np.testing.assert_allclose(hp, constraints.track_corridor(tr, path, margin(row)), rtol=0, atol=HP_ATOL, err_msg=tag)
    else:
        assert np.asarray(hp).tobytes() == constraints.disabled(row.H).tobytes(), tag
    with _corridor_bounds(eps):
        M.check_tick(row, t, o, x, res, xref, U, projidx_in, counts)
    check_slot_costs(row, o, x, costs, counts, eps, tag)


def check_slot_costs(row, o, x, costs, counts, eps, tag):
    """Every rolled-out cost of the tick (costs: LLAMPC.corridor_costs(), [slots, C] in the record's
    slot order) against the oracle's slot_costs: the same NaN / +inf pattern, RTOL_ROLL or the pair's
    core-error bound (conftest.assert_costs_close), counted with the record's pairs for the
    BOUND_SHARE_MAX cap.  The record alone carries each slot's best candidate: a penalty on the others
    (mobil-mixed: on no slot's best) would go unchecked."""
    from conftest import assert_costs_close
    want = np.asarray(o["slot_costs"])
    models = list(o["slot_models"])
    costs = np.asarray(costs)
    if o["warm"]:
        assert costs.shape == (1, row.C), (tag, costs.shape)
        got = costs
    else:
        assert costs.shape == (row.K + 1, row.C), (tag, costs.shape)
        kk = len(models) - 1                      # min(N, K) top-K slots, then the selection's at K
        assert np.isnan(costs[kk:row.K]).all(), tag
        got = np.vstack([costs[:kk], costs[row.K:]])
    assert got.shape == want.shape, (tag, got.shape, want.shape)

    def bound(idx):
        return pair_bounds(row, o, x, [(models[int(i) // row.C], int(i) % row.C) for i in idx], eps)

    counts["pairs"] += int(np.isfinite(want).sum())
    counts["bound"] += assert_costs_close(got, want, M.RTOL_ROLL, bound)


def record_from(row, o):
    """The llampc_ctl_out an exact device would write for the oracle's tick o, as a CtlResult: what the
    CPU file feeds the checker with (a mutant's tick against the true oracle's record)."""
    from llampc import _native as nat
    from llampc.mpc.controller import CtlResult
    r = nat.CtlOut()
    p = r.plan
    nan = float("nan")
    p.window_count, p.window_full, p.K, p.sel_owned = o["window_count"], int(o["window_full"]), row.K, 1
    p.sel_model, p.sel_cand, p.sel_cost, p.n_nonfinite = o["best_model"], o["best_cand"], o["cost"], o["n_nonfinite"]
    p.status = 0
    for k in range(nat.KMAX):
        p.topk[k], p.topk_cand[k] = -1, -1
        p.topk_val[k] = p.topk_Df[k] = p.topk_Dr[k] = p.topk_cost[k] = nan
    if o["warm"]:
        p.lb_best, p.lb_best_val = -1, nan
        p.la_best_model, p.la_best_cand, p.la_best_cost = -1, -1, nan
    else:
        p.lb_best, p.lb_best_val = o["lb_best"], o["lb_best_val"]
        p.la_best_model, p.la_best_cand, p.la_best_cost = o["la_best_model"], o["la_best_cand"], o["la_best_cost"]
        for k in range(len(o["topk"])):
            p.topk[k], p.topk_cand[k] = int(o["topk"][k]), int(o["topk_cand"][k])
            p.topk_val[k], p.topk_cost[k] = o["topk_val"][k], o["topk_cost"][k]
            p.topk_Df[k], p.topk_Dr[k] = o["topk_Df"][k], o["topk_Dr"][k]
    r.tick, r.projidx, r.warm = o["tick"], o["projidx"], int(o["warm"])
    r.mu_used = nan if o["mu_used"] is None else o["mu_used"]
    r.scale_used = o["scale_used"]
    r.mu_pred = nan if o["mu_pred"] is None else o["mu_pred"]
    r.dr_mean, r.df_mean = o["dr_mean"], o["df_mean"]
    useq = np.ascontiguousarray(np.asarray(o["u_seq"]).T)
    ctypes.memmove(r.u_seq, useq.ctypes.data, useq.nbytes)
    return CtlResult(r, row.H)


def device_costs(row, o):
    """LLAMPC.corridor_costs() of an exact device for the oracle's tick o: its slot_costs in the
    record's K + 1 slots (NaN where the bank has no model for a top-K slot), one slot while warm."""
    sc = np.asarray(o["slot_costs"])
    if o["warm"]:
        return sc.copy()
    out = np.full((row.K + 1, row.C), np.nan)
    out[:len(sc) - 1] = sc[:-1]
    out[row.K] = sc[-1]
    return out


def variant(row):
    """llampc_ctl_variant_corridor of the row's shape on its track (host only)."""
    from llampc import _native as nat
    return nat.ctl_variant_corridor(row.N, row.C, row.H, row.K, M.KNOTS[row.track], track_n(row))


def controller(row, b, prelaunch=False, corridor=True):
    """LLAMPC in device mode over ModelBank b with the row's configuration and corridor (or none)."""
    from llampc import _native as nat
    from llampc.mpc import LLAMPC
    tr, _ = M.tracks(row.track)
    return LLAMPC(b, tr, H=row.H, Ts=row.Ts, K=row.K, C=row.C, v_factor=row.v_factor, mu_init=row.mu_init, S=row.S,
                  cost=M.cost(row), seed=row.seed, nan_policy=nat.NAN_FIRST if row.nan_first else nat.NAN_IGNORE,
                  sigma=row.sigma, debug_inputs=True, prelaunch=prelaunch,
                  corridor_weight=row.weight if corridor else 0.0, corridor_margin=margin(row) if corridor else 0.0)

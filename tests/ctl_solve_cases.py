"""The fused control step's rows (LLAMPC.step, llampc_ctl_step; csrc/ctl_solve.hip) and their oracle
chain, shared by test_ctl_solve_cpu.py (the conditions, on the oracle alone) and
test_ctl_solve_gpu.py (the device against the chain).

The chain is built from what oracle/ already has.  Per tick t at state x:

    o = ControllerOracle.tick(x)
    p6 = the nominal model if o["warm"], else bank[:, o["best_model"]]
    u, j = O.nlp_cem(shared, p6, x, o["xref"], o["uprev"], base=o["u_seq"].T, has_hold=True, ...,
                     call=the number of solves so far), with the controller's cost and bounds
    if u is not None: orc.u_seq, orc.u_prev = u, u[0]        (the commit)

and the plant (ctl_matrix.reference's RK6 vehicle, Df / Dr dropping 1/260 per tick) is driven by the
applied input: u[0], or the tick's own candidate when the solve found nothing finite or the tick was
a plain one (``plain``).  ``J0`` is the NLP objective of the tick's chosen sequence: sample 0 of the
solve's round 0 is that sequence, so fval <= J0.

Rows (W = 2, K = 3, C = 8, bank seed 21, NLP seed 0, sigma0 (0.3, 0.15), floor 1e-4): the smallest
shapes that still cross every branch —

  base          ETHZ, N = 200, H = 20, 9 ticks; NLP (64 samples, 8 elite, 3 rounds): warm -> selected,
                the model changing; one block
  blocks4       H = 22, 8 ticks; (256, 17, 3): four blocks, a pad list
  mobil-H40     ETHZMobil, N = 100, H = 40, 7 ticks; (128, 64, 2): the unstaged horizon, list length
                64, the 500-knot table
  nan-selected  base with nan_models = (0, 57), 7 ticks: from tick 3 the NaN model 0 is selected, no
                objective is finite, nothing is committed and the tick's candidate carries on
  mixed         base with tick 4 a plain tick(): the call word counts steps, not ticks, and that
                tick's candidate is the applied input

CHAIN_GAP_MIN = 1e-7 is the smallest relative gap between adjacent elite costs a compared solve may
have: nlp_matrix's 1e-9 assumes bit-identical inputs, and here the device's xref is held to the
oracle's at 1e-10 only, hence three orders above that."""
import numpy as np

import ctl_matrix as CM
from oracle import llampc_oracle as O

CHAIN_GAP_MIN = 1e-7
NLP_SEED = 0
NLP_SIGMA = (0.3, 0.15)
NLP_FLOOR = 1e-4


class SRow:
    """A fused-step row: ``row`` the ctl_matrix.Row of its controller, ``nlp`` = (samples, elite,
    iters), ``plain`` the ticks that are a plain tick() (no solve), ``fail_from`` the first tick whose
    solve must find nothing finite (None: every solve succeeds)."""

    def __init__(self, name, nlp, plain=(), fail_from=None, what="", **kw):
        kw = dict(dict(N=200, C=8, H=20, K=3, W=2, bank_seed=21), **kw)
        self.name, self.row, self.nlp, self.plain, self.fail_from, self.what = name, CM.Row(name, **kw), nlp, tuple(plain), fail_from, what

    def __repr__(self):
        return self.name

    def solve_kw(self):
        """LLAMPC(solve=...) of the row."""
        samples, elite, iters = self.nlp
        return dict(samples=samples, elite=elite, iters=iters, sigma=NLP_SIGMA, std_floor=NLP_FLOOR, seed=NLP_SEED)


ROWS = [
    SRow("base", (64, 8, 3), ticks=9, what="warm -> selected, the model changing; one block"),
    SRow("blocks4", (256, 17, 3), H=22, ticks=8, what="four blocks, a pad list"),
    SRow("mobil-H40", (128, 64, 2), N=100, H=40, track="ETHZMobil", ticks=7,
         what="the unstaged horizon, list length 64, the 500-knot table"),
    SRow("nan-selected", (64, 8, 3), ticks=7, nan_models=(0, 57), fail_from=3,
         what="the NaN model 0 is selected: nothing finite, nothing committed"),
    SRow("mixed", (64, 8, 3), ticks=9, plain=(4,), what="tick 4 a plain tick(): the call word counts steps"),
]
BY_NAME = {r.name: r for r in ROWS}

# Rows moved off bank seed 21 because the oracle chain misses a condition there: name -> (the fields
# changed, what was missed).  The conditions stay.
REPICKED = {}
for _name, (_kw, _why) in REPICKED.items():
    for _k, _v in _kw.items():
        setattr(BY_NAME[_name].row, _k, _v)


def model_p6(row, o):
    """The parameters the tick's solve runs with: the nominal model while warm, else the selection's."""
    return tuple(float(v) for v in (CM.nominal6() if o["warm"] else CM.bank(row)[:, int(o["best_model"])]))


def nlp_kw(srow):
    """oracle.nlp_cem's keywords of the row: the controller's cost, bounds and rate bounds."""
    row = srow.row
    samples, elite, iters = srow.nlp
    m = row.rate_max
    return dict(samples=samples, iters=iters, elite=elite, sigma0=NLP_SIGMA, std_floor=NLP_FLOOR, seed=NLP_SEED,
                Q=row.Q, R=row.R, P=row.P, umin=row.umin, umax=row.umax,
                rate_lo=tuple(None if v is None else -v * row.Ts for v in m),
                rate_hi=tuple(None if v is None else v * row.Ts for v in m),
                rate_max_steer=m[1], rate_max_pwm=m[0])


def nlp_objective(srow, p6, x, U, xref, uprev):
    """The Euler-NLP objective of sequences U [n, H, 2] (+inf where infeasible), as nlp_cem ranks them."""
    row = srow.row
    U = np.ascontiguousarray(U, dtype=np.float64)
    with np.errstate(all="ignore"):
        traj = O.rollout_euler_nlp(CM.shared(), tuple(np.array([v]) for v in p6), x, U, row.Ts)
        J = O.mpc_cost(traj, U, xref, uprev, row.Q, row.R, row.P)
    m = row.rate_max
    ok = O.candidates_feasible(U, uprev, row.umin, row.umax, np.inf if m[1] is None or m[1] < 0 else m[1], row.Ts, m[0])
    return np.where(ok, J, np.inf)


def solve(srow, o, x, call):
    """The chain's solve of tick o at state x: dict(u [H, 2] or None, j, info, J0, p6, call)."""
    row = srow.row
    p6 = model_p6(row, o)
    info = {}
    base = np.ascontiguousarray(o["u_seq"].T)
    with np.errstate(all="ignore"):
        u, j = O.nlp_cem(CM.shared(), p6, x, o["xref"], o["uprev"], base, True, row.H, row.Ts, call=call, info=info,
                         **nlp_kw(srow))
    J0 = float(nlp_objective(srow, p6, x, base[None], o["xref"], o["uprev"])[0])
    if u is not None:
        u.setflags(write=False)
    return dict(u=u, j=j, info=info, J0=J0, p6=p6, call=call)


_CACHE = {}


def chain(srow, applied=None):
    """The row's closed loop on the oracle, computed once and left unchanged: per tick a dict
    (o: the oracle's tick, x: the state, sol: the solve or None on a plain tick, u0: the applied
    input [2]).  applied(t, o) -> (u0 [2], useq [H, 2] or None), if given, replaces the solve on
    every tick: the overridden oracle that llampc_ctl_set_applied is held to (not cached)."""
    if applied is None and srow.name in _CACHE:
        return _CACHE[srow.name]
    row = srow.row
    orc = CM.oracle_for(row)
    plant = O.Vehicle.from_params(O.orca_params())
    x = CM.start_state(row)
    out, call = [], 0
    for t in range(row.ticks):
        with np.errstate(all="ignore"):
            o = orc.tick(x)
        sol = None
        u0 = o["u_seq"][:, 0].copy()
        if applied is not None:
            u0, useq = applied(t, o)
            u0 = np.array(u0, dtype=np.float64)
            if useq is None:
                useq = orc.u_seq.copy()
                useq[0] = u0
            orc.u_seq, orc.u_prev = np.array(useq, dtype=np.float64), u0.copy()
        elif t not in srow.plain:
            sol = solve(srow, o, x, call)
            call += 1
            if sol["u"] is not None:
                orc.u_seq, orc.u_prev = sol["u"].copy(), sol["u"][0].copy()
                u0 = sol["u"][0].copy()
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        xc = x.copy()
        xc.setflags(write=False)
        out.append(dict(o=o, x=xc, sol=sol, u0=u0))
        plant.Df *= 1 - 1 / 260.0
        plant.Dr *= 1 - 1 / 260.0
        xn, _ = O.sim_continuous(plant, x, u0.reshape(2, 1), [0, row.Ts])
        x = xn[:, -1]
    if applied is None:
        _CACHE[srow.name] = out
    return out


def check_conditions(srow, t, step):
    """On the oracle alone, one tick of the chain: printed, then asserted.  Every compared solve has
    every sample finite in every round (a failing tick: none) and its elite gap above CHAIN_GAP_MIN;
    fval <= J0; the tick's own gaps stay above ctl_matrix's."""
    row, o, sol = srow.row, step["o"], step["sol"]
    gc, gf, gm = CM.tick_gaps(row, o)
    line = f"{srow.name} tick {t}: model {o['best_model']} warm {o['warm']} gaps cand {gc:.3g} flat {gf:.3g} mean {gm:.3g}"
    if sol is None:
        print(line + " | plain tick")
    else:
        info = sol["info"]
        print(line + f" | call {sol['call']} finite {info['finite']} best round {info['best_round']} gap {info['gap']:.3g} "
              f"fval {sol['j']!r} J0 {sol['J0']!r}")
    assert gc > CM.GAP_COST and gf > CM.GAP_COST and gm > CM.GAP_MEAN, (srow.name, t, gc, gf, gm)
    if sol is None:
        return
    samples, _, iters = srow.nlp
    failing = srow.fail_from is not None and t >= srow.fail_from
    if failing:
        assert sol["info"]["finite"] == [0] * iters and sol["u"] is None, (srow.name, t, sol["info"]["finite"])
        return
    assert sol["info"]["finite"] == [samples] * iters, (srow.name, t, sol["info"]["finite"])
    assert sol["info"]["gap"] > CHAIN_GAP_MIN, (srow.name, t, sol["info"]["gap"])
    assert sol["u"] is not None and sol["j"] <= sol["J0"], (srow.name, t, sol["j"], sol["J0"])


def controller(srow, b, solve=True, debug_inputs=True, **kw):
    """LLAMPC in device mode over ModelBank b with the row's configuration; solve: with the row's
    solver attached (which forces prelaunch off), else a plain launched controller."""
    from llampc import _native as nat
    from llampc.mpc import LLAMPC
    row = srow.row
    tr, _ = CM.tracks(row.track)
    return LLAMPC(b, tr, H=row.H, Ts=row.Ts, K=row.K, C=row.C, v_factor=row.v_factor, mu_init=row.mu_init, S=row.S,
                  cost=CM.cost(row), seed=row.seed, nan_policy=nat.NAN_FIRST if row.nan_first else nat.NAN_IGNORE,
                  sigma=row.sigma, debug_inputs=debug_inputs, prelaunch=False,
                  solve=srow.solve_kw() if solve else None, **kw)


# ---- llampc_ctl_set_applied's reference: the oracle with overridden u_prev / u_seq --------------------
OFFSET = np.array([0.07, -0.03])


def offset_applied(srow):
    """applied(t, o) of test 3: the chosen u0 plus a fixed offset, clipped to the bounds; the chosen
    sequence is kept (its row 0 replaced)."""
    row = srow.row

    def f(t, o):
        return np.clip(o["u_seq"][:, 0] + OFFSET, row.umin, row.umax), None
    return f

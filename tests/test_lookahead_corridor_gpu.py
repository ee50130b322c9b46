"""The look-ahead under a soft track corridor (llampc_lookahead_corridor, llampc_plan_corridor) against
the oracle: J_c = O.mpc_cost + w pen on the oracle's own rollouts (tests/corridor_ref.py).

Every case runs the 97-model bank of test_lookahead_matrix_gpu on its realistic inputs, under the
strip around the reference line whose half width is the oracle's median, over the pairs, of the
largest lateral offset (weight 1e4): about half of the pairs pay a penalty, up to 3,000 times their
unconstrained cost, and it changes the per-model argmin of 20-48 models wherever C > 1.  Both are
asserted on the oracle alone before the device runs (a kernel that ignores hp fails the argmin
check).  One case differs: NLP-Euler at H = 1, where the position after one step depends on neither
the model nor the candidate — every pair has the same offset, the strip is 0.9 of it and every pair
pays the same penalty.

The lanes per rollout are forced with LLAMPC_LPM and asserted, with the staging, through
llampc_plan_variant_corridor.  Inputs are held to the oracle's own J_c moving by <= RTOL_ROLL: RK4
under the cores' measured errors (conftest.core_error_bound's construction on cost + penalty),
NLP-Euler under ULP_FACTOR one-ulp sensitivities.  Then: the same NaN / inf pattern, every finite
cost within RTOL_ROLL (relative, no absolute slack), the per-model argmin and the global best by
the separation rule (check_choice).

Each case prints one `CORRIDOR` line (variant, largest relative cost error, condition, share of
penalised pairs, models whose argmin the corridor changed): the source of DESIGN.md's table."""
import numpy as np
import pytest

import corridor_ref as CR
from conftest import golden
from oracle import llampc_oracle as O
from test_lookahead_matrix_gpu import (COSTS, F8, H1, H64, LPMS, MW, N, RATE_PWM, RATE_STEER, RTOL_ROLL, RTOL_STEP, S,
                                       STAGED, ULP_FACTOR, UMAX, UMIN, UW, bank, check_choice,
                                       check_costs_and_choices, close, feasibility_inputs, nat,  # noqa: F401
                                       realistic_inputs, shared)

pytestmark = pytest.mark.gpu

TS = 0.02
WEIGHT = 1e4
FLIP = (31, 64)                  # staged without the corridor, unstaged with its 48 H bytes
STAGED_C = {**STAGED, FLIP: False}
INTEGRATORS = ("rk4", "euler_nlp")

_REF = {}


def reference(integrator, shape, cost="default", feas=False):
    """The case's inputs, corridor and oracle costs, computed once and shared by the lanes per
    rollout: dict(x0, uprev, U, xref, hp, plain [N, C], cref [N, C] (J_c, +inf where infeasible),
    pen [N, C], ok [C], bound, changed).  The preconditions are asserted here, on the oracle."""
    key = (integrator, shape, cost, feas)
    if key in _REF:
        return _REF[key]
    C, H = shape
    x0, uprev, U, xref = feasibility_inputs(C, H, TS) if feas else realistic_inputs(C, H, TS)
    p, sh = bank(), shared()
    Q, R, P = COSTS[cost]
    with np.errstate(all="ignore"):
        traj = CR.ROLLOUTS[integrator](sh, tuple(p), x0, U, TS)
    same = integrator == "euler_nlp" and H == 1          # module doc
    hp = CR.median_strip(traj, xref, 0.9 if same else 1.0)
    hp.setflags(write=False)
    jc, pen = CR.corridor_cost(traj, U, xref, uprev, Q, R, P, hp, WEIGHT)
    plain = O.mpc_cost(traj, U, xref, uprev, Q, R, P).reshape(N, C)
    cref, pen = jc.reshape(N, C), pen.reshape(N, C)
    ok = np.ones(C, dtype=bool)
    if feas:
        ok = O.candidates_feasible(U, uprev, UMIN, UMAX, RATE_STEER, TS, rate_max_pwm=RATE_PWM)
        cref, plain = np.where(ok[None, :], cref, np.inf), np.where(ok[None, :], plain, np.inf)
    changed = int(np.sum(np.argmin(cref, axis=1) != np.argmin(plain, axis=1)))
    if same:
        assert pen[0, 0] > 0 and np.all(pen == pen[0, 0])
    else:
        assert np.mean(pen > 0) >= 0.25 and np.mean(pen == 0) >= 0.25, np.mean(pen > 0)
        if C > 1:
            assert changed >= 1, "the corridor must change some model's argmin"
    if integrator == "rk4":
        bound = float(CR.core_error_bound_corridor(sh, tuple(p), x0, U, xref, uprev, Q, R, P, hp, WEIGHT, Ts=TS).max())
    else:
        bound = ULP_FACTOR * CR.ulp_sensitivity_corridor(O.rollout_euler_nlp, sh, tuple(p), x0, U, xref, uprev, Q, R, P,
                                                         hp, WEIGHT, Ts=TS)
    cref.setflags(write=False)
    _REF[key] = dict(x0=x0, uprev=uprev, U=U, xref=xref, hp=hp, plain=plain, cref=cref, pen=pen, ok=ok, bound=bound,
                     changed=changed)
    return _REF[key]


def variant(nat, monkeypatch, integrator, lpm, shape):
    """Force the lanes per rollout and assert the corridor launch takes the variant the case means."""
    monkeypatch.setenv("LLAMPC_LPM", str(lpm))
    v = nat.plan_variant_corridor(N, shape[0], shape[1], integrator)
    assert (v["lpm"], v["stage"]) == (lpm, STAGED_C[shape]), (integrator, lpm, shape, v)
    return f"({integrator}, {v['lpm']}, {'staged' if v['stage'] else 'unstaged'}) G={v['G']}"


def cost_struct(nat, cost, feas=False):
    Q, R, P = COSTS[cost]
    return nat.cost_struct(Q=Q, R=R, P=P, rate_max=(RATE_PWM, RATE_STEER) if feas else (-1.0, RATE_STEER),
                           enforce_bounds=feas)


def run_case(nat, monkeypatch, integrator, lpm, shape, cost="default", feas=False):
    from llampc.mpc import ModelBank
    C, H = shape
    vtxt = variant(nat, monkeypatch, integrator, lpm, shape)
    ref = reference(integrator, shape, cost, feas)
    assert ref["bound"] <= RTOL_ROLL, f"ill-conditioned input (condition {ref['bound']:.3g}): choose another input"
    with ModelBank(bank(), device=0) as b:
        n0 = b.launches
        r = b.lookahead(ref["x0"], ref["U"], ref["xref"], ref["uprev"], Ts=TS, cost=cost_struct(nat, cost, feas),
                        integrator=integrator, return_costs=True, return_best_cand=True, corridor=ref["hp"],
                        corridor_weight=WEIGHT)
        assert b.launches == n0 + 1
    cref = ref["cref"]
    err, ties = check_costs_and_choices(r["costs"], cref, r["best_cand_per_model"], r["best_model"], r["best_cand"],
                                        r["best_cost"])
    print(f"CORRIDOR {vtxt} C={C} H={H} cost={cost} feas={int(feas)}: err {err:.2e} bound {ref['bound']:.2e} "
          f"penalised {np.mean(ref['pen'] > 0):.3f} argmin changed {ref['changed']} ties {ties}")
    assert err <= RTOL_ROLL, err          # relative on every finite pair (close() adds an absolute term)
    if feas:
        ok = ref["ok"]
        assert np.all(np.isposinf(r["costs"][:, ~ok])) and np.all(np.isfinite(r["costs"][:, ok]))
        heavy = WEIGHT * ref["pen"][:, ok] > ref["plain"][:, ok]      # the penalty outweighs the cost itself
        assert heavy.any() and np.all(r["costs"][:, ok][heavy] > 2 * ref["plain"][:, ok][heavy] * (1 - RTOL_ROLL))
    return r


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


MATRIX = [(l, sh) for sh in (S, UW, H1, H64) for l in LPMS] + [(1, MW), (2, FLIP)]


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("lpm,shape", MATRIX, ids=_ids)
def test_parity_diagonal_weights(nat, monkeypatch, integrator, lpm, shape):
    """Q = I, P = 0: at LPM 4 the corridor launch takes the unsplit rollout where the plain launch
    splits the position.  Staged, unstaged, a model across four waves (LPM 1), H = 1 and H = 64, and
    the shape the corridor's own LDS moves from staged to unstaged."""
    run_case(nat, monkeypatch, integrator, lpm, shape)


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("lpm", LPMS)
def test_parity_full_weights(nat, monkeypatch, integrator, lpm):
    run_case(nat, monkeypatch, integrator, lpm, S, cost="full")


def test_parity_enforce_bounds(nat, monkeypatch):
    """The feasibility mask still gives +inf; the finite pairs carry the penalty."""
    run_case(nat, monkeypatch, "rk4", 4, F8, feas=True)


# ----------------------------------------------------------------- the corridor that changes nothing
# (integrator, lpm, shape, cost) -> bitwise?  Bitwise wherever the plain launch runs the unsplit
# rollout too; at LPM 4 with diagonal Q and P it runs the split / quadrature rollout: RTOL_ROLL.
NOOP = [("rk4", 2, S, "default", True), ("rk4", 1, S, "default", True), ("rk4", 4, S, "full", True),
        ("euler_nlp", 4, S, "default", True), ("euler_nlp", 2, S, "default", True), ("euler_nlp", 1, S, "default", True),
        ("rk4", 1, UW, "default", True), ("euler_nlp", 4, UW, "default", True),
        ("rk4", 4, S, "default", False), ("rk4", 4, UW, "default", False)]


@pytest.mark.parametrize("integrator,lpm,shape,cost,bitwise", NOOP, ids=_ids)
def test_noop_corridor_equals_the_plain_launch(nat, monkeypatch, integrator, lpm, shape, cost, bitwise):
    """constraints.disabled(H) at weight 1e4, and the live corridor at weight 0."""
    from llampc.mpc import ModelBank, constraints
    variant(nat, monkeypatch, integrator, lpm, shape)
    ref = reference(integrator, shape, cost)
    args = (ref["x0"], ref["U"], ref["xref"], ref["uprev"])
    kw = dict(Ts=TS, cost=cost_struct(nat, cost), integrator=integrator, return_costs=True, return_best_cand=True)
    with ModelBank(bank(), device=0) as b:
        plain = b.lookahead(*args, **kw)
        for hp, w in ((constraints.disabled(shape[1]), WEIGHT), (ref["hp"], 0.0)):
            r = b.lookahead(*args, corridor=hp, corridor_weight=w, **kw)
            if bitwise:
                np.testing.assert_array_equal(r["costs"], plain["costs"])
                np.testing.assert_array_equal(r["best_cand_per_model"], plain["best_cand_per_model"])
                assert (r["best_model"], r["best_cand"], r["best_cost"]) == \
                    (plain["best_model"], plain["best_cand"], plain["best_cost"])
            else:
                np.testing.assert_allclose(r["costs"], plain["costs"], rtol=RTOL_ROLL, atol=0)
            np.testing.assert_allclose(r["costs"], ref["plain"], rtol=RTOL_ROLL, atol=0)


# ----------------------------------------------------------------- the fused tick
@pytest.mark.parametrize("lpm", [4, 1])
def test_fused_tick_with_corridor(nat, monkeypatch, lpm):
    """plan_raw(corridor=hp) on a W = 1 bank: the look-back half untouched (errors at RTOL_STEP, the
    selection from the oracle's look-back), the record's choices against J_c — once with the
    outputs copied back, once record-only — and one launch per tick."""
    from llampc.mpc import ModelBank
    C, H = S
    variant(nat, monkeypatch, "rk4", lpm, S)
    ref = reference("rk4", S)
    assert ref["bound"] <= RTOL_ROLL
    cref = ref["cref"]
    d = golden("dyn_slice.npz")
    x_prev, u_prev = d["states"][:, 39].copy(), d["inputs"][:, 39].copy()
    p = bank()
    e = O.lookback_errors(O.evaluate_models_vectorized(shared(), tuple(p), x_prev, u_prev, TS), ref["x0"])
    sel = int(np.argmin(e))
    assert np.sort(e)[1] - e[sel] > 10 * RTOL_STEP * e[sel], "the look-back selection must be decided"
    assert np.argmin(cref[sel]) != np.argmin(ref["plain"][sel]), "the corridor must change the selected model's choice"
    with ModelBank(p, W=1, device=0) as b:
        for record_only in (False, True):
            n0 = b.launches
            out, err, _, costs = b.plan_raw(x_prev, u_prev, ref["x0"], ref["U"], ref["xref"], ref["uprev"], Ts=TS, K=10,
                                            cost=cost_struct(nat, "default"), return_errors=not record_only,
                                            return_costs=not record_only, corridor=ref["hp"], corridor_weight=WEIGHT)
            assert b.launches == n0 + 1
            o = nat.plan_out_to_dict(out)
            assert o["status"] == 0 and o["window_full"] and o["lb_best"] == sel and o["sel_model"] == sel
            check_choice(cref[sel:sel + 1], np.array([o["sel_cand"]]), "record: chosen candidate")
            check_choice(cref.reshape(1, -1), np.array([o["la_best_model"] * C + o["la_best_cand"]]), "record: global best")
            np.testing.assert_allclose(o["sel_cost"], cref[sel, o["sel_cand"]], rtol=RTOL_ROLL)
            np.testing.assert_allclose(o["la_best_cost"], cref[o["la_best_model"], o["la_best_cand"]], rtol=RTOL_ROLL)
            assert o["n_nonfinite"] == 0
            if not record_only:
                close(err, e, RTOL_STEP)
                np.testing.assert_allclose(costs, cref, rtol=RTOL_ROLL, atol=0)


# ----------------------------------------------------------------- refusals
def test_refusals_enqueue_nothing(nat, monkeypatch):
    """LLAMPC_E_ARG with the launch counter unchanged: RK6, the raceline reference, a NaN normal, a
    -inf offset, a negative weight (the C entry points themselves: the Python layer raises
    ValueError for the first two and the last before it calls them)."""
    from llampc.mpc import ModelBank
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    C, H = S
    ref = reference("rk4", S)
    lib, ct = nat.load(), nat.C
    U, xref, x0, uprev = (nat.f64(ref[k]) for k in ("U", "xref", "x0", "uprev"))
    cs = cost_struct(nat, "default")
    costs = np.empty((N, C))

    def lookahead(b, hp, w, integ=nat.RK4):
        bm, bc, bv = ct.c_int64(), ct.c_int32(), ct.c_double()
        hp = nat.f64(hp)
        return lib.llampc_lookahead_corridor(b.handle, nat.dptr(x0), nat.dptr(U), C, H, nat.dptr(xref), nat.dptr(uprev),
                                             ct.byref(cs), TS, integ, nat.dptr(costs), None, ct.byref(bm), ct.byref(bc),
                                             ct.byref(bv), nat.dptr(hp), float(w))

    def bad(k, v):
        hp = ref["hp"].copy()
        hp.flat[k] = v
        return hp
    with ModelBank(bank(), W=1, device=0) as b:
        n0 = b.launches
        assert lookahead(b, ref["hp"], WEIGHT, nat.RK6) == nat.E_ARG
        assert "RK6" in lib.llampc_last_error().decode()
        pin, keep = b._plan_in(np.zeros(6), np.zeros(2), x0, U, xref, uprev, TS, 10, "rk4", True, True, 0, nat.NAN_FIRST,
                               cs, raceline_start=(0.0, 1.0, 1.0))
        out = nat.PlanOut()
        hp = nat.f64(ref["hp"])
        assert lib.llampc_plan_corridor(b.handle, ct.byref(pin), nat.dptr(hp), WEIGHT, ct.byref(out), None, None,
                                        None) == nat.E_ARG
        assert "RACELINE" in lib.llampc_last_error().decode()
        assert lookahead(b, bad(6 * 3 + 1, float("nan")), WEIGHT) == nat.E_ARG
        assert lookahead(b, bad(6 * 5 + 2, -np.inf), WEIGHT) == nat.E_ARG
        assert lookahead(b, bad(6 * 7 + 5, float("nan")), WEIGHT) == nat.E_ARG
        assert lookahead(b, ref["hp"], -1.0) == nat.E_ARG
        assert lookahead(b, ref["hp"], float("inf")) == nat.E_ARG
        assert lib.llampc_lookahead_corridor(b.handle, nat.dptr(x0), nat.dptr(U), C, H, nat.dptr(xref), nat.dptr(uprev),
                                             ct.byref(cs), TS, nat.RK4, None, None, None, None, None, None,
                                             WEIGHT) == nat.E_ARG
        assert b.launches == n0
        with pytest.raises(nat.NativeError) as ei:       # through the Python layer: the library's E_ARG
            b.lookahead(x0, U, xref, uprev, corridor=bad(0, np.inf))
        assert ei.value.code == nat.E_ARG and b.launches == n0
        # a +inf offset disables a half-plane and is accepted; the bank still ticks
        assert lookahead(b, bad(2, np.inf), WEIGHT) == 0 and b.launches == n0 + 1

"""Look-ahead parity over the variant table: integrator (RK4, NLP-Euler, RK6) x lanes per
rollout (LPM 4, 2, 1) x staged / unstaged candidate inputs x a model inside one wave / across
waves, for the default and weighted costs, the feasibility mask (both rate bounds, a non-zero
uprev), other time steps than 0.02, an input_acc bank and the horizon edges H = 1 and H = 64.

Every case builds its inputs from the recorded slice (tests/golden/dyn_slice.npz, step 40), runs a
97-model bank (prime: every block layout ends in a ragged block), forces the lanes per rollout
with LLAMPC_LPM, asserts through llampc_plan_variant that the launch takes the (lpm, stage) it
means to test, and compares against the oracle's rollout + cost + feasibility:
  * equal NaN / inf patterns, every finite cost within RTOL_ROLL (1e-7, never widened);
  * the per-model argmin exact wherever the oracle's best and runner-up differ by more than
    2 RTOL_ROLL (relative), elsewhere the chosen candidate's ORACLE cost within 2 RTOL_ROLL of the
    minimum; the global best by the same rule; an infeasible candidate never chosen while a
    feasible one exists.
RK4 inputs are first held to conftest.core_error_bound(...).max() <= RTOL_ROLL (the oracle's own
rollout under the device cores' measured errors; it never sees the kernel's output): an input
that fails it is ill-conditioned and has to be replaced, not its tolerance.  NLP-Euler and RK6
inputs are held to ULP_FACTOR times the oracle's own one-ulp sensitivity <= RTOL_ROLL (below).
Inputs replaced for that reason: H = 64 uses the recorded inputs instead of one held input; the
feasibility candidates ride on a rising pwm; RK6 runs its unstaged shape at Ts = 0.01, and its
Ts = 0.05 case at H = 6.

RK6 reference: O.rk6 (the scalar odeintRK6 restatement) is given the whole batch as one flat
state vector with a batched right-hand side (O.diffequation_batch), so all 97 models are compared;
two rollouts per case are also checked against O.sim_continuous itself.

Each case prints one `MATRIX` line (family, variant, largest relative cost error, the condition of
its input — the core-error bound or the scaled sensitivity — and the near-tied models): the source
of the table in DESIGN.md §4."""
import numpy as np
import pytest

from conftest import core_error_bound, golden
from oracle import llampc_oracle as O

pytestmark = pytest.mark.gpu

RTOL_STEP = 1e-9
RTOL_ROLL = 1e-7
N = 97
UMIN, UMAX = np.array([-0.1, -0.35]), np.array([1.0, 0.35])
RATE_PWM, RATE_STEER = 8.0, 5.0                      # family C: both rate bounds live
# NLP-Euler / RK6 conditioning (reference(): no core-error model covers them).  The device's general
# sin / cos / atan / atan2 are within ~4 ulp of NumPy's, and on the rollouts that are sensitive at
# all the sensitivity grows geometrically along the horizon (measured on the RK6 oracle: x5 per 4
# steps, 1.4e-10 at H = 24 -> 1.1e-7 at H = 40), so the earliest roundings dominate and the sum over
# the later ones is below 3x the first: 4 ulp x 3 ~ 10 one-ulp sensitivities.  An input whose
# oracle cost moves by more than RTOL_ROLL / 10 under one ulp of x0 is replaced (a shorter H).
ULP_FACTOR = 10.0
X_SLOW = np.array([0.1, 0.2, 0.3, 0.03, 0.01, 0.2])  # vx < vmin: the NLP form's clamp

# (C, H) -> staged?  (192 + 16 (H + 1) + 64 C H <= 128 KiB; asserted through llampc_plan_variant)
S, UW, MW, ONE, F8 = (3, 12), (64, 40), (130, 20), (1, 12), (8, 12)
H1, H64, S_SHORT = (5, 1), (2, 64), (3, 6)
STAGED = {S: True, UW: False, MW: False, ONE: True, F8: True, H1: True, H64: True, S_SHORT: True}

_QF, _PF = np.array([[1.0, 0.3], [0.2, 2.0]]), np.array([[0.5, -0.1], [0.4, 1.0]])
COSTS = {
    "default": (np.eye(2), np.diag([5e-3, 1.0]), np.zeros((2, 2))),
    "diag": (np.diag([2.0, 0.5]), np.diag([5e-3, 1.0]), np.diag([3.0, 0.25])),         # the LPM-4 split
    "full": (_QF, np.array([[5e-3, 2e-3], [1e-3, 1.0]]), _PF),
    "full_upper": (_QF, np.array([[5e-3, 3e-3], [0.0, 1.0]]), _PF),                     # same R[1] + R[2]
    "full_neg": (_QF, np.array([[5e-3, -2e-3], [-2e-3, 1.0]]), _PF),
    "full_rdiag": (_QF, np.diag([5e-3, 1.0]), _PF),                                     # oracle only
}
LPMS = (4, 2, 1)


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


def shared(acc=False):
    p = O.orca_params()
    sh = {k: p[k] for k in ("lf", "lr", "mass", "Iz", "Cm1", "Cm2", "Cr0", "Cr2")}
    if acc:
        sh["input_acc"] = True
    return sh


def close(a, b, rtol, scale=None):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    fin = np.isfinite(b)
    np.testing.assert_array_equal(np.isfinite(a), fin)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    sc = np.max(np.abs(b[fin])) if scale is None and fin.any() else (scale or 1.0)
    np.testing.assert_allclose(a[fin], b[fin], rtol=rtol, atol=rtol * 1e-3 * sc)


_BANK = []


def bank():
    from llampc.mpc import generate_bank
    if not _BANK:
        p = generate_bank(N, seed=97)
        p.setflags(write=False)
        _BANK.append(p)
    return _BANK[0]


def realistic_inputs(C, H, Ts, slow=False):
    """x0 = the recorded state 40 (or the vx < vmin state), uprev = the recorded input 39, U = the
    recorded inputs from step 40 for every candidate with uniform +-0.03 noise on candidates 1..,
    clipped to the input bounds; xref = the straight line from x0 at its speed and heading, offset
    by (+0.01, -0.02).  (H = 64 uses the recorded inputs 40..103 too: holding input 40 — full
    brake at full steering lock — for 64 steps stops the car, and the oracle's own rollout then
    moves by 2e-4 relative under the cores' errors, far beyond the 1e-7 condition below.)"""
    d = golden("dyn_slice.npz")
    s, u = d["states"], d["inputs"]
    x0 = X_SLOW.copy() if slow else s[:, 40].copy()
    uprev = u[:, 39].copy()
    base = u[:, 40:40 + H].T.copy()
    assert base.shape == (H, 2)
    U = np.repeat(base[None], C, axis=0)
    rng = np.random.RandomState(1000 * C + H)
    U[1:] = np.clip(U[1:] + rng.uniform(-0.03, 0.03, (C - 1, H, 2)), UMIN, UMAX)
    return x0, uprev, U, straight_xref(x0, H, Ts)


def straight_xref(x0, H, Ts):
    v, t = np.hypot(x0[3], x0[4]), np.arange(H + 1) * Ts
    return np.vstack([x0[0] + v * np.cos(x0[2]) * t + 0.01, x0[1] + v * np.sin(x0[2]) * t - 0.02])


FEAS_MASK = [True, True, False, False, False, False, True, True]


def feasibility_inputs(C, H, Ts, all_infeasible=False):
    """Family C.  The base sequence starts at the recorded (non-zero) uprev: the steering held, the
    pwm rising by half its rate bound per step up to 0.5 (the recorded inputs themselves break the
    pwm rate bound, and uprev held for 40 steps — full brake at full lock — is ill-conditioned).
    Per candidate
      0 the base (feasible)               1 a steering step of exactly 5 Ts mid-horizon (feasible)
      2 that step times 1 + 1e-6          3 a step-0 steering value legal from 0, not from uprev
      4 pwm one ulp above umax (reached inside the pwm rate bound where the horizon allows it)
      5 a pwm step just beyond 8 Ts       6 steering at exactly umin (feasible)
      7.. the base + noise well inside both rate bounds (feasible)."""
    d = golden("dyn_slice.npz")
    x0, uprev = d["states"][:, 40].copy(), d["inputs"][:, 39].copy()
    assert np.all(uprev > UMIN) and np.all(uprev < UMAX) and abs(uprev[1]) > 0.3
    rp, rs = RATE_PWM * Ts, RATE_STEER * Ts
    U = np.tile(uprev, (C, H, 1))
    U[:, :, 0] = np.minimum(uprev[0] + 0.5 * rp * np.arange(1, H + 1), 0.5)
    m = H // 2
    sg = -np.sign(uprev[1])
    U[1, m:, 1] = uprev[1] + sg * rs
    U[2, m:, 1] = uprev[1] + sg * rs * (1 + 1e-6)
    U[3, :, 1] = sg * 0.9 * rs
    ramp = uprev[0] + 0.9 * rp * np.arange(1, H + 1)
    top = np.nextafter(UMAX[0], 2.0)
    if ramp[H - 2] >= UMAX[0]:                         # the bound alone: every step inside the rate
        U[4, :, 0] = np.minimum(ramp, UMAX[0])
        U[4, H - 1, 0] = top
    else:
        U[4, m:, 0] = top
    U[5, m:, 0] = U[5, m - 1, 0] + rp * (1 + 1e-6)
    U[6, :, 1] = np.maximum(uprev[1] - 0.9 * rs * np.arange(1, H + 1), UMIN[1])
    rng = np.random.RandomState(7 * C + H)
    U[7:] = np.clip(U[7:] + rng.uniform(-1, 1, (C - 7, H, 2)) * (0.2 * np.array([rp, rs])), UMIN, UMAX)
    if all_infeasible:
        U[:, 0, 0] = 1.2
    # the oracle's mask is the intended one, before anything runs
    ok = O.candidates_feasible(U, uprev, UMIN, UMAX, RATE_STEER, Ts, rate_max_pwm=RATE_PWM)
    if all_infeasible:
        assert not ok.any()
    else:
        assert list(ok) == FEAS_MASK + [True] * (C - 8), ok
        assert U[6, :, 1].min() == UMIN[1] and U[4].max() == top
        legal0 = O.candidates_feasible(U[3:4], np.array([uprev[0], 0.0]), UMIN, UMAX, RATE_STEER, Ts, RATE_PWM)
        assert legal0[0], "candidate 3 is legal from a zero previous steering"
        # 4 and 5 are refused by the pwm bounds alone: without the pwm rate bound 5 passes, and so
        # does 4 up to its last step where the ramp reaches umax inside the horizon
        no_pwm_rate = O.candidates_feasible(U, uprev, UMIN, UMAX, RATE_STEER, Ts)
        assert no_pwm_rate[5] and not no_pwm_rate[4]
    return x0, uprev, U, straight_xref(x0, H, Ts)


def rollout_rk6(sh, p, x0, U, Ts, check=True):
    """[H+1, N*C, 6] (lane n*C + c): one O.rk6 step per control interval on the flattened batch."""
    n, C, H = p.shape[1], U.shape[0], U.shape[1]
    L = n * C
    par = {k: np.repeat(p[i], C) for i, k in enumerate(O.BANK_ORDER)}
    v = O.Vehicle(**{k: sh[k] for k in ("lf", "lr", "mass", "Iz", "Cm1", "Cm2", "Cr0", "Cr2")}, **par,
                  input_acc=bool(sh.get("input_acc", False)))
    f = lambda t, y, ub: O.diffequation_batch(v, y.reshape(L, 6), ub).ravel()
    y = np.tile(np.asarray(x0, dtype=np.float64), (L, 1)).ravel()
    traj = np.empty((H + 1, L, 6))
    traj[0] = y.reshape(L, 6)
    for k in range(H):
        y = O.rk6(f, y, [0.0, Ts], (np.tile(U[:, k, :], (n, 1)),))[-1]
        traj[k + 1] = y.reshape(L, 6)
    # the batched use of O.rk6 is the scalar plant integrator: two rollouts against sim_continuous
    for n_, c in ((0, 0), (n - 1, C - 1)) if check else ():
        vs = O.Vehicle.from_params({**O.orca_params(), **{k: p[i, n_] for i, k in enumerate(O.BANK_ORDER)}})
        vs.input_acc = v.input_acc
        xs, _ = O.sim_continuous(vs, x0, U[c].T, np.arange(H + 1) * Ts)
        np.testing.assert_allclose(traj[:, n_ * C + c], xs.T, rtol=1e-9, atol=1e-12)
    return traj


_REF = {}


def reference(key, integrator, acc, x0, uprev, U, xref, Ts, cost, enforce):
    """(cref [N, C] with +inf where infeasible, feasible [C], core-error bound or nan), computed
    once per input set and shared by the cases that differ only in the lanes per rollout."""
    if key not in _REF:
        p, sh = bank(), shared(acc)
        Q, R, P = COSTS[cost]
        def cost_of(x):
            with np.errstate(all="ignore"):
                if integrator == "rk4":
                    traj = O.rollout_rk4(sh, tuple(p), x, U, Ts)
                elif integrator == "euler_nlp":       # the NLP form ignores input_acc
                    traj = O.rollout_euler_nlp(shared(), tuple(p), x, U, Ts)
                else:
                    traj = rollout_rk6(sh, p, x, U, Ts, check=x is x0)
                return O.mpc_cost(traj, U, xref, uprev, Q, R, P).reshape(N, U.shape[0])

        cref = cost_of(x0)
        ok = np.ones(U.shape[0], dtype=bool)
        if enforce:
            ok = O.candidates_feasible(U, uprev, UMIN, UMAX, RATE_STEER, Ts, rate_max_pwm=RATE_PWM)
            cref = np.where(ok[None, :], cref, np.inf)
        if integrator == "rk4":
            bound = float(core_error_bound(sh, tuple(p), x0, U, xref, uprev, Q, R, P, Ts=Ts).max())
        else:
            # No core-error model exists for these two integrators (they evaluate the general
            # transcendentals, a few ulp from NumPy's).  Their condition is the oracle's own
            # sensitivity: the largest relative cost change when x0 moves by one ulp (every
            # component up, every component down, alternating), times ULP_FACTOR.
            c0 = cost_of(x0).ravel()
            s = np.zeros_like(c0)
            for sign in (np.ones(6), -np.ones(6), np.array([1.0, -1, 1, -1, 1, -1])):
                xp = np.array([np.nextafter(v, np.inf * sg) for v, sg in zip(x0, sign)])
                s = np.maximum(s, np.abs(cost_of(xp).ravel() - c0) / np.abs(c0))
            bound = ULP_FACTOR * float(s.max())
        cref.setflags(write=False)
        _REF[key] = (cref, ok, bound)
    return _REF[key]


def check_choice(cm, got, what):
    """cm [rows, K] oracle costs (NaN as +inf), got [rows] the device's choice per row: exact
    where the best and the runner-up are separated by more than 2 RTOL_ROLL, else a choice whose
    oracle cost is within 2 RTOL_ROLL of the minimum; all-inf rows choose 0.  Returns the number
    of rows decided by the cost check (near ties)."""
    rows = np.arange(cm.shape[0])
    assert np.all((got >= 0) & (got < cm.shape[1])), (what, got)
    want = np.argmin(cm, axis=1)
    best = cm[rows, want]
    rest = cm.copy()
    rest[rows, want] = np.inf
    second = rest.min(axis=1)
    none = ~np.isfinite(best)
    np.testing.assert_array_equal(got[none], 0, err_msg=f"{what}: all candidates infeasible -> 0")
    with np.errstate(invalid="ignore"):
        sep = ~none & ((second - best) > 2 * RTOL_ROLL * np.abs(best))
    np.testing.assert_array_equal(got[sep], want[sep], err_msg=what)
    near = ~none & ~sep
    chosen = cm[rows, got]
    assert np.all(np.isfinite(chosen[~none])), f"{what}: an infeasible candidate chosen over a feasible one"
    assert np.all(chosen[near] - best[near] <= 2 * RTOL_ROLL * np.abs(best[near])), \
        (what, np.max((chosen[near] - best[near]) / np.abs(best[near])))
    return int(near.sum())


def check_costs_and_choices(costs, cref, per_model, best_model, best_cand, best_cost):
    """The assertions of every case; returns (largest relative cost error, near-tied models)."""
    C = cref.shape[1]
    close(costs, cref, RTOL_ROLL)
    cm = np.where(np.isnan(cref), np.inf, cref)
    ties = check_choice(cm, np.asarray(per_model, dtype=np.int64), "per-model argmin")
    check_choice(cm.reshape(1, -1), np.array([best_model * C + best_cand]), "global best")
    assert 0 <= best_model < N and 0 <= best_cand < C
    got_best = costs[best_model, best_cand]
    assert best_cost == got_best or (np.isinf(best_cost) and np.isinf(got_best)), (best_cost, got_best)
    fin = np.isfinite(cref)
    err = float(np.max(np.abs(costs[fin] - cref[fin]) / np.abs(cref[fin]))) if fin.any() else 0.0
    return err, ties


def variant(nat, monkeypatch, integrator, lpm, shape):
    """Force the lanes per rollout and assert the launch takes the variant the case means."""
    monkeypatch.setenv("LLAMPC_LPM", str(lpm))
    v = nat.plan_variant(N, shape[0], shape[1], integrator)
    assert (v["lpm"], v["stage"]) == (lpm, STAGED[shape]), (integrator, lpm, shape, v)
    return f"({integrator}, {v['lpm']}, {'staged' if v['stage'] else 'unstaged'}) G={v['G']}"


def run_case(nat, monkeypatch, fam, integrator, lpm, shape, Ts=0.02, cost="default", acc=False, slow=False,
             feas=None):
    """One look-ahead launch against the oracle.  feas: None (realistic inputs, bounds not
    enforced), "mask" or "none_feasible" (family C inputs, enforce_bounds with both rate bounds)."""
    from llampc.mpc import ModelBank
    C, H = shape
    vtxt = variant(nat, monkeypatch, integrator, lpm, shape)
    if feas is None:
        x0, uprev, U, xref = realistic_inputs(C, H, Ts, slow)
    else:
        x0, uprev, U, xref = feasibility_inputs(C, H, Ts, all_infeasible=feas == "none_feasible")
    key = (integrator, shape, Ts, cost, acc, slow, feas)
    cref, ok, bound = reference(key, integrator, acc, x0, uprev, U, xref, Ts, cost, feas is not None)
    assert bound <= RTOL_ROLL, f"ill-conditioned input (condition {bound:.3g} > {RTOL_ROLL:g}): choose another input"
    Q, R, P = COSTS[cost]
    cs = nat.cost_struct(Q=Q, R=R, P=P, rate_max=(RATE_PWM, RATE_STEER) if feas else (-1.0, RATE_STEER),
                         enforce_bounds=feas is not None)
    with ModelBank(bank(), device=0, input_acc=acc) as b:
        r = b.lookahead(x0, U, xref, uprev, Ts=Ts, cost=cs, integrator=integrator, return_costs=True,
                        return_best_cand=True)
    err, ties = check_costs_and_choices(r["costs"], cref, r["best_cand_per_model"], r["best_model"],
                                        r["best_cand"], r["best_cost"])
    if feas == "none_feasible":     # llampc.h: candidate 0 of model 0 at +inf (np.argmin over all-inf)
        assert np.all(np.isposinf(r["costs"])) and np.all(r["best_cand_per_model"] == 0)
        assert (r["best_model"], r["best_cand"]) == (0, 0) and np.isposinf(r["best_cost"])
    elif feas:
        assert np.all(np.isposinf(r["costs"][:, ~ok])) and np.all(np.isfinite(r["costs"][:, ok]))
    print(f"MATRIX {fam} {vtxt} C={C} H={H} Ts={Ts} cost={cost} acc={int(acc)} slow={int(slow)} feas={feas}: "
          f"err {err:.2e} bound {bound:.2e} ties {ties}")
    return r["costs"], cref


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


# ----------------------------------------------------------------- A: integrator x LPM x staging
A_EULER = [(l, sh) for sh in (S, UW, ONE) for l in LPMS] + [(1, MW)]
A_RK4 = [(l, sh) for sh in (S, UW) for l in LPMS] + [(1, MW)]


@pytest.mark.parametrize("slow", [False, True], ids=["recorded", "vx_below_vmin"])
@pytest.mark.parametrize("lpm,shape", A_EULER, ids=_ids)
def test_a_euler_nlp(nat, monkeypatch, lpm, shape, slow):
    """NLP-Euler at every lanes-per-rollout, staged (the plan kernel's record of pwm, delta, sin,
    cos, rate term, feasibility) and unstaged, a model across four waves (C = 130) and a single
    candidate; from the recorded state and from the vx < vmin state (the clamp of
    dynamic.py:195-226)."""
    run_case(nat, monkeypatch, "A", "euler_nlp", lpm, shape, slow=slow)


@pytest.mark.parametrize("shape,Ts", [(S, 0.02), (UW, 0.01), (MW, 0.02), (ONE, 0.02)], ids=_ids)
def test_a_rk6(nat, monkeypatch, shape, Ts):
    """RK6 staged, unstaged within a wave, across four waves, one candidate.  The unstaged shape
    runs at Ts = 0.01: at 0.02 the oracle's own RK6 cost of some (slippery model, candidate) pairs
    moves by 1e-7 under one ulp of x0 (condition 1e-6; 1e-11 at Ts = 0.01)."""
    run_case(nat, monkeypatch, "A", "rk6", 1, shape, Ts=Ts)


@pytest.mark.parametrize("lpm,shape", A_RK4, ids=_ids)
def test_a_rk4_control(nat, monkeypatch, lpm, shape):
    """The control row: RK4 on the same inputs (the other rows are read against it)."""
    run_case(nat, monkeypatch, "A", "rk4", lpm, shape)


# ----------------------------------------------------------------- B: cost weights
@pytest.mark.parametrize("shape", [S, UW], ids=_ids)
@pytest.mark.parametrize("lpm", LPMS)
def test_b_diagonal_weights(nat, monkeypatch, lpm, shape):
    """Q = diag(2, .5), P = diag(3, .25): the position split at LPM 4, the plain path below."""
    run_case(nat, monkeypatch, "B", "rk4", lpm, shape, cost="diag")


@pytest.mark.parametrize("shape", [S, UW], ids=_ids)
@pytest.mark.parametrize("lpm", LPMS)
def test_b_full_weights_and_r_offdiagonal(nat, monkeypatch, lpm, shape):
    """Full Q, P and R = [[5e-3, 2e-3], [1e-3, 1]] (act_term's off-diagonal terms, staged record
    and unstaged route); du' R du only sees R[1] + R[2], so R = [[5e-3, 3e-3], [0, 1]] must give
    the same costs (to rounding: 1e-12, the two forms differ by a few ulp per step's term)."""
    a, _ = run_case(nat, monkeypatch, "B", "rk4", lpm, shape, cost="full")
    b, _ = run_case(nat, monkeypatch, "B", "rk4", lpm, shape, cost="full_upper")
    np.testing.assert_allclose(b, a, rtol=1e-12)


@pytest.mark.parametrize("lpm,shape", [(4, S), (1, UW)], ids=_ids)
def test_b_negative_r_offdiagonal_differs_from_diagonal(nat, monkeypatch, lpm, shape):
    """R[1] = R[2] = -2e-3: the costs follow the oracle's and differ from the diagonal-R costs
    wherever the oracle's do (a kernel that drops the off-diagonal terms returns the latter)."""
    got, cref = run_case(nat, monkeypatch, "B", "rk4", lpm, shape, cost="full_neg")
    C, H = shape
    x0, uprev, U, xref = realistic_inputs(C, H, 0.02)
    cdiag, _, _ = reference(("rk4", shape, 0.02, "full_rdiag", False, False, None), "rk4", False, x0, uprev, U, xref,
                            0.02, "full_rdiag", False)
    differs = np.abs(cdiag - cref) > 100 * RTOL_ROLL * np.abs(cref)
    assert differs.sum() >= N, "the inputs must make the off-diagonal terms visible"
    assert np.all(np.abs(got - cdiag)[differs] > 50 * RTOL_ROLL * np.abs(cref[differs]))


@pytest.mark.parametrize("integrator,lpm", [("euler_nlp", 4), ("euler_nlp", 1), ("rk6", 1)])
def test_b_full_weights_other_integrators(nat, monkeypatch, integrator, lpm):
    run_case(nat, monkeypatch, "B", integrator, lpm, S, cost="full")


# ----------------------------------------------------------------- C: feasibility
@pytest.mark.parametrize("shape", [F8, UW], ids=_ids)
@pytest.mark.parametrize("lpm", LPMS)
def test_c_feasibility_rk4(nat, monkeypatch, lpm, shape):
    """enforce_bounds with the recorded non-zero uprev and both rate bounds: the staged record's
    feasibility word (H = 12) and the unstaged input_feasible route (C = 64, H = 40); the mask, the
    finite costs and the choices."""
    run_case(nat, monkeypatch, "C", "rk4", lpm, shape, feas="mask")


@pytest.mark.parametrize("integrator,lpm", [("euler_nlp", 4), ("euler_nlp", 1), ("rk6", 1)])
def test_c_feasibility_other_integrators(nat, monkeypatch, integrator, lpm):
    run_case(nat, monkeypatch, "C", integrator, lpm, F8, feas="mask")


@pytest.mark.parametrize("Ts", [0.01, 0.05])
@pytest.mark.parametrize("lpm", LPMS)
def test_c_feasibility_bound_moves_with_ts(nat, monkeypatch, lpm, Ts):
    """The rate bounds are rate_max Ts: the candidates sit at 5 Ts and 8 Ts for this Ts."""
    run_case(nat, monkeypatch, "C", "rk4", lpm, F8, Ts=Ts, feas="mask")


@pytest.mark.parametrize("lpm,shape", [(4, F8), (1, UW)], ids=_ids)
def test_c_every_candidate_infeasible(nat, monkeypatch, lpm, shape):
    """llampc.h: every cost +inf, every model's best candidate 0, the global best (0, 0) at +inf."""
    run_case(nat, monkeypatch, "C", "rk4", lpm, shape, feas="none_feasible")


# ----------------------------------------------------------------- D: time step
@pytest.mark.parametrize("Ts", [0.01, 0.05])
@pytest.mark.parametrize("lpm", LPMS)
def test_d_time_step_rk4(nat, monkeypatch, lpm, Ts):
    """h folded into FusedK, the scaled yaw rate x[5] Ts (LPM 4 / 1) at other steps than 0.02."""
    run_case(nat, monkeypatch, "D", "rk4", lpm, S, Ts=Ts)


@pytest.mark.parametrize("lpm", LPMS)
def test_d_time_step_rk4_unstaged(nat, monkeypatch, lpm):
    run_case(nat, monkeypatch, "D", "rk4", lpm, UW, Ts=0.01)


@pytest.mark.parametrize("Ts", [0.01, 0.05])
@pytest.mark.parametrize("integrator,lpm", [("euler_nlp", 4), ("euler_nlp", 1), ("rk6", 1)])
def test_d_time_step_other_integrators(nat, monkeypatch, integrator, lpm, Ts):
    """RK6 at Ts = 0.05 runs H = 6: at H = 12 its oracle fails the conditioning screen (1.1e-7)."""
    run_case(nat, monkeypatch, "D", integrator, lpm, S_SHORT if (integrator, Ts) == ("rk6", 0.05) else S, Ts=Ts)


@pytest.mark.parametrize("lpm", LPMS)
def test_d_fused_tick_time_step(nat, monkeypatch, lpm):
    """The fused tick (plan_raw: look-back + look-ahead + selection in one launch) at Ts = 0.01
    with the diagonal weights: the look-back errors (lbl.Ts) at RTOL_STEP, the costs at RTOL_ROLL,
    the record's chosen candidate of the selected model and its global best by the separation
    rule — once with the outputs copied back and once record-only, where the inputs travel as
    kernel arguments (the inline pack: 16 + 26 + 72 doubles)."""
    from llampc.mpc import ModelBank
    Ts, (C, H) = 0.01, S
    vtxt = variant(nat, monkeypatch, "rk4", lpm, S)
    d = golden("dyn_slice.npz")
    x_prev, u_prev = d["states"][:, 39].copy(), d["inputs"][:, 39].copy()
    x0, uprev, U, xref = realistic_inputs(C, H, Ts)
    cref, _, bound = reference(("rk4", S, Ts, "diag", False, False, None), "rk4", False, x0, uprev, U, xref, Ts, "diag",
                               False)
    assert bound <= RTOL_ROLL
    p = bank()
    e = O.lookback_errors(O.evaluate_models_vectorized(shared(), tuple(p), x_prev, u_prev, Ts), x0)
    Q, R, P = COSTS["diag"]
    cs = nat.cost_struct(Q=Q, R=R, P=P)
    sel = int(np.argmin(e))
    assert np.sort(e)[1] - e[sel] > 10 * RTOL_STEP * e[sel], "the look-back selection must be decided"
    cm = np.where(np.isnan(cref), np.inf, cref)
    with ModelBank(p, W=1, device=0) as b:
        for record_only in (False, True):
            out, err, _, costs = b.plan_raw(x_prev, u_prev, x0, U, xref, uprev, Ts=Ts, K=10, cost=cs,
                                            return_errors=not record_only, return_costs=not record_only)
            o = nat.plan_out_to_dict(out)
            assert o["status"] == 0 and o["window_full"] and o["lb_best"] == sel and o["sel_model"] == sel
            check_choice(cm[sel:sel + 1], np.array([o["sel_cand"]]), "record: chosen candidate")
            check_choice(cm.reshape(1, -1), np.array([o["la_best_model"] * C + o["la_best_cand"]]), "record: global best")
            np.testing.assert_allclose(o["sel_cost"], cref[sel, o["sel_cand"]], rtol=RTOL_ROLL)
            np.testing.assert_allclose(o["la_best_cost"], cref[o["la_best_model"], o["la_best_cand"]], rtol=RTOL_ROLL)
            if not record_only:
                close(err, e, RTOL_STEP)
                close(costs, cref, RTOL_ROLL)
                fin = np.isfinite(cref)
                rel = float(np.max(np.abs(costs[fin] - cref[fin]) / np.abs(cref[fin])))
                print(f"MATRIX D-fused {vtxt} C={C} H={H} Ts={Ts} cost=diag: err {rel:.2e} bound {bound:.2e} "
                      f"lookback err {float(np.max(np.abs(err - e) / e)):.2e}")


# ----------------------------------------------------------------- E: input_acc bank
@pytest.mark.parametrize("lpm,shape", [(l, S) for l in LPMS] + [(4, UW), (1, UW)], ids=_ids)
def test_e_input_acc_rk4(nat, monkeypatch, lpm, shape):
    """An input_acc bank rolled out (StageK's (k1, k2, k0, k3) = (mass, 0, 0, 0) into FusedK)."""
    run_case(nat, monkeypatch, "E", "rk4", lpm, shape, acc=True)


def test_e_input_acc_rk6(nat, monkeypatch):
    run_case(nat, monkeypatch, "E", "rk6", 1, S, acc=True)


# ----------------------------------------------------------------- F: horizon edges
@pytest.mark.parametrize("shape", [H1, H64], ids=_ids)
@pytest.mark.parametrize("lpm", LPMS)
def test_f_horizon_edges_rk4(nat, monkeypatch, lpm, shape):
    """H = 1 (the terminal step is the only step; near ties down to a 6e-9 relative gap) and
    H = 64 (the longest horizon of the controller record)."""
    run_case(nat, monkeypatch, "F", "rk4", lpm, shape)


@pytest.mark.parametrize("integrator,lpm", [("euler_nlp", 4), ("euler_nlp", 2), ("euler_nlp", 1), ("rk6", 1)])
def test_f_single_step_other_integrators(nat, monkeypatch, integrator, lpm):
    run_case(nat, monkeypatch, "F", integrator, lpm, H1)

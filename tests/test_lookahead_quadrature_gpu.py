"""The plan kernel's LPM-4 look-ahead with the position as a per-step quadrature in quad lanes
2 / 3 (rollout_dev.hpp kRQuadr, dyn.hpp step_fused kPosQuadr): every lane sums vy r and vx r of its
own chain result over the RK4 stages, one swap per step hands lane 2 its X and lane 3 its Y, and
lanes 0 / 1 carry garbage in their position slot that must reach nothing.

Against the oracle (rollout_rk4 + mpc_cost, the raceline reference by constant_speed_from):
  * small shapes N in {1, 5, 17, 65} (a partial quad group, a wave boundary at 16 rollouts, a block
    boundary at 64 models) x H in {1, 2, 20} x C in {1, 3}, diagonal Q with P = 0 and P != 0, the
    shared and the per-model raceline reference; one staged-out shape (C = 64, H = 40);
  * a bank with |D| = 1e300 (the largest chain_static_ok admits): lanes 0 / 1's discarded sums
    overflow, the valid lanes' rollouts are non-finite in the oracle too and are counted;
  * models that leave the fast domain (a standstill start, |C| > 1.9 beside fast quads in one wave,
    a linear-tire bank): the general re-run;
  * a full Q / P: the unsplit path.
Costs: the same NaN / inf pattern and RTOL = 1e-6 on every finite cost; the per-model argmin, the
global argmin and the non-finite count exact.  Exact choices need decided inputs: every case first
asserts, on the oracle's costs alone, that the best and the runner-up of every row it checks differ
by more than 2 RTOL (the smallest gap of the small shapes is 1.7e-5)."""
import os

import numpy as np
import pytest

from conftest import golden
from oracle import llampc_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-6
TS = 0.02
NMAX = 65
NAN_MODEL = 3                                        # a NaN Bf: the model's costs are NaN, counted
R = np.diag([5e-3, 1.0])
QD = np.diag([2.0, 0.5])
COSTS = {"P0": (QD, np.zeros((2, 2))), "Pdiag": (QD, np.diag([3.0, 0.25]))}
UMIN, UMAX = np.array([-0.1, -0.35]), np.array([1.0, 0.35])


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


def shared():
    p = O.orca_params()
    return {k: p[k] for k in ("lf", "lr", "mass", "Iz", "Cm1", "Cm2", "Cr0", "Cr2")}


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_array_equal(np.isposinf(a), np.isposinf(b))
    np.testing.assert_array_equal(np.isneginf(a), np.isneginf(b))
    fin = np.isfinite(b)
    err = float(np.max(np.abs(a[fin] - b[fin]) / np.abs(b[fin]))) if fin.any() else 0.0
    np.testing.assert_allclose(a[fin], b[fin], rtol=rtol, atol=0.0)
    return err


def start():
    """The recorded state 30 and the input before it (on the ETHZ track: the raceline cases)."""
    d = golden("dyn_slice.npz")
    return d["states"][:, 30].copy(), d["inputs"][:, 29].copy(), d["inputs"]


def candidates(C, H):
    """The recorded inputs from step 30; candidate 1 steers +0.04 at 0.05 less pwm, candidate 2
    steers -0.04; further candidates (the staged-out shape) uniform noise of +-0.03."""
    _, _, u = start()
    U = np.repeat(u[:, 30:30 + H].T[None].copy(), C, axis=0)
    if C > 1:
        U[1, :, 1] += 0.04
        U[1, :, 0] -= 0.05
    if C > 2:
        U[2, :, 1] -= 0.04
    if C > 3:
        U[3:] += np.random.RandomState(C + H).uniform(-0.03, 0.03, (C - 3, H, 2))
    return np.clip(U, UMIN, UMAX)


def straight_xref(x0, H):
    v, t = np.hypot(x0[3], x0[4]), np.arange(H + 1) * TS
    return np.vstack([x0[0] + v * np.cos(x0[2]) * t + 0.01, x0[1] + v * np.sin(x0[2]) * t - 0.02])


_BANK, _TRAJ, _TRACK = [], {}, []


def bank():
    """NMAX models, the small shapes take the first N; model NAN_MODEL has a NaN Bf (its friction
    mu_n = (Df + Dr) / (9.81 m) of the raceline reference stays finite)."""
    from llampc.mpc import generate_bank
    if not _BANK:
        p = generate_bank(NMAX, seed=8)
        p[0, NAN_MODEL] = np.nan
        p.setflags(write=False)
        _BANK.append(p)
    return _BANK[0]


def traj_of(C, H):
    """The oracle's rollouts of the NMAX-model bank [H + 1, NMAX C, 6]: once per (C, H)."""
    if (C, H) not in _TRAJ:
        x0, _, _ = start()
        with np.errstate(all="ignore"):
            t = O.rollout_rk4(shared(), tuple(bank()), x0, candidates(C, H), TS)
        t.setflags(write=False)
        _TRAJ[(C, H)] = t
    return _TRAJ[(C, H)]


def track():
    if not _TRACK:
        from llampc.mpc.planner import raceline_start
        from llampc.tracks import ETHZ
        tr = ETHZ('optimal', True)
        td = np.load(os.path.join(os.path.dirname(__file__), "..", "lla-mpc_amd", "llampc", "tracks", "data", "tracks.npz"))
        ref = O.RacelineRef(td["ETHZ_x"], td["ETHZ_y"], td["ETHZ_speeds"], td["ETHZ_mus"])
        s0, _ = raceline_start(start()[0], tr, 0)
        _TRACK.append((tr, ref, float(s0)))
    return _TRACK[0]


def decided(cm, what):
    """cm [rows, K] oracle costs, NaN as +inf: the best and the runner-up of every row that has a
    finite best differ by more than 2 RTOL (an input condition: it never sees the device)."""
    if cm.shape[1] < 2:
        return
    srt = np.sort(cm, axis=1)
    fin = np.isfinite(srt[:, 0])
    gap = (srt[fin, 1] - srt[fin, 0]) / np.abs(srt[fin, 0])
    assert np.all(gap > 2 * RTOL), f"{what}: near tie in the oracle ({gap.min():.2e}): choose other inputs"


def force_quad(nat, monkeypatch, N, C, H, staged=True):
    monkeypatch.setenv("LLAMPC_LPM", "4")
    v = nat.plan_variant(N, C, H, "rk4")
    assert (v["lpm"], bool(v["stage"])) == (4, staged), v


def check_lookahead(nat, p, x0, U, xref, uprev, Q, P, cref, approx=False):
    """One look-ahead launch (costs, per-model argmin, global argmin) and one plan tick without the
    look-back (the record's non-finite count and global best) against cref [N, C]."""
    from llampc.mpc import ModelBank, plan
    N, C = cref.shape
    cm = np.where(np.isnan(cref), np.inf, cref)
    decided(cm, "per-model argmin")
    decided(cm.reshape(1, -1), "global argmin")
    cs = nat.cost_struct(Q=Q, R=R, P=P)
    with ModelBank(p, device=0, approx=approx) as b:
        r = b.lookahead(x0, U, xref, uprev, Ts=TS, cost=cs, return_costs=True, return_best_cand=True)
        res = plan(b, x0, uprev, x0, xref, U, uprev=uprev, Ts=TS, do_lookback=False, cost=cs, return_costs=True)
    err = close(r["costs"], cref)
    close(res.costs, cref)
    np.testing.assert_array_equal(r["best_cand_per_model"], np.argmin(cm, axis=1))
    j = int(np.argmin(cm.ravel()))
    assert r["best_model"] * C + r["best_cand"] == j
    assert res.global_best[0] * C + res.global_best[1] == j
    assert res.n_nonfinite == int(np.count_nonzero(~np.isfinite(cref)))
    return err


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H", [1, 2, 20])
@pytest.mark.parametrize("N", [1, 5, 17, 65])
def test_small_shapes_shared_reference(nat, monkeypatch, N, H, C):
    """Diagonal Q with P = 0 and P != 0 on the shared reference sx[2 (k + 1) + pc], staged."""
    force_quad(nat, monkeypatch, N, C, H)
    x0, uprev, _ = start()
    U, xref = candidates(C, H), straight_xref(x0, H)
    tr = traj_of(C, H)[:, :N * C]
    for name, (Q, P) in COSTS.items():
        cref = O.mpc_cost(tr, U, xref, uprev, Q, R, P).reshape(N, C)
        err = check_lookahead(nat, bank()[:, :N], x0, U, xref, uprev, Q, P, cref)
        print(f"QUADR shared N={N} H={H} C={C} {name}: err {err:.2e}")


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H", [1, 2, 20])
@pytest.mark.parametrize("N", [1, 5, 17, 65])
def test_small_shapes_raceline_reference(nat, monkeypatch, N, H, C):
    """The per-model reference xpm[2 k + pc] (xref_mode RACELINE): costs, the global argmin, the
    non-finite count and the record's candidate of the selected model (the tick has no per-model
    argmin output on this route: the last model, in the ragged group, is selected)."""
    from llampc.mpc import ModelBank, plan
    force_quad(nat, monkeypatch, N, C, H)
    x0, uprev, _ = start()
    U = candidates(C, H)
    trk, ref, s0 = track()
    p = bank()[:, :N]
    mu = (p[2] + p[5]) / (9.81 * O.orca_params()["mass"])
    tr = traj_of(C, H)
    xr = [O.constant_speed_from(s0, x0[:2], float(x0[3]), ref, H, TS, 0.9, mu[n])[0] for n in range(N)]
    for name, (Q, P) in COSTS.items():
        cref = np.stack([O.mpc_cost(tr[:, n * C:(n + 1) * C], U, xr[n], uprev, Q, R, P) for n in range(N)])
        cm = np.where(np.isnan(cref), np.inf, cref)
        decided(cm, "per-model argmin")
        decided(cm.reshape(1, -1), "global argmin")
        with ModelBank(p, device=0) as b:
            b.set_raceline(trk)
            res = plan(b, x0, uprev, x0, None, U, uprev=uprev, Ts=TS, do_lookback=False, current_model=N - 1,
                       cost=nat.cost_struct(Q=Q, R=R, P=P), return_costs=True, raceline_start=(s0, float(x0[3]), 0.9))
        err = close(res.costs, cref)
        assert res.global_best[0] * C + res.global_best[1] == int(np.argmin(cm.ravel()))
        assert res.best_model == N - 1 and res.best_cand == int(np.argmin(cm[N - 1]))
        assert res.n_nonfinite == int(np.count_nonzero(~np.isfinite(cref)))
        print(f"QUADR raceline N={N} H={H} C={C} {name}: err {err:.2e}")


def test_staged_out_shape(nat, monkeypatch):
    """C = 64, H = 40: the candidates are read from U itself (no staged record), 4 lanes forced."""
    N, C, H = 5, 64, 40
    force_quad(nat, monkeypatch, N, C, H, staged=False)
    x0, uprev, _ = start()
    U, xref = candidates(C, H), straight_xref(x0, H)
    Q, P = COSTS["Pdiag"]
    cref = O.mpc_cost(traj_of(C, H)[:, :N * C], U, xref, uprev, Q, R, P).reshape(N, C)
    err = check_lookahead(nat, bank()[:, :N], x0, U, xref, uprev, Q, P, cref)
    print(f"QUADR unstaged N={N} H={H} C={C}: err {err:.2e}")


HUGE = {1: (2, 1e300), 6: (5, 1e300), 10: (2, -1e300), 11: (5, -1e300), 16: (2, 1e300)}   # model: (row, D)


@pytest.mark.parametrize("H", [1, 20])
def test_enormous_d_does_not_leak(nat, monkeypatch, H):
    """|Df| or |Dr| = 1e300 in five of 17 models, beside ordinary models in the same quads' waves:
    lanes 0 / 1 of those quads sum vy F with F ~ 1e300 (inf, NaN) into their position slot.  The
    oracle's own costs of those models are non-finite (asserted first, on the CPU) and the others'
    finite: the device must return that pattern, the finite costs, the choices and the count."""
    from llampc.mpc import generate_bank
    N, C = 17, 3
    force_quad(nat, monkeypatch, N, C, H)
    p = generate_bank(N, seed=8)
    for n, (row, D) in HUGE.items():
        p[row, n] = D
    x0, uprev, _ = start()
    U, xref = candidates(C, H), straight_xref(x0, H)
    Q, P = COSTS["Pdiag"]
    with np.errstate(all="ignore"):
        cref = O.mpc_cost(O.rollout_rk4(shared(), tuple(p), x0, U, TS), U, xref, uprev, Q, R, P).reshape(N, C)
    huge = np.zeros(N, dtype=bool)
    huge[list(HUGE)] = True
    assert not np.isfinite(cref[huge]).any() and np.isfinite(cref[~huge]).all()
    err = check_lookahead(nat, p, x0, U, xref, uprev, Q, P, cref)
    print(f"QUADR huge D H={H}: err {err:.2e}, non-finite {int((~np.isfinite(cref)).sum())}")


@pytest.mark.parametrize("case", ["standstill", "mixed_C", "linear_tires"])
def test_leaving_the_fast_domain_reruns_general_path(nat, monkeypatch, case):
    """A standstill start (0/0 in the slip angles: every rollout re-runs), Cf = 2.6 in every fifth
    model (their quads re-run beside fast quads of the same wave) and a linear-tire bank."""
    from llampc.mpc import generate_bank
    N, C, H = 17, 3, 20
    force_quad(nat, monkeypatch, N, C, H)
    p = generate_bank(N, seed=8)
    x0, uprev, _ = start()
    if case == "standstill":
        x0 = np.array([x0[0], x0[1], 0.4, 0.0, 0.0, 0.0])
    elif case == "mixed_C":
        p[1, 2::5] = 2.6
    U, xref = candidates(C, H), straight_xref(x0, H)
    Q, P = COSTS["Pdiag"]
    approx = case == "linear_tires"
    with np.errstate(all="ignore"):
        cref = O.mpc_cost(O.rollout_rk4(shared(), tuple(p), x0, U, TS, approx=approx), U, xref, uprev, Q, R,
                          P).reshape(N, C)
    assert np.isfinite(cref).all()
    err = check_lookahead(nat, p, x0, U, xref, uprev, Q, P, cref, approx=approx)
    print(f"QUADR {case}: err {err:.2e}")


def test_full_q_takes_the_unsplit_path(nat, monkeypatch):
    """Off-diagonal Q and P: every lane integrates both components (no quadrature)."""
    N, C, H = 17, 3, 20
    force_quad(nat, monkeypatch, N, C, H)
    x0, uprev, _ = start()
    U, xref = candidates(C, H), straight_xref(x0, H)
    Q, P = np.array([[1.0, 0.3], [0.2, 2.0]]), np.array([[0.5, -0.1], [0.4, 1.0]])
    cref = O.mpc_cost(traj_of(C, H)[:, :N * C], U, xref, uprev, Q, R, P).reshape(N, C)
    err = check_lookahead(nat, bank()[:, :N], x0, U, xref, uprev, Q, P, cref)
    print(f"QUADR full Q: err {err:.2e}")

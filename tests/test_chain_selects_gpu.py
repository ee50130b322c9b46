"""The look-ahead tire chain's atan cores after the select work (csrc/fastmath.hpp): the octant
fix-up as one high-word select and an FMA (octant_fix: atan2_fast and the two-way atan_fast, precise
and lean) and the lean atan in three zones (atan_zones: the fused look-ahead stages).

  1. the raw cores (llampc_math_batch fn 4 / 5 precise, 10 / 11 lean) at the zone edges and the
     octant boundaries against NumPy;
  2. look-ahead rollouts at the smallest shapes that can go wrong, on a bank whose B spans two
     decades so that every zone is taken (test_chain_zones_cpu.py holds the bank to that on the
     oracle alone), against the oracle;
  3. the extremes: |B| = 1e300 and |D| = 1e300 (the largest chain_static_ok admits), fast path and
     general re-run;
  4. the look-back (precise cores, one lane per model: it keeps the select form of the fix-up, and
     in any form its values must not move).

What the raw cores are asked at arguments outside their stated domains (fastmath.hpp): the lean
atan takes every argument — +-inf gives +-pi/2 and NaN gives NaN, asserted.  The precise atan
(|z| <= 2^1000) and both atan2 (2^-1000 <= |y| + x <= 2^1000) keep their two-way min / max form, in
which v_min / v_max drop a NaN operand (atan_fast(NaN) = +-pi/4) and an infinite divisor gives NaN
where NumPy has +-pi/2: their callers judge the domain and re-run (dyn.hpp Dom), so these three are
held to NumPy on their domains only, and NaN-in / NaN-out is asserted where the rollouts rely on
it — at the look-ahead's costs (a NaN model, case 2)."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":                                 # the parent-library child of case 4
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import chain_zones as Z
from conftest import assert_costs_close, core_error_bound
from oracle import llampc_oracle as O

pytestmark = pytest.mark.gpu

RTOL_ROLL = 1e-7                     # the suite's rollout tolerance (test_configs_gpu.py)
RTOL_STEP = 1e-9                     # one integration step: the look-back
LEAN_ULP, PRECISE_ULP = 2.0 ** 16, 4.0
R = np.diag([5e-3, 1.0])
QD = np.diag([2.0, 0.5])
COSTS = {"P0": (QD, np.zeros((2, 2))), "Pdiag": (QD, np.diag([3.0, 0.25])),
         "full": (np.array([[1.0, 0.3], [0.2, 2.0]]), np.array([[0.5, -0.1], [0.4, 1.0]]))}
NAN_MODEL = 2                        # a NaN Bf: its costs are NaN in the oracle and on the device


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


def _math(nat, fn, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    out = np.empty_like(a)
    nat.check(nat.load().llampc_math_batch(fn, a.ctypes.data, None if bb is None else bb.ctypes.data, a.size,
                                           out.ctypes.data, 0))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------ 1. the cores
@pytest.mark.parametrize("fn,bound", [(11, LEAN_ULP), (5, PRECISE_ULP)], ids=["lean", "precise"])
def test_atan_cores_at_the_zone_edges(nat, fn, bound):
    """0, +-tiny, +-2^1000, tan(pi/8), 1 and 1 + sqrt(2) with their neighbours, both signs: within
    the core's bound of NumPy, zeros with their sign, atan(-z) == -atan(z) bitwise.  Lean: +-inf
    gives +-pi/2 exactly and NaN gives NaN (the module docstring has the precise core's domain)."""
    z = Z.atan_edges(nonfinite=False)
    got, want = _math(nat, fn, z), np.arctan(z)
    u = Z.ulp_err(got, want)
    print(f"CHAIN atan fn {fn}: {u:.1f} ulp at the edges")
    assert np.isfinite(got).all() and u <= bound
    np.testing.assert_array_equal(_bits(got[z == 0]), _bits(z[z == 0]))
    np.testing.assert_array_equal(_bits(_math(nat, fn, -z)), _bits(-got))
    if fn == 11:
        nf = np.array([np.inf, -np.inf, np.nan])
        g = _math(nat, fn, nf)
        np.testing.assert_array_equal(_bits(g[:2]), _bits(np.array([Z.PIO2, -Z.PIO2])))
        assert np.isnan(g[2])
        big = np.array([2.0 ** 1001, -2.0 ** 1001, 1.7e308, -1.7e308])     # beyond the clamp
        np.testing.assert_array_equal(_bits(_math(nat, fn, big)), _bits(np.arctan(big)))


@pytest.mark.parametrize("fn,bound", [(10, LEAN_ULP), (4, PRECISE_ULP)], ids=["lean", "precise"])
def test_atan2_cores_at_the_octant_boundaries(nat, fn, bound):
    """Every octant boundary of the reduction in both signs of y (chain_zones.atan2_edges): within
    the core's bound of NumPy, signed zeros kept, atan2(-y, x) == -atan2(y, x) bitwise."""
    y, x = Z.atan2_edges()
    got, want = _math(nat, fn, y, x), np.arctan2(y, x)
    u = Z.ulp_err(got, want)
    print(f"CHAIN atan2 fn {fn}: {u:.1f} ulp at the octant boundaries")
    assert np.isfinite(got).all() and u <= bound
    np.testing.assert_array_equal(_bits(got[y == 0]), _bits(want[y == 0]))
    np.testing.assert_array_equal(_bits(_math(nat, fn, -y, x)), _bits(-got))


def test_lean_atan_across_the_zones(nat):
    """2^17 arguments over +-4 and a Cauchy tail: the three-zone lean atan within its bound of
    NumPy on every zone (measured 734 / 738 / 186 ulp in zones I / II / III: the 8-term fit's
    1.1e-13, as the two-way form's 744), and odd bitwise."""
    rng = np.random.RandomState(7)
    z = np.concatenate([rng.uniform(-4, 4, 1 << 16), rng.standard_cauchy(1 << 16) * 3])
    got, want = _math(nat, 11, z), np.arctan(z)
    az = np.abs(z)
    for name, m in (("I", az <= Z.TP8), ("II", (az > Z.TP8) & (az <= Z.CTP8)), ("III", az > Z.CTP8)):
        u = Z.ulp_err(got[m], want[m])
        print(f"CHAIN lean atan zone {name}: {u:.1f} ulp over {int(m.sum())} arguments")
        assert m.sum() > 1000 and u <= LEAN_ULP
    np.testing.assert_array_equal(_bits(_math(nat, 11, -z)), _bits(-got))


# --------------------------------------------------------------------------- 2. the rollouts
_TRAJ = {}


def bank(n):
    p = Z.zone_bank(n)
    if n > NAN_MODEL:
        p[0, NAN_MODEL] = np.nan
    return p


def traj_of(C, H):
    """The oracle's rollouts of the NMAX-model zone bank [H + 1, NMAX C, 6]: once per (C, H)."""
    if (C, H) not in _TRAJ:
        x0, _, _ = Z.start()
        with np.errstate(all="ignore"):
            t = O.rollout_rk4(Z.shared(), tuple(bank(Z.NMAX)), x0, Z.candidates(C, H), Z.TS)
        t.setflags(write=False)
        _TRAJ[(C, H)] = t
    return _TRAJ[(C, H)]


def decided(cm, what):
    """The best and the runner-up of every row with a finite best differ by more than 2 RTOL_ROLL
    in the oracle (an input condition; the zone bank's smallest gap is 9e-5)."""
    if cm.shape[1] < 2:
        return
    srt = np.sort(cm, axis=1)
    fin = np.isfinite(srt[:, 0])
    gap = (srt[fin, 1] - srt[fin, 0]) / np.abs(srt[fin, 0])
    assert np.all(gap > 2 * RTOL_ROLL), f"{what}: near tie in the oracle ({gap.min():.2e}): choose other inputs"


def check_lookahead(nat, p, x0, U, xref, uprev, Q, P, cref):
    """One look-ahead launch and one plan tick without the look-back against cref [N, C]: costs by
    conftest.assert_costs_close, per-model and global argmin and the non-finite count exact."""
    from llampc.mpc import ModelBank, plan
    N, C = cref.shape
    cm = np.where(np.isnan(cref), np.inf, cref)
    decided(cm, "per-model argmin")
    decided(cm.reshape(1, -1), "global argmin")
    cs = nat.cost_struct(Q=Q, R=R, P=P)
    with ModelBank(p, device=0) as b:
        r = b.lookahead(x0, U, xref, uprev, Ts=Z.TS, cost=cs, return_costs=True, return_best_cand=True)
        res = plan(b, x0, uprev, x0, xref, U, uprev=uprev, Ts=Z.TS, do_lookback=False, cost=cs, return_costs=True)

    def bound(idx):
        return core_error_bound(Z.shared(), tuple(p), x0, U, xref, uprev, Q, R, P, Ts=Z.TS)[idx]

    fin = np.isfinite(cref)
    err = float(np.max(np.abs(r["costs"][fin] - cref[fin]) / np.abs(cref[fin]))) if fin.any() else 0.0
    n_bound = assert_costs_close(r["costs"], cref, RTOL_ROLL, bound)
    assert_costs_close(res.costs, cref, RTOL_ROLL, bound)
    np.testing.assert_array_equal(r["best_cand_per_model"], np.argmin(cm, axis=1))
    j = int(np.argmin(cm.ravel()))
    assert r["best_model"] * C + r["best_cand"] == j
    assert res.global_best[0] * C + res.global_best[1] == j
    assert res.n_nonfinite == int(np.count_nonzero(~np.isfinite(cref)))
    return err, n_bound


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H", [1, 2, 20])
@pytest.mark.parametrize("N", [1, 3, 17, 65])
def test_rollouts_small_shapes_every_zone(nat, monkeypatch, N, H, C):
    """The quad (LPM 4) on the zone bank: N = 1, 3 (a partial quad row), 17 (a partial wave), 65
    (two blocks, the second partial) x H x C; diagonal Q with P = 0 and P != 0 (the position
    quadrature) and a full Q / P (the unsplit path).  Model 2 has a NaN Bf: NaN costs, counted."""
    monkeypatch.setenv("LLAMPC_LPM", "4")
    assert nat.plan_variant(N, C, H, "rk4")["lpm"] == 4
    x0, uprev, _ = Z.start()
    U, xref = Z.candidates(C, H), Z.straight_xref(x0, H)
    tr = traj_of(C, H)[:, :N * C]
    for name, (Q, P) in COSTS.items():
        cref = O.mpc_cost(tr, U, xref, uprev, Q, R, P).reshape(N, C)
        err, nb = check_lookahead(nat, bank(N), x0, U, xref, uprev, Q, P, cref)
        print(f"CHAIN zones N={N} H={H} C={C} {name}: err {err:.2e}, {nb} pairs by their core-error bound")


@pytest.mark.parametrize("lpm", ["1", "2"])
def test_rollouts_other_lane_splits_every_zone(nat, monkeypatch, lpm):
    """The same bank with one and two lanes per rollout (chain_fast with the lean cores)."""
    N, C, H = 65, 3, 20
    monkeypatch.setenv("LLAMPC_LPM", lpm)
    assert nat.plan_variant(N, C, H, "rk4")["lpm"] == int(lpm)
    x0, uprev, _ = Z.start()
    U, xref = Z.candidates(C, H), Z.straight_xref(x0, H)
    Q, P = COSTS["Pdiag"]
    cref = O.mpc_cost(traj_of(C, H), U, xref, uprev, Q, R, P).reshape(N, C)
    err, nb = check_lookahead(nat, bank(N), x0, U, xref, uprev, Q, P, cref)
    print(f"CHAIN zones lpm={lpm}: err {err:.2e}, {nb} pairs by their core-error bound")


# --------------------------------------------------------------------------- 3. the extremes
HUGE_B = {1: (0, 1e300), 6: (3, 1e300), 10: (0, -1e300), 11: (3, -1e300), 16: (0, 1e300)}   # model: (row, B)
HUGE_D = {1: (2, 1e300), 6: (5, 1e300), 10: (2, -1e300), 11: (5, -1e300), 16: (2, 1e300)}   # model: (row, D)


@pytest.mark.parametrize("path", ["fast", "general"])
@pytest.mark.parametrize("H", [1, 20])
@pytest.mark.parametrize("what", ["B", "D"])
def test_extreme_b_and_d(nat, monkeypatch, what, H, path):
    """|Bf| or |Br| = 1e300 in five of 17 models: |B slip| is ~1e298 or more, far in zone III, the
    tire force D sin(+-C pi/2) — finite costs in the oracle (asserted first) and on the fast path,
    well-conditioned (a one-ulp change of x0 moves them by 2e-14).  |D| = 1e300: the oracle's costs of
    those models are non-finite, the device must return that pattern and count it.  path =
    "general": Cf = 2.6 in the same five models and two ordinary ones, outside sin_wide's range, so
    their quads are re-run with the general evaluation beside fast quads of the same wave; it must
    agree with the oracle in the same way."""
    from llampc.mpc import generate_bank
    N, C = 17, 3
    monkeypatch.setenv("LLAMPC_LPM", "4")
    p = generate_bank(N, seed=8)
    for n, (row, v) in (HUGE_B if what == "B" else HUGE_D).items():
        p[row, n] = v
    if path == "general":
        p[1, list(HUGE_B) + [3, 12]] = 2.6
    x0, uprev, _ = Z.start()
    U, xref = Z.candidates(C, H), Z.straight_xref(x0, H)
    Q, P = COSTS["Pdiag"]
    with np.errstate(all="ignore"):
        cref = O.mpc_cost(O.rollout_rk4(Z.shared(), tuple(p), x0, U, Z.TS), U, xref, uprev, Q, R, P).reshape(N, C)
    huge = np.zeros(N, dtype=bool)
    huge[list(HUGE_B)] = True
    assert np.isfinite(cref[~huge]).all()
    assert np.isfinite(cref[huge]).all() if what == "B" else not np.isfinite(cref[huge]).any()
    err, nb = check_lookahead(nat, p, x0, U, xref, uprev, Q, P, cref)
    print(f"CHAIN huge {what} H={H} {path}: err {err:.2e}, {nb} pairs by their core-error bound, "
          f"non-finite {int((~np.isfinite(cref)).sum())}")


# ---------------------------------------------------------------------------- 4. the look-back
LB_N, LB_W, LB_K = 257, 10, 10


def lookback_tick():
    """W + 1 look-back ticks on the recorded states at N = 257 (four blocks and one model): the
    top-K indices, the selected model and the full error window [N, W]."""
    from conftest import golden
    from llampc.mpc import ModelBank, generate_bank
    d = golden("dyn_slice.npz")
    s, u = d["states"], d["inputs"]
    p = generate_bank(LB_N, seed=4)
    with ModelBank(p, W=LB_W, device=0) as b:
        for t in range(1, LB_W + 2):
            r = b.lookback(s[:, t - 1], u[:, t - 1], s[:, t], Ts=Z.TS, K=LB_K)
        win = b.window()
    return p, s, u, np.asarray(r["topk"], dtype=np.int64), int(r["best"]), win


def test_lookback_untouched(nat, tmp_path):
    """The look-back evaluates the precise cores (fastmath.hpp octant_fix: either form of the
    fix-up has the same bits): a full window at N = 257.  With LLAMPC_PARENT_LIB naming a build of the parent commit, the top-K
    indices and the error window are bitwise those of that library (run in a fresh process, one
    library per process).  Without it: the window against the oracle at the suite's one-step
    tolerance 1e-9, indices exact."""
    p, s, u, topk, best, win = lookback_tick()
    parent = os.environ.get("LLAMPC_PARENT_LIB")
    if parent and os.path.exists(parent):
        out = str(tmp_path / "parent.npz")
        env = dict(os.environ, LLAMPC_HIP_LIB=parent)
        subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=env, timeout=120)
        ref = np.load(out)
        np.testing.assert_array_equal(topk, ref["topk"])
        assert best == int(ref["best"])
        np.testing.assert_array_equal(_bits(win), _bits(ref["win"]))
        print("CHAIN look-back: bitwise equal to the parent library")
        return
    ow = O.LookbackWindow(LB_N, LB_W, LB_K)
    cols = []
    for t in range(1, LB_W + 2):
        e = O.lookback_errors(O.evaluate_models_vectorized(Z.shared(), tuple(p), s[:, t - 1], u[:, t - 1], Z.TS), s[:, t])
        ow.push(e)
        cols.append(e)
    want = np.stack(cols[-LB_W:], axis=1)
    np.testing.assert_allclose(win, want, rtol=RTOL_STEP, atol=0.0)
    np.testing.assert_array_equal(topk, ow.best_k)
    assert best == ow.current
    print(f"CHAIN look-back: window within {float(np.max(np.abs(win - want) / np.abs(want))):.2e} of the oracle")


if __name__ == "__main__":
    _, _, _, topk_, best_, win_ = lookback_tick()
    np.savez(sys.argv[1], topk=topk_, best=best_, win=win_)

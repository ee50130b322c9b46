"""The fused look-ahead quad's yaw fold after round 10 (csrc/dyn.hpp chain_fold<SCALED>,
rollout_dev.hpp rollout): quad lane 3 carries the scaled yaw Psi + 1, so its fold is lane 2's and its
sine is cos psi; the sign flip is one shift-add on the high word; B fw is a per-rollout constant; the
rear lane's chain returns (h/m) Fry.

Against the oracle (rollout_rk4 + mpc_cost; LLAMPC.tick against ControllerOracle), costs through
conftest.assert_costs_close with core_error_bound at test_chain_selects_gpu.py's RTOL_ROLL; per-model
argmin, global argmin and the non-finite count exact:
  * N in {1, 5, 17, 65} x H in {1, 2, 20} x C in {1, 3} on the zone bank (shared reference rollouts),
    diagonal Q with P = 0 and P != 0 (the quadrature) and a full Q / P (the unsplit path: its lanes
    hold both position components, lane 3's offset yaw reaches its own fold only);
  * start yaws on the fold's edges — 0, +-pi/2, +-pi, +-3 pi/2, each also one ulp and 1e-9 to either
    side: the parity of k flips there and Psi = an odd integer is a tie of the rounding — +-1e5,
    just beyond the fold's range (the general re-run), NaN and +-inf.  The start state is one per
    launch, so the quads of a wave share the yaw and differ in their models;
  * a spinning start, |omega0| = 140 rad/s: 2.8 rad of yaw per step, the stage yaws of one step cross
    one or two quadrant boundaries (the oracle's costs are asserted finite first);
  * a linear-tire bank and |C| > 1.9 in every fifth model: general re-runs beside fast quads;
  * the controller's quad rollouts (kRSplit with kRS4) from psi0 = pi/2 - 1e-9;
  * the look-back's window, bit for bit the parent library's where LLAMPC_PARENT_LIB names one."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_zones as Z
import ctl_matrix as M
import test_chain_selects_gpu as CS
from oracle import llampc_oracle as O
from test_chain_selects_gpu import COSTS, R, RTOL_ROLL, check_lookahead

pytestmark = pytest.mark.gpu

PIO2 = Z.PIO2
N_YAW, C_YAW, H_YAW = 17, 3, 20
# the fold's range in the units it is compared in: |Psi| = |psi| 2/pi <= 2^20 pi/2 (dyn.hpp Dom, kSinCosMax)
PSI_RANGE = 2.0 ** 20 * PIO2 * PIO2
YAW_BASES = {"0": 0.0, "+pi/2": PIO2, "-pi/2": -PIO2, "+pi": 2 * PIO2, "-pi": -2 * PIO2, "+3pi/2": 3 * PIO2,
             "-3pi/2": -3 * PIO2}


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


def around(v):
    """v, its two neighbours and v -+ 1e-9."""
    return [v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf), v - 1e-9, v + 1e-9]


def force_quad(nat, monkeypatch, N, C, H):
    monkeypatch.setenv("LLAMPC_LPM", "4")
    assert nat.plan_variant(N, C, H, "rk4")["lpm"] == 4


def yaw_case(psi0, p=None, approx=False, omega0=None):
    """(p, x0, uprev, U, xref, cref [N, C]) of the N_YAW-model launch from the recorded state with yaw
    psi0 (and yaw rate omega0): the reference runs straight on along the new heading."""
    p = Z.zone_bank(N_YAW) if p is None else p
    x0, uprev, _ = Z.start()
    x0[2] = psi0
    if omega0 is not None:
        x0[5] = omega0
    U = Z.candidates(C_YAW, H_YAW)
    Q, P = COSTS["Pdiag"]
    with np.errstate(all="ignore"):
        xref = Z.straight_xref(x0, H_YAW)
        cref = O.mpc_cost(O.rollout_rk4(Z.shared(), tuple(p), x0, U, Z.TS, approx=approx), U, xref, uprev, Q, R,
                          P).reshape(N_YAW, C_YAW)
    return p, x0, uprev, U, xref, cref


# ------------------------------------------------------------------------------- the shapes
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H", [1, 2, 20])
@pytest.mark.parametrize("N", [1, 5, 17, 65])
def test_small_shapes(nat, monkeypatch, N, H, C):
    """N = 1, 5 (a partial quad row), 17 (a partial wave), 65 (two blocks) x H x C on the zone bank
    (model 2 has a NaN Bf) with the three cost settings; the reference rollouts are
    test_chain_selects_gpu.py's, computed once per (C, H)."""
    force_quad(nat, monkeypatch, N, C, H)
    x0, uprev, _ = Z.start()
    U, xref = Z.candidates(C, H), Z.straight_xref(x0, H)
    tr = CS.traj_of(C, H)[:, :N * C]
    for name, (Q, P) in COSTS.items():
        cref = O.mpc_cost(tr, U, xref, uprev, Q, R, P).reshape(N, C)
        err, nb = check_lookahead(nat, CS.bank(N), x0, U, xref, uprev, Q, P, cref)
        print(f"YAWFOLD N={N} H={H} C={C} {name}: err {err:.2e}, {nb} pairs by their core-error bound")


# ---------------------------------------------------------------------------- the start yaws
@pytest.mark.parametrize("base", list(YAW_BASES), ids=list(YAW_BASES))
def test_start_yaw_on_a_fold_edge(nat, monkeypatch, base):
    """psi0 a multiple of pi/2, its neighbours and +-1e-9 (five launches): across the value Psi is to
    either side of an integer — an odd one is the tie of the nearest-even rounding and flips the
    parity of k, an even one changes the sign of the residue — and lane 3's Psi + 1 crosses the
    other kind at the same time."""
    force_quad(nat, monkeypatch, N_YAW, C_YAW, H_YAW)
    Q, P = COSTS["Pdiag"]
    for psi0 in around(YAW_BASES[base]):
        p, x0, uprev, U, xref, cref = yaw_case(psi0)
        assert np.isfinite(cref).all()
        err, nb = check_lookahead(nat, p, x0, U, xref, uprev, Q, P, cref)
        print(f"YAWFOLD psi0 = {base} {psi0 - YAW_BASES[base]:+.3e}: err {err:.2e}, {nb} pairs by their core-error bound")


@pytest.mark.parametrize("psi0", [1e5, -1e5, PSI_RANGE * (1 + 1e-9), -PSI_RANGE * (1 + 1e-9)],
                         ids=["+1e5", "-1e5", "+beyond", "-beyond"])
def test_start_yaw_far_out(nat, monkeypatch, psi0):
    """+-1e5 rad is inside the fold's range (Psi = 6.4e4: the offset lane's Psi + 1 rounds at 7e-12);
    just beyond 2^20 pi/2 in the compared units Dom::ok fails in every lane and the quads re-run in
    the general evaluation from x0 — the same costs against the oracle either way."""
    force_quad(nat, monkeypatch, N_YAW, C_YAW, H_YAW)
    Q, P = COSTS["Pdiag"]
    p, x0, uprev, U, xref, cref = yaw_case(psi0)
    assert np.isfinite(cref).all()
    err, nb = check_lookahead(nat, p, x0, U, xref, uprev, Q, P, cref)
    print(f"YAWFOLD psi0 = {psi0:.6e}: err {err:.2e}, {nb} pairs by their core-error bound")


@pytest.mark.parametrize("psi0", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_start_yaw_not_finite(nat, monkeypatch, psi0):
    """A NaN or infinite yaw: every cost is NaN in the oracle (asserted first) and on the device, in
    the look-ahead's costs and the plan tick's, and all N C of them are counted."""
    from llampc.mpc import ModelBank, plan
    force_quad(nat, monkeypatch, N_YAW, C_YAW, H_YAW)
    Q, P = COSTS["Pdiag"]
    p, x0, uprev, U, xref, cref = yaw_case(psi0)
    assert np.isnan(cref).all()
    cs = nat.cost_struct(Q=Q, R=R, P=P)
    with ModelBank(p, device=0) as b:
        r = b.lookahead(x0, U, xref, uprev, Ts=Z.TS, cost=cs, return_costs=True, return_best_cand=True)
        res = plan(b, x0, uprev, x0, xref, U, uprev=uprev, Ts=Z.TS, do_lookback=False, cost=cs, return_costs=True)
    assert np.isnan(np.asarray(r["costs"])).all() and np.isnan(np.asarray(res.costs)).all()
    assert res.n_nonfinite == N_YAW * C_YAW


# ----------------------------------------------------------------------- the spinning start
@pytest.mark.parametrize("omega0", [140.0, -140.0], ids=["+140", "-140"])
def test_spinning_start(nat, monkeypatch, omega0):
    """|omega0| = 140 rad/s, the order of the 164 rad/s the seeded banks' rollouts reach: 2.8
    rad of yaw per step and 1.4 rad between stage yaws, so k moves by one or two within a step in
    lanes 2 and 3.  (From this start the oracle's explicit RK4 itself overflows at +-164 rad/s in one
    to sixteen of the 17 models; at +-140 every cost is finite and a one-ulp change of x0 moves none
    by more than 1.5e-15, conftest.cost_sensitivity.)"""
    force_quad(nat, monkeypatch, N_YAW, C_YAW, H_YAW)
    Q, P = COSTS["Pdiag"]
    p, x0, uprev, U, xref, cref = yaw_case(0.3, omega0=omega0)
    assert np.isfinite(cref).all(), "the spinning start's reference costs must be numbers"
    err, nb = check_lookahead(nat, p, x0, U, xref, uprev, Q, P, cref)
    print(f"YAWFOLD omega0 = {omega0:+.0f}: err {err:.2e}, {nb} pairs by their core-error bound")


# --------------------------------------------------------------------- the general re-run
@pytest.mark.parametrize("case", ["mixed_C", "linear_tires"])
def test_general_path_beside_fast_quads(nat, monkeypatch, case):
    """Cf = 2.6 in every fifth model (outside sin_wide's range: their quads re-run from x0 beside
    fast quads of the same wave, whose lane 3 ran on Psi + 1) and a linear-tire bank (every quad
    re-runs), from psi0 = pi/2 - 1e-9."""
    from llampc.mpc import ModelBank, generate_bank, plan
    force_quad(nat, monkeypatch, N_YAW, C_YAW, H_YAW)
    p = generate_bank(N_YAW, seed=8)
    if case == "mixed_C":
        p[1, 2::5] = 2.6
    approx = case == "linear_tires"
    Q, P = COSTS["Pdiag"]
    p, x0, uprev, U, xref, cref = yaw_case(PIO2 - 1e-9, p=p, approx=approx)
    assert np.isfinite(cref).all()
    if not approx:
        err, nb = check_lookahead(nat, p, x0, U, xref, uprev, Q, P, cref)
    else:                               # check_lookahead's banks are Pacejka banks
        from conftest import assert_costs_close, core_error_bound
        cm = cref
        CS.decided(cm, "per-model argmin")
        CS.decided(cm.reshape(1, -1), "global argmin")
        cs = nat.cost_struct(Q=Q, R=R, P=P)
        with ModelBank(p, device=0, approx=True) as b:
            r = b.lookahead(x0, U, xref, uprev, Ts=Z.TS, cost=cs, return_costs=True, return_best_cand=True)
            res = plan(b, x0, uprev, x0, xref, U, uprev=uprev, Ts=Z.TS, do_lookback=False, cost=cs, return_costs=True)

        def bound(idx):                 # the linear tires evaluate no lean core: no allowance beyond RTOL_ROLL
            return np.zeros(len(idx))

        err = float(np.max(np.abs(r["costs"] - cref) / np.abs(cref)))
        nb = assert_costs_close(r["costs"], cref, RTOL_ROLL, bound)
        assert_costs_close(res.costs, cref, RTOL_ROLL, bound)
        np.testing.assert_array_equal(r["best_cand_per_model"], np.argmin(cm, axis=1))
        j = int(np.argmin(cm.ravel()))
        assert r["best_model"] * C_YAW + r["best_cand"] == j
        assert res.global_best[0] * C_YAW + res.global_best[1] == j
        assert res.n_nonfinite == 0
    print(f"YAWFOLD {case}: err {err:.2e}, {nb} pairs by their core-error bound")


# ------------------------------------------------------------------------------ the controller
def test_controller_quad_rollouts(nat, monkeypatch):
    """LLAMPC.tick in device mode at the controller matrix's smallest shape (N = C = H = K = W = 1,
    ctl_kernel<4>) from psi0 = pi/2 - 1e-9, five ticks in closed loop against ControllerOracle
    (ctl_matrix.check_tick: the whole record per tick)."""
    monkeypatch.delenv("LLAMPC_CTL_NO_STAGE", raising=False)
    row = M.Row("yaw-C1-H1-K1-N1", N=1, C=1, H=1, K=1, W=1, ticks=5, variant=dict(lpm=4, G=1, cpl=1, mpb=64))
    got = M.variant(row)
    for f, w in row.variant.items():
        assert got[f] == w, (f, got)
    orc = M.oracle_for(row)
    plant = O.Vehicle.from_params(O.orca_params())
    x = M.start_state(row)
    x[2] = PIO2 - 1e-9
    outs, xs = [], []
    for _ in range(row.ticks):                       # ctl_matrix.reference with this start
        with np.errstate(all="ignore"):
            o = orc.tick(x)
        outs.append(o)
        xs.append(x.copy())
        plant.Df *= 1 - 1 / 260.0
        plant.Dr *= 1 - 1 / 260.0
        xn, _ = O.sim_continuous(plant, x, o["u_seq"][:, 0].reshape(2, 1), [0, row.Ts])
        x = xn[:, -1]
    assert all(np.isfinite(o["cost"]) for o in outs)
    M._CACHE[row.name] = (outs, xs)
    try:
        M.run_device(row)
    finally:
        del M._CACHE[row.name]


# ------------------------------------------------------------------------------ the look-back
def test_lookback_untouched(nat, tmp_path):
    """The look-back runs the precise cores in one lane per model and none of the changed code: a
    full window at N = 257 (test_chain_selects_gpu.lookback_tick).  With LLAMPC_PARENT_LIB naming a
    build of the parent commit the top-K indices and the error window are bitwise that library's
    (a fresh process, one library per process); without it the window is held to the oracle at the
    suite's one-step tolerance, indices exact."""
    p, s, u, topk, best, win = CS.lookback_tick()
    parent = os.environ.get("LLAMPC_PARENT_LIB")
    if parent and os.path.exists(parent):
        out = str(tmp_path / "parent.npz")
        env = dict(os.environ, LLAMPC_HIP_LIB=parent)
        subprocess.run([sys.executable, os.path.abspath(CS.__file__), out], check=True, env=env, timeout=120)
        ref = np.load(out)
        np.testing.assert_array_equal(topk, ref["topk"])
        assert best == int(ref["best"])
        np.testing.assert_array_equal(CS._bits(win), CS._bits(ref["win"]))
        print("YAWFOLD look-back: bitwise equal to the parent library")
        return
    ow = O.LookbackWindow(CS.LB_N, CS.LB_W, CS.LB_K)
    cols = []
    for t in range(1, CS.LB_W + 2):
        e = O.lookback_errors(O.evaluate_models_vectorized(Z.shared(), tuple(p), s[:, t - 1], u[:, t - 1], Z.TS), s[:, t])
        ow.push(e)
        cols.append(e)
    want = np.stack(cols[-CS.LB_W:], axis=1)
    np.testing.assert_allclose(win, want, rtol=CS.RTOL_STEP, atol=0.0)
    np.testing.assert_array_equal(topk, ow.best_k)
    assert best == ow.current

"""The controller matrix's conditions (tests/ctl_matrix.py), on the oracle and the host-only
llampc_ctl_variant alone — no GPU: every row takes the launch variant it claims, is what it claims
(the clip rows clip, the ring wraps, the NaN policies select differently, ...), rests no exact index on
a near-tie, and compares costs as well conditioned as the existing closed-loop case's.

Conditioning, measured (conftest.cost_sensitivity: the relative cost change for one ulp of x0; the
90th percentile over every compared pair of every tick): test_ctl_closed_loop_vs_oracle's row 1
(200, 8, 20, 4, 10, "ETHZ", 14, None, 21), which passes on the device, reads 8.82e-16; the 63 rows read
2.03e-16 (v-C1-H1-K1-N1) to 8.75e-16 (v-C8-K32), and each must stay at or below the reference row's value
as measured in the same run.  Both are a few ulps of the cost: every row is far from the 1e-7 it is compared
under, and on the device no pair of any row needed its core-error bound (0 of 11 to 139 pairs per row; the
cap is 1 in 10).  Rows that read above the reference at the first choice of bank were moved
(ctl_matrix.REPICKED)."""
import numpy as np
import pytest

import ctl_matrix as M
from oracle import llampc_oracle as O


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    return _native


# (n, C, H, K, rl_n) -> (lpm, G, cpl, mpb, s4, zfit, R, nb_lb, nb_la), by hand from the rules:
#   G = the power of two >= C, at most 256; cpl = ceil(C / G); lpm = 4 if 4 G <= 256 else 2 if 2 G <= 256
#   else 1; mpb = 256 / (G lpm); nb_la = ceil((K + 1) / mpb); zfit = C H <= 16 * 192 = 3072;
#   R = ceil(n / (256 min(640 // K, 128))) (64 kListsPerLane / kWaves = 128); nb_lb = ceil(n / (256 R)).
#   s4 is the staged layout's size against 160 KiB (ctl_lds): small shapes fit, C H = 4096 does not.
KNOWN = [
    ((1, 1, 1, 1, 700), (4, 1, 1, 64, 1, 1, 1, 1, 1)),
    ((200, 8, 20, 10, 700), (4, 8, 1, 8, 1, 1, 1, 1, 2)),
    ((10000, 64, 40, 10, 700), (4, 64, 1, 1, 1, 1, 1, 40, 11)),
    ((100, 65, 20, 10, 700), (2, 128, 1, 1, 1, 1, 1, 1, 11)),
    ((100, 128, 24, 5, 700), (2, 128, 1, 1, None, 1, 1, 1, 6)),      # C H = 3072: the last that fits
    ((100, 128, 25, 5, 700), (2, 128, 1, 1, None, 0, 1, 1, 6)),
    ((100, 129, 8, 10, 700), (1, 256, 1, 1, 1, 1, 1, 1, 11)),
    ((50, 300, 10, 3, 500), (1, 256, 2, 1, None, 1, 1, 1, 4)),
    ((5120, 8, 10, 32, 700), (4, 8, 1, 8, 1, 1, 1, 20, 5)),          # 640 // 32 = 20 blocks: R = 1 up to 5120
    ((5121, 8, 10, 32, 700), (4, 8, 1, 8, 1, 1, 2, 11, 5)),
    ((16385, 8, 10, 10, 700), (4, 8, 1, 8, 1, 1, 2, 33, 2)),         # 640 // 10 = 64 blocks of 256: R = 1 up to 16384
]


@pytest.mark.parametrize("shape,want", KNOWN)
def test_ctl_variant_known(nat, monkeypatch, shape, want):
    """llampc_ctl_variant against tuples worked out by hand (s4 None: not claimed)."""
    monkeypatch.delenv("LLAMPC_CTL_NO_STAGE", raising=False)
    got = nat.ctl_variant(*shape)
    for f, w in zip(M.VARIANT_FIELDS, want):
        if w is not None:
            assert got[f] == w, (shape, f, got)


def test_ctl_variant_no_stage_and_refusals(nat, monkeypatch):
    """LLAMPC_CTL_NO_STAGE=1 turns the staging off and nothing else (as llampc_ctl_create reads it);
    a shape whose unstaged layout exceeds the CU's LDS and arguments out of range are LLAMPC_E_ARG."""
    monkeypatch.delenv("LLAMPC_CTL_NO_STAGE", raising=False)
    a = nat.ctl_variant(100, 96, 20, 10, 700)
    monkeypatch.setenv("LLAMPC_CTL_NO_STAGE", "1")
    b = nat.ctl_variant(100, 96, 20, 10, 700)
    assert a["s4"] == 1 and b["s4"] == 0 and {**a, "s4": 0} == b
    monkeypatch.delenv("LLAMPC_CTL_NO_STAGE")
    r = M.REFUSED
    for bad in ((r["N"], r["C"], r["H"], r["K"], M.KNOTS[r["track"]]), (0, 8, 20, 10, 700), (10, 0, 20, 10, 700),
                (10, 8, 65, 10, 700), (10, 8, 20, 33, 700), (10, 8, 20, 10, 1), (10, 2 ** 16 + 1, 20, 10, 700),
                (10, 2 ** 31 - 1, 64, 10, 700)):
        with pytest.raises(nat.NativeError) as e:
            nat.ctl_variant(*bad)
        assert e.value.code == nat.E_ARG, bad


def test_ctl_matrix_covers_every_variant(nat, monkeypatch):
    """Between them the rows run ctl_kernel<4>, <2> and <1>, each staged and unstaged, <2> and <1> also
    armed; the knots the rows assume are the tracks'."""
    monkeypatch.delenv("LLAMPC_CTL_NO_STAGE", raising=False)
    seen = {(M.variant(r)["lpm"], M.variant(r)["s4"]) for r in M.ROWS}
    assert seen == {(l, s) for l in (4, 2, 1) for s in (0, 1)}, seen
    assert {M.variant(r)["lpm"] for r in M.ROWS if r.armed} >= {2, 1}
    assert {M.variant(r)["lpm"] for r in M.ROWS if r.nostage} >= {2, 1}
    assert all(M.variant(r)["s4"] == 1 for r in M.ROWS if r.nostage)
    for name, n in M.KNOTS.items():
        assert len(M.tracks(name)[0].device_table()[0]) == n


P90_REFERENCE = None


def _p90_reference():
    global P90_REFERENCE
    if P90_REFERENCE is None:
        P90_REFERENCE = M.sensitivity_p90(M.reference_row())
    return P90_REFERENCE


@pytest.mark.parametrize("row", M.ROWS, ids=repr)
def test_ctl_row_conditions(nat, monkeypatch, row):
    """The row on the oracle: its variant, its claim, its gaps and its conditioning."""
    monkeypatch.delenv("LLAMPC_CTL_NO_STAGE", raising=False)
    got = M.variant(row)
    for f, w in row.variant.items():
        assert got[f] == w, (row.name, f, got)
    outs, xs = M.reference(row)
    assert len(outs) == row.ticks and not outs[-1]["warm"]
    sel = [o for o in outs if not o["warm"]]
    assert len(sel) >= 3 and outs[row.W]["warm"] and not outs[row.W + 1]["warm"]
    # what the row claims
    if row.clip_min is not None:
        share = M.clip_share(outs, row.clip_input)
        print(f"{row.name}: clip share {share:.3f}")
        assert share >= row.clip_min, share
    if row.sigma == (0.0, 0.0):
        for o in outs:
            assert all(np.array_equal(o["U"][c], o["U"][0]) for c in range(row.C))
            assert o["best_cand"] == 0 and (o["warm"] or np.all(o["topk_cand"] == 0))
    if row.name.startswith("S3-wrap"):
        assert len(sel) > row.S
    if row.standstill:
        assert xs[0][3] == 0.0 and xs[0][4] == 0.0 and xs[0][5] == 0.0
    if row.variant.get("R"):
        assert got["R"] == row.variant["R"] == 2
    if row.nan_models:
        other = M.BY_NAME[row.name.replace("nan-first", "nan-X").replace("nan-ignore", "nan-first").replace("nan-X", "nan-ignore")]
        mine, theirs = sel[0], [o for o in M.reference(other)[0] if not o["warm"]][0]
        assert mine["best_model"] != theirs["best_model"]
        if row.nan_first:
            assert mine["best_model"] == 0 and np.isnan(mine["cost"]) and mine["best_cand"] == 0
            assert mine["n_nonfinite"] >= row.C and np.isnan(mine["lb_best_val"])
        else:
            assert mine["best_model"] not in row.nan_models and np.isfinite(mine["cost"])
            assert mine["best_model"] == int(np.nanargmin(mine["window_means"]))
    # gaps
    gaps = np.array([M.tick_gaps(row, o) for o in outs])
    gc, gf, gm = gaps.min(axis=0)
    p90 = M.sensitivity_p90(row)
    print(f"{row.name}: gaps candidate {gc:.3g} flattened {gf:.3g} window mean {gm:.3g}; sensitivity p90 {p90:.3g} "
          f"(reference {_p90_reference():.3g})")
    assert gc > M.GAP_COST and gf > M.GAP_COST, (gc, gf)
    assert gm > M.GAP_MEAN, gm
    # conditioning
    assert p90 <= _p90_reference(), (p90, _p90_reference())


def test_terminal_cost_changes_the_choice():
    """P = 0 (base-C8) against P != 0 (cost-P-C8), everything else equal — bank, Q, R, seeds, start: the
    oracle chooses another candidate on some selection tick, so a terminal term the device dropped would be seen."""
    base, row = M.BASE, M.BY_NAME["cost-P-C8"]
    for f in ("N", "C", "H", "K", "W", "track", "ticks", "bank_seed", "Ts", "umin", "umax", "rate_max", "sigma", "seed",
              "S", "v_factor", "mu_init", "nan_first", "nan_models", "standstill"):
        assert getattr(base, f) == getattr(row, f), f
    assert np.array_equal(base.Q, row.Q) and np.array_equal(base.R, row.R)
    assert not base.P.any() and row.P.any()
    (a, xa), (b, xb) = M.reference(base), M.reference(row)
    # the first tick whose choices differ had the same state, candidates and model: P alone moved it
    i = next(i for i, (x, y) in enumerate(zip(a, b)) if x["best_cand"] != y["best_cand"])
    assert np.array_equal(xa[i], xb[i]) and np.array_equal(a[i]["U"], b[i]["U"]) and a[i]["best_model"] == b[i]["best_model"]
    assert any(not x["warm"] and x["best_cand"] != y["best_cand"] for x, y in zip(a, b))


def test_oracle_nan_policy_and_pwm_rate_reach_the_oracle():
    """ControllerOracle's nan_first reaches its window; the pwm rate bound reaches the feasibility."""
    w = O.LookbackWindow(3, 1, 2, nan_first=False)
    w.push(np.array([np.nan, 2.0, 1.0]))
    assert w.current == 2 and list(w.best_k) == [2, 1]
    w = O.LookbackWindow(3, 1, 2)
    w.push(np.array([1.0, np.nan, 0.5]))
    assert w.current == 1 and list(w.best_k) == [2, 0]
    U = np.zeros((1, 3, 2))
    U[0, 1:, 0] = 0.5
    assert O.candidates_feasible(U, np.zeros(2), (-1, -1), (1, 1), 5.0, 0.02)[0]
    assert not O.candidates_feasible(U, np.zeros(2), (-1, -1), (1, 1), 5.0, 0.02, rate_max_pwm=2.0)[0]
    U[0, :, 1] = 0.3
    assert O.candidates_feasible(U, np.zeros(2), (-1, -1), (1, 1), -1.0, 0.02)[0]
    assert not O.candidates_feasible(U, np.zeros(2), (-1, -1), (1, 1), 5.0, 0.02)[0]

"""The look-back on the device over the matrix of tests/lookback_matrix.py: window lengths 1 .. 128
with every ring slot the newest twice, list counts round lb_final's `L >= K` and past 512 entries,
several models per lane (R > 1) with a real window, exact ties across every boundary of the layout,
NaN and +inf errors, K changing between ticks over one ring, reset(), and the fused plan launch.

Every tick of every row goes through lookback_matrix.check_tick: the errors against the oracle at
RTOL_STEP; the ring, the window mean (against np.mean of the ring the device holds) and the top-K
values as bits; the indices exact.  No tolerance but RTOL_STEP appears.  reset / replay and fused
vs plain compare two device paths bit for bit, and each of the two also passes check_tick (the
fused launch: its ring through check_window, its record against the checked path's)."""
import numpy as np
import pytest

import lookback_matrix as M
from conftest import golden

pytestmark = pytest.mark.gpu

R1_ROWS = [r for r in M.ROWS if r.R == 1]
FUSED_ROWS = ["w9", "n2305-k10-plain", "n5377-k32-w9-plain"]


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


def device_bank(row):
    from llampc.mpc import ModelBank
    return ModelBank(M.bank_params(row), W=row.W, device=0)


def same_bits(a, b, what):
    np.testing.assert_array_equal(M.bits(a), M.bits(b), err_msg=what)


@pytest.mark.parametrize("policy", M.POLICIES, ids=("nan-first", "nan-ignore"))
@pytest.mark.parametrize("row", M.ROWS, ids=lambda r: r.name)
def test_lookback_row(nat, row, policy):
    keep = []
    with device_bank(row) as b:
        M.run_row(b, row, policy, keep=keep)
    if row.recipe == "dups":                   # the copies tie exactly on the device too, on every tick
        ties = M.ties_of(row)
        for t, r in enumerate(keep):
            assert len(set(M.bits(r["errors"][ties]).tolist())) == 1, (row.name, t)
    if row.recipe == "inf-tick":               # +inf means while the tick is in the ring, finite after it
        full = [r["full"] and bool(np.isposinf(r["window_mean"]).all()) for r in keep]
        assert [t for t, f in enumerate(full) if f] == list(range(row.W + 1, 2 * row.W + 1))
        assert np.isfinite(keep[-1]["window_mean"]).all()


@pytest.mark.parametrize("row", R1_ROWS, ids=lambda r: r.name)
def test_lookback_row_without_mean_readback(nat, row):
    """R = 1 keeps the mean in a register; wm_keep (the caller reads the means) is launch-uniform:
    without the read-back the selection must be the same bits."""
    keep = []
    oe = M.oracle_errors(row)
    with device_bank(row) as a, device_bank(row) as b:
        M.run_row(a, row, M.NAN_FIRST, keep=keep)
        prev = None
        for t in range(row.ticks):
            r = b.lookback(*M.transition(row, t), Ts=M.TS, K=row.K, return_errors=True, return_window_mean=False)
            assert r["window_mean"] is None
            M.close(r["errors"], oe[t], M.RTOL_STEP)
            win = b.window()
            M.check_window(row, t, prev, win, r["errors"])
            prev = win
            w = keep[t]
            what = f"{row.name} t={t}"
            same_bits(r["errors"], w["errors"], what)
            assert (r["window_count"], r["full"], r["best"]) == (w["window_count"], w["full"], w["best"]), what
            if r["full"]:
                np.testing.assert_array_equal(r["topk"], w["topk"], err_msg=what)
                same_bits(r["topk_val"], w["topk_val"], what)


def test_lookback_k_changes_between_ticks(nat):
    """K = 32, 10, 1 in turn over one ring: R = 2, 1, 1, so the block layout changes from tick to tick."""
    base = M.KCYCLE
    oe = M.oracle_errors(base)
    for policy in M.POLICIES:
        with device_bank(base) as b:
            prev = None
            for t in range(base.ticks):
                K, _, R, L = M.KCYCLE_SHAPES[t % 3]
                row = base._replace(K=K, R=R, L=L)
                r = b.lookback(*M.transition(row, t), Ts=M.TS, K=K, nan_policy=policy, return_errors=True,
                               return_window_mean=True)
                prev = M.check_tick(b, row, t, prev, r, oe[t], policy)


def test_lookback_reset_replays(nat):
    row = M.BY_NAME["n5377-k32-w9-plain"]
    first, again = [], []
    with device_bank(row) as b:
        M.run_row(b, row, M.NAN_FIRST, keep=first)
        b.reset()
        assert b.window_count == 0
        M.run_row(b, row, M.NAN_FIRST, ticks=row.W + 1, keep=again)
    assert len(again) == row.W + 1
    for t, (r, w) in enumerate(zip(again, first)):
        same_bits(r["errors"], w["errors"], f"t={t}")
        assert (r["window_count"], r["full"], r["best"]) == (w["window_count"], w["full"], w["best"]), t
        if r["full"]:
            same_bits(r["window_mean"], w["window_mean"], f"t={t}")
            np.testing.assert_array_equal(r["topk"], w["topk"])
            same_bits(r["topk_val"], w["topk_val"], f"t={t}")


@pytest.mark.parametrize("name", FUSED_ROWS)
def test_plan_fused_lookback_equals_lookback(nat, name):
    """The look-back inside a plan launch that also rolls out a small look-ahead (C = 2, H = 3):
    its errors, means, ring and the record's look-back fields are those of a look-back-only bank."""
    row = M.BY_NAME[name]
    d = golden("dyn_slice.npz")
    C, H, K = 2, 3, row.K
    p = M.bank_params(row)
    plain = []
    with device_bank(row) as a, device_bank(row) as b:
        M.run_row(a, row, M.NAN_FIRST, keep=plain)
        prev = None
        for t in range(row.ticks):
            x_prev, u_prev, x_now = M.transition(row, t)
            U = np.repeat(d["inputs"][:, t + 1:t + 1 + H].T[None], C, axis=0)
            U[1] *= 0.9
            xref = d["states"][:2, t + 1:t + H + 2]
            out, err, wm, _ = b.plan_raw(x_prev, u_prev, x_now, U, xref, u_prev, Ts=M.TS, K=K,
                                         return_errors=True, return_window_mean=True)
            w = plain[t]
            what = f"{name} t={t}"
            same_bits(err, w["errors"], what)
            win = b.window()
            M.check_window(row, t, prev, win, err)
            prev = win
            assert (out.window_count, bool(out.window_full), out.K, out.status) == (w["window_count"], w["full"], K, 0), what
            if not w["full"]:
                assert out.lb_best == -1 and np.all(np.array(out.topk[:]) == -1), what
                continue
            same_bits(wm, w["window_mean"], what)
            topk = np.array(out.topk[:K])
            assert out.lb_best == w["best"], what
            same_bits(out.lb_best_val, w["window_mean"][w["best"]], what)
            np.testing.assert_array_equal(topk, w["topk"], err_msg=what)
            same_bits(np.array(out.topk_val[:K]), w["topk_val"], what)
            same_bits(np.array(out.topk_Df[:K]), p[2][topk], what)
            same_bits(np.array(out.topk_Dr[:K]), p[5][topk], what)
            assert np.all(np.array(out.topk[K:]) == -1), what
            assert out.sel_model == w["best"] and out.la_best_model >= 0, what

"""The plan tick's tail after the last look-ahead rollout (csrc/final_dev.hpp final_poll / final_write,
csrc/lookahead_dev.hpp la_publish and the block epilogue): a block's five tagged words are stored by
five lanes (each folds the waves' picks itself), and the record's look-ahead best is split from its key
(goff + n) C + c by split_key — at C = 1 taken as it is — not by a 64-bit / and %.

Shapes: the smallest at which that code can go wrong — n in {1, 15, 16, 17, 64, 65, 257} (one model, a
partial wave of quads, exactly one wave, the two block boundaries at 64 models per LPM-4 block, more than
one block) x C in {1, 3, 64} (the two-word path, a key split by a non-power of two, a model spanning
several waves), H = 3, W = K = 4, W + 1 ticks (partial-window ticks: topk = -1 and NaN fields; full-window
ticks), and one bank with a shard offset goff > 0.

Asserted per tick: the polled completion and the ticket completion (LLAMPC_NO_POLL=1 set around the call,
as tests/test_gpu_parity.py test_polled_completion_equals_ticket_completion does; the library reads it
per launch) agree bitwise on every record field and on the per-model costs; the costs agree with
oracle.plan_cpu within conftest.assert_costs_close at the suite's 1e-6; the record's selection, top-K,
non-finite count and look-ahead best are the oracle's, and its per-model results (sel_cand / sel_cost,
topk_cand / topk_cost — the per-model results a polled tick delivers) are the NaN-last argmin of the
device's own cost rows, bitwise.

C per tick: llampc_plan takes C with every tick's inputs, so the stale-tag case switches 1 -> 3 -> 1 on
one bank.

test_every_model_nan: when every cost of the tick is NaN the record has no look-ahead best (-1, -1,
NaN; llampc.h).  That is the one record that is not the parent commit's: a bank-wide NaN still carries
keys through la_publish's NaN-last picks, and the parent's final_write stored the lowest of them, (0, 0,
NaN) (measured on the MI355X, C = 1 and C = 3); final_write now takes a NaN best cost for no best.  A
tick with any cost that is a number, +inf included, is bitwise the parent's."""
import os

import numpy as np
import pytest

from conftest import assert_costs_close, core_error_bound, golden
from oracle import llampc_oracle as O

pytestmark = pytest.mark.gpu

RTOL_ROLL = 1e-6
TS = 0.02
H, W, K = 3, 4, 4
Q, R, P = np.eye(2), np.diag([5e-3, 1.0]), np.zeros((2, 2))
NS = (1, 15, 16, 17, 64, 65, 257)
CS = (1, 3, 64)


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


def tick_args(t, C):
    """Tick t of the recorded slice: the transition t - 1 -> t, C candidates (the recorded inputs, +-0.02
    noise on candidates 1..), the recorded positions shifted by 1 cm in y as the reference."""
    d = golden("dyn_slice.npz")
    s, u = d["states"], d["inputs"]
    U = np.repeat(u[:, t:t + H].T[None], C, axis=0).copy()
    U[1:] += np.random.RandomState(1000 * t + C).uniform(-0.02, 0.02, U[1:].shape)
    xref = s[:2, t:t + H + 1] + 0.01 * np.arange(2)[:, None]
    return (s[:, t - 1].copy(), u[:, t - 1].copy(), s[:, t].copy(), U, xref, u[:, t - 1].copy())


_ORACLE = {}


def oracle_ticks(N, C, w, ticks, bank_key, bank):
    """The oracle's ticks 1..ticks on `bank` (window w), once per (shape, bank): per tick (full, current,
    best_k, cref [N, C])."""
    key = (N, C, w, ticks, bank_key)
    if key not in _ORACLE:
        win = O.LookbackWindow(N, w, K)
        rows = []
        with np.errstate(all="ignore"):
            for t in range(1, ticks + 1):
                cur, bk, cref = O.plan_cpu(shared(), bank, win, *tick_args(t, C), TS, Q, R, P)
                cref.setflags(write=False)
                rows.append((win.count >= w, int(cur), np.array(bk).copy(), cref))
        _ORACLE[key] = rows
    return _ORACLE[key]


def both(nat, pb, tb, args, **kw):
    """One tick on the polled bank and on the ticket bank: (record dict, costs) of each."""
    o, _, _, pc = pb.plan_raw(*args, Ts=TS, K=K, return_costs=True, **kw)
    os.environ["LLAMPC_NO_POLL"] = "1"
    try:
        w, _, _, tc = tb.plan_raw(*args, Ts=TS, K=K, return_costs=True, **kw)
    finally:
        del os.environ["LLAMPC_NO_POLL"]
    return nat.plan_out_to_dict(o), pc, nat.plan_out_to_dict(w), tc


def same_record(A, B, what):
    for k in A:
        if isinstance(A[k], np.ndarray):
            np.testing.assert_array_equal(A[k], B[k], err_msg=f"{what}: {k}")
        else:
            assert A[k] == B[k] or (A[k] != A[k] and B[k] != B[k]), (what, k, A[k], B[k])


def argmin_nl(row):
    return O.argmin_nan_last(row)


def check_against(A, costs, goff, full, cur, best_k, cref, C, args, bank, what):
    """The record A and the device's costs against the oracle's tick."""
    N = cref.shape[0]
    x_prev, u_prev, x0, U, xref, uprev = args

    def bound(idx):
        return core_error_bound(shared(), tuple(bank), x0, U, xref, uprev, Q, R, P, Ts=TS)[idx]

    assert_costs_close(costs, cref, RTOL_ROLL, bound)
    assert A["status"] == 0, what
    assert bool(A["window_full"]) == full, what
    sel = goff + cur if full else goff                       # current_model = goff while the window fills
    assert A["sel_model"] == sel and A["sel_owned"] == 1, what
    sl = sel - goff
    assert A["sel_cand"] == argmin_nl(costs[sl]) and A["sel_cost"] == costs[sl, A["sel_cand"]], what
    kk = min(K, N)
    if full:
        assert A["lb_best"] == goff + cur, what
        np.testing.assert_array_equal(A["topk"][:kk], goff + best_k[:kk], err_msg=what)
        np.testing.assert_array_equal(A["topk"][kk:], -1, err_msg=what)
        for k in range(kk):
            m = int(A["topk"][k]) - goff
            assert A["topk_cand"][k] == argmin_nl(costs[m]) and A["topk_cost"][k] == costs[m, A["topk_cand"][k]], (what, k)
        np.testing.assert_array_equal(A["topk_cand"][kk:], -1, err_msg=what)
        assert np.isnan(A["topk_cost"][kk:]).all(), what
    else:                                                    # a partial window: no look-back result
        assert A["lb_best"] == -1 and np.isnan(A["lb_best_val"]), what
        np.testing.assert_array_equal(A["topk"], -1, err_msg=what)
        np.testing.assert_array_equal(A["topk_cand"], -1, err_msg=what)
        for f in ("topk_val", "topk_Df", "topk_Dr", "topk_cost"):
            assert np.isnan(A[f]).all(), (what, f)
    assert A["n_nonfinite"] == int(np.count_nonzero(~np.isfinite(cref))), what
    j = argmin_nl(cref.ravel())                              # the oracle's NaN-last argmin over (model, candidate)
    jd = argmin_nl(costs.ravel())
    assert (A["la_best_model"], A["la_best_cand"]) == (goff + jd // C, jd % C), what
    assert A["la_best_cost"] == costs.ravel()[jd] or (np.isnan(A["la_best_cost"]) and np.isnan(costs.ravel()[jd])), what
    assert jd == j, (what, "the device's argmin is not the oracle's", jd, j)


def run_shape(nat, N, C, goff):
    from llampc.mpc import ModelBank, generate_bank
    bank = generate_bank(N, seed=3)
    rows = oracle_ticks(N, C, W, W + 1, "seed3", bank)
    pb = ModelBank(bank, W=W, device=0, global_offset=goff)
    tb = ModelBank(bank, W=W, device=0, global_offset=goff)
    try:
        for t in range(1, W + 2):
            args = tick_args(t, C)
            A, pc, B, tc = both(nat, pb, tb, args, current_model=goff)
            what = f"n={N} C={C} goff={goff} tick {t}"
            same_record(A, B, what + " polled vs ticket")
            np.testing.assert_array_equal(pc, tc, err_msg=what)
            full, cur, bk, cref = rows[t - 1]
            assert full == (t >= W)
            check_against(A, pc, goff, full, cur, bk, cref, C, args, bank, what)
    finally:
        pb.close()
        tb.close()


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("N", NS)
def test_record_polled_equals_ticket_equals_oracle(nat, N, C):
    run_shape(nat, N, C, 0)


@pytest.mark.parametrize("C", CS)
def test_record_with_shard_offset(nat, C):
    """goff > 0: the key is (goff + n) C + c; goff = 10^6 + 7 puts the C = 64 keys above 2^26 and the
    record's indices off every power of two."""
    run_shape(nat, 65, C, 1000007)


def nan_bank(N, which):
    from llampc.mpc import generate_bank
    bank = generate_bank(N, seed=3).copy()
    bank[2, which] = np.nan                                  # Df: the front tire force, every rollout step
    return bank


def nan_tick(nat, N, C, which, key):
    """One tick (W = 1: the first tick fills the window) of a bank whose models `which` have a NaN Df:
    (polled record, polled costs, cref); polled and ticket held bitwise equal on the way."""
    from llampc.mpc import ModelBank
    bank = nan_bank(N, which)
    full, cur, bk, cref = oracle_ticks(N, C, 1, 1, key, bank)[0]
    pb, tb = ModelBank(bank, W=1, device=0), ModelBank(bank, W=1, device=0)
    try:
        A, pc, B, tc = both(nat, pb, tb, tick_args(1, C))
    finally:
        pb.close()
        tb.close()
    same_record(A, B, f"NaN bank {key} C={C} polled vs ticket")
    np.testing.assert_array_equal(pc, tc)
    np.testing.assert_array_equal(np.isnan(pc), np.isnan(cref))
    return A, pc, cref


@pytest.mark.parametrize("C", (1, 3))
def test_one_nan_model(nat, C):
    """Model 37 of 65 goes NaN in the look-ahead (asserted of the oracle first): n_nonfinite is the
    oracle's count, la_best_* the oracle's NaN-last argmin."""
    N, bad = 65, 37
    A, pc, cref = nan_tick(nat, N, C, [bad], "nan37")
    assert np.isnan(cref[bad]).all() and np.isfinite(np.delete(cref, bad, axis=0)).all()
    assert A["status"] == 0
    assert A["n_nonfinite"] == int(np.count_nonzero(~np.isfinite(cref))) == C
    j = argmin_nl(cref.ravel())
    assert (A["la_best_model"], A["la_best_cand"]) == (j // C, j % C) and j // C != bad
    np.testing.assert_allclose(A["la_best_cost"], cref.ravel()[j], rtol=RTOL_ROLL)
    assert A["la_best_cost"] == pc.ravel()[j]


@pytest.mark.parametrize("C", (1, 3))
def test_every_model_nan(nat, C):
    """Every model NaN: no look-ahead best — la_best_model = -1, la_best_cand = -1, cost NaN — and
    n_nonfinite = n C.  (The parent commit's library gives la_best_model 0, la_best_cand 0 here: module
    docstring.)"""
    N = 17
    A, pc, cref = nan_tick(nat, N, C, list(range(N)), "nanall")
    assert np.isnan(cref).all()
    assert A["status"] == 0
    assert A["n_nonfinite"] == N * C
    print(f"ALLNAN C={C}: la_best_model {A['la_best_model']} la_best_cand {A['la_best_cand']} la_best_cost {A['la_best_cost']}")
    assert np.isnan(A["la_best_cost"])
    assert (A["la_best_model"], A["la_best_cand"]) == (-1, -1)


def fresh_record(nat, bank, t, C):
    from llampc.mpc import ModelBank
    with ModelBank(bank, W=1, device=0) as b:
        o, _, _, c = b.plan_raw(*tick_args(t, C), Ts=TS, K=K, return_costs=True)
        return nat.plan_out_to_dict(o), c


@pytest.mark.parametrize("Cseq", ((1, 1), (3, 3), (1, 3, 1), (3, 1, 3)))
def test_stale_tags_never_pass(nat, Cseq):
    """Consecutive ticks on one bank (W = 1, so a tick's record depends on that tick's inputs alone) with
    different inputs, and with C switching between ticks (1 -> 3 -> 1: the words an earlier tick left
    behind carry its tag, whatever C it ran at, and none of them may pass for this tick's): every record equals a fresh bank's record for that tick's input, bitwise, costs
    included."""
    from llampc.mpc import ModelBank, generate_bank
    N = 65
    bank = generate_bank(N, seed=3)
    with ModelBank(bank, W=1, device=0) as b:
        for i, C in enumerate(Cseq):
            t = 1 + 2 * i
            o, _, _, c = b.plan_raw(*tick_args(t, C), Ts=TS, K=K, return_costs=True)
            A = nat.plan_out_to_dict(o)
            F, fc = fresh_record(nat, bank, t, C)
            assert A["status"] == 0
            same_record(A, F, f"Cseq {Cseq} tick {i} (C = {C}): used bank vs fresh bank")
            np.testing.assert_array_equal(c, fc)

"""The look-back matrix's conditions (tests/lookback_matrix.py) on NumPy alone — no GPU: the checker
accepts the reference (FakeBank), four wrong look-backs each fail it on a row that names them, the
bitwise mean comparison has power on these inputs, and the dups rows tie across every boundary they
claim.  That each row has the (R, L) it states is test_capi_native.py's test_shape_block_counts,
which takes the rows from lookback_matrix.SHAPE_ROWS.

Power of the bitwise comparison, measured on the oracle's errors of the W-sweep bank (N = 300, over
the W + 2 full windows of the row's 2 W + 1 ticks): the share of (model, tick) pairs whose sequentially
summed mean differs in bits from np.mean, W >= 8, and whose mean over the window rotated by one slot
does, W >= 3 (both must be >= 10 %; test_mean_comparison_has_power prints them; no row needed another seed):

    W           3     7     8     9    15    16    17    24    25    32    33    64   127   128
    sequential  -     -  42.1  33.6  20.9  54.0  47.6  52.6  51.4  63.1  59.8  72.5  77.6  80.8  %
    rotated  21.7  36.4  30.8  40.1  42.9  27.9  42.1  23.9  40.2  29.0  45.0  27.9  47.3  28.5  %"""
import numpy as np
import pytest

import lookback_matrix as M

POWER_MIN = 0.10
CPU_ROWS = [r for r in M.ROWS if r.N <= 5377]


@pytest.mark.parametrize("row", CPU_ROWS, ids=lambda r: r.name)
def test_checker_accepts_reference(row):
    for policy in M.POLICIES:
        M.run_row(M.FakeBank(M.bank_params(row), row.W), row, policy)


# ------------------------------------------------------------------------------- the checker's teeth
class SequentialMean(M.FakeBank):
    def _mean(self, win):
        s = np.zeros(win.shape[0])
        for c in range(win.shape[1]):
            s = s + win[:, c]
        return s / win.shape[1]


class RingOneSlotLate(M.FakeBank):
    """The window summed from the wrong oldest slot: the same W values, one slot round."""

    def _mean(self, win):
        return np.mean(np.ascontiguousarray(np.roll(win, 1, axis=1)), axis=1)


class UnstableTies(M.FakeBank):
    """Equal means come out with the higher index first."""

    def _order(self, wm):
        key = np.where(np.isnan(wm), np.inf, wm)
        return np.lexsort((-np.arange(len(wm)), np.isnan(wm), key))


class ArgminSkipsNan(M.FakeBank):
    def _argmin(self, wm, policy):
        return int(np.nanargmin(wm)) if not np.isnan(wm).all() else 0


MUTANTS = [(SequentialMean, ["w8", "w17", "w128", "n16385-k10-w16-plain"], "window mean bits"),
           (RingOneSlotLate, ["w3", "w16", "w33", "n5377-k32-w9-plain", "n2305-k10-plain"], "window mean bits"),
           (UnstableTies, ["n2305-k10-dups", "n257-k1-dups", "n5377-k32-w9-dups"], "topk"),
           (ArgminSkipsNan, ["n5121-k32-w8-nan", "n2305-k10-nan-most"], None)]


@pytest.mark.parametrize("mutant,names,why", MUTANTS, ids=lambda v: v.__name__ if isinstance(v, type) else "")
def test_checker_has_teeth(mutant, names, why):
    """Each wrong look-back fails check_tick on every row that names it — by the assertion meant for it —
    and only from the first full window on."""
    for name in names:
        row = M.BY_NAME[name]
        if row.N > 5377:                       # the large rows: the first full windows are enough
            row = row._replace(ticks=row.W + 1)
        with pytest.raises(AssertionError) as exc:
            M.run_row(mutant(M.bank_params(row), row.W), row, M.NAN_FIRST)
        assert (why or "policy=0") in str(exc.value), (name, str(exc.value)[:300])
    # the mutants are right where they do not differ: a wrong argmin passes under NaN-ignore
    row = M.BY_NAME["n5121-k32-w8-nan"]
    M.run_row(ArgminSkipsNan(M.bank_params(row), row.W), row, M.NAN_IGNORE)


# ------------------------------------------------------------------------------- power
def _windows(row):
    """[ticks - W + 1, N, W]: every full window of the row under the oracle, oldest slot first."""
    e = M.oracle_errors(row)
    return np.array([np.ascontiguousarray(e[t - row.W + 1:t + 1].T) for t in range(row.W - 1, row.ticks)])


@pytest.mark.parametrize("row", [r for r in M.W_SWEEP if r.W >= 3], ids=lambda r: r.name)
def test_mean_comparison_has_power(row):
    """A condition on the inputs: a wrong summation order or a wrong oldest slot must change the
    mean's bits on at least 10 % of the (model, tick) pairs the row compares.  A row that misses it
    gets another bank seed (lookback_matrix.BANK_SEED); the threshold stays."""
    W = row.W
    wins = _windows(row)
    assert wins.shape == (W + 2, row.N, W)
    ref = np.mean(wins, axis=2)
    seq = np.zeros(ref.shape)
    for c in range(W):
        seq = seq + wins[:, :, c]
    seq /= W
    rot = np.mean(np.ascontiguousarray(np.roll(wins, 1, axis=2)), axis=2)
    s_seq = float(np.mean(M.bits(seq) != M.bits(ref)))
    s_rot = float(np.mean(M.bits(rot) != M.bits(ref)))
    print(f"{row.name}: sequential {100 * s_seq:.1f} %, rotated {100 * s_rot:.1f} %")
    if W >= 8:
        assert s_seq >= POWER_MIN, (row.name, s_seq)
    assert s_rot >= POWER_MIN, (row.name, s_rot)


def test_mean_reference_is_numpys_pairwise_order():
    """np.mean over a C-contiguous row is the pairwise order the kernel restates (oracle.np_pairwise_sum)."""
    from oracle import llampc_oracle as O
    for row in M.W_SWEEP:
        win = _windows(row)[-1][:40]
        want = np.array([O.np_pairwise_sum(list(w)) / row.W for w in win])
        np.testing.assert_array_equal(M.bits(np.mean(win, axis=1)), M.bits(want), err_msg=row.name)


# ------------------------------------------------------------------------------- the recipes
@pytest.mark.parametrize("row", [r for r in M.ROWS if r.recipe == "dups"], ids=lambda r: r.name)
def test_dups_rows_tie_across_every_boundary(row):
    ties = M.ties_of(row)
    e = M.oracle_errors(row)
    assert len(ties) >= 4
    for t in range(row.ticks):                         # exact ties on every tick, and they are the minimum
        assert len(set(M.bits(e[t, ties]).tolist())) == 1, (row.name, t)
    # the ties decide an output: the tied models are the argmin of the first full window's mean (the
    # lower index wins the argmin and the first top-K entry) and stay inside the top-K on later ticks
    rank = []
    for t in range(row.W - 1, row.ticks):
        wm = np.mean(np.ascontiguousarray(e[t - row.W + 1:t + 1].T), axis=1)
        rank.append(int((wm < wm[ties[0]]).sum()))
    assert rank[0] == 0 and sum(r < row.K for r in rank) >= min(2, row.K), (row.name, rank)
    seen = set()
    for a in ties:
        for b in ties:
            if a < b:
                seen |= M.tie_classes(int(a), int(b), row.N, row.R)
    assert seen >= M.classes_of(row), (row.name, seen)


def test_recipes_are_what_they_claim():
    for row in M.ROWS:
        p, e = M.bank_params(row), M.oracle_errors(row)
        assert p.shape == (6, row.N) and e.shape == (row.ticks, row.N) and not p.flags.writeable
        assert row.N >= row.K and row.ticks > row.W
        per = M.KBLOCK * row.R
        assert row.L == -(-row.N // per)
        if row.recipe == "nan":
            bad = np.flatnonzero(np.isnan(e[0]))
            assert bad.tolist() == sorted({11, row.N // 2, row.N - 1})
            assert (row.N - 1) // per == row.L - 1
        elif row.recipe == "nan-most":
            assert np.isfinite(e).sum(axis=1).tolist() == [5] * row.ticks and 5 < row.K
        elif row.recipe == "inf-tick":
            inf = np.isposinf(e).all(axis=1)
            assert np.flatnonzero(inf).tolist() == [row.W + 1] and np.isfinite(e[~inf]).all()
            assert row.ticks >= 2 * row.W + 2          # a finite mean again after the W infinite ones
        else:
            assert np.isfinite(e).all()
    # the rows the issue names
    short = {r.N: r.N - (r.L - 1) * M.KBLOCK * r.R for r in M.ROWS}
    assert short[2305] == 1 and short[4869] == 5 and short[5121] == 1 and short[5377] == 257 and short[1792] == 256
    assert {(k, n): (r, l) for k, n, r, l in M.SHAPE_ROWS}[(32, 4869)] == (1, 20) and 20 * 32 > 512

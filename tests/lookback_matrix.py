"""The look-back parity matrix's rows, recipes and checker, shared by test_lookback_matrix_cpu.py
(the checker on a NumPy stand-in, its teeth, the power of the bitwise comparison) and
test_lookback_matrix_gpu.py (the device through ModelBank).

A row = (name, N, W, K, recipe, ticks, R, L).  R and L are the STATED models per look-back lane and
look-back block count: test_capi_native.py's test_shape_block_counts holds them against plan_shape
(SHAPE_ROWS).  Tick t runs the transition (states[:, t % 150], inputs[:, t % 150], states[:, t % 150 + 1])
of tests/golden/dyn_slice.npz at Ts = 0.02 on generate_bank(N, seed=N) (BANK_SEED names the rows that
took another seed, and why), changed by the row's recipe — a pure function of the row:

  plain     the generated bank
  dups      the parameters of one model copied onto indices so that exact ties cross every boundary
            the row has (tie_classes: the same wave, another wave of the block, another block, another
            r row of the block when R > 1, index N - 1).  The model is the oracle argmin of the first
            full window's mean (dup_source; at W = 1 the tick-0 argmin): the tick-0 argmin alone is
            outside the top-K of every full window at W = 9 and 16, where the ties would decide nothing
  nan       Df = NaN on model 11, on the last model (the last block) and on N // 2
  nan-most  every model NaN but 5 (fewer finite models than K = 10)
  inf-tick  the plain bank; on tick W + 1, x_now[0] = 1e200: every error is +inf on that tick and every
            window mean +inf while it stays in the ring (W ticks), then finite again

check_tick is the one set of assertions every path is held to.  Apart from the errors against the oracle
(RTOL_STEP, test_gpu_parity.close) every comparison is exact: the ring and the mean as uint64 views
against NumPy (np.mean(window, axis=1): the kernel's win_pre / win_finish claim its bits), the
selection from the path's own window mean."""
import collections
import functools

import numpy as np

from conftest import golden
from oracle import llampc_oracle as O
from test_gpu_parity import RTOL_STEP, TS, close, shared

NAN_FIRST, NAN_IGNORE = 0, 1
POLICIES = (NAN_FIRST, NAN_IGNORE)
KBLOCK = 256
SLICE_TICKS = 150

Row = collections.namedtuple("Row", "name N W K recipe ticks R L")

# rows whose bank is not generate_bank(N, seed=N): {N: (seed, why)} (the power condition of
# test_lookback_matrix_cpu.py moves a bank, never its threshold)
BANK_SEED = {}

W_SWEEP_W = (1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 25, 32, 33, 64, 127, 128)
W_SWEEP = [Row(f"w{W}", 300, W, 10, "plain", 2 * W + 1, 1, 2) for W in W_SWEEP_W]

# (N, K, R, L): L == K - 1 (no threshold: every entry is a candidate) | L == K, the last block holds one
# model | L == K + 1 | L == K, N a multiple of 256 | K = 1 | M = L K = 640 > 512, the last block holds 5
# models (fewer than K): its list's missing entries sit at e >= 512
LIST_SHAPES = [(2304, 10, 1, 9), (2305, 10, 1, 10), (2561, 10, 1, 11), (1792, 7, 1, 7), (257, 1, 1, 2),
               (4869, 32, 1, 20)]
LIST_ROWS = [Row(f"n{N}-k{K}-{rec}", N, 3, K, rec, 8, R, L) for N, K, R, L in LIST_SHAPES for rec in ("plain", "dups")]

# (N, K, W, R, L): the last block holds one model (r = 0, lane 0) | its r = 0 row full, r = 1 one model |
# R = 3 | R = 2 at K = 10, W % 8 == 0
R_SHAPES = [(5121, 32, 8, 2, 11), (5377, 32, 9, 2, 11), (10241, 32, 3, 3, 14), (16385, 10, 16, 2, 33)]
R_ROWS = [Row(f"n{N}-k{K}-w{W}-{rec}", N, W, K, rec, 2 * W + 1, R, L)
          for N, K, W, R, L in R_SHAPES for rec in ("plain", "dups", "nan")]

# nan-most: 5 finite models, K = 10.  inf-tick: the +inf errors of tick W + 1 leave the ring after tick
# 2 W, so the W = 9 row runs 2 W + 3 ticks (two finite ticks after them); 8 ticks do at W = 3.
SPECIAL_ROWS = [Row("n2305-k10-nan-most", 2305, 3, 10, "nan-most", 8, 1, 10),
                Row("w9-inf-tick", 300, 9, 10, "inf-tick", 21, 1, 2),
                Row("n2561-k10-inf-tick", 2561, 3, 10, "inf-tick", 8, 1, 11)]

ROWS = W_SWEEP + LIST_ROWS + R_ROWS + SPECIAL_ROWS
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)

# K cycling over one ring (test_lookback_k_changes_between_ticks): R = 2, 1, 1
KCYCLE = Row("kcycle", 6000, 4, None, "plain", 14, None, None)
KCYCLE_SHAPES = [(32, 6000, 2, 12), (10, 6000, 1, 24), (1, 6000, 1, 24)]

# (K, n, R, nb_lb) of every row, for test_capi_native.py's test_shape_block_counts
SHAPE_ROWS = sorted({(r.K, r.N, r.R, r.L) for r in ROWS} | set(KCYCLE_SHAPES))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------- recipes
def transition(row, t):
    """(x_prev, u_prev, x_now) of tick t."""
    d = golden("dyn_slice.npz")
    j = t % SLICE_TICKS
    x_now = d["states"][:, j + 1].copy()
    if row.recipe == "inf-tick" and t == row.W + 1:
        x_now[0] = 1e200
    return d["states"][:, j].copy(), d["inputs"][:, j].copy(), x_now


def _errors(p, x_prev, u_prev, x_now):
    with np.errstate(all="ignore"):
        return O.lookback_errors(O.evaluate_models_vectorized(shared(), tuple(p), x_prev, u_prev, TS), x_now)


def tie_classes(i, j, N, R):
    """The boundaries the pair (i, j) of equal models crosses, by the look-back's layout: a block is
    256 R models, its row r the 256 at base + 256 r, a wave 64 lanes of a row."""
    per = KBLOCK * R
    out = set()
    if i // per != j // per:
        out.add("block")
    elif (i % per) // KBLOCK != (j % per) // KBLOCK:
        out.add("row")
    elif (i % KBLOCK) // 64 == (j % KBLOCK) // 64:
        out.add("wave")
    else:
        out.add("waves")
    if max(i, j) == N - 1:
        out.add("last")
    return out


def classes_of(row):
    return {"wave", "waves", "block", "last"} | ({"row"} if row.R > 1 else set())


def _plain(N):
    from llampc.mpc import generate_bank
    return generate_bank(N, seed=BANK_SEED.get(N, (N,))[0])


def dup_indices(N, R, best):
    """The indices that take model `best`'s parameters (best itself included)."""
    per = KBLOCK * R
    L = -(-N // per)
    a = best if best < (L - 1) * per else best % per         # an anchor in a full block
    base, r, lane = a // per * per, (a % per) // KBLOCK, a % KBLOCK
    ob = (a // per + 1) % L
    other = ob * per + lane
    idx = {best, a, base + r * KBLOCK + (lane ^ 1), base + r * KBLOCK + (lane + 64) % KBLOCK,
           other if other < N else ob * per, N - 1}
    if R > 1:
        idx.add(base + (r + 1) % R * KBLOCK + lane)
    assert all(0 <= i < N for i in idx), (N, R, best, idx)
    return np.array(sorted(idx))


@functools.lru_cache(maxsize=None)
def dup_source(N, W):
    """The model a dups row copies: the plain bank's oracle argmin of the first full window's mean."""
    row0 = Row("", N, W, 1, "plain", W, 1, 0)
    e = np.array([_errors(_plain(N), *transition(row0, t)) for t in range(W)])
    return int(np.argmin(np.mean(np.ascontiguousarray(e.T), axis=1)))


@functools.lru_cache(maxsize=None)
def _bank(N, recipe, R, W):
    p = _plain(N)
    if recipe == "dups":
        best = dup_source(N, W)
        p[:, dup_indices(N, R, best)] = p[:, [best]]
    elif recipe == "nan":
        p[2, [11, N - 1, N // 2]] = np.nan
    elif recipe == "nan-most":
        keep = np.array([5, 700, 1500, N - 2, N - 1])
        mask = np.ones(N, dtype=bool)
        mask[keep] = False
        p[2, mask] = np.nan
    else:
        assert recipe in ("plain", "inf-tick"), recipe
    p.setflags(write=False)
    return p


def bank_params(row):
    """The row's bank [6, N], read-only."""
    return _bank(row.N, row.recipe, row.R, row.W if row.recipe == "dups" else 0)


def ties_of(row):
    """dups rows: the indices that share the copied model's parameters."""
    p = bank_params(row)
    best = dup_source(row.N, row.W)
    return np.flatnonzero((p == p[:, [best]]).all(axis=0))


@functools.lru_cache(maxsize=None)
def _oracle_errors(N, W, recipe, ticks, R):
    row = Row("", N, W, 1, recipe, ticks, R, 0)
    e = np.array([_errors(bank_params(row), *transition(row, t)) for t in range(ticks)])
    e.setflags(write=False)
    return e


def oracle_errors(row):
    """[ticks, N]: the oracle's look-back errors of every tick of the row, computed once, read-only."""
    return _oracle_errors(row.N, row.W, row.recipe, row.ticks, row.R)


# ------------------------------------------------------------------------------- the stand-in
class FakeBank:
    """NumPy's look-back behind ModelBank's lookback() / window() / reset() surface: the oracle's
    one-step errors, rt.py's rolled window, np.mean, np.argmin / nanargmin, the stable argsort."""

    def __init__(self, params6, W):
        self.params = np.asarray(params6, dtype=np.float64)
        self.n, self.W = self.params.shape[1], int(W)
        self.reset()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def reset(self):
        self.win = np.zeros((self.n, self.W))
        self.window_count = 0

    def window(self):
        return self.win.copy()

    # what the mutants of test_lookback_matrix_cpu.py replace
    def _mean(self, win):
        return np.mean(win, axis=1)

    def _order(self, wm):
        return wm.argsort(kind="stable")

    def _argmin(self, wm, policy):
        if policy == NAN_FIRST:
            return int(np.argmin(wm))
        return int(np.nanargmin(wm)) if not np.isnan(wm).all() else 0

    def lookback(self, x_prev, u_prev, x_now, Ts=TS, K=10, nan_policy=NAN_FIRST, return_errors=False,
                 return_window_mean=False):
        with np.errstate(all="ignore"):
            e = O.lookback_errors(O.evaluate_models_vectorized(shared(), tuple(self.params), x_prev, u_prev, Ts), x_now)
        self.win = np.roll(self.win, -1, axis=1)
        self.win[:, -1] = e
        self.window_count = min(self.window_count + 1, self.W)
        full = self.window_count >= self.W
        best = topk = topv = wm = None
        if full:
            with np.errstate(all="ignore"):
                wm = self._mean(self.win)
            best = self._argmin(wm, nan_policy)
            kk = min(K, self.n)
            topk = np.full(K, -1, dtype=np.int64)
            topk[:kk] = self._order(wm)[:kk]
            topv = np.full(K, np.nan)
            topv[:kk] = wm[topk[:kk]]
        return dict(best=best, topk=topk, topk_val=topv, window_count=self.window_count, full=full,
                    errors=e if return_errors else None, window_mean=wm if return_window_mean else None)


# ------------------------------------------------------------------------------- the checker
def check_window(row, t, prev_win, win, errors):
    """Step 2: the newest column is this tick's errors and the tick wrote no other slot, as bits."""
    N, W = row.N, row.W
    assert win.shape == (N, W)
    count = min(t + 1, W)
    np.testing.assert_array_equal(bits(win[:, -1]), bits(errors), err_msg=f"{row.name} t={t}: newest slot")
    if t > 0:
        # the count - 1 older columns that window_unroll fills are the previous tick's newest count - 1
        np.testing.assert_array_equal(bits(win[:, W - count:W - 1]), bits(prev_win[:, W - count + 1:]),
                                      err_msg=f"{row.name} t={t}: a slot other than the newest changed")


def check_tick(bank, row, t, prev_win, r, oracle_err, policy=NAN_FIRST):
    """One tick's result r (lookback(..., return_errors=True, return_window_mean=True)) of `bank`
    against the oracle's errors of that tick and NumPy.  prev_win: window() after the previous tick
    (None at t = 0).  Returns window(), the next tick's prev_win."""
    N, W, K = row.N, row.W, row.K
    what = f"{row.name} t={t} policy={policy}"
    # 1. the errors against the oracle; infinities with their sign
    close(r["errors"], oracle_err, RTOL_STEP)
    np.testing.assert_array_equal(np.isposinf(r["errors"]), np.isposinf(oracle_err), err_msg=what)
    # 2. the ring
    win = bank.window()
    check_window(row, t, prev_win, win, r["errors"])
    # 5. the count
    count = min(t + 1, W)
    assert r["window_count"] == count == bank.window_count, (what, r["window_count"], bank.window_count)
    assert bool(r["full"]) == (count >= W), what
    if count < W:
        assert r["best"] is None and r["topk"] is None and r["window_mean"] is None, what
        return win
    # 3. the mean's bits
    wm = r["window_mean"]
    with np.errstate(all="ignore"):
        ref = np.mean(win, axis=1)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(wm), nan, err_msg=f"{what}: NaN means")
    np.testing.assert_array_equal(bits(wm)[~nan], bits(ref)[~nan], err_msg=f"{what}: window mean bits vs np.mean")
    # 4. the selection from the path's own means, exact
    kk = min(K, N)
    topk = np.asarray(r["topk"])
    assert topk.shape == (K,), what
    np.testing.assert_array_equal(topk[:kk], wm.argsort(kind="stable")[:K], err_msg=f"{what}: topk")
    assert np.all(topk[kk:] == -1), what
    np.testing.assert_array_equal(bits(np.asarray(r["topk_val"])[:kk]), bits(wm[topk[:kk]]), err_msg=f"{what}: topk_val")
    if policy == NAN_FIRST:
        assert r["best"] == int(np.argmin(wm)), (what, r["best"])
    else:
        assert r["best"] == (int(np.nanargmin(wm)) if not nan.all() else 0), (what, r["best"])
    return win


def run_row(bank, row, policy, ticks=None, keep=None, **kw):
    """Runs the row's ticks on `bank` through check_tick.  keep: a list that takes every tick's result."""
    oe = oracle_errors(row)
    prev = None
    for t in range(row.ticks if ticks is None else ticks):
        r = bank.lookback(*transition(row, t), Ts=TS, K=row.K, nan_policy=policy, return_errors=True,
                          return_window_mean=True, **kw)
        prev = check_tick(bank, row, t, prev, r, oe[t], policy)
        if keep is not None:
            keep.append(r)

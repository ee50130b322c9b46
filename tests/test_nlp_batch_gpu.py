"""setupNLPBatch.solve (llampc_nlp_batch_*, csrc/nlp_batch.hip): B problems of a model bank in one
launch, against oracle.nlp_cem with each problem's own bank column (tests/nlp_batch_cases.py) and
against setupNLP built on that column.  The conditions that keep the comparisons from passing
vacuously or hanging on a rank flip are asserted on the restatement in test_nlp_batch_cpu.py and
again here before every comparison.

Per problem (``check_problem``): umpc bitwise the restatement's, fval at nlp_matrix's RTOL_ROLL =
1e-7; independently of it, xmpc is O.rollout_euler_nlp of the returned umpc with that problem's p6
(RTOL_STEP x 10 = 1e-8, atol 1e-12), fval is O.mpc_cost of that trajectory (RTOL_ROLL), and umpc is
inside the bounds (exactly) and the rates (the restatement's RATE_TOL).

Against the single solver (test_equals_the_single_solver): the batch kernel is the single solve's
kernel template with the problem's words and inputs taken at entry, so umpc, fval AND xmpc are
asserted bitwise; each run prints whether they were (see SINGLE_EXACT below for the run the
exactness was read from)."""
import numpy as np
import pytest

import nlp_batch_cases as BC
import nlp_matrix as M
from oracle import llampc_oracle as O

pytestmark = pytest.mark.gpu

RTOL_STEP = 1e-9
RTOL_ROLL = 1e-7
# fval and xmpc of a batched problem against setupNLP on the same column and seed, read on the
# MI355X over the 12 (shape, problem) pairs of test_equals_the_single_solver
SINGLE_EXACT = True
SINGLE_EXACT_NOTE = ("bitwise in umpc, fval and xmpc for all 12 pairs: relative fval deviation 0, largest |xmpc| "
                     "difference 0 (the module's first MI355X run, profiles/r11/nlp_batch/new_tests_figures.log)")


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


@pytest.fixture()
def bank(nat):
    from llampc.mpc import ModelBank
    with ModelBank(BC.bank(), W=3, device=0) as b:
        yield b


def check_problem(shape, ref, umpc, fval, xmpc, tag=""):
    c = BC.case(shape)
    H = c.H
    dev = abs(fval - ref["j"]) / abs(ref["j"])
    print(f"FVAL_DEV {BC.sid(shape)} model {ref['model']}{tag}: device {fval!r} restated {ref['j']!r} "
          f"relative {dev:.3g} umpc equal {np.array_equal(umpc.T, ref['u'])}")
    assert umpc.shape == (2, H) and xmpc.shape == (6, H + 1)
    np.testing.assert_array_equal(umpc.T, ref["u"])
    np.testing.assert_allclose(fval, ref["j"], rtol=RTOL_ROLL)
    bank6 = tuple(np.array([v]) for v in BC.p6(ref["model"]))
    U = np.ascontiguousarray(umpc.T)[None]
    traj = O.rollout_euler_nlp(M.shared(), bank6, ref["x0"], U, c.Ts)
    np.testing.assert_allclose(xmpc, traj[:, 0, :].T, rtol=RTOL_STEP * 10, atol=1e-12)
    np.testing.assert_allclose(fval, O.mpc_cost(traj, U, ref["xref"], ref["up"], c.Q, c.R, c.P)[0], rtol=RTOL_ROLL)
    assert np.all(umpc >= np.array(c.umin)[:, None]) and np.all(umpc <= np.array(c.umax)[:, None])
    for j, m in enumerate(c.rate_m()):
        if m is not None:
            dd = np.diff(np.concatenate([ref["up"][j:j + 1], umpc[j]]))
            assert np.all(np.abs(dd) <= m * c.Ts * (1.0 + O.RATE_TOL)), (j, np.max(np.abs(dd)))
    return dev


def solve_six(nb, shape, x0=None):
    x, up, xref = BC.inputs(shape)
    return nb.solve(BC.MODELS, x if x0 is None else x0, xref, up, seeds=BC.SEEDS)


@pytest.mark.parametrize("shape", BC.SHAPES, ids=BC.sid)
def test_batch_equals_restatement(bank, shape):
    """1. One batched solve of the six problems per shape; one launch."""
    refs = BC.restate_batch(shape)
    for ref in refs:
        BC.check_conditions(shape, ref)
    nb = BC.batch_solver(shape, bank)
    try:
        before = bank.launches
        umpc, fval, xmpc, ok = solve_six(nb, shape)
        assert bank.launches == before + 1
    finally:
        nb.close()
    assert ok.tolist() == [True] * 6 and umpc.shape == (6, 2, shape[3]) and xmpc.shape == (6, 6, shape[3] + 1)
    devs = [check_problem(shape, refs[p], umpc[p], fval[p], xmpc[p]) for p in range(6)]
    print(f"FVAL_DEV_MAX {BC.sid(shape)}: {max(devs):.3g}")


@pytest.mark.parametrize("shape", BC.SINGLE_SHAPES, ids=BC.sid)
def test_equals_the_single_solver(bank, shape):
    """2. Each problem also equals setupNLP on that bank column with that seed: umpc bitwise, fval
    and xmpc at the restatement's tolerances and — measured: SINGLE_EXACT_NOTE — bitwise."""
    nb = BC.batch_solver(shape, bank)
    try:
        umpc, fval, xmpc, ok = solve_six(nb, shape)
    finally:
        nb.close()
    assert ok.all()
    x0, up, xref = BC.inputs(shape)
    for p, (model, seed) in enumerate(zip(BC.MODELS, BC.SEEDS)):
        one = BC.single_solver(shape, model, seed)
        try:
            u1, f1, x1, _ = one.solve(x0[p], xref[p], up[p])
        finally:
            one.close()
        exact_f, exact_x = f1 == fval[p], np.array_equal(x1, xmpc[p])
        rel = abs(f1 - fval[p]) / abs(f1)
        print(f"SINGLE {BC.sid(shape)} problem {p} model {model}: fval bitwise {exact_f} (relative {rel:.3g}) "
              f"xmpc bitwise {exact_x} (max abs {np.max(np.abs(x1 - xmpc[p])):.3g})")
        np.testing.assert_array_equal(umpc[p], u1)
        np.testing.assert_allclose(fval[p], f1, rtol=RTOL_ROLL)
        np.testing.assert_allclose(xmpc[p], x1, rtol=RTOL_STEP * 10, atol=1e-12)
        if SINGLE_EXACT:
            assert exact_f and exact_x


def test_warm_chain_with_a_changing_model(bank):
    """3. Slot p is a car: its warm start is its own previous umpc shifted, whatever model it uses.
    Slot 0's model goes 0 -> 3 -> 7, slot 1 stays on 11; call = 0, 1, 2."""
    chain = BC.restate_chain()
    for call, refs in enumerate(chain):
        for ref in refs:
            BC.check_conditions(BC.CHAIN_SHAPE, ref, f" chain call {call}")
    nb = BC.batch_solver(BC.CHAIN_SHAPE, bank)
    try:
        for call, (t, models) in enumerate(zip(BC.CHAIN_TICKS, BC.CHAIN_MODELS)):
            x0, up, xref = BC.inputs(BC.CHAIN_SHAPE, (t, t))
            umpc, fval, xmpc, ok = nb.solve(models, x0, xref[0], up, seeds=BC.CHAIN_SEEDS)   # xref shared
            assert ok.all()
            for p in range(2):
                check_problem(BC.CHAIN_SHAPE, chain[call][p], umpc[p], fval[p], xmpc[p], f" call {call} slot {p}")
    finally:
        nb.close()


@pytest.mark.parametrize("shape", [BC.SHAPES[2], BC.SHAPES[3]], ids=BC.sid)
def test_one_problem_alone_equals_it_in_the_batch(bank, shape):
    """4. B = 1 is the same kernel and the same arithmetic: bitwise in umpc, fval and xmpc."""
    x0, up, xref = BC.inputs(shape)
    nb = BC.batch_solver(shape, bank)
    try:
        six = solve_six(nb, shape)
    finally:
        nb.close()
    for p in (0, 3):
        nb = BC.batch_solver(shape, bank)
        try:
            one = nb.solve([BC.MODELS[p]], x0[p:p + 1], xref[p:p + 1], up[p:p + 1], seeds=[BC.SEEDS[p]])
        finally:
            nb.close()
        assert one[3].all() and six[3].all()
        for a, b in zip(one[:3], six[:3]):
            np.testing.assert_array_equal(a[0], b[p])


def test_chunking(bank):
    """5. max_resident = two problems' blocks, B = 5: three launches (2, 2, 1), each consuming one
    solve number; the results are the restatement's with the chunks' call numbers."""
    shape = BC.CHUNK_SHAPE
    refs = BC.restate_chunked()
    for p, ref in enumerate(refs):
        BC.check_conditions(shape, ref, f" chunk call {p // BC.CHUNK_PER_LAUNCH}")
    nb = BC.batch_solver(shape, bank, max_resident=BC.CHUNK_PER_LAUNCH * (shape[0] // 64))
    try:
        assert nb.per_launch == BC.CHUNK_PER_LAUNCH
        x0, up, xref = BC.inputs(shape)
        B = BC.CHUNK_B
        before = bank.launches
        umpc, fval, xmpc, ok = nb.solve(BC.MODELS[:B], x0[:B], xref[:B], up[:B], seeds=BC.SEEDS[:B])
        assert bank.launches == before + 3
    finally:
        nb.close()
    assert ok.all()
    for p in range(B):
        check_problem(shape, refs[p], umpc[p], fval[p], xmpc[p], f" chunk {p // BC.CHUNK_PER_LAUNCH}")


def test_a_failed_problem_stops_no_other(bank):
    """6. Problem 2's state holds a NaN: ok[2] False, umpc zeros, fval inf; every other problem is
    bitwise what it is without the NaN neighbour; the next solve succeeds for all, slot 2 cold."""
    shape = BC.ISO_SHAPE
    first, nxt = BC.restate_isolation()
    for ref in nxt:
        BC.check_conditions(shape, ref, " after the NaN neighbour")
    x0, up, xref = BC.inputs(shape)
    bad = x0.copy()
    bad[BC.ISO_BAD, 2] = np.nan
    nb = BC.batch_solver(shape, bank)
    try:
        clean = solve_six(nb, shape)
    finally:
        nb.close()
    nb = BC.batch_solver(shape, bank)
    try:
        umpc, fval, xmpc, ok = solve_six(nb, shape, bad)
        assert ok.tolist() == [p != BC.ISO_BAD for p in range(6)]
        assert np.all(umpc[BC.ISO_BAD] == 0.0) and fval[BC.ISO_BAD] == np.inf
        for p in range(6):
            if p != BC.ISO_BAD:
                for a, b in zip((umpc, fval, xmpc), clean[:3]):
                    np.testing.assert_array_equal(a[p], b[p])
                check_problem(shape, first[p], umpc[p], fval[p], xmpc[p], " beside the NaN")
        umpc, fval, xmpc, ok = solve_six(nb, shape)
        assert ok.all()
        for p in range(6):
            check_problem(shape, nxt[p], umpc[p], fval[p], xmpc[p], " after the NaN neighbour")
    finally:
        nb.close()


def test_refusals_launch_nothing(nat, bank):
    """7. Argument errors raise before any launch: the bank's launch counter is unchanged."""
    shape = BC.SHAPES[0]
    H = shape[3]
    x0, up, xref = BC.inputs(shape)
    nb = BC.batch_solver(shape, bank, max_batch=4)
    try:
        before = bank.launches
        for models in ([0, -1], [0, BC.N_BANK]):
            with pytest.raises(ValueError, match="models"):
                nb.solve(models, x0[:2], xref[:2], up[:2])
        # the library's own check, below the Python layer's
        st = np.zeros(2, dtype=np.int32)
        hold = np.zeros(2, dtype=np.int32)
        out = (np.zeros((2, H, 2)), np.zeros(2), np.zeros((2, H + 1, 6)))
        for models in ([0, -1], [0, BC.N_BANK]):
            idx = np.array(models, dtype=np.int64)
            rc = nat.load().llampc_nlp_batch_solve(nb._h, 2, idx.ctypes.data, None, x0.ctypes.data, xref.ctypes.data,
                                                    up.ctypes.data, None, hold.ctypes.data, out[0].ctypes.data,
                                                    out[1].ctypes.data, out[2].ctypes.data, st.ctypes.data)
            assert rc == nat.E_ARG
        idx = np.zeros(5, dtype=np.int64)
        st5, hold5 = np.zeros(5, dtype=np.int32), np.zeros(5, dtype=np.int32)
        out5 = (np.zeros((5, H, 2)), np.zeros(5), np.zeros((5, H + 1, 6)))
        for B in (0, 5):                 # B < 1, B above max_batch = 4
            rc = nat.load().llampc_nlp_batch_solve(nb._h, B, idx.ctypes.data, None, x0.ctypes.data, xref.ctypes.data,
                                                    up.ctypes.data, None, hold5.ctypes.data, out5[0].ctypes.data,
                                                    out5[1].ctypes.data, out5[2].ctypes.data, st5.ctypes.data)
            assert rc == nat.E_ARG
        rc = nat.load().llampc_nlp_batch_solve(nb._h, 2, None, None, x0.ctypes.data, xref.ctypes.data, up.ctypes.data,
                                                None, hold.ctypes.data, out[0].ctypes.data, out[1].ctypes.data,
                                                out[2].ctypes.data, st.ctypes.data)
        assert rc == nat.E_ARG
        for kw in (dict(x0=x0[:2, :5]), dict(x0=x0[:3]), dict(xref=xref[:2, :, :H]), dict(xref=xref[:3]),
                   dict(uprev=up[:3]), dict(uprev=up[:2, :1]), dict(seeds=[1, 2, 3]), dict(models=[[0, 1]]),
                   dict(models=[])):
            a = dict(models=[0, 1], x0=x0[:2], xref=xref[:2], uprev=up[:2])
            a.update(kw)
            with pytest.raises(ValueError):
                nb.solve(**a)
        assert bank.launches == before
        # B above max_batch through the Python layer is chunked, not refused: 5 problems, 2 launches
        umpc, fval, xmpc, ok = nb.solve(BC.MODELS[:5], x0[:5], xref[:5], up[:5], seeds=BC.SEEDS[:5])
        assert ok.all() and bank.launches == before + 2
    finally:
        nb.close()
    # max_batch x nl above the CU count: refused at create
    big = BC.SHAPES[2]
    probe = BC.batch_solver(big, bank, max_batch=1)
    cus = probe.cus
    probe.close()
    assert cus >= 96, cus
    with pytest.raises(nat.NativeError, match="exceed") as e:
        BC.batch_solver(big, bank, max_batch=cus // (big[0] // 64) + 1)
    assert e.value.code == nat.E_ARG
    assert bank.launches == before + 2


def test_borrowed_bank_still_plans(nat):
    """8. setupNLPBatch on a bank that also serves plan(): a plan() tick before and after a batched
    solve returns what it returns without the solve, and close() leaves the bank open."""
    from llampc.mpc import ModelBank, plan
    shape = BC.SHAPES[0]
    H, C = shape[3], 4
    x0, up, xref = BC.inputs(shape)
    rng = np.random.RandomState(3)
    U = np.clip(up[0] + 0.05 * rng.randn(C, H, 2), [-0.1, -0.35], [1.0, 0.35])

    def ticks(with_solve):
        got = []
        with ModelBank(BC.bank(), W=1, device=0) as b:
            nb = BC.batch_solver(shape, b) if with_solve else None
            for k in (0, 1, 2):
                if nb is not None and k == 1:
                    assert solve_six(nb, shape)[3].all()
                r = plan(b, x0[k + 1], up[k + 1], x0[k], xref[k + 1], U, Ts=0.02, K=3, return_errors=True,
                         return_costs=True)
                got.append((r.best_model, r.best_cand, r.cost, r.window_full, r.topk, r.lookback_err, r.costs))
            if nb is not None:
                nb.close()
                r = plan(b, x0[4], up[4], x0[3], xref[4], U, Ts=0.02, K=3)     # the bank outlives the solver
                assert r.window_full
        return got

    for a, b in zip(ticks(False), ticks(True)):
        for va, vb in zip(a, b):
            np.testing.assert_array_equal(va, vb)

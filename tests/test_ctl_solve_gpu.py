"""LLAMPC.step (llampc_ctl_step; csrc/ctl_solve.hip, capi_ctl_solve.hip) and LLAMPC.set_applied
(llampc_ctl_set_applied) on the device, against the oracle chain of tests/ctl_solve_cases.py (its
conditions: test_ctl_solve_cpu.py, asserted again here before every comparison).

1. Parity, every row and tick: the tick record passes ctl_matrix.check_tick against the chain's tick;
   umpc equals the chain's u BITWISE; fval within RTOL_ROLL = 1e-7; xmpc is the Euler rollout of the
   returned umpc with the solved model (RTOL_STEP x 10 = 1e-8, atol 1e-12: test_nlp_batch_gpu.py's);
   uprev and model exact; committed follows the chain; umpc inside the bounds (exactly) and the rate
   (the oracle's RATE_TOL).  A step is two counted launches, a plain tick one.
2. Commit == set_applied: a second controller on its own bank runs tick(x_t), then
   set_applied(umpc[:, 0], umpc) with the fused run's umpc (no call on uncommitted ticks): its records
   equal the fused run's tick records bitwise.
3. set_applied against the overridden oracle (the applied input = the chosen u0 + a fixed offset,
   clipped); a control run that is never told must differ in the window means at tick 3.
4. fval <= J0 (1 + RTOL_ROLL) at every committed tick, J0 the oracle's Euler-NLP objective of the
   tick's chosen sequence: sample 0 of round 0 is that sequence, and the device's objective agrees
   with the oracle's to RTOL_ROLL.
5. Every refusal: E_STATE / E_ARG raised, bank.launches unchanged, the next step still the chain's.
6. After close_solver() the controller ticks as one that never had a solver (but for the inputs
   committed before)."""
import numpy as np
import pytest

import ctl_matrix as CM
import ctl_solve_cases as SC
from oracle import llampc_oracle as O
from test_ctl_gpu import _ctl_words, _same_words

pytestmark = pytest.mark.gpu

RTOL_STEP = 1e-9
RTOL_ROLL = CM.RTOL_ROLL


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


def _bank(srow):
    from llampc.mpc import ModelBank
    return ModelBank(np.array(CM.bank(srow.row)), W=srow.row.W, device=0)


def check_solve(srow, t, step, res):
    """One step's solve (res: StepResult) against the chain's."""
    row, o, sol, x = srow.row, step["o"], step["sol"], step["x"]
    tag = f"{srow.name} tick {t}"
    H = row.H
    assert res.umpc.shape == (2, H) and res.xmpc.shape == (6, H + 1), tag
    np.testing.assert_array_equal(res.uprev, o["uprev"], err_msg=tag)
    assert res.model == (-1 if o["warm"] else int(o["best_model"])), (tag, res.model)
    assert res.committed == (sol["u"] is not None) == res.solved, (tag, res.committed, res.status)
    if sol["u"] is None:
        from llampc import _native as nat
        assert res.status == nat.NLP_NO_FINITE and np.isinf(res.fval) and not res.umpc.any(), tag
        assert res.u0 == res.tick.u0, tag
        print(f"STEP {tag}: nothing finite, not committed; the tick's candidate {res.u0} is applied")
        return
    dev = abs(res.fval - sol["j"]) / abs(sol["j"])
    print(f"STEP {tag}: call {sol['call']} fval device {res.fval!r} chain {sol['j']!r} relative {dev:.3g} "
          f"J0 {sol['J0']!r} umpc equal {np.array_equal(res.umpc.T, sol['u'])}")
    np.testing.assert_array_equal(res.umpc.T, sol["u"], err_msg=tag)
    np.testing.assert_allclose(res.fval, sol["j"], rtol=RTOL_ROLL, err_msg=tag)
    assert res.u0 == (sol["u"][0, 0], sol["u"][0, 1]), tag
    U = np.ascontiguousarray(res.umpc.T)[None]
    traj = O.rollout_euler_nlp(CM.shared(), tuple(np.array([v]) for v in sol["p6"]), x, U, row.Ts)
    np.testing.assert_allclose(res.xmpc, traj[:, 0, :].T, rtol=RTOL_STEP * 10, atol=1e-12, err_msg=tag)
    assert np.all(res.umpc >= np.array(row.umin)[:, None]) and np.all(res.umpc <= np.array(row.umax)[:, None]), tag
    for j, m in enumerate(row.rate_max):
        if m is not None and m >= 0:
            dd = np.diff(np.concatenate([o["uprev"][j:j + 1], res.umpc[j]]))
            assert np.all(np.abs(dd) <= m * row.Ts * (1.0 + O.RATE_TOL)), (tag, j, np.max(np.abs(dd)))
    # 4. never worse than the tick's chosen sequence
    assert res.fval <= sol["J0"] * (1.0 + RTOL_ROLL), (tag, res.fval, sol["J0"])


_FUSED = {}


def fused(srow):
    """The row's checked fused run (once per session): per tick (the tick record's words, umpc [2, H]
    or None when nothing was committed)."""
    if srow.name in _FUSED:
        return _FUSED[srow.name]
    steps = SC.chain(srow)
    for t, step in enumerate(steps):
        SC.check_conditions(srow, t, step)
    row = srow.row
    counts = dict(pairs=0, bound=0)
    out = []
    with _bank(srow) as b, SC.controller(srow, b) as ctl:
        projidx = 0
        for t, step in enumerate(steps):
            l0 = b.launches
            if step["sol"] is None:
                res = None
                tick = ctl.tick(step["x"])
                assert b.launches - l0 == 1, (srow.name, t)
            else:
                res = ctl.step(step["x"])
                tick = res.tick
                assert b.launches - l0 == 2, (srow.name, t)
            xref, U = ctl.inputs()
            CM.check_tick(row, t, step["o"], step["x"], tick, xref, U, projidx, counts)
            projidx = tick.raw.projidx
            umpc = None
            if res is not None:
                check_solve(srow, t, step, res)
                umpc = res.umpc.copy() if res.committed else None
                np.testing.assert_array_equal(ctl.u_prev, step["u0"])
            out.append((_ctl_words(tick.raw, row.H), umpc))
    share = counts["bound"] / max(counts["pairs"], 1)
    print(f"{srow.name}: {counts['bound']} of {counts['pairs']} cost pairs passed by the core-error bound ({share:.3f})")
    assert share <= CM.BOUND_SHARE_MAX, (srow.name, counts)
    _FUSED[srow.name] = out
    return out


@pytest.mark.parametrize("srow", SC.ROWS, ids=repr)
def test_step_vs_chain(nat, srow):
    """1 and 4: every tick's record and solve against the chain."""
    fused(srow)


@pytest.mark.parametrize("name", ["base", "nan-selected"])
def test_commit_equals_set_applied(nat, name):
    """2. tick() + set_applied(umpc[:, 0], umpc) leaves the state the fused step's commit leaves."""
    srow = SC.BY_NAME[name]
    want = fused(srow)
    steps = SC.chain(srow)
    assert any(u is None for _, u in want) == (srow.fail_from is not None)
    with _bank(srow) as b, SC.controller(srow, b, solve=False, debug_inputs=False) as ctl:
        for t, (step, (words, umpc)) in enumerate(zip(steps, want)):
            tick = ctl.tick(step["x"])
            _same_words(words, _ctl_words(tick.raw, srow.row.H))
            if umpc is not None:
                l0 = b.launches
                ctl.set_applied(umpc[:, 0], umpc)
                assert b.launches == l0
                np.testing.assert_array_equal(ctl.u_prev, umpc[:, 0])


def test_set_applied_vs_oracle(nat):
    """3. The overridden oracle, tick by tick; and the control run that is never told."""
    srow = SC.BY_NAME["base"]
    row = srow.row
    over = SC.chain(srow, applied=SC.offset_applied(srow))
    counts = dict(pairs=0, bound=0)
    told = []
    with _bank(srow) as b, SC.controller(srow, b, solve=False) as ctl:
        with pytest.raises(nat.NativeError) as e:      # needs a completed tick
            ctl._ctl.set_applied(over[0]["u0"])
        assert e.value.code == nat.E_STATE
        projidx = 0
        for t, step in enumerate(over):
            tick = ctl.tick(step["x"])
            xref, U = ctl.inputs()
            CM.check_tick(row, t, step["o"], step["x"], tick, xref, U, projidx, counts)
            projidx = tick.raw.projidx
            told.append(tick)
            ctl.set_applied(step["u0"])
            for bad in (np.array([np.nan, 0.0]), np.array([0.0, np.inf])):
                with pytest.raises(nat.NativeError) as e:
                    ctl.set_applied(bad)
                assert e.value.code == nat.E_ARG
    with _bank(srow) as b, SC.controller(srow, b, solve=False, debug_inputs=False) as ctl:
        untold = [ctl.tick(step["x"]) for step in over[:4]]
    K = row.K
    for t in range(3):                      # the warm-up records carry no window mean: equal but for the sequences' base
        assert told[t].raw.plan.lb_best == untold[t].raw.plan.lb_best == -1
    a, c = told[3].raw.plan, untold[3].raw.plan
    va, vc = np.ctypeslib.as_array(a.topk_val)[:K], np.ctypeslib.as_array(c.topk_val)[:K]
    print(f"set_applied: tick 3 top-K window means told {va} untold {vc}")
    assert not np.allclose(va, vc, rtol=1e3 * CM.RTOL_MEAN, atol=0), (va, vc)


def test_refusals(nat):
    """5. Each refusal raises, launches nothing, and leaves the next step the chain's."""
    from llampc.mpc import DeviceController
    srow = SC.BY_NAME["base"]
    row = srow.row
    want = fused(srow)
    steps = SC.chain(srow)
    tr, _ = CM.tracks(row.track)
    kw = srow.solve_kw()

    lib = nat.load()
    pg = np.ascontiguousarray(np.array(CM.bank(row)))

    def refused(b, code, word, fn):
        """fn raises `code` with `word` in its message (the refusal meant, not another that happens to
        answer the same code) and the bank has launched nothing."""
        l0 = b.launches
        with pytest.raises(nat.NativeError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), (e.value.code, str(e.value))
        assert b.launches == l0

    def plain(b, **kw_):
        return DeviceController(b, tr, H=row.H, C=row.C, K=row.K, Ts=row.Ts, cost=CM.cost(row), **kw_)

    def mailbox():
        """This process's mailbox of a world of one (its own box is open from its creation)."""
        mb = nat.C.c_void_p()
        nat.check(lib.llampc_mailbox_create(1, 0, 0, nat.C.byref(mb)))
        return mb

    def still_ticks(dc):
        """The refused controller's next tick is the chain's tick 0 (no solver: there is no step)."""
        _same_words(want[0][0], _ctl_words(dc.tick(steps[0]["x"]), row.H))

    # create: prelaunch on, a corridor weight, an exchange, a gather transport, a cfg that is not the controller's
    with _bank(srow) as b:
        dc = plain(b, prelaunch=True)
        refused(b, nat.E_STATE, "armed launches", lambda: dc.attach_solver(**kw))
        dc.set_prelaunch(False)
        dc.H = row.H + 1                     # attach_solver takes the controller's H: pretend another
        refused(b, nat.E_ARG, "H must equal", lambda: dc.attach_solver(**kw))
        dc.H = row.H
        refused(b, nat.E_ARG, "samples", lambda: dc.attach_solver(**dict(kw, samples=8192)))
        dc.attach_solver(**kw)
        refused(b, nat.E_STATE, "already has a solver", lambda: dc.attach_solver(**kw))
        dc.close()
    with _bank(srow) as b:
        dc = plain(b, corridor_weight=1.0)
        refused(b, nat.E_STATE, "no corridor ticks", lambda: dc.attach_solver(**kw))
        dc.close()
    with _bank(srow) as b:
        dc, mb = plain(b), mailbox()
        try:
            nat.check(lib.llampc_ctl_set_exchange(dc._h, mb, nat.dptr(pg), pg.shape[1]))
            refused(b, nat.E_STATE, "unsharded", lambda: dc.attach_solver(**kw))
            still_ticks(dc)
        finally:
            dc.close()
            lib.llampc_mailbox_destroy(mb)
    with _bank(srow) as b:
        dc = plain(b)
        nat.check(lib.llampc_ctl_set_gather(dc._h, 1, 0, None, nat.dptr(pg), pg.shape[1]))
        refused(b, nat.E_STATE, "unsharded", lambda: dc.attach_solver(**kw))
        still_ticks(dc)
        dc.close()
    # attached: the setters refuse between the chain's steps — each with the solver's own message: from
    # tick 1 on both transports would be refused anyway ("before the first tick") — and the chain goes
    # on unchanged
    mb = mailbox()
    try:
        with _bank(srow) as b, SC.controller(srow, b, debug_inputs=False) as ctl:
            h = ctl._ctl._h
            for t, (step, (words, umpc)) in enumerate(zip(steps, want)):
                if t in (0, 2, 5):
                    refused(b, nat.E_STATE, "a solver is attached", lambda: ctl.set_prelaunch(True))
                    refused(b, nat.E_STATE, "a solver is attached", lambda: ctl.set_corridor(1.0, 0.0))
                    refused(b, nat.E_STATE, "a solver is attached: the fused step is unsharded (set_exchange)",
                            lambda: nat.check(lib.llampc_ctl_set_exchange(h, mb, nat.dptr(pg), pg.shape[1])))
                    refused(b, nat.E_STATE, "a solver is attached: the fused step is unsharded (set_gather)",
                            lambda: nat.check(lib.llampc_ctl_set_gather(h, 1, 0, None, nat.dptr(pg), pg.shape[1])))
                    ctl.set_prelaunch(False)     # off stays allowed
                res = ctl.step(step["x"])
                _same_words(words, _ctl_words(res.tick.raw, row.H))
                np.testing.assert_array_equal(res.umpc, umpc)
    finally:
        lib.llampc_mailbox_destroy(mb)
    # a controller without a solver has no step
    with _bank(srow) as b, SC.controller(srow, b, solve=False, debug_inputs=False) as ctl:
        refused(b, nat.E_STATE, "needs", lambda: ctl.step(steps[0]["x"]))


def test_borrowed_controller_still_ticks(nat):
    """6. Four fused steps, close_solver(), then plain ticks: the records of a controller that never had
    a solver and was told the same applied inputs."""
    srow = SC.BY_NAME["base"]
    steps = SC.chain(srow)
    want = fused(srow)
    H, cut = srow.row.H, 4
    with _bank(srow) as b, SC.controller(srow, b, debug_inputs=False) as ctl:
        for step in steps[:cut]:
            ctl.step(step["x"])
        ctl.close_solver()
        with pytest.raises(nat.NativeError):
            ctl.step(steps[cut]["x"])
        got = [_ctl_words(ctl.tick(step["x"]).raw, H) for step in steps[cut:]]
        ctl.set_prelaunch(True)              # allowed again
    with _bank(srow) as b, SC.controller(srow, b, solve=False, debug_inputs=False) as ctl:
        for step, (_, umpc) in zip(steps[:cut], want):
            ctl.tick(step["x"])
            ctl.set_applied(umpc[:, 0], umpc)
        ref = [_ctl_words(ctl.tick(step["x"]).raw, H) for step in steps[cut:]]
    for a, c in zip(got, ref):
        _same_words(a, c)
    # and they are not the fused run's from the second plain tick on: tick 4's solve improved on the
    # tick's candidate (test_ctl_solve_cpu.py prints fval < J0 there) and was not run here
    assert steps[cut]["sol"]["j"] < steps[cut]["sol"]["J0"]
    assert not np.array_equal(got[1][-1], want[cut + 1][0][-1])

"""The NLP entries' host path against itself (csrc/capi_nlp.hip, csrc/capi_nlp_batch.hip over capi_host.hpp's
NLP section and capi_common.hpp's TrackTables / BankIdle): refused calls leave no trace in the call number or
the tags, a replaced track table is the table a fresh object holds (all four owners of track tables), every
entry is refused while an async plan tick is outstanding on the bank, and the single and the batched track
solve share one built-corridor step.  Everything is compared bitwise with a twin object that saw only the good
calls, so the module holds on any library whose entries behave as documented in include/llampc.h.

The smallest shapes that reach the paths: samples 64 (one block per problem), elite 4, two rounds, H = 3; the
single solver on its one-model bank, the batched one on a three-model bank with max_batch = B = 2; the
four-point square track of plan_track_cases and the same square with its midpoints (eight points, shifted and
narrower) as the replacement."""

import numpy as np
import pytest

import nlp_batch_cases as BC
import nlp_matrix as M
import plan_track_cases as PC

pytestmark = pytest.mark.gpu

SHAPE = (64, 4, 2, 3)                    # samples, elite, iters, H
H = SHAPE[3]
SEED = 5
TICKS, MODELS = (20, 21), (0, 2)
WEIGHT, MARGIN = 10.0, 0.2
BUSY = "an async tick is outstanding on the bank"


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


def tables(track, doubled=False):
    """(centre [2, n], theta [n], length, width) of the track; doubled: 2 n points — every segment's midpoint
    added, the line shifted by 0.1 and the width 2.0, so that a stale table or width shows in a corridor."""
    from llampc.mpc import constraints
    c, th, L, w = constraints.track_tables(track)
    if not doubled:
        return c, th, L, w
    n = c.shape[1]
    c2, th2 = np.empty((2, 2 * n)), np.empty(2 * n)
    c2[:, 0::2], th2[0::2] = c, th
    c2[:, 1::2] = (c + np.roll(c, -1, axis=1)) / 2
    th2[1::2] = (th + np.append(th[1:], L)) / 2
    return np.ascontiguousarray(c2 + 0.1), th2, L, 2.0


def set_track(lib, fn, handle, tab):
    c, th, L, w = tab
    return getattr(lib, fn)(handle, c.ctypes.data, th.ctypes.data, c.shape[1], L, w)


def inputs(B):
    x0, up, xref = BC.inputs(SHAPE, TICKS[:B])
    return np.ascontiguousarray(x0), np.ascontiguousarray(up), np.ascontiguousarray(xref)


class Single:
    """llampc_nlp_* on setupNLP's handle (bank column MODELS[0], seed SEED): B = 1 arrays in, arrays out."""
    B, track_fn = 1, "llampc_nlp_set_track"

    def __init__(self, nat):
        self.nat, self.lib = nat, nat.load()
        self.obj = BC.single_solver(SHAPE, MODELS[0], SEED)
        self.obj._ensure()
        self.h, self.bank = self.obj._h, self.obj._bank
        self.x0, self.up, self.xref = inputs(1)

    def close(self):
        self.obj.close()

    def outs(self):
        return dict(umpc=np.full((1, H, 2), np.nan), fval=np.full(1, np.nan), xmpc=np.full((1, H + 1, 6), np.nan),
                    slack=np.full(1, np.nan), hp=np.full((1, H, 6), np.nan))

    def call(self, kind, base=None, hp=None, weight=WEIGHT, path=None, margin=MARGIN):
        o = self.outs()
        a = (self.h, self.x0.ctypes.data, self.xref.ctypes.data, self.up.ctypes.data,
             None if base is None else base.ctypes.data, int(base is not None))
        r = (o["umpc"].ctypes.data, o["fval"].ctypes.data, o["xmpc"].ctypes.data)
        if kind == "solve":
            rc = self.lib.llampc_nlp_solve(*a, *r)
        elif kind == "corridor":
            rc = self.lib.llampc_nlp_solve_corridor(*a, hp.ctypes.data, float(weight), *r, o["slack"].ctypes.data)
        else:
            rc = self.lib.llampc_nlp_solve_track(*a, path.ctypes.data, float(margin), float(weight), *r,
                                                 o["slack"].ctypes.data, o["hp"].ctypes.data)
        return rc, o

    def track_corridor(self, path, margin=MARGIN):
        hp, th = np.full((1, H, 6), np.nan), np.full((1, H), np.nan)
        return self.lib.llampc_nlp_track_corridor(self.h, path.ctypes.data, float(margin), hp.ctypes.data, th.ctypes.data), hp, th


class Batch:
    """llampc_nlp_batch_* on setupNLPBatch's handle over a three-model bank, max_batch = B."""
    track_fn = "llampc_nlp_batch_set_track"

    def __init__(self, nat, B=2):
        from llampc.mpc import ModelBank
        self.nat, self.lib, self.B = nat, nat.load(), B
        self.bank = ModelBank(np.ascontiguousarray(BC.bank()[:, :3]), W=3, device=0)
        self.obj = BC.batch_solver(SHAPE, self.bank, max_batch=B)
        self.h = self.obj._h
        self.x0, self.up, self.xref = inputs(B)
        self.models = np.array(MODELS[:B], dtype=np.int64)
        self.seeds = np.full(B, SEED, dtype=np.uint64)

    def close(self):
        self.obj.close()
        self.bank.close()

    def outs(self):
        B = self.B
        return dict(umpc=np.full((B, H, 2), np.nan), fval=np.full(B, np.nan), xmpc=np.full((B, H + 1, 6), np.nan),
                    slack=np.full(B, np.nan), hp=np.full((B, H, 6), np.nan), status=np.full(B, -1, dtype=np.int32))

    def call(self, kind, base=None, hp=None, weight=WEIGHT, path=None, margin=MARGIN):
        o = self.outs()
        hold = np.full(self.B, int(base is not None), dtype=np.int32)
        w = np.full(self.B, float(weight))
        a = (self.h, self.B, self.models.ctypes.data, self.seeds.ctypes.data, self.x0.ctypes.data, self.xref.ctypes.data,
             self.up.ctypes.data, None if base is None else base.ctypes.data, hold.ctypes.data)
        r = (o["umpc"].ctypes.data, o["fval"].ctypes.data, o["xmpc"].ctypes.data, o["status"].ctypes.data)
        if kind == "solve":
            rc = self.lib.llampc_nlp_batch_solve(*a, *r)
        elif kind == "corridor":
            rc = self.lib.llampc_nlp_batch_solve_corridor(*a, hp.ctypes.data, w.ctypes.data, *r, o["slack"].ctypes.data)
        else:
            rc = self.lib.llampc_nlp_batch_solve_track(*a, path.ctypes.data, float(margin), w.ctypes.data, *r,
                                                       o["slack"].ctypes.data, o["hp"].ctypes.data)
        return rc, o

    def track_corridor(self, path, margin=MARGIN):
        hp, th = np.full((self.B, H, 6), np.nan), np.full((self.B, H), np.nan)
        return (self.lib.llampc_nlp_batch_track_corridor(self.h, self.B, path.ctypes.data, float(margin), hp.ctypes.data,
                                                         th.ctypes.data), hp, th)


def make(nat, kind, **kw):
    return Single(nat) if kind == "single" else Batch(nat, **kw)


def same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs\n{a[k]}\n{b[k]}"


def warm(umpc):
    """The next solve's warm start of every problem: its solution [B, H, 2] shifted one step."""
    return np.ascontiguousarray(np.stack([M.warm(u) for u in umpc]))


def good_pair(s, between=None):
    """A cold plain solve, then (after `between`) the track set and a warm track solve along xref: the two
    solves' outputs.  Launches: one per search, one more for the corridor kernel."""
    n0 = s.bank.launches
    rc, first = s.call("solve")
    assert rc == 0 and np.isfinite(first["fval"]).all(), s.lib.llampc_last_error()
    assert s.bank.launches == n0 + 1
    if between:
        between(s)
    assert s.bank.launches == n0 + 1, "a refused call launches nothing"
    assert set_track(s.lib, s.track_fn, s.h, tables(PC.track("square"))) == 0
    if between:
        between(s, tracked=True)
    assert s.bank.launches == n0 + 1
    rc, last = s.call("track", base=warm(first["umpc"]), path=s.xref)
    assert rc == 0 and np.isfinite(last["fval"]).all() and np.isfinite(last["hp"]).all(), s.lib.llampc_last_error()
    assert s.bank.launches == n0 + 3
    return first, last


@pytest.fixture(scope="module")
def twins(nat):
    """kind -> the two good solves of an object that saw nothing else."""
    out = {}
    for kind in ("single", "batch"):
        s = make(nat, kind)
        try:
            out[kind] = good_pair(s)
        finally:
            s.close()
    return out


@pytest.mark.parametrize("kind", ["single", "batch"])
def test_refused_calls_leave_no_trace(nat, twins, kind):
    """solve; a corridor solve with a negative weight, a track solve without a track; set_track; a track solve
    with margin = width / 2; a track solve: its outputs are the twin's bitwise, so no refused call advanced
    the call number (the Philox counter and the tags) or wrote a buffer the next solve reads."""
    err = lambda s: s.lib.llampc_last_error().decode()
    hp = np.tile(np.array([1.0, 0.0, 10.0, 0.0, 1.0, 10.0]), (2, H, 1))

    def between(s, tracked=False):
        if not tracked:
            rc, _ = s.call("corridor", hp=hp, weight=-1.0)
            assert rc == nat.E_ARG and err(s).endswith("weight must be finite and >= 0"), err(s)
            rc, _ = s.call("track", path=s.xref)
            assert rc == nat.E_STATE and err(s) == f"no track set: call {s.track_fn} first"
        else:
            rc, _ = s.call("track", path=s.xref, margin=1.2)
            assert rc == nat.E_ARG and err(s) == "margin 1.2 leaves no corridor (track width 2.4)"
            rc, _, _ = s.track_corridor(s.xref, margin=1.2)
            assert rc == nat.E_ARG and err(s) == "margin 1.2 leaves no corridor (track width 2.4)"
    s = make(nat, kind)
    try:
        first, last = good_pair(s, between)
    finally:
        s.close()
    same(first, twins[kind][0], f"{kind}: the first solve")
    same(last, twins[kind][1], f"{kind}: the solve after the refused calls")
    # the second solve is not the first again: the call number and the warm start are in it
    assert last["umpc"].tobytes() != first["umpc"].tobytes()


@pytest.mark.parametrize("kind", ["single", "batch"])
def test_bank_busy(nat, twins, kind):
    """With llampc_plan_async outstanding on the solver's bank every entry that needs the bank idle returns
    LLAMPC_E_STATE with one message and launches nothing; after llampc_plan_wait the solver is where a
    fresh one is."""
    s = make(nat, kind)
    try:
        lib = s.lib
        assert set_track(lib, s.track_fn, s.h, tables(PC.track("square"))) == 0
        x_prev, u_prev, x_t, uprev, U, xref = PC.tick_inputs(0, 2, H)
        s.bank.plan_async(x_prev, u_prev, x_t, U, xref, uprev, Ts=PC.TS, K=1, do_lookback=False)
        n0 = s.bank.launches
        hp = np.tile(np.array([1.0, 0.0, 10.0, 0.0, 1.0, 10.0]), (2, H, 1))
        doubled = tables(PC.track("square"), doubled=True)
        got = []
        for f in (lambda: s.call("solve"), lambda: s.call("corridor", hp=hp), lambda: s.call("track", path=s.xref),
                  lambda: s.track_corridor(s.xref), lambda: (set_track(lib, s.track_fn, s.h, doubled),)):
            got.append((f()[0], lib.llampc_last_error().decode()))
        assert got == [(nat.E_STATE, BUSY)] * 5, got
        assert s.bank.launches == n0
        s.bank.plan_wait()
        first, last = good_pair(s)
    finally:
        s.close()
    same(first, twins[kind][0], f"{kind}: the first solve after the wait")
    same(last, twins[kind][1], f"{kind}: the track solve after the wait")


def test_single_and_batched_track_solves_agree(nat, twins):
    """B = 1 on the same bank column, seed, inputs, path, margin and weight: the same hp_out and max_slack
    bitwise (one built-corridor step), and the same solve."""
    s = Batch(nat, B=1)
    try:
        first, last = good_pair(s)
    finally:
        s.close()
    one = twins["single"][1]
    assert last["hp"].tobytes() == one["hp"].tobytes() and last["slack"].tobytes() == one["slack"].tobytes()
    assert last["slack"][0] > 0, "the corridor along xref costs the returned trajectory nothing: nothing compared"
    for k in ("umpc", "fval", "xmpc"):
        assert last[k].tobytes() == one[k].tobytes(), k
    assert last["status"].tolist() == [nat.NLP_OK]


# ---- replacing the track: n points, 2 n points, the first again — against an object that saw only the first ----
def replaced(lib, fn, handle, track, again):
    """The n-point table; `again`: then the doubled one and the first once more (reserve's grow, then reuse)."""
    seq = (False, True, False) if again else (False,)
    for doubled in seq:
        rc = set_track(lib, fn, handle, tables(track, doubled))
        assert rc == 0, lib.llampc_last_error()


@pytest.mark.parametrize("kind", ["single", "batch"])
def test_replacing_the_track_nlp(nat, kind):
    got = []
    for again in (True, False):
        s = make(nat, kind)
        try:
            replaced(s.lib, s.track_fn, s.h, PC.track("square"), again)
            if again:                    # the doubled table really is another track
                assert set_track(s.lib, s.track_fn, s.h, tables(PC.track("square"), True)) == 0
                other = s.track_corridor(s.xref)
                assert set_track(s.lib, s.track_fn, s.h, tables(PC.track("square"))) == 0
            rc, hp, th = s.track_corridor(s.xref)
            assert rc == 0 and np.isfinite(hp).all() and np.isfinite(th).all(), s.lib.llampc_last_error()
            got.append((hp, th))
        finally:
            s.close()
    assert other[0] == 0 and other[1].tobytes() != got[0][0].tobytes()
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()


def test_replacing_the_track_bank(nat):
    """llampc_bank_set_track, read back through one seeded track tick (llampc_bank_track_corridor)."""
    from llampc.mpc import ModelBank
    lib = nat.load()
    C = 2
    x_prev, u_prev, x_t, uprev, U, xref = PC.tick_inputs(0, C, H)
    got = []
    for again in (True, False):
        with ModelBank(np.ascontiguousarray(BC.bank()[:, :3]), W=2, device=0) as b:
            b.set_track(PC.track("square"))
            if again:
                replaced(lib, "llampc_bank_set_track", b.handle, PC.track("square"), True)
            b.set_corridor_path(xref)
            b.plan_raw(x_prev, u_prev, x_t, U, xref, uprev, Ts=PC.TS, K=1, do_lookback=False, current_model=0,
                       track_corridor=True, corridor_weight=WEIGHT, corridor_margin=MARGIN)
            rb = b.track_corridor()
            assert rb["valid"] and np.isfinite(rb["hp"]).all()
            got.append(rb)
    for k in got[0]:
        assert np.asarray(got[0][k]).tobytes() == np.asarray(got[1][k]).tobytes(), k


def test_replacing_the_track_controller(nat):
    """llampc_ctl_set_track (the corridor off), read back after the second corridor tick, the first with a
    path (llampc_ctl_corridor)."""
    from llampc.mpc import DeviceController, ModelBank, generate_bank
    from llampc.params import ORCA
    from test_ctl_gpu import start_state, tracks
    lib = nat.load()
    tr, _ = tracks("ETHZ")
    nominal = [ORCA()[k] for k in ("Bf", "Cf", "Df", "Br", "Cr", "Dr")]
    x0 = start_state("ETHZ", tr)
    got = []
    for again in (True, False):
        with ModelBank(generate_bank(64, seed=3), W=3, device=0) as b:
            c = DeviceController(b, tr, H=4, C=2, K=2, nominal6=nominal)
            try:
                replaced(lib, "llampc_ctl_set_track", c._h, tr, again)
                c._has_track = True
                c.set_corridor(100.0, 0.0)
                c.tick(x0)
                c.tick(x0)
                path, hp, theta, valid = c.corridor()
                assert valid and np.isfinite(hp).all()
                got.append((path, hp, theta))
            finally:
                c.close()
    for a, b_ in zip(*got):
        assert a.tobytes() == b_.tobytes()

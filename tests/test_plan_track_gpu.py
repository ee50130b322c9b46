"""The track tick on the device (llampc_plan_track: the corridor built inside the plan launch, chained
from tick to tick by the controller's path rule) against a twin bank that takes the read-back rows
through llampc_plan_corridor, and against the oracle (cases, margins and oracle chain:
plan_track_cases.py).

Both banks run lookahead_block<RK4, STAGE, LPM, 0, 0, CORR>'s rollouts with hp in LDS, so the record's
bytes, the costs, the look-back errors and the window means are compared BITWISE; the rows are held to
constraints.track_corridor within 1e-12 (the device builder's figure, corridor_dev.hpp) and the path to
the oracle's RK4 positions within 1e-6 (the controller corridor test's path tolerance).

One assertion of the issue is not made: "X_0 == x_t exactly where H >= 2 reads it back".  The path
state and its read-back hold P_j = X[ctl_path_index(j, H)], whose index is at least 1 at every H, so
X_0 is in neither."""
import numpy as np
import pytest

import plan_track_cases as PC
from test_lookahead_matrix_gpu import F8, feasibility_inputs, nat  # noqa: F401
from test_lookahead_matrix_gpu import RATE_PWM, RATE_STEER

pytestmark = pytest.mark.gpu

TS, K, W, N = PC.TS, PC.K, PC.W, PC.N
HP_ATOL, PATH_ATOL = 1e-12, 1e-6
STAGED = {PC.S: True, PC.UW: False, PC.H1: True, PC.HM: True}


def raw(out):
    return bytes(out)


def same_record(nat, a, b, what):
    if raw(a) != raw(b):
        da, db = nat.plan_out_to_dict(a), nat.plan_out_to_dict(b)
        diff = {k: (da[k], db[k]) for k in da if not np.array_equal(np.asarray(da[k]), np.asarray(db[k]), equal_nan=True)}
        raise AssertionError(f"{what}: records differ: {diff}")


def tick_kw(t, record_only):
    return dict(Ts=TS, K=K, do_lookback=t >= 1, current_model=0, return_errors=not record_only,
                return_window_mean=not record_only, return_costs=not record_only)


def run_chain(nat, shape, track_name, ticks, lpm=None):
    """`ticks` closed-loop ticks on bank A (track ticks) and its twin B (the read-back rows through
    plan_raw(corridor=)), with every assertion of the chain test; returns the read-backs."""
    from llampc.mpc import ModelBank, constraints
    C, H = shape
    key = (shape, track_name)
    row, tr = PC.CHAIN[key], PC.track(track_name)
    tn = tr.center_line.shape[1]
    v = nat.plan_variant_track(N, C, H, tn)
    assert v["nb_cor"] == H and v["stage"] == STAGED[shape] and (lpm is None or v["lpm"] == lpm), v
    # the preconditions, on the oracle alone, before the device runs
    outs = PC.oracle_chain(*key)
    shares = [o["share"] for o in outs[1:]]
    assert sum(0.1 <= s <= 0.9 for s in shares) >= 2
    if track_name == "ETHZ" and shape in (PC.S, PC.UW):
        assert any(o["moved"] for o in outs)
    w = row["weight"]
    rbs, prev = [], None
    with ModelBank(PC.bank(), W=W, device=0) as A, ModelBank(PC.bank(), W=W, device=0) as B:
        A.set_track(tr)
        for t in range(ticks):
            x_prev, u_prev, x_t, uprev, U, xref = PC.tick_inputs(t, C, H)
            record_only = t % 2 == 1
            kw = tick_kw(t, record_only)
            margin = row["margins"][t]
            n0 = A.launches
            oa, ea, wa, ca = A.plan_raw(x_prev, u_prev, x_t, U, xref, uprev, track_corridor=True, corridor_weight=w,
                                        corridor_margin=margin, **kw)
            assert A.launches == n0 + 1, "one launch per tick"
            rb = A.track_corridor()
            ob, eb, wb, cb = B.plan_raw(x_prev, u_prev, x_t, U, xref, uprev, corridor=rb["hp"], corridor_weight=w, **kw)
            o = nat.plan_out_to_dict(oa)
            print(f"TRACK {shape} {track_name} lpm {v['lpm']} tick {t}: valid {int(rb['valid'])} sel {o['sel_model']}/"
                  f"{o['sel_cand']} cost {o['sel_cost']:.6g} next_valid {int(rb['next_valid'])} window {o['window_count']}")
            assert o["status"] == 0 and o["window_count"] == min(t, W) and o["window_full"] == int(t >= W)
            same_record(nat, oa, ob, f"tick {t}")
            if not record_only:
                assert ca.tobytes() == cb.tobytes(), f"tick {t}: costs differ in {np.count_nonzero(ca != cb)} entries"
                if t >= 1:
                    assert ea.tobytes() == eb.tobytes()
                if t >= W:
                    assert wa.tobytes() == wb.tobytes()
            # the read-back
            assert rb["valid"] == (t >= 1)
            if t == 0:
                assert rb["hp"].tobytes() == constraints.disabled(H).tobytes()
                assert np.isnan(rb["path"]).all()
            else:
                assert rb["path"].tobytes() == prev["next_path"].tobytes(), "the path is the one the tick before left"
                want = constraints.track_corridor(tr, rb["path"], margin)
                assert np.max(np.abs(rb["hp"] - want)) <= HP_ATOL, np.max(np.abs(rb["hp"] - want))
            assert rb["next_valid"] and o["sel_owned"] == 1 and 0 <= o["sel_cand"] < C
            assert np.float64(rb["next_cost"]).tobytes() == np.float64(o["sel_cost"]).tobytes(), (rb["next_cost"], o["sel_cost"])
            X = PC.chosen_positions(x_t, U, int(o["sel_model"]), int(o["sel_cand"]))
            assert np.max(np.abs(rb["next_path"] - PC.shifted(X, H))) <= PATH_ATOL
            rbs.append(rb)
            prev = rb
    return rbs


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


# ----------------------------------------------------------------- 1. the chain against a twin
@pytest.mark.parametrize("lpm,shape", [(4, PC.S), (2, PC.S), (1, PC.S), (1, PC.UW)], ids=_ids)
def test_chain_against_twin(nat, monkeypatch, lpm, shape):
    """Six ticks with W = 2: tick 0 without a look-back (no look-back block: the ticket completion),
    tick 1 with a window that is not full, ticks 2.. polled; record-only ticks alternate with ticks
    that copy the outputs back.  (64, 40) at LPM 1: the look-ahead unstaged."""
    monkeypatch.setenv("LLAMPC_LPM", str(lpm))
    rbs = run_chain(nat, shape, "ETHZ", PC.TICKS, lpm)
    assert [int(r["valid"]) for r in rbs] == [0, 1, 1, 1, 1, 1]


# ----------------------------------------------------------------- 2. edges
def test_edge_single_step(nat, monkeypatch):
    """H = 1: one corridor block, P_0 = P_1 = X_1."""
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    rbs = run_chain(nat, PC.H1, "ETHZ", 2)
    for r in rbs:
        assert r["next_path"][:, 0].tobytes() == r["next_path"][:, 1].tobytes()


def test_edge_longest_horizon(nat, monkeypatch):
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    assert PC.HM[1] == nat.HMAX
    run_chain(nat, PC.HM, "ETHZ", 2)


def test_edge_four_point_track(nat, monkeypatch):
    """A centre line of four points: 252 of a corridor block's 256 lanes hold no segment."""
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    run_chain(nat, PC.S, "square", 2)


# ----------------------------------------------------------------- 3. validity on the device
def _tick(b, t, shape, **kw):
    x_prev, u_prev, x_t, uprev, U, xref = PC.tick_inputs(t, *shape)
    return b.plan_raw(x_prev, u_prev, x_t, U, xref, uprev, **{**tick_kw(t, False), **kw})


def test_all_infeasible_leaves_no_path(nat, monkeypatch):
    """Every candidate infeasible under enforce_bounds: sel_cost = +inf, no valid path; the following
    track tick runs on the disabled rows, bitwise the twin's under constraints.disabled."""
    from llampc.mpc import ModelBank, constraints
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    C, H = F8
    x0, uprev, U, xref = feasibility_inputs(C, H, TS, all_infeasible=True)
    cs = nat.cost_struct(rate_max=(RATE_PWM, RATE_STEER), enforce_bounds=True)
    with ModelBank(PC.bank(), W=W, device=0) as A, ModelBank(PC.bank(), W=W, device=0) as B:
        A.set_track(PC.track())
        A.set_corridor_path(np.tile(x0[:2, None], (1, H + 1)))          # a path is on offer: the tick builds live rows
        out, _, _, costs = A.plan_raw(np.zeros(6), np.zeros(2), x0, U, xref, uprev, Ts=TS, K=K, do_lookback=False, cost=cs,
                                      return_costs=True, track_corridor=True, corridor_margin=0.05)
        o = nat.plan_out_to_dict(out)
        rb = A.track_corridor()
        assert rb["valid"] and np.isposinf(costs).all() and np.isposinf(o["sel_cost"]) and o["sel_owned"] == 1
        assert not rb["next_valid"]
        oa, _, _, ca = _tick(A, 0, F8, track_corridor=True, corridor_margin=0.05)
        rb = A.track_corridor()
        assert not rb["valid"] and rb["hp"].tobytes() == constraints.disabled(H).tobytes() and rb["next_valid"]
        ob, _, _, cb = _tick(B, 0, F8, corridor=constraints.disabled(H))
        same_record(nat, oa, ob, "after an all-infeasible tick")
        assert ca.tobytes() == cb.tobytes()


def test_plain_tick_invalidates_and_seed_validates(nat, monkeypatch):
    """A plain plan_raw between two track ticks invalidates the path; set_corridor_path(P) seeds one (the
    rows within 1e-12 of track_corridor along P); set_corridor_path(None) invalidates it."""
    from llampc.mpc import ModelBank, constraints
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    C, H = PC.S
    tr = PC.track()
    margin = 0.03
    with ModelBank(PC.bank(), W=W, device=0) as A:
        A.set_track(tr)
        _tick(A, 0, PC.S, track_corridor=True, corridor_margin=margin)
        assert A.track_corridor()["next_valid"]
        _tick(A, 1, PC.S)                                              # a plain tick
        with pytest.raises(nat.NativeError) as ei:
            A.track_corridor()
        assert ei.value.code == nat.E_STATE
        _tick(A, 2, PC.S, track_corridor=True, corridor_margin=margin)
        rb = A.track_corridor()
        assert not rb["valid"] and rb["hp"].tobytes() == constraints.disabled(H).tobytes() and rb["next_valid"]
        _tick(A, 3, PC.S, track_corridor=True, corridor_margin=margin)
        assert A.track_corridor()["valid"]
        # a seeded path
        P = np.ascontiguousarray(PC.tick_inputs(4, C, H)[5]) + 0.01
        A.set_corridor_path(P)
        _tick(A, 4, PC.S, track_corridor=True, corridor_margin=margin)
        rb = A.track_corridor()
        assert rb["valid"] and rb["path"].tobytes() == P.tobytes()
        assert np.max(np.abs(rb["hp"] - constraints.track_corridor(tr, P, margin))) <= HP_ATOL
        # ... of another horizon is not offered
        A.set_corridor_path(P[:, :H])
        _tick(A, 5, PC.S, track_corridor=True, corridor_margin=margin)
        assert not A.track_corridor()["valid"]
        A.set_corridor_path(P)
        A.set_corridor_path(None)
        _tick(A, 5, PC.S, track_corridor=True, corridor_margin=margin)
        assert not A.track_corridor()["valid"]
        # reset and set_track clear it too
        A.reset()
        _tick(A, 0, PC.S, track_corridor=True, corridor_margin=margin)
        assert not A.track_corridor()["valid"]
        A.set_track(tr)
        _tick(A, 0, PC.S, track_corridor=True, corridor_margin=margin)
        assert not A.track_corridor()["valid"]
        _tick(A, 0, PC.S, track_corridor=True, corridor_margin=margin)
        assert A.track_corridor()["valid"]


def test_shard_that_does_not_own_the_selection(nat, monkeypatch):
    """global_offset > 0, the current model outside the shard: sel_owned = 0 and no path."""
    from llampc.mpc import ModelBank
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    C, H = PC.S
    with ModelBank(PC.bank(), W=W, device=0, global_offset=1000) as A:
        A.set_track(PC.track())
        out, _, _, _ = _tick(A, 0, PC.S, track_corridor=True, corridor_margin=0.03)
        o = nat.plan_out_to_dict(out)
        assert o["sel_model"] == 0 and o["sel_owned"] == 0
        rb = A.track_corridor()
        assert not rb["next_valid"] and np.isnan(rb["next_cost"])
        out, _, _, _ = _tick(A, 0, PC.S, track_corridor=True, corridor_margin=0.03, current_model=1003)
        assert nat.plan_out_to_dict(out)["sel_owned"] == 1 and not A.track_corridor()["valid"]
        assert A.track_corridor()["next_valid"]


def test_read_back_after_a_horizon_change(nat, monkeypatch):
    """track_corridor() takes no horizon: its arrays have the last track tick's, whatever came before.
    H = 40 then H = 12 then H = 40 (the shorter one is where a caller's own, stale H would have the
    library write past the arrays); a tick of another horizon is not offered the path, and its rows
    are the next tick's path again; async ticks count."""
    from llampc.mpc import ModelBank, constraints
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    tr = PC.track()
    with ModelBank(PC.bank(), W=W, device=0) as A:
        A.set_track(tr)
        prev = None
        for t, shape in enumerate(((3, 40), PC.S, PC.S, (3, 40))):
            C, H = shape
            if t == 2:                                      # the same tick enqueued
                x_prev, u_prev, x_t, uprev, U, xref = PC.tick_inputs(t, C, H)
                A.plan_async(x_prev, u_prev, x_t, U, xref, uprev, Ts=TS, K=K, track_corridor=True, corridor_margin=0.03)
                A.plan_wait()
            else:
                _tick(A, t, shape, track_corridor=True, corridor_margin=0.03)
            rb = A.track_corridor()
            assert rb["path"].shape == rb["next_path"].shape == (2, H + 1)
            assert rb["hp"].shape == (H, 6) and rb["theta"].shape == (H,)
            same_h = prev is not None and prev["hp"].shape[0] == H
            assert rb["valid"] == same_h and rb["next_valid"]
            if same_h:
                assert rb["path"].tobytes() == prev["next_path"].tobytes()
                assert np.max(np.abs(rb["hp"] - constraints.track_corridor(tr, rb["path"], 0.03))) <= HP_ATOL
            else:
                assert rb["hp"].tobytes() == constraints.disabled(H).tobytes() and np.isnan(rb["path"]).all()
            assert np.isfinite(rb["next_path"]).all()
            prev = rb


# ----------------------------------------------------------------- 4. async
def test_async_equals_blocking(nat, monkeypatch):
    """llampc_plan_track_async + llampc_plan_wait: the record and the read-back bitwise the blocking
    call's, on the same two ticks."""
    from llampc.mpc import ModelBank
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    C, H = PC.S
    row = PC.CHAIN[(PC.S, "ETHZ")]
    with ModelBank(PC.bank(), W=W, device=0) as A, ModelBank(PC.bank(), W=W, device=0) as B:
        A.set_track(PC.track())
        B.set_track(PC.track())
        for t in range(2):
            x_prev, u_prev, x_t, uprev, U, xref = PC.tick_inputs(t, C, H)
            kw = dict(Ts=TS, K=K, do_lookback=t >= 1, current_model=0, track_corridor=True, corridor_weight=row["weight"],
                      corridor_margin=row["margins"][t])
            oa, _, _, _ = A.plan_raw(x_prev, u_prev, x_t, U, xref, uprev, **kw)
            n0 = B.launches
            B.plan_async(x_prev, u_prev, x_t, U, xref, uprev, **kw)
            with pytest.raises(nat.NativeError) as ei:       # one outstanding tick per bank
                B.plan_async(x_prev, u_prev, x_t, U, xref, uprev, **kw)
            assert ei.value.code == nat.E_STATE
            ob = B.plan_wait()
            assert B.launches == n0 + 1
            same_record(nat, oa, ob, f"async tick {t}")
            ra, rb = A.track_corridor(), B.track_corridor()
            for k in ra:
                assert np.asarray(ra[k]).tobytes() == np.asarray(rb[k]).tobytes(), (t, k)
            assert ra["valid"] == (t == 1) and ra["next_valid"]


# ----------------------------------------------------------------- 5. refusals
def test_refusals_enqueue_nothing(nat, monkeypatch):
    """Each error code of the C entries with the launch counter unchanged."""
    from llampc.mpc import ModelBank
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    C, H = PC.S
    lib, ct = nat.load(), nat.C
    tr = PC.track()
    x_prev, u_prev, x_t, uprev, U, xref = PC.tick_inputs(1, C, H)
    out = nat.PlanOut()

    def pin_of(b, integrator="rk4", do_lookahead=True, raceline_start=None):
        return b._plan_in(x_prev, u_prev, x_t, U, xref, uprev, TS, K, integrator, True, do_lookahead, 0, nat.NAN_FIRST, None,
                          raceline_start=raceline_start)

    def track_tick(b, pin, w=1e4, m=0.03):
        return lib.llampc_plan_track(b.handle, ct.byref(pin), float(w), float(m), ct.byref(out), None, None, None)

    with ModelBank(PC.bank(), W=W, device=0) as b:
        n0 = b.launches
        pin, keep = pin_of(b)
        assert track_tick(b, pin) == nat.E_STATE and "no track set" in lib.llampc_last_error().decode()
        buf = np.empty((2, H + 1))
        v = ct.c_int32()
        c = ct.c_double()
        assert lib.llampc_bank_track_corridor(b.handle, nat.dptr(buf), nat.dptr(np.empty((H, 6))), nat.dptr(np.empty(H)),
                                              ct.byref(v), nat.dptr(buf.copy()), ct.byref(v), ct.byref(c)) == nat.E_STATE
        b.set_track(tr)
        for kw, word in ((dict(do_lookahead=False), "do_lookahead"), (dict(integrator="rk6"), "RK6"),
                         (dict(integrator="euler_nlp"), "NLP-Euler"), (dict(raceline_start=(0.0, 1.0, 1.0)), "RACELINE")):
            p2, keep2 = pin_of(b, **kw)
            assert track_tick(b, p2) == nat.E_ARG, kw
            assert word in lib.llampc_last_error().decode(), (kw, lib.llampc_last_error().decode())
        for w in (-1.0, float("nan"), float("inf")):
            assert track_tick(b, pin, w=w) == nat.E_ARG
        for m in (float("nan"), float("inf"), float(tr.track_width) / 2, 1.0):
            assert track_tick(b, pin, m=m) == nat.E_ARG
        assert lib.llampc_plan_track_async(b.handle, ct.byref(pin), -1.0, 0.03) == nat.E_ARG
        # llampc_bank_set_path: a non-finite entry, H outside [1, LLAMPC_HMAX]
        P = np.ascontiguousarray(xref).copy()
        assert lib.llampc_bank_set_path(b.handle, nat.dptr(P), 0) == nat.E_ARG
        assert lib.llampc_bank_set_path(b.handle, nat.dptr(np.zeros((2, nat.HMAX + 2))), nat.HMAX + 1) == nat.E_ARG
        P[1, 3] = np.nan
        assert lib.llampc_bank_set_path(b.handle, nat.dptr(P), H) == nat.E_ARG
        # llampc_bank_set_track: llampc_nlp_set_track's refusals
        centre = np.ascontiguousarray(tr.center_line, dtype=np.float64)
        theta = np.ascontiguousarray(tr.theta_track, dtype=np.float64)
        n = centre.shape[1]
        assert lib.llampc_bank_set_track(b.handle, centre.ctypes.data, theta.ctypes.data, 1, tr.track_length, 0.37) == nat.E_ARG
        assert lib.llampc_bank_set_track(b.handle, centre.ctypes.data, theta.ctypes.data, n, theta[-1], 0.37) == nat.E_ARG
        assert lib.llampc_bank_set_track(b.handle, centre.ctypes.data, theta.ctypes.data, n, tr.track_length, 0.0) == nat.E_ARG
        assert b.launches == n0
        # an async tick outstanding
        assert lib.llampc_plan_async(b.handle, ct.byref(pin)) == 0
        n1 = b.launches
        assert track_tick(b, pin) == nat.E_STATE and "async" in lib.llampc_last_error().decode()
        assert lib.llampc_plan_track_async(b.handle, ct.byref(pin), 1e4, 0.03) == nat.E_STATE
        assert b.launches == n1 == n0 + 1
        b.plan_wait()
        # and the bank still ticks
        assert track_tick(b, pin) == 0 and b.launches == n1 + 1
        # the Python layer raises before the library is touched
        with pytest.raises(ValueError):
            b.plan_raw(x_prev, u_prev, x_t, U, xref, uprev, track_corridor=True, corridor_margin=1.0)
        assert b.launches == n1 + 1

"""The plan tick's entries against each other: every route to a tick's record gives the same bytes.

One small shape — n = 70 (two waves, not a multiple of 64), W = 2, K = 2, (C, H) = (2, 3), RK4, the given
xref, the four-point track — and four closed-loop ticks (plan_track_cases.tick_inputs): tick 0 without a
look-back (the ticket completion), tick 1 with a window that is not full, ticks 2 and 3 polled on a full
window.  Three kinds of tick: the plain tick, the corridor tick on a fixed finite corridor, the track tick.

Every route runs in a fresh child process (this file as a script) on banks of its own; the children run side
by side and their results are shared by the tests below:
  plan      llampc_plan / llampc_plan_corridor / llampc_plan_track, the record alone (host completion)
  async     llampc_plan_async / llampc_plan_track_async + llampc_plan_wait
  device    llampc_plan_device on device inputs, the record and the err / wmean / cost arrays read back
  sync      the blocking and the async entries under LLAMPC_SYNC_COMPLETION=1 (the copy path)
  noinline  the blocking entries under LLAMPC_NO_INLINE=1 (the inputs staged, not kernel arguments)
  outputs   the blocking entries with err_out / wmean_out / cost_out
  refused   `outputs` with refused calls between ticks 1 and 2 — a plan tick with K = 0 on every kind's
            bank, a track tick with a negative weight on the track tick's: the twin of `outputs`
Records are compared bitwise; so are the arrays wherever two routes return them, and, for the track tick,
llampc_bank_track_corridor's read-back after every tick (after a corridor tick it is LLAMPC_E_STATE on
every route: the bank's last launch was no track tick)."""
import ctypes as ct
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import plan_track_cases as PC

pytestmark = pytest.mark.gpu

N, W, K, SHAPE, TICKS, TS = 70, 2, 2, (2, 3), 4, PC.TS
WEIGHT, MARGIN = 1e4, 0.2
KINDS = ("plain", "corridor", "track")
ROUTES = {"plan": {}, "async": {}, "device": {}, "sync": {"LLAMPC_SYNC_COMPLETION": "1"},
          "noinline": {"LLAMPC_NO_INLINE": "1"}, "outputs": {}, "refused": {}}
KNOBS = ("LLAMPC_SYNC_COMPLETION", "LLAMPC_NO_INLINE", "LLAMPC_NO_POLL", "LLAMPC_LPM")


def fixed_corridor():
    """hp [H, 6], finite: along the heading a of tick 0's state p_0, a.p <= a.p_0 + 0.02 (two centimetres of
    progress: a step of the recorded car is longer) and -a.p <= -a.p_0 + 1 (never reached)."""
    x0 = PC.tick_inputs(0, *SHAPE)[2]
    a = np.array([np.cos(x0[2]), np.sin(x0[2])])
    s0 = float(a @ x0[:2])
    return np.tile(np.array([a[0], a[1], s0 + 0.02, -a[0], -a[1], 1.0 - s0]), (SHAPE[1], 1))


def bank_params():
    from llampc.mpc import generate_bank
    return generate_bank(N, seed=70)


# --------------------------------------------------------------------------- the child
def run_kind(nat, kind, route):
    """One kind of tick through one route on a bank of its own: per tick dict(rec, err, wm, cost, rb)."""
    from llampc.mpc import ModelBank
    lib = nat.load()
    C, H = SHAPE
    hp = fixed_corridor()
    want_out = route in ("outputs", "refused")
    ticks = []
    with ModelBank(bank_params(), W=W, device=0) as b:
        if kind == "track":
            b.set_track(PC.track("square"))
        extra = {"corridor": dict(corridor=hp, corridor_weight=WEIGHT),
                 "track": dict(track_corridor=True, corridor_weight=WEIGHT, corridor_margin=MARGIN)}.get(kind, {})
        if route == "device":
            import torch
            dev = torch.device("cuda", 0)
            d_out = torch.zeros(ct.sizeof(nat.PlanOut), dtype=torch.uint8, device=dev)
            d_err, d_wm, d_cost = (torch.full((m,), float("nan"), dtype=torch.float64, device=dev) for m in (N, N, N * C))
            torch.cuda.synchronize()
        for t in range(TICKS):
            x_prev, u_prev, x_t, uprev, U, xref = PC.tick_inputs(t, C, H)
            kw = dict(Ts=TS, K=K, do_lookback=t >= 1, current_model=0)
            n0 = b.launches
            if route == "refused" and t == 2:
                out = nat.PlanOut()
                pin, keep = b._plan_in(x_prev, u_prev, x_t, U, xref, uprev, TS, 0, "rk4", True, True, 0, nat.NAN_FIRST, None)
                nul = (None, None, None)
                rc = {"plain": lambda: lib.llampc_plan(b.handle, ct.byref(pin), ct.byref(out), *nul),
                      "corridor": lambda: lib.llampc_plan_corridor(b.handle, ct.byref(pin), nat.dptr(hp), WEIGHT, ct.byref(out), *nul),
                      "track": lambda: lib.llampc_plan_track(b.handle, ct.byref(pin), WEIGHT, MARGIN, ct.byref(out), *nul)}[kind]()
                assert rc == nat.E_ARG and lib.llampc_last_error().decode() == "K=0 outside [1, 32]", (rc, lib.llampc_last_error())
                if kind == "track":
                    pin.K = K
                    assert lib.llampc_plan_track(b.handle, ct.byref(pin), -1.0, MARGIN, ct.byref(out), *nul) == nat.E_ARG
                    assert lib.llampc_last_error().decode() == "track tick: weight must be finite and >= 0"
                    assert lib.llampc_plan_track_async(b.handle, ct.byref(pin), -1.0, MARGIN) == nat.E_ARG
                assert b.launches == n0, "a refused call enqueues nothing"
            err = wm = cost = None
            if route == "device":
                pack = np.concatenate([x_prev, u_prev, x_t, uprev, xref.ravel(), U.ravel()])
                d_in = torch.from_numpy(pack).to(dev)
                pin, keep = b._plan_in(x_prev, u_prev, x_t, U, xref, uprev, TS, K, "rk4", t >= 1, True, 0, nat.NAN_FIRST, None)
                p0 = d_in.data_ptr()
                pin.x_prev, pin.u_prev, pin.x_now, pin.uprev = p0, p0 + 8 * 6, p0 + 8 * 8, p0 + 8 * 14
                pin.xref, pin.U = p0 + 8 * 16, p0 + 8 * (16 + 2 * (H + 1))
                nat.check(lib.llampc_plan_device(b.handle, ct.byref(pin), d_out.data_ptr(), d_err.data_ptr(), d_wm.data_ptr(),
                                                 d_cost.data_ptr(), None))
                torch.cuda.synchronize()
                rec = d_out.cpu().numpy().tobytes()
                err, wm, cost = d_err.cpu().numpy(), d_wm.cpu().numpy(), d_cost.cpu().numpy().reshape(N, C)
            elif route.endswith("async"):
                b.plan_async(x_prev, u_prev, x_t, U, xref, uprev, **kw, **{k: v for k, v in extra.items() if k != "corridor"})
                rec = bytes(b.plan_wait())
            else:
                o, err, wm, cost = b.plan_raw(x_prev, u_prev, x_t, U, xref, uprev, return_errors=want_out,
                                              return_window_mean=want_out, return_costs=want_out, **kw, **extra)
                rec = bytes(o)
            assert b.launches == n0 + 1, "one launch per tick"
            rb = None
            if kind == "track":
                rb = b.track_corridor()
            elif kind == "corridor":            # no track tick: the read-back is refused
                z = np.zeros(6 * nat.HMAX + 8)
                v, c = ct.c_int32(), ct.c_double()
                rb = lib.llampc_bank_track_corridor(b.handle, nat.dptr(z), nat.dptr(z.copy()), nat.dptr(z.copy()), ct.byref(v),
                                                    nat.dptr(z.copy()), ct.byref(v), ct.byref(c))
            ticks.append(dict(rec=rec, err=err if t >= 1 else None, wm=wm if t >= W else None, cost=cost, rb=rb))
    return ticks


def child(route):
    from llampc import _native as nat
    out = {}
    for kind in KINDS:
        if route == "device" and kind != "plain":
            continue                            # llampc_plan_device is the plain tick's
        if route == "async" and kind == "corridor":
            continue                            # the corridor tick has no async entry
        out[kind] = run_kind(nat, kind, route)
        if route == "sync" and kind != "corridor":
            out[kind + "_async"] = run_kind(nat, kind, "sync_async")
    return out


if __name__ == "__main__":
    with open(sys.argv[2], "wb") as f:
        pickle.dump(child(sys.argv[1]), f)
    sys.exit(0)


# --------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """{route: {kind: ticks}}: one child per route, all started at once."""
    d = tmp_path_factory.mktemp("entries")
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    procs = {r: subprocess.Popen([sys.executable, os.path.abspath(__file__), r, str(d / f"{r}.pkl")], env=dict(base, **env))
             for r, env in ROUTES.items()}
    res = {}
    try:
        for r, p in procs.items():
            assert p.wait(timeout=120) == 0, f"route {r}: the child exited with {p.returncode}"
            with open(d / f"{r}.pkl", "rb") as f:
                res[r] = pickle.load(f)
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
                p.wait()
    return res


def plan_out(rec):
    from llampc import _native as nat
    return nat.plan_out_to_dict(nat.PlanOut.from_buffer_copy(rec))


def same_records(a, b, what):
    assert len(a) == len(b) == TICKS
    for t, (x, y) in enumerate(zip(a, b)):
        if x["rec"] != y["rec"]:
            da, db = plan_out(x["rec"]), plan_out(y["rec"])
            diff = {k: (da[k], db[k]) for k in da if not np.array_equal(np.asarray(da[k]), np.asarray(db[k]), equal_nan=True)}
            raise AssertionError(f"{what}, tick {t}: records differ: {diff}")


def same_arrays(a, b, what):
    n = 0
    for t, (x, y) in enumerate(zip(a, b)):
        for k in ("err", "wm", "cost"):
            assert (x[k] is None) == (y[k] is None), (what, t, k)
            if x[k] is not None:
                assert x[k].tobytes() == y[k].tobytes(), f"{what}, tick {t}: {k} differs in {np.count_nonzero(x[k] != y[k])} entries"
                n += 1
    return n


def same_read_back(a, b, what):
    for t, (x, y) in enumerate(zip(a, b)):
        if isinstance(x["rb"], dict):
            assert set(x["rb"]) == set(y["rb"])
            for k in x["rb"]:
                assert np.asarray(x["rb"][k]).tobytes() == np.asarray(y["rb"][k]).tobytes(), (what, t, k)
        else:
            assert x["rb"] == y["rb"], (what, t)


def test_the_ticks_are_the_ones_meant(routes):
    """The reference route's own records: no status, the window's progress, the selection inside the bank;
    the corridor changes costs (it is not a no-op), the track tick is offered its path from tick 1 on."""
    from llampc import _native as nat
    ref = routes["plan"]
    for kind in KINDS:
        outs = [plan_out(t["rec"]) for t in ref[kind]]
        assert [o["status"] for o in outs] == [0] * TICKS, kind
        assert [(o["window_count"], o["window_full"]) for o in outs] == [(0, 0), (1, 0), (2, 1), (2, 1)], kind
        assert all(o["sel_owned"] == 1 and 0 <= o["sel_cand"] < SHAPE[0] and np.isfinite(o["sel_cost"]) for o in outs), kind
    plain, cor = routes["outputs"]["plain"], routes["outputs"]["corridor"]
    assert any((c["cost"] > p["cost"]).any() for p, c in zip(plain, cor)), "the fixed corridor penalises nothing"
    assert [int(t["rb"]["valid"]) for t in ref["track"]] == [0, 1, 1, 1]
    assert all(t["rb"]["next_valid"] for t in ref["track"])
    assert [t["rb"] for t in ref["corridor"]] == [nat.E_STATE] * TICKS


@pytest.mark.parametrize("route,kind", [
    ("async", "plain"), ("device", "plain"), ("sync", "plain"), ("sync", "plain_async"), ("noinline", "plain"),
    ("outputs", "plain"), ("sync", "corridor"), ("noinline", "corridor"), ("outputs", "corridor"),
    ("async", "track"), ("sync", "track"), ("sync", "track_async"), ("noinline", "track"), ("outputs", "track")])
def test_route_equals_blocking(routes, route, kind):
    """The route's four records bitwise those of the blocking host-completion entry; the track tick's
    read-back after every tick too."""
    ref = routes["plan"][kind.replace("_async", "")]
    got = routes[route][kind]
    same_records(got, ref, f"{route} / {kind}")
    same_read_back(got, ref, f"{route} / {kind}")


def test_arrays_equal_across_routes(routes):
    """err (ticks with a look-back), wmean (a full window) and cost (every tick) of llampc_plan's copy path
    bitwise those llampc_plan_device leaves on the device."""
    assert same_arrays(routes["outputs"]["plain"], routes["device"]["plain"], "outputs / device") == 3 + 2 + 4


@pytest.mark.parametrize("kind", KINDS)
def test_refused_calls_leave_no_trace(routes, kind):
    """After a plan tick with K = 0 (and, on the track tick's bank, a track tick with a negative weight)
    between ticks 1 and 2, the records, the arrays and the read-back are those of the twin bank that never
    saw the refused calls."""
    got, twin = routes["refused"][kind], routes["outputs"][kind]
    same_records(got, twin, f"refused / {kind}")
    assert same_arrays(got, twin, f"refused / {kind}") == 3 + 2 + 4
    same_read_back(got, twin, f"refused / {kind}")

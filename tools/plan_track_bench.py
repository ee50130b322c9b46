"""What the track tick costs: plan() on ETHZ at N = 10^4, H = 20, W = 5, K = 20, for C = 1 and C = 64,
record-only (host completion), on the recorded states of dyn_slice.  Modes per C, passes alternating in
one process so that a clock drift shows in all of them:
  plan       (a) llampc_plan as it is
  corridor   (b) llampc_plan_corridor with hp already on the host (built once, outside the timed calls)
  track      (d) llampc_plan_track: the corridor built in the launch, chained on the device
and (c) constraints.track_corridor on the host, the builder a plan(corridor=hp) loop would call per tick.
Per mode: the call's p50 / p99 / min (host clock; for the track tick this is call-to-record: the record
precedes the winner's re-run), back to back and again with GAP_US of host spinning between the calls (a
back-to-back call queues behind the launch before it, whose end — the re-run — follows its record), and the
plan kernel's own mean duration (llampc_bank_timing events, a pass of their own; the kernel's end follows
the re-run).  A measurement, no threshold.
usage: python tools/plan_track_bench.py [calls per pass] [passes]"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "lla-mpc_amd")]
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
from llampc import _native as nat  # noqa: E402
from llampc.mpc import ModelBank, constraints, generate_bank  # noqa: E402
from llampc.tracks import ETHZ, dyn_slice  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N, H, W, K, Ts, warm = 10000, 20, 5, 20, 0.02, 30
MARGIN, WEIGHT = 0.03, 1e4
GAP_US = 150.0
UMIN, UMAX = np.array([-0.1, -0.35]), np.array([1.0, 0.35])
tr = ETHZ('optimal', True)
d = dyn_slice()
S, Uin = d["states"], d["inputs"]
T0, SPAN = 20, 100                       # the loop runs over the recorded ticks T0 .. T0 + SPAN - 1


def tick_inputs(i, C):
    """Tick i of the loop: the recorded transition, the recorded inputs from there for every candidate
    (noise on candidates 1..), the straight reference from x_t."""
    t = T0 + i % SPAN
    x_prev, u_prev, x_t = S[:, t - 1], Uin[:, t - 1], S[:, t]
    U = np.repeat(Uin[:, t:t + H].T[None], C, axis=0).copy()
    if C > 1:
        U[1:] = np.clip(U[1:] + np.random.RandomState(i).uniform(-0.03, 0.03, (C - 1, H, 2)), UMIN, UMAX)
    v, tt = np.hypot(x_t[3], x_t[4]), np.arange(H + 1) * Ts
    xref = np.vstack([x_t[0] + v * np.cos(x_t[2]) * tt, x_t[1] + v * np.sin(x_t[2]) * tt])
    return x_prev, u_prev, x_t, U, xref


def one_pass(bank, ins, mode, hp, timed, gap_us=0.0):
    kw = dict(Ts=Ts, K=K)
    if mode == "corridor":
        kw.update(corridor=hp, corridor_weight=WEIGHT)
    elif mode == "track":
        kw.update(track_corridor=True, corridor_weight=WEIGHT, corridor_margin=MARGIN)
    lib = nat.load()
    if timed:
        nat.check(lib.llampc_bank_timing(bank.handle, 1, calls + warm))
    lat = []
    for i in range(calls + warm):
        x_prev, u_prev, x_t, U, xref = ins[i % SPAN]
        if gap_us:
            until = time.perf_counter() + gap_us * 1e-6
            while time.perf_counter() < until:
                pass
        t0 = time.perf_counter()
        out, _, _, _ = bank.plan_raw(x_prev, u_prev, x_t, U, xref, u_prev, **kw)
        lat.append(time.perf_counter() - t0)
    if timed:
        avg, cnt = (nat.C.c_double * 3)(), (nat.C.c_int64 * 3)()
        nat.check(lib.llampc_bank_timing_read(bank.handle, avg, cnt))
        nat.check(lib.llampc_bank_timing(bank.handle, 0, 0))
        return {"kernel_us": avg[0] * 1e3}
    lat = np.array(lat[warm:]) * 1e6
    r = {"p50": float(np.median(lat)), "p99": float(np.percentile(lat, 99)), "min": float(lat.min()),
         "sel_cost": float(out.sel_cost)}
    if mode == "track":
        rb = bank.track_corridor()
        r.update(path_valid=bool(rb["valid"]), next_valid=bool(rb["next_valid"]))
    return r


def host_builder(path):
    lat = []
    for _ in range(60):
        t0 = time.perf_counter()
        constraints.track_corridor(tr, path, MARGIN)
        lat.append(time.perf_counter() - t0)
    lat = np.array(lat[10:]) * 1e6
    return {"p50": float(np.median(lat)), "min": float(lat.min())}


out = {"N": N, "H": H, "W": W, "K": K, "calls": calls, "track_n": int(tr.center_line.shape[1])}
with ModelBank(generate_bank(N, seed=0), W=W, device=0) as bank:
    bank.set_track(tr)
    for C in (1, 64):
        ins = [tick_inputs(i, C) for i in range(SPAN)]
        path = constraints.default_path(ins[0][2], H, Ts)
        hp = constraints.track_corridor(tr, path, MARGIN)
        modes = ("plan", "corridor", "track")
        res = {m: {"call_us": [], "call_us_gap": [], "kernel_us": []} for m in modes}
        res["host_track_corridor_us"] = []
        for _ in range(passes):
            for m in modes:
                res[m]["call_us"].append(one_pass(bank, ins, m, hp, False))
            for m in modes:
                res[m]["call_us_gap"].append(one_pass(bank, ins, m, hp, False, GAP_US))
            for m in modes:
                res[m]["kernel_us"].append(one_pass(bank, ins, m, hp, True)["kernel_us"])
            res["host_track_corridor_us"].append(host_builder(path))
        out[f"C{C}"] = {"variant": nat.plan_variant(N, C, H), "variant_corridor": nat.plan_variant_corridor(N, C, H),
                        "variant_track": nat.plan_variant_track(N, C, H, out["track_n"]), "modes": res}
print(json.dumps(out))

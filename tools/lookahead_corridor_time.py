"""What the corridor costs a look-ahead launch: ModelBank.lookahead with and without corridor=hp at
N = 10^4, H = 20, for C = 1 (4 lanes per rollout: the plain launch splits the position over the quad,
the corridor launch cannot) and C = 64 (1 lane per rollout: the plain launch takes the work-queue
layout, the corridor launch the block-per-models one).  Modes per C, passes alternating in one
process so that a clock drift shows in all of them:
  plain          llampc_lookahead as it is
  plain_unsplit  (C = 1) Q[0][1] = 1e-300: the plain launch on the unsplit LPM-4 rollout
  plain_no_wq    (C = 64) LLAMPC_NO_WQ=1: the plain launch on the block-per-models layout
  corridor       llampc_lookahead_corridor, a strip of half width 0.05 m around xref, weight 1e4
Per mode: the call's p50 / p99 (host clock, record-only completion) and the plan kernel's own mean
duration (llampc_bank_timing events, a pass of their own).  A measurement, no threshold.
usage: python tools/lookahead_corridor_time.py [calls per pass] [passes]"""
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

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 3
N, H, Ts, warm = 10000, 20, 0.02, 30
x0 = np.array([0.5, -1.0, -0.6, 1.8, 0.05, 0.4])
uprev = np.array([0.5, 0.05])
xref = np.vstack([x0[0] + 0.03 * np.arange(H + 1), x0[1] + 0.01 * np.arange(H + 1)])
hp = constraints.strip(xref.T, 0.05)


def candidates(C):
    U = np.repeat(np.tile(uprev, (H, 1))[None], C, axis=0)
    if C > 1:
        U[1:, :, 1] += np.linspace(-0.05, 0.05, C - 1)[:, None]
    return U


def one_pass(bank, U, mode, timed):
    kw = {}
    if mode == "corridor":
        kw = dict(corridor=hp, corridor_weight=1e4)
    elif mode == "plain_unsplit":
        kw = dict(cost=nat.cost_struct(Q=np.array([[1.0, 1e-300], [0.0, 1.0]])))
    if mode == "plain_no_wq":
        os.environ["LLAMPC_NO_WQ"] = "1"
    lib = nat.load()
    try:
        if timed:
            nat.check(lib.llampc_bank_timing(bank.handle, 1, calls + warm))
        lat = []
        for _ in range(calls + warm):
            t0 = time.perf_counter()
            r = bank.lookahead(x0, U, xref, uprev, Ts=Ts, **kw)
            lat.append(time.perf_counter() - t0)
        if timed:
            avg, cnt = (nat.C.c_double * 3)(), (nat.C.c_int64 * 3)()
            nat.check(lib.llampc_bank_timing_read(bank.handle, avg, cnt))
            nat.check(lib.llampc_bank_timing(bank.handle, 0, 0))
            return {"kernel_us": avg[0] * 1e3, "launches": int(cnt[0])}
    finally:
        os.environ.pop("LLAMPC_NO_WQ", None)
    lat = np.array(lat[warm:]) * 1e6
    return {"p50": float(np.median(lat)), "p99": float(np.percentile(lat, 99)), "min": float(lat.min()),
            "best_cost": r["best_cost"]}


out = {"N": N, "H": H, "calls": calls}
with ModelBank(generate_bank(N, seed=0), device=0) as bank:
    for C, modes in ((1, ("plain", "plain_unsplit", "corridor")), (64, ("plain", "plain_no_wq", "corridor"))):
        U = candidates(C)
        v, vc = nat.plan_variant(N, C, H), nat.plan_variant_corridor(N, C, H)
        res = {m: {"call_us": [], "kernel_us": []} for m in modes}
        for _ in range(passes):
            for m in modes:
                res[m]["call_us"].append(one_pass(bank, U, m, False))
            for m in modes:
                res[m]["kernel_us"].append(one_pass(bank, U, m, True)["kernel_us"])
        out[f"C{C}"] = {"variant": v, "variant_corridor": vc, "modes": res}
print(json.dumps(out))

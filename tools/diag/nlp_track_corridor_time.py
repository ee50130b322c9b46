"""Diagnostic: what the device-built track corridor costs and what it removes (DESIGN §3 "The
corridor").  Default shape, the DYN-slice states of bench.py's solve_latency, 50 warm-up and
`solves` timed calls per pass, the passes alternating twice in one process:
  (a) plain      setupNLP.solve() unconstrained
  (b) given      solve(corridor=hp), hp = constraints.track_corridor(track, xref) built beforehand
  (c) device     setupNLP(device_corridor=True).solve(corridor_path=xref): the same corridor (to
                 1e-12) built by track_corridor_kernel ahead of the search, so (c) - (b) is that launch
  (d) host       constraints.track_corridor(track, xref) alone, on the CPU
then the corridor kernel's own time and the search's from llampc_bank_timing (HIP events around
each launch: kernel 1 and kernel 0) over 200 more device-corridor solves.
usage: python tools/diag/nlp_track_corridor_time.py [solves] [margin] [out.json]"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "lla-mpc_amd")]
from llampc import _native as nat  # noqa: E402
from llampc.models import Dynamic  # noqa: E402
from llampc.mpc import constraints  # noqa: E402
from llampc.mpc.nmpc import setupNLP  # noqa: E402
from llampc.mpc.planner import ConstantSpeed  # noqa: E402
from llampc.params import ORCA  # noqa: E402
from llampc.tracks import ETHZ  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
margin = float(sys.argv[2]) if len(sys.argv) > 2 else 0.0
out_path = sys.argv[3] if len(sys.argv) > 3 else None
H, warm = 20, 50
d = np.load(os.path.join(REPO, "tests", "golden", "dyn_slice.npz"))
s, u = d["states"], d["inputs"]
tr = ETHZ('optimal', True)
p = ORCA(control="pwm")
cases, projidx = [], 0
for t in range(10, 50):
    xref, projidx, _ = ConstantSpeed(s[:2, t], s[3, t], tr, H, 0.02, projidx)
    xref = np.ascontiguousarray(xref[:2], dtype=np.float64)
    cases.append((s[:, t].copy(), xref, u[:, t - 1].copy(), constraints.track_corridor(tr, xref, margin)))


def stats(lat):
    lat = np.array(lat[warm:]) * 1e6
    return {"p50": float(np.median(lat)), "p99": float(np.percentile(lat, 99)), "min": float(lat.min()),
            "calls": int(lat.size)}


def solver(device_corridor):
    return setupNLP(H, 0.02, np.eye(2), np.zeros((2, 2)), np.diag([5e-3, 1]), p, Dynamic(**p, device=0), tr, device=0,
                    device_corridor=device_corridor, corridor_margin=margin)


def run(mode):
    if mode == "host":
        lat = []
        for i in range(n + warm):
            xref = cases[i % len(cases)][1]
            t0 = time.perf_counter()
            constraints.track_corridor(tr, xref, margin)
            lat.append(time.perf_counter() - t0)
        return stats(lat)
    nlp = solver(mode == "device")
    lat, diff = [], 0.0
    try:
        for i in range(n + warm):
            x0, xref, up, hp = cases[i % len(cases)]
            kw = {"given": {"corridor": hp}, "device": {"corridor_path": xref}}.get(mode, {})
            t0 = time.perf_counter()
            nlp.solve(x0, xref, up, **kw)
            lat.append(time.perf_counter() - t0)
            if mode == "device":
                diff = max(diff, float(np.max(np.abs(nlp.last_corridor - hp))))
    finally:
        nlp.close()
    r = stats(lat)
    if mode == "device":
        r["max_abs_diff_to_host_corridor"] = diff
    return r


def kernel_times(count=200):
    """llampc_bank_timing on a device-corridor solver: the mean of HIP-event pairs around every
    launch of the search (kernel 0) and of the corridor kernel (kernel 1)."""
    nlp = solver(True)
    try:
        for i in range(warm):
            x0, xref, up, _ = cases[i % len(cases)]
            nlp.solve(x0, xref, up, corridor_path=xref)
        lib = nat.load()
        nat.check(lib.llampc_bank_timing(nlp._bank.handle, 1, count))
        for i in range(count):
            x0, xref, up, _ = cases[i % len(cases)]
            nlp.solve(x0, xref, up, corridor_path=xref)
        avg, cnt = (nat.C.c_double * 3)(), (nat.C.c_int64 * 3)()
        nat.check(lib.llampc_bank_timing_read(nlp._bank.handle, avg, cnt))
        nat.check(lib.llampc_bank_timing(nlp._bank.handle, 0, 0))
        return {"search_us": avg[0] * 1e3, "search_launches": cnt[0], "corridor_kernel_us": avg[1] * 1e3,
                "corridor_launches": cnt[1]}
    finally:
        nlp.close()


# alternating passes, so that a clock drift over the run shows in all of them
res = {"plain": [], "given": [], "device": [], "host": []}
for _ in range(2):
    for mode in res:
        res[mode].append(run(mode))
line = json.dumps({"H": H, "margin": margin, "solve_us": res, "event_timing": kernel_times()})
print(line)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")

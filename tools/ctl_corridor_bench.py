#!/usr/bin/env python
"""The controller step of bench.py's controller_ticks (an ETHZ and an ETHZMobil controller ticked
together, N models each, H = 40, C = 64, paced at 1 kHz) with the tick's soft track corridor on or off,
armed or launched: one JSON line with the step's p50 / p99 and llampc_ctl_device_us's.  The library is
LLAMPC_HIP_LIB's (an A/B against another build), LLAMPC_CTL_NO_SPEC=1 gives the plain tick without
speculative blocks — the corridor tick's like-for-like.
  tools/ctl_corridor_bench.py [--corridor W] [--launched] [--n N] [--ticks T] [--label S]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "lla-mpc_amd")]

HALF = {"ETHZ": 0.10, "ETHZMobil": 0.15}     # the corridor's half widths (tests/ctl_corridor_cases.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corridor", type=float, default=0.0)
    ap.add_argument("--launched", action="store_true")
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--ticks", type=int, default=400)
    ap.add_argument("--warm", type=int, default=60)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    from llampc.models import Dynamic
    from llampc.mpc import LLAMPC, ModelBank, generate_bank
    from llampc.params import ORCA
    from llampc.tracks import ETHZ, ETHZMobil, dyn_slice
    p = ORCA()
    setups = []
    for seed, tr in ((0, ETHZ('optimal', True)), (1, ETHZMobil('optimal', True))):
        b = ModelBank(generate_bank(a.n, seed=seed), W=10, device=0)
        b.set_concurrency(2)
        kw = {}
        if a.corridor > 0:
            kw = dict(corridor_weight=a.corridor, corridor_margin=float(tr.track_width) / 2 - HALF[tr.name])
        ctl = LLAMPC(b, tr, H=40, C=64, K=10, mode="device", prelaunch=not a.launched, **kw)
        x = dyn_slice()["states"][:, 0].copy() if tr.name == "ETHZ" else np.array([tr.x_init, tr.y_init, tr.psi_init, 1.0, 0.0, 0.0])
        setups.append([b, ctl, Dynamic(**p, device=0), x])
    lat, devt, valid = [], [], 0
    period = 1e-3
    try:
        nxt = time.perf_counter() + period
        for i in range(a.warm + a.ticks):
            while time.perf_counter() < nxt:
                pass
            nxt = max(nxt + period, time.perf_counter())
            t0 = time.perf_counter()
            for s in setups:
                s[1].tick_begin(s[3])
            res = [s[1].tick_end() for s in setups]
            lat.append(time.perf_counter() - t0)
            devt.append([s[1].device_us() for s in setups])
            for s, r in zip(setups, res):
                pl = s[2]
                pl.Df -= pl.Df / 2600.
                pl.Dr -= pl.Dr / 2600.
                xn, _ = pl.sim_continuous(s[3], r.u_seq[:, 0].reshape(2, 1), [0, 0.02])
                s[3] = xn[:, -1]
        if a.corridor > 0:
            valid = [bool(s[1].corridor()[3]) for s in setups]
        launches = [int(s[0].launches) for s in setups]
    finally:
        for s in setups:
            s[1].close()
            s[0].close()
    q = lambda v: {"p50": round(float(np.percentile(v, 50)), 2), "p99": round(float(np.percentile(v, 99)), 2)}
    print(json.dumps({"label": a.label, "lib": os.environ.get("LLAMPC_HIP_LIB", "tree"),
                      "no_spec": os.environ.get("LLAMPC_CTL_NO_SPEC", "0"), "corridor": a.corridor,
                      "armed": not a.launched, "n": a.n, "ticks": a.ticks,
                      "step_us": q(np.array(lat[a.warm:]) * 1e6), "device_us": q(np.array(devt[a.warm:]).ravel()),
                      "last_path_valid": valid, "launches": launches}))


if __name__ == "__main__":
    main()

"""Diagnostic: setupNLP.solve(..., corridor=track_corridor(track, xref)) back to back on DYN-slice
states (bench.py solve_latency's cases) at the default shape, beside the unconstrained solve on
the same states: the corridor's cost per solve (DESIGN §3 "setupNLP").  The corridor is built
outside the timed region (it is host work of the caller's, once per tick).
usage: python tools/diag/nlp_corridor_solve.py [solves] [margin]"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "lla-mpc_amd")]
from llampc.models import Dynamic  # noqa: E402
from llampc.mpc import constraints  # noqa: E402
from llampc.mpc.nmpc import setupNLP  # noqa: E402
from llampc.mpc.planner import ConstantSpeed  # noqa: E402
from llampc.params import ORCA  # noqa: E402
from llampc.tracks import ETHZ  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
margin = float(sys.argv[2]) if len(sys.argv) > 2 else 0.0
H, warm = 20, 50
d = np.load(os.path.join(REPO, "tests", "golden", "dyn_slice.npz"))
s, u = d["states"], d["inputs"]
tr = ETHZ('optimal', True)
p = ORCA(control="pwm")
cases, projidx = [], 0
for t in range(10, 50):
    xref, projidx, _ = ConstantSpeed(s[:2, t], s[3, t], tr, H, 0.02, projidx)
    cases.append((s[:, t].copy(), xref, u[:, t - 1].copy(), constraints.track_corridor(tr, xref, margin)))


def run(with_corridor):
    nlp = setupNLP(H, 0.02, np.eye(2), np.zeros((2, 2)), np.diag([5e-3, 1]), p, Dynamic(**p, device=0), tr, device=0)
    lat, viol, slack = [], 0, 0.0
    try:
        for i in range(n + warm):
            x0, xref, up, hp = cases[i % len(cases)]
            t0 = time.perf_counter()
            out = nlp.solve(x0, xref, up, corridor=hp if with_corridor else None)
            lat.append(time.perf_counter() - t0)
            viol += out[3] != 0.0
            slack = max(slack, nlp.max_slack)
    finally:
        nlp.close()
    lat = np.array(lat[warm:]) * 1e6
    return {"p50": float(np.median(lat)), "p99": float(np.percentile(lat, 99)), "min": float(lat.min()),
            "solves": int(lat.size), "violations": int(viol), "max_slack": slack}


# alternating passes, so that a clock drift over the run shows in both
res = {"plain": [], "corridor": []}
for _ in range(2):
    res["plain"].append(run(False))
    res["corridor"].append(run(True))
print(json.dumps({"H": H, "margin": margin, "solve_us": res}))

#!/usr/bin/env python
"""Wall time of setupNLPBatch.solve (B problems of a model bank in one launch) beside B sequential
setupNLP.solve calls (one solver per bank column), at the default shape (1,024 samples, 8 rounds,
32 elite) and H = 20: p50 / p99 over --reps timed calls after --warmup, per B, and the launches' own
duration from HIP events (kernel_us: one launch batched, the sum of the B launches sequential).

    python tools/nlp_batch_bench.py                      # B in 1 2 4 8 16, batched and sequential
    python tools/nlp_batch_bench.py --pairs 3 --B 8      # three alternating (batched, sequential) pairs

Every measurement is a step of its own: a fresh child process under its own time limit, one JSON
line each; the chain stops at the first step that fails or runs out of time (nothing more is
started on the device after that).  A batched step whose problems did not all report (B x 16 blocks
do not fit beside whatever else holds CUs) prints the count in "failed" and ends the chain too: lower
max_resident instead of retrying.  Both paths solve the same problems: bank column p, seed p, the
same state, reference and previous input, warm-started from call to call as a controller's ticks
are."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "lla-mpc_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, TS, N_BANK = 20, 0.02, 64


def problems(B):
    import numpy as np
    x0 = np.tile([0.5, -1.0, -0.6, 1.8, 0.05, 0.4], (B, 1)) + 0.01 * np.arange(B)[:, None]
    k = np.arange(H + 1)
    c, s = np.cos(x0[:, 2]), np.sin(x0[:, 2])
    xref = np.stack([x0[:, :1] + 1.8 * TS * k * c[:, None], x0[:, 1:2] + 1.8 * TS * k * s[:, None]], axis=1)
    up = np.tile([0.5, 0.05], (B, 1))
    return x0, xref, up


def step(mode, B, reps, warmup):
    import numpy as np
    from llampc.mpc import ModelBank, generate_bank, setupNLP, setupNLPBatch
    from llampc.params import ORCA
    from llampc.mpc.bank import BANK_ORDER
    params = ORCA(control="pwm")
    Q, P, R = np.eye(2), np.zeros((2, 2)), np.diag([5e-3, 1.0])
    bank6 = generate_bank(N_BANK, seed=0)
    x0, xref, up = problems(B)
    failed = 0
    if mode == "batched":
        bank = ModelBank(bank6, W=1, device=0)
        nb = setupNLPBatch(H, TS, Q, P, R, params, bank, max_batch=B)
        models, seeds = list(range(B)), list(range(B))

        def call():
            return int((~nb.solve(models, x0, xref, up, seeds=seeds)[3]).sum())
        closers, banks = [nb, bank], lambda: [bank]
    else:
        solvers = []
        for p in range(B):
            m = dict(params)
            m.update(zip(BANK_ORDER, bank6[:, p]))
            solvers.append(setupNLP(H, TS, Q, P, R, params, m, None, seed=p))

        def call():
            for p, s in enumerate(solvers):
                s.solve(x0[p], xref[p], up[p])
            return 0
        closers, banks = solvers, lambda: [s._bank for s in solvers]    # created at the first solve
    for _ in range(warmup):
        failed += call()
    t = np.empty(reps)
    for i in range(reps):
        t0 = time.perf_counter()
        failed += call()
        t[i] = time.perf_counter() - t0
    # the launches' own duration (HIP events around each, llampc_bank_timing), over 100 more calls:
    # per launch, and summed over the B launches of a sequential call
    from llampc import _native as nat
    lib, banks = nat.load(), banks()
    for b in banks:
        nat.check(lib.llampc_bank_timing(b.handle, 1, 100))
    for _ in range(100):
        failed += call()
    kernel_us = 0.0
    for b in banks:
        avg, cnt = (nat.C.c_double * 3)(), (nat.C.c_int64 * 3)()
        nat.check(lib.llampc_bank_timing_read(b.handle, avg, cnt))
        nat.check(lib.llampc_bank_timing(b.handle, 0, 0))
        kernel_us += avg[0] * 1e3
    for c in closers:
        c.close()
    print(json.dumps(dict(mode=mode, B=B, H=H, samples=1024, reps=reps, p50_us=round(float(np.percentile(t, 50)) * 1e6, 2),
                          p99_us=round(float(np.percentile(t, 99)) * 1e6, 2), mean_us=round(float(t.mean()) * 1e6, 2),
                          kernel_us=round(kernel_us, 2), failed=failed)), flush=True)
    return 3 if failed else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--pairs", type=int, default=1, help="alternating (batched, sequential) pairs per B")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--step-timeout", type=float, default=90.0, help="seconds per step")
    ap.add_argument("--step", choices=["batched", "sequential"], help="run one step in this process (internal)")
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.B[0], a.reps, a.warmup)
    for B in a.B:
        for _ in range(a.pairs):
            for mode in ("batched", "sequential"):
                cmd = [sys.executable, os.path.abspath(__file__), "--step", mode, "--B", str(B), "--reps", str(a.reps),
                       "--warmup", str(a.warmup)]
                try:
                    rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
                except subprocess.TimeoutExpired:
                    print(json.dumps(dict(mode=mode, B=B, error=f"step exceeded {a.step_timeout} s")), flush=True)
                    return 124
                if rc:
                    print(json.dumps(dict(mode=mode, B=B, error=f"step ended with status {rc}")), flush=True)
                    return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""Wall time of the batched corridor solve (setupNLPBatch.solve(..., corridor=hp [B, H, 6],
corridor_weight=w [B]): B problems, each under its own soft corridor, in one launch) at the default
shape (1,024 samples, 8 rounds, 32 elite) and H = 20, beside what it is to be read against on the
same build, per B:

    batched_corridor      (a) the batched corridor solve
    batched_plain         (b) the batched plain solve (its code object is untouched by the corridor)
    sequential_corridor   (c) B sequential setupNLP.solve(..., corridor=hp[p]) calls, one solver per column
    sequential_plain          B sequential plain setupNLP.solve calls (the single solver's own
                              corridor - plain difference is (c) - this)
    batched_track             the device-built pair: the builder kernel (B x H blocks) and the search

p50 / p99 over --reps timed calls after --warmup, and the launches' own duration from HIP events
(llampc_bank_timing: kernel_us the search — one launch batched, the sum of the B launches
sequential — and builder_us the corridor kernel).

    python tools/nlp_batch_corridor_bench.py                    # B in 1 2 8, every mode
    python tools/nlp_batch_corridor_bench.py --B 8 --modes batched_corridor batched_plain

Every measurement is a step of its own: a fresh child process under its own time limit, one JSON
line each; the chain stops at the first step that fails or runs out of time (nothing more is
started on the device after that).  All modes solve the same problems (tools/nlp_batch_bench.py's):
bank column p, seed p, warm-started from call to call; the corridor is a strip of half-width 0.05 m
around each problem's reference, weight 1e3; the device-built one is the ETHZ track's along the
reference."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "lla-mpc_amd"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from nlp_batch_bench import H, N_BANK, TS, problems  # noqa: E402

MODES = ("batched_corridor", "batched_plain", "sequential_corridor", "sequential_plain", "batched_track")
HALF, WEIGHT = 0.05, 1e3


def step(mode, B, reps, warmup):
    import numpy as np
    from llampc.mpc import ModelBank, constraints, generate_bank, setupNLP, setupNLPBatch
    from llampc.params import ORCA
    from llampc.mpc.bank import BANK_ORDER
    params = ORCA(control="pwm")
    Q, P, R = np.eye(2), np.zeros((2, 2)), np.diag([5e-3, 1.0])
    bank6 = generate_bank(N_BANK, seed=0)
    x0, xref, up = problems(B)
    hp = np.array([constraints.strip(xref[p].T, HALF) for p in range(B)])
    w = np.full(B, WEIGHT)
    failed = 0
    if mode.startswith("batched"):
        bank = ModelBank(bank6, W=1, device=0)
        kw = {}
        if mode == "batched_track":
            from llampc.tracks import ETHZ
            kw = dict(track=ETHZ('optimal', True), device_corridor=True, corridor_weight=WEIGHT)
        nb = setupNLPBatch(H, TS, Q, P, R, params, bank, max_batch=B, **kw)
        models, seeds = list(range(B)), list(range(B))
        extra = {"batched_corridor": dict(corridor=hp, corridor_weight=w), "batched_plain": {},
                 "batched_track": dict(corridor_path=xref)}[mode]

        def call():
            return int((~nb.solve(models, x0, xref, up, seeds=seeds, **extra)[3]).sum())
        closers, banks = [nb, bank], lambda: [bank]
    else:
        solvers = []
        for p in range(B):
            m = dict(params)
            m.update(zip(BANK_ORDER, bank6[:, p]))
            solvers.append(setupNLP(H, TS, Q, P, R, params, m, None, seed=p, corridor_weight=WEIGHT))
        cor = mode == "sequential_corridor"

        def call():
            for p, s in enumerate(solvers):
                s.solve(x0[p], xref[p], up[p], corridor=hp[p] if cor else None)
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
    kernel_us = builder_us = 0.0
    for b in banks:
        avg, cnt = (nat.C.c_double * 3)(), (nat.C.c_int64 * 3)()
        nat.check(lib.llampc_bank_timing_read(b.handle, avg, cnt))
        nat.check(lib.llampc_bank_timing(b.handle, 0, 0))
        kernel_us += avg[0] * 1e3
        builder_us += avg[1] * 1e3 if cnt[1] else 0.0
    for c in closers:
        c.close()
    print(json.dumps(dict(mode=mode, B=B, H=H, samples=1024, reps=reps, p50_us=round(float(np.percentile(t, 50)) * 1e6, 2),
                          p99_us=round(float(np.percentile(t, 99)) * 1e6, 2), mean_us=round(float(t.mean()) * 1e6, 2),
                          kernel_us=round(kernel_us, 2), builder_us=round(builder_us, 2), failed=failed)), flush=True)
    return 3 if failed else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--B", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--modes", nargs="+", choices=MODES, default=list(MODES))
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--step-timeout", type=float, default=90.0, help="seconds per step")
    ap.add_argument("--step", choices=MODES, help="run one step in this process (internal)")
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.B[0], a.reps, a.warmup)
    for B in a.B:
        for mode in a.modes:
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

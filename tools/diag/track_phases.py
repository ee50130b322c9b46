"""Diagnostic (stamps build): where the track tick's time goes.  Runs llampc_plan_track record-only on
ETHZ (N models, H = 20, W = 5, K = 20, the loop of tools/plan_track_bench.py) for C = 1 and C = 64 and
prints, for the last ticks, the phase boundaries of the launch's blocks relative to its first block's
entry (µs, s_memrealtime at 100 MHz; min / median / max over the blocks of a role, the first 1024
blocks of the grid): corridor blocks — entry, row published; look-ahead blocks — entry, inputs staged,
half-planes polled, rolled out, published; the completing block — completion entered, record (and host
tag) stored, path written.
usage: python tools/diag/track_phases.py [N] [ticks printed]"""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("LLAMPC_HIP_LIB", os.path.join(REPO, "lla-mpc_amd/llampc/_lib/libllampc_hip_stamps.so"))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
sys.path[:0] = [REPO, os.path.join(REPO, "lla-mpc_amd")]
from llampc import _native as nat  # noqa: E402
from llampc.mpc import ModelBank, generate_bank  # noqa: E402
from llampc.tracks import ETHZ, dyn_slice  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 4
H, W, K, Ts = 20, 5, 20, 0.02
lib = nat.load()
lib.llampc_debug_track_ph.argtypes = [ctypes.c_void_p]
tr = ETHZ('optimal', True)
d = dyn_slice()
S, Uin = d["states"], d["inputs"]
buf = (ctypes.c_ulonglong * (1024 * 8))()


def q(v):
    return f"{v.min():.1f}/{np.median(v):.1f}/{v.max():.1f}"


with ModelBank(generate_bank(N, seed=0), W=W, device=0) as bank:
    bank.set_track(tr)
    for C in (1, 64):
        v = nat.plan_variant_track(N, C, H, tr.center_line.shape[1])
        print(f"C = {C}: {v}", flush=True)
        for i in range(40 + T):
            t = 20 + i
            U = np.repeat(Uin[:, t:t + H].T[None], C, axis=0).copy()
            if C > 1:
                U[1:] = np.clip(U[1:] + np.random.RandomState(i).uniform(-0.03, 0.03, (C - 1, H, 2)), [-0.1, -0.35], [1.0, 0.35])
            x_t = S[:, t]
            sp, tt = np.hypot(x_t[3], x_t[4]), np.arange(H + 1) * Ts
            xref = np.vstack([x_t[0] + sp * np.cos(x_t[2]) * tt, x_t[1] + sp * np.sin(x_t[2]) * tt])
            out, _, _, _ = bank.plan_raw(S[:, t - 1], Uin[:, t - 1], x_t, U, xref, Uin[:, t - 1], Ts=Ts, K=K,
                                         track_corridor=True, corridor_margin=0.03)
            if i < 40:
                continue
            rb = bank.track_corridor()                       # drains the stream: the launch has ended
            lib.llampc_debug_track_ph(buf)
            Z = np.frombuffer(buf, dtype=np.uint64).reshape(1024, 8).astype(np.int64)
            base = Z[Z[:, 0] > 0, 0].min()
            cur = Z[:, 0] >= base
            us = lambda a: (a - base) / 100.0  # noqa: E731
            done = np.where(Z[:, 7] >= base)[0]
            win = int(done[np.argmax(Z[done, 7])])
            cor = [k for k in range(1024) if cur[k] and Z[k, 1] >= base and Z[k, 3] < base]     # never rolled out
            la = [k for k in range(1024) if cur[k] and Z[k, 4] >= base]
            parts = [f"tick {i} valid {int(rb['valid'])}: corridor blocks {len(cor)} entry {q(us(Z[cor, 0]))} published {q(us(Z[cor, 1]))} |",
                     f"look-ahead blocks {len(la)} entry {q(us(Z[la, 0]))} staged {q(us(Z[la, 1]))} polled {q(us(Z[la, 2]))} "
                     f"rolled {q(us(Z[la, 3]))} published {q(us(Z[la, 4]))} |",
                     f"completing block {win}: entered {us(Z[win, 5]):.1f} record {us(Z[win, 6]):.1f} path {us(Z[win, 7]):.1f}"]
            print(" ".join(parts), flush=True)

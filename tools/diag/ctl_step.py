"""Measurement: the fused control step against the best unfused composition of the same build, in one
process.  ETHZ, N = 10^4 models, H = 20, C = 64, K = 10, NLP 1,024 samples x 8 rounds; each leg runs its
own closed loop (its own bank, controller and plant state) paced at 1 kHz.

  (a) fused     LLAMPC(solve=...).step(x_t): tick, build, solve and commit in one chain, one host wait
  (b) unfused   a launched tick(); llampc_ctl_reference with the record's mu_used / scale_used and the
                projection index the tick started from (the tick's own reference, once more);
                setupNLPBatch.solve([best_model]) — setupNLP on the nominal model while the tick is
                warm; set_applied(umpc[:, 0], umpc)

The legs alternate in blocks of BLOCK steps (other work shares the host), after WARM warm-up steps
each; the step time is the host clock from x_t known to the applied input known (every leg ends in a
wait on the device's tag).  A second pass, of its own, brackets each leg's launches with
llampc_bank_timing (device events cost host time, so no latency is taken there) and reports the device
time per step: (a) the chain as one group, (b) the tick's launch plus the solve's launch (the
reference kernel between them is not bracketed).  Writes one JSON document.

usage: python tools/diag/ctl_step.py [--steps 500] [--warm 50] [--n 10000] [--out profiles/ctl_step/ctl_step.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "lla-mpc_amd")]

BLOCK = 50
PERIOD = 1e-3
H, C, K, TS = 20, 64, 10, 0.02
SOLVE = dict(samples=1024, iters=8, elite=32, sigma=(0.3, 0.15), std_floor=1e-4, seed=0)


class Leg:
    """One leg's closed loop: bank, controller, plant state, and step(x) -> the applied input."""

    def __init__(self, name, n, fused):
        from llampc import _native as nat
        from llampc.mpc import LLAMPC, ModelBank, generate_bank, setupNLP, setupNLPBatch
        from llampc.models import Dynamic
        from llampc.params import ORCA
        from llampc.tracks import ETHZ
        self.name, self.fused, self.nat = name, fused, nat
        self.track = ETHZ('optimal', True)
        self.bank = ModelBank(generate_bank(n, seed=0), W=10, device=0)
        self.ctl = LLAMPC(self.bank, self.track, H=H, C=C, K=K, Ts=TS, prelaunch=False, solve=SOLVE if fused else None)
        self.x = np.load(os.path.join(REPO, "tests", "golden", "dyn_slice.npz"))["states"][:, 0].copy()
        self.lat, self.committed, self.projidx = [], 0, 0
        self.nom = self.batch = None
        if not fused:
            p = ORCA(control="pwm")
            Q, R, P = np.eye(2), np.diag([5e-3, 1.0]), np.zeros((2, 2))
            kw = {k: SOLVE[k] for k in ("samples", "iters", "elite", "sigma", "std_floor", "seed")}
            self.batch = setupNLPBatch(H, TS, Q, P, R, p, self.bank, max_batch=1, **kw)
            self.nom = setupNLP(H, TS, Q, P, R, p, Dynamic(**p, device=0), self.track, device=0, **kw)

    def step(self, x):
        if self.fused:
            r = self.ctl.step(x)
            self.committed += r.committed
            return r.u0
        res = self.ctl.tick(x)
        o = res.raw
        xref, _, _ = self.ctl._ctl.reference(x[:2], x[3], H, self.projidx, curr_mu=o.mu_used, scale=o.scale_used)
        self.projidx = o.projidx
        uprev = self.uprev
        if res.nominal:
            umpc, fval, _, _ = self.nom.solve(x, xref, uprev)
            ok = np.isfinite(fval)
        else:
            um, fv, _, okb = self.batch.solve([res.best_model], x[None], xref[None], uprev[None])
            umpc, ok = um[0], bool(okb[0])
        if not ok:
            return res.u0
        self.ctl.set_applied(umpc[:, 0], umpc)
        self.committed += 1
        return (umpc[0, 0], umpc[1, 0])

    def run(self, steps, plant, timed):
        """`steps` paced steps of this leg's loop; timed: their latencies are kept."""
        nxt = time.perf_counter()
        for _ in range(steps):
            nxt = max(nxt + PERIOD, time.perf_counter())
            while time.perf_counter() < nxt:
                pass
            self.uprev = np.zeros(2) if self.ctl.u_prev is None else np.asarray(self.ctl.u_prev, dtype=np.float64)
            t0 = time.perf_counter()
            u0 = self.step(self.x)
            dt = time.perf_counter() - t0
            if timed:
                self.lat.append(dt)
            xn, _ = plant.sim_continuous(self.x, np.array(u0, dtype=np.float64).reshape(2, 1), [0, TS])
            self.x = xn[:, -1]

    def device_ms(self, steps, plant):
        """The leg's launches bracketed by device events over `steps` more steps: the mean device time
        per step (ms) and the bracketed launches per step."""
        nat, lib = self.nat, self.nat.load()
        nat.check(lib.llampc_bank_timing(self.bank.handle, 1, 2 * steps + 8))
        self.run(steps, plant, timed=False)
        avg = (nat.C.c_double * 3)()
        cnt = (nat.C.c_int64 * 3)()
        nat.check(lib.llampc_bank_timing_read(self.bank.handle, avg, cnt))
        nat.check(lib.llampc_bank_timing(self.bank.handle, 0, 0))
        return avg[0] * cnt[0] / steps, cnt[0] / steps

    def close(self):
        for s in (self.nom, self.batch, self.ctl, self.bank):
            if s is not None:
                s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--device-steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ctl_step", "ctl_step.json"))
    a = ap.parse_args()
    from llampc import _native as nat
    from llampc.models import Dynamic
    from llampc.params import ORCA
    if nat.device_count() < 1:
        raise SystemExit("no HIP device: this is a measurement on the GPU")
    plant = Dynamic(**ORCA(), device=0)
    legs = [Leg("fused", a.n, True), Leg("unfused", a.n, False)]
    for leg in legs:
        leg.run(a.warm, plant, timed=False)
    done = 0
    while done < a.steps:
        nb = min(BLOCK, a.steps - done)
        for leg in legs:
            leg.run(nb, plant, timed=True)
        done += nb
    out = dict(shape=dict(track="ETHZ", N=a.n, H=H, C=C, K=K, Ts=TS, solve=dict(SOLVE, sigma=list(SOLVE["sigma"]))),
               warmup_steps=a.warm, steps=a.steps, period_us=PERIOD * 1e6, block=BLOCK, device_steps=a.device_steps, legs={})
    for leg in legs:
        lat = np.array(leg.lat) * 1e6
        committed = leg.committed            # of the warm-up and the timed steps
        dev_ms, per_step = leg.device_ms(a.device_steps, plant)
        out["legs"][leg.name] = dict(p50_us=float(np.percentile(lat, 50)), p99_us=float(np.percentile(lat, 99)),
                                     min_us=float(lat.min()), mean_us=float(lat.mean()), committed=int(committed),
                                     device_us_per_step=dev_ms * 1e3, bracketed_launches_per_step=per_step)
        print(f"{leg.name}: step us p50 {out['legs'][leg.name]['p50_us']:.1f} p99 {out['legs'][leg.name]['p99_us']:.1f} "
              f"min {lat.min():.1f} | device {dev_ms * 1e3:.1f} us per step ({per_step:.2f} bracketed launches)")
    for leg in legs:
        leg.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

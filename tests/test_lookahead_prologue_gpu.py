"""The look-ahead block's prologue (lookahead_dev.hpp, shared-xref path): every thread issues its
clamped, unconditional input loads (start state, previous input, its reference element, its staging
element's input pairs) in one batch, the per-model setup runs under their latency, and the plan
kernels touch their argument lines first.  The shapes are the smallest at which that can go wrong:

  * N = 1 and N = 65 at C = 1, H = 1: dead lanes and a partial last block, every surplus lane's
    loads clamped to the one element there is;
  * C = 8, H = 32: exactly one block (256) of staging elements;
  * C = 13, H = 21: 273 elements, a second, partial staging pass;
  * C = 64, H = 40: unstaged (the prologue without the staging batch),

each at 1, 2 and 4 lanes per rollout (LLAMPC_LPM, asserted through llampc_plan_variant).  The tick
runs over the three input routes through that code, each on a bank of its own (W = 1: the first
tick fills the window):

  * device pointers (llampc_plan_device), the pack [x_prev | u_prev | x_now | uprev | xref | U]
    placed as the LAST bytes of a device allocation of its own, so a load past an array's end
    leaves the allocation;
  * host pointers with the inputs as kernel arguments (llampc_plan, record only; the pack has
    352 doubles at most, so the larger shapes take the copy there too);
  * host pointers with the H2D copy (LLAMPC_NO_INLINE=1).

Asserted: the per-model costs of the device-pointer tick against oracle.plan_cpu with
conftest.assert_costs_close at the suite's 1e-6, and the three records equal field for field."""
import ctypes
import os

import numpy as np
import pytest

from conftest import assert_costs_close, core_error_bound, golden
from oracle import llampc_oracle as O

pytestmark = pytest.mark.gpu

RTOL_ROLL = 1e-6
TS = 0.02
Q, R, P = np.eye(2), np.diag([5e-3, 1.0]), np.zeros((2, 2))
UMIN, UMAX = np.array([-0.1, -0.35]), np.array([1.0, 0.35])
# the caching allocator hands sizes from 10 MiB on to the driver as they are (rounded to 2 MiB),
# one allocation each: the last byte of this tensor is the last byte of a device allocation
ALLOC_BYTES = 12 << 20

# name -> (N, C, H, staged)
SHAPES = {"n1": (1, 1, 1, True), "n65": (65, 1, 1, True), "one_block": (97, 8, 32, True),
          "second_pass": (97, 13, 21, True), "unstaged": (97, 64, 40, False)}


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


@pytest.fixture(scope="module")
def tail_buffer(nat):
    import torch
    return torch.empty(ALLOC_BYTES, dtype=torch.uint8, device=torch.device("cuda", 0))


def shared():
    p = O.orca_params()
    return {k: p[k] for k in ("lf", "lr", "mass", "Iz", "Cm1", "Cm2", "Cr0", "Cr2")}


_CASE = {}


def case(name):
    """Inputs from the recorded slice (the transition 39 -> 40, the inputs from step 40 with +-0.03
    noise on candidates 1.., a straight reference from x0) and the oracle's tick, once per shape."""
    if name not in _CASE:
        from llampc.mpc import generate_bank
        N, C, H, _ = SHAPES[name]
        d = golden("dyn_slice.npz")
        s, u = d["states"], d["inputs"]
        x_prev, u_prev, x0, uprev = s[:, 39].copy(), u[:, 39].copy(), s[:, 40].copy(), u[:, 39].copy()
        U = np.repeat(u[:, 40:40 + H].T.copy()[None], C, axis=0)
        rng = np.random.RandomState(1000 * C + H)
        U[1:] = np.clip(U[1:] + rng.uniform(-0.03, 0.03, (C - 1, H, 2)), UMIN, UMAX)
        v, t = np.hypot(x0[3], x0[4]), np.arange(H + 1) * TS
        xref = np.vstack([x0[0] + v * np.cos(x0[2]) * t + 0.01, x0[1] + v * np.sin(x0[2]) * t - 0.02])
        bank = generate_bank(N, seed=97)
        K = min(5, N)
        win = O.LookbackWindow(N, 1, K)
        sel, topk, cref = O.plan_cpu(shared(), bank, win, x_prev, u_prev, x0, U, xref, uprev, TS, Q, R, P)
        for a in (bank, U, xref, cref):
            a.setflags(write=False)
        _CASE[name] = dict(N=N, C=C, H=H, K=K, bank=bank, args=(x_prev, u_prev, x0, U, xref, uprev), sel=int(sel),
                           cref=cref)
    return _CASE[name]


def device_tick(nat, b, cs, c, buf):
    """llampc_plan_device with the input pack at the end of `buf`; returns (PlanOut, costs)."""
    import torch
    x_prev, u_prev, x0, U, xref, uprev = c["args"]
    pack = np.concatenate([x_prev, u_prev, x0, uprev, xref.ravel(), U.ravel()]).astype(np.float64)
    tail = buf[buf.numel() - pack.nbytes:]
    tail.copy_(torch.from_numpy(pack.view(np.uint8)))
    assert tail.data_ptr() + pack.nbytes == buf.data_ptr() + ALLOC_BYTES and tail.data_ptr() % 8 == 0
    base, H = tail.data_ptr(), c["H"]
    pin = nat.PlanIn()
    pin.x_prev, pin.u_prev, pin.x_now, pin.uprev = base, base + 8 * 6, base + 8 * 8, base + 8 * 14
    pin.xref, pin.U = base + 8 * 16, base + 8 * (16 + 2 * (H + 1))
    pin.C, pin.H, pin.K = c["C"], H, c["K"]
    pin.integrator = nat.INTEGRATORS["rk4"]
    pin.do_lookback, pin.do_lookahead = 1, 1
    pin.nan_policy = nat.NAN_FIRST
    pin.Ts = TS
    pin.cost = cs
    d_out = torch.zeros(nat.PLAN_OUT_BYTES, dtype=torch.uint8, device=buf.device)
    d_cost = torch.full((c["N"], c["C"]), float("nan"), dtype=torch.float64, device=buf.device)
    torch.cuda.synchronize()
    nat.check(nat.load().llampc_plan_device(b.handle, ctypes.byref(pin), d_out.data_ptr(), None, None,
                                            d_cost.data_ptr(), None))
    torch.cuda.synchronize()
    return nat.PlanOut.from_buffer_copy(d_out.cpu().numpy().tobytes()), d_cost.cpu().numpy()


def same_records(nat, got, want, what):
    A, B = nat.plan_out_to_dict(got), nat.plan_out_to_dict(want)
    assert A["status"] == 0 and B["status"] == 0, (what, A["status"], B["status"])
    for k in A:
        if isinstance(A[k], np.ndarray):
            np.testing.assert_array_equal(A[k], B[k], err_msg=f"{what}: {k}")
        else:
            assert A[k] == B[k] or (A[k] != A[k] and B[k] != B[k]), (what, k, A[k], B[k])


@pytest.mark.parametrize("lpm", [4, 2, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_prologue_shapes_and_input_routes(nat, monkeypatch, tail_buffer, name, lpm):
    from llampc.mpc import ModelBank
    c = case(name)
    N, C, H = c["N"], c["C"], c["H"]
    monkeypatch.setenv("LLAMPC_LPM", str(lpm))
    monkeypatch.delenv("LLAMPC_NO_INLINE", raising=False)
    v = nat.plan_variant(N, C, H)
    assert (v["lpm"], bool(v["stage"])) == (lpm, SHAPES[name][3]), (name, lpm, v)
    cs = nat.cost_struct(Q=Q, R=R, P=P)
    banks = [ModelBank(c["bank"], W=1, device=0) for _ in range(3)]
    try:
        dev, costs = device_tick(nat, banks[0], cs, c, tail_buffer)
        inl = banks[1].plan_raw(*c["args"], Ts=TS, K=c["K"], cost=cs)[0]
        os.environ["LLAMPC_NO_INLINE"] = "1"
        try:
            cpy = banks[2].plan_raw(*c["args"], Ts=TS, K=c["K"], cost=cs)[0]
        finally:
            del os.environ["LLAMPC_NO_INLINE"]
    finally:
        for b in banks:
            b.close()

    def bound(idx):
        x_prev, u_prev, x0, U, xref, uprev = c["args"]
        return core_error_bound(shared(), tuple(c["bank"]), x0, U, xref, uprev, Q, R, P, Ts=TS)[idx]

    fin = np.isfinite(c["cref"])
    print(f"PROLOGUE {name} lpm={lpm} G={v['G']} cpl={v['cpl']}: largest relative cost error "
          f"{float(np.max(np.abs(costs[fin] - c['cref'][fin]) / np.abs(c['cref'][fin]))):.2e}")
    assert_costs_close(costs, c["cref"], RTOL_ROLL, bound)
    same_records(nat, inl, dev, "kernel-argument inputs vs device pointers")
    same_records(nat, cpy, dev, "copied inputs vs device pointers")
    o = nat.plan_out_to_dict(dev)
    assert o["window_full"] and o["sel_model"] == c["sel"]
    assert o["sel_cost"] == costs[o["sel_model"], o["sel_cand"]]

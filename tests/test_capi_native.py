"""csrc/capi_host.hpp (the C ABI's pure host helpers: tick numbers, poll bounds, the input
pack, the window unroll, the raceline view and the launch fields that come from the bank)
compiled for the host with AddressSanitizer and UBSan and run on the CPU.  The harness
(tests/native/capi_host.cpp) prints values; what they must be is worked out here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INT32_MAX, UINT32_MAX, U64_MAX = 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 64 - 1
XREF_GIVEN, XREF_RACELINE = 0, 1
RK4, EULER_NLP, RK6 = 0, 1, 2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("capi") / "capi_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer",
           f"-I{os.path.join(REPO, 'lla-mpc_amd', 'csrc')}", f"-I{os.path.join(REPO, 'include')}",
           os.path.join(REPO, "tests", "native", "capi_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)

    def run(*args, env=None):
        e = {k: v for k, v in os.environ.items() if not k.startswith("LLAMPC_POLL_")}
        e.update(ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1", **(env or {}))
        r = subprocess.run([out, *map(str, args)], capture_output=True, text=True, env=e)
        assert r.returncode == 0, r.stderr
        return r.stdout
    return run


def test_header_enums_match():
    src = open(os.path.join(REPO, "include", "llampc.h")).read()
    for name, val in (("LLAMPC_XREF_GIVEN", XREF_GIVEN), ("LLAMPC_XREF_RACELINE", XREF_RACELINE), ("LLAMPC_RK4", RK4),
                      ("LLAMPC_EULER_NLP", EULER_NLP), ("LLAMPC_RK6", RK6)):
        assert f"{name} = {val}" in src or f"{name}={val}" in src or f"#define {name} {val}" in src, name


def test_next_seq(harness):
    chain = lambda s, k: [int(x) for x in harness("seq", s, k).split()]
    assert chain(0, 2) == [1, 2]
    assert chain(0xFFFFFFFE, 2) == [0xFFFFFFFF, 2]
    seq = [0xFFFFFFFA] + chain(0xFFFFFFFA, 12)          # across the wrap
    assert 0 not in seq
    assert all((a ^ b) & 1 for a, b in zip(seq, seq[1:])), seq   # the mailbox slot alternates


def poll_model(n, C, H, floor_s=2.0, step_ns=40.0):
    steps = float(n) * float(C) * float(H)
    ticks = 1e8 * floor_s + 0.1 * step_ns * steps
    ticks = U64_MAX if ticks >= 1.8e19 else int(ticks)
    units = lambda mx: min(max(((ticks + 0xFFFF) & U64_MAX) >> 16, 1), mx)   # the sum in 64 bits, as the field's
    return [ticks, units(INT32_MAX), units(UINT32_MAX)]


@pytest.mark.parametrize("n,C,H,env", [
    (1, 1, 1, {}),                                               # the default floor alone: 2 s
    (10 ** 7, 64, 40, {}),                                       # the default step term: ~1024 s
    (1, 1, 1, {"LLAMPC_POLL_BOUND_S": "0", "LLAMPC_POLL_STEP_NS": "0"}),        # 0 ticks, 1 unit
    (97, 3, 5, {"LLAMPC_POLL_BOUND_S": "0.001", "LLAMPC_POLL_STEP_NS": "0"}),   # below one unit
    (10 ** 7, 64, 40, {"LLAMPC_POLL_STEP_NS": "76800"}),         # past INT32_MAX units, below UINT32_MAX
    (10 ** 7, 64, 40, {"LLAMPC_POLL_STEP_NS": "1e12"}),          # the ~0ull saturation: the sum wraps, 1 unit
    (10 ** 7, 64, 40, {"LLAMPC_POLL_STEP_NS": "6e9"}),           # 1.5e19 ticks, below it: both clamps
    (1, 1, 1, {"LLAMPC_POLL_BOUND_S": "-3", "LLAMPC_POLL_STEP_NS": "-1"}),      # negatives read as 0
])
def test_poll_bound(harness, n, C, H, env):
    got = [int(x) for x in harness("poll", n, C, H, env=env).split()]
    want = poll_model(n, C, H, max(0.0, float(env.get("LLAMPC_POLL_BOUND_S", 2.0))),
                      max(0.0, float(env.get("LLAMPC_POLL_STEP_NS", 40.0))))
    assert got == want
    assert 1 <= got[1] <= INT32_MAX and 1 <= got[2] <= UINT32_MAX


def test_poll_bound_known_values(harness):
    assert poll_model(1, 1, 1) == [200000004, 3052, 3052]
    assert poll_model(1, 1, 1, 0.0, 0.0) == [0, 1, 1]
    assert poll_model(10 ** 7, 64, 40, 2.0, 1e12) == [U64_MAX, 1, 1]
    assert poll_model(10 ** 7, 64, 40, 2.0, 6e9)[1:] == [INT32_MAX, UINT32_MAX]
    t, a, b = poll_model(10 ** 7, 64, 40, 2.0, 76800.0)
    assert a == INT32_MAX < b < UINT32_MAX
    for ticks, mx, want in ((0, 7, 1), (1, 7, 1), (0x10000, 7, 1), (0x10001, 7, 2), (0x70000, 7, 7), (0x70001, 7, 7),
                            (U64_MAX, UINT32_MAX, 1), (U64_MAX - 0xFFFF, U64_MAX, 2 ** 48 - 1),
                            (U64_MAX - 0xFFFE, U64_MAX, 1)):
        assert int(harness("units", ticks, mx)) == want, (ticks, mx)


@pytest.mark.parametrize("C,H,mode,la,prev", [
    (1, 1, XREF_GIVEN, 1, 1), (2, 3, XREF_GIVEN, 1, 1), (1, 1, XREF_RACELINE, 1, 1), (2, 3, XREF_RACELINE, 1, 1),
    (2, 3, XREF_GIVEN, 0, 1), (2, 3, XREF_GIVEN, 1, 0), (2, 3, XREF_RACELINE, 0, 0)])
def test_pack(harness, C, H, mode, la, prev):
    """x_prev[6] u_prev[2] x_now[6] uprev[2] xref[2][H+1] U[C][H][2]; the harness packs into a heap
    block of exactly pack_len doubles from inputs of exactly their documented sizes."""
    out = harness("pack", C, H, mode, la, prev).split()
    n, got = int(out[0]), np.array(out[1:], dtype=np.float64)
    ramp = lambda k, base: base + np.arange(k, dtype=np.float64)
    head = np.concatenate([ramp(6, 100) if prev else np.zeros(6), ramp(2, 200) if prev else np.zeros(2), ramp(6, 300),
                           ramp(2, 400)])
    if not la:
        # look-ahead off: 16 doubles; the pack's empty xref[2][1] (H = 0) keeps the harness's fill
        assert n == 18
        np.testing.assert_array_equal(got, np.concatenate([head, np.full(2, -7.0)]))
        return
    xref = ramp(2 * (H + 1), 500)
    if mode == XREF_RACELINE:
        xref = np.concatenate([ramp(3, 500), np.zeros(2 * (H + 1) - 3)])
    want = np.concatenate([head, xref, ramp(2 * C * H, 1000)])
    assert n == 16 + 2 * (H + 1) + 2 * C * H == len(got)
    np.testing.assert_array_equal(got, want)


def test_window_unroll(harness):
    """The ring [W][n] (row `slot` written next, `count` rows filled) as rt.py's [n][W]: the newest
    entry in column W-1, unfilled columns zero — every (count, slot) at W = 3, n = 2."""
    W, n = 3, 2
    raw = 10.0 * np.arange(W)[:, None] + np.arange(n)[None, :] + 1.0
    rows = harness("window", W, n).strip().splitlines()
    cases = [(c, s) for c in range(W + 1) for s in range(W)]
    assert len(rows) == len(cases)
    for (count, slot), row in zip(cases, rows):
        hist = [raw[(slot - 1 - age) % W] for age in range(count)]          # newest first
        want = np.zeros((n, W))
        if hist:
            want[:, W - count:] = np.array(hist[::-1]).T
        np.testing.assert_array_equal(np.array(row.split(), dtype=np.float64).reshape(n, W), want, err_msg=str((count, slot)))


def test_raceline_view(harness):
    """knots[n] | xy[2][4][n-1] | speed[M][4][n-1] | mus[M] at n = 5, M = 2."""
    f = harness("raceline").split()
    n, M = 5, 2
    assert int(f[0], 16) == 0x80000
    assert [int(x) for x in f[1:7]] == [n, n + 8 * (n - 1), n + 8 * (n - 1) + 4 * (n - 1) * M, n, M, 0]
    assert [float(x) for x in f[7:]] == [0.25, 3.5]


@pytest.mark.parametrize("integrator", [RK4, EULER_NLP, RK6])
def test_launch_builders(harness, integrator):
    """A plan tick and a controller tick take the same bank fields: each builder's output is the
    bank's addresses and sizes, whichever tick asks (the NLP form alone drops input_acc / approx)."""
    rows = {}
    for ln in harness("builders", integrator).strip().splitlines():
        who, part, *vals = ln.split()
        rows[who, part] = vals
    addr = lambda *a: [format(x, "x") for x in a]
    lb = addr(0x1000) + ["5", "70", "0.5", "0.25"] + addr(0x2000) + ["3", "2"] + \
        addr(0x3000, 0x4000, 0x5000, 0x6000, 0x7000)
    fin = addr(0x1000) + ["5", "70"] + addr(0x4000, 0x5000, 0x6000, 0x7000)
    for who in ("plan", "ctl"):
        assert rows[who, "lb"] == lb and rows[who, "fin"] == fin, who
    keep = lambda integ: "0" if integ == EULER_NLP else "1"
    la = lambda integ: addr(0x1000) + ["5", "70", "0.5", "0.25", keep(integ), keep(integ), str(integ)]
    assert rows["plan", "la"] == la(integrator) and rows["ctl", "la"] == la(RK4)
    assert rows["plan", "la"][:5] == rows["ctl", "la"][:5]


@pytest.mark.parametrize("code", [-1, -2, -3, -6])
def test_spin_for_tag(harness, code):
    """The three outcomes and the callback's own code stay apart: an LLAMPC_E_* code that on_timeout
    returns (a failed synchronise: LLAMPC_E_HIP = -2) comes back as it is, never as the timeout."""
    now, late, consts = (list(map(int, ln.split())) for ln in harness("spin", code).strip().splitlines())
    stopped, timeout, e_arg, e_hip = consts
    assert (e_arg, e_hip) == (-1, -2) and stopped > 0 and timeout > 0 and stopped != timeout
    assert now == [0, stopped, 0]                    # arrived; stopped; on_timeout never ran
    assert late == [code, timeout, 0, 3]             # passed on; timed out; arrived during on_timeout

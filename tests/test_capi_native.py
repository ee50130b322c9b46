"""csrc/capi_host.hpp (the C ABI's pure host helpers: tick numbers, poll bounds, the input
pack, the window unroll, the raceline view, the launch fields that come from the bank, the plan
tick's prepare / commit, its track state's layout, its entries' refusals, the controller launch's
shape, and the controller tick's prepare / commit, speculative look-ahead decision, corridor layout,
doorbell words and entries' refusals) and csrc/launch_shape.hpp (the plan launch's shape) compiled for the
host with AddressSanitizer and UBSan and run on the CPU.  The harness (tests/native/capi_host.cpp)
prints values; what they must be is worked out here."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from lookback_matrix import SHAPE_ROWS as LOOKBACK_MATRIX_SHAPES

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
        e = {k: v for k, v in os.environ.items() if not k.startswith("LLAMPC_")}   # every knob: the test's own
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


# ---- the plan launch's shape (csrc/launch_shape.hpp plan_shape) and the controller's (ctl_shape) ----------
# The rule, restated here from DESIGN.md ("The launch dispatch") and the header's comments; the harness's
# `shape` mode prints every PlanShape field for the PlanShapeIn fields and the CU count it is given.
KIB = 1024
BLOCK, WAVES, KMAX = 256, 4, 32
SCRATCH = 192                                   # the carve every block role starts with
RANK_BYTES = 64 * 8 + 64 * 4 + 256              # a wave's ranking lists
ENT, ENTS, BENT = 16, 24, 24                    # sizeof(Ent), sizeof(EntS), sizeof(BEnt)
PLAN_OUT = 16 + 16 + 24 + 24 + KMAX * (8 + 8 + 8 + 8 + 4 + 8)   # sizeof(llampc_plan_out), test_host_cpu.py
KNOT_PAD = 8
STAGE_LIMIT, ONE_BLOCK_PER_CU, PLAN_LDS_MAX = 128 * KIB, 82 * KIB, 159 * KIB
INLINE_DOUBLES, PEER_FUSE_MAX = 352, 16
PLAIN, INLINE, CORRIDOR = 0, 1, 2
SHAPE_DEFAULTS = dict(n=0, K=0, lb=0, full=0, la=0, C=0, H=0, integrator=RK4, xref_mode=XREF_GIVEN, rl_n=0, rl_M=0,
                      share=1, px_G=0, pack=0, corridor=0, wq_counter=0)
NO = dict(
    corridor_la="the corridor belongs to the look-ahead: do_lookahead is 0",
    corridor_rk6="the corridor look-ahead has no RK6 rollout",
    corridor_raceline="the corridor look-ahead takes the given xref only (not LLAMPC_XREF_RACELINE)",
    corridor_inputs="the corridor launch takes device inputs and no fused peer exchange",
    integrator="unknown integrator",
    work="nothing to launch: no look-back and no look-ahead block",
    peer="the fused peer exchange: RK4, the given xref, device inputs, at most kPeerFuseMax ranks",
    pack="the inline pack: an RK4 look-ahead on the given xref, staged, within kInlineDoubles")


def cdiv(a, b):
    return -(-a // b)


def group(C):
    G = 1
    while G < C and G < BLOCK:
        G *= 2
    return G


def lpm_rule(n, C, integrator, share, env):
    """4 lanes per rollout up to 16384 lanes (n G share), 2 up to 32768, else 1, each only while
    lpm G <= 256; RK6 always 1; LLAMPC_LPM taken while v G <= 256."""
    if integrator == RK6:
        return 1
    G = group(C)
    v = int(env.get("LLAMPC_LPM", 0))
    if v == 1 or (v in (2, 4) and v * G <= BLOCK):
        return v
    lanes = n * G * max(share, 1)
    if lanes <= 16384 and 4 * G <= BLOCK:
        return 4
    return 2 if lanes <= 32768 and 2 * G <= BLOCK else 1


def lookahead_lds(C, H, extra=0):
    """scratch + xref [H+1][2] + extra, and the staged inputs (64 B per candidate and step) while all of
    it stays within 128 KiB."""
    base, ub = SCRATCH + 16 * (H + 1) + extra, 64 * C * H
    return (base + ub, True) if base + ub <= STAGE_LIMIT else (base, False)


def lookback_r(n, K):
    return max(1, cdiv(n, BLOCK * max(1, min(640 // max(1, K), 64 * 8 // WAVES))))


def lb_final_lds(nb_lb, K):
    M, L = nb_lb * K, nb_lb
    return max(SCRATCH + 8 * (3 * M + L) + ENT * L * WAVES + 4 * (3 * M + L + KMAX + 2) + 8 + 16,
               SCRATCH + WAVES * RANK_BYTES + WAVES * KMAX * BENT)


def raceline_lds(n, M):
    return 8 * (n + KNOT_PAD) + 64 * (n - 1) + 8 * ((M + 1) & ~1)


def shape_model(cus, env, **fields):
    f = dict(SHAPE_DEFAULTS, **fields)
    n, C, H, la, lb = f["n"], f["C"], f["H"], f["la"], f["lb"]
    integ = f["integrator"] if la else RK4
    raceline = bool(la) and f["xref_mode"] == XREF_RACELINE
    given = f["xref_mode"] == XREF_GIVEN
    if f["corridor"]:
        for bad, why in ((not la, "corridor_la"), (f["integrator"] == RK6, "corridor_rk6"), (not given, "corridor_raceline"),
                         (f["pack"] or f["px_G"], "corridor_inputs")):
            if bad:
                return dict(refuse=NO[why])
    if f["px_G"] and (f["pack"] or integ != RK4 or raceline or f["px_G"] > PEER_FUSE_MAX):
        return dict(refuse=NO["peer"])
    if f["pack"] and (not la or integ != RK4 or not given or C < 1 or H < 1):
        return dict(refuse=NO["pack"])
    if integ not in (RK4, EULER_NLP, RK6):
        return dict(refuse=NO["integrator"])
    s = dict(family=CORRIDOR if f["corridor"] else INLINE if f["pack"] else PLAIN, integ=integ, lpm=1, G=1, cpl=1, stage=0,
             wq=0, px=int(f["px_G"] != 0), xm=int(raceline), R=0, nb_lb=0, nb_la=0, threads=BLOCK, wcap=0, refuse="-")
    lds = SCRATCH
    if lb:
        s["R"] = max(lookback_r(n, max(1, f["K"])), max(1, int(env.get("LLAMPC_LB_R", 1))))
        s["nb_lb"] = cdiv(n, BLOCK * s["R"])
        if f["full"]:
            lds = max(lds, lb_final_lds(s["nb_lb"], f["K"]))
    if la:
        s["G"] = group(C)
        s["cpl"] = cdiv(C, s["G"])
        s["lpm"] = lpm_rule(n, C, integ, f["share"], env)
        s["nb_la"] = cdiv(n, BLOCK // (s["G"] * s["lpm"]))
        if raceline:
            # the knots and rows, the staged inputs if they fit beside them, the rest for the speed window
            rl, per_seg = raceline_lds(f["rl_n"], f["rl_M"]), 32 * max(1, f["rl_M"])
            base, stage = lookahead_lds(C, H)
            if base + rl > PLAN_LDS_MAX:
                base, stage = SCRATCH + 16 * (H + 1), False
            s["wcap"] = min(max(PLAN_LDS_MAX - base - rl, 0) // per_seg, f["rl_n"] - 1)
            lds = max(lds, base + rl + per_seg * s["wcap"])
        else:
            b, stage = lookahead_lds(C, H, 48 * H if f["corridor"] else 0)
            lds = max(lds, b)
        s["stage"] = int(stage)
    if s["nb_lb"] + s["nb_la"] == 0:
        return dict(refuse=NO["work"])
    if (la and f["wq_counter"] and s["lpm"] == 1 and s["G"] <= 64 and integ == RK4 and given and not f["pack"]
            and not f["corridor"] and "LLAMPC_NO_WQ" not in env):
        nw, forced = max(1, cus - 1), int(env.get("LLAMPC_WQ_WAVES", 0))
        if 4 * s["nb_la"] >= 7 * nw or (forced and s["nb_la"] > nw):
            units = cdiv(n, 64 // s["G"])
            s["nb_la"] = nw
            s["wq"] = 2 if s["stage"] and (forced == 8 if forced else units >= 4 * nw * WAVES) else 1
            s["threads"] = 512 if s["wq"] == 2 else BLOCK
    if f["px_G"]:
        lds = max(lds, 256 + f["px_G"] * (PLAN_OUT + 2 * KMAX * ENTS) + WAVES * 4)
    if f["pack"] and (not s["stage"] or 16 + 2 * (H + 1) + 2 * C * H > INLINE_DOUBLES):
        return dict(refuse=NO["pack"])
    s["lds"] = max(lds, ONE_BLOCK_PER_CU)
    return s


def parse_fields(text):
    out = {}
    for ln in text.strip().splitlines():
        k, _, v = ln.partition(" ")
        out[k] = v if k == "refuse" else int(v)
    return out


@pytest.fixture(scope="module")
def shape(harness):
    """shape(cus, env=None, **fields): the harness's PlanShape, checked against shape_model field by field."""
    def run(cus, env=None, **fields):
        got = parse_fields(harness("shape", cus, *(f"{k}={int(v)}" for k, v in fields.items()), env=env))
        want = shape_model(cus, env or {}, **fields)
        if want["refuse"] != "-":
            assert got["refuse"] == want["refuse"], (fields, got)
        else:
            assert got == want, (cus, env, fields)
        return got
    return run


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    return _native


def test_shape_lpm_and_groups(shape):
    """test_plan_variant_dispatch's cases (test_host_cpu.py) on the whole struct: the LPM thresholds
    with share, RK6, the width limit, G / cpl from C, the LLAMPC_LPM override."""
    la = lambda n, C_, integ=RK4, share=1, env=None: shape(256, env, n=n, la=1, C=C_, H=12, integrator=integ, share=share)
    for integ in (RK4, EULER_NLP):
        assert [la(n, 1, integ)["lpm"] for n in (16384, 16385, 32768, 32769)] == [4, 2, 2, 1]
        assert [la(n, 64, integ)["lpm"] for n in (256, 257, 512, 513)] == [4, 2, 2, 1]
        assert [la(n, 1, integ, 2)["lpm"] for n in (8192, 8193, 16384, 16385)] == [4, 2, 2, 1]
        assert [la(n, 64, integ, 2)["lpm"] for n in (128, 129, 256, 257)] == [4, 2, 2, 1]
    assert [la(n, C_, RK6)["lpm"] for n, C_ in ((1, 1), (97, 3), (97, 64), (10 ** 5, 1))] == [1, 1, 1, 1]
    assert [la(3, C_)["lpm"] for C_ in (64, 65, 128, 129, 256, 1000)] == [4, 2, 2, 1, 1, 1]
    for C_, G, cpl in ((1, 1, 1), (2, 2, 1), (3, 4, 1), (64, 64, 1), (65, 128, 1), (130, 256, 1), (257, 256, 2),
                       (1000, 256, 4)):
        v = la(97, C_)
        assert (v["G"], v["cpl"], v["family"], v["integ"], v["threads"]) == (G, cpl, PLAIN, RK4, 256), (C_, v)
        assert v["nb_la"] == cdiv(97, 256 // (G * v["lpm"])) and v["nb_lb"] == 0 and v["R"] == 0
    for env, cases in (("4", ((10 ** 6, 64, 4), (97, 65, 2), (97, 130, 1))), ("2", ((10 ** 6, 128, 2), (97, 3, 2), (97, 130, 1))),
                       ("1", ((97, 3, 1), (97, 130, 1))), ("3", ((97, 3, 4), (10 ** 6, 3, 1)))):
        for n, C_, want in cases:
            assert la(n, C_, env={"LLAMPC_LPM": env})["lpm"] == want, (env, n, C_)
        assert la(97, 3, RK6, env={"LLAMPC_LPM": env})["lpm"] == 1


WQ = dict(la=1, C=64, H=20, integrator=RK4, wq_counter=1, lb=1, K=10)


def test_shape_work_queue_taken(shape):
    """256 CUs, G = 64, LPM 1, RK4: one block per four models, so the queue opens at the first n with
    4 ceil(n / 4) >= 255 x 7 = 1785 and runs 255 blocks; 8 waves from 4 x 255 x 4 = 4080 units (models,
    at G = 64) on, when staged; the knobs."""
    at = lambda n, env=None, **kw: shape(256, env, **dict(WQ, n=n, **kw))
    assert 4 * cdiv(1784, 4) < 1785 <= 4 * cdiv(1785, 4)
    a, b = at(1784), at(1785)
    assert (a["wq"], a["nb_la"], a["lpm"]) == (0, 446, 1) and (b["wq"], b["nb_la"], b["threads"]) == (1, 255, 256)
    a, b = at(4079), at(4080)
    assert (a["wq"], a["nb_la"], a["threads"]) == (1, 255, 256) and (b["wq"], b["nb_la"], b["threads"]) == (2, 255, 512)
    u = at(4080, H=32)                                           # C = 64, H = 32: unstaged, never 8 waves
    assert (u["stage"], u["wq"], u["threads"]) == (0, 1, 256)
    assert (at(5000, {"LLAMPC_NO_WQ": "1"})["wq"], at(5000, {"LLAMPC_NO_WQ": "1"})["nb_la"]) == (0, 1250)
    assert at(1785, {"LLAMPC_WQ_WAVES": "8"})["wq"] == 2 and at(5000, {"LLAMPC_WQ_WAVES": "4"})["wq"] == 1
    assert at(4080, {"LLAMPC_WQ_WAVES": "8"}, H=32)["wq"] == 1   # unstaged: 4 waves even when 8 are forced
    # a forced block size opens the queue as soon as there are more blocks than CUs - 1
    assert at(1100)["wq"] == 0 and (at(1100, {"LLAMPC_WQ_WAVES": "4"})["wq"], at(1100, {"LLAMPC_WQ_WAVES": "4"})["nb_la"]) == (1, 255)
    assert at(1020, {"LLAMPC_WQ_WAVES": "4"})["wq"] == 0         # 255 blocks: not more than 255
    # G = 8: 32 models per block, 8 per wave: open from 447 blocks (n = 14273), 8 waves from 4080 units (n = 32633)
    g8 = lambda n: shape(256, None, **dict(WQ, n=n, C=8))
    assert [g8(n)["wq"] for n in (14272, 14273, 32632, 32633)] == [0, 1, 1, 2]
    # the CU count is an argument: 8 CUs, 7 blocks, open from 13 blocks, 8 waves from 112 units
    s = shape(8, None, **dict(WQ, n=513))
    assert (s["wq"], s["nb_la"], s["threads"]) == (2, 7, 512)
    assert shape(104, None, **dict(WQ, n=1785))["nb_la"] == 103


@pytest.mark.parametrize("why,kw", [
    ("G > 64", dict(C=65)), ("NLP-Euler", dict(integrator=EULER_NLP)), ("RK6", dict(integrator=RK6)),
    ("the raceline", dict(xref_mode=XREF_RACELINE, rl_n=700, rl_M=3)), ("an inline pack", dict(pack=1, H=2)),
    ("a corridor", dict(corridor=1)), ("no counter", dict(wq_counter=0)), ("LPM 2 forced", dict(env={"LLAMPC_LPM": "2"}))])
def test_shape_work_queue_never_taken(shape, why, kw):
    kw = dict(kw)
    env = kw.pop("env", None)
    s = shape(256, env, **dict(WQ, n=5000, **kw))
    assert s["wq"] == 0 and s["threads"] == 256 and s["nb_la"] == cdiv(5000, 256 // (s["G"] * s["lpm"])), (why, s)
    assert shape(256, None, **dict(WQ, n=5000))["wq"] == 2      # the same launch without it


@pytest.mark.parametrize("C_", [1, 3, 64, 130, 256])
def test_shape_staging_boundary(shape, C_):
    """Staged while 192 + 16 (H + 1) + 64 C H (+ 48 H with a corridor) <= 128 KiB: the last H that fits
    and the next, without and with the corridor."""
    for corridor, per_h in ((0, 16 + 64 * C_), (1, 16 + 48 + 64 * C_)):
        H = (STAGE_LIMIT - SCRATCH - 16) // per_h
        a, b = (shape(256, None, n=97, la=1, C=C_, H=h, corridor=corridor) for h in (H, H + 1))
        assert (a["stage"], b["stage"]) == (1, 0), (C_, corridor, H)
        assert a["lds"] == SCRATCH + 16 + per_h * H > ONE_BLOCK_PER_CU == b["lds"]
        assert a["family"] == (CORRIDOR if corridor else PLAIN)


def test_shape_staged_without_corridor_unstaged_with(shape):
    a, b = (shape(256, None, n=97, la=1, C=31, H=64, corridor=c) for c in (0, 1))
    assert (a["stage"], b["stage"]) == (1, 0)
    assert 192 + 16 * 65 + 64 * 31 * 64 <= STAGE_LIMIT < 192 + 16 * 65 + 48 * 64 + 64 * 31 * 64


def test_shape_lds_requests(shape):
    """Every request is at least 82 KiB (one block per CU).  The look-back's terms (lb_final's region and
    the waves' ranking lists, at most ~25 KB while nb_lb K stays near 640) and the peer exchange's (3024 B
    per rank, 16 ranks at most) never pass that floor on their own: the model holds them, the total shows
    the floor — test_ctl_shape shows both terms where no floor hides them.  The staged inputs and the
    raceline's window do pass it."""
    assert shape(256, None, n=97, la=1, C=3, H=12)["lds"] == ONE_BLOCK_PER_CU
    assert lb_final_lds(20, 32) == 192 + 8 * 1940 + 16 * 80 + 4 * 1974 + 24 == 24912 < ONE_BLOCK_PER_CU
    assert lb_final_lds(1, 1) == 192 + 4 * 1024 + 4 * 32 * 24 == 7360
    assert shape(256, None, n=5120, lb=1, full=1, K=32)["lds"] == ONE_BLOCK_PER_CU
    assert shape(256, None, n=5120, lb=1, full=0, K=32, la=1, C=3, H=12)["lds"] == ONE_BLOCK_PER_CU
    for G in (2, 16):
        assert 256 + G * (1488 + 1536) + 16 < ONE_BLOCK_PER_CU
        s = shape(256, None, n=5120, lb=1, full=1, K=10, la=1, C=3, H=12, px_G=G)
        assert (s["px"], s["lds"]) == (1, ONE_BLOCK_PER_CU)
    s = shape(256, None, n=5120, lb=1, full=1, K=10, la=1, C=64, H=31, px_G=16)
    assert (s["stage"], s["lds"]) == (1, 192 + 16 * 32 + 64 * 64 * 31)
    # the raceline: 700 knots, 3 frictions: 50432 B of tables beside 10768 B of staged inputs leave room for
    # 1058 segments of 96 B: the whole lap (699); 8 frictions (256 B per segment): 396 segments
    rl = dict(n=97, la=1, C=8, H=20, xref_mode=XREF_RACELINE, rl_n=700)
    a, b = shape(256, None, rl_M=3, **rl), shape(256, None, rl_M=8, **rl)
    assert raceline_lds(700, 3) == 50432 and lookahead_lds(8, 20) == (10768, True)
    assert (a["xm"], a["stage"], a["wcap"], a["lds"]) == (1, 1, 699, 10768 + 50432 + 96 * 699)
    assert (b["wcap"], b["lds"]) == (396, 10768 + 50464 + 256 * 396) and b["lds"] <= PLAN_LDS_MAX
    # inputs that are staged on their own but not beside the tables go unstaged
    c = shape(256, None, rl_M=3, **dict(rl, C=64, H=31))
    assert lookahead_lds(64, 31)[1] and (c["stage"], c["wcap"]) == (0, 699)


@pytest.mark.parametrize("why,kw", [
    ("corridor_rk6", dict(corridor=1, integrator=RK6)),
    ("corridor_raceline", dict(corridor=1, xref_mode=XREF_RACELINE, rl_n=700, rl_M=3)),
    ("corridor_inputs", dict(corridor=1, pack=1, H=2)),
    ("corridor_inputs", dict(corridor=1, px_G=2)),
    ("corridor_la", dict(corridor=1, la=0, lb=1, K=10)),
    ("corridor_la", dict(corridor=1, la=0, C=-5, H=2 ** 31 - 1)),      # refused before any size is worked out
    ("integrator", dict(corridor=1, integrator=7)),
    ("integrator", dict(integrator=7)), ("integrator", dict(integrator=-1)),
    ("pack", dict(pack=1, C=64, H=40)),
    ("pack", dict(pack=1, C=8, H=40)),
    ("pack", dict(pack=1, la=0, lb=1, K=10)),
    ("pack", dict(pack=1, integrator=EULER_NLP, H=2)), ("pack", dict(pack=1, integrator=RK6, H=2)),
    ("pack", dict(pack=1, xref_mode=XREF_RACELINE, rl_n=700, rl_M=3, H=2)),
    ("peer", dict(px_G=17)),
    ("peer", dict(px_G=2, integrator=EULER_NLP)), ("peer", dict(px_G=2, integrator=RK6)),
    ("peer", dict(px_G=2, xref_mode=XREF_RACELINE, rl_n=700, rl_M=3)),
    ("peer", dict(px_G=2, pack=1, H=2)),
    ("work", dict(la=0)), ("work", dict(la=0, lb=1, n=0, K=10))])
def test_shape_refusals(shape, why, kw):
    got = shape(256, None, **dict(dict(n=97, la=1, C=3, H=12), **kw))
    assert got["refuse"] == NO[why], (kw, got)


def test_shape_accepts_what_it_should(shape):
    """The neighbours of the refusals: each family's plain case, 16 ranks, the largest pack."""
    base = dict(n=97, la=1, C=3, H=12)
    for kw, family in ((dict(), PLAIN), (dict(corridor=1), CORRIDOR), (dict(corridor=1, integrator=EULER_NLP), CORRIDOR),
                       (dict(pack=1), INLINE), (dict(px_G=16, lb=1, K=10), PLAIN), (dict(integrator=RK6), PLAIN),
                       (dict(la=0, lb=1, K=10), PLAIN), (dict(pack=1, C=8, H=18), INLINE)):
        s = shape(256, None, **dict(base, **kw))
        assert s["refuse"] == "-" and s["family"] == family, (kw, s)
    assert 16 + 2 * 19 + 2 * 8 * 18 <= INLINE_DOUBLES < 16 + 2 * 20 + 2 * 8 * 19
    assert shape(256, None, **dict(base, pack=1, C=8, H=19))["refuse"] == NO["pack"]


SHAPE_BLOCK_ROWS = [
    (1, 32768, 1, 128), (1, 32769, 2, 65),        # 64 x 8 / 4 = 128 blocks at most per R step
    (10, 16384, 1, 64), (10, 16385, 2, 33),       # 640 // 10 = 64 blocks
    (32, 5120, 1, 20), (32, 5121, 2, 11),         # 640 // 32 = 20 blocks
    (10, 1, 1, 1), (10, 256, 1, 1), (10, 257, 1, 2)]
# + the look-back matrix's stated (K, N, R, L), those not already above (two are: the same ids)
SHAPE_BLOCK_ROWS += [r for r in LOOKBACK_MATRIX_SHAPES if r not in SHAPE_BLOCK_ROWS]


@pytest.mark.parametrize("K,n,R,nb_lb", SHAPE_BLOCK_ROWS)
def test_shape_block_counts(shape, K, n, R, nb_lb):
    for full in (0, 1):
        s = shape(256, None, n=n, lb=1, full=full, K=K)
        assert (s["R"], s["nb_lb"], s["nb_la"]) == (R, nb_lb, 0)
    s = shape(256, {"LLAMPC_LB_R": "3"}, n=n, lb=1, K=K)
    assert (s["R"], s["nb_lb"]) == (max(R, 3), cdiv(n, 256 * max(R, 3)))


def test_plan_variant_entries_agree_with_shape(harness, nat, monkeypatch):
    """llampc_plan_variant and llampc_plan_variant_corridor are plan_shape's (lpm, G, cpl, stage)."""
    four = lambda s: dict(lpm=s["lpm"], G=s["G"], cpl=s["cpl"], stage=bool(s["stage"]))
    for lpm_env in (None, "2"):
        env = {"LLAMPC_LPM": lpm_env} if lpm_env else {}
        monkeypatch.delenv("LLAMPC_LPM", raising=False)
        if lpm_env:
            monkeypatch.setenv("LLAMPC_LPM", lpm_env)
        for n in (1, 257, 513, 10 ** 5):
            for C_, H in ((1, 12), (3, 12), (31, 64), (64, 31), (64, 32), (65, 20), (130, 15), (257, 4)):
                for integ in (RK4, EULER_NLP, RK6):
                    for share in (1, 2):
                        args = dict(n=n, la=1, C=C_, H=H, integrator=integ, share=share)
                        got = parse_fields(harness("shape", 256, *(f"{k}={v}" for k, v in args.items()), env=env))
                        assert nat.plan_variant(n, C_, H, integ, share) == four(got), (args, lpm_env)
                        if integ != RK6:
                            got = parse_fields(harness("shape", 256, "corridor=1", *(f"{k}={v}" for k, v in args.items()), env=env))
                            assert nat.plan_variant_corridor(n, C_, H, integ, share) == four(got), (args, lpm_env)


def ctl_lds_model(H, C, n, s4):
    """ctl_lds.hpp: xref | U | knots + pad | two profiles | (s4) the staged terms | 1 KiB, 16-B aligned."""
    a16 = lambda x: (x + 15) & ~15
    o = a16(SCRATCH + 16 * (H + 1))
    o = a16(o + 16 * C * H)
    o = a16(o + 8 * (n + KNOT_PAD))
    o = a16(o + 64 * (n - 1))
    if s4:
        o = a16(o + 16 * C * H + 16 * C)
    return o + 1024


def test_ctl_shape(harness, nat, monkeypatch):
    """ctl_shape on the CPU: llampc_ctl_variant's nine fields are its own, and its LDS request is the
    largest of the look-ahead layout, lb_final's region / the ranking lists and the exchange's region,
    16-B aligned, plus the completing block's 4 KiB."""
    monkeypatch.delenv("LLAMPC_CTL_NO_STAGE", raising=False)
    ctl = lambda *a: parse_fields(harness("ctl_shape", *a))
    for n, C_, H, K, rl_n in ((1, 1, 1, 1, 700), (200, 8, 20, 10, 700), (10000, 64, 40, 10, 700), (100, 128, 25, 5, 700),
                              (50, 300, 10, 3, 500), (5121, 8, 10, 32, 700), (16385, 8, 10, 10, 700), (100, 96, 20, 10, 700)):
        got = ctl(n, C_, H, K, rl_n, 0, 1, 0, 0)
        assert nat.ctl_variant(n, C_, H, K, rl_n) == {f: got[f] for f in nat.CTL_VARIANT_FIELDS}, (n, C_, H, K, rl_n)
        assert got["nslots"] == K + 1
        want = max(ctl_lds_model(H, C_, rl_n, got["s4"]), lb_final_lds(got["nb_lb"], K))
        assert (got["poll_off"], got["lds"]) == (want, want + 4096)
    # a tiny look-ahead on a two-knot track: the ranking lists (7360 B), then lb_final's region at 20 blocks
    # of K = 32 (24912 B), then the exchange of 16 ranks (192 + 8448 + 8192 + 144 B)
    assert ctl_lds_model(1, 1, 2, True) == 1440
    assert ctl(1, 1, 1, 1, 2, 0, 1, 0, 0)["poll_off"] == 7360
    assert ctl(5120, 1, 1, 32, 2, 0, 1, 0, 0)["poll_off"] == 24912
    assert ctl(1, 1, 1, 32, 2, 0, 1, 0, 16)["poll_off"] == 192 + 4 * 16 * 4 * 33 + 16 * 16 * 32 + 4 * 32 + 16 == 16976
    # warm-up ticks roll one model out; without a look-back one block completes; no_stage drops s4 alone
    w = ctl(200, 8, 20, 10, 700, 1, 0, 0, 0)
    assert (w["nslots"], w["nb_la"], w["nb_lb"]) == (1, 1, 1)
    a, b = ctl(100, 96, 20, 10, 700, 0, 1, 0, 0), ctl(100, 96, 20, 10, 700, 0, 1, 1, 0)
    assert a["s4"] == 1 and b["s4"] == 0 and b["lds"] < a["lds"] and {**a, "s4": 0, "lds": 0, "poll_off": 0} == {**b, "lds": 0, "poll_off": 0}


# ---- the plan tick's host path (capi_host.hpp plan_tick_prepare / plan_tick_commit, plan_track_layout, ----
# ---- the entries' refusals) --------------------------------------------------------------------------
# The harness's `prep` mode runs ticks of one kind on a fake bank (tests/native/capi_host.cpp fake_plan_view:
# distinct addresses that are never dereferenced) and prints every field of the launch structs, of the next
# state and of the bank after plan_tick_commit; prep_model restates kernels.hpp's comments on them.
HMAX, PATH_STRIDE = 64, 65
VIEW = dict(params=0x1000, n=5, goff=70, lf=0.5, mass=0.25, ring=0x2000, W=3, wmean=0x3000, am_val=0x4000, am_idx=0x5000,
            tk_val=0x6000, tk_idx=0x7000, rl=0x80000, rl_n=5, rl_M=2, rl_hmin=0.25, rl_vmax=3.5, best_cand=0x9000,
            best_cost=0xA000, pv=0xB000, pidx=0xC000, pnf=0xD000, la_tag=0xE000, blk_tag=0xF000, wq=0x10000, tickets=0x11000,
            xref_pm=0x12000, track=0x20000, tr_n=4, tr_L=8.0, tr_width=2.4, trk=0x30000, trk_flags=0x40000, hp_tag=0x50000,
            px_box=0x60000, px_G=2, px_rank=1, px_bound=10 ** 9)
IN = dict(x_prev=0x100000, u_prev=0x100100, x_now=0x100200, U=0x100300, xref=0x100400, uprev=0x100500)
TICK = dict(out=0x200000, err=0x201000, wmean=0x202000, cost=0x203000, host_tag=0x204000, host_seq=9, px_merged=0x205000)
PREP_DEFAULTS = dict(lb=1, la=1, xref_mode=XREF_GIVEN, integrator=RK4, C=2, H=3, K=4, Ts=0.02, nan_policy=0, current_model=3,
                     err=0, wmean=0, cost=0, host=0, pk=0, cor=0, px=0, tt=0, tw=1e4, margin=0.05,
                     count=1, slot=2, W=3, seq=7, tseq=11, trk_cur=0, path_H=0, last_H=0, px_seq=5, ticks=1)


def next_seq(s):
    return 2 if s == 0xFFFFFFFF else s + 1


def prep_model(env, **kw):
    """[one dict per tick] of every printed field, as strings the way the harness prints them."""
    a = dict(PREP_DEFAULTS, **kw)
    V, hx, g = VIEW, (lambda p: format(p, "x")), (lambda d: repr(float(d)))
    st = dict(count=a["count"], slot=a["slot"], W=a["W"], seq=a["seq"], tseq=a["tseq"], trk_cur=a["trk_cur"],
              trk_path=a["path_H"], trk_last_H=a["last_H"], px_seq=a["px_seq"] if a["px"] else 0)
    box = a["px_seq"]
    lb, la, tt, px = bool(a["lb"]), bool(a["la"]), bool(a["tt"]), bool(a["px"])
    C, H, K, Ts = a["C"], a["H"], a["K"], a["Ts"]
    nan_first = int(a["nan_policy"] == 0)
    bound = poll_model(V["n"], C, H, max(0.0, float(env.get("LLAMPC_POLL_BOUND_S", 2.0))),
                       max(0.0, float(env.get("LLAMPC_POLL_STEP_NS", 40.0))))[1]
    ticks = []
    for _ in range(a["ticks"]):
        nx = dict(st)
        if lb:                                   # the window advances with a look-back only, and saturates at W
            nx["count"], nx["slot"] = min(st["count"] + 1, st["W"]), (st["slot"] + 1) % st["W"]
        full = int(nx["count"] >= st["W"])
        poll = int(lb and la and "LLAMPC_NO_POLL" not in env)     # a look-back block hosts the poller
        if poll:
            nx["seq"] = next_seq(st["seq"])
        o = {"has.lb": int(lb), "has.la": int(la), "has.tt": int(tt)}
        if lb:
            o.update({"lb.params": hx(V["params"]), "lb.n": V["n"], "lb.goff": V["goff"], "lb.veh.lf": g(V["lf"]),
                      "lb.veh.mass": g(V["mass"]), "lb.x_prev": hx(IN["x_prev"]), "lb.u_prev": hx(IN["u_prev"]),
                      "lb.x_now": hx(IN["x_now"]), "lb.Ts": g(Ts), "lb.ring": hx(V["ring"]), "lb.W": V["W"],
                      "lb.slot": st["slot"], "lb.full": full, "lb.K": K, "lb.nan_first": nan_first, "lb.R": 0,
                      "lb.wm_keep": int(bool(a["wmean"])), "lb.err_out": hx(TICK["err"] if a["err"] else 0),
                      "lb.wm_buf": hx(TICK["wmean"] if a["wmean"] else V["wmean"]), "lb.am_val": hx(V["am_val"]),
                      "lb.am_idx": hx(V["am_idx"]), "lb.tk_val": hx(V["tk_val"]), "lb.tk_idx": hx(V["tk_idx"])})
        if la:
            nlp = a["integrator"] == EULER_NLP
            race = a["xref_mode"] == XREF_RACELINE
            m = V["rl_n"] - 1
            xy = V["rl"] + 8 * V["rl_n"]
            o.update({"la.params": hx(V["params"]), "la.n": V["n"], "la.goff": V["goff"], "la.veh.lf": g(V["lf"]),
                      "la.veh.mass": g(V["mass"]), "la.veh.input_acc": int(not nlp), "la.veh.approx": int(not nlp),
                      "la.x0": hx(IN["x_now"]), "la.U": hx(IN["U"]), "la.xref": hx(IN["xref"]), "la.uprev": hx(IN["uprev"]),
                      "la.C": C, "la.H": H, "la.integrator": a["integrator"], "la.Ts": g(Ts),
                      "la.cost.umin0": g(-0.1), "la.cost.umin1": g(-0.35), "la.cost.umax0": g(1.0), "la.cost.umax1": g(0.35),
                      "la.cost.dmax0": g(-1.0), "la.cost.dmax1": g(2.0 * Ts * (1.0 + 1e-9)), "la.cost.enforce": 1,
                      "la.cost.pad": 0, "la.cost_out": hx(TICK["cost"] if a["cost"] else 0), "la.best_cand": hx(V["best_cand"]),
                      "la.best_cost": hx(V["best_cost"]), "la.pv": hx(V["pv"]), "la.pidx": hx(V["pidx"]), "la.pnf": hx(V["pnf"]),
                      "la.xref_mode": a["xref_mode"],
                      "la.rl.knots": hx(V["rl"] if race else 0), "la.rl.xy": hx(xy if race else 0),
                      "la.rl.speed": hx(xy + 8 * 8 * m if race else 0),
                      "la.rl.mus": hx(xy + 8 * 8 * m + 8 * 4 * m * V["rl_M"] if race else 0),
                      "la.rl.n": V["rl_n"] if race else 0, "la.rl.M": V["rl_M"] if race else 0, "la.rl.wcap": 0,
                      "la.rl.hmin": g(V["rl_hmin"] if race else 0), "la.rl.vmax": g(V["rl_vmax"] if race else 0),
                      "la.xref_pm": hx(V["xref_pm"] if race else 0), "la.la_tag": hx(V["la_tag"]), "la.blk_tag": hx(V["blk_tag"]),
                      "la.seq": nx["seq"], "la.poll": poll, "la.wq": hx(V["wq"])})
            for i in range(4):
                o.update({f"la.cost.Q{i}": g(1 + i), f"la.cost.R{i}": g(10 + i), f"la.cost.P{i}": g(20 + i)})
        if px:
            nx["px_seq"] = next_seq(st["px_seq"])
        o.update({"f.out": hx(TICK["out"]), "f.tickets": hx(V["tickets"]), "f.do_lb": 0, "f.do_la": 0, "f.full": full,
                  "f.window_count": nx["count"], "f.K": K if lb else 0, "f.nan_first": nan_first, "f.nb_lb": 0, "f.nb_la": 0,
                  "f.C": C if la else 1, "f.current_model": a["current_model"], "f.n": V["n"], "f.goff": V["goff"],
                  "f.params": hx(V["params"]), "f.best_cand": hx(V["best_cand"]), "f.best_cost": hx(V["best_cost"]),
                  "f.am_val": hx(V["am_val"]), "f.am_idx": hx(V["am_idx"]), "f.tk_val": hx(V["tk_val"]),
                  "f.tk_idx": hx(V["tk_idx"]), "f.pv": hx(V["pv"]), "f.pidx": hx(V["pidx"]), "f.pnf": hx(V["pnf"]),
                  "f.la_tag": hx(V["la_tag"]), "f.blk_tag": hx(V["blk_tag"]), "f.seq": nx["seq"], "f.poll": bound if poll else 0,
                  "f.host_tag": hx(TICK["host_tag"] if a["host"] else 0), "f.host_seq": TICK["host_seq"] if a["host"] else 0,
                  "f.px_box": hx(V["px_box"] if px else 0), "f.px_merged": hx(TICK["px_merged"] if px else 0),
                  "f.px_G": V["px_G"] if px else 0, "f.px_rank": V["px_rank"] if px else 0, "f.px_seq": nx["px_seq"] if px else 0,
                  "f.px_bound": min(max((V["px_bound"] + 0xFFFF) >> 16, 1), UINT32_MAX) if px else 0, "f.wq": hx(V["wq"])})
        if tt:
            rd, wr = st["trk_cur"], st["trk_cur"] ^ 1
            nx["tseq"], nx["trk_cur"] = next_seq(st["tseq"]), wr
            path = lambda r: V["trk"] + 8 * 2 * PATH_STRIDE * r
            costs = V["trk"] + 8 * 4 * PATH_STRIDE
            o.update({"trk.cx": hx(V["track"]), "trk.cy": hx(V["track"] + 8 * V["tr_n"]), "trk.tt": hx(V["track"] + 16 * V["tr_n"]),
                      "trk.n": V["tr_n"], "trk.npad": 0, "trk.L": g(V["tr_L"]), "trk.hw": g(V["tr_width"] / 2 - a["margin"]),
                      "trk.weight": g(a["tw"]), "trk.hp_tag": hx(V["hp_tag"]), "trk.path_rd": hx(path(rd)),
                      "trk.path_wr": hx(path(wr)), "trk.valid_rd": hx(V["trk_flags"] + 4 * rd),
                      "trk.valid_wr": hx(V["trk_flags"] + 4 * wr), "trk.cost_wr": hx(costs + 8 * wr), "trk.dbg": hx(costs + 16),
                      "trk.dbg_valid": hx(V["trk_flags"] + 8), "trk.late": hx(V["trk_flags"] + 12), "trk.seq": nx["tseq"],
                      "trk.poll": bound, "trk.path_ok": int(st["trk_path"] != 0 and st["trk_path"] == H), "trk.pad": 0})
        nx["trk_path"] = H if tt else 0                              # track_path_next: a track tick leaves its H
        nx["trk_last_H"] = H if tt else 0
        o.update({f"next.{k}": v for k, v in nx.items()})
        if px:
            box = nx["px_seq"]
        o.update({f"bank.{k}": v for k, v in nx.items() if k != "px_seq"})
        o["box.seq"] = box
        ticks.append({k: (v if isinstance(v, str) else str(v)) for k, v in o.items()})
        st = nx
    return ticks


@pytest.fixture(scope="module")
def prep(harness):
    """prep(env=None, **fields): the harness's ticks, each checked against prep_model field by field."""
    def run(env=None, **fields):
        rows = [ln.split() for ln in harness("prep", *(f"{k}={v}" for k, v in fields.items()), env=env).strip().splitlines()]
        want = prep_model(env or {}, **fields)
        got = [dict() for _ in want]
        for key, val in rows:
            t, _, name = key.partition(".")
            got[int(t[1:])][name] = val
        for t, (g_, w_) in enumerate(zip(got, want)):
            assert set(g_) == set(w_), (t, set(g_) ^ set(w_))
            for k in w_:
                dbl = k.split(".")[-1] in ("lf", "mass", "Ts", "hmin", "vmax", "L", "hw", "weight") or ".cost." in k and \
                    k not in ("la.cost.enforce", "la.cost.pad")
                assert (float(g_[k]) == float(w_[k])) if dbl else (g_[k] == w_[k]), (fields, t, k, g_[k], w_[k])
        return got
    return run


PREP_KINDS = {
    "lookback": dict(la=0, err=1, wmean=1),
    "lookahead": dict(lb=0, cost=1),
    "both_polled": dict(),
    "both_host": dict(host=1, pk=1),
    "raceline": dict(xref_mode=XREF_RACELINE),
    "exchange": dict(px=1),
    "corridor": dict(cor=1, cost=1),
    "track": dict(tt=1, path_H=3),
    "track_no_lookback": dict(tt=1, lb=0, path_H=4),
    "nlp_euler": dict(integrator=EULER_NLP),
}


@pytest.mark.parametrize("kind", sorted(PREP_KINDS))
def test_plan_tick_prepare(prep, kind):
    """Every field of the launch structs and of the next state, for each kind of tick, polled and under
    LLAMPC_NO_POLL; what prepare never reads (pk, cor) changes nothing."""
    kw = PREP_KINDS[kind]
    for env in (None, {"LLAMPC_NO_POLL": "1"}, {"LLAMPC_POLL_BOUND_S": "0.5"}):
        prep(env, **kw)
    if kind == "corridor":
        assert prep(None, **kw) == prep(None, cost=1) == prep(None, cost=1, pk=1)


def test_plan_tick_state_rules(prep):
    """seq advances on polled ticks only; tseq and trk_cur on track ticks only; slot and count with a
    look-back only, count saturating at W; trk_path as track_path_next; the mailbox's seq with px only."""
    nxt = lambda env=None, **kw: {k[5:]: int(v) for k, v in prep(env, **kw)[0].items() if k.startswith("next.")}
    base = dict(count=1, slot=2, W=3, seq=7, tseq=11, trk_cur=0, trk_path=0, trk_last_H=0, px_seq=0)
    assert nxt() == dict(base, count=2, slot=0, seq=8)
    assert nxt({"LLAMPC_NO_POLL": "1"}) == dict(base, count=2, slot=0)
    assert nxt(lb=0) == base and nxt(la=0) == dict(base, count=2, slot=0)
    assert nxt(count=3, slot=1) == dict(base, count=3, slot=2, seq=8)
    assert nxt(count=0, slot=0, W=1) == dict(base, count=1, slot=0, W=1, seq=8)
    assert nxt(px=1) == dict(base, count=2, slot=0, seq=8, px_seq=6)
    assert nxt(px=1, px_seq=0xFFFFFFFF)["px_seq"] == 2
    assert nxt(tt=1, lb=0) == dict(base, tseq=12, trk_cur=1, trk_path=3, trk_last_H=3)
    assert nxt(tt=1, trk_cur=1, tseq=0xFFFFFFFF) == dict(base, count=2, slot=0, seq=8, tseq=2, trk_cur=0, trk_path=3, trk_last_H=3)
    assert nxt(path_H=3, last_H=3) == dict(base, count=2, slot=0, seq=8)          # any other launch clears the path
    # the path is offered only at the tick's own horizon
    ok = lambda **kw: int(prep(None, tt=1, **kw)[0]["trk.path_ok"])
    assert [ok(path_H=3), ok(path_H=4), ok(path_H=0), ok(path_H=3, H=4)] == [1, 0, 0, 0]


def test_plan_tick_chain(prep):
    """Three ticks chained through plan_tick_commit across seq = 0xFFFFFFFF (never 0, the parity alternates);
    the track tick reads one path copy and writes the other, and the two swap on the next tick."""
    ticks = prep(None, tt=1, px=0, ticks=3, seq=0xFFFFFFFE, tseq=0xFFFFFFFE, count=0, slot=0, W=2)
    assert [int(t["f.seq"]) for t in ticks] == [0xFFFFFFFF, 2, 3] == [int(t["bank.seq"]) for t in ticks]
    assert [int(t["trk.seq"]) for t in ticks] == [0xFFFFFFFF, 2, 3]
    assert [(int(t["bank.count"]), int(t["bank.slot"]), int(t["lb.slot"]), int(t["f.full"])) for t in ticks] == \
        [(1, 1, 0, 0), (2, 0, 1, 1), (2, 1, 0, 1)]
    for a, b in zip(ticks, ticks[1:]):
        assert a["trk.path_rd"] != a["trk.path_wr"] and a["trk.valid_rd"] != a["trk.valid_wr"]
        assert (b["trk.path_rd"], b["trk.path_wr"]) == (a["trk.path_wr"], a["trk.path_rd"])
        assert (b["trk.valid_rd"], b["trk.valid_wr"]) == (a["trk.valid_wr"], a["trk.valid_rd"])
        assert a["trk.cost_wr"] != b["trk.cost_wr"] and a["trk.dbg"] == b["trk.dbg"]
    assert [int(t["trk.path_ok"]) for t in ticks] == [0, 1, 1]
    ex = prep(None, px=1, ticks=3, px_seq=0xFFFFFFFE)
    assert [int(t["f.px_seq"]) for t in ex] == [0xFFFFFFFF, 2, 3] == [int(t["box.seq"]) for t in ex]
    plain = prep(None, lb=0, ticks=3)
    assert all(t["bank.seq"] == "7" and t["box.seq"] == "5" and t["bank.tseq"] == "11" for t in plain)


def test_plan_track_layout(harness):
    """d_trk: path copy 0 | path copy 1 | cost 0, cost 1 | the read-back: path | hp [HMAX][6] | theta [HMAX]
    (kernels.hpp PlanTrack's dbg); d_trk_flags: valid 0, valid 1, the read-back's, the late word; d_hp_tag
    [12 HMAX].  The regions are pairwise disjoint and inside their allocations, in that order; the largest
    read-back copies (H = HMAX) end inside the buffer."""
    L = parse_fields(harness("track_layout"))
    assert (L["HMAX"], L["kPlanPathStride"], L["kPlanTrackDbgDoubles"]) == (HMAX, PATH_STRIDE, 2 * PATH_STRIDE + 7 * HMAX)
    assert (L["row"], L["path_doubles"]) == (PATH_STRIDE, 2 * PATH_STRIDE)
    regions = [("path0", L["path0"], L["path_doubles"]), ("path1", L["path1"], L["path_doubles"]), ("cost0", L["cost0"], 1),
               ("cost1", L["cost1"], 1), ("rb_path", L["rb_path"], L["path_doubles"]), ("rb_hp", L["rb_hp"], 6 * HMAX),
               ("rb_theta", L["rb_theta"], HMAX)]
    end = 0
    for name, off, size in regions:                      # in order, touching, none overlapping
        assert off == end, (name, off, end)
        end = off + size
    assert end == L["trk_doubles"] == 4 * PATH_STRIDE + 2 + L["kPlanTrackDbgDoubles"]
    assert L["rb_theta"] + HMAX - L["rb_path"] == L["kPlanTrackDbgDoubles"]
    # the read-back's copies at H = HMAX: rows of H + 1 doubles at a stride of `row`, 6 H and H doubles
    for base in (L["rb_path"], L["path0"], L["path1"]):
        assert base + L["row"] + (HMAX + 1) <= base + L["path_doubles"] <= L["trk_doubles"]
    assert L["rb_hp"] + 6 * HMAX <= L["rb_theta"] and L["rb_theta"] + HMAX <= L["trk_doubles"]
    flags = [L["valid0"], L["valid1"], L["flag_rb_valid"], L["flag_late"]]
    assert sorted(flags) == [0, 1, 2, 3] == list(range(L["flags"])) and flags == [0, 1, 2, 3]
    assert L["hp_tag_words"] == 12 * HMAX


E_ARG, E_STATE = -1, -4
ASYNC = "an async tick is outstanding: call llampc_plan_wait"
NO_TRACK = "no track set: call llampc_bank_set_track first"
REFUSALS = [
    # one bad field at a time: the plan input (the texts: capi.hip's check_plan_in)
    (dict(null_in=1), E_ARG, "plan input is NULL"),
    (dict(K=0), E_ARG, "K=0 outside [1, 32]"), (dict(K=33), E_ARG, "K=33 outside [1, 32]"),
    (dict(no_prev=1), E_ARG, "look-back needs x_prev, u_prev and x_now"),
    (dict(no_now=1), E_ARG, "look-back needs x_prev, u_prev and x_now"),
    (dict(C=0), E_ARG, "C=0 H=3 must be >= 1"), (dict(H=0), E_ARG, "C=2 H=0 must be >= 1"),
    (dict(C=8193, H=8192), E_ARG, "C*H too large"),
    (dict(no_U=1), E_ARG, "look-ahead needs x_now, U, xref and uprev"),
    (dict(no_now=1, lb=0), E_ARG, "look-ahead needs x_now, U, xref and uprev"),
    (dict(integrator=3), E_ARG, "unknown integrator 3"), (dict(integrator=-1), E_ARG, "unknown integrator -1"),
    (dict(xref_mode=2), E_ARG, "unknown xref_mode 2"),
    (dict(xref_mode=XREF_RACELINE), E_STATE, "xref_mode RACELINE needs llampc_bank_set_raceline first"),
    (dict(lb=0, la=0), E_ARG, "nothing to do: look-back and look-ahead both off"),
    (dict(Ts=0), E_ARG, "Ts must be finite > 0"), (dict(Ts="nan"), E_ARG, "Ts must be finite > 0"),
    (dict(Ts="inf"), E_ARG, "Ts must be finite > 0"), (dict(Ts=-0.02), E_ARG, "Ts must be finite > 0"),
    # ... the corridor entries (check_corridor_mode: plan_shape's words; corridor_invalid's)
    (dict(hp=1, la=0), E_ARG, NO["corridor_la"]), (dict(hp=1, integrator=RK6), E_ARG, NO["corridor_rk6"]),
    (dict(hp=1, xref_mode=XREF_RACELINE, raceline=1), E_ARG, NO["corridor_raceline"]),
    (dict(hp=1, weight=-1), E_ARG, "corridor: weight must be finite and >= 0"),
    (dict(hp=1, weight="nan"), E_ARG, "corridor: weight must be finite and >= 0"),
    (dict(hp=1, hp_bad=1), E_ARG, "corridor: a normal component is not finite"),
    # ... the track entries (check_track_tick)
    (dict(tt=1, tr_n=0), E_STATE, NO_TRACK), (dict(tt=1, **{"async": 1}), E_STATE, ASYNC),
    (dict(tt=1, la=0), E_ARG, "the track tick's corridor belongs to the look-ahead: do_lookahead is 0"),
    (dict(tt=1, integrator=RK6), E_ARG, "the track tick has no RK6 rollout"),
    (dict(tt=1, integrator=EULER_NLP), E_ARG,
     "the track tick has no NLP-Euler rollout (llampc_plan_corridor takes host-built rows)"),
    (dict(tt=1, xref_mode=XREF_RACELINE, raceline=1), E_ARG, "the track tick takes the given xref only (not LLAMPC_XREF_RACELINE)"),
    (dict(tt=1, tw=-1), E_ARG, "track tick: weight must be finite and >= 0"),
    (dict(tt=1, tw="inf"), E_ARG, "track tick: weight must be finite and >= 0"),
    (dict(tt=1, margin=1.2), E_ARG, "track tick: margin must be finite and below track_width / 2"),
    (dict(tt=1, margin="nan"), E_ARG, "track tick: margin must be finite and below track_width / 2"),
    (dict(tt=1, H=HMAX + 1), E_ARG, "H=65 above 64 (the path state's horizon)"),
    # pairs: the order within an entry
    (dict(tt=1, tr_n=0, tw=-1), E_STATE, NO_TRACK),                       # no track before a bad weight
    (dict(tt=1, tr_n=0, **{"async": 1}), E_STATE, NO_TRACK),              # ... and before the outstanding tick
    (dict(tt=1, integrator=RK6, **{"async": 1}), E_STATE, ASYNC),         # the outstanding tick before RK6
    (dict(tt=1, integrator=RK6, tw=-1), E_ARG, "the track tick has no RK6 rollout"),
    (dict(tt=1, tw=-1, K=0), E_ARG, "track tick: weight must be finite and >= 0"),
    (dict(tt=1, null_in=1, tw=-1), E_ARG, "track tick: weight must be finite and >= 0"),
    (dict(tt=1, null_in=1), E_ARG, "plan input is NULL"),
    (dict(K=0, Ts=0), E_ARG, "K=0 outside [1, 32]"),                      # a bad K before a bad Ts
    (dict(tt=1, K=0, H=HMAX + 1), E_ARG, "K=0 outside [1, 32]"),          # the plan input before the path's horizon
    (dict(hp=1, integrator=RK6, K=0), E_ARG, NO["corridor_rk6"]),         # the corridor's modes before the plan input
    (dict(hp=1, K=0, weight=-1), E_ARG, "K=0 outside [1, 32]"),           # ... its rows and weight after
    (dict(hp=1, H=0, hp_bad=1), E_ARG, "C=2 H=0 must be >= 1"),
    (dict(**{"async": 1}), 0, ""),                  # every other entry refuses it after the disarm, not here
]


@pytest.mark.parametrize("kw,code,msg", REFUSALS, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_plan_entry_refusals(harness, kw, code, msg):
    """Code and message of plan_entry_refused, one bad field at a time and in pairs that show the order.
    ("n*C overflows" is not here: with n <= 2^31 - 1, llampc_bank_create's bound, and C <= 2^26 no input reaches it.)"""
    out = harness("refuse", *(f"{k}={v}" for k, v in kw.items())).rstrip("\n")
    got_code, _, got_msg = out.partition(" ")
    assert (int(got_code), got_msg) == (code, msg)


def test_plan_entries_accept(harness):
    for kw in (dict(), dict(lb=0), dict(la=0), dict(hp=1), dict(tt=1), dict(tt=1, H=HMAX), dict(xref_mode=XREF_RACELINE, raceline=1),
               dict(hp=1, integrator=EULER_NLP), dict(C=8192, H=8192), dict(tt=1, margin=-3.0), dict(tt=1, tw=0), dict(lb=0, no_prev=1)):
        assert harness("refuse", *(f"{k}={v}" for k, v in kw.items())).strip() == "0", kw


# ---- the controller tick's host path (capi_host.hpp ctl_tick_prepare / ctl_tick_commit, ctl_spec_models, ----
# ---- ctl_gather_split, ctl_cor_layout, the doorbell's words, ctl_arm_fires, the entries' refusals) ----------
# The harness's `ctl_prep` mode runs controller ticks on a fake controller, bank and mailbox (fake_ctl_view:
# fake_bank's addresses and 0x400000 on, never dereferenced; the mus a heap block of exactly rl_M doubles)
# and prints every field of CtlLaunch, CtlCorridor, lpm, lds, the next state and the state after the
# commit; ctl_model restates ctl.hpp's comments on the fields and rt.py's rule for the ticks.
CV = dict(st=0x400000, out=0x401000, host_tag=0x402000, sel_tag=0x403000, slot_tag=0x404000, tickets=0x405000, dbg=0x406000,
          znoise=0x407000, ztag=0x408000, pts=0x409000, prefix=0x409800, np=9, door=0x40A000, door_dev=0x40B000,
          spec_val=0x40C000, spec_idx=0x40D000, spec_tag=0x40E000, spec_res=0x40F000, xref_tag=0x410000, gparams=0x411000,
          px_box=0x412000, px_world=2, px_rank=1, px_bound=10 ** 9, xg_world=3, xg_rank=2, xsend=0x413000, xgath=0x414000,
          track=0x420000, tr_n=4, tr_L=8.0, tr_width=2.4, cor=0x430000, cor_flag=0x440000, hp_tag=0x450000, cor_cost=0x460000,
          mus=(0.5, 1.5), x_t=tuple(0.25 + j for j in range(6)), nominal=tuple(1.5 + j for j in range(6)), sigma=(0.1, 0.05),
          seed=77, v_factor=0.9, mu_init=0.8, S=20, lap_projidx=7)
CTL_DEFAULTS = dict(C=2, H=3, K=2, Ts=0.02, nan_policy=0, q1=0.0, transport="none", n_global=12, cor_w=0.0, cor_margin=0.05,
                    spec_nb=1, spec_cap=32, no_spec=0, no_stage=0, cus=256, share=1, t=0, hseq=40, seq=7, door_ctr=3, hint_p0=5,
                    hint_mu=0.75, cor_prev=0, count=0, slot=0, px_seq=5, kinds="l", reset=-1)
CTL_PATH_STRIDE, CTL_COR_DBG = HMAX + 1, 2 * (HMAX + 1) + 7 * HMAX
REC_WORDS = PLAN_OUT // 4                # kernels.hpp kRecWords: a mailbox slot's words per rank (372)
E_WINDOW = "tick %d: the look-back window is not full after the warm-up (was the bank reset?)"


def a16(x):
    return (x + 15) & ~15


def mu_bracket_model(mus, mu):
    """raceline.hpp mu_bracket (planner.py:48-62): lo, hi, single, wa, wb, den."""
    M = len(mus)
    if mu < mus[0] or mu > mus[-1]:
        i = M - 1 if mu > mus[-1] else 0
        return i, i, 1, 1.0, 0.0, 1.0
    hi = sum(1 for j in range(M - 1) if not mus[j] >= mu)
    lo = M - 1 if hi == 0 else hi - 1
    return lo, hi, 0, mus[hi] - mu, mu - mus[lo], mus[hi] - mus[lo]


def ctl_off_model(H, C, rl_n, nb_lb, K, s4, px_G=0, n_spec=0, extra=0, role_min=0):
    """ctl_lds.hpp ctl_lds_bytes' offset of the completing block's area: the largest of the look-ahead layout
    (+ a corridor tick's extra, or another role's whole request), the exchange's region, lb_final's and the
    speculative look-ahead's, 16-B aligned; the launch asks for 4 KiB more."""
    end = max(a16(ctl_lds_model(H, C, rl_n, s4) + extra), role_min)
    px = SCRATCH + a16(4 * px_G * 4 * (K + 1)) + 16 * px_G * K + 4 * KMAX + 16 if px_G else 0
    spec = 0
    if n_spec:
        o = a16(SCRATCH + 16 * (H + 1))
        o = a16(o + 16 * C * H)
        o = a16(o + 16 * C * H + 16 * C)
        o = a16(o + 16 * C * H) + 8 * 64 + 256
        spec_px = a16(2 * ENT * nb_lb * n_spec) + a16(16 * px_G * n_spec) + 2 * ENT * px_G * n_spec if px_G else 0
        spec = max(o, SCRATCH + max(12 * BLOCK, 2 * ENT * nb_lb * n_spec, spec_px))
    return a16(max(end, px, lb_final_lds(nb_lb, K), spec))


def spec_model(armed=1, no_spec=0, warm=0, full=1, diag=1, mailbox=0, R=1, s4=1, lpm=4, cpl=1, G=2, C=2, H=3, K=2, rl_n=5,
               xg_world=0, px_G=0, nb_lb=1, nb_la=3, spec_nb=1, spec_cap=32, cus=256, share=1, n=5):
    """ctl_spec_models: (n_spec, lds, poll_off); (0, None, None) when none."""
    room = (cus if cus >= 1 else 256) // max(1, share) - (nb_lb + nb_la)
    ns = min(spec_cap, room, n)
    px_fits = not mailbox or (px_G and 4 * (K + 1) + 4 * ns <= REC_WORDS)
    ok = (armed and not no_spec and not warm and full and R == 1 and s4 and lpm == 4 and cpl == 1 and G == C and diag
          and not xg_world and px_fits and ns >= 4 and nb_lb <= spec_nb)
    if not ok:
        return 0, None, None
    off = ctl_off_model(H, C, rl_n, nb_lb, K, True, px_G, ns)
    return (ns, off + 4096, off) if off + 4096 <= 160 * KIB else (0, None, None)


def ctl_model(env, **kw):
    """[one dict per step of `kinds`] of every printed field."""
    a = dict(CTL_DEFAULTS, **kw)
    V, B, hx = CV, VIEW, (lambda p: format(p, "x"))
    C, H, K, Ts, W, n, rl_n = a["C"], a["H"], a["K"], a["Ts"], VIEW["W"], VIEW["n"], VIEW["rl_n"]
    mailbox, gather = a["transport"] == "mailbox", a["transport"] == "gather"
    nan_first = int(a["nan_policy"] == 0)
    c = dict(t=a["t"], hseq=a["hseq"], seq=a["seq"], door_ctr=a["door_ctr"], cor_prev=a["cor_prev"], cor_nslots=0, xg_seq=a["px_seq"])
    bank, box = dict(count=a["count"], slot=a["slot"]), a["px_seq"]
    poll0 = poll_model(n, C, H, max(0.0, float(env.get("LLAMPC_POLL_BOUND_S", 2.0))),
                       max(0.0, float(env.get("LLAMPC_POLL_STEP_NS", 40.0))))[2]
    m, xy = rl_n - 1, B["rl"] + 8 * rl_n
    steps = []
    for s, kind in enumerate(a["kinds"]):
        if s == a["reset"]:
            bank = dict(count=0, slot=0)
        armed, t = kind != "l", c["t"]
        st_px = box if mailbox else c["xg_seq"]
        # rt.py:278-366: the look-back from the second transition on, the nominal model through tick W, the
        # window full once W errors are in, mu-hat used from tick W + 2 on
        do_lb, warm, use_mu = int(t >= 2), int(t <= W), int(t > W + 1)
        count = min(bank["count"] + 1, W) if do_lb else bank["count"]
        full = int(bool(do_lb) and count >= W)
        o = {}
        nx = dict(t=t, hseq=c["hseq"], seq=c["seq"], door_ctr=c["door_ctr"], hint_p0=a["hint_p0"], hint_mu=a["hint_mu"],
                  cor_prev=c["cor_prev"], cor_nslots=c["cor_nslots"], count=bank["count"], slot=bank["slot"], W=W, px_seq=st_px, px=0)

        def finish(rc, why=None):
            o["rc"] = rc
            if why is not None:
                o["why"] = why
            o.update({f"ctl.{k}": v for k, v in c.items()})
            o.update({"bank.count": bank["count"], "bank.slot": bank["slot"], "box.seq": box})
            steps.append(o)

        if not warm and not full:
            finish(E_STATE, E_WINDOW % t)
            continue
        nx.update(t=t + 1, hseq=c["hseq"] + 1, seq=next_seq(c["seq"]))
        if do_lb:
            nx.update(count=count, slot=(bank["slot"] + 1) % W)
        if armed:
            nx["door_ctr"] = 1 if c["door_ctr"] == 0xFFFFFFFF else c["door_ctr"] + 1
            c["door_ctr"] = nx["door_ctr"]                      # ctl_arm stores it before its launch call
        R = lookback_r(n, K)
        corr = a["cor_w"] > 0
        G = group(C)
        lpm = 4 if 4 * G <= BLOCK else 2 if 2 * G <= BLOCK else 1
        mpb, cpl = BLOCK // (G * lpm), cdiv(C, G)
        nb_lb = cdiv(n, BLOCK * R) if do_lb else 1
        nslots = 1 if warm else K + 1
        nb_la = cdiv(nslots, mpb)
        sharded = mailbox or gather
        px_G = (V["px_world"] if mailbox else V["xg_world"]) if sharded and full else 0
        if px_G:
            nx.update(px=1, px_seq=next_seq(st_px))
        if corr:
            s4 = 0
            off = ctl_off_model(H, C, rl_n, nb_lb, K, False, px_G, 0, 48 * H + 16 * (H + 1) + 16, 64 + 24 * V["tr_n"])
        else:
            off = ctl_off_model(H, C, rl_n, nb_lb, K, True, px_G)
            s4 = int(not a["no_stage"] and off + 4096 <= 160 * KIB)
            if not s4:
                off = ctl_off_model(H, C, rl_n, nb_lb, K, False, px_G)
        lds = off + 4096
        n_spec, lds_sp, off_sp = spec_model(armed, a["no_spec"], warm, full, int(a["q1"] == 0.0), int(mailbox), R, s4, lpm, cpl, G, C,
                                            H, K, rl_n, V["xg_world"] if gather else 0, px_G, nb_lb, nb_la, a["spec_nb"],
                                            a["spec_cap"], a["cus"], a["share"], a["n_global"] if mailbox else n)
        if n_spec:
            lds, off = lds_sp, off_sp
        lds = max(lds, ONE_BLOCK_PER_CU)
        poll = poll0
        px_bound = 0
        if px_G:
            px_bound = min(max((V["px_bound"] + 0xFFFF) >> 16, 1), UINT32_MAX) if mailbox else 16
            if mailbox:
                poll = max(poll, px_bound)
        la_params, la_n, la_goff = (V["gparams"], a["n_global"], 0) if sharded else (B["params"], n, B["goff"])
        br = (0, 0, 0, 0.0, 0.0, 0.0) if armed else mu_bracket_model(V["mus"], a["hint_mu"] if use_mu else 1.0)
        L = {"lb.params": hx(B["params"]), "lb.n": n, "lb.goff": B["goff"], "lb.veh.lf": B["lf"], "lb.veh.mass": B["mass"],
             "lb.x_prev": hx(V["st"]), "lb.u_prev": hx(V["st"] + 48), "lb.x_now": "0", "lb.Ts": Ts, "lb.ring": hx(B["ring"]),
             "lb.W": W, "lb.slot": bank["slot"], "lb.full": full, "lb.K": K, "lb.nan_first": nan_first, "lb.R": R, "lb.wm_keep": 0,
             "lb.err_out": "0", "lb.wm_buf": hx(B["wmean"]), "lb.am_val": hx(B["am_val"]), "lb.am_idx": hx(B["am_idx"]),
             "lb.tk_val": hx(B["tk_val"]), "lb.tk_idx": hx(B["tk_idx"]),
             "la.params": hx(la_params), "la.n": la_n, "la.goff": la_goff, "la.veh.lf": B["lf"], "la.veh.mass": B["mass"],
             "la.veh.input_acc": 1, "la.veh.approx": 1, "la.x0": "0", "la.U": "0", "la.xref": "0", "la.uprev": "0", "la.C": C,
             "la.H": H, "la.integrator": RK4, "la.Ts": Ts, "la.cost.umin0": -0.1, "la.cost.umin1": -0.35, "la.cost.umax0": 1.0,
             "la.cost.umax1": 0.35, "la.cost.dmax0": -1.0, "la.cost.dmax1": 2.0 * Ts * (1.0 + 1e-9), "la.cost.enforce": 1,
             "la.cost.pad": 0, "la.cost_out": "0", "la.best_cand": "0", "la.best_cost": "0", "la.pv": "0", "la.pidx": "0",
             "la.pnf": "0", "la.xref_mode": XREF_GIVEN, "la.rl.knots": hx(B["rl"]), "la.rl.xy": hx(xy),
             "la.rl.speed": hx(xy + 8 * 8 * m), "la.rl.mus": hx(xy + 8 * 8 * m + 8 * 4 * m * B["rl_M"]), "la.rl.n": rl_n,
             "la.rl.M": B["rl_M"], "la.rl.wcap": rl_n - 1, "la.rl.hmin": B["rl_hmin"], "la.rl.vmax": B["rl_vmax"],
             "la.xref_pm": "0", "la.la_tag": "0", "la.blk_tag": "0", "la.seq": 0, "la.poll": 0, "la.wq": "0",
             "f.out": hx(V["out"]), "f.tickets": "0", "f.do_lb": do_lb, "f.do_la": 1, "f.full": full, "f.window_count": count,
             "f.K": K, "f.nan_first": nan_first, "f.nb_lb": nb_lb, "f.nb_la": 0, "f.C": C, "f.current_model": 0, "f.n": n,
             "f.goff": B["goff"], "f.params": hx(B["params"]), "f.best_cand": "0", "f.best_cost": "0", "f.am_val": hx(B["am_val"]),
             "f.am_idx": hx(B["am_idx"]), "f.tk_val": hx(B["tk_val"]), "f.tk_idx": hx(B["tk_idx"]), "f.pv": "0", "f.pidx": "0",
             "f.pnf": "0", "f.la_tag": "0", "f.blk_tag": "0", "f.seq": 0, "f.poll": 0, "f.host_tag": "0", "f.host_seq": 0,
             "f.px_box": "0", "f.px_merged": "0", "f.px_G": 0, "f.px_rank": 0, "f.px_seq": 0, "f.px_bound": 0, "f.wq": "0",
             "L.st": hx(V["st"]), "L.out": hx(V["out"]), "L.host_tag": hx(V["host_tag"]), "L.host_seq": nx["hseq"],
             "L.sel_tag": hx(V["sel_tag"]), "L.slot_tag": hx(V["slot_tag"]), "L.tickets": hx(V["tickets"]), "L.dbg": hx(V["dbg"]),
             "L.znoise": hx(V["znoise"]), "L.ztag": hx(V["ztag"]), "L.pts": hx(V["pts"]), "L.prefix": hx(V["prefix"]), "L.tick": t,
             "L.seed": V["seed"], "L.mu_fixed": 1.0, "L.scale_fixed": 1.0, "L.v_factor": V["v_factor"], "L.mu_init": V["mu_init"],
             "L.poll_off": off, "L.seq": nx["seq"], "L.poll": poll, "L.np": V["np"], "L.lap_projidx": V["lap_projidx"],
             "L.do_lb": do_lb, "L.warm": warm, "L.use_mu": use_mu, "L.full": full, "L.nslots": nslots, "L.mpb": mpb, "L.G": G,
             "L.cpl": cpl, "L.S": V["S"], "L.K": K, "L.nb_lb": nb_lb, "L.nb_la": nb_la, "L.s4": s4,
             "L.p0_walk": 0 if armed else a["hint_p0"], "L.br.lo": br[0], "L.br.hi": br[1], "L.br.single": br[2], "L.br.wa": br[3],
             "L.br.wb": br[4], "L.br.den": br[5], "L.sel_goff": 0 if sharded else B["goff"],
             "L.px_box": hx(V["px_box"] if mailbox and px_G else 0), "L.px_G": px_G,
             "L.px_rank": (V["px_rank"] if mailbox else V["xg_rank"]) if px_G else 0, "L.px_seq": nx["px_seq"] if px_G else 0,
             "L.px_bound": px_bound, "L.px_phase": int(gather and bool(px_G)), "L.px_send": hx(V["xsend"] if gather and px_G else 0),
             "L.px_gath": hx(V["xgath"] if gather and px_G else 0), "L.px_spec_off": 4 * (K + 1) if n_spec else 0,
             "L.px_spec_wait": 20000 if n_spec else 0, "L.door": hx(V["door"] if armed else 0), "L.door_dev": hx(V["door_dev"]),
             "L.door_seq": nx["door_ctr"] if armed else 0, "L.door_bound": int(2.0 * 1e8 / 65536.0) + 1 if armed else 0,
             "L.n_spec": n_spec, "L.spec_val": hx(V["spec_val"] if n_spec else 0), "L.spec_idx": hx(V["spec_idx"] if n_spec else 0),
             "L.spec_tag": hx(V["spec_tag"] if n_spec else 0), "L.spec_res": hx(V["spec_res"] if n_spec else 0),
             "L.xref_tag": hx(V["xref_tag"] if n_spec else 0), "lpm": lpm, "lds": lds}
        q = (1.0, a["q1"], 0.0, 4.0)
        for i in range(4):
            L.update({f"la.cost.Q{i}": q[i], f"la.cost.R{i}": 10.0 + i, f"la.cost.P{i}": (20.0 + i) if i in (0, 3) else 0.0})
        for j in range(6):
            L.update({f"L.x_t{j}": 0.0 if armed else V["x_t"][j], f"L.nominal{j}": V["nominal"][j]})
        for j in range(2):
            L.update({f"L.nscale{j}": math.sqrt(3.0) * V["sigma"][j], f"L.rate{j}": (-1.0, 2.0 * Ts)[j],
                      f"L.umin{j}": (-0.1, -0.35)[j], f"L.umax{j}": (1.0, 0.35)[j]})
        o.update(L)
        o["corr"] = int(corr)
        if corr:
            wr = t & 1
            rd = wr ^ 1
            path = lambda r: V["cor"] + 8 * 2 * CTL_PATH_STRIDE * r
            rb = lambda r: V["cor"] + 8 * (4 * CTL_PATH_STRIDE + CTL_COR_DBG * r)
            o.update({"cor.cx": hx(V["track"]), "cor.cy": hx(V["track"] + 8 * V["tr_n"]), "cor.tt": hx(V["track"] + 16 * V["tr_n"]),
                      "cor.n": V["tr_n"], "cor.npad": 0, "cor.L": V["tr_L"], "cor.hw": V["tr_width"] / 2 - a["cor_margin"],
                      "cor.weight": a["cor_w"], "cor.hp_tag": hx(V["hp_tag"]), "cor.path_rd": hx(path(rd)), "cor.path_wr": hx(path(wr)),
                      "cor.valid_rd": hx(V["cor_flag"] + 4 * rd), "cor.valid_wr": hx(V["cor_flag"] + 4 * wr), "cor.dbg": hx(rb(wr)),
                      "cor.dbg_valid": hx(V["cor_flag"] + 4 * (2 + wr)), "cor.path_ok": int(bool(c["cor_prev"])), "cor.pad": 0,
                      "cor.dbg_cost": hx(V["cor_cost"])})
        if gather and px_G:
            # the gather transport's two launches: the look-back blocks alone, then block 0 with the look-ahead blocks
            o.update({f"s1.{k}": v for k, v in dict(L, **{"L.nb_la": 0, "L.n_spec": 0}).items()})
            o.update({f"s2.{k}": v for k, v in dict(L, **{"L.px_phase": 2, "L.nb_lb": 1}).items()})
        nx.update(cor_prev=int(corr), cor_nslots=nslots if corr else 0)
        o.update({f"next.{k}": v for k, v in nx.items()})
        if kind != "f":                  # the commit: everything but the doorbell number
            c.update(t=nx["t"], hseq=nx["hseq"], seq=nx["seq"], cor_prev=nx["cor_prev"], cor_nslots=nx["cor_nslots"])
            bank = dict(count=nx["count"], slot=nx["slot"])
            if nx["px"]:
                if mailbox:
                    box = nx["px_seq"]
                else:
                    c["xg_seq"] = nx["px_seq"]
        finish(0)
    return steps


@pytest.fixture(scope="module")
def ctl_prep(harness):
    """ctl_prep(env=None, **fields): the harness's steps, each checked against ctl_model field by field."""
    def run(env=None, **fields):
        out = harness("ctl_prep", *(f"{k}={v}" for k, v in fields.items()), env=env)
        want = ctl_model(env or {}, **fields)
        got = [dict() for _ in want]
        for ln in out.strip().splitlines():
            key, _, val = ln.partition(" ")
            t, _, name = key.partition(".")
            got[int(t[1:])][name] = val
        for t, (g_, w_) in enumerate(zip(got, want)):
            assert set(g_) == set(w_), (fields, t, sorted(set(g_) ^ set(w_)))
            for k, w in w_.items():
                ok = float(g_[k]) == w if isinstance(w, float) else g_[k] == str(w)
                assert ok, (fields, t, k, g_[k], w)
        return got
    return run


FULL = dict(t=5, count=3, slot=1)        # a tick past the warm-up on a full window: use_mu
CTL_KINDS = {
    "launched": dict(FULL),
    "armed": dict(FULL, kinds="a"),                                    # the speculative look-ahead's five models
    "armed_no_spec": dict(FULL, kinds="a", no_spec=1),
    "armed_off_diagonal": dict(FULL, kinds="a", q1=0.5),
    "warm_first": dict(t=0),
    "warm_lookback": dict(t=2, count=0),
    "unstaged": dict(FULL, no_stage=1),
    "nan_ignore": dict(FULL, nan_policy=1),
    "mailbox_full": dict(FULL, transport="mailbox"),
    "mailbox_full_armed": dict(FULL, transport="mailbox", kinds="a"),
    "mailbox_not_full": dict(t=2, count=0, transport="mailbox"),
    "mailbox_not_full_armed": dict(t=2, count=0, transport="mailbox", kinds="a"),
    "gather_full": dict(FULL, transport="gather"),                     # with both halves of ctl_gather_split
    "gather_not_full": dict(t=3, count=1, transport="gather"),
    "corridor_even": dict(FULL, t=6, cor_w=1e4, cor_prev=1),
    "corridor_odd": dict(FULL, cor_w=1e4, cor_prev=1),
    "corridor_even_first": dict(FULL, t=6, cor_w=1e4),
    "corridor_odd_first": dict(FULL, cor_w=1e4, cor_margin=-0.5),
    "corridor_armed": dict(FULL, cor_w=2.5, cor_prev=1, kinds="a"),
    "corridor_warm": dict(t=1, cor_w=1e4),
}


@pytest.mark.parametrize("kind", sorted(CTL_KINDS))
def test_ctl_tick_prepare(ctl_prep, kind):
    """Every field of CtlLaunch, CtlCorridor, lpm, lds and the next state for each kind of tick, and under
    another poll bound."""
    kw = CTL_KINDS[kind]
    got = ctl_prep(None, **kw)[0]
    ctl_prep({"LLAMPC_POLL_BOUND_S": "0.5"}, **kw)
    assert got["rc"] == "0"
    if kind == "armed":
        assert (got["L.n_spec"], got["L.door_seq"], got["next.door_ctr"]) == ("5", "4", "4")
    if kind in ("armed_no_spec", "armed_off_diagonal", "corridor_armed", "mailbox_not_full_armed"):
        assert got["L.n_spec"] == "0" and got["L.door"] != "0"
    if kind == "mailbox_full_armed":     # the ranks' lists in the slot after the selection record: 12 + 4 x 12 words
        assert (got["L.n_spec"], got["L.px_spec_off"], got["L.px_seq"], got["next.px"]) == ("12", "12", "6", "1")
    if kind == "gather_full":
        assert (got["L.px_phase"], got["s1.L.px_phase"], got["s2.L.px_phase"]) == ("1", "1", "2")
        assert (got["s1.L.nb_la"], got["s1.L.nb_lb"], got["s2.L.nb_la"], got["s2.L.nb_lb"]) == ("0", got["L.nb_lb"], got["L.nb_la"], "1")
    if kind.startswith("corridor"):
        assert got["L.s4"] == "0" and got["cor.path_rd"] != got["cor.path_wr"]
        assert got["cor.path_ok"] == str(kw.get("cor_prev", 0)) and got["next.cor_prev"] == "1"


def rt_rule(t, W):
    """rt.py:278-366 per tick t on a window of W: (do_lb, warm, full, use_mu, window_count, slot after the tick)."""
    errors = max(0, t - 1)               # the look-back runs from tick 2 on, one error per tick
    return int(t >= 2), int(t <= W), int(errors >= W), int(t > W + 1), min(errors, W), errors % W


def test_ctl_tick_chain(ctl_prep):
    """t = 0 .. W + 3 chained through ctl_tick_commit, launched and armed: warm, look-back, full and use_mu ticks
    by rt.py's rule; the sequences across 0xFFFFFFFF; the transport's sequence on full ticks only."""
    W = VIEW["W"]
    for kinds in ("l" * (W + 4), "laalala"):
        for tr in ("none", "mailbox", "gather"):
            if tr == "gather" and "a" in kinds:
                continue                 # no armed launches over a gather transport (ctl_arm)
            ticks = ctl_prep(None, kinds=kinds, transport=tr, seq=0xFFFFFFFD, door_ctr=0xFFFFFFFE, px_seq=0xFFFFFFFE)
            px_seq, doors = 0xFFFFFFFE, []
            for t, o in enumerate(ticks):
                do_lb, warm, full, use_mu, wc, slot = rt_rule(t, W)
                assert [int(o[k]) for k in ("L.do_lb", "L.warm", "L.full", "L.use_mu", "f.window_count", "bank.count", "bank.slot")] == \
                    [do_lb, warm, full, use_mu, wc, wc, slot], (kinds, tr, t)
                assert (int(o["L.tick"]), int(o["ctl.t"]), int(o["L.host_seq"])) == (t, t + 1, 41 + t)
                assert int(o["L.nslots"]) == (1 if warm else 3) and int(o["lb.full"]) == int(o["f.full"]) == full
                if tr != "none" and full:
                    px_seq = next_seq(px_seq)
                assert int(o["box.seq" if tr == "mailbox" else "ctl.xg_seq"]) == px_seq, (kinds, tr, t)
                assert int(o["L.px_G"]) == (0 if tr == "none" or not full else 2 if tr == "mailbox" else 3)
                if kinds[t] == "a":
                    doors.append(int(o["L.door_seq"]))
            assert [int(o["L.seq"]) for o in ticks] == [0xFFFFFFFE, 0xFFFFFFFF, 2, 3, 4, 5, 6]      # never 0, the next value 2
            assert doors == [0xFFFFFFFF, 1, 2, 3][:len(doors)]                                     # never 0, the next value 1
            assert int(ticks[-1]["ctl.door_ctr"]) == (doors[-1] if doors else 0xFFFFFFFE)
            assert px_seq == (0xFFFFFFFE if tr == "none" else 3)                                    # 0xFFFFFFFF, 2, 3: three full ticks


def test_ctl_tick_window_refused(ctl_prep):
    """Past the warm-up a window that is not full is refused (LLAMPC_E_STATE) and nothing advances — not even
    an armed prepare's doorbell number."""
    for kind in "la":
        ticks = ctl_prep(None, kinds="lllll" + kind + kind, reset=5, door_ctr=9)
        for o in ticks[5:]:
            assert (int(o["rc"]), o["why"]) == (E_STATE, E_WINDOW % 5)
            assert (o["ctl.t"], o["ctl.hseq"], o["ctl.seq"], o["ctl.door_ctr"], o["bank.count"]) == ("5", "45", "12", "9", "0")
    assert ctl_prep(None, t=4, count=1)[0]["rc"] == str(E_STATE)
    assert ctl_prep(None, t=3, count=1)[0]["rc"] == "0"                  # the last warm tick may still be filling


def test_ctl_armed_launch_failed(ctl_prep):
    """An armed prepare whose launch call failed spends its doorbell number and nothing else; the next armed
    prepare of the same tick takes the number after."""
    a, b, c = ctl_prep(None, kinds="faa", transport="mailbox", **FULL)
    assert (a["L.door_seq"], b["L.door_seq"], c["L.door_seq"]) == ("4", "5", "6")
    assert (a["ctl.t"], a["ctl.hseq"], a["ctl.seq"], a["ctl.door_ctr"], a["bank.count"], a["bank.slot"], a["box.seq"]) == \
        ("5", "40", "7", "4", "3", "1", "5")
    same = lambda x, y: {k: v for k, v in x.items() if k.startswith(("L.", "lb.", "la.", "f.")) and x[k] != y[k]}
    assert set(same(a, b)) == {"L.door_seq"}                             # the relaunch is the same tick
    assert (b["ctl.t"], b["ctl.hseq"], b["ctl.seq"], b["box.seq"], b["bank.slot"]) == ("6", "41", "8", "6", "2")


SPEC_ELIGIBLE = dict(armed=1, no_spec=0, warm=0, full=1, diag=1, mailbox=0, R=1, s4=1, lpm=4, cpl=1, G=2, C=2, xg_world=0, nb_lb=1,
                     spec_nb=1, n=5)


@pytest.fixture(scope="module")
def ctl_spec(harness):
    def run(**kw):
        ns, lds, off = (int(x) for x in harness("ctl_spec", *(f"{k}={v}" for k, v in kw.items())).split())
        want = spec_model(**kw)
        assert (ns, lds, off) == (want[0], want[1] if want[0] else -1, want[2] if want[0] else -1), kw
        return ns
    return run


def test_ctl_spec_models(ctl_spec):
    """From an eligible tick every term flipped alone gives none; the room is cus / share less the tick's own
    blocks; spec_cap, the models and the record's room with a mailbox bound it; fewer than four: none."""
    assert ctl_spec(**SPEC_ELIGIBLE) == 5
    for flip in (dict(armed=0), dict(no_spec=1), dict(warm=1), dict(full=0), dict(R=2), dict(s4=0), dict(lpm=2), dict(cpl=2),
                 dict(G=4), dict(diag=0), dict(xg_world=2), dict(mailbox=1), dict(n=3), dict(nb_lb=2)):
        assert ctl_spec(**dict(SPEC_ELIGIBLE, **flip)) == 0, flip
    assert ctl_spec(**dict(SPEC_ELIGIBLE, mailbox=1, px_G=2, n=12)) == 12           # 12 + 4 x 12 words of 372
    assert ctl_spec(**dict(SPEC_ELIGIBLE, mailbox=1, px_G=2, K=32, n=100, spec_cap=64)) == 0     # 132 + 256 > 372: not cut, none
    assert ctl_spec(**dict(SPEC_ELIGIBLE, mailbox=1, px_G=2, K=32, n=100, spec_cap=60)) == 60    # 132 + 240 = 372
    assert ctl_spec(**dict(SPEC_ELIGIBLE, nb_lb=2, spec_nb=2)) == 5
    big = dict(SPEC_ELIGIBLE, n=10 ** 6, spec_cap=64, nb_lb=40, spec_nb=40, nb_la=11)
    assert ctl_spec(**dict(big, cus=256, share=1)) == 64                              # room 205: the cap
    assert ctl_spec(**dict(big, cus=256, share=2)) == 64                              # room 77
    assert ctl_spec(**dict(big, cus=256, share=2, nb_la=50)) == 38                    # room 128 - 90 = 38, below the cap
    assert ctl_spec(**dict(big, cus=256, share=4, nb_la=11)) == 13                    # 64 - 51
    assert ctl_spec(**dict(big, cus=256, share=4, nb_la=21)) == 0                     # room 3
    assert ctl_spec(**dict(big, cus=0, share=2, nb_la=50)) == 38                      # an unknown CU count reads as 256
    assert ctl_spec(**dict(big, cus=104, share=0)) == 53                              # share below 1 reads as 1
    assert ctl_spec(**dict(big, spec_cap=32)) == 32 and ctl_spec(**dict(big, spec_cap=3)) == 0
    assert ctl_spec(**dict(SPEC_ELIGIBLE, n=4)) == 4 and ctl_spec(**dict(SPEC_ELIGIBLE, n=3)) == 0
    # the spec layout's LDS: three [C][H] arrays of 16 B — 162 KiB at C H = 64 x 54, above the CU's 160
    assert 3 * 16 * 64 * 53 <= 160 * KIB < 3 * 16 * 64 * 54
    assert ctl_spec(**dict(SPEC_ELIGIBLE, G=64, C=64, H=54, rl_n=700)) == 0
    assert ctl_spec(**dict(SPEC_ELIGIBLE, G=64, C=64, H=40, rl_n=700)) == 5


def test_ctl_cor_layout(harness):
    """d_cor: path copy 0 | path copy 1 | read-back copy 0 | read-back copy 1, a read-back copy being path rows |
    hp [HMAX][6] | theta [HMAX] (ctl.hpp CtlCorridor's dbg); d_cor_flag: valid 0, valid 1, the read-backs' two;
    d_hp_tag [12 HMAX].  In order, touching, inside their allocations; the inner offsets are the device's."""
    L = parse_fields(harness("ctl_cor_layout"))
    assert (L["HMAX"], L["kCtlPathStride"], L["kCtlCorDbgDoubles"]) == (HMAX, CTL_PATH_STRIDE, CTL_COR_DBG)
    assert (L["row"], L["path_doubles"], L["rb_doubles"]) == (CTL_PATH_STRIDE, 2 * CTL_PATH_STRIDE, CTL_COR_DBG)
    end = 0
    for name, size in (("path0", L["path_doubles"]), ("path1", L["path_doubles"]), ("rb0", L["rb_doubles"]), ("rb1", L["rb_doubles"])):
        assert L[name] == end, (name, L[name], end)
        end += size
    assert end == L["cor_doubles"] == 4 * CTL_PATH_STRIDE + 2 * CTL_COR_DBG
    # inside a read-back copy: the device writes P at 0 (rows kCtlPathStride apart), hp at 2 kCtlPathStride, theta 6 HMAX on
    assert (L["rb_hp"], L["rb_theta"]) == (2 * CTL_PATH_STRIDE, 2 * CTL_PATH_STRIDE + 6 * HMAX)
    assert L["row"] + HMAX + 1 <= L["rb_hp"] and L["rb_hp"] + 6 * HMAX <= L["rb_theta"] and L["rb_theta"] + HMAX == L["rb_doubles"]
    assert [L["valid0"], L["valid1"], L["rb_valid0"], L["rb_valid1"]] == [0, 1, 2, 3] == list(range(L["flags"]))
    assert L["hp_tag_words"] == 12 * HMAX


def test_ctl_door_words(harness):
    """Twelve data words tag | high half, tag | low half of each x_t[j] (a NaN's payload and -0.0's sign kept),
    then tag | fire; the cancel word; the fire rule one condition at a time."""
    x = [1.5, -0.0, float.fromhex("0x1.fffffffffffffp+1023"), 5e-324, -2.75, 0.0]
    bits = [struct.unpack("<Q", struct.pack("<d", v))[0] for v in x]
    bits[3] = 0x7FF80000DEADBEEF         # a NaN with a payload
    for seq in (1, 0x12345678, 0xFFFFFFFF):
        out = harness("ctl_door", seq, *(hex(b) for b in bits)).split()
        words, cancel, consts = [int(w, 16) for w in out[:13]], int(out[13], 16), out[14:]
        fire_c, cancel_c = int(consts[0]), int(consts[1])
        assert (fire_c, cancel_c, float(consts[2]), float(consts[3])) == (1, 2, 0.5, 2.0)
        tag = seq << 32
        want = [tag | h for b in bits for h in (b >> 32, b & 0xFFFFFFFF)] + [tag | fire_c]
        assert words == want and cancel == tag | cancel_c
    assert bits[1] == 1 << 63
    fires = lambda age=0.1, arm_t=4, t=4, px_G=0, mb=0, arm_px=0, mb_seq=0: int(harness("ctl_fires", age, arm_t, t, px_G, mb, arm_px, mb_seq))
    assert fires() == 1
    assert fires(age=0.499) == 1 and fires(age=0.5) == 0 and fires(age=3.0) == 0        # fresh: younger than kArmFreshS
    assert fires(arm_t=3) == 0 and fires(arm_t=5) == 0                                  # armed for another tick
    assert fires(px_G=2, mb=1, arm_px=6, mb_seq=5) == 1                                 # the mailbox's next number
    assert fires(px_G=2, mb=1, arm_px=6, mb_seq=6) == 0 and fires(px_G=2, mb=1, arm_px=6, mb_seq=4) == 0
    assert fires(px_G=2, mb=1, arm_px=2, mb_seq=0xFFFFFFFF) == 1                        # across the wrap
    assert fires(px_G=0, mb=1, arm_px=0, mb_seq=9) == 1                                 # no exchange on the armed tick
    assert fires(px_G=2, mb=0, arm_px=6, mb_seq=9) == 1                                 # no mailbox


LDS_CREATE = "controller tick needs %d B of LDS (> 160 KiB): C*H=%d too large for this track"
VARIANT = "n=%d C=%d (1..65536) H=%d (1..64) K=%d (1..32) rl_n=%d"
CTL_REFUSALS = [
    # llampc_ctl_create
    ("create", dict(out_null=1), E_ARG, "out is NULL"), ("create", dict(arg_null=1), E_ARG, "NULL argument"),
    ("create", dict(null_cfg=1), E_ARG, "NULL argument"),
    ("create", dict(C=0), E_ARG, "C=0 H=3 (1..64) K=2 (1..32)"), ("create", dict(H=0), E_ARG, "C=2 H=0 (1..64) K=2 (1..32)"),
    ("create", dict(H=65), E_ARG, "C=2 H=65 (1..64) K=2 (1..32)"), ("create", dict(K=0), E_ARG, "C=2 H=3 (1..64) K=0 (1..32)"),
    ("create", dict(K=33), E_ARG, "C=2 H=3 (1..64) K=33 (1..32)"),
    ("create", dict(S=0), E_ARG, "S=0 outside [1, 64]"), ("create", dict(S=65), E_ARG, "S=65 outside [1, 64]"),
    ("create", dict(Ts=0), E_ARG, "Ts must be finite > 0"), ("create", dict(Ts="nan"), E_ARG, "Ts must be finite > 0"),
    ("create", dict(Ts="inf"), E_ARG, "Ts must be finite > 0"), ("create", dict(np=1), E_ARG, "np=1 < 2"),
    ("create", dict(nan_policy=2), E_ARG, "nan_policy"),
    ("create", dict(raceline=0), E_STATE, "the controller needs the bank's raceline (llampc_bank_set_raceline)"),
    ("create", dict(C=300, H=40, rl_n=700), E_ARG, LDS_CREATE % (ctl_off_model(40, 300, 700, 1, 2, False) + 4096, 12000)),
    ("create", dict(out_null=1, arg_null=1), E_ARG, "out is NULL"), ("create", dict(arg_null=1, C=0), E_ARG, "NULL argument"),
    ("create", dict(C=0, S=0), E_ARG, "C=0 H=3 (1..64) K=2 (1..32)"), ("create", dict(S=0, Ts=0), E_ARG, "S=0 outside [1, 64]"),
    ("create", dict(Ts=0, np=1), E_ARG, "Ts must be finite > 0"), ("create", dict(np=1, nan_policy=2), E_ARG, "np=1 < 2"),
    ("create", dict(nan_policy=2, raceline=0), E_ARG, "nan_policy"),
    ("create", dict(raceline=0, C=300, H=40, rl_n=700), E_STATE, "the controller needs the bank's raceline (llampc_bank_set_raceline)"),
    ("create", dict(), 0, ""), ("create", dict(C=64, H=40, K=32, S=64, np=2, nan_policy=1, rl_n=700), 0, ""),
    # llampc_ctl_set_corridor
    ("corridor", dict(pending=1), E_STATE, "a controller tick is outstanding"),
    ("corridor", dict(tr_n=0), E_STATE, "no track set: call llampc_ctl_set_track first"),
    ("corridor", dict(sharded=1), E_STATE, "a sharded controller has no corridor ticks"),
    ("corridor", dict(weight=-1), E_ARG, "weight must be finite and >= 0"), ("corridor", dict(weight="nan"), E_ARG, "weight must be finite and >= 0"),
    ("corridor", dict(weight="inf"), E_ARG, "weight must be finite and >= 0"),
    ("corridor", dict(margin=1.2), E_ARG, "margin 1.2 leaves no corridor (track width 2.4)"),
    ("corridor", dict(margin="nan"), E_ARG, "margin nan leaves no corridor (track width 2.4)"),
    ("corridor", dict(C=300, H=40, rl_n=700), E_ARG, "a corridor tick needs %d B of LDS (> 160 KiB)" %
     (ctl_off_model(40, 300, 700, 1, 2, False, 0, 0, 48 * 40 + 16 * 41 + 16, 64 + 24 * 4) + 4096)),
    ("corridor", dict(pending=1, tr_n=0), E_STATE, "a controller tick is outstanding"),
    ("corridor", dict(tr_n=0, sharded=1), E_STATE, "no track set: call llampc_ctl_set_track first"),
    ("corridor", dict(sharded=1, weight=-1), E_STATE, "a sharded controller has no corridor ticks"),
    ("corridor", dict(weight=-1, margin=1.2), E_ARG, "weight must be finite and >= 0"),
    ("corridor", dict(margin=1.2, C=300, H=40, rl_n=700), E_ARG, "margin 1.2 leaves no corridor (track width 2.4)"),
    ("corridor", dict(weight=0, C=300, H=40, rl_n=700), 0, ""),                    # off: no shape to refuse
    ("corridor", dict(), 0, ""), ("corridor", dict(margin=-3.0), 0, ""), ("corridor", dict(weight=0), 0, ""),
    # llampc_ctl_variant and llampc_ctl_variant_corridor
    ("variant", dict(out_null=1), E_ARG, "NULL argument"), ("variant", dict(out_null=1, track_n=4), E_ARG, "NULL argument"),
    ("variant", dict(n=0), E_ARG, VARIANT % (0, 2, 3, 2, 5)), ("variant", dict(C=0), E_ARG, VARIANT % (5, 0, 3, 2, 5)),
    ("variant", dict(C=65537), E_ARG, VARIANT % (5, 65537, 3, 2, 5)), ("variant", dict(H=65), E_ARG, VARIANT % (5, 2, 65, 2, 5)),
    ("variant", dict(K=33), E_ARG, VARIANT % (5, 2, 3, 33, 5)), ("variant", dict(rl_n=1), E_ARG, VARIANT % (5, 2, 3, 2, 1)),
    ("variant", dict(C=65537, track_n=4), E_ARG, VARIANT % (5, 65537, 3, 2, 5) + " track_n=4 (2..4096)"),
    ("variant", dict(track_n=1), E_ARG, VARIANT % (5, 2, 3, 2, 5) + " track_n=1 (2..4096)"),
    ("variant", dict(track_n=4097), E_ARG, VARIANT % (5, 2, 3, 2, 5) + " track_n=4097 (2..4096)"),
    ("variant", dict(C=300, H=40, rl_n=700), E_ARG, LDS_CREATE % (ctl_off_model(40, 300, 700, 1, 2, False) + 4096, 12000)),
    ("variant", dict(C=300, H=40, rl_n=700, track_n=4), E_ARG, "a corridor tick needs %d B of LDS (> 160 KiB)" %
     (ctl_off_model(40, 300, 700, 1, 2, False, 0, 0, 48 * 40 + 16 * 41 + 16, 64 + 24 * 4) + 4096)),
    ("variant", dict(out_null=1, n=0), E_ARG, "NULL argument"), ("variant", dict(n=0, C=300, H=40, rl_n=700), E_ARG, VARIANT % (0, 300, 40, 2, 700)),
    ("variant", dict(C=65536, H=1, rl_n=2), E_ARG, LDS_CREATE % (ctl_off_model(1, 65536, 2, 1, 2, False) + 4096, 65536)),
    ("variant", dict(), 0, "lpm=4 nb_cor=0"), ("variant", dict(track_n=4), 0, "lpm=4 nb_cor=3"), ("variant", dict(track_n=4096, C=130), 0, "lpm=1 nb_cor=3"),
]


@pytest.mark.parametrize("entry,kw,code,msg", CTL_REFUSALS,
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else v if isinstance(v, str) and " " not in v else None)
def test_ctl_entry_refusals(harness, entry, kw, code, msg):
    """Code and message of ctl_create_refused, ctl_corridor_refused and ctl_variant_refused (one
    kCtlVariantCMax), one bad field at a time and in pairs that show each entry's order."""
    out = harness("ctl_refuse", entry, *(f"{k}={v}" for k, v in kw.items())).rstrip("\n")
    got_code, _, got_msg = out.partition(" ")
    assert (int(got_code), got_msg) == (code, msg)

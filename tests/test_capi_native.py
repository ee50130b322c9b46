"""csrc/capi_host.hpp (the C ABI's pure host helpers: tick numbers, poll bounds, the input
pack, the window unroll, the raceline view, the launch fields that come from the bank, the plan
tick's prepare / commit, its track state's layout, its entries' refusals and the controller launch's
shape) and csrc/launch_shape.hpp (the plan launch's shape) compiled for the
host with AddressSanitizer and UBSan and run on the CPU.  The harness (tests/native/capi_host.cpp)
prints values; what they must be is worked out here."""
import os
import shutil
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

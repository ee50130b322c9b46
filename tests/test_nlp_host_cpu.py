"""The NLP solve's pure host section (csrc/capi_host.hpp: nlp_inline_pack, nlp_result_unpack /
nlp_batch_unpack, nlp_launch_args, nlp_built_corridor, the margin / path / cfg refusals, nlp_ltraj_flags)
without a device: compiled into a stand-alone program (tests/native/nlp_host.cpp) with AddressSanitizer
and UBSan and run on the CPU.  Every buffer there is a heap block of exactly its size, pre-filled with a
sentinel NaN; what the program prints (64-bit words in hex) must equal what is worked out here from what
llampc_nlp_solve and llampc_nlp_batch_solve have always assigned."""
import os
import shutil
import struct
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HMAX = 64
SENTINEL = 0xFFF8DEADBEEF0000
OK, NO_FINITE, NO_TAG = 0, 1, 2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("nlp_host") / "nlp_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer",
           f"-I{os.path.join(REPO, 'lla-mpc_amd', 'csrc')}", f"-I{os.path.join(REPO, 'include')}",
           os.path.join(REPO, "tests", "native", "nlp_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)

    def run(*args):
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([out, *map(str, args)], capture_output=True, text=True, env=e)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return r.stdout
    return run


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def val(field, i):
    return bits(100.0 * field + i + 0.25)


def words(out):
    """{name: [words]} of the program's hex lines; other lines as {first word: rest}."""
    d = {}
    for ln in out.splitlines():
        name, _, rest = ln.partition(" ")
        try:
            d[name] = [int(w, 16) for w in rest.split()]
        except ValueError:
            d[name] = rest
    return d


@pytest.mark.parametrize("H", [1, 3, HMAX])
@pytest.mark.parametrize("with_base", [0, 1])
def test_inline_pack(harness, H, with_base):
    """x0 | xref [2][H+1] | the first mean [H][2] (base, or uprev held), every double read back; the tail
    of the NlpInline past 6 + 2 (H + 1) + 2 H is not written."""
    pk = words(harness("pack", H, with_base))["pk"]
    assert len(pk) == 6 + 2 * (HMAX + 1) + 2 * HMAX
    want = [val(0, i) for i in range(6)] + [val(1, i) for i in range(2 * (H + 1))]
    want += [val(3, i) if with_base else val(2, i % 2) for i in range(2 * H)]
    assert len(want) == 6 + 2 * (H + 1) + 2 * H
    assert pk[:len(want)] == want
    assert pk[len(want):] == [SENTINEL] * (len(pk) - len(want))


def result_words(H):
    """best_u [HMAX][2] rows 0..H-1 and traj [HMAX+1][6] rows 0..H of the synthetic NlpResult: contiguous."""
    return [val(4, i) for i in range(2 * H)], val(6, 0), [val(5, i) for i in range(6 * (H + 1))]


@pytest.mark.parametrize("H", [1, 3, HMAX])
@pytest.mark.parametrize("best_it,status", [(0, OK), (5, OK), (-1, NO_FINITE)])
@pytest.mark.parametrize("fval_null,xmpc_null", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_single_unpack(harness, H, best_it, status, fval_null, xmpc_null):
    """llampc_nlp_solve copies umpc, fval and xmpc whatever best_it says (the entry then reports a missing
    finite objective); a null fval / xmpc is not written."""
    o = words(harness("unpack", "single", 1, best_it, H, fval_null, xmpc_null))
    u, j, x = result_words(H)
    assert o["status"] == [status]
    assert o["umpc"] == u
    assert o["fval"] == ([SENTINEL] if fval_null else [j])
    assert o["xmpc"] == ([SENTINEL] * len(x) if xmpc_null else x)


@pytest.mark.parametrize("H", [1, 3, HMAX])
@pytest.mark.parametrize("arrived,best_it,status", [(1, 0, OK), (1, 7, OK), (1, -1, NO_FINITE), (0, 3, NO_TAG), (0, -1, NO_TAG)])
def test_batch_unpack(harness, H, arrived, best_it, status):
    """A solved problem as the single solver's; else umpc +0.0 and fval +inf bitwise, xmpc the trajectory
    if the tag arrived and +0.0 if it did not."""
    o = words(harness("unpack", "batch", arrived, best_it, H, 0, 0))
    u, j, x = result_words(H)
    assert o["status"] == [status]
    ok = status == OK
    assert o["umpc"] == (u if ok else [0] * len(u))
    assert o["fval"] == [j if ok else bits(float("inf"))]
    assert o["xmpc"] == (x if arrived else [0] * len(x))


@pytest.mark.parametrize("calls", [0, 1, 41, 2 ** 40])
@pytest.mark.parametrize("corridor", [0, 1])
@pytest.mark.parametrize("ltraj", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("rounds", [1, 8])
def test_launch_args(harness, calls, corridor, ltraj, rounds):
    """Every field nlp_solve and nlp_batch_run assigned by hand: the buffers, host_seq = calls + 1, call =
    calls, ltraj by corridor, it = 0, rounds (1: the single solver's launch per round; iters: every round in
    one launch) — and no other field of the launch."""
    first, rest = harness("launch", calls, corridor, ltraj[0], ltraj[1], rounds).splitlines()
    got = dict(kv.split("=") for kv in first.split())
    assert got == {"st": "0x1000", "list_tag": "0x2000", "cand": "0x3000", "ms_tag": "0x4000", "res": "0x5000",
                   "host_tag": "0x6000", "host_seq": str(calls + 1), "call": str(calls),
                   "ltraj": str(ltraj[1] if corridor else ltraj[0]), "it": "0", "rounds": str(rounds)}
    assert rest == "rest 0"


def test_built_corridor(harness):
    """Copied out of the mapped buffer to hp_out before the check; the slack only of a valid corridor, 0 for
    a problem that did not solve."""
    H = 3
    rows = []
    for k in range(H):
        rows += [bits(v) for v in (1.0, 0.0, 0.5 + k, 0.0, -1.0, float("inf"))]
    o = words(harness("built", H, 2.0, 1, -1))
    assert o["why"] == "ok" and o["hp_out"] == rows and o["slack"] == o["want"] and o["want"] != [0]
    o = words(harness("built", H, 2.0, 0, -1))
    assert o["why"] == "ok" and o["hp_out"] == rows and o["slack"] == [0]
    o = words(harness("built", H, 2.0, 1, 1))
    assert o["why"] == "a normal component is not finite" and o["slack"] == [SENTINEL]
    assert o["hp_out"][:6] == rows[:6] and o["hp_out"][7:] == rows[7:] and o["hp_out"][6] != rows[6]
    o = words(harness("built", H, -1.0, 1, -1))
    assert o["why"] == "weight must be finite and >= 0" and o["slack"] == [SENTINEL]


@pytest.mark.parametrize("margin,width,msg", [
    (0.0, 2.4, "ok"), (1.19, 2.4, "ok"), (-3.0, 2.4, "ok"),                       # a negative margin widens
    (1.2, 2.4, "margin 1.2 leaves no corridor (track width 2.4)"),                 # margin = width / 2
    (5, 2.4, "margin 5 leaves no corridor (track width 2.4)"),
    ("nan", 2.4, "margin nan leaves no corridor (track width 2.4)"),
    ("inf", 2.4, "margin inf leaves no corridor (track width 2.4)"),
    ("-inf", 2.4, "margin -inf leaves no corridor (track width 2.4)"),
    (0.185, 0.37, "margin 0.185 leaves no corridor (track width 0.37)")])
def test_margin_refusal(harness, margin, width, msg):
    assert harness("margin", margin, width).rstrip("\n") == msg


def test_path_refusals(harness):
    """The single entries' message names the entry, the batch's the problem too; the first bad entry wins."""
    H = 3
    assert harness("path", H, -1, 0).strip() == "ok"
    for bad, v in ((0, "nan"), (3, "inf"), (2 * (H + 1) - 1, "-inf")):
        assert harness("path", H, bad, v).strip() == f"path: entry {bad} is not finite"
    assert harness("bpath", 2, H, 0, -1, 0).strip() == "ok"
    for q, bad, v in ((0, 0, "nan"), (1, 5, "inf"), (1, 2 * (H + 1) - 1, "nan")):
        assert harness("bpath", 2, H, q, bad, v).strip() == f"problem {q}: path entry {bad} is not finite"
    assert harness("path", HMAX, 2 * HMAX + 1, "nan").strip() == f"path: entry {2 * HMAX + 1} is not finite"


LDS_MAX = 160 * 1024


@pytest.mark.parametrize("cfg,msg", [
    ((3, 64, 4, 2, 0.02, LDS_MAX), "ok"),
    ((0, 64, 4, 2, 0.02, 0), "H=0 outside [1, 64]"), ((65, 64, 4, 2, 0.02, 0), "H=65 outside [1, 64]"),
    ((3, 32, 4, 2, 0.02, 0), "samples=32: a power of two in [64, 4096]"),
    ((3, 96, 4, 2, 0.02, 0), "samples=96: a power of two in [64, 4096]"),
    ((3, 8192, 4, 2, 0.02, 0), "samples=8192: a power of two in [64, 4096]"),
    ((3, 64, 0, 2, 0.02, 0), "elite=0 (1..64, <= samples) iters=2 (1..1024)"),
    ((3, 128, 65, 2, 0.02, 0), "elite=65 (1..64, <= samples) iters=2 (1..1024)"),
    ((3, 64, 4, 0, 0.02, 0), "elite=4 (1..64, <= samples) iters=0 (1..1024)"),
    ((3, 64, 4, 1025, 0.02, 0), "elite=4 (1..64, <= samples) iters=1025 (1..1024)"),
    ((3, 64, 4, 2, 0.0, 0), "Ts must be finite > 0"), ((3, 64, 4, 2, "nan", 0), "Ts must be finite > 0"),
    ((3, 64, 4, 2, "inf", 0), "Ts must be finite > 0"),
    ((3, 64, 4, 2, 0.02, LDS_MAX + 1), "H x elite too large for LDS"),
    # the order: the first failing check of llampc_nlp_create's
    ((0, 32, 0, 0, 0.0, LDS_MAX + 1), "H=0 outside [1, 64]"),
    ((3, 32, 0, 0, 0.0, LDS_MAX + 1), "samples=32: a power of two in [64, 4096]"),
    ((3, 64, 0, 0, 0.0, LDS_MAX + 1), "elite=0 (1..64, <= samples) iters=0 (1..1024)"),
    ((3, 64, 4, 2, 0.0, LDS_MAX + 1), "Ts must be finite > 0")])
def test_cfg_refusals(harness, cfg, msg):
    assert harness("cfg", *cfg).splitlines()[0] == msg


def test_corridor_lds_refusal(harness):
    """The corridor solve's own bound: the search's LDS and the half-planes' 48 H bytes."""
    H = 3
    assert harness("cfg", H, 64, 4, 2, 0.02, LDS_MAX - 48 * H).splitlines() == ["ok", "ok"]
    assert harness("cfg", H, 64, 4, 2, 0.02, LDS_MAX - 48 * H + 1).splitlines() == ["ok", "H x elite too large for LDS with a corridor"]


@pytest.mark.parametrize("plain", [0, 1])
@pytest.mark.parametrize("cor", [0, 1])
@pytest.mark.parametrize("rerun", [0, 1])
def test_ltraj_flags(harness, plain, cor, rerun):
    assert harness("ltraj", plain, cor, rerun).split() == [str(int(plain and not rerun)), str(int(cor and not rerun))]

"""The fused control step's pure helpers (csrc/ctl_solve.hpp) compiled for the host with
AddressSanitizer (tests/native/ctl_solve_host.cpp, a stand-alone program): the record writer the
build kernel runs equals capi_host.hpp nlp_batch_pack BITWISE — the batched search reads the device
record exactly as it reads the host's — at H = 1, 20 and 64, warm and selected, written by one thread
and by a block's stride; the parameter table takes the nominal model while warm and the bank's
column otherwise (NaN for a column the bank does not hold); the refusals' predicates give their
verdicts."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("ctl_solve") / "ctl_solve_host")
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fno-omit-frame-pointer",
           f"-I{os.path.join(REPO, 'lla-mpc_amd', 'csrc')}", f"-I{os.path.join(REPO, 'include')}",
           os.path.join(REPO, "tests", "native", "ctl_solve_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def run(harness, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    r = subprocess.run([harness, *map(str, args)], capture_output=True, text=True, env=env, check=True)
    return r.stdout.strip().splitlines()


@pytest.mark.parametrize("warm", [1, 0], ids=["warm", "selected"])
@pytest.mark.parametrize("H", [1, 20, 64])
def test_record_equals_nlp_batch_pack(harness, H, warm):
    for stride in (1, 256):
        out = run(harness, "record", H, warm, stride)
        rec_words, up_off, bad = map(int, out[0].split())
        assert up_off == 6 + 2 * (H + 1) + 2 * H and rec_words % 8 == 0 and rec_words >= up_off + 4
        assert bad == 0, (H, warm, stride, bad)
        for j, line in enumerate(out[1:7]):
            assert line.split() == [str(j), "1", "1"], line


def test_create_refusals(harness):
    """llampc_ctl_solver_create's state and cfg predicates."""
    ok = (0, 0, 0, 0, 0, 0.0)
    assert run(harness, "state", *ok) == ["ok"]
    for i, word in enumerate(("already has a solver", "outstanding", "armed", "unsharded", "unsharded")):
        args = list(ok)
        args[i] = 1
        assert word in run(harness, "state", *args)[0], (i, word)
    assert "corridor" in run(harness, "state", 0, 0, 0, 0, 0, 0.5)[0]
    good = (20, 0.02, 1024, 20, 0.02, 256)
    assert run(harness, "cfg", *good) == ["ok"]
    assert "H must equal" in run(harness, "cfg", 22, 0.02, 1024, 20, 0.02, 256)[0]
    assert "Ts must equal" in run(harness, "cfg", 20, 0.01, 1024, 20, 0.02, 256)[0]
    assert "one launch" in run(harness, "cfg", 20, 0.02, 4096 * 2, 20, 0.02, 256)[0]
    assert run(harness, "cfg", 20, 0.02, 4096, 20, 0.02, 256) == ["ok"]           # 64 blocks: persistent
    assert "CUs" in run(harness, "cfg", 20, 0.02, 1024, 20, 0.02, 8)[0]
    assert run(harness, "cfg", 20, 0.02, 512, 20, 0.02, 8) == ["ok"]


def test_attached_setters(harness):
    """While a solver is attached: prelaunch on, a corridor weight, an exchange and a gather transport
    are refused; switching off and a controller without a solver are not."""
    for setter, word in enumerate(("armed", "corridor", "set_exchange", "set_gather")):
        assert word in run(harness, "blocks", 1, setter, 1)[0]
        assert run(harness, "blocks", 1, setter, 0) == ["ok"]
        assert run(harness, "blocks", 0, setter, 1) == ["ok"]


def test_applied_values(harness):
    assert run(harness, "applied", 20, -1) == ["1 1"]
    assert run(harness, "applied", 20, 0) == ["0 0"]
    assert run(harness, "applied", 20, 1) == ["0 0"]
    assert run(harness, "applied", 20, 2) == ["0 1"]             # useq alone is bad: NULL passes
    assert run(harness, "applied", 20, 2 + 39) == ["0 1"]
    assert run(harness, "applied", 1, 3) == ["0 1"]

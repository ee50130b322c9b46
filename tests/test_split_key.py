"""The plan record's look-ahead best is a key (goff + n) C + c that final_write splits with split_key
(csrc/dev_wave.hpp) instead of the 64-bit / and %.  split_key is device code; split_key_hd in the same
header is its arithmetic, host-callable (split_key calls it), and tests/native/split_key_host.cpp holds it
exact against / and % on the CPU: C in {1, 2, 3, 63, 64, 65, 1000}; keys 0, C - 1, C, m C - 1, m C, m C + 1
for m up to 10^7 (every m to 4096, then every 997th, and 10^7 itself); the 4097 keys around 2^53 and the
multiples of C next to it.  No GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_split_key_equals_div_mod(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    out = str(tmp_path / "split_key_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           f"-I{os.path.join(REPO, 'lla-mpc_amd', 'csrc')}", f"-I{os.path.join(REPO, 'include')}",
           os.path.join(REPO, "tests", "native", "split_key_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([out], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[-1]) > 7 * 3 * 14000

"""The batched corridor solve without a device: (1) the conditions of
tests/nlp_batch_corridor_cases.py on the restatement alone — every compared problem's round-0 share
of penalised samples, its smallest adjacent elite-cost gap, the unconstrained optimum's slack and
the count of problems the corridor moved — so that the GPU module's bitwise comparisons can neither
pass vacuously nor hang on a rank flip; (2) the constructor's refusals, which need no device; and
(3) the pure host helpers the C ABI uses for the corridors (csrc/capi_host.hpp: the corridor
buffer's layout and pack, the per-problem argument checks, the slack per problem), compiled into a
stand-alone program (tests/native/nlp_batch_corridor_host.cpp) with AddressSanitizer and UBSan and
run on the CPU as a subprocess.  Nothing sanitised is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nlp_batch_cases as BC
import nlp_batch_corridor_cases as CC
import nlp_matrix as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HMAX = 64


@pytest.mark.parametrize("shape", CC.MIXED_SHAPES, ids=BC.sid)
def test_mixed_batch_meets_the_conditions(shape):
    refs = CC.mixed(shape)
    CC.check_mixed_conditions(shape, refs, CC.MIXED_MOVED[shape])
    # every problem has its own half-planes and its own weight
    hp = CC.mixed_hp(refs)
    assert len({h.tobytes() for h in hp}) == 6 and set(CC.weights()) == {1e3, 1e5}
    assert [r["w"] for r in refs] == CC.weights().tolist()


def test_the_restatement_without_half_planes_is_the_oracles():
    """nlp_cem_corridor with hp = None and a problem's own p6, seed and shape is oracle.nlp_cem."""
    for shape in (CC.MIXED_SHAPES[0], CC.MIXED_SHAPES[1]):
        for p, (m, t, s) in enumerate(zip(BC.MODELS, BC.TICKS, BC.SEEDS)):
            np.testing.assert_array_equal(CC.plain(shape, m, t, s)["u"], BC.restate(shape, m, t, s)["u"])


def test_chain_meets_the_conditions():
    outs = CC.chain()
    for call, (ref, plain) in enumerate(outs):
        CC.check_problem_conditions(BC.CHAIN_SHAPE, ref, f" chain call {call}")
        assert ref["moved"]
        BC.check_conditions(BC.CHAIN_SHAPE, plain, f" chain call {call} slot 1")
    # slot 0's warm start is its own previous corridor solution: the calls differ
    assert len({r["u"].tobytes() for r, _ in outs}) == 3


def test_chunks_meet_the_conditions():
    refs = CC.chunked()
    CC.check_mixed_conditions(BC.CHUNK_SHAPE, refs, 4, " chunked")
    assert [p // BC.CHUNK_PER_LAUNCH for p in range(BC.CHUNK_B)] == [0, 0, 1, 1, 2]


@pytest.mark.parametrize("shape", CC.DEVICE_SHAPES, ids=BC.sid)
def test_device_built_batch_meets_the_conditions(shape):
    """On the host-built corridors along the same paths (the device's agree with them to 1e-12)."""
    CC.check_device_conditions(shape, CC.device_refs(shape, CC.device_host_corridors(shape)))


def test_constructor_refusals_need_no_device():
    from llampc.mpc import ModelBank, setupNLPBatch
    c = BC.case(BC.SHAPES[0])
    bank = ModelBank.__new__(ModelBank)      # never opened: every refusal below comes before the library
    args = (c.Ts, c.Q, c.P, c.R, M.params(c), bank)
    for H in (0, HMAX + 1, 100):
        with pytest.raises(ValueError, match="horizon"):
            setupNLPBatch(H, *args)
    for w in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="corridor_weight"):
            setupNLPBatch(20, *args, corridor_weight=w)
    with pytest.raises(ValueError, match="track"):
        setupNLPBatch(20, *args, device_corridor=True)
    tr = CC.track()
    for m in (float(tr.track_width) / 2, 1.0, np.nan):
        with pytest.raises(ValueError, match="margin"):
            setupNLPBatch(20, *args, track=tr, device_corridor=True, corridor_margin=m)
    with pytest.raises(TypeError):           # the new arguments are keyword-only
        setupNLPBatch(20, *args, 8, 64, 3, 32, (0.3, 0.15), 1e-4, 0, None, tr)


# ---- the host helpers, under the sanitizers ------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("nlp_batch_corridor") / "nlp_batch_corridor_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer",
           f"-I{os.path.join(REPO, 'lla-mpc_amd', 'csrc')}", f"-I{os.path.join(REPO, 'include')}",
           os.path.join(REPO, "tests", "native", "nlp_batch_corridor_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)

    def run(*args):
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([out, *map(str, args)], capture_output=True, text=True, env=e)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return r.stdout
    return run


@pytest.mark.parametrize("H", [1, 20, 29, 64])
def test_corridor_layout_holds_what_the_kernels_touch(harness, H):
    """From the kernels' own indexing: the search reads doubles [0, 6 H) and the one at w_off of a
    problem's part, the builder writes rows [0, 6 H) and theta_off + [0, H) and reads [0, 2 (H + 1))
    of a problem's path: all inside the strides for every H <= HMAX; parts are whole 64-byte lines."""
    B = 5
    lines = harness("layout", H, B).splitlines()
    cor, theta, w, path, a_cor, a_w = map(int, lines[0].split())
    assert theta >= 6 * HMAX and w >= theta + HMAX and cor > w and path >= 2 * (HMAX + 1)
    assert cor % 8 == 0 and path % 8 == 0
    assert (a_cor, a_w) == (cor, w)
    # the packed parts read back: rows and weight in place, the rest untouched by any neighbour
    assert [tuple(map(int, ln.split())) for ln in lines[1:]] == [(p, 0) for p in range(B)]


def test_per_problem_argument_checks(harness):
    ok = lambda *a: harness("check", *a).strip()
    assert ok(6, 20, 0, "ok") == "ok"
    assert ok(6, 20, 3, "pinf_off") == "ok"                # +inf disables a half-plane
    for badp in (0, 2, 5):
        assert ok(6, 20, badp, "normal") == f"problem {badp}: a normal component is not finite"
        for what in ("nan_off", "ninf_off"):
            got = ok(6, 20, badp, what)
            assert got.startswith(f"problem {badp}: an offset"), got
        for what in ("neg_w", "nan_w", "inf_w", "nohp_neg_w"):
            assert ok(6, 20, badp, what) == f"problem {badp}: weight must be finite and >= 0"
    assert ok(6, 20, 0, "null_w") == "weight is NULL"
    assert ok(1, 1, 0, "ok") == "ok" and ok(1, 64, 0, "nan_off").startswith("problem 0")


def test_path_checks(harness):
    ok = lambda *a: harness("paths", *a).strip()
    assert ok(6, 20, 0, -1) == "ok"
    assert ok(6, 20, 4, 0) == "problem 4: path entry 0 is not finite"
    assert ok(6, 20, 5, 41) == "problem 5: path entry 41 is not finite"
    assert ok(1, 64, 0, 129) == "problem 0: path entry 129 is not finite"


@pytest.mark.parametrize("H", [1, 8, 20])
def test_slack_per_problem(harness, H):
    want, got, failed, no_tag, single = map(float, harness("slack", H).split())
    assert got == want == single           # the single solver's corridor_max_slack
    assert failed == 0.0 and no_tag == 0.0
    assert (want > 0) == (H > 5)

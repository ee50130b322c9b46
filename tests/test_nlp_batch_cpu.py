"""The batched NLP solve without a device: (1) the conditions of tests/nlp_batch_cases.py on the
restatement alone — every compared solve has all its samples finite in every round and its smallest
adjacent elite-cost gap above nlp_matrix.GAP_MIN, so the GPU module's bitwise umpc comparisons can
neither pass vacuously nor hang on a rank flip — and (2) the pure host helpers the C ABI uses for
the batch (csrc/capi_host.hpp: the buffer layout, the record pack, the create / solve refusals, the
B-tag wait), compiled into a stand-alone program (tests/native/nlp_batch_host.cpp) with
AddressSanitizer and UBSan and run on the CPU.  What the program prints must equal what is worked
out here from the kernel's own use of the buffers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import nlp_batch_cases as BC
import nlp_matrix as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HMAX = 64


@pytest.mark.parametrize("shape", BC.SHAPES, ids=BC.sid)
def test_first_solves_meet_the_conditions(shape):
    refs = BC.restate_batch(shape)
    for ref in refs:
        BC.check_conditions(shape, ref)
    # the model that appears twice (problems 1 and 2) is solved from different states
    assert BC.MODELS[1] == BC.MODELS[2] and not np.array_equal(refs[1]["u"], refs[2]["u"])


def test_cases_are_not_vacuous():
    """The best round varies over the cases (a result from the last round and from an earlier one:
    both writers of the result), and the two slots of the chain really change / keep their model."""
    rounds = {r["info"]["best_round"] for s in BC.SHAPES for r in BC.restate_batch(s)}
    print("best rounds", sorted(rounds))
    assert {0, 1, 2} <= rounds
    gaps = [(r["info"]["gap"], BC.sid(s), r["model"]) for s in BC.SHAPES for r in BC.restate_batch(s)]
    print("smallest gap", min(gaps))
    assert min(gaps)[0] > M.GAP_MIN
    assert len({m[0] for m in BC.CHAIN_MODELS}) == 3 and len({m[1] for m in BC.CHAIN_MODELS}) == 1


def test_chain_chunks_and_isolation_meet_the_conditions():
    for call, refs in enumerate(BC.restate_chain()):
        for ref in refs:
            BC.check_conditions(BC.CHAIN_SHAPE, ref, f" chain call {call}")
    for p, ref in enumerate(BC.restate_chunked()):
        BC.check_conditions(BC.CHUNK_SHAPE, ref, f" chunk call {p // BC.CHUNK_PER_LAUNCH}")
    first, nxt = BC.restate_isolation()
    for p, ref in enumerate(first):
        if p == BC.ISO_BAD:
            assert ref["u"] is None and ref["j"] == np.inf and ref["info"]["finite"] == [0] * BC.ISO_SHAPE[2]
        else:                            # the neighbours are the clean batch's problems
            assert ref is BC.restate_batch(BC.ISO_SHAPE)[p]
    for ref in nxt:
        BC.check_conditions(BC.ISO_SHAPE, ref, " after the NaN neighbour")


# ---- the host helpers, under the sanitizers ------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("nlp_batch") / "nlp_batch_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer",
           f"-I{os.path.join(REPO, 'lla-mpc_amd', 'csrc')}", f"-I{os.path.join(REPO, 'include')}",
           os.path.join(REPO, "tests", "native", "nlp_batch_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)

    def run(*args):
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([out, *map(str, args)], capture_output=True, text=True, env=e)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return r.stdout
    return run


def list_len(elite):
    return 1 << max(0, (elite - 1).bit_length())


@pytest.mark.parametrize("H,samples", [(1, 64), (20, 1024), (22, 256), (29, 64), (40, 128), (64, 4096)])
def test_layout_holds_what_the_kernel_touches(harness, H, samples):
    """Strides from the kernel's own indexing: a problem's record, lists (both parities, three word
    rows of nl x len <= samples entries), sequences (both parities, [samples][H][2]) and mean / std
    words ([4 H] doubles as two tagged halves) all end inside its stride, so problem p + 1's start
    where problem p's end; records are whole 64-byte lines."""
    B = 5
    lines = harness("layout", H, samples, B).splitlines()
    rec, up, lst, cand, ms, tag, nl_log2 = map(int, lines[0].split())
    assert up == 6 + 2 * (H + 1) + 2 * H                  # x0 | xref | the first mean, then uprev
    assert rec >= up + 4 and rec % 8 == 0 and rec - (up + 4) < 8
    nl = samples // 64
    assert 1 << nl_log2 == nl
    for elite in (1, 17, 32, 64):
        if elite <= samples:
            assert lst >= 2 * 3 * nl * list_len(elite)
    assert cand >= 2 * samples * H * 2
    assert ms >= 2 * 4 * H and ms == 8 * HMAX
    assert tag * 8 == 64                                   # a problem's host tag on its own line
    # the packed records read back: every field, and the pad after it untouched by any neighbour
    assert [tuple(map(int, ln.split())) for ln in lines[1:]] == [(p, 0) for p in range(B)]


def test_create_refusals(harness):
    ok = lambda *a: harness("create", *a).strip()
    assert ok(12, 1024, 8, 256) == "ok"
    assert ok(1, 64, 1, 1) == "ok"
    assert ok(12, 1024, 16, 256) == "ok"                   # exactly the chip
    assert "exceed" in ok(12, 1024, 17, 256)
    assert "exceed" in ok(12, 4096, 1, 32)
    assert "exceed" in ok(12, 64, 1, 0)                    # an unknown CU count admits nothing
    assert "max_batch" in ok(12, 64, 0, 256) and "max_batch" in ok(12, 64, -3, 256)
    assert "no model" in ok(0, 64, 1, 256)
    assert "index word" in ok(2 ** 32, 64, 1, 256) and ok(2 ** 32 - 1, 64, 1, 256) == "ok"
    assert "exceed" in ok(12, 4096, 2 ** 31 - 1, 256)      # the product in 64 bits


def test_solve_refusals(harness):
    ok = lambda B, mb, n, mask, *idx: harness("args", B, mb, n, mask, *idx).strip()
    assert ok(3, 8, 12, 0, 0, 11, 5) == "ok"
    for bit in range(9):                                   # each required pointer in turn
        assert ok(3, 8, 12, 1 << bit, 0, 11, 5) == "NULL argument"
    assert "B outside" in ok(0, 8, 12, 0, 0)
    assert "B outside" in ok(-1, 8, 12, 0, 0)
    assert "B outside" in ok(9, 8, 12, 0, *range(9))
    assert ok(8, 8, 12, 0, *range(8)) == "ok"
    assert "model index" in ok(3, 8, 12, 0, 0, -1, 5)
    assert "model index" in ok(3, 8, 12, 0, 0, 5, 12)
    assert "model index" in ok(1, 8, 12, 0, 2 ** 40)


def test_one_bounded_wait_for_all_tags(harness):
    """Every tag present: no timeout.  Tags missing: the timeout handler runs ONCE for the whole
    batch, the missing are reported, those behind a missing one are still seen."""
    assert harness("tags", 4, 7, 0b1111).split() == ["0", "0", "1", "1", "1", "1"]
    assert harness("tags", 4, 7, 0b1011).split() == ["0", "1", "1", "1", "0", "1"]
    assert harness("tags", 4, 7, 0b0100).split() == ["0", "1", "0", "0", "1", "0"]
    assert harness("tags", 1, 1, 0).split() == ["0", "1", "0"]

"""The track tick without a GPU (cases and oracle: plan_track_cases.py): the margins' preconditions on
the oracle alone; csrc's host-checkable parts in a stand-alone program built with AddressSanitizer and
UBSan (tests/native/plan_track_host.cpp) — plan_shape with a track, the path rule's index, the host's
half of the path's validity as a state machine; the Python layer's argument checks, which raise before
any device call; the new C entries declared and bound."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import plan_track_cases as PC
from conftest import REPO

HIPCC = "/opt/rocm/bin/hipcc"
RK4, EULER, RK6 = 0, 1, 2
KBLOCK, ONE_BLOCK_LDS = 256, 82 * 1024


@pytest.mark.parametrize("key", list(PC.CHAIN), ids=lambda k: f"{k[0][0]}x{k[0][1]}-{k[1]}")
def test_margin_preconditions(key):
    """On the oracle alone, under CHAIN's margins and weight: the path is valid from tick 1 on, between
    10 % and 90 % of the pairs pay a penalty in at least two valid ticks (here: in every one, the table's
    share to 0.01), and the selected model's argmin under J_c leaves its plain argmin in the ticks the
    table names — at least one for the chain test's shapes."""
    row, outs = PC.CHAIN[key], PC.oracle_chain(*key)
    shares = [o["share"] for o in outs[1:]]
    moved = tuple(t for t, o in enumerate(outs) if o["moved"])
    print(f"{key}: weight {row['weight']:g} margins {row['margins']} shares {[round(s, 3) for s in shares]} moved {moved}")
    assert [o["valid"] for o in outs] == [False] + [True] * (PC.TICKS - 1)
    assert np.array_equal(outs[0]["cref"], outs[0]["plain"])
    assert sum(0.1 <= s <= 0.9 for s in shares) >= 2
    np.testing.assert_allclose(shares, row["shares"], atol=0.01)
    assert moved == row["moved"]
    if key in ((PC.S, "ETHZ"), (PC.UW, "ETHZ")):
        assert len(moved) >= 1
    tr = PC.track(key[1])
    assert all(m < tr.track_width / 2 for m in row["margins"])


def test_python_argument_checks():
    """ValueError before any device call: corridor= with track_corridor=, no track, no look-ahead, rk6,
    euler_nlp, raceline_start, a bad weight, a margin that leaves no corridor or is not finite; set_track
    on a track without the tables; a path of the wrong shape."""
    from llampc.mpc import ModelBank, constraints
    from llampc.mpc.bank import check_track_tick
    tr = PC.track()
    assert check_track_tick(tr, 1e4, 0.05) == (1e4, 0.05)
    with pytest.raises(ValueError, match="cannot be combined"):
        check_track_tick(tr, 1e4, 0.0, corridor=constraints.disabled(12))
    with pytest.raises(ValueError, match="set_track"):
        check_track_tick(None, 1e4, 0.0)
    with pytest.raises(ValueError, match="look-ahead"):
        check_track_tick(tr, 1e4, 0.0, do_lookahead=False)
    for integ in ("rk6", "euler_nlp"):
        with pytest.raises(ValueError, match=f"no {integ} rollout"):
            check_track_tick(tr, 1e4, 0.0, integrator=integ)
    with pytest.raises(ValueError, match="raceline_start"):
        check_track_tick(tr, 1e4, 0.0, raceline_start=(0.0, 1.0, 1.0))
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="corridor_weight must be finite and >= 0"):
            check_track_tick(tr, w, 0.0)
    for m in (float(tr.track_width) / 2, 1.0):
        with pytest.raises(ValueError, match="leaves no corridor"):
            check_track_tick(tr, 1e4, m)
    for m in (float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="not finite"):
            check_track_tick(tr, 1e4, m)
    # through the bank's methods, on an object that never reached the library
    b = ModelBank.__new__(ModelBank)
    b._h = None
    x, u = np.zeros(6), np.zeros(2)
    U, xref = np.zeros((3, 12, 2)), np.zeros((2, 13))
    with pytest.raises(ValueError, match="set_track"):
        b.plan_raw(x, u, x, U, xref, u, track_corridor=True)
    with pytest.raises(ValueError, match="cannot be combined"):
        b.plan_raw(x, u, x, U, xref, u, track_corridor=True, corridor=constraints.disabled(12))
    with pytest.raises(ValueError, match="set_track"):
        b.plan_async(x, u, x, U, xref, u, track_corridor=True)

    class Bare:
        pass
    with pytest.raises(ValueError, match="needs a track with center_line"):
        b.set_track(Bare())
    with pytest.raises(ValueError, match=r"path must be \[2, H\+1\]"):
        b.set_corridor_path(np.zeros((3, 13)))


def test_read_back_takes_no_horizon(monkeypatch):
    """ModelBank.track_corridor() has no horizon argument, and its buffers hold the largest horizon: a
    stand-in library that writes LLAMPC_HMAX's worth through every pointer (the most the real one can,
    whatever horizon it remembers) stays inside them, and the arrays come back cut to the horizon of
    the last track tick made through the object."""
    import inspect

    from llampc import _native as nat
    from llampc.mpc import ModelBank
    assert list(inspect.signature(ModelBank.track_corridor).parameters) == ["self"]
    HM = nat.HMAX

    class Lib:
        @staticmethod
        def llampc_bank_track_corridor(h, path, hp, theta, valid, nxt, nvalid, ncost):
            for ptr, n, base in ((path, 2 * (HM + 1), 0.0), (hp, 6 * HM, 1000.0), (theta, HM, 2000.0),
                                 (nxt, 2 * (HM + 1), 3000.0)):
                for i in range(n):
                    ptr[i] = base + i
            valid._obj.value, nvalid._obj.value, ncost._obj.value = 1, 1, 2.5
            return 0
    monkeypatch.setattr(nat, "load", lambda: Lib)
    b = ModelBank.__new__(ModelBank)
    b._h = 1
    with pytest.raises(nat.NativeError, match="horizon is unknown"):
        b.track_corridor()
    for H in (1, 12, HM):
        b._track_H = H
        rb = b.track_corridor()
        assert rb["path"].shape == rb["next_path"].shape == (2, H + 1) and rb["hp"].shape == (H, 6)
        assert rb["theta"].shape == (H,) and rb["valid"] and rb["next_valid"] and rb["next_cost"] == 2.5
        np.testing.assert_array_equal(rb["path"].ravel(), np.arange(2 * (H + 1)))
        np.testing.assert_array_equal(rb["hp"].ravel(), 1000.0 + np.arange(6 * H))
        np.testing.assert_array_equal(rb["next_path"].ravel(), 3000.0 + np.arange(2 * (H + 1)))
    b._h = None


def test_entries_declared_and_bound():
    from llampc import _native as nat
    text = open(os.path.join(REPO, "include", "llampc.h")).read()
    for name in ("llampc_bank_set_track", "llampc_bank_set_path", "llampc_plan_track", "llampc_plan_track_async",
                 "llampc_bank_track_corridor", "llampc_plan_variant_track"):
        assert f"int {name}(" in text and name in nat._SIGNATURES
    srcs = open(os.path.join(REPO, "lla-mpc_amd", "csrc", "Makefile")).read()
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert "plan_track_rk4.hip" in srcs and "plan_track_rk4.hip" in entry


# ---- the stand-alone host program -----------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("plan_track") / "plan_track_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer",
           f"-I{os.path.join(REPO, 'lla-mpc_amd', 'csrc')}", f"-I{os.path.join(REPO, 'include')}",
           os.path.join(REPO, "tests", "native", "plan_track_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)

    def run(*args):
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        for k in ("LLAMPC_LPM", "LLAMPC_NO_WQ", "LLAMPC_WQ_WAVES", "LLAMPC_LB_R"):
            e.pop(k, None)
        r = subprocess.run([out, *map(str, args)], capture_output=True, text=True, env=e)
        assert r.returncode == 0, r.stderr
        return r.stdout.strip().splitlines()
    return run


def shape(harness, n, C, H, K=10, lb=1, full=1, la=1, integ=RK4, xref=0, pack=0, px=0, corridor=0, track_n=0):
    lines = harness("shape", n, C, H, K, lb, full, la, integ, xref, pack, px, corridor, track_n)
    if lines[0].startswith("refuse "):
        return lines[0][len("refuse "):]
    return {k: int(v) for k, v in (ln.split() for ln in lines)}


SHAPES = (PC.S, PC.UW, PC.H1, PC.HM)


def track_ns():
    return (4, PC.track().center_line.shape[1], 4096)


@pytest.mark.parametrize("C,H", SHAPES, ids=lambda v: str(v))
def test_native_plan_shape_track(harness, C, H):
    """plan_shape with track_n > 0: the family, nb_cor = H, the grid nb_lb + H + nb_la, never the work
    queue, the LDS at least a corridor block's 64 + 24 n — the lane split, the staging and the block
    counts are the corridor launch's — and llampc_plan_variant_track reports the same."""
    from llampc import _native as nat
    assert track_ns()[1] == 666
    for tn in track_ns():
        for n, lb in ((PC.N, 1), (PC.N, 0), (100000, 1)):
            got = shape(harness, n, C, H, lb=lb, track_n=tn)
            cor = shape(harness, n, C, H, lb=lb, corridor=1)
            assert got["family"] == 3 and cor["family"] == 2
            for f in ("lpm", "G", "cpl", "stage", "nb_lb", "nb_la"):
                assert got[f] == cor[f], (f, n, C, H, tn)
            assert got["nb_cor"] == H and got["wq"] == 0
            assert got["grid"] == got["nb_lb"] + H + got["nb_la"]
            if not lb:                               # the corridor blocks come first
                assert got["nb_lb"] == 0 and got["grid"] == H + got["nb_la"]
            mpb = KBLOCK // (got["G"] * got["lpm"])
            assert got["nb_la"] == -(-n // mpb)
            assert got["lds"] >= 64 + 24 * tn and got["lds"] >= 192 + 16 * (H + 1) + 48 * H
            assert got["lds"] >= max(cor["lds"], ONE_BLOCK_LDS)
            if tn == 4096 and (C, H) != PC.UW:       # the tables outweigh everything else of these launches
                assert got["lds"] == 64 + 24 * 4096
            v = nat.plan_variant_track(n, C, H, tn)
            assert v == dict(lpm=got["lpm"], G=got["G"], cpl=got["cpl"], stage=bool(got["stage"]), nb_cor=H)
    # where the plain launch takes the work queue (C = 64 at LPM 1, many look-ahead blocks), the track tick does not
    if (C, H) == PC.UW:
        assert shape(harness, 100000, C, H)["wq"] != 0


def test_native_plan_shape_unchanged_without_track(harness):
    """track_n = 0 changes nothing: no corridor block, the families as before."""
    for C, H in SHAPES:
        for kw, fam in ((dict(), 0), (dict(corridor=1), 2)):
            got = shape(harness, PC.N, C, H, **kw)
            assert got["family"] == fam and got["nb_cor"] == 0 and got["grid"] == got["nb_lb"] + got["nb_la"]


def test_native_refusals(harness):
    """Every refusal of the track tick, by its own message."""
    C, H = PC.S
    tn = 666
    want = {
        "do_lookahead is 0": dict(la=0),
        "no RK6 rollout": dict(integ=RK6),
        "no NLP-Euler rollout": dict(integ=EULER),
        "given xref only": dict(xref=1),
        "no inline pack": dict(pack=1),
        "no fused peer exchange": dict(px=2),
    }
    for msg, kw in want.items():
        got = shape(harness, PC.N, C, H, track_n=tn, **kw)
        assert isinstance(got, str) and got.startswith("the track tick") and msg in got, (kw, got)
    assert len({shape(harness, PC.N, C, H, track_n=tn, **kw) for kw in want.values()}) == len(want)
    assert "builds its own corridor" in shape(harness, PC.N, C, H, track_n=tn, corridor=1)


def test_native_path_index(harness):
    """ctl_path_index at H = 1, 2 and 12: P_j = X_{j+1}, the last repeated; H = 1: P_0 = P_1 = X_1."""
    assert [int(v) for v in harness("index", 1)] == [1, 1]
    assert [int(v) for v in harness("index", 2)] == [1, 2, 2]
    assert [int(v) for v in harness("index", 12)] == list(range(1, 13)) + [12]
    for H in (1, 2, 12):
        assert [int(v) for v in harness("index", H)] == [PC.path_index(j, H) for j in range(H + 1)]


def test_native_validity_state_machine(harness):
    """The host's half of the path rule (capi_host.hpp track_path_next / track_path_offered)."""
    run = lambda *ev: [int(v) for v in harness("state", *ev)]
    assert run("offer:12") == [0]                                       # a fresh bank
    assert run("tick:12", "offer:12", "tick:12", "offer:12") == [1, 1]   # track -> tick -> tick
    assert run("tick:12", "plain", "offer:12") == [0]                    # a plain tick between
    assert run("tick:12", "plain", "tick:12", "offer:12") == [1]          # ... and the chain starts again
    assert run("seed:12", "offer:12") == [1]                              # set_path seeds
    assert run("tick:12", "plain", "seed:12", "offer:12") == [1]
    assert run("tick:12", "offer:20", "offer:12") == [0, 1]                # an H change
    assert run("seed:12", "offer:1") == [0]
    assert run("tick:12", "clear", "offer:12") == [0]                      # set_track, reset, set_path(NULL)
    assert run("seed:12", "clear", "offer:12") == [0]
    assert run("seed:12", "plain", "offer:12") == [0]


def test_native_tick_arguments(harness):
    assert harness("tick", 1e4, 0.05, 0.37) == ["ok"]
    assert harness("tick", 0.0, -0.5, 0.37) == ["ok"]
    for w in ("-1", "nan", "inf"):
        assert "weight" in harness("tick", w, 0.0, 0.37)[0]
    for m in ("0.185", "1", "nan", "inf", "-inf"):
        assert "margin" in harness("tick", 1e4, m, 0.37)[0]

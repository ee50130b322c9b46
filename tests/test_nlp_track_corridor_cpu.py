"""The device-built track corridor's host side, no GPU: csrc/corridor_dev.hpp's __host__ __device__
functions compiled for the host with AddressSanitizer and UBSan (tests/native/track_corridor_host.cpp)
against constraints.track_corridor and Track.xy_to_param on the nine cases of
tests/track_corridor_cases.py at 1e-12 (derived there); the three new C entries' declarations
against their ctypes signatures; the refusals setupNLP makes before it touches the library; and
constraints.default_path."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import track_corridor_cases as TC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("track_corridor")
    out = str(tmp / "track_corridor_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer",
           f"-I{os.path.join(REPO, 'lla-mpc_amd', 'csrc')}", f"-I{os.path.join(REPO, 'include')}",
           os.path.join(REPO, "tests", "native", "track_corridor_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)

    def run(c):
        tr = c["track"]
        n = tr.center_line.shape[1]
        hw = float(tr.track_width) / 2 - c["margin"]
        words = np.concatenate([[n, c["H"], float(tr.track_length), hw], tr.center_line[0], tr.center_line[1],
                                tr.theta_track, c["path"].ravel()]).astype(np.float64)
        f = str(tmp / "case.bin")
        words.tofile(f)
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([out, f], capture_output=True, text=True, env=e)
        assert r.returncode == 0, r.stderr
        got = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
        assert got.shape == (2 * c["H"], 7)
        return got[:c["H"]], got[c["H"]:]
    return run


@pytest.mark.parametrize("name", TC.CASES)
def test_header_functions_equal_host_corridor(harness, name):
    """corridor_record (one scan) and the kernel's split of the scan (256 strided partial scans,
    merged with ties to the lower segment) give the same rows bitwise, and those equal
    constraints.track_corridor and xy_to_param to 1e-12."""
    c = TC.case(name)
    scan, split = harness(c)
    np.testing.assert_array_equal(scan, split)
    hp, theta = scan[:, 1:], scan[:, 0]
    print(f"{name}: max |hp - host| {np.max(np.abs(hp - c['hp'])):.3g} max |theta - host| "
          f"{np.max(np.abs(theta - c['theta'])):.3g}")
    np.testing.assert_allclose(hp, c["hp"], rtol=0, atol=TC.TOL)
    np.testing.assert_allclose(theta, c["theta"], rtol=0, atol=TC.TOL)
    np.testing.assert_array_equal(hp[:, 3:5], -hp[:, 0:2])


def test_cases_take_the_branches_they_are_for():
    """On the host reference alone: the wrap case lands on the closing segment and on both sides
    of the lap's end; the vertex case's points are centre points; the polygons have the sizes that
    put fewer segments than lanes, and a second segment, into a lane."""
    w = TC.case("ethz-wrap")
    tr = w["track"]
    L = float(tr.track_length)
    assert np.any(w["theta"] > tr.theta_track[-1]) and np.any(w["theta"] < 1.0) and np.any(w["theta"] > L - 1.0)
    assert np.any((w["theta"] + 0.05 >= L)) and np.any(w["theta"] - 0.05 < 0)
    v = TC.case("mobil-vertices")
    n = v["track"].center_line.shape[1]
    np.testing.assert_array_equal(v["path"], v["track"].center_line[:, n // 2:n // 2 + 21])
    assert n // 2 > 0 and n // 2 + 21 < n
    assert [TC.case(f"polygon-{k}")["track"].center_line.shape[1] for k in (5, 64, 257)] == [5, 64, 257]
    assert TC.case("ethz-H64")["H"] == 64 and TC.case("ethz-H1")["hp"].shape == (1, 6)


ENTRIES = {"llampc_nlp_set_track": 6, "llampc_nlp_track_corridor": 5, "llampc_nlp_solve_track": 14}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_declares_track_entries(name):
    """The C header's declaration and the ctypes signature carry the same number of arguments."""
    from llampc import _native
    src = open(os.path.join(REPO, "include", "llampc.h")).read()
    decl = src[src.index(f"int {name}("):]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)      # the shapes' comments hold commas
    assert decl.count(",") + 1 == ENTRIES[name] == len(_native._SIGNATURES[name][1])
    assert "#define LLAMPC_ABI_VERSION 1\n" in src            # additions only


def _nlp(track, H=20, **kw):
    from llampc.models import Dynamic
    from llampc.mpc.nmpc import setupNLP
    from llampc.params import ORCA
    p = ORCA(control="pwm")
    return setupNLP(H, TC.TS, np.eye(2), np.zeros((2, 2)), np.diag([5e-3, 1]), p, Dynamic(**p), track, **kw)


@pytest.fixture
def no_library(monkeypatch):
    from llampc import _native
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("the library was touched"))


def test_constructor_refusals_before_the_library(no_library, tmp_path):
    """device_corridor=True without a track, with a track that lacks the centre line's tables
    (Raceline.from_raceline_npz) or with a margin that leaves no corridor: ValueError, no library
    call; device_corridor=False takes any of them, as before."""
    from llampc.tracks import Raceline
    tr = TC.track("ETHZ")
    f = str(tmp_path / "rl.npz")
    np.savez(f, x=tr.x_raceline, y=tr.y_raceline, speed=np.ones_like(tr.x_raceline), time=np.zeros_like(tr.x_raceline))
    bare = Raceline.from_raceline_npz(f)
    with pytest.raises(ValueError, match="device_corridor"):
        _nlp(None, device_corridor=True)
    with pytest.raises(ValueError, match="center_line"):
        _nlp(bare, device_corridor=True)
    for m in (tr.track_width / 2, 1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="corridor_margin"):
            _nlp(tr, device_corridor=True, corridor_margin=m)
    for t in (None, bare):
        nlp = _nlp(t, corridor_margin=1.0)
        assert nlp.device_corridor is False and nlp._h is None
    nlp = _nlp(tr, device_corridor=True, corridor_margin=0.03)
    assert nlp.device_corridor and nlp.corridor_margin == 0.03 and nlp.last_corridor is None
    assert nlp._h is None and nlp._bank is None
    with pytest.raises(NotImplementedError, match=r"corridor=.*constraints\.track_corridor"):
        _nlp(tr, track_cons=True, device_corridor=True)


@pytest.mark.parametrize("shape", [(2, 20), (2, 22), (21, 2), (42,), (6, 21)])
def test_corridor_path_shape_refused_before_the_library(no_library, shape):
    nlp = _nlp(TC.track("ETHZ"), device_corridor=True)
    with pytest.raises(ValueError, match="corridor_path"):
        nlp.solve(np.zeros(6), np.zeros((2, 21)), np.zeros(2), corridor_path=np.zeros(shape))
    with pytest.raises(ValueError, match="corridor_path"):
        nlp.track_corridor(np.zeros(shape))
    assert nlp._h is None and nlp._bank is None


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_corridor_path_values_refused_before_the_library(no_library, bad):
    nlp = _nlp(TC.track("ETHZ"), device_corridor=True)
    path = np.zeros((2, 21))
    path[1, 20] = bad
    with pytest.raises(ValueError, match="finite"):
        nlp.solve(np.zeros(6), np.zeros((2, 21)), np.zeros(2), corridor_path=path)
    with pytest.raises(ValueError, match="finite"):
        nlp.track_corridor(path)
    assert nlp._h is None and nlp._bank is None


def test_corridor_path_needs_device_corridor(no_library):
    nlp = _nlp(TC.track("ETHZ"))
    with pytest.raises(ValueError, match="device_corridor"):
        nlp.solve(np.zeros(6), np.zeros((2, 21)), np.zeros(2), corridor_path=np.zeros((2, 21)))
    with pytest.raises(ValueError, match="device_corridor"):
        nlp.track_corridor(np.zeros((2, 21)))
    assert nlp._h is None


def test_default_path():
    """The first solve's ray P_k = (X0, Y0) + k Ts max(vx0, 0.05) (cos psi0, sin psi0), and the
    later solves' shifted positions, bitwise against slicing."""
    from llampc.mpc import constraints
    x0 = np.array([0.7, -1.2, 0.6, 1.5, 0.1, -0.3])
    for H in (1, 20, 64):
        P = constraints.default_path(x0, H, 0.02)
        assert P.shape == (2, H + 1)
        k = np.arange(H + 1)
        np.testing.assert_allclose(P[0], 0.7 + k * 0.02 * 1.5 * np.cos(0.6), rtol=0, atol=1e-15)
        np.testing.assert_allclose(P[1], -1.2 + k * 0.02 * 1.5 * np.sin(0.6), rtol=0, atol=1e-15)
        assert P[0, 0] == 0.7 and P[1, 0] == -1.2
    # a car that stands or rolls backwards: the NLP's own vmin
    for vx in (0.0, -0.4, 0.01):
        P = constraints.default_path([0.0, 0.0, np.pi / 2, vx, 0.0, 0.0], 20, 0.02)
        np.testing.assert_allclose(P[1], np.arange(21) * 0.02 * 0.05, rtol=0, atol=1e-15)
        np.testing.assert_allclose(P[0], 0.0, atol=1e-16)
    rng = np.random.RandomState(3)
    xm = rng.standard_normal((6, 21))
    keep = xm.copy()
    P = constraints.default_path(x0, 20, 0.02, prev_xmpc=xm)
    np.testing.assert_array_equal(P[:, :-1], xm[:2, 1:])
    np.testing.assert_array_equal(P[:, -1], xm[:2, -1])
    np.testing.assert_array_equal(xm, keep)
    np.testing.assert_array_equal(constraints.default_path(x0, 20, 0.02, prev_xmpc=xm[:2]), P)
    with pytest.raises(ValueError):
        constraints.default_path(x0, 19, 0.02, prev_xmpc=xm)

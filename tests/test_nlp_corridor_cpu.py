"""The corridor's host side, no GPU: llampc.mpc.constraints (track_corridor, strip, slacks), the
argument checks setupNLP makes before it touches the library, and the C ABI's pure corridor
helpers (csrc/capi_host.hpp corridor_max_slack, corridor_invalid) compiled for the host with
AddressSanitizer and UBSan (tests/native/corridor_host.cpp) against hand-computed corridors."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INF = float("inf")


def _track(name):
    from llampc.tracks import ETHZ, ETHZMobil
    return (ETHZ if name == "ETHZ" else ETHZMobil)('optimal', True)


def _centre_run(tr, start, H=20):
    """xref [2, H+1]: H + 1 consecutive centre-line points from index `start`, cyclically."""
    n = tr.center_line.shape[1]
    return tr.center_line[:, (start + np.arange(H + 1)) % n]


@pytest.mark.parametrize("name", ["ETHZ", "ETHZMobil"])
@pytest.mark.parametrize("place", ["start", "middle", "wrap"])
def test_track_corridor_geometry(name, place):
    """xref = 20 consecutive centre points (after the first) at three places, one across the lap
    wrap: every centre point has slack 0; c +/- (hw + 0.01) n leaves exactly one half-plane, by
    0.01 to 1e-12; margin shrinks the corridor by that amount."""
    from llampc.mpc import constraints
    tr = _track(name)
    n_pts = tr.center_line.shape[1]
    start = {"start": 3, "middle": n_pts // 2, "wrap": n_pts - 9}[place]
    xref = _centre_run(tr, start)
    H = xref.shape[1] - 1
    hw = tr.track_width / 2
    hp = constraints.track_corridor(tr, xref)
    assert hp.shape == (H, 6) and np.all(np.isfinite(hp))
    n = hp[:, 0:2]
    np.testing.assert_allclose(np.hypot(n[:, 0], n[:, 1]), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(hp[:, 3:5], -n)
    # the left normal: the run's direction turned by +90 degrees
    d = xref[:, 2:] - xref[:, :-2]
    d = np.concatenate([d, d[:, -1:]], axis=1)
    assert np.all(-d[1] * n[:, 0] + d[0] * n[:, 1] > 0)
    c = xref[:, 1:]                                   # the centres p_1 .. p_H
    np.testing.assert_allclose(hp[:, 2] + hp[:, 5], 2 * hw, rtol=0, atol=1e-12)

    def slacks_at(points, corridor=hp):
        return constraints.slacks(corridor, np.concatenate([xref[:, :1], points], axis=1))
    assert np.all(slacks_at(c) == 0.0)
    left, right = slacks_at(c + (hw + 0.01) * n.T), slacks_at(c - (hw + 0.01) * n.T)
    np.testing.assert_allclose(left[:, 0], 0.01, rtol=0, atol=1e-12)
    assert np.all(left[:, 1] == 0.0)
    np.testing.assert_allclose(right[:, 1], 0.01, rtol=0, atol=1e-12)
    assert np.all(right[:, 0] == 0.0)
    # margin: the same normals, each wall 0.05 closer
    hm = constraints.track_corridor(tr, xref, margin=0.05)
    np.testing.assert_array_equal(hm[:, [0, 1, 3, 4]], hp[:, [0, 1, 3, 4]])
    np.testing.assert_allclose(hm[:, [2, 5]], hp[:, [2, 5]] - 0.05, rtol=0, atol=1e-12)
    edge = slacks_at(c + (hw - 0.05 + 0.01) * n.T, hm)
    np.testing.assert_allclose(edge[:, 0], 0.01, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        constraints.track_corridor(tr, xref, margin=hw)


def test_strip_and_disabled():
    """strip around a polyline: the normal of P[min(k+1, H)] - P[k-1] turned left, the centre
    n.P[k] + offset_k, the half-width; disabled() constrains nothing."""
    from llampc.mpc import constraints
    P = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [2.0, 1.0]])          # east, east, then north
    hp = constraints.strip(P, 0.25, [0.0, 0.5, 0.0])
    s = np.sqrt(0.5)
    np.testing.assert_allclose(hp[0], [0, 1, 0.25, 0, -1, 0.25], atol=1e-15)            # |Y| <= 0.25
    np.testing.assert_allclose(hp[1], [-s, s, -2 * s + 0.75, s, -s, 2 * s - 0.25], atol=1e-15)
    np.testing.assert_allclose(hp[2], [-1, 0, -2 + 0.25, 1, 0, 2 + 0.25], atol=1e-15)   # |X - 2| <= 0.25
    np.testing.assert_array_equal(constraints.strip(P.T, 0.25, [0.0, 0.5, 0.0]), hp)
    assert np.all(constraints.slacks(hp[[0, 2]], np.array([[0.0, 1.0, 2.0], [0.0, 0.0, 1.0]])) == 0.0)
    np.testing.assert_allclose(constraints.slacks(hp[:1], np.array([[0.0, 1.0], [0.0, 0.5]])), [[0.25, 0.0]])
    off = constraints.disabled(3)
    assert off.shape == (3, 6) and np.all(off[:, [2, 5]] == INF) and np.all(off[:, [0, 1, 3, 4]] == 0)
    assert np.all(constraints.slacks(off, 1e6 * np.ones((2, 4))) == 0.0)
    with pytest.raises(ValueError):
        constraints.strip(np.zeros((1, 2)), 0.1)


def _nlp(**kw):
    from llampc.models import Dynamic
    from llampc.mpc.nmpc import setupNLP
    from llampc.params import ORCA
    p = ORCA(control="pwm")
    return setupNLP(20, 0.02, np.eye(2), np.zeros((2, 2)), np.diag([5e-3, 1]), p, Dynamic(**p), None, **kw)


@pytest.mark.parametrize("shape", [(19, 6), (20, 5), (6, 20), (120,), (21, 6)])
def test_solve_rejects_corridor_shape_before_the_library(shape, monkeypatch):
    """A corridor that is not [H, 6] raises before any device object exists (no library call)."""
    from llampc import _native
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("the library was touched"))
    nlp = _nlp()
    with pytest.raises(ValueError, match="corridor"):
        nlp.solve(np.zeros(6), np.zeros((2, 21)), np.zeros(2), corridor=np.zeros(shape))
    assert nlp._h is None and nlp._bank is None


def test_corridor_constructor_arguments():
    nlp = _nlp()
    assert nlp.corridor_weight == 1e4 and nlp.corridor_tol == 1e-4 and nlp.max_slack == 0.0
    nlp = _nlp(corridor_weight=250.0, corridor_tol=1e-3)
    assert nlp.corridor_weight == 250.0 and nlp.corridor_tol == 1e-3
    for w in (-1.0, float("nan"), INF):
        with pytest.raises(ValueError):
            _nlp(corridor_weight=w)


def test_track_cons_points_to_corridor():
    with pytest.raises(NotImplementedError, match=r"corridor=.*constraints\.track_corridor"):
        _nlp(track_cons=True)


def test_header_declares_corridor_entry():
    """The C header's declaration and the ctypes signature carry the same twelve arguments."""
    from llampc import _native
    src = open(os.path.join(REPO, "include", "llampc.h")).read()
    decl = src[src.index("int llampc_nlp_solve_corridor("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == 12 == len(_native._SIGNATURES["llampc_nlp_solve_corridor"][1])
    assert "#define LLAMPC_ABI_VERSION 1\n" in src            # additions only


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("corridor") / "corridor_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer",
           f"-I{os.path.join(REPO, 'lla-mpc_amd', 'csrc')}", f"-I{os.path.join(REPO, 'include')}",
           os.path.join(REPO, "tests", "native", "corridor_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)

    def run(*args):
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([out, *map(str, args)], capture_output=True, text=True, env=e)
        assert r.returncode == 0, r.stderr
        return r.stdout.strip()
    return run


def _traj(points):
    """xmpc [H+1][6] flattened: p_0 = (9, 9) and the given positions, the other states 7."""
    rows = [[9.0, 9.0, 7.0, 7.0, 7.0, 7.0]] + [[x, y, 7.0, 7.0, 7.0, 7.0] for x, y in points]
    return [v for r in rows for v in r]


# Hand-computed (every number a short binary fraction: the arithmetic is exact).
#  1. X <= 1 and Y <= 2 at both steps.  p_1 = (1.5, 1): s = (0.5, 0); p_2 = (0.5, 2.25): s = (0, 0.25).
#  2. every half-plane disabled: 0 wherever the trajectory goes.
#  3. a = (0.5, -0.25), b = 1 and c = -a, d = 0.5: p_1 = (4, 2): a.p = 1.5, s1 = 0.5, c.p = -1.5;
#     p_2 = (-4, 8): a.p = -4, c.p = 4, s2 = 3.5; p_3 = (2, 0): a.p = 1, on the line, s = 0.
HAND = [
    ([[1, 0, 1, 0, 1, 2]] * 2, [(1.5, 1.0), (0.5, 2.25)], 0.5),
    ([[0, 0, INF, 0, 0, INF]] * 2, [(1e9, -1e9), (-3.0, 4.0)], 0.0),
    ([[0.5, -0.25, 1, -0.5, 0.25, 0.5]] * 3, [(4.0, 2.0), (-4.0, 8.0), (2.0, 0.0)], 3.5),
]


@pytest.mark.parametrize("hp,points,want", HAND, ids=["box", "disabled", "oblique"])
def test_max_slack_helper(harness, hp, points, want):
    from llampc.mpc import constraints
    H = len(hp)
    flat = [float(v) for r in hp for v in r]
    assert float(harness("slack", H, *flat, *_traj(points))) == want
    xy = np.array([(9.0, 9.0)] + points).T
    assert float(np.max(constraints.slacks(np.array(hp, dtype=float), xy))) == want


def test_corridor_invalid_helper(harness):
    """What llampc_nlp_solve_corridor refuses: a non-finite normal component, an offset NaN or
    -inf, a weight negative or non-finite; +inf offsets and weight 0 pass."""
    good = [0.5, -0.25, 1.0, -0.5, 0.25, INF] * 2

    def verdict(w, k=None, v=None):
        h = list(good)
        if k is not None:
            h[k] = v
        return harness("valid", 2, float(w), *h)
    assert verdict(1e4) == "ok" and verdict(0.0) == "ok" and verdict(1.0, 8, INF) == "ok"
    for k in (0, 1, 3, 4, 6, 10):
        for v in (float("nan"), INF, -INF):
            assert "normal" in verdict(1.0, k, v), (k, v)
    for k in (2, 5, 8, 11):
        for v in (float("nan"), -INF):
            assert "offset" in verdict(1.0, k, v), (k, v)
    for w in (-1.0, -0.0 - 1e-300, float("nan"), INF, -INF):
        assert "weight" in verdict(w), w

"""The track corridor built on the device (kernels.hip track_corridor_kernel, csrc/corridor_dev.hpp;
llampc_nlp_set_track, llampc_nlp_track_corridor, llampc_nlp_solve_track;
setupNLP(device_corridor=True)).

1. setupNLP.track_corridor against constraints.track_corridor and Track.xy_to_param on the nine
   cases of tests/track_corridor_cases.py, at its TOL = 1e-12 absolute (derived there).
2. The plumbing, bitwise: a device-corridor solver A (the first solve's ray, then the shifted
   positions) against a twin B that is handed A.last_corridor through ``corridor=`` — the search
   is llampc_nlp_solve_corridor's own launch in both, so umpc, fval and xmpc are equal bit for bit.
   Asserted first: the corridor binds (the unconstrained optimum leaves it by more than 0.01 and
   the solution moves), so the comparison cannot pass on a corridor nobody touches.
3. The C entries' refusals, and a second llampc_nlp_set_track replacing the first.
4. device_corridor=False changes nothing."""
import numpy as np
import pytest

import track_corridor_cases as TC

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
MARGIN = 0.03
SHAPES = [(64, 5, 3, 20), (512, 32, 3, 40), (1024, 32, 8, 20)]


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


def _solver(track, samples=1024, elite=32, iters=8, H=20, **kw):
    from llampc.models import Dynamic
    from llampc.mpc.nmpc import setupNLP
    from llampc.params import ORCA
    p = ORCA(control="pwm")
    return setupNLP(H, TC.TS, np.eye(2), np.zeros((2, 2)), np.diag([5e-3, 1]), p, Dynamic(**p), track,
                    samples=samples, elite=elite, iters=iters, **kw)


@pytest.mark.parametrize("name", TC.CASES)
def test_device_corridor_equals_host(nat, name):
    """1. A solver at (64, 5, 3) with the case's H and track; the margin once from the
    constructor and once as the argument."""
    c = TC.case(name)
    nlp = _solver(c["track"], 64, 5, 3, c["H"], device_corridor=True, corridor_margin=c["margin"])
    try:
        hp, theta = nlp.track_corridor(c["path"])
        assert hp.shape == (c["H"], 6) and theta.shape == (c["H"],)
        print(f"{name}: max |hp - host| {np.max(np.abs(hp - c['hp'])):.3g} max |theta - host| "
              f"{np.max(np.abs(theta - c['theta'])):.3g}")
        np.testing.assert_allclose(hp, c["hp"], rtol=0, atol=TC.TOL)
        np.testing.assert_allclose(theta, c["theta"], rtol=0, atol=TC.TOL)
        np.testing.assert_array_equal(hp[:, 3:5], -hp[:, 0:2])
        again, _ = nlp.track_corridor(c["path"], margin=c["margin"])
        np.testing.assert_array_equal(again, hp)
        # another margin moves the offsets alone
        wider, th2 = nlp.track_corridor(c["path"], margin=c["margin"] - 0.01)
        np.testing.assert_array_equal(wider[:, [0, 1, 3, 4]], hp[:, [0, 1, 3, 4]])
        np.testing.assert_allclose(wider[:, [2, 5]], hp[:, [2, 5]] + 0.01, rtol=0, atol=TC.TOL)
        np.testing.assert_array_equal(th2, theta)
    finally:
        nlp.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_corridor_solve_equals_given_corridor(nat, shape):
    """2. Ticks 20, 21, 22 (module doc)."""
    from llampc.mpc import constraints
    samples, elite, iters, H = shape
    tr = TC.track("ETHZ")
    A = _solver(tr, samples, elite, iters, H, device_corridor=True, corridor_margin=MARGIN)
    B = _solver(tr, samples, elite, iters, H)
    plain = _solver(tr, samples, elite, iters, H)
    try:
        prev = None
        for tick in (20, 21, 22):
            x0, up, xref = TC.tick_inputs(tick, H)
            path = constraints.default_path(x0, H, TC.TS, prev)
            if prev is None:                 # the first solve: the ray from the car
                v = max(x0[3], 0.05)
                ray = x0[:2] + 3 * TC.TS * v * np.array([np.cos(x0[2]), np.sin(x0[2])])
                np.testing.assert_allclose(path[:, 3], ray, rtol=0, atol=1e-15)
            ua, fa, xa, va = A.solve(x0, xref, up)
            hp = A.last_corridor
            assert hp.shape == (H, 6) and np.all(np.isfinite(hp))
            if tick == 20:                   # non-vacuity, before any comparison
                u0, f0, x0mpc, _ = plain.solve(x0, xref, up)
                s0 = float(np.max(constraints.slacks(hp, x0mpc[:2])))
                print(f"shape {shape}: the unconstrained optimum's slack on the device corridor {s0:.4f}")
                assert s0 > 0.01, s0
                assert not np.array_equal(ua, u0)
            ub, fb, xb, vb = B.solve(x0, xref, up, corridor=hp)
            print(f"shape {shape} tick {tick}: fval {fa!r} max_slack {A.max_slack!r} violation {va}")
            np.testing.assert_array_equal(ua, ub)
            assert fa == fb
            np.testing.assert_array_equal(xa, xb)
            assert A.max_slack == B.max_slack and va == vb
            assert abs(A.max_slack - float(np.max(constraints.slacks(hp, xa[:2])))) <= 1e-12
            built, _ = A.track_corridor(path)
            np.testing.assert_array_equal(built, hp)
            # and that corridor is the host's along the same path
            np.testing.assert_allclose(hp, constraints.track_corridor(tr, path, MARGIN), rtol=0, atol=TC.TOL)
            prev = xa
    finally:
        for s in (A, B, plain):
            s.close()


def test_corridor_path_argument(nat):
    """2b. corridor_path wins over the default path; corridor= wins over both."""
    from llampc.mpc import constraints
    tr = TC.track("ETHZ")
    x0, up, xref = TC.tick_inputs(20, 20)
    A = _solver(tr, 64, 5, 3, 20, device_corridor=True, corridor_margin=MARGIN)
    B = _solver(tr, 64, 5, 3, 20, device_corridor=True, corridor_margin=MARGIN)
    try:
        A.solve(x0, xref, up, corridor_path=xref)
        np.testing.assert_array_equal(A.last_corridor, A.track_corridor(xref)[0])
        np.testing.assert_allclose(A.last_corridor, constraints.track_corridor(tr, xref, MARGIN), rtol=0, atol=TC.TOL)
        given = constraints.disabled(20)
        out = B.solve(x0, xref, up, corridor=given, corridor_path=np.full((2, 21), np.nan))
        assert B.last_corridor is None and B.max_slack == 0.0 and out[3] == 0.0
    finally:
        A.close()
        B.close()


def _raw(nlp):
    nlp._ensure()
    return nlp._h, nlp._io, nlp._addr


def test_refusals(nat):
    """3. No track: LLAMPC_E_STATE.  llampc_nlp_set_track's refusals one by one (none of them sets
    a track).  With a track: a NaN path and margin = track_width / 2 are LLAMPC_E_ARG with nothing
    launched.  A second set_track takes effect."""
    lib = nat.load()
    eth, poly = TC.case("ethz-H20"), TC.case("polygon-64")
    tr = eth["track"]
    x0, up, xref = TC.tick_inputs(20, 20)
    nlp = _solver(tr, 64, 5, 3, 20)
    try:
        h, b, a = _raw(nlp)
        b["x0"][:], b["xref"][:], b["up"][:], b["path"][:] = x0, xref, up, eth["path"]

        def corridor(margin=MARGIN):
            return lib.llampc_nlp_track_corridor(h, a["path"], margin, a["hp"], a["theta"])

        def solve(margin=MARGIN, weight=1e4):
            return lib.llampc_nlp_solve_track(h, a["x0"], a["xref"], a["up"], None, 0, a["path"], margin, weight,
                                              a["umpc"], a["fval"], a["xmpc"], a["slack"], a["hp"])

        def set_track(t, centre=None, theta=None, n=None, L=None, width=None):
            centre = np.ascontiguousarray(t.center_line if centre is None else centre, dtype=np.float64)
            theta = np.ascontiguousarray(t.theta_track if theta is None else theta, dtype=np.float64)
            return lib.llampc_nlp_set_track(h, centre.ctypes.data, theta.ctypes.data,
                                            centre.shape[1] if n is None else n,
                                            float(t.track_length if L is None else L),
                                            float(t.track_width if width is None else width))
        assert corridor() == E_STATE and solve() == E_STATE
        n = tr.center_line.shape[1]
        big = np.zeros((2, 4097))
        nan_c = tr.center_line.copy()
        inf_t, t0, flat = tr.theta_track.copy(), tr.theta_track.copy(), tr.theta_track.copy()
        nan_c[1, n - 1] = np.nan
        inf_t[n - 1] = np.inf
        t0[0] = 1e-9
        flat[5] = flat[4]
        refused = [dict(n=1), dict(centre=big, theta=np.arange(4097.0), n=4097), dict(centre=nan_c), dict(theta=inf_t),
                   dict(theta=t0), dict(theta=flat), dict(L=tr.theta_track[-1]), dict(L=np.nan), dict(L=np.inf),
                   dict(centre=np.array([[0.0, 0.1], [0.0, 0.0]]), theta=np.array([0.0, 0.1]), L=0.2),
                   dict(width=0.0), dict(width=-0.37), dict(width=np.nan)]
        for kw in refused:
            assert set_track(tr, **kw) == E_ARG, kw
            assert corridor() == E_STATE, kw
        assert lib.llampc_nlp_set_track(h, None, None, 5, 1.0, 0.1) == E_ARG

        assert set_track(tr) == 0
        before = nlp._bank.launches
        assert corridor() == 0
        np.testing.assert_allclose(b["hp"], eth["hp"], rtol=0, atol=TC.TOL)
        np.testing.assert_allclose(b["theta"], eth["theta"], rtol=0, atol=TC.TOL)
        assert nlp._bank.launches == before + 1
        # theta may be NULL
        assert lib.llampc_nlp_track_corridor(h, a["path"], MARGIN, a["hp"], None) == 0
        before = nlp._bank.launches
        for margin in (tr.track_width / 2, 1.0, np.nan, np.inf):
            assert corridor(margin) == E_ARG and solve(margin) == E_ARG, margin
        for w in (-1.0, np.nan, np.inf):
            assert solve(weight=w) == E_ARG, w
        for bad in (np.nan, np.inf, -np.inf):
            for at in ((0, 0), (1, 20), (0, 7)):
                b["path"][:] = eth["path"]
                b["path"][at] = bad
                assert corridor() == E_ARG and solve() == E_ARG, (bad, at)
        b["path"][:] = eth["path"]
        assert lib.llampc_nlp_track_corridor(h, None, MARGIN, a["hp"], a["theta"]) == E_ARG
        assert lib.llampc_nlp_track_corridor(h, a["path"], MARGIN, None, a["theta"]) == E_ARG
        assert nlp._bank.launches == before          # nothing was launched
        assert nlp._last is None and solve() == 0    # and the handle still solves: call 0
        np.testing.assert_allclose(b["hp"], eth["hp"], rtol=0, atol=TC.TOL)

        # the second track replaces the first
        assert set_track(poly["track"]) == 0
        b["path"][:] = poly["path"]
        assert corridor(poly["margin"]) == 0
        np.testing.assert_allclose(b["hp"], poly["hp"], rtol=0, atol=TC.TOL)
        np.testing.assert_allclose(b["theta"], poly["theta"], rtol=0, atol=TC.TOL)
        assert corridor(0.2) == E_ARG                # the polygon's half width, not ETHZ's 0.185
    finally:
        nlp.close()


def test_device_corridor_off_is_noop(nat):
    """4. device_corridor=False (spelled out, with a margin that would be refused otherwise)
    against a solver built without the new keywords: solve() and solve(corridor=hp) bitwise, two
    fresh solvers each."""
    from llampc.mpc import constraints
    tr = TC.track("ETHZ")
    x0, up, xref = TC.tick_inputs(20, 20)
    hp = constraints.track_corridor(tr, xref, MARGIN)
    for corridor in (None, hp):
        outs = []
        for kw in ({}, dict(device_corridor=False, corridor_margin=1.0)):
            nlp = _solver(tr, **kw)
            try:
                outs.append((nlp.solve(x0, xref, up, corridor=corridor), nlp.max_slack, nlp.last_corridor))
            finally:
                nlp.close()
        (ua, fa, xa, va), sa, la = outs[0]
        (ub, fb, xb, vb), sb, lb = outs[1]
        np.testing.assert_array_equal(ua, ub)
        assert fa == fb and va == vb and sa == sb and la is None and lb is None
        np.testing.assert_array_equal(xa, xb)

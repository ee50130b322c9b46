"""The look-ahead corridor's host side, no GPU: the reference helper (tests/corridor_ref.py) pinned
to the hand-computed corridors of test_nlp_corridor_cpu.py and to constraints.slacks; the argument
checks ModelBank.lookahead, plan_raw and plan() make before they touch the library; the header's
declarations of the three new entries against their ctypes signatures; and the variant a corridor
launch reports (host only)."""
import os

import numpy as np
import pytest

import corridor_ref as CR
from test_nlp_corridor_cpu import HAND

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the summed squared slacks of HAND's three cases (short binary fractions: exact)
#  box: 0.5^2 + 0.25^2; disabled: 0; oblique: 0.5^2 + 3.5^2 + 0
HAND_PEN = [0.3125, 0.0, 12.5]


def _traj(points, lanes=1):
    """traj [H+1, lanes, 6]: p_0 = (9, 9), then the given positions; the other states 7."""
    rows = np.array([[9.0, 9.0, 7.0, 7.0, 7.0, 7.0]] + [[x, y, 7.0, 7.0, 7.0, 7.0] for x, y in points])
    return np.repeat(rows[:, None, :], lanes, axis=1)


@pytest.mark.parametrize("case,want", list(zip(HAND, HAND_PEN)), ids=["box", "disabled", "oblique"])
def test_penalty_helper_on_hand_computed_corridors(case, want):
    from llampc.mpc import constraints
    hp, points, max_slack = case
    hp = np.array(hp, dtype=float)
    traj = _traj(points, lanes=3)
    pen = CR.penalty(hp, traj)
    assert pen.shape == (3,) and np.all(pen == want)
    s = constraints.slacks(hp, traj[:, 0, :2].T)
    assert float(np.max(s)) == max_slack
    acc = 0.0
    for k in range(len(hp)):                       # ascending k, (s1^2 + s2^2) added per step
        acc = acc + (s[k, 0] * s[k, 0] + s[k, 1] * s[k, 1])
    assert pen[0] == acc


def test_penalty_helper_matches_slacks_on_a_rollout():
    """On an oracle rollout and the matrix's own corridor: the helper is constraints.slacks squared
    and summed in ascending k, bitwise, for every pair; J_c = J + (w pen) with the product rounded
    first; about half of the pairs leave the median strip."""
    from llampc.mpc import constraints
    from oracle import llampc_oracle as O
    from test_lookahead_matrix_gpu import COSTS, bank, realistic_inputs, shared
    x0, uprev, U, xref = realistic_inputs(3, 12, 0.02)
    traj = O.rollout_rk4(shared(), tuple(bank()), x0, U, 0.02)
    hp = CR.median_strip(traj, xref)
    np.testing.assert_array_equal(hp[:, 3:5], -hp[:, 0:2])
    Jc, pen = CR.corridor_cost(traj, U, xref, uprev, *COSTS["default"], hp, 1e4)
    for lane in (0, 7, traj.shape[1] - 1):
        s = constraints.slacks(hp, traj[:, lane, :2].T)
        acc = 0.0
        for k in range(12):
            acc = acc + (s[k, 0] * s[k, 0] + s[k, 1] * s[k, 1])
        assert pen[lane] == acc
    J = O.mpc_cost(traj, U, xref, uprev, *COSTS["default"])
    np.testing.assert_array_equal(Jc, J + 1e4 * pen)
    assert 0.25 <= np.mean(pen > 0) <= 0.75
    # a disabled corridor and a zero weight change nothing
    np.testing.assert_array_equal(CR.corridor_cost(traj, U, xref, uprev, *COSTS["default"], constraints.disabled(12), 1e4)[0], J)
    np.testing.assert_array_equal(CR.corridor_cost(traj, U, xref, uprev, *COSTS["default"], hp, 0.0)[0], J)


def _bank_without_library():
    from llampc.mpc import ModelBank
    b = ModelBank.__new__(ModelBank)
    b.n, b._h = 4, None
    return b


H, C = 12, 3
GOOD = dict(x0=np.zeros(6), U=np.zeros((C, H, 2)), xref=np.zeros((2, H + 1)), uprev=np.zeros(2))


@pytest.mark.parametrize("shape", [(H - 1, 6), (H, 5), (6, H), (6 * H,), (H + 1, 6)])
@pytest.mark.parametrize("entry", ["lookahead", "plan_raw", "plan"])
def test_corridor_shape_is_rejected_before_the_library(entry, shape, monkeypatch):
    _call_expecting_value_error(entry, monkeypatch, "corridor must be", corridor=np.zeros(shape))


@pytest.mark.parametrize("weight", [-1.0, float("nan"), float("inf")])
@pytest.mark.parametrize("entry", ["lookahead", "plan_raw", "plan"])
def test_corridor_weight_is_rejected_before_the_library(entry, weight, monkeypatch):
    _call_expecting_value_error(entry, monkeypatch, "corridor_weight", corridor=np.zeros((H, 6)), corridor_weight=weight)


@pytest.mark.parametrize("entry", ["lookahead", "plan_raw", "plan"])
def test_corridor_with_rk6_is_rejected_before_the_library(entry, monkeypatch):
    _call_expecting_value_error(entry, monkeypatch, "rk6", corridor=np.zeros((H, 6)), integrator="rk6")


@pytest.mark.parametrize("entry", ["plan_raw", "plan"])
def test_corridor_with_raceline_start_is_rejected_before_the_library(entry, monkeypatch):
    _call_expecting_value_error(entry, monkeypatch, "raceline_start", corridor=np.zeros((H, 6)),
                                raceline_start=(0.0, 1.0, 1.0))


def _call_expecting_value_error(entry, monkeypatch, match, **kw):
    from llampc import _native
    from llampc.mpc import plan
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("the library was touched"))
    b = _bank_without_library()
    g = GOOD
    with pytest.raises(ValueError, match=match):
        if entry == "lookahead":
            b.lookahead(g["x0"], g["U"], g["xref"], g["uprev"], **kw)
        elif entry == "plan_raw":
            b.plan_raw(np.zeros(6), np.zeros(2), g["x0"], g["U"], g["xref"], g["uprev"], **kw)
        else:
            plan(b, g["x0"], np.zeros(2), np.zeros(6), g["xref"], g["U"], **kw)


def test_keywords_default_to_no_corridor():
    import inspect
    from llampc.mpc import ModelBank, plan
    for fn in (ModelBank.lookahead, ModelBank.plan_raw, plan):
        p = inspect.signature(fn).parameters
        assert p["corridor"].default is None and p["corridor_weight"].default == 1e4, fn


@pytest.mark.parametrize("name,count", [("llampc_lookahead_corridor", 17), ("llampc_plan_corridor", 8),
                                        ("llampc_plan_variant_corridor", 6)])
def test_header_declares_the_corridor_entries(name, count):
    """The C header's declaration and the ctypes signature carry the same arguments; each comment
    cites the entry it extends."""
    from llampc import _native
    src = open(os.path.join(REPO, "include", "llampc.h")).read()
    at = src.index(f"int {name}(")
    decl = src[at:]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == count == len(_native._SIGNATURES[name][1])
    comment = src[src.rindex("/*", 0, at):at]
    assert name.replace("_corridor", "") in comment
    assert "#define LLAMPC_ABI_VERSION 1\n" in src            # additions only


def test_corridor_variant_counts_the_corridor_lds(monkeypatch):
    """Host only: the corridor's 48 H bytes move (31, 64) from staged to unstaged; the lanes per
    rollout, G and cpl are the plain launch's; RK6 is refused."""
    from llampc import _native
    monkeypatch.delenv("LLAMPC_LPM", raising=False)
    for integ in ("rk4", "euler_nlp"):
        for shape in [(3, 12), (64, 40), (130, 20), (5, 1), (2, 64), (31, 64), (1, 20)]:
            for n in (97, 10000):
                v, vc = _native.plan_variant(n, *shape, integ), _native.plan_variant_corridor(n, *shape, integ)
                assert {k: v[k] for k in ("lpm", "G", "cpl")} == {k: vc[k] for k in ("lpm", "G", "cpl")}
                assert vc["stage"] == (v["stage"] and shape != (31, 64)), (integ, shape, v, vc)
    assert _native.plan_variant(97, 31, 64)["stage"]
    with pytest.raises(_native.NativeError) as e:
        _native.plan_variant_corridor(97, 3, 12, "rk6")
    assert e.value.code == _native.E_ARG

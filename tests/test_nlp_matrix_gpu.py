"""setupNLP.solve's unconstrained device search (csrc/nlp.hip, llampc_nlp_*) over the values it
chooses its code paths from — selection shapes, horizons, cost matrices, bounds, rates, time step,
sampler parameters, launch modes, the result's owner and the failure contract — against its NumPy
restatement oracle.nlp_cem.  The cases and their inputs are tests/nlp_matrix.py's; the conditions
that keep a case from passing vacuously or from failing on a rank flip are asserted on the
restatement alone in test_nlp_matrix_cpu.py (and again here, before every comparison).

Every solve of a-f, h and one leg of g is compared two ways (``check_solve``):

  1. against the restatement: ``umpc`` bitwise (the samples are bitwise the restatement's; the
     ranking follows costs that agree far more tightly than the smallest elite gap, GAP_MIN = 1e-9)
     and ``fval`` at RTOL_ROLL = 1e-7;
  2. independently of it: ``xmpc`` is O.rollout_euler_nlp of the returned ``umpc`` (RTOL_STEP x 10
     = 1e-8, atol 1e-12), ``fval`` is O.mpc_cost of that trajectory with the case's own Q, R, P
     (RTOL_ROLL), and ``umpc`` is inside the case's bounds (exactly: they are clip results) and
     rates (the restatement's RATE_TOL).

Measured on the MI355X over the 62 compared solves of this module: the largest relative
|fval_device - fval_restated| is 1.09e-15 (terminal-only, fval 0.1526; next 4.3e-16 at
(4096, 32, 2, 64) and 4.2e-16 at the full matrices, H = 20; most solves 0) — MEASURED_FVAL_DEV
below.  That is six orders under GAP_MIN = 1e-9 and under the 1e-11 above which the gap bound would
have to become 100 x the figure, so GAP_MIN stays (every solve prints its own figure, -s).

Ties (f): with Q = P = R = 0 every objective is exactly 0 on both sides, so the index alone ranks.
The result shows the overall winner (round 0's sample 0, across every block's merged list: ``umpc``
= uprev held, ``fval`` = 0); the later rounds' elites (samples 0 .. E - 1) do not reach the result,
since no later round can be strictly better — they are pinned on the restatement
(test_nlp_matrix_cpu.py) and run here for three rounds without a visible effect.

Failure contract (i): the infeasible-uprev solver's bounds are fixed at create, so the feasible
solve that follows it takes uprev[1] = 0.05 (tick 20's own 0.279 would fail again); the one after
the NaN state takes tick 20's plain inputs."""
import numpy as np
import pytest

import nlp_matrix as M
from oracle import llampc_oracle as O

pytestmark = pytest.mark.gpu

RTOL_STEP = 1e-9
RTOL_ROLL = 1e-7
# the largest relative |fval_device - fval_restated| over every compared solve of this module
MEASURED_FVAL_DEV = 1.09e-15


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


def check_independent(case, ref, out):
    """2. xmpc, fval and the constraints from the returned umpc alone."""
    umpc, fval, xmpc, viol = out
    H = case.H
    assert umpc.shape == (2, H) and xmpc.shape == (6, H + 1) and viol == 0.0
    bank6 = tuple(np.array([v]) for v in M._env()[2])
    U = np.ascontiguousarray(umpc.T)[None]
    traj = O.rollout_euler_nlp(M.shared(), bank6, ref["x0"], U, case.Ts)
    np.testing.assert_allclose(xmpc, traj[:, 0, :].T, rtol=RTOL_STEP * 10, atol=1e-12)
    np.testing.assert_allclose(fval, O.mpc_cost(traj, U, ref["xref"], ref["up"], case.Q, case.R, case.P)[0],
                               rtol=RTOL_ROLL)
    assert np.all(umpc >= np.array(case.umin)[:, None]) and np.all(umpc <= np.array(case.umax)[:, None])
    for j, m in enumerate(case.rate_m()):
        if m is not None:
            dd = np.diff(np.concatenate([ref["up"][j:j + 1], umpc[j]]))
            assert np.all(np.abs(dd) <= m * case.Ts * (1.0 + O.RATE_TOL)), (j, np.max(np.abs(dd)))


def check_solve(case, ref, out, tag=""):
    umpc, fval, xmpc, _ = out
    dev = abs(fval - ref["j"]) / abs(ref["j"]) if ref["j"] else abs(fval)
    print(f"FVAL_DEV {case.name}{tag}: device {fval!r} restated {ref['j']!r} relative {dev:.3g} "
          f"umpc equal {np.array_equal(umpc.T, ref['u'])}")
    np.testing.assert_array_equal(umpc.T, ref["u"])
    np.testing.assert_allclose(fval, ref["j"], rtol=RTOL_ROLL)
    check_independent(case, ref, out)


@pytest.mark.parametrize("case", M.SINGLE, ids=repr)
def test_solve_equals_restatement(nat, case):
    """a-e, h: one first solve per case."""
    ref = M.restate(case)
    M.check_conditions(case, ref)
    nlp = M.solver(case)
    try:
        check_solve(case, ref, nlp.solve(ref["x0"], ref["xref"], ref["up"]))
    finally:
        nlp.close()


def test_oversized_search_is_refused(nat):
    """a: (4096, 64, 2, 64) needs 230 KiB of LDS: LLAMPC_E_ARG at create, nothing launched."""
    nlp = M.solver(M.Case("refused", M.REFUSED_SHAPE))
    x0, up, xref = M.inputs(M.Case("refused-in", M.REFUSED_SHAPE))
    try:
        with pytest.raises(nat.NativeError, match="llampc error -1.*LDS") as e:
            nlp.solve(x0, xref, up)
        assert e.value.code == nat.E_ARG and nlp._h is None
        assert nlp._bank.launches == 0
    finally:
        nlp.close()


def test_asymmetric_rates_solve_the_tighter_side(nat):
    """d: min / max rates (-3, +5) rad/s.  The chain clips to the +-3 the feasibility test uses, so
    the solve is the +-3 solve bitwise and equals the restatement, which counts 1,024 finite
    objectives in every round.  (With the chain at [-3, +5] Ts every sample it left beyond 3 Ts was
    scored +inf: 1 finite objective of 1,024 in round 0, another umpc and a worse fval.)"""
    ra, rs = M.restate(M.ASYM), M.restate(M.SYM3)
    assert ra["info"]["finite"] == [1024] * 8
    outs = []
    for case, ref in ((M.ASYM, ra), (M.SYM3, rs)):
        nlp = M.solver(case)
        try:
            outs.append(nlp.solve(ref["x0"], ref["xref"], ref["up"]))
        finally:
            nlp.close()
    a, s = outs
    print(f"asymmetric fval {a[1]!r} symmetric {s[1]!r} restated {ra['j']!r}")
    np.testing.assert_array_equal(a[0], s[0])
    assert a[1] == s[1]
    np.testing.assert_array_equal(a[2], s[2])
    check_solve(M.ASYM, ra, a)


@pytest.mark.parametrize("case", M.TIES, ids=repr)
def test_ties_go_to_the_lower_index(nat, case):
    """f: every objective exactly 0; the winner over all blocks' lists is round 0's sample 0."""
    ref = M.restate(case)
    M.check_conditions(case, ref)
    assert ref["info"]["best_round"] == 0 and ref["info"]["best_sample"] == 0
    nlp = M.solver(case)
    try:
        out = nlp.solve(ref["x0"], ref["xref"], ref["up"])
    finally:
        nlp.close()
    assert out[1] == 0.0
    np.testing.assert_array_equal(out[0].T, np.tile(ref["up"], (case.H, 1)))
    check_solve(case, ref, out)


def _chain(case, refs=None):
    """Three warm-started solves at MODE_TICKS on one solver; refs: compared with the restatement."""
    nlp = M.solver(case)
    try:
        got = []
        for call, t in enumerate(M.MODE_TICKS):
            x0, up, xref = M.inputs(case, t)
            out = nlp.solve(x0, xref, up)
            if refs is not None:
                check_solve(case, refs[call], out, f" call {call}")
            got.append(out)
        return got
    finally:
        nlp.close()


@pytest.mark.parametrize("env,exact", [("LLAMPC_NLP_ROUND_LAUNCHES", True), ("LLAMPC_NLP_RERUN_TRAJ", False)],
                         ids=["round-launches", "rerun-traj"])
@pytest.mark.parametrize("shape", M.MODE_SHAPES, ids=M._sid)
def test_modes_agree(nat, monkeypatch, shape, env, exact):
    """g: every round in one launch against one launch per round (the best so far and the mean /
    std carried across launches), and the kept states against the re-run trajectory, at a
    length-64 unstaged shape, a multi-level nlp_complete32 shape and the last horizon that keeps its
    states: umpc and fval bitwise, xmpc bitwise (round launches) or to 1e-12 (re-run), over three
    warm-started solves; the default leg also against the restatement with call = 0, 1, 2."""
    case = M.Case("mode-" + M._sid(shape), shape)
    refs = M.restate_chain(case)
    for ref in refs:
        M.check_conditions(case, ref)
    monkeypatch.setenv(env, "0")
    base = _chain(case, refs)
    monkeypatch.setenv(env, "1")
    other = _chain(case)
    for a, b in zip(base, other):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]
        if exact:
            np.testing.assert_array_equal(a[2], b[2])
        else:
            np.testing.assert_allclose(a[2], b[2], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("case,best_round", M.OWNER, ids=lambda v: repr(v))
def test_result_owner(nat, monkeypatch, case, best_round):
    """h: on a shape that keeps its states, a best from the last round is written by its sample's
    own block from LDS, an earlier round's by block 0 re-running it (nlp_owner's two branches):
    both equal the restatement, and the re-run-always mode bitwise in umpc / fval, 1e-12 in xmpc."""
    ref = M.restate(case)
    M.check_conditions(case, ref)
    assert ref["info"]["best_round"] == best_round
    outs = []
    for rerun in ("0", "1"):
        monkeypatch.setenv("LLAMPC_NLP_RERUN_TRAJ", rerun)
        nlp = M.solver(case)
        try:
            outs.append(nlp.solve(ref["x0"], ref["xref"], ref["up"]))
        finally:
            nlp.close()
        check_solve(case, ref, outs[-1], f" rerun {rerun}")
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1]
    np.testing.assert_allclose(outs[0][2], outs[1][2], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("case", M.FAILURES, ids=repr)
def test_no_finite_objective(nat, case):
    """i: no finite objective in any round (every sample infeasible; a NaN state): solve raises
    LLAMPC_E_DEVICE with the "no finite objective" message, the result buffers hold zeros and
    +inf, the warm start is not updated; the solver's next solve is call 1 without a warm start
    and equals the restatement."""
    ref = M.restate(case)
    M.check_conditions(case, ref)
    assert ref["u"] is None and ref["j"] == np.inf
    after = M.AFTER_FAILURE[case.name]
    ref2 = M.restate(after, call=1)
    M.check_conditions(after, ref2)
    nlp = M.solver(case)
    try:
        with pytest.raises(nat.NativeError, match="no finite objective") as e:
            nlp.solve(ref["x0"], ref["xref"], ref["up"])
        assert e.value.code == nat.E_DEVICE
        assert nlp._last is None
        assert np.all(nlp._io["umpc"] == 0.0) and nlp._io["fval"][0] == np.inf
        check_solve(after, ref2, nlp.solve(ref2["x0"], ref2["xref"], ref2["up"]), " after the failure")
    finally:
        nlp.close()

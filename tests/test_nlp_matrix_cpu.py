"""The conditions of the setupNLP.solve parity matrix (tests/nlp_matrix.py), on the restatement
alone (oracle.nlp_cem with its ``info``), no GPU: what keeps every case of
test_nlp_matrix_gpu.py from passing vacuously or from failing on a rank flip.

  * the smallest relative gap between adjacent costs among every round's first elite + 1 finite
    ones is above GAP_MIN = 1e-9 (pairs with bitwise identical sequences skipped: their costs are
    identical on the device too) — the bitwise ``umpc`` comparison then cannot hang on costs the
    device and the restatement order differently.  Exempt: the tie cases (every cost exactly 0 on
    both sides, the index alone decides — that is what they test) and the failure cases (nothing
    finite);
  * the finite objectives per round: every sample, or none (the failure contract's triggers);
  * where a case claims active clipping, round 0's share of clipped values is at least 0.3;
  * the result owner's cases take their best from the last round and from round 0;
  * the full cost matrices move fval by more than 1e-3 relative against their diagonal parts
    (and the terminal term against none), so a dropped element cannot pass at RTOL_ROLL.

Also here: setupNLP hands the rate chain and the feasibility test one symmetric bound (host code),
and nlp_cem's defaults are bitwise what they were (a committed value)."""
import numpy as np
import pytest

import nlp_matrix as M
from oracle import llampc_oracle as O


@pytest.mark.parametrize("case", M.SINGLE + M.TIES + M.FAILURES, ids=repr)
def test_conditions(case):
    M.check_conditions(case, M.restate(case))


@pytest.mark.parametrize("shape", M.MODE_SHAPES, ids=M._sid)
def test_conditions_warm_started(shape):
    """g: the three warm-started solves (call 0, 1, 2; the held uprev in round 0 from call 1)."""
    case = M.Case("mode-" + M._sid(shape), shape)
    for ref in M.restate_chain(case):
        M.check_conditions(case, ref)


@pytest.mark.parametrize("case", M.AFTER_FAILURE.values(), ids=repr)
def test_conditions_after_failure(case):
    """i: the solve after a failed one is call 1 without a warm start."""
    M.check_conditions(case, M.restate(case, call=1))


@pytest.mark.parametrize("case,best_round", M.OWNER, ids=lambda v: repr(v))
def test_owner_rounds(case, best_round):
    """h: both branches of the kernel's nlp_owner need a best from the last round and one from
    an earlier round, on a shape that keeps its states (H <= 22)."""
    assert case.H <= 22 and case.shape[2] == 8
    assert M.restate(case)["info"]["best_round"] == best_round


@pytest.mark.parametrize("case", M.COST, ids=repr)
def test_cost_matrices_matter(case):
    """c: the restatement's optimum scored with the diagonal parts alone (full matrices), or
    without the terminal term (terminal only), differs by more than 1e-3 relative."""
    ref = M.restate(case)
    bank6 = tuple(np.array([v]) for v in M._env()[2])
    U = ref["u"][None]
    traj = O.rollout_euler_nlp(M.shared(), bank6, ref["x0"], U, case.Ts)
    full = O.mpc_cost(traj, U, ref["xref"], ref["up"], case.Q, case.R, case.P)[0]
    assert full == ref["j"]
    dg = lambda m: np.diag(np.diag(m))
    if np.any(case.Q):
        less = O.mpc_cost(traj, U, ref["xref"], ref["up"], dg(case.Q), dg(case.R), dg(case.P))[0]
    else:
        less = O.mpc_cost(traj, U, ref["xref"], ref["up"], case.Q, case.R, M.ZERO)[0]
    print(f"{case.name}: fval {full!r} reduced {less!r} relative {abs(full - less) / abs(full):.3g}")
    assert abs(full - less) > 1e-3 * abs(full)


def test_ties_restated():
    """f: with Q = P = R = 0 the best is round 0's sample 0 = uprev held, and every round's elite
    is samples 0 .. elite - 1 (the next mean their mean)."""
    for case in M.TIES:
        ref = M.restate(case)
        info = ref["info"]
        assert ref["j"] == 0.0 and info["best_round"] == 0 and info["best_sample"] == 0
        np.testing.assert_array_equal(ref["u"], np.tile(ref["up"], (case.H, 1)))
        for el in info["elite"]:
            np.testing.assert_array_equal(el, np.arange(case.shape[1]))


def test_uprev_outside_restated():
    """d: uprev[1] = 0.279 above umax[1] = 0.2 by less than one rate step (0.1): the chain brings
    u_0[1] to the bound and every sample stays feasible."""
    ref = M.restate(next(c for c in M.BOUNDS if c.name == "uprev-outside"))
    assert 0.2 < ref["up"][1] < 0.3 and ref["u"][0, 1] == 0.2


def test_asymmetric_rates_restated():
    """d: (-3, +5) rad/s is restated as the +-3 solve: all samples feasible in every round."""
    a, s = M.restate(M.ASYM), M.restate(M.SYM3)
    assert a["info"]["finite"] == [1024] * 8
    np.testing.assert_array_equal(a["u"], s["u"])
    assert a["j"] == s["j"]


@pytest.mark.parametrize("lo,hi,m", [(-3.0, 5.0, 3.0), (-5.0, 3.0, 3.0), (-5.0, 5.0, 5.0), (-2.0, 2.0, 2.0)])
@pytest.mark.parametrize("Ts", [0.02, 0.05])
def test_setupnlp_one_symmetric_rate_bound(lo, hi, m, Ts):
    """setupNLP's rate chain clips to the bound its feasibility test uses: [-m, +m] Ts with
    m = min(-lo, hi), on either input; None stays "no bound"."""
    case = M.Case("rates", Ts=Ts, min_rates=(None, lo), max_rates=(None, hi))
    nlp = M.solver(case)
    assert nlp.rate == [(None, None), (-m * Ts, m * Ts)]
    assert tuple(nlp.cost.rate_max) == (-1.0, m)
    nlp = M.solver(M.Case("rates0", Ts=Ts, min_rates=(lo, None), max_rates=(hi, None)))
    assert nlp.rate == [(-m * Ts, m * Ts), (None, None)]
    assert tuple(nlp.cost.rate_max) == (m, -1.0)


def test_setupnlp_rejects_inverted_rates():
    with pytest.raises(ValueError, match="min_rates"):
        M.solver(M.Case("bad", min_rates=(None, 1.0), max_rates=(None, 5.0)))


def test_nlp_cem_defaults_unchanged():
    """The restatement's existing callers: the default call returns what it returned before
    ``rate_max_pwm`` and ``info`` existed (fval at DYN-slice tick 20, read on the parent commit),
    and filling ``info`` does not change the result."""
    c = M.Case("default")
    x0, up, xref = M.inputs(c)
    u, j = O.nlp_cem(M.shared(), M._env()[2], x0, xref, up, None, False, 20, 0.02)
    assert j == 18.92304556554456
    ref = M.restate(c)
    np.testing.assert_array_equal(u, ref["u"])
    assert j == ref["j"]

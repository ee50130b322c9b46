"""The fused control step's conditions, on the oracle chain alone (tests/ctl_solve_cases.py): what the
device comparison of test_ctl_solve_gpu.py rests on.  Printed per row and tick, then asserted:

  * every compared solve has every sample finite in every round — except on nan-selected's failing
    ticks, where none is and the chain commits nothing;
  * its smallest adjacent elite-cost gap is above CHAIN_GAP_MIN = 1e-7 (the bitwise umpc comparison
    cannot hang on a rank flip: the device's xref is the oracle's to 1e-10 only);
  * ctl_matrix.tick_gaps stay above GAP_COST / GAP_MEAN (the tick's exact indices);
  * fval <= J0, the NLP objective of the tick's chosen sequence (sample 0 of round 0 is that sequence);
  * the rows cross what they claim: warm and selected ticks, a changing model, the call word on mixed.

And the reference of llampc_ctl_set_applied: the oracle with overridden u_prev / u_seq differs from
the plain loop where it must (the next look-back's window means), and not before."""
import numpy as np
import pytest

import ctl_matrix as CM
import ctl_solve_cases as SC


@pytest.mark.parametrize("srow", SC.ROWS, ids=repr)
def test_chain_conditions(srow):
    steps = SC.chain(srow)
    assert len(steps) == srow.row.ticks
    for t, step in enumerate(steps):
        SC.check_conditions(srow, t, step)
    # the plain ticks have no solve, and the call word counts the solves
    calls = [s["sol"]["call"] for s in steps if s["sol"] is not None]
    assert calls == list(range(len(calls)))
    assert [t for t, s in enumerate(steps) if s["sol"] is None] == list(srow.plain)
    warm = [s["o"]["warm"] for s in steps]
    assert warm[:srow.row.W + 1] == [True] * (srow.row.W + 1) and not any(warm[srow.row.W + 1:])


def test_base_crosses_models():
    """base: warm -> selected, and the selection changes at least twice after the warm-up."""
    models = [int(s["o"]["best_model"]) for s in SC.chain(SC.BY_NAME["base"]) if not s["o"]["warm"]]
    print("base: selected models", models)
    assert len(set(models)) >= 2, models


def test_committed_solutions_are_applied():
    """A committed solve's first input drives the plant and the next tick's du_0; an uncommitted one
    leaves the tick's candidate."""
    for srow in SC.ROWS:
        steps = SC.chain(srow)
        for t in range(len(steps) - 1):
            sol, nxt = steps[t]["sol"], steps[t + 1]["o"]
            want = sol["u"][0] if sol is not None and sol["u"] is not None else steps[t]["o"]["u_seq"][:, 0]
            np.testing.assert_array_equal(steps[t]["u0"], want)
            np.testing.assert_array_equal(nxt["uprev"], want, err_msg=f"{srow.name} tick {t + 1}")


def test_nan_selected_fails_from_tick_3():
    srow = SC.BY_NAME["nan-selected"]
    steps = SC.chain(srow)
    for t, s in enumerate(steps):
        assert (s["sol"]["u"] is None) == (t >= srow.fail_from), t
        if t >= srow.fail_from:
            assert int(s["o"]["best_model"]) == 0 and np.isnan(CM.bank(srow.row)[2, 0])
    # the warm ticks are base's: the same bank but for the NaN columns, the nominal model solved
    base = SC.chain(SC.BY_NAME["base"])
    for t in range(srow.row.W + 1):
        np.testing.assert_array_equal(steps[t]["sol"]["u"], base[t]["sol"]["u"])


def test_mixed_call_word():
    """mixed: the solve after the plain tick 4 draws call 4's noise, not call 5's, and differs from
    base from tick 4 on (tick 4's candidate was applied)."""
    steps, base = SC.chain(SC.BY_NAME["mixed"]), SC.chain(SC.BY_NAME["base"])
    assert steps[4]["sol"] is None and steps[5]["sol"]["call"] == 4 and base[5]["sol"]["call"] == 5
    for t in range(4):
        np.testing.assert_array_equal(steps[t]["sol"]["u"], base[t]["sol"]["u"])
    assert not np.array_equal(steps[5]["o"]["uprev"], base[5]["o"]["uprev"])


def test_set_applied_reference():
    """The overridden oracle (ctl_solve_cases.chain(applied=...)): u_prev and u_seq row 0 replaced by
    the applied input.  Against the plain loop driven by the same states it must differ in the window
    means of tick 3 (the first full window: transitions under the applied inputs), and every tick's
    du_0 reference is the applied input."""
    srow = SC.BY_NAME["base"]
    row = srow.row
    over = SC.chain(srow, applied=SC.offset_applied(srow))
    for t in range(1, len(over)):
        np.testing.assert_array_equal(over[t]["o"]["uprev"], over[t - 1]["u0"])
        assert not np.array_equal(over[t - 1]["u0"], over[t - 1]["o"]["u_seq"][:, 0])
    # the control: a plain oracle ticked with the overridden loop's states, never told what was applied
    orc = CM.oracle_for(row)
    with np.errstate(all="ignore"):
        plain = [orc.tick(s["x"]) for s in over[:4]]
    wm_over, wm_plain = over[3]["o"]["window_means"], plain[3]["window_means"]
    rel = np.nanmax(np.abs(wm_over - wm_plain) / np.abs(wm_over))
    print(f"set_applied: window means at tick 3 differ by up to {rel:.3g} relative")
    assert rel > 1e3 * CM.RTOL_MEAN
    for t, s in enumerate(over):
        gc, gf, gm = CM.tick_gaps(row, s["o"])
        print(f"set_applied tick {t}: gaps cand {gc:.3g} flat {gf:.3g} mean {gm:.3g}")
        assert gc > CM.GAP_COST and gf > CM.GAP_COST and gm > CM.GAP_MEAN, (t, gc, gf, gm)

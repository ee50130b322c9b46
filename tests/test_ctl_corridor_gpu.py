"""The controller tick's soft track corridor on the device (LLAMPC(corridor_weight=...), csrc/ctl_corr.hip)
against ctl_corridor_cases.CorridorOracle.  Per row the loop runs interleaved — device tick, corridor(),
oracle tick on the device's hp, check, plant step — so the oracle's costs do not inherit the 1e-12 between
the device's half-planes and constraints.track_corridor; ctl_corridor_cases.check_tick holds the corridor
(valid, path 1e-6, hp 1e-12, the disabled rows bitwise), the whole record (ctl_matrix.check_tick's
tolerances) and every rolled-out cost (corridor_costs(): the record carries each slot's best alone), at
most BOUND_SHARE_MAX of all those cost pairs by their core-error bound.  One launch per tick.
Then: armed ticks equal launched ones bitwise; weight 0 mid-run gives the plain controller's records
bitwise; switching on again starts with the disabled corridor; the refusals.

Measured on the MI355X: on every row none of the compared cost pairs (873 to 20 913 per row: the record's
113 and every rolled-out cost) needed its core-error bound (all within RTOL_ROLL); 13 ticks with a valid
path per row, 5 on ethz-nan."""
import numpy as np
import pytest

import ctl_corridor_cases as CC
import ctl_matrix as M
from oracle import llampc_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


def _words(res, H):
    from test_ctl_gpu import _ctl_words
    return _ctl_words(res.raw, H)


@pytest.mark.parametrize("row", CC.ROWS, ids=repr)
def test_row_vs_oracle(row, nat):
    from llampc.mpc import ModelBank
    got = CC.variant(row)
    assert got["s4"] == 0 and got["nb_cor"] == row.H, got
    assert all(got[f] == v for f, v in row.variant.items()), (row.name, got)
    orc = CC.oracle_for(row)
    plant = O.Vehicle.from_params(O.orca_params())
    x = M.start_state(row)
    counts = dict(pairs=0, bound=0)
    valid_ticks = 0
    with ModelBank(np.array(M.bank(row)), W=row.W, device=0) as b, CC.controller(row, b) as ctl:
        projidx = 0
        for t in range(row.ticks):
            l0 = b.launches
            res = ctl.tick(x)
            assert b.launches - l0 == 1, (row.name, t)
            cor = ctl.corridor()
            o = orc.tick(x, hp=cor[1])
            xref, U = ctl.inputs()
            CC.check_tick(row, t, o, x, res, xref, U, projidx, counts, cor, ctl.corridor_costs())
            valid_ticks += int(cor[3])
            projidx = res.raw.projidx
            x = CC.plant_step(row, plant, x, o)
    share = counts["bound"] / max(counts["pairs"], 1)
    print(f"{row.name}: {counts['bound']} of {counts['pairs']} cost pairs passed by the core-error bound ({share:.3f}); "
          f"{valid_ticks} ticks with a valid path")
    assert valid_ticks == CC.TABLE[row.name][2]
    assert share <= M.BOUND_SHARE_MAX, (row.name, counts)


def _run_states(row, prelaunch, read_at=(6, 13)):
    """The row ticked with the oracle loop's states: every record's words, and the corridor read back
    at the ticks read_at only (the read-back cancels an armed launch: the tick after it is launched)."""
    from llampc.mpc import ModelBank
    _, xs = CC.reference(row)
    words, cors = [], {}
    with ModelBank(np.array(M.bank(row)), W=row.W, device=0) as b, CC.controller(row, b, prelaunch=prelaunch) as ctl:
        for t, x in enumerate(xs):
            l0 = b.launches
            res = ctl.tick(x)
            assert b.launches - l0 == 1, (row.name, t)
            words.append(_words(res, row.H))
            if t in read_at:
                cors[t] = ctl.corridor()
    return words, cors


@pytest.mark.parametrize("row", CC.ARMED, ids=repr)
def test_armed_equals_launched(row, nat):
    from test_ctl_gpu import _same_words
    wl, cl = _run_states(row, False)
    wa, ca = _run_states(row, True)
    for a, c in zip(wl, wa):
        _same_words(a, c)
    assert sorted(cl) == sorted(ca)
    for t in cl:
        assert cl[t][3] == ca[t][3]
        for a, c in zip(cl[t][:3], ca[t][:3]):
            assert np.asarray(a).tobytes() == np.asarray(c).tobytes(), (row.name, t)


def test_off_mid_run_then_on_again(nat):
    """mobil-wide (no candidate penalised, so the corridor controller's choices and state are the plain
    one's): corridor ticks 0..6, weight 0 from tick 7, on again from tick 10.  Ticks 7..9 equal a
    controller that never had a corridor bitwise; before, the choices agree (the costs differ in their
    last bits: unsplit against split rollouts); tick 10 runs on the disabled corridor, tick 11 on a path."""
    from llampc.mpc import ModelBank, constraints
    from test_ctl_gpu import _same_words
    row = CC.BY_NAME["mobil-wide"]
    _, xs = CC.reference(row)
    bank = np.array(M.bank(row))
    with ModelBank(bank, W=row.W, device=0) as ba, CC.controller(row, ba) as a, \
            ModelBank(bank, W=row.W, device=0) as bb, CC.controller(row, bb, corridor=False) as p:
        for t, x in enumerate(xs[:12]):
            if t == 7:
                a.set_corridor(0.0)
            if t == 10:
                a.set_corridor(row.weight, CC.margin(row))
            la, lp = ba.launches, bb.launches
            ra, rp = a.tick(x), p.tick(x)
            assert (ba.launches - la, bb.launches - lp) == (1, 1)
            if 7 <= t < 10:
                _same_words(_words(ra, row.H), _words(rp, row.H))
                with pytest.raises(nat.NativeError):
                    a.corridor()
            else:
                assert (ra.best_model, ra.best_cand) == (rp.best_model, rp.best_cand), t
                np.testing.assert_array_equal(ra.u_seq, rp.u_seq)
                _, hp, _, valid = a.corridor()
                assert valid == (t not in (0, 10)), t
                if not valid:
                    assert hp.tobytes() == constraints.disabled(row.H).tobytes()


def test_refusals(nat):
    """No track, a bad weight or margin, a sharded controller: each its error code, nothing enqueued."""
    from llampc.mpc import ModelBank, constraints
    row = CC.BY_NAME["ethz-c8"]
    tr, _ = M.tracks(row.track)
    lib = nat.load()
    x = M.start_state(row)

    with ModelBank(np.array(M.bank(row)), W=row.W, device=0) as b, CC.controller(row, b, corridor=False) as ctl, \
            CC.controller(row, b, corridor=False) as ctl2:
        h, h2 = ctl._ctl._h, ctl2._ctl._h
        ctl.tick(x)
        l0 = b.launches
        assert lib.llampc_ctl_set_corridor(h, 1.0, 0.0) == nat.E_STATE           # no track
        centre, theta, length, width = constraints.track_tables(tr)
        bad = theta.copy()
        bad[3] = bad[2]
        assert lib.llampc_ctl_set_track(h, centre.ctypes.data, bad.ctypes.data, centre.shape[1], length,
                    width) == nat.E_ARG                                                # llampc_nlp_set_track's checks
        assert lib.llampc_ctl_set_track(h, centre.ctypes.data, theta.ctypes.data, centre.shape[1], length, width) == 0
        for w, m in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.0, width / 2), (1.0, float("nan")),
                     (1.0, float("inf"))):
            assert lib.llampc_ctl_set_corridor(h, w, m) == nat.E_ARG, (w, m)
        # a sharded controller refuses the corridor, and a corridor controller the sharding
        g = np.ascontiguousarray(M.bank(row))
        assert lib.llampc_ctl_set_track(h2, centre.ctypes.data, theta.ctypes.data, centre.shape[1], length, width) == 0
        assert lib.llampc_ctl_set_gather(h2, 1, 0, None, nat.dptr(g), g.shape[1]) == 0
        assert lib.llampc_ctl_set_corridor(h2, 1.0, 0.0) == nat.E_STATE
        assert b.launches == l0
    with ModelBank(np.array(M.bank(row)), W=row.W, device=0) as b, CC.controller(row, b) as ctl:
        l0 = b.launches
        g = np.ascontiguousarray(M.bank(row))
        assert lib.llampc_ctl_set_gather(ctl._ctl._h, 1, 0, None, nat.dptr(g), g.shape[1]) == nat.E_STATE
        assert b.launches == l0
        ctl.tick(x)                                   # still a working corridor controller
        assert ctl.corridor()[3] is False

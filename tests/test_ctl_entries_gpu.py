"""Every route to a controller tick's record gives the same bytes (csrc/capi_ctl*.hip over capi_host.hpp's
ctl_tick_prepare / ctl_tick_commit): llampc_ctl_tick against tick_async + wait, armed and rung against
launched, after refused calls, the host-carried gather at world 1 (shard_record, resume, wait) against the
unsharded controller, and the corridor switched on, off and on again with llampc_ctl_corridor's read-back
equal between an armed and a launched run.  N = 64, C = 2, H = 4, W = 3, K = 2 over seven ticks: tick 0
and 1 without a look-back, ticks up to 3 warm, the window full from tick 4, mu-hat used from tick 5.  The
states are one closed loop's (the blocking controller with the RK6 plant), computed once.  No armed launch
is slept into staleness: the fire rule is tests/test_capi_native.py's."""
import numpy as np
import pytest

from oracle import llampc_oracle as O
from test_ctl_gpu import TS, _ctl_words, _same_words, start_state, tracks

pytestmark = pytest.mark.gpu

N, C, H, W, K, T = 64, 2, 4, 3, 2, 7


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


@pytest.fixture(scope="module")
def setup(nat):
    from llampc.mpc import generate_bank
    from llampc.params import ORCA
    tr, _ = tracks("ETHZ")
    return dict(tr=tr, params=generate_bank(N, seed=3), nominal=[ORCA()[k] for k in ("Bf", "Cf", "Df", "Br", "Cr", "Dr")],
                x0=start_state("ETHZ", tr))


class Run:
    """A bank and its controller for one route."""

    def __init__(self, setup, **kw):
        from llampc.mpc import DeviceController, ModelBank
        self.bank = ModelBank(setup["params"], W=W, device=0)
        try:
            self.ctl = DeviceController(self.bank, setup["tr"], H=H, C=C, K=K, nominal6=setup["nominal"], **kw)
        except BaseException:
            self.bank.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctl.close()
        self.bank.close()


@pytest.fixture(scope="module")
def reference(setup):
    """The blocking controller in closed loop with the plant: the states every route is ticked with, and its records."""
    plant = O.Vehicle.from_params(O.orca_params())
    xs, words = [], []
    x = setup["x0"].copy()
    with Run(setup) as r:
        for t in range(T):
            xs.append(x.copy())
            o = r.ctl.tick(x)
            words.append(_ctl_words(o, H))
            xn, _ = O.sim_continuous(plant, x, np.array(o.u_seq[0][:]).reshape(2, 1), [0, TS])
            x = xn[:, -1]
        assert r.bank.launches == T
    # the ticks' kinds all occur: warm ones, the first look-back, the full window, mu-hat in use
    assert [w[3] for w in words] == [1, 1, 1, 1, 0, 0, 0] and [w[1] for w in words] == list(range(T))
    return xs, words


def same(words, reference):
    assert len(words) == len(reference[1])
    for a, b in zip(reference[1], words):
        _same_words(a, b)


def test_async_wait_equals_blocking(setup, reference):
    with Run(setup) as r:
        words = []
        for x in reference[0]:
            r.ctl.tick_async(x)
            words.append(_ctl_words(r.ctl.wait(), H))
        assert r.bank.launches == T
    same(words, reference)


def test_armed_equals_launched(setup, reference):
    """Every tick after the first is an armed launch, rung by tick_async: one launch per tick all the same."""
    with Run(setup, prelaunch=True) as r:
        words = [_ctl_words(r.ctl.tick(x), H) for x in reference[0]]
        assert r.bank.launches == T                # the bank counts a rung launch as the tick's one
    same(words, reference)
    with Run(setup, prelaunch=True) as r:          # ... and through tick_async + wait
        words = []
        for x in reference[0]:
            r.ctl.tick_async(x)
            words.append(_ctl_words(r.ctl.wait(), H))
    same(words, reference)


@pytest.mark.parametrize("prelaunch", [False, True])
def test_refused_calls_change_nothing(nat, setup, reference, prelaunch):
    """A wait with no tick outstanding and a second tick_async while one is pending are refused
    (LLAMPC_E_STATE) and leave the tick in flight and every later one as they were."""
    with Run(setup, prelaunch=prelaunch) as r:
        words = []
        for t, x in enumerate(reference[0]):
            with pytest.raises(nat.NativeError, match="no controller tick outstanding"):
                r.ctl.wait()
            r.ctl.tick_async(x)
            if t % 2 == 0:
                with pytest.raises(nat.NativeError, match="a controller tick is outstanding: call llampc_ctl_wait"):
                    r.ctl.tick_async(x + 1.0)
            words.append(_ctl_words(r.ctl.wait(), H))
        assert r.bank.launches == T
    same(words, reference)


def test_host_carried_gather_at_world_one(nat, setup, reference):
    """llampc_ctl_set_gather without a communicator, world 1: a full-window tick is two launches with the
    shard's record read (shard_record) and handed back (resume) in between; the records are the unsharded
    controller's."""
    lib = nat.load()
    with Run(setup) as r:
        h, pg = r.ctl._h, np.ascontiguousarray(setup["params"], dtype=np.float64)
        nat.check(lib.llampc_ctl_set_gather(h, 1, 0, None, nat.dptr(pg), int(pg.shape[1])))
        buf = np.zeros(int(lib.llampc_ctl_record_words(K)), dtype=np.uint64)
        words, carried = [], []
        for x in reference[0]:
            l0 = r.bank.launches
            r.ctl.tick_async(x)
            nw = nat.C.c_int32()
            nat.check(lib.llampc_ctl_shard_record(h, buf.ctypes.data, nat.C.byref(nw)))
            carried.append(nw.value)
            if nw.value:
                with pytest.raises(nat.NativeError, match="the tick's records are not gathered yet"):
                    r.ctl.wait()
                nat.check(lib.llampc_ctl_resume(h, buf.ctypes.data))
            words.append(_ctl_words(r.ctl.wait(), H))
            assert r.bank.launches - l0 == 1       # the bank counts the tick, not its launches
        assert carried == [0, 0, 0, 0] + [4 * (K + 1)] * 3           # the exchange runs on full-window ticks only
    same(words, reference)


def corridor_run(setup, xs, prelaunch):
    """Corridor on for ticks 0-2, off for 3-4, on again for 5-6; the read-back after ticks 2 and 6."""
    words, cors = [], {}
    with Run(setup, prelaunch=prelaunch, corridor_weight=50.0, corridor_margin=0.05) as r:
        for t, x in enumerate(xs):
            if t == 3:
                r.ctl.set_corridor(0.0)
            if t == 5:
                r.ctl.set_corridor(50.0, 0.05)
            l0 = r.bank.launches
            words.append(_ctl_words(r.ctl.tick(x), H))
            assert r.bank.launches - l0 == 1, t
            if t in (2, 6):
                cors[t] = r.ctl.corridor()
            if t == 4:
                with pytest.raises(Exception, match="the last tick was not a corridor tick"):
                    r.ctl.corridor()
    return words, cors


def test_corridor_on_off_on_armed_equals_launched(setup, reference):
    wl, cl = corridor_run(setup, reference[0], False)
    wa, ca = corridor_run(setup, reference[0], True)
    for a, b in zip(wl, wa):
        _same_words(a, b)
    for t in (2, 6):
        assert cl[t][3] == ca[t][3], t
        for a, b in zip(cl[t][:3], ca[t][:3]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), t
    assert [w[1] for w in wl] == list(range(T))

"""The controller tick's parity matrix on the device (tests/ctl_matrix.py; conditions:
test_ctl_matrix_cpu.py): every row asserts through llampc_ctl_variant the launch variant it means to
run — ctl_kernel<4>, <2> and <1>, staged and unstaged inputs, the cross-wave slot reductions, the
candidates-per-lane loop, R = 2 look-back lanes, every degenerate size — then ticks LLAMPC (ONE launch
per tick, launched) against ControllerOracle in closed loop and compares, per tick, the whole record:
candidates, reference, selection, top-K, the look-ahead best, the non-finite count, the window and
estimator fields and the padding (ctl_matrix.check_tick; tolerances: test_ctl_gpu.py's).  At most one
cost pair in ten of a row may pass by its core-error bound rather than by 1e-7.  Staged rows equal their
LLAMPC_CTL_NO_STAGE=1 run and the armed rows their launched run, bitwise."""
import pytest

import ctl_matrix as M
from test_ctl_gpu import _same_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


_LAUNCHED = {}


def _launched(row):
    """The row's launched, staged, checked run (once per session): its records."""
    if row.name not in _LAUNCHED:
        _LAUNCHED[row.name] = M.run_device(row)
    return _LAUNCHED[row.name]


def _assert_variant(row):
    got = M.variant(row)
    for f, w in row.variant.items():
        assert got[f] == w, (row.name, f, got)
    return got


@pytest.mark.parametrize("row", M.ROWS, ids=repr)
def test_ctl_row_vs_oracle(nat, monkeypatch, row):
    """The row's variant, then every tick's record against the oracle."""
    monkeypatch.delenv("LLAMPC_CTL_NO_STAGE", raising=False)
    _assert_variant(row)
    _launched(row)


@pytest.mark.parametrize("row", [r for r in M.ROWS if r.nostage], ids=repr)
def test_ctl_row_unstaged_equals_staged(nat, monkeypatch, row):
    """A staged row with LLAMPC_CTL_NO_STAGE=1 (the rollout forms the input terms per step): the
    variant entry reports s4 = 0 and nothing else changed, the records equal the staged run's bitwise."""
    monkeypatch.delenv("LLAMPC_CTL_NO_STAGE", raising=False)
    staged = _assert_variant(row)
    assert staged["s4"] == 1
    want = _launched(row)
    monkeypatch.setenv("LLAMPC_CTL_NO_STAGE", "1")
    assert M.variant(row) == {**staged, "s4": 0}
    got = M.run_device(row, check=False)
    for a, b in zip(want, got):
        _same_words(a, b)


@pytest.mark.parametrize("row", [r for r in M.ROWS if r.armed], ids=repr)
def test_ctl_row_armed_equals_launched(nat, monkeypatch, row):
    """ctl_kernel<2> / <1> behind the doorbell (prelaunch=True: each tick's launch armed during the one
    before): the records equal the launched run's bitwise."""
    monkeypatch.delenv("LLAMPC_CTL_NO_STAGE", raising=False)
    _assert_variant(row)
    want = _launched(row)
    got = M.run_device(row, prelaunch=True, check=False)
    for a, b in zip(want, got):
        _same_words(a, b)


def test_ctl_refused_shape_launches_nothing(nat):
    """C H beyond the CU's LDS even unstaged: llampc_ctl_variant and llampc_ctl_create both answer
    LLAMPC_E_ARG, and the bank has launched nothing."""
    from llampc.mpc import DeviceController, ModelBank, generate_bank
    r = M.REFUSED
    with pytest.raises(nat.NativeError) as e:
        nat.ctl_variant(r["N"], r["C"], r["H"], r["K"], M.KNOTS[r["track"]])
    assert e.value.code == nat.E_ARG
    tr, _ = M.tracks(r["track"])
    with ModelBank(generate_bank(r["N"], seed=0), W=2, device=0) as b:
        with pytest.raises(nat.NativeError) as e:
            DeviceController(b, tr, H=r["H"], C=r["C"], K=r["K"])
        assert e.value.code == nat.E_ARG
        assert b.launches == 0

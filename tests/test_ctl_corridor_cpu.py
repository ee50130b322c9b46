"""The controller tick's corridor without a GPU (rows, oracle and checker: ctl_corridor_cases.py):
the rows' table — the share of penalised candidates, the ticks with a valid path — and ctl_matrix's
exact-index gaps recomputed on the oracle; the checker against three mutant oracles (the corridor along
the reference, the path not shifted, the penalty dropped) on every row where the corridor bites; the
Python argument checks, which raise before any device call; and csrc's host-checkable parts in a
stand-alone program built with AddressSanitizer and UBSan (tests/native/ctl_corridor_host.cpp): the
path rule and its validity bitwise against NumPy, ctl_shape with the corridor against the rule below."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ctl_corridor_cases as CC
import ctl_matrix as M
from conftest import REPO

HIPCC = "/opt/rocm/bin/hipcc"
# The checker's bounds need the lean cores' relative errors, measured on the device; here 1e-13 each,
# some 500 ulp: far above any measured value (test_fastmath_gpu.py holds the cores to a few ulp), so the
# mutants are rejected under bounds looser than the GPU file's.
CPU_EPS = dict(atan2=1e-13, atan=1e-13, sin=1e-13)


@pytest.mark.parametrize("row", CC.ROWS, ids=repr)
def test_rows_table_and_gaps(row):
    """The row does what ctl_corridor_cases.TABLE says of it, and every exact index of its ticks rests
    on a gap above GAP_COST / GAP_MEAN (ctl_matrix.tick_gaps)."""
    outs, _ = CC.reference(row)
    lo, hi, valid = CC.TABLE[row.name]
    pos = sum(int(np.count_nonzero(o["pen"] > 0)) for o in outs)
    tot = sum(o["pen"].size for o in outs)
    print(f"{row.name}: {pos} of {tot} rolled-out candidates penalised, "
          f"{sum(o['path_valid'] for o in outs)} ticks with a valid path")
    assert lo <= pos / tot <= hi, (row.name, pos / tot)
    assert sum(o["path_valid"] for o in outs) == valid
    from llampc.mpc import constraints
    assert not outs[0]["path_valid"] and np.array_equal(outs[0]["hp"], constraints.disabled(row.H))
    if row.name.startswith("ethz-c"):                       # every candidate of every tick with a path
        assert all((o["pen"] > 0).all() for o in outs if o["path_valid"])
    g = np.array([M.tick_gaps(row, o) for o in outs])
    assert g[:, 0].min() > M.GAP_COST and g[:, 1].min() > M.GAP_COST and g[:, 2].min() > M.GAP_MEAN, g.min(axis=0)


def test_wide_corridor_is_the_plain_oracle():
    """mobil-wide: no slack anywhere, so the corridor oracle's ticks are the plain oracle's."""
    row = CC.BY_NAME["mobil-wide"]
    outs, xs = CC.reference(row)
    plain = M.oracle_for(row)
    for o, x in zip(outs, xs):
        with np.errstate(all="ignore"):
            p = plain.tick(x)
        assert (p["best_model"], p["best_cand"], p["cost"]) == (o["best_model"], o["best_cand"], o["cost"])
        np.testing.assert_array_equal(p["slot_costs"], o["slot_costs"])
        np.testing.assert_array_equal(p["u_seq"], o["u_seq"])


def _run_checker(row, cls):
    """The true oracle's records against cls's ticks on the true loop's states."""
    outs, xs = CC.reference(row)
    orc = CC.oracle_for(row, cls)
    counts = dict(pairs=0, bound=0)
    projidx = 0
    for t, (o, x) in enumerate(zip(outs, xs)):
        m = orc.tick(x)
        cor = (o["path"], o["hp"], None, o["path_valid"])
        CC.check_tick(row, t, m, x, CC.record_from(row, o), o["xref"], o["U"], projidx, counts, cor,
                      CC.device_costs(row, o), eps=CPU_EPS)
        projidx = o["projidx"]
    return counts


@pytest.mark.parametrize("row", CC.ROWS, ids=repr)
def test_checker_accepts_the_oracle(row):
    counts = _run_checker(row, CC.CorridorOracle)
    assert counts["pairs"] > 0 and counts["bound"] == 0


@pytest.mark.parametrize("cls", CC.MUTANTS, ids=lambda c: c.__name__)
@pytest.mark.parametrize("row", CC.BITES, ids=repr)
def test_checker_rejects_mutants(row, cls):
    """The checker rejects the mutant on at least one tick of the row: an index, a cost beyond RTOL_ROLL,
    or (AlongXref, NotShifted) the path beyond PATH_ATOL.  On mobil-mixed the penalised costs (33 of
    the 832 rolled out, w pen <= 2.8e-3 against J ~ 4) are never a slot's best and no argmin moves without
    the penalty: the record alone is the true oracle's, and NoPenalty falls by the rolled-out costs
    (LLAMPC.corridor_costs, check_slot_costs)."""
    with pytest.raises(AssertionError):
        _run_checker(row, cls)


def test_python_argument_checks():
    """Refused before any device call (no bank is touched): a bad weight, a weight in host mode, a
    track without the corridor's tables, a margin that leaves no corridor."""
    from llampc.mpc import LLAMPC
    from llampc.mpc.controller import DeviceController
    tr, _ = M.tracks("ETHZ")

    class Bare:
        lap_projidx = 0
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="corridor_weight must be finite and >= 0"):
            LLAMPC(None, tr, corridor_weight=w)
        with pytest.raises(ValueError, match="corridor_weight must be finite and >= 0"):
            DeviceController(None, tr, corridor_weight=w)
    with pytest.raises(ValueError, match="mode='device'"):
        LLAMPC(None, tr, mode="host", corridor_weight=1.0)
    with pytest.raises(ValueError, match="needs a track with center_line, theta_track, track_length and track_width"):
        LLAMPC(None, Bare(), corridor_weight=1.0)
    for m in (float(tr.track_width) / 2, 1.0, float("nan")):
        with pytest.raises(ValueError, match="leaves no corridor"):
            LLAMPC(None, tr, corridor_weight=1.0, corridor_margin=m)
    with pytest.raises(ValueError, match="must be finite"):
        DeviceController(None, tr, corridor_weight=1.0, corridor_margin=float("-inf"))


def test_entries_declared_and_bound():
    """The five new C entries: declared in include/llampc.h, bound in llampc/_native.py."""
    from llampc import _native as nat
    text = open(os.path.join(REPO, "include", "llampc.h")).read()
    for name in ("llampc_ctl_set_track", "llampc_ctl_set_corridor", "llampc_ctl_corridor", "llampc_ctl_corridor_costs",
                 "llampc_ctl_variant_corridor"):
        assert f"int {name}(" in text and name in nat._SIGNATURES


# ---- the stand-alone host program -----------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("ctl_corridor")
    out = str(tmp / "ctl_corridor_host")
    cmd = [hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer",
           f"-I{os.path.join(REPO, 'lla-mpc_amd', 'csrc')}", f"-I{os.path.join(REPO, 'include')}",
           os.path.join(REPO, "tests", "native", "ctl_corridor_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)

    def run(*args):
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        e.pop("LLAMPC_CTL_NO_STAGE", None)
        r = subprocess.run([out, *map(str, args)], capture_output=True, text=True, env=e)
        assert r.returncode == 0, r.stderr
        return r.stdout.strip().splitlines()
    run.tmp = tmp
    return run


def test_native_path_rule(harness):
    """ctl_path_index / ctl_path_valid: the path bitwise constraints.default_path's, valid exactly when
    the cost and all H + 1 positions are finite."""
    from llampc.mpc import constraints
    rng = np.random.RandomState(3)
    for H in (1, 2, 20, 64):
        for bad in (None, "cost_nan", "cost_inf", "x0", "xH", "y_mid"):
            xy = rng.uniform(-3, 3, size=(2, H + 1))
            cost = 12.5
            if bad == "cost_nan":
                cost = np.nan
            elif bad == "cost_inf":
                cost = np.inf
            elif bad == "x0":
                xy[0, 0] = np.inf
            elif bad == "xH":
                xy[0, H] = np.nan
            elif bad == "y_mid":
                xy[1, H // 2] = -np.inf
            f = str(harness.tmp / "path.bin")
            np.concatenate([[H, cost], xy[0], xy[1]]).astype(np.float64).tofile(f)
            lines = harness("path", f)
            assert lines[0] == f"valid {int(bad is None)}", (H, bad, lines[0])
            got = np.array([[float(v) for v in ln.split()] for ln in lines[1:]]).T
            want = constraints.default_path(None, H, 0.02, xy)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (H, bad)


def test_native_ctl_shape_corridor(harness):
    """ctl_shape with the corridor: the plain shape's lane split and block counts, never staged, H
    corridor blocks, and the LDS the largest of the look-ahead layout with hp [H][6], the winner's
    positions [2][H+1] and a 16-B flag behind it, the look-back's regions, and a corridor block's
    64 B + three tables of track_n doubles — plus the completing block's 4 KiB; llampc_ctl_variant_corridor
    reports the same fields."""
    from llampc import _native as nat
    from test_capi_native import ctl_lds_model, lb_final_lds
    a16 = lambda v: (v + 15) & ~15
    fields = lambda lines: {k: int(v) for k, v in (ln.split() for ln in lines)}
    for n, C_, H, K, rl_n, tn in ((200, 8, 20, 10, 700, 666), (100, 96, 20, 10, 700, 666), (100, 200, 20, 10, 700, 666),
                                  (200, 64, 40, 10, 500, 300), (10000, 64, 40, 10, 700, 666), (1, 1, 1, 1, 2, 4096),
                                  (5121, 8, 10, 32, 700, 2)):
        got = fields(harness("shape", n, C_, H, K, rl_n, 0, 1, tn))
        plain = nat.ctl_variant(n, C_, H, K, rl_n)
        for f in ("lpm", "G", "cpl", "mpb", "zfit", "R", "nb_lb", "nb_la"):
            assert got[f] == plain[f], (f, n, C_, H)
        assert (got["s4"], got["nb_cor"], got["nslots"]) == (0, H, K + 1)
        la = a16(ctl_lds_model(H, C_, rl_n, False) + 48 * H + 16 * (H + 1) + 16)
        want = a16(max(la, 64 + 24 * tn, lb_final_lds(got["nb_lb"], K)))
        assert (got["poll_off"], got["lds"]) == (want, want + 4096), (n, C_, H, K, rl_n, tn)
        assert nat.ctl_variant_corridor(n, C_, H, K, rl_n, tn) == {f: got[f] for f in nat.CTL_VARIANT_FIELDS + ("nb_cor",)}
    # the largest centre line's tables outweigh a small look-ahead; a warm-up tick rolls one model out
    assert fields(harness("shape", 1, 1, 1, 1, 2, 0, 1, 4096))["poll_off"] == a16(64 + 24 * 4096)
    w = fields(harness("shape", 200, 8, 20, 10, 700, 1, 0, 666))
    assert (w["nslots"], w["nb_la"], w["nb_lb"], w["nb_cor"]) == (1, 1, 1, 20)

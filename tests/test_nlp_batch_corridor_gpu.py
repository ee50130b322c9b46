"""setupNLPBatch.solve(..., corridor=, corridor_weight=, corridor_path=) (llampc_nlp_batch_solve_corridor,
llampc_nlp_batch_solve_track; csrc/nlp_batch_corr.hip, csrc/corridor_batch.hip): B problems in one
launch, each under its OWN soft corridor and weight, against the restatement
test_nlp_corridor_gpu.nlp_cem_corridor with each problem's own bank column, seed, call number, warm
start, half-planes and weight (tests/nlp_batch_corridor_cases.py), and against setupNLP's corridor
solve on that column.  The conditions that keep the comparisons from passing vacuously or hanging on
a rank flip are asserted on the restatement in test_nlp_batch_corridor_cpu.py and again here before
every comparison.

Tolerances (test_nlp_corridor_gpu.py's): umpc bitwise, fval 1e-6 relative, xmpc 1e-8 relative and
1e-12 absolute, max_slack within 1e-12 of the value recomputed from the returned xmpc, violation
consistent with corridor_tol."""
import numpy as np
import pytest

import nlp_batch_cases as BC
import nlp_batch_corridor_cases as CC
import nlp_matrix as M

pytestmark = pytest.mark.gpu

RTOL_FVAL = 1e-6
RTOL_XMPC = 1e-8
ATOL_XMPC = 1e-12
ATOL_SLACK = 1e-12
ATOL_BUILDER = 1e-12                     # the single device builder's tolerance against the host's
# fval and xmpc of a batched corridor problem against setupNLP.solve(..., corridor=) on the same
# column, seed, half-planes and weight, read on the MI355X over the 12 (shape, problem) pairs of
# test_equals_the_single_corridor_solver; None: not read yet (the tolerances alone are asserted)
SINGLE_EXACT = True
SINGLE_EXACT_NOTE = ("bitwise in umpc, fval, xmpc and max_slack for all 12 pairs: relative fval deviation 0, largest "
                     "|xmpc| difference 0 (the module's first MI355X run, "
                     "profiles/r12/nlp_batch_corridor/new_tests_figures.log)")


@pytest.fixture(scope="module")
def nat():
    from llampc import _native
    _native.load()
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X")
    return _native


@pytest.fixture()
def bank(nat):
    from llampc.mpc import ModelBank
    with ModelBank(BC.bank(), W=3, device=0) as b:
        yield b


def check_problem(nb, shape, ref, p, out, tag=""):
    """Problem p of a corridor solve `out` on solver nb against its restatement."""
    umpc, fval, xmpc = out[0][p], out[1][p], out[2][p]
    H = shape[3]
    dev = abs(fval - ref["j"]) / abs(ref["j"])
    want_slack = CC.max_slack_of(ref["hp"], xmpc[:2])
    print(f"FVAL_DEV {BC.sid(shape)} problem {p} model {ref['model']}{tag}: device {fval!r} restated {ref['j']!r} "
          f"relative {dev:.3g} umpc equal {np.array_equal(umpc.T, ref['u'])} max_slack {nb.max_slack[p]!r} "
          f"recomputed {want_slack!r}")
    assert umpc.shape == (2, H) and xmpc.shape == (6, H + 1)
    np.testing.assert_array_equal(umpc.T, ref["u"])
    np.testing.assert_allclose(fval, ref["j"], rtol=RTOL_FVAL)
    np.testing.assert_allclose(xmpc, ref["xm"].T, rtol=RTOL_XMPC, atol=ATOL_XMPC)
    assert abs(nb.max_slack[p] - want_slack) <= ATOL_SLACK
    assert nb.violation[p] == (nb.Ts if nb.max_slack[p] > nb.corridor_tol else 0.0)
    return dev


def solve_mixed(nb, shape, refs, x0=None, B=6):
    x, up, xref = BC.inputs(shape)
    return nb.solve(BC.MODELS[:B], (x if x0 is None else x0)[:B], xref[:B], up[:B], seeds=BC.SEEDS[:B],
                    corridor=CC.mixed_hp(refs), corridor_weight=CC.weights(B))


@pytest.mark.parametrize("shape", CC.MIXED_SHAPES, ids=BC.sid)
def test_mixed_batch_equals_restatement(bank, shape):
    """1. Six problems, each with its own half-planes and its own weight, in one launch."""
    refs = CC.mixed(shape)
    CC.check_mixed_conditions(shape, refs, CC.MIXED_MOVED[shape])
    nb = BC.batch_solver(shape, bank)
    try:
        before = bank.launches
        out = solve_mixed(nb, shape, refs)
        assert bank.launches == before + 1
        assert out[3].tolist() == [True] * 6 and nb.max_slack.shape == (6,) and nb.violation.shape == (6,)
        assert nb.last_corridor is None
        devs = [check_problem(nb, shape, refs[p], p, out) for p in range(6)]
    finally:
        nb.close()
    print(f"FVAL_DEV_MAX {BC.sid(shape)}: {max(devs):.3g}")


@pytest.mark.parametrize("shape", CC.SINGLE_SHAPES, ids=BC.sid)
def test_equals_the_single_corridor_solver(bank, shape):
    """2. Each problem equals setupNLP on that column and seed with solve(..., corridor=hp[p]) and
    corridor_weight = w[p]: umpc bitwise, fval and xmpc at the tolerances; whether those two were
    bitwise is printed and, once read on the MI355X (SINGLE_EXACT_NOTE), asserted."""
    refs = CC.mixed(shape)
    nb = BC.batch_solver(shape, bank)
    try:
        umpc, fval, xmpc, ok = solve_mixed(nb, shape, refs)
        slack = nb.max_slack.copy()
    finally:
        nb.close()
    assert ok.all()
    x0, up, xref = BC.inputs(shape)
    exact = []
    for p, (model, seed) in enumerate(zip(BC.MODELS, BC.SEEDS)):
        one = BC.single_solver(shape, model, seed)
        one.corridor_weight = refs[p]["w"]
        try:
            u1, f1, x1, _ = one.solve(x0[p], xref[p], up[p], corridor=refs[p]["hp"])
            s1 = one.max_slack
        finally:
            one.close()
        exact_f, exact_x = f1 == fval[p], np.array_equal(x1, xmpc[p])
        exact.append(exact_f and exact_x)
        print(f"SINGLE {BC.sid(shape)} problem {p} model {model} w {refs[p]['w']:g}: fval bitwise {exact_f} (relative "
              f"{abs(f1 - fval[p]) / abs(f1):.3g}) xmpc bitwise {exact_x} (max abs {np.max(np.abs(x1 - xmpc[p])):.3g}) "
              f"max_slack equal {s1 == slack[p]}")
        np.testing.assert_array_equal(umpc[p], u1)
        np.testing.assert_allclose(fval[p], f1, rtol=RTOL_FVAL)
        np.testing.assert_allclose(xmpc[p], x1, rtol=RTOL_XMPC, atol=ATOL_XMPC)
        assert abs(s1 - slack[p]) <= ATOL_SLACK
    print(f"SINGLE_EXACT {BC.sid(shape)}: {all(exact)}")
    if SINGLE_EXACT is not None:
        assert all(exact) == SINGLE_EXACT, SINGLE_EXACT_NOTE


def test_warm_chain_with_a_changing_model(bank):
    """3. Slot 0 (model 0 -> 3 -> 7) under the +0.05 / 1e3 funnel rebuilt per call, warm-started from
    its own previous corridor umpc; slot 1 under constraints.disabled(H): bitwise a plain
    setupNLPBatch's slot 1 over the same three calls (J + w 0 = J), max_slack 0."""
    from llampc.mpc import constraints
    shape = BC.CHAIN_SHAPE
    H = shape[3]
    chain = CC.chain()
    for call, (ref, plain) in enumerate(chain):
        CC.check_problem_conditions(shape, ref, f" chain call {call}")
        assert ref["moved"]
        BC.check_conditions(shape, plain, f" chain call {call} slot 1")
    plain_out = []
    nb = BC.batch_solver(shape, bank)
    try:
        for t, models in zip(BC.CHAIN_TICKS, BC.CHAIN_MODELS):
            x0, up, xref = BC.inputs(shape, (t, t))
            plain_out.append(nb.solve(models, x0, xref[0], up, seeds=BC.CHAIN_SEEDS))
    finally:
        nb.close()
    nb = BC.batch_solver(shape, bank)
    try:
        for call, (t, models) in enumerate(zip(BC.CHAIN_TICKS, BC.CHAIN_MODELS)):
            ref, plain = chain[call]
            x0, up, xref = BC.inputs(shape, (t, t))
            hp = np.array([ref["hp"], constraints.disabled(H)])
            out = nb.solve(models, x0, xref[0], up, seeds=BC.CHAIN_SEEDS, corridor=hp,
                           corridor_weight=[CC.VARIANTS[0][1], CC.VARIANTS[1][1]])
            assert out[3].all()
            check_problem(nb, shape, ref, 0, out, f" call {call} slot 0")
            for a, b in zip(out[:3], plain_out[call][:3]):
                np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(out[0][1].T, plain["u"])
            assert nb.max_slack[1] == 0.0 and nb.violation[1] == 0.0
    finally:
        nb.close()


def test_chunking(bank):
    """4. max_resident = two problems' blocks, B = 5 under the mixed rule: three launches with call
    numbers 0, 0, 1, 1, 2; each chunk takes its own rows of the corridors and weights."""
    shape = BC.CHUNK_SHAPE
    B = BC.CHUNK_B
    refs = CC.chunked()
    CC.check_mixed_conditions(shape, refs, 4, " chunked")
    nb = BC.batch_solver(shape, bank, max_resident=BC.CHUNK_PER_LAUNCH * (shape[0] // 64))
    try:
        assert nb.per_launch == BC.CHUNK_PER_LAUNCH
        before = bank.launches
        out = solve_mixed(nb, shape, refs, B=B)
        assert bank.launches == before + 3
        assert out[3].all()
        for p in range(B):
            check_problem(nb, shape, refs[p], p, out, f" chunk {p // BC.CHUNK_PER_LAUNCH}")
    finally:
        nb.close()


def test_a_failed_neighbour(bank):
    """5. Problem 2's x0[2] is NaN under the mixed corridors: ok[2] False, umpc zeros, fval inf,
    max_slack and violation 0; every other problem is bitwise what it is without the NaN neighbour."""
    shape = BC.ISO_SHAPE
    refs = CC.mixed(shape)
    x0, up, xref = BC.inputs(shape)
    bad = x0.copy()
    bad[BC.ISO_BAD, 2] = np.nan
    nb = BC.batch_solver(shape, bank)
    try:
        clean = solve_mixed(nb, shape, refs)
        clean_slack = nb.max_slack.copy()
    finally:
        nb.close()
    nb = BC.batch_solver(shape, bank)
    try:
        umpc, fval, xmpc, ok = solve_mixed(nb, shape, refs, bad)
        assert ok.tolist() == [p != BC.ISO_BAD for p in range(6)]
        assert np.all(umpc[BC.ISO_BAD] == 0.0) and fval[BC.ISO_BAD] == np.inf
        assert nb.max_slack[BC.ISO_BAD] == 0.0 and nb.violation[BC.ISO_BAD] == 0.0
        for p in range(6):
            if p != BC.ISO_BAD:
                for a, b in zip((umpc, fval, xmpc, nb.max_slack), clean[:3] + (clean_slack,)):
                    np.testing.assert_array_equal(a[p], b[p])
                check_problem(nb, shape, refs[p], p, (umpc, fval, xmpc), " beside the NaN")
    finally:
        nb.close()


@pytest.mark.parametrize("shape", CC.ALONE_SHAPES, ids=BC.sid)
def test_one_problem_alone_equals_it_in_the_batch(bank, shape):
    """6. B = 1 is the same kernel and the same arithmetic: bitwise in umpc, fval, xmpc, max_slack."""
    refs = CC.mixed(shape)
    x0, up, xref = BC.inputs(shape)
    nb = BC.batch_solver(shape, bank)
    try:
        six = solve_mixed(nb, shape, refs)
        six_slack = nb.max_slack.copy()
    finally:
        nb.close()
    assert six[3].all()
    for p in (0, 3):
        nb = BC.batch_solver(shape, bank)
        try:
            one = nb.solve([BC.MODELS[p]], x0[p:p + 1], xref[p:p + 1], up[p:p + 1], seeds=[BC.SEEDS[p]],
                           corridor=refs[p]["hp"], corridor_weight=refs[p]["w"])     # [H, 6] and a scalar
            assert one[3].all() and nb.max_slack[0] == six_slack[p]
        finally:
            nb.close()
        for a, b in zip(one[:3], six[:3]):
            np.testing.assert_array_equal(a[0], b[p])


def device_solver(shape, bank, **kw):
    return BC.batch_solver(shape, bank, track=CC.track(), device_corridor=True, corridor_margin=CC.device_margin(),
                           corridor_weight=CC.DEVICE_WEIGHT, **kw)


@pytest.mark.parametrize("shape", CC.DEVICE_SHAPES, ids=BC.sid)
def test_device_built_corridors(bank, shape):
    """7. The track's corridors built on the device along the six unconstrained optima: the builder
    against constraints.track_corridor and track.xy_to_param (1e-12); the pair is two launches; the
    solve is bitwise the same solver's solve(..., corridor=last_corridor) on a fresh handle and
    equals the restatement under the built half-planes; the next solve follows each slot's shifted
    xmpc (constraints.default_path)."""
    from llampc.mpc import constraints
    H, tr = shape[3], CC.track()
    paths = CC.device_paths(shape)
    host = CC.device_host_corridors(shape)
    x0, up, xref = BC.inputs(shape)
    nb = device_solver(shape, bank)
    try:
        before = bank.launches
        out = nb.solve(BC.MODELS, x0, xref, up, seeds=BC.SEEDS, corridor_path=paths)
        assert bank.launches == before + 2            # the builder and the search
        assert out[3].all()
        built, slack, viol = nb.last_corridor.copy(), nb.max_slack.copy(), nb.violation.copy()
        print(f"BUILDER {BC.sid(shape)}: largest |hp - host| {np.max(np.abs(built - host)):.3g}")
        np.testing.assert_allclose(built, host, rtol=0, atol=ATOL_BUILDER)
        refs = CC.device_refs(shape, built)
        CC.check_device_conditions(shape, refs, " device-built")
        for p in range(6):
            check_problem(nb, shape, refs[p], p, out, " device-built")
        # the second solve, no corridor_path: along each slot's previous xmpc shifted one step
        nxt = nb.solve(BC.MODELS, x0, xref, up, seeds=BC.SEEDS)
        assert bank.launches == before + 4 and nxt[3].all()
        for p in range(6):
            want = constraints.track_corridor(tr, constraints.default_path(x0[p], H, nb.Ts, out[2][p]), CC.device_margin())
            np.testing.assert_allclose(nb.last_corridor[p], want, rtol=0, atol=ATOL_BUILDER)
            assert abs(nb.max_slack[p] - CC.max_slack_of(nb.last_corridor[p], nxt[2][p][:2])) <= ATOL_SLACK
        # the builder alone: the same bits as the solve's, and theta
        hp2, theta = nb.track_corridor(paths)
        assert bank.launches == before + 5
        np.testing.assert_array_equal(hp2, built)
        want_theta = np.array([[float(tr.xy_to_param(P[0, k], P[1, k])) for k in range(1, H + 1)] for P in paths])
        np.testing.assert_allclose(theta, want_theta, rtol=0, atol=ATOL_BUILDER)
    finally:
        nb.close()
    fresh = device_solver(shape, bank)
    try:
        again = fresh.solve(BC.MODELS, x0, xref, up, seeds=BC.SEEDS, corridor=built)
        for a, b in zip(again[:3] + (fresh.max_slack, fresh.violation), out[:3] + (slack, viol)):
            np.testing.assert_array_equal(a, b)
        assert fresh.last_corridor is None
    finally:
        fresh.close()


def test_refusals_launch_nothing(nat, bank):
    """8. Argument errors raise before any launch: the bank's launch counter is unchanged."""
    shape = CC.MIXED_SHAPES[0]
    H = shape[3]
    refs = CC.mixed(shape)
    hp, w = CC.mixed_hp(refs), CC.weights()
    x0, up, xref = BC.inputs(shape)
    args = (BC.MODELS, x0, xref, up)

    def bad(p, row, col, v):
        h = hp.copy()
        h[p, row, col] = v
        return h
    nb = BC.batch_solver(shape, bank, max_batch=6)
    dv = device_solver(shape, bank, max_batch=6)
    try:
        before = bank.launches
        # the library's per-problem checks name the problem
        for p, h in ((3, bad(3, 0, 0, np.nan)), (5, bad(5, 19, 4, np.inf)), (1, bad(1, 7, 2, -np.inf)),
                     (0, bad(0, 2, 5, np.nan))):
            with pytest.raises(nat.NativeError, match=f"problem {p}") as e:
                nb.solve(*args, seeds=BC.SEEDS, corridor=h, corridor_weight=w)
            assert e.value.code == nat.E_ARG
        # weights: the Python layer's check, and the library's own below it
        for bw in (-1.0, np.nan, np.inf, [1, 1, -1, 1, 1, 1], [1.0] * 5, np.ones((6, 1))):
            with pytest.raises(ValueError, match="corridor_weight"):
                nb.solve(*args, corridor=hp, corridor_weight=bw)
        models, seeds = np.array(BC.MODELS, dtype=np.int64), np.array(BC.SEEDS, dtype=np.uint64)
        xr = np.ascontiguousarray(xref)
        hold, st = np.zeros(6, dtype=np.int32), np.zeros(6, dtype=np.int32)
        o = (np.zeros((6, H, 2)), np.zeros(6), np.zeros((6, H + 1, 6)), np.zeros(6))
        lib = nat.load()

        def c_solve(B, hp_, w_, slack=o[3]):
            return lib.llampc_nlp_batch_solve_corridor(
                nb._h, B, models.ctypes.data, seeds.ctypes.data, x0.ctypes.data, xr.ctypes.data, up.ctypes.data, None,
                hold.ctypes.data, None if hp_ is None else hp_.ctypes.data, None if w_ is None else w_.ctypes.data,
                o[0].ctypes.data, o[1].ctypes.data, o[2].ctypes.data, st.ctypes.data,
                None if slack is None else slack.ctypes.data)
        wneg = w.copy()
        wneg[4] = -1.0
        for rc in (c_solve(6, hp, wneg), c_solve(6, None, w), c_solve(6, hp, None), c_solve(6, hp, w, None),
                   c_solve(7, hp, w), c_solve(0, hp, w)):          # B above max_batch = 6, B < 1
            assert rc == nat.E_ARG
        # shapes
        for kw in (dict(corridor=hp[:5]), dict(corridor=hp[:, :H - 1]), dict(corridor=hp[:, :, :5]),
                   dict(corridor=np.zeros((H + 1, 6)))):
            with pytest.raises(ValueError, match="corridor must be"):
                nb.solve(*args, **kw)
        # corridor_path without a track; a refused horizon (the constructor's cap)
        with pytest.raises(ValueError, match="device_corridor=True"):
            nb.solve(*args, corridor_path=CC.device_paths(shape))
        with pytest.raises(ValueError, match="device_corridor=True"):
            nb.track_corridor(CC.device_paths(shape))
        with pytest.raises(ValueError, match="horizon"):
            BC.batch_solver((64, 32, 3, 65), bank)
        # the device-built solver: paths and margins
        paths = CC.device_paths(shape)
        for bp in (paths[:5], paths[:, :, :H], paths[:, :1]):
            with pytest.raises(ValueError, match="corridor_path must be"):
                dv.solve(*args, corridor_path=bp)
        nanp = paths.copy()
        nanp[2, 1, 7] = np.nan
        with pytest.raises(ValueError, match="finite"):
            dv.solve(*args, corridor_path=nanp)
        with pytest.raises(ValueError, match="margin"):
            dv.track_corridor(paths, margin=float(CC.track().track_width) / 2)
        with pytest.raises(ValueError, match="margin"):
            BC.batch_solver(shape, bank, track=CC.track(), device_corridor=True,
                            corridor_margin=float(CC.track().track_width) / 2)
        hp_o, th_o = np.zeros((6, H, 6)), np.zeros((6, H))
        for B, pth, margin in ((6, paths, float(CC.track().track_width) / 2), (6, paths, np.nan), (6, nanp, 0.0),
                               (7, paths, 0.0), (0, paths, 0.0)):
            pth = np.ascontiguousarray(pth)
            rc = lib.llampc_nlp_batch_track_corridor(dv._h, B, pth.ctypes.data, margin, hp_o.ctypes.data, th_o.ctypes.data)
            assert rc == nat.E_ARG
        rc = lib.llampc_nlp_batch_track_corridor(nb._h, 6, paths.ctypes.data, 0.0, hp_o.ctypes.data, th_o.ctypes.data)
        assert rc == nat.E_STATE                          # no track set
        assert bank.launches == before
        # the handles are as they were: the next valid solve is call 0's, equal to the restatement
        out = solve_mixed(nb, shape, refs)
        assert bank.launches == before + 1 and out[3].all()
        for p in range(6):
            check_problem(nb, shape, refs[p], p, out, " after the refusals")
    finally:
        nb.close()
        dv.close()


def test_the_existing_path_is_unchanged(bank):
    """9. A plain solve() on a solver constructed with the new keyword arguments at their defaults is
    bitwise a solver's constructed without them, and the restatement's."""
    shape = BC.SHAPES[1]
    x0, up, xref = BC.inputs(shape)
    outs = []
    for kw in ({}, dict(track=None, corridor_weight=1e4, corridor_tol=1e-4, device_corridor=False, corridor_margin=0.0)):
        nb = BC.batch_solver(shape, bank, **kw)
        try:
            before = bank.launches
            outs.append(nb.solve(BC.MODELS, x0, xref, up, seeds=BC.SEEDS))
            assert bank.launches == before + 1
            assert nb.max_slack is None and nb.violation is None and nb.last_corridor is None
        finally:
            nb.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    for p, ref in enumerate(BC.restate_batch(shape)):
        np.testing.assert_array_equal(outs[0][0][p].T, ref["u"])

"""The batched corridor solve's cases (setupNLPBatch.solve(..., corridor=, corridor_weight=,
corridor_path=); llampc_nlp_batch_solve_corridor / _solve_track), shared by
test_nlp_batch_corridor_cpu.py (the conditions, on the restatement alone) and
test_nlp_batch_corridor_gpu.py (the device against the restatement and against setupNLP).

The problems are nlp_batch_cases' six (models, ticks, seeds, the bank).  The reference of a problem
is test_nlp_corridor_gpu.nlp_cem_corridor — oracle.nlp_cem's loop with J + w pen — with that
problem's bank column, seed, call number, warm start, half-planes and weight, computed once per key
and left unchanged.

The mixed batch: around each problem's UNCONSTRAINED optimum (the restatement with hp = None), with P
its Euler positions, hp[p] = constraints.strip(P, 0.03, off arange(1..H) / H) with (off, w) =
(+0.05, 1e3) for even p and (-0.05, 1e5) for odd p: the optimum leaves its funnel by 0.02 at the
horizon's end, every problem has its own half-planes AND its own weight, so a wrong stride or a
shared weight cannot pass.

The device-built batch: the ETHZ track's corridor (margin track_width / 2 - 0.03, weight 1e3) along
each problem's unconstrained optimum's positions.

Conditions (``check_*``), asserted on the restatement alone: every problem's round-0 share of
penalised samples >= 0.10, at least one problem of a mixed shape <= 0.95, every adjacent elite gap >
1e-9 relative, the unconstrained optimum's slack > 0.015 (mixed), and enough problems moved."""
import numpy as np

import nlp_batch_cases as BC
import nlp_matrix as M
from test_nlp_corridor_gpu import corridor_pen, max_slack_of, nlp_cem_corridor  # noqa: F401  (re-exported)

HALF = 0.03
OFF = 0.05
VARIANTS = ((+OFF, 1e3), (-OFF, 1e5))            # even p, odd p
MIXED_SHAPES = [(64, 32, 3, 20), (256, 17, 3, 22), (128, 64, 2, 40), (1024, 32, 2, 20)]
# the least number of the six problems whose umpc differs from the unconstrained one
MIXED_MOVED = {(64, 32, 3, 20): 5, (256, 17, 3, 22): 5, (128, 64, 2, 40): 3, (1024, 32, 2, 20): 5}
SINGLE_SHAPES = [(64, 32, 3, 20), (1024, 32, 2, 20)]
ALONE_SHAPES = [(256, 17, 3, 22), (128, 64, 2, 40)]        # one staged, one unstaged
DEVICE_SHAPES = [(64, 32, 3, 20), (256, 17, 3, 22)]
DEVICE_INSET, DEVICE_WEIGHT = 0.03, 1e3
SHARE_MIN, SHARE_SOME_MAX, SLACK0_MIN, GAP_MIN = 0.10, 0.95, 0.015, 1e-9

assert set(MIXED_SHAPES) <= set(BC.SHAPES) and BC.CHAIN_SHAPE in MIXED_SHAPES and BC.CHUNK_SHAPE in MIXED_SHAPES


def variant(p):
    return VARIANTS[p % 2]


def weights(B=6):
    return np.array([variant(p)[1] for p in range(B)])


_CACHE = {}


def _key(a):
    return None if a is None else np.asarray(a, dtype=np.float64).tobytes()


def _cem(shape, model, tick, seed, call, base, hp, w):
    samples, elite, iters, H = shape
    x0, up, xref = M.inputs(BC.case(shape), tick)
    return nlp_cem_corridor(BC.p6(model), x0, xref, up, base, base is not None, H, hp, w, samples=samples, iters=iters,
                            elite=elite, call=call, seed=seed)


def plain(shape, model, tick, seed, call=0, base=None):
    """The unconstrained restatement: dict(x0, up, xref, u [H, 2], j, xm [H+1, 6])."""
    key = ("plain", shape, model, tick, seed, call, _key(base))
    if key not in _CACHE:
        x0, up, xref = M.inputs(BC.case(shape), tick)
        u, j, xm, _ = _cem(shape, model, tick, seed, call, base, None, 0.0)
        _CACHE[key] = _frozen(dict(x0=x0, up=up, xref=xref, u=u, j=j, xm=xm, model=model))
    return _CACHE[key]


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def penalised(shape, model, tick, seed, hp, w, call=0, base=None, u0=None):
    """The restatement under hp [H, 6] with weight w: dict(x0, up, xref, hp, w, u, j, xm, info, moved,
    slack); u0: the unconstrained optimum `moved` is judged against."""
    key = ("pen", shape, model, tick, seed, call, _key(base), _key(hp), float(w))
    if key not in _CACHE:
        x0, up, xref = M.inputs(BC.case(shape), tick)
        u, j, xm, info = _cem(shape, model, tick, seed, call, base, hp, w)
        _CACHE[key] = _frozen(dict(x0=x0, up=up, xref=xref, hp=np.array(hp), w=float(w), u=u, j=j, xm=xm, info=info,
                                   model=model, moved=None if u0 is None else not np.array_equal(u, u0),
                                   slack=max_slack_of(hp, xm[:, :2].T)))
    return _CACHE[key]


def funnel(ref0, off):
    """constraints.strip around the unconstrained optimum's Euler positions."""
    from llampc.mpc import constraints
    H = ref0["u"].shape[0]
    return constraints.strip(ref0["xm"][:, :2], HALF, off * np.arange(1, H + 1) / H)


def mixed_problem(shape, p, call=0, base=None, model=None, tick=None, seed=None, var=None):
    """Problem p of the mixed batch: (the unconstrained restatement, the penalised one)."""
    model = BC.MODELS[p] if model is None else model
    tick = BC.TICKS[p] if tick is None else tick
    seed = BC.SEEDS[p] if seed is None else seed
    off, w = variant(p) if var is None else var
    r0 = plain(shape, model, tick, seed, call, base)
    ref = penalised(shape, model, tick, seed, funnel(r0, off), w, call, base, u0=r0["u"])
    ref["slack0"] = max_slack_of(ref["hp"], r0["xm"][:, :2].T)
    return r0, ref


def mixed(shape, B=6):
    """The mixed batch's first solves (call 0, cold): the B penalised restatements."""
    return [mixed_problem(shape, p)[1] for p in range(B)]


def mixed_hp(refs):
    return np.array([r["hp"] for r in refs])


def chain():
    """CHAIN under corridors: slot 0 takes the (+0.05, 1e3) funnel rebuilt per call around the
    unconstrained restatement from the same warm start — the slot's own previous CORRIDOR umpc,
    shifted — slot 1 constraints.disabled(H).  -> per call (slot 0's penalised restatement, slot 1's
    plain restatement of nlp_batch_cases.restate_chain)."""
    outs, base = [], None
    plain_chain = BC.restate_chain()
    for call, (t, models) in enumerate(zip(BC.CHAIN_TICKS, BC.CHAIN_MODELS)):
        _, ref = mixed_problem(BC.CHAIN_SHAPE, 0, call, base, model=models[0], tick=t, seed=BC.CHAIN_SEEDS[0],
                               var=VARIANTS[0])
        outs.append((ref, plain_chain[call][1]))
        base = M.warm(ref["u"])
    return outs


def chunked():
    """CHUNK under the mixed rule: problem p is in launch p // CHUNK_PER_LAUNCH, whose call number that is."""
    return [mixed_problem(BC.CHUNK_SHAPE, p, call=p // BC.CHUNK_PER_LAUNCH)[1] for p in range(BC.CHUNK_B)]


def track():
    return M._env()[1]


def device_margin():
    return float(track().track_width) / 2 - DEVICE_INSET


def device_paths(shape):
    """[6, 2, H+1]: the unconstrained optima's positions."""
    return np.array([plain(shape, m, t, s)["xm"][:, :2].T for m, t, s in zip(BC.MODELS, BC.TICKS, BC.SEEDS)])


def device_host_corridors(shape):
    """constraints.track_corridor along device_paths: what the device builder is compared with."""
    from llampc.mpc import constraints
    key = ("track", shape)
    if key not in _CACHE:
        _CACHE[key] = np.array([constraints.track_corridor(track(), P, device_margin()) for P in device_paths(shape)])
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def device_refs(shape, hp):
    """The restatements under hp [6, H, 6] (the host-built corridors on the CPU, the device-built
    ones' own bits on the GPU) with DEVICE_WEIGHT."""
    out = []
    for p, (m, t, s) in enumerate(zip(BC.MODELS, BC.TICKS, BC.SEEDS)):
        r0 = plain(shape, m, t, s)
        out.append(penalised(shape, m, t, s, hp[p], DEVICE_WEIGHT, u0=r0["u"]))
    return out


def check_problem_conditions(shape, ref, tag="", slack0=True):
    info = ref["info"]
    print(f"{BC.sid(shape)} model {ref['model']}{tag} w {ref['w']:g}: round-0 share {info['share0']:.3f} smallest elite "
          f"gap {info['gap']:.3g} moved {ref['moved']} slack {ref['slack']:.3g} J {ref['j']!r}")
    assert info["share0"] >= SHARE_MIN, info["share0"]
    assert info["gap"] > GAP_MIN, info["gap"]
    if slack0:
        assert ref["slack0"] > SLACK0_MIN, ref["slack0"]


def check_mixed_conditions(shape, refs, moved_min, tag=""):
    for ref in refs:
        check_problem_conditions(shape, ref, tag)
    assert min(r["info"]["share0"] for r in refs) <= SHARE_SOME_MAX
    moved = sum(bool(r["moved"]) for r in refs)
    print(f"{BC.sid(shape)}{tag}: moved {moved} of {len(refs)}")
    assert moved >= moved_min, (moved, moved_min)


def check_device_conditions(shape, refs, tag=""):
    for ref in refs:
        check_problem_conditions(shape, ref, tag, slack0=False)
    assert all(r["moved"] for r in refs), [r["moved"] for r in refs]

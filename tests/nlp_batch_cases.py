"""The batched NLP solve's cases (setupNLPBatch, llampc_nlp_batch_*), shared by
test_nlp_batch_cpu.py (the conditions, on the restatement alone) and test_nlp_batch_gpu.py (the
device against the restatement and against setupNLP).

Bank = generate_bank(12, seed=0).  Six problems: models (0, 3, 3, 7, 11, 5) — one model twice, with
different states — at the DYN-slice ticks (20, 21, 22, 30, 40, 50) (nlp_matrix.inputs), seeds 0..5,
ORCA's bounds, rates and cost otherwise.  The reference of a problem is oracle.nlp_cem with the
problem's OWN bank column as p6 (``restate`` here; nlp_matrix.restate fixes ORCA's parameters),
computed once per (shape, model, tick, seed, call, warm start) and left unchanged.

The smallest adjacent elite-cost gap must stay above nlp_matrix.GAP_MIN = 1e-9 for every compared
solve (``check_conditions``: the device's costs agree with the restatement's to ~1e-15 relative, so
no rank can flip and the bitwise umpc comparison cannot hang on a tie).  Read on the CPU for the
30 (shape, problem) pairs: every gap >= 1.08e-7 (the minimum at (1024, 32, 2, 20), model 0), all
samples finite in every round, the best round varying over 0, 1 and 2."""
import functools

import numpy as np

import nlp_matrix as M
from oracle import llampc_oracle as O

N_BANK = 12
MODELS = (0, 3, 3, 7, 11, 5)
TICKS = (20, 21, 22, 30, 40, 50)
SEEDS = (0, 1, 2, 3, 4, 5)
# (samples, elite, iters, H): one block per problem | four blocks, a pad list, the kept-states
# edge | 16 blocks, the two-level merge, 96 blocks in flight | list length 64, the generic
# completion, unstaged | the first unstaged horizon
SHAPES = [(64, 32, 3, 20), (256, 17, 3, 22), (1024, 32, 2, 20), (128, 64, 2, 40), (64, 8, 2, 29)]
# against the single solver: the first and the third shape
SINGLE_SHAPES = [SHAPES[0], SHAPES[2]]

# warm chains with a changing model: two slots over three ticks; slot 0's model goes 0 -> 3 -> 7,
# slot 1 stays on 11
CHAIN_SHAPE = SHAPES[1]
CHAIN_TICKS = (20, 21, 22)
CHAIN_MODELS = ((0, 11), (3, 11), (7, 11))
CHAIN_SEEDS = (0, 4)

# chunking: five problems, two per launch -> launches of 2, 2, 1 with call numbers 0, 1, 2
CHUNK_SHAPE = SHAPES[0]
CHUNK_B, CHUNK_PER_LAUNCH = 5, 2

# isolation: problem 2's x0[2] is NaN
ISO_SHAPE = SHAPES[1]
ISO_BAD = 2


def sid(shape):
    return M._sid(shape)


def case(shape):
    """The nlp_matrix Case of a shape: ORCA's defaults (bounds, rates, cost, sigma, Ts)."""
    return M.Case("batch-" + sid(shape), shape)


@functools.lru_cache(maxsize=None)
def bank():
    from llampc.mpc import generate_bank
    b = generate_bank(N_BANK, seed=0)
    b.setflags(write=False)
    return b


def p6(model):
    """The model's column of the bank, in oracle.BANK_ORDER (the bank's row order)."""
    return tuple(float(v) for v in bank()[:, model])


def inputs(shape, ticks=TICKS):
    """(x0 [B, 6], uprev [B, 2], xref [B, 2, H+1]) of the problems at their ticks."""
    c = case(shape)
    x0, up, xref = zip(*(M.inputs(c, t) for t in ticks))
    return np.array(x0), np.array(up), np.array(xref)


_CACHE = {}


def restate(shape, model, tick, seed, call=0, base=None, x0_nan=None):
    """oracle.nlp_cem on one problem: dict(x0, up, xref, u [H, 2] or None, j, info)."""
    key = (shape, model, tick, seed, call, None if base is None else np.asarray(base).tobytes(), x0_nan)
    if key in _CACHE:
        return _CACHE[key]
    c = case(shape)
    samples, elite, iters, H = shape
    x0, up, xref = M.inputs(c, tick)
    if x0_nan is not None:
        x0 = x0.copy()
        x0[x0_nan] = np.nan
    m = c.rate_m()
    info = {}
    with np.errstate(all="ignore"):
        u, j = O.nlp_cem(M.shared(), p6(model), x0, xref, up, base, base is not None, H, c.Ts, samples=samples,
                         iters=iters, elite=elite, sigma0=c.sigma, std_floor=c.std_floor, seed=seed, call=call,
                         Q=c.Q, R=c.R, P=c.P, umin=c.umin, umax=c.umax,
                         rate_lo=tuple(None if v is None else -v * c.Ts for v in m),
                         rate_hi=tuple(None if v is None else v * c.Ts for v in m),
                         rate_max_steer=m[1], rate_max_pwm=m[0], info=info)
    out = dict(x0=x0, up=up, xref=xref, u=u, j=j, info=info, model=model)
    if u is not None:
        u.setflags(write=False)
    _CACHE[key] = out
    return out


def restate_batch(shape):
    """The six problems' first solves (call 0, cold)."""
    return [restate(shape, m, t, s) for m, t, s in zip(MODELS, TICKS, SEEDS)]


def restate_chain():
    """CHAIN: per call the two slots' restatements, each slot warm-started from its own previous u
    whatever its model was (call = 0, 1, 2; p6 switching for slot 0)."""
    outs, base = [], [None, None]
    for call, (t, models) in enumerate(zip(CHAIN_TICKS, CHAIN_MODELS)):
        outs.append([restate(CHAIN_SHAPE, models[p], t, CHAIN_SEEDS[p], call, base[p]) for p in range(2)])
        base = [M.warm(r["u"]) for r in outs[-1]]
    return outs


def restate_chunked():
    """CHUNK: problem p is in launch p // CHUNK_PER_LAUNCH, whose call number that is."""
    return [restate(CHUNK_SHAPE, MODELS[p], TICKS[p], SEEDS[p], call=p // CHUNK_PER_LAUNCH) for p in range(CHUNK_B)]


def restate_isolation():
    """ISO: (the first solves with problem ISO_BAD's state NaN, the next solves — call 1, every slot
    warm but ISO_BAD, which failed and starts cold)."""
    first = [restate(ISO_SHAPE, m, t, s, x0_nan=2 if p == ISO_BAD else None)
             for p, (m, t, s) in enumerate(zip(MODELS, TICKS, SEEDS))]
    clean = restate_batch(ISO_SHAPE)
    nxt = [restate(ISO_SHAPE, m, t, s, call=1, base=None if p == ISO_BAD else M.warm(clean[p]["u"]))
           for p, (m, t, s) in enumerate(zip(MODELS, TICKS, SEEDS))]
    return first, nxt


def check_conditions(shape, ref, tag=""):
    """On the restatement alone: every sample finite in every round, the gap above GAP_MIN."""
    info = ref["info"]
    print(f"{sid(shape)} model {ref['model']}{tag}: finite {info['finite']} best round {info['best_round']} "
          f"gap {info['gap']:.3g} fval {ref['j']!r}")
    assert info["finite"] == [shape[0]] * shape[2], info["finite"]
    assert info["gap"] > M.GAP_MIN, info["gap"]


def single_solver(shape, model, seed):
    """setupNLP on the bank's column `model` with `seed`, through its public constructor."""
    from llampc.mpc.nmpc import setupNLP
    c = case(shape)
    samples, elite, iters, H = shape
    mdl = dict(M._env()[0])
    mdl.update(zip(O.BANK_ORDER, p6(model)))
    return setupNLP(H, c.Ts, c.Q, c.P, c.R, M.params(c), mdl, M._env()[1], samples=samples, elite=elite, iters=iters,
                    sigma=c.sigma, std_floor=c.std_floor, seed=seed)


def batch_solver(shape, bank_obj, **kw):
    from llampc.mpc import setupNLPBatch
    c = case(shape)
    samples, elite, iters, H = shape
    return setupNLPBatch(H, c.Ts, c.Q, c.P, c.R, M.params(c), bank_obj, samples=samples, elite=elite, iters=iters,
                         sigma=c.sigma, std_floor=c.std_floor, **kw)

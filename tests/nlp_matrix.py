"""The setupNLP.solve parity matrix's cases, shared by test_nlp_matrix_cpu.py (the conditions, on
the restatement alone) and test_nlp_matrix_gpu.py (the device against the restatement).

A case = a search shape (samples, elite, iters, H) + the cost, bounds, rates, time step and
sampler parameters + a DYN-slice tick (x0 = states[:, tick], uprev = inputs[:, tick - 1], the ETHZ
ConstantSpeed reference built with the case's Ts).  ``restate`` runs oracle.nlp_cem on it once and
caches the result read-only; ``solver`` builds the device solver from the same numbers through
setupNLP's own constructor (ORCA's dict with the case's bounds), so nothing is told to the
restatement that the device was not told through the public interface.

GAP_MIN is the smallest relative gap between adjacent elite costs a case may have on the
restatement (the corridor module's bound): the device's costs agree with the restatement's to
1.1e-15 relative (measured: test_nlp_matrix_gpu.py's docstring), so a gap above 1e-9
cannot flip a rank and the bitwise ``umpc`` comparison cannot hang on a tie.  A case that misses it
at tick 20 / seed 0 got another tick or seed (REPICKED says which and why); the bound and the
comparison stay."""
import functools

import numpy as np

from conftest import golden
from oracle import llampc_oracle as O

GAP_MIN = 1e-9
DEFAULT = (1024, 32, 8, 20)
EYE, ZERO = np.eye(2), np.zeros((2, 2))
R_DIAG = np.diag([5e-3, 1.0])
Q_FULL = np.array([[2.0, 0.3], [0.3, 0.5]])
P_FULL = np.array([[3.0, -0.4], [-0.4, 0.25]])
R_FULL = np.array([[5e-3, 2e-3], [2e-3, 1.0]])
P_TERM = np.diag([3.0, 0.25])


class Case:
    """One configuration of the search; every field has setupNLP's / ORCA's default."""

    def __init__(self, name, shape=DEFAULT, tick=20, Ts=0.02, Q=EYE, R=R_DIAG, P=ZERO, umin=(-0.1, -0.35),
                 umax=(1.0, 0.35), min_rates=(None, -5.0), max_rates=(None, 5.0), sigma=(0.3, 0.15), std_floor=1e-4,
                 seed=0, x0_nan=None, up1=None, finite=None, clip_min=None, gap=True):
        self.name, self.shape, self.tick, self.Ts = name, tuple(shape), tick, Ts
        self.Q, self.R, self.P = (np.asarray(m, dtype=np.float64) for m in (Q, R, P))
        self.umin, self.umax = tuple(umin), tuple(umax)
        self.min_rates, self.max_rates = tuple(min_rates), tuple(max_rates)
        self.sigma, self.std_floor, self.seed = tuple(sigma), std_floor, seed
        self.x0_nan = x0_nan            # index of a component of x0 replaced by NaN
        self.up1 = up1                  # uprev[1] replaced by this value
        self.finite = finite            # the finite objectives every round must count (None: all samples)
        self.clip_min = clip_min        # the least round-0 share of clipped values the case claims
        self.gap = gap                  # False: the case is about equal costs (ties) or has none finite

    @property
    def H(self):
        return self.shape[3]

    def rate_m(self):
        """The symmetric rate bounds m_j = min(-lo, hi) (None: none) that setupNLP enforces."""
        return tuple(None if lo is None else min(-lo, hi) for lo, hi in zip(self.min_rates, self.max_rates))

    def __repr__(self):
        return self.name


def _sid(shape):
    return "x".join(map(str, shape))


# a. selection: every completion path (nlp_complete32 with and without its multi-level Phase B,
#    pad lists, nlp_complete with and without its merge tree, staged and unstaged)
SELECTION = [Case("sel-" + _sid(s), s) for s in [
    (128, 32, 3, 20), (2048, 32, 2, 20), (2048, 1, 2, 20), (4096, 20, 2, 20), (64, 64, 3, 20), (256, 33, 3, 20),
    (512, 64, 3, 40), (2048, 32, 2, 40), (4096, 32, 2, 64)]]
REFUSED_SHAPE = (4096, 64, 2, 64)       # 230 KiB of LDS: LLAMPC_E_ARG at create

# b. horizon edges: the rate chain's batches of 8 and tail, kept states (22 / 23), staged / unstaged
#    (28 / 29), the completion's second column pass (33), H = 1 and LLAMPC_HMAX
H_EDGES = (1, 2, 7, 8, 9, 22, 23, 28, 29, 32, 33, 64)
# H = 1 at tick 20, seed 0 has a gap of 5.2e-11 (one-step sequences, most of them clipped to the
# same corner, whose costs differ in the last bits; seeds 0..39 at tick 20 all stay below 1e-9):
# tick 10, seed 5 reads 1.06e-8 (see REPICKED)
HORIZON = [Case(f"H{H}", (256, 17, 3, H), **(dict(tick=10, seed=5) if H == 1 else {})) for H in H_EDGES]

# c. cost: full matrices (off-diagonal Q, R, P and a terminal term), staged and unstaged; the
#    terminal term alone
COST = [Case("full-H20", Q=Q_FULL, P=P_FULL, R=R_FULL),
        Case("full-H40", (512, 32, 3, 40), Q=Q_FULL, P=P_FULL, R=R_FULL), Case("terminal-only", Q=ZERO, P=P_TERM)]

# d. bounds and time step
ASYM = Case("rates-asym-3+5", min_rates=(None, -3.0), max_rates=(None, 5.0))
SYM3 = Case("rates-sym-3", min_rates=(None, -3.0), max_rates=(None, 3.0))
FAIL_BOUNDS = Case("infeasible-uprev", umin=(-0.1, -0.1), umax=(1.0, 0.1), finite=0, gap=False)
FAIL_NAN = Case("nan-x0", x0_nan=2, finite=0, gap=False)
BOUNDS = [Case("Ts0.01", Ts=0.01), Case("Ts0.05", Ts=0.05),
          Case("pwm-rate", min_rates=(-2.0, -5.0), max_rates=(2.0, 5.0), clip_min=0.3),
          Case("no-rates", min_rates=(None, None), max_rates=(None, None)),
          Case("tight-bounds", umin=(0.8, 0.2), umax=(1.0, 0.3), seed=4, clip_min=0.3),
          Case("uprev-outside", umin=(-0.1, -0.2), umax=(1.0, 0.2)), ASYM, SYM3]

# e. sampler parameters: the Philox key's high word, another spread, no floor
SAMPLER = [Case("sampler", seed=2 ** 32 + 7, sigma=(0.1, 0.05), std_floor=0.0)]

# f. ties: every objective exactly 0, the index alone ranks
TIES = [Case("ties-" + _sid(s), s, Q=ZERO, R=ZERO, P=ZERO, gap=False) for s in [(1024, 32, 3, 20), (512, 64, 3, 40)]]

# g. modes x shapes: three warm-started solves at ticks 20, 21, 22
MODE_SHAPES = [(512, 64, 3, 40), (2048, 32, 2, 20), (256, 17, 3, 22)]
MODE_TICKS = (20, 21, 22)

# h. result owner: the best from the last round (tick 20: round 7) and from an earlier one (tick 40: 0)
OWNER = [(Case("owner-last", tick=20), 7), (Case("owner-early", tick=40), 0)]

# i. the failure contract's two triggers
FAILURES = [FAIL_BOUNDS, FAIL_NAN]
# The feasible tick-20 solve that follows on the same solver: call 1, no warm start
# (restate(.., call=1)).  After the NaN state: the plain inputs.  The infeasible-uprev solver keeps
# its bounds of +-0.1 (they are fixed at create), under which tick 20's own uprev[1] = 0.279 fails
# again, so its next solve takes uprev[1] = 0.05, inside them.
AFTER_FAILURE = {"infeasible-uprev": Case("after-infeasible-uprev", umin=(-0.1, -0.1), umax=(1.0, 0.1), up1=0.05),
                 "nan-x0": Case("after-nan-x0")}

SINGLE = SELECTION + HORIZON + COST + BOUNDS + SAMPLER + [c for c, _ in OWNER]

# cases whose inputs are not tick 20 / seed 0 because the restatement misses GAP_MIN there
REPICKED = {"H1": "tick 20, seed 0: gap 5.2e-11 < 1e-9 -> tick 10, seed 5: 1.06e-8",
            "tight-bounds": "seed 0: gap 1.42e-9, 1.4 x the bound -> seed 4: 7.0e-8 (the clip share stays 0.75)"}


def shared():
    p = O.orca_params()
    return {k: p[k] for k in ("lf", "lr", "mass", "Iz", "Cm1", "Cm2", "Cr0", "Cr2")}


@functools.lru_cache(maxsize=None)
def _env():
    from llampc.params import ORCA
    from llampc.tracks import ETHZ
    p = ORCA(control="pwm")
    return p, ETHZ('optimal', True), tuple(p[k] for k in O.BANK_ORDER)


def params(case):
    """ORCA's dict with the case's bounds and rates (what setupNLP reads them from)."""
    p = dict(_env()[0])
    p["min_inputs"], p["max_inputs"] = list(case.umin), list(case.umax)
    p["min_rates"], p["max_rates"] = list(case.min_rates), list(case.max_rates)
    return p


def solver(case):
    from llampc.models import Dynamic
    from llampc.mpc.nmpc import setupNLP
    samples, elite, iters, H = case.shape
    return setupNLP(H, case.Ts, case.Q, case.P, case.R, params(case), Dynamic(**_env()[0]), _env()[1],
                    samples=samples, elite=elite, iters=iters, sigma=case.sigma, std_floor=case.std_floor,
                    seed=case.seed)


@functools.lru_cache(maxsize=None)
def _inputs(tick, H, Ts):
    from llampc.mpc.planner import ConstantSpeed
    d = golden("dyn_slice.npz")
    x0, up = d["states"][:, tick].copy(), d["inputs"][:, tick - 1].copy()
    xref, _, _ = ConstantSpeed(x0[:2], x0[3], _env()[1], H, Ts, 0)
    xref = np.ascontiguousarray(xref[:2])
    for a in (x0, up, xref):
        a.setflags(write=False)
    return x0, up, xref


def inputs(case, tick=None):
    """(x0, uprev, xref [2, H+1]) of the case at its tick (or another), read-only."""
    x0, up, xref = _inputs(case.tick if tick is None else tick, case.H, case.Ts)
    if case.x0_nan is not None:
        x0 = x0.copy()
        x0[case.x0_nan] = np.nan
        x0.setflags(write=False)
    if case.up1 is not None:
        up = np.array([up[0], case.up1])
        up.setflags(write=False)
    return x0, up, xref


_CACHE = {}


def restate(case, tick=None, call=0, base=None):
    """oracle.nlp_cem on the case: dict(x0, up, xref, u [H, 2] or None, j, info), computed once per
    (case, tick, call, warm start) and left unchanged.  base: the warm start [H, 2] (the held uprev
    is then round 0's sample 1), None: the first solve."""
    key = (case.name, tick, call, None if base is None else np.asarray(base).tobytes())
    if key in _CACHE:
        return _CACHE[key]
    samples, elite, iters, H = case.shape
    x0, up, xref = inputs(case, tick)
    m = case.rate_m()
    info = {}
    with np.errstate(all="ignore"):     # the NaN state's rollout
        u, j = O.nlp_cem(shared(), _env()[2], x0, xref, up, base, base is not None, H, case.Ts, samples=samples,
                         iters=iters, elite=elite, sigma0=case.sigma, std_floor=case.std_floor, seed=case.seed,
                         call=call, Q=case.Q, R=case.R, P=case.P, umin=case.umin, umax=case.umax,
                         rate_lo=tuple(None if v is None else -v * case.Ts for v in m),
                         rate_hi=tuple(None if v is None else v * case.Ts for v in m),
                         rate_max_steer=m[1], rate_max_pwm=m[0], info=info)
    out = dict(x0=x0, up=up, xref=xref, u=u, j=j, info=info)
    if u is not None:
        u.setflags(write=False)
    _CACHE[key] = out
    return out


def warm(u):
    """The next solve's warm start: the last solution shifted one step."""
    return np.concatenate([u[1:], u[-1:]])


def restate_chain(case, ticks=MODE_TICKS):
    """Successive warm-started solves (call = 0, 1, ..) at the ticks: the list of restate()s."""
    outs, base = [], None
    for call, t in enumerate(ticks):
        outs.append(restate(case, t, call, base))
        base = warm(outs[-1]["u"])
    return outs


def check_conditions(case, ref):
    """On the restatement alone: the case can neither pass vacuously nor fail on a rank flip."""
    info = ref["info"]
    print(f"{case.name}: finite {info['finite']} best round {info['best_round']} sample {info['best_sample']} "
          f"clip share {info['clip0']:.3f} gap {info['gap']:.3g} fval {ref['j']!r}")
    want = case.shape[0] if case.finite is None else case.finite
    assert info["finite"] == [want] * case.shape[2], info["finite"]
    if case.gap:
        assert info["gap"] > GAP_MIN, info["gap"]
    if case.clip_min is not None:
        assert info["clip0"] >= case.clip_min, info["clip0"]

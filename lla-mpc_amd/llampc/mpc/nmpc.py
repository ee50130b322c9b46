"""``setupNLP`` drop-in: the selected model's NMPC solved on the GPU by a cross-entropy search.

The reference (llampc/mpc/nmpc.py:14-203) transcribes the problem for CasADi/IPOPT:
states x[6, H+1] with x_{k+1} = x_k + Ts f_nlp(x_k, u_k) (dynamic.py:195-226 +
nmpc.py:58-60), objective (x_H - xref_H)' P (.) + sum_k [(x_{k+1} - xref_{k+1})' Q (.) +
du_k' R du_k], du_0 = u_0 - uprev (nmpc.py:44-111), bounds on u and on the steering rate
(nmpc.py:102-105).  CasADi and IPOPT are not available on this platform (and IPOPT's optimum
is not reproducible here: parity unpinned), so this ``solve()`` keeps the
interface and the problem and minimises it on the device (llampc_nlp_solve, csrc/nlp.hip):
``iters`` rounds of ``samples`` control sequences drawn around the current mean (the warm
start first: the previous solution shifted one step; the held uprev is a candidate of the
first round) with a per-(step, input) spread, clipped to the bounds and rate-clipped in order,
every one rolled out with the NLP's own Euler transcription and scored with its objective
(infeasible: +inf); the ``elite`` best set the next mean and spread (the cross-entropy
method).  All rounds run in ONE launch on the GPU (the sample blocks wait for each round's
mean and spread), the result comes back through pinned host memory.  Every returned
``umpc`` satisfies the NLP's bounds and rate constraints; ``fval`` is the objective of
``umpc`` and ``xmpc`` its Euler trajectory — the same triple IPOPT's feasible point would give.

Rate bounds are symmetric on the device: ``params["min_rates"][j]`` = lo and ``["max_rates"][j]``
= hi (both None: no bound on input j) are enforced as |u_k - u_{k-1}| <= m Ts with m = min(-lo, hi),
by the rate chain and by the feasibility test alike.  An asymmetric pair is therefore solved on
its tighter symmetric side (a subset of the NLP's feasible set): (-3, +5) rad/s gives the ±3
rad/s solve.  (Until the chain and the test shared the bound, the chain clipped to [lo, hi] Ts and
every sample it left beyond m Ts was scored +inf: the search all but stopped sampling.)

A *corridor* keeps the search on the track: ``solve(x0, xref, uprev, corridor=hp)`` with ``hp``
[H, 6], row k - 1 = (a0, a1, b, c0, c1, d) the half-planes a.p_k <= b and c.p_k <= d on the
position p_k after k Euler steps (a = 0, b = +inf disables one).  Every sample's objective gains
``corridor_weight`` x sum_k max(a.p_k - b, 0)^2 + max(c.p_k - d, 0)^2 (a soft constraint, evaluated
in the rollout on the device: llampc_nlp_solve_corridor); ``fval`` includes it, and the fourth
return value is ``Ts`` if the largest slack along ``xmpc`` (``self.max_slack``) exceeds
``corridor_tol`` (1e-4, IPOPT's constr_viol_tol), else 0.0.  ``llampc.mpc.constraints`` builds
corridors: ``track_corridor(track, xref)`` from a track's centre line and width, ``strip`` around
any polyline.  ``corridor=None`` is the unconstrained solve, unchanged.

``setupNLP(..., device_corridor=True, corridor_margin=m)`` builds the track's corridor on the
device instead (llampc_nlp_solve_track: a small kernel ahead of the search on the same stream,
csrc/corridor_dev.hpp — ``track_corridor`` in scalar form, equal to it to 1e-12; the host
function's Python loop costs milliseconds per tick).  The track's centre line, arc lengths, length
and width are uploaded once; a solve without ``corridor=`` then takes the corridor along
``corridor_path`` [2, H+1] if given, else along ``constraints.default_path``: the previous solve's
positions shifted one step, or on the first solve the ray from the car (which leaves the track at
a long horizon with a spinning car: pass ``corridor_path`` then).  ``last_corridor`` is a copy of
the half-planes the device built; ``max_slack`` and the violation flag are as for ``corridor=``,
which still wins when given.  ``track_corridor(path)`` is the device builder alone.

``track_cons=True`` (rt.py:63 uses False everywhere) would add the track-boundary half-planes
of constraints.py with the reference's own linearisation and slack variables, which cannot be
restated here (constraints.py is not available): it raises, and points to
``corridor=``.
"""
from __future__ import annotations

import numpy as np

from llampc import _native as nat
from llampc.mpc import constraints
from llampc.mpc.bank import ModelBank, SHARED_KEYS

_PACEJKA = ("Bf", "Cf", "Df", "Br", "Cr", "Dr")


def _attr(model, k, default=None):
    if isinstance(model, dict):
        return model.get(k, default)
    return getattr(model, k, default)


def _bounds_cost(params, Ts, Q, R, P):
    """(umin, umax, rate, cost) as the solvers read them from ``params``: the input bounds, the
    per-step rate bounds [(lo Ts, hi Ts) or (None, None)] and the llampc_cost."""
    umin = np.asarray(params["min_inputs"], dtype=np.float64)
    umax = np.asarray(params["max_inputs"], dtype=np.float64)
    # rate bounds min_rates[j]*Ts <= d u_j <= max_rates[j]*Ts (nmpc.py:104-105: the steering
    # rate; ORCA leaves the pwm rate None, unconstrained).  The kernel's feasibility test is
    # symmetric, |du| <= rate_max*Ts: an asymmetric pair is narrowed to its tighter side
    # m = min(-lo, hi), and the rate chain clips to the same [-m, +m]*Ts — every sample it
    # produces is then feasible by construction (module doc).
    rate_max = tuple(-1.0 if lo is None else min(-float(lo), float(hi))
                     for lo, hi in zip(params["min_rates"], params["max_rates"]))
    if any(lo is not None and not m >= 0 for m, lo in zip(rate_max, params["min_rates"])):
        raise ValueError("min_rates must be <= 0 <= max_rates (the symmetric rate bound min(-lo, hi))")
    rate = [(None, None) if m < 0 else (-m * Ts, m * Ts) for m in rate_max]
    cost = nat.cost_struct(Q=Q, R=R, P=P, umin=umin, umax=umax, rate_max=rate_max, enforce_bounds=True)
    return umin, umax, rate, cost


def _nlp_cfg(s):
    """llampc_nlp_cfg of a solver object (its horizon, samples, iters, elite, Ts, std_floor, seed,
    sigma, cost and rate)."""
    cfg = nat.NlpCfg()
    cfg.H, cfg.samples, cfg.iters, cfg.elite = s.horizon, s.samples, s.iters, s.elite
    cfg.Ts, cfg.std_floor, cfg.seed = s.Ts, s.std_floor, s.seed
    cfg.sigma0[0], cfg.sigma0[1] = float(s.sigma[0]), float(s.sigma[1])
    cfg.cost = s.cost
    for j, (lo, hi) in enumerate(s.rate):
        cfg.rate_lo[j], cfg.rate_hi[j] = (1.0, -1.0) if lo is None else (lo, hi)
    return cfg


class setupNLP:
    """Same constructor and ``solve`` contract as nmpc.py:14-203 (see module doc)."""

    def __init__(self, horizon, Ts, Q, P, R, params, model, track, track_cons=False,
                 samples=1024, iters=8, elite=32, sigma=(0.3, 0.15), std_floor=1e-4, seed=0, device=0,
                 corridor_weight=1e4, corridor_tol=1e-4, device_corridor=False, corridor_margin=0.0):
        if track_cons:
            raise NotImplementedError("track_cons=True (constraints.py boundary half-planes) is not "
                                      "implemented: the reference's LLA-MPC runs use TRACK_CONS=False (rt.py:63); "
                                      "pass solve(..., corridor=llampc.mpc.constraints.track_corridor(track, xref)) "
                                      "for soft track half-planes in the device search")
        self.corridor_weight, self.corridor_tol = float(corridor_weight), float(corridor_tol)
        if not (np.isfinite(self.corridor_weight) and self.corridor_weight >= 0):
            raise ValueError("corridor_weight must be finite and >= 0")
        self.max_slack = 0.0         # the last corridor solve's largest slack along xmpc
        self.device_corridor, self.corridor_margin = bool(device_corridor), float(corridor_margin)
        if self.device_corridor:
            constraints.require_track(track, "device_corridor=True")
            constraints.require_margin(track, corridor_margin)
        self.last_corridor = None    # the last device-built corridor [H, 6]
        self._last_xmpc = None       # the last solve's positions [2, H+1] (constraints.default_path)
        self.horizon, self.Ts = int(horizon), float(Ts)
        self.params, self.model, self.track, self.track_cons = params, model, track, track_cons
        self.samples, self.iters, self.elite = int(samples), int(iters), int(elite)
        self.sigma = np.asarray(sigma, dtype=np.float64)
        self.std_floor, self.seed, self.device = float(std_floor), int(seed), device
        self.umin, self.umax, self.rate, self.cost = _bounds_cost(params, self.Ts, Q, R, P)
        self._bank = None
        self._h = None
        self._dyn = None
        self._last = None            # previous umpc [H, 2] for the warm start

    # the device objects are created at the first solve(): rt.py builds one setupNLP per
    # bank model (rt.py:195-202) but solves with one of them per tick
    def _ensure(self):
        if self._h is not None:
            return
        m = self.model
        p6 = np.array([[float(_attr(m, k))] for k in _PACEJKA])
        shared = {k: float(_attr(m, k, 0.0) or 0.0) for k in SHARED_KEYS}
        approx = any(_attr(m, k) is None for k in ("Bf", "Br", "Df", "Dr")) or bool(_attr(m, "approx", False))
        if approx:
            p6 = np.nan_to_num(p6)
        self._bank = ModelBank(p6, shared=shared, W=1, device=self.device,
                               input_acc=bool(_attr(m, "input_acc", False)), approx=approx)
        cfg = _nlp_cfg(self)
        h = nat.C.c_void_p()
        nat.check(nat.load().llampc_nlp_create(self._bank.handle, nat.C.byref(cfg), nat.C.byref(h)))
        self._h = h
        self.cfg = cfg
        H = self.horizon
        self._io = {"x0": np.zeros(6), "xref": np.zeros((2, H + 1)), "up": np.zeros(2), "base": np.zeros((H, 2)),
                    "umpc": np.zeros((H, 2)), "fval": np.zeros(1), "xmpc": np.zeros((H + 1, 6)),
                    "hp": np.zeros((H, 6)), "slack": np.zeros(1), "path": np.zeros((2, H + 1)),
                    "theta": np.zeros(H)}
        self._addr = {k: v.ctypes.data for k, v in self._io.items()}
        if self.device_corridor:
            centre, theta, length, width = constraints.track_tables(self.track)
            nat.check(nat.load().llampc_nlp_set_track(h, centre.ctypes.data, theta.ctypes.data, centre.shape[1],
                                                      length, width))

    def _path(self, path):
        """A corridor path as the library takes it: [2, H+1], finite (checked before the library)."""
        path = np.asarray(path, dtype=np.float64)
        if path.shape != (2, self.horizon + 1):
            raise ValueError(f"corridor_path must be [2, H+1] = {(2, self.horizon + 1)}, got {path.shape}")
        if not np.all(np.isfinite(path)):
            raise ValueError("corridor_path must be finite")
        return path

    def track_corridor(self, path, margin=None):
        """The track's corridor along ``path`` [2, H+1] built on the device
        (llampc_nlp_track_corridor): -> (hp [H, 6], theta [H]), constraints.track_corridor(track,
        path, margin) and track.xy_to_param of the path's points to 1e-12.  margin: None =
        corridor_margin.  Needs device_corridor=True."""
        if not self.device_corridor:
            raise ValueError("track_corridor needs setupNLP(..., device_corridor=True)")
        path = self._path(path)
        self._ensure()
        b, a = self._io, self._addr
        b["path"][:] = path
        m = self.corridor_margin if margin is None else float(margin)
        nat.check(nat.load().llampc_nlp_track_corridor(self._h, a["path"], m, a["hp"], a["theta"]))
        return b["hp"].copy(), b["theta"].copy()

    def solve(self, x0, xref, uprev, corridor=None, corridor_path=None):
        """-> (umpc [2, H], fval, xmpc [6, H+1], violation in {0, Ts}) as nmpc.py:161-203.
        corridor: None, or the half-planes [H, 6] (module doc); violation is then Ts if the largest
        slack along xmpc exceeds corridor_tol.  With device_corridor=True and no corridor: the
        track's corridor along corridor_path [2, H+1], or along constraints.default_path."""
        if corridor is not None:
            corridor = np.asarray(corridor, dtype=np.float64)
            if corridor.shape != (self.horizon, 6):
                raise ValueError(f"corridor must be [H, 6] = {(self.horizon, 6)}, got {corridor.shape}")
        elif corridor_path is not None:
            if not self.device_corridor:
                raise ValueError("corridor_path needs setupNLP(..., device_corridor=True)")
            corridor_path = self._path(corridor_path)
        self._ensure()
        b = self._io
        H = self.horizon
        # the inputs into the persistent buffers (their addresses cached at the first solve: the
        # per-call ctypes pointer objects cost more host time than the copies)
        b["x0"][:] = np.asarray(x0, dtype=np.float64).ravel()
        b["xref"][:] = np.asarray(xref, dtype=np.float64)[:2, :H + 1]
        b["up"][:] = np.asarray(uprev, dtype=np.float64).ravel()
        hold = self._last is not None
        if hold:                         # the warm start: the last solution shifted one step
            b["base"][:-1] = self._last[1:]
            b["base"][-1] = self._last[-1]
        a = self._addr
        violation = 0.0
        if corridor is None and self.device_corridor:
            if corridor_path is None:
                corridor_path = constraints.default_path(b["x0"], H, self.Ts, self._last_xmpc)
            b["path"][:] = corridor_path
            nat.check(nat.load().llampc_nlp_solve_track(self._h, a["x0"], a["xref"], a["up"],
                                                         a["base"] if hold else None, int(hold), a["path"],
                                                         self.corridor_margin, self.corridor_weight, a["umpc"],
                                                         a["fval"], a["xmpc"], a["slack"], a["hp"]))
            self.last_corridor = b["hp"].copy()
            self.max_slack = float(b["slack"][0])
            violation = self.Ts if self.max_slack > self.corridor_tol else 0.0
        elif corridor is None:
            nat.check(nat.load().llampc_nlp_solve(self._h, a["x0"], a["xref"], a["up"], a["base"] if hold else None,
                                                   int(hold), a["umpc"], a["fval"], a["xmpc"]))
        else:
            b["hp"][:] = corridor
            nat.check(nat.load().llampc_nlp_solve_corridor(self._h, a["x0"], a["xref"], a["up"],
                                                            a["base"] if hold else None, int(hold), a["hp"],
                                                            self.corridor_weight, a["umpc"], a["fval"], a["xmpc"],
                                                            a["slack"]))
            self.max_slack = float(b["slack"][0])
            violation = self.Ts if self.max_slack > self.corridor_tol else 0.0
        umpc = b["umpc"].copy()
        self._last = umpc
        xmpc = b["xmpc"].T.copy()
        if self.device_corridor:
            self._last_xmpc = xmpc[:2].copy()
        return umpc.T.copy(), float(b["fval"][0]), xmpc, violation

    def close(self):
        if self._h is not None:
            nat.load().llampc_nlp_destroy(self._h)
            self._h = None
        if self._bank is not None:
            self._bank.close()
            self._bank = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class setupNLPBatch:
    """One solver bound to a whole ``ModelBank``: ``solve`` runs B independent NMPC problems, each
    with its own bank model (by index), state, reference, previous input, warm start and noise
    seed, in ONE launch (llampc_nlp_batch_solve, csrc/nlp_batch.hip), each on its own samples / 64
    blocks.  The reference builds one setupNLP per bank model (rt.py:195-202) and solves with the
    one the look-back selected (rt.py:305); here the index from ``plan()`` / ``LLAMPC.tick`` (and
    the top-K's, or a second track's car) goes straight into ``models``.

    A problem's search is ``setupNLP.solve``'s bit for bit: problem p of the solver's c-th launch
    equals the c-th solve of a ``setupNLP`` built on bank column ``models[p]`` with ``seeds[p]``.

    ``bank`` is borrowed (``close()`` leaves it open; close the solver first).  Bounds and rates are
    read from ``params`` as setupNLP reads them.  **Slot p is a car, not a model**: slot p's warm
    start is slot p's previous ``umpc`` shifted one step, whatever model it uses this time; a slot
    whose last solve failed, or that ``reset`` dropped, starts cold.

    The problems' blocks wait for each other's rounds, so a launch of B problems needs (and holds
    for the solve's duration) B x samples / 64 CUs: ``max_batch`` x samples / 64 must not exceed the
    device's CU count (refused at construction), and a ``solve`` of more than ``max_batch`` problems
    or of more than ``max_resident`` blocks (default: the CU count; lower it for co-tenants) is
    issued as consecutive launches of as many problems as fit.  Chunking changes no result bit of a
    first solve; each chunk consumes one solve number (the Philox call word), and the chunk counts
    follow from the shapes alone, so call numbers stay deterministic: problem p of a chunked solve
    is in chunk p // per_launch, whose number is the count of launches before it.

    Corridors (module doc) are per problem: ``solve(..., corridor=hp [B, H, 6], corridor_weight=w [B])``
    keeps the batch one launch, every problem with its own half-planes and weight
    (csrc/nlp_batch_corr.hip).  ``setupNLPBatch(..., track=t, device_corridor=True,
    corridor_margin=m)`` builds the track's corridors on the device along ``corridor_path``
    [B, 2, H+1] (one kernel of B x H blocks ahead of the search on the same stream), and
    ``track_corridor(paths)`` is that builder alone.  One track per solver: cars on two tracks take
    two solvers, or host-built ``corridor=``.  The horizon is at most LLAMPC_HMAX = 64."""

    def __init__(self, horizon, Ts, Q, P, R, params, bank, max_batch=8, samples=1024, iters=8, elite=32,
                 sigma=(0.3, 0.15), std_floor=1e-4, seed=0, max_resident=None, *, track=None, corridor_weight=1e4,
                 corridor_tol=1e-4, device_corridor=False, corridor_margin=0.0):
        if not isinstance(bank, ModelBank):
            raise TypeError("bank must be a ModelBank")
        self.horizon, self.Ts = int(horizon), float(Ts)
        if not 1 <= self.horizon <= nat.HMAX:
            raise ValueError(f"horizon must lie in [1, {nat.HMAX}], got {horizon}")
        self.corridor_weight, self.corridor_tol = float(corridor_weight), float(corridor_tol)
        if not (np.isfinite(self.corridor_weight) and self.corridor_weight >= 0):
            raise ValueError("corridor_weight must be finite and >= 0")
        self.track = track
        self.device_corridor, self.corridor_margin = bool(device_corridor), float(corridor_margin)
        if self.device_corridor:
            constraints.require_track(track, "device_corridor=True")
            constraints.require_margin(track, corridor_margin)
        self.max_slack = None        # the last corridor solve's largest slack along each xmpc [B]
        self.violation = None        # ... Ts where it exceeds corridor_tol, else 0.0 [B]
        self.last_corridor = None    # the last device-built corridors [B, H, 6]
        self._last_xmpc = {}         # slot -> its last solve's positions [2, H+1] (constraints.default_path)
        self.params, self.bank, self.max_batch = params, bank, int(max_batch)
        self.samples, self.iters, self.elite = int(samples), int(iters), int(elite)
        self.sigma = np.asarray(sigma, dtype=np.float64)
        self.std_floor, self.seed = float(std_floor), int(seed)
        self.umin, self.umax, self.rate, self.cost = _bounds_cost(params, self.Ts, Q, R, P)
        self._h = None
        self.cfg = _nlp_cfg(self)
        h = nat.C.c_void_p()
        nat.check(nat.load().llampc_nlp_batch_create(bank.handle, nat.C.byref(self.cfg), self.max_batch,
                                                     nat.C.byref(h)))
        self._h = h
        cus = nat.C.c_int32()
        nat.check(nat.load().llampc_nlp_batch_info(h, None, nat.C.byref(cus)))
        self.cus = cus.value
        self.max_resident = self.cus if max_resident is None else int(max_resident)
        nl = self.samples // 64
        if self.max_resident < nl:
            self.close()
            raise ValueError(f"max_resident={self.max_resident} holds no problem ({nl} blocks each)")
        self.per_launch = min(self.max_batch, self.max_resident // nl)     # problems per launch
        self._last = {}              # slot -> previous umpc [H, 2] (absent: cold)
        if self.device_corridor:
            centre, theta, length, width = constraints.track_tables(track)
            try:
                nat.check(nat.load().llampc_nlp_batch_set_track(h, centre.ctypes.data, theta.ctypes.data,
                                                                centre.shape[1], length, width))
            except Exception:
                self.close()
                raise

    def reset(self, slots=None):
        """Drops the warm starts (and the default corridor paths) of ``slots`` (None: all)."""
        if slots is None:
            self._last.clear()
            self._last_xmpc.clear()
        else:
            for p in slots:
                self._last.pop(int(p), None)
                self._last_xmpc.pop(int(p), None)

    def _paths(self, paths, B):
        """Corridor paths as the library takes them: [B, 2, H+1], finite (checked before the library)."""
        H = self.horizon
        paths = np.ascontiguousarray(paths, dtype=np.float64)
        if paths.shape != (B, 2, H + 1):
            raise ValueError(f"corridor_path must be [B, 2, H+1] = {(B, 2, H + 1)}, got {paths.shape}")
        if not np.all(np.isfinite(paths)):
            raise ValueError("corridor_path must be finite")
        return paths

    def track_corridor(self, paths, margin=None):
        """The track's corridors along ``paths`` [B, 2, H+1] built on the device
        (llampc_nlp_batch_track_corridor, chunks of max_batch): -> (hp [B, H, 6], theta [B, H]), each
        problem's constraints.track_corridor(track, paths[p], margin) and track.xy_to_param of its
        points to 1e-12.  margin: None = corridor_margin.  Needs device_corridor=True."""
        if not self.device_corridor:
            raise ValueError("track_corridor needs setupNLPBatch(..., device_corridor=True)")
        if self._h is None:
            raise nat.NativeError("solver is closed")
        paths = np.asarray(paths, dtype=np.float64)
        if paths.ndim != 3:
            raise ValueError(f"paths must be [B, 2, H+1], got {paths.shape}")
        B, H = paths.shape[0], self.horizon
        paths = self._paths(paths, B)
        m = self.corridor_margin if margin is None else float(margin)
        constraints.require_margin(self.track, m)
        hp, theta = np.zeros((B, H, 6)), np.zeros((B, H))
        for lo in range(0, B, self.max_batch):
            hi = min(B, lo + self.max_batch)
            nat.check(nat.load().llampc_nlp_batch_track_corridor(self._h, hi - lo, paths[lo:hi].ctypes.data, m,
                                                                 hp[lo:hi].ctypes.data, theta[lo:hi].ctypes.data))
        return hp, theta

    def solve(self, models, x0, xref, uprev, seeds=None, corridor=None, corridor_weight=None, corridor_path=None):
        """models [B] bank indices, x0 [B, 6], xref [B, 2, H+1] (or [2, H+1] shared), uprev [B, 2],
        seeds [B] (None: the solver's seed for all) -> (umpc [B, 2, H], fval [B], xmpc [B, 6, H+1],
        ok [B]).  A problem that found no finite objective, or whose completion never arrived, has
        ok False, umpc zeros and fval inf, and does not disturb the others.

        corridor: None, or the problems' half-planes [B, H, 6] ([H, 6]: shared; a problem that wants
        none takes constraints.disabled(H)), each with its own corridor_weight (a scalar or [B];
        None: the solver's) — still one launch (llampc_nlp_batch_solve_corridor); problem p is then
        setupNLP.solve(..., corridor=corridor[p]) with that weight, bit for bit.  With
        device_corridor=True and no corridor: the track's corridors, built on the device ahead of
        the search (llampc_nlp_batch_solve_track), along corridor_path [B, 2, H+1], or per slot along
        constraints.default_path (the slot's previous xmpc shifted one step; the ray from the car on
        a cold slot).  After a corridor solve: max_slack [B], violation [B] (Ts where the slack
        exceeds corridor_tol, else 0.0; both 0 for a failed problem) and, device-built,
        last_corridor [B, H, 6]."""
        if self._h is None:
            raise nat.NativeError("solver is closed")
        H = self.horizon
        models = np.ascontiguousarray(models, dtype=np.int64)
        if models.ndim != 1 or models.size < 1:
            raise ValueError(f"models must be a non-empty 1-d sequence of bank indices, got shape {models.shape}")
        B = models.size
        if np.any(models < 0) or np.any(models >= self.bank.n):
            raise ValueError(f"models must lie in [0, {self.bank.n}), got {models.tolist()}")
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x0.shape != (B, 6):
            raise ValueError(f"x0 must be [B, 6] = {(B, 6)}, got {x0.shape}")
        xref = np.asarray(xref, dtype=np.float64)
        if xref.shape == (2, H + 1):
            xref = np.broadcast_to(xref, (B, 2, H + 1))
        if xref.shape != (B, 2, H + 1):
            raise ValueError(f"xref must be [B, 2, H+1] = {(B, 2, H + 1)} or [2, H+1], got {xref.shape}")
        xref = np.ascontiguousarray(xref)
        uprev = np.ascontiguousarray(uprev, dtype=np.float64)
        if uprev.shape != (B, 2):
            raise ValueError(f"uprev must be [B, 2] = {(B, 2)}, got {uprev.shape}")
        if seeds is None:
            seeds = np.full(B, self.seed, dtype=np.uint64)
        else:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
            if seeds.shape != (B,):
                raise ValueError(f"seeds must be [B] = {(B,)}, got {seeds.shape}")
        # the corridor's arguments: all checked before anything is launched
        paths = None
        if corridor is not None:
            corridor = np.asarray(corridor, dtype=np.float64)
            if corridor.shape == (H, 6):
                corridor = np.broadcast_to(corridor, (B, H, 6))
            if corridor.shape != (B, H, 6):
                raise ValueError(f"corridor must be [B, H, 6] = {(B, H, 6)} or [H, 6], got {corridor.shape}")
            corridor = np.ascontiguousarray(corridor)
        elif corridor_path is not None:
            if not self.device_corridor:
                raise ValueError("corridor_path needs setupNLPBatch(..., track=..., device_corridor=True)")
            paths = self._paths(corridor_path, B)
        elif self.device_corridor:
            paths = self._paths([constraints.default_path(x0[p], H, self.Ts, self._last_xmpc.get(p))
                                 for p in range(B)], B)
        with_corridor = corridor is not None or paths is not None
        if with_corridor or corridor_weight is not None:
            w = self.corridor_weight if corridor_weight is None else corridor_weight
            w = np.asarray(w, dtype=np.float64)
            if w.shape == ():
                w = np.broadcast_to(w, (B,))
            if w.shape != (B,):
                raise ValueError(f"corridor_weight must be a scalar or [B] = {(B,)}, got {w.shape}")
            if not (np.all(np.isfinite(w)) and np.all(w >= 0)):
                raise ValueError("corridor_weight must be finite and >= 0")
            weights = np.ascontiguousarray(w)
        hold = np.array([p in self._last for p in range(B)], dtype=np.int32)
        base = np.zeros((B, H, 2))
        for p in range(B):
            if hold[p]:                  # the warm start: the slot's last solution shifted one step
                base[p, :-1] = self._last[p][1:]
                base[p, -1] = self._last[p][-1]
        umpc, fval = np.zeros((B, H, 2)), np.zeros(B)
        xmpc, status = np.zeros((B, H + 1, 6)), np.zeros(B, dtype=np.int32)
        slack = np.zeros(B)
        built = np.zeros((B, H, 6)) if paths is not None else None
        lib = nat.load()
        for lo in range(0, B, self.per_launch):
            hi = min(B, lo + self.per_launch)
            ins = (self._h, hi - lo, models[lo:hi].ctypes.data, seeds[lo:hi].ctypes.data, x0[lo:hi].ctypes.data,
                   xref[lo:hi].ctypes.data, uprev[lo:hi].ctypes.data, base[lo:hi].ctypes.data, hold[lo:hi].ctypes.data)
            outs = (umpc[lo:hi].ctypes.data, fval[lo:hi].ctypes.data, xmpc[lo:hi].ctypes.data, status[lo:hi].ctypes.data)
            if corridor is not None:
                nat.check(lib.llampc_nlp_batch_solve_corridor(*ins, corridor[lo:hi].ctypes.data, weights[lo:hi].ctypes.data,
                                                              *outs, slack[lo:hi].ctypes.data))
            elif paths is not None:
                nat.check(lib.llampc_nlp_batch_solve_track(*ins, paths[lo:hi].ctypes.data, self.corridor_margin,
                                                           weights[lo:hi].ctypes.data, *outs, slack[lo:hi].ctypes.data,
                                                           built[lo:hi].ctypes.data))
            else:
                nat.check(lib.llampc_nlp_batch_solve(*ins, *outs))
        ok = status == nat.NLP_OK
        for p in range(B):
            if ok[p]:
                self._last[p] = umpc[p].copy()
            else:
                self._last.pop(p, None)
        xm = np.ascontiguousarray(xmpc.transpose(0, 2, 1))
        if self.device_corridor:
            for p in range(B):
                if ok[p]:
                    self._last_xmpc[p] = xm[p, :2].copy()
                else:
                    self._last_xmpc.pop(p, None)
        if with_corridor:
            self.max_slack = slack
            self.violation = np.where(ok & (slack > self.corridor_tol), self.Ts, 0.0)
            if built is not None:
                self.last_corridor = built
        return np.ascontiguousarray(umpc.transpose(0, 2, 1)), fval, xm, ok

    def close(self):
        if self._h is not None:
            nat.load().llampc_nlp_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

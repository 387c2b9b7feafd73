"""Host-side mirror of the AutoGP surface that NowcastAutoGP calls.

Every symbol below stands where the reference calls into AutoGP.jl:

    GPModel(ds, y; n_particles, config)      src/make_and_fit_model.jl:84-87
    Schedule.linear_schedule(n, p)           src/make_and_fit_model.jl:90
    fit_smc!(model; schedule, n_mcmc, n_hmc) src/make_and_fit_model.jl:91
    add_data!(model, ds, y)                  src/forecasting.jl:135
    maybe_resample!(model, ess)              src/forecasting.jl:138-141
    num_particles(model)                     src/forecasting.jl:140
    mcmc_structure!(model, n_mcmc, n_hmc)    src/forecasting.jl:146
    mcmc_parameters!(model, n_hmc)           src/forecasting.jl:65,148
    predict_mvn(model, dates) -> rand        src/forecasting.jl:46-47,66-67
    Dict(model) / GPModel(dict)              src/forecasting.jl:128,133

The arithmetic (covariance assembly, Cholesky, log marginal likelihoods, their gradients,
predictive solves) is NOT here: it is the HIP library behind ``engine`` (``_lib.Context`` through
the C-ABI of include/ngp.h).  This file is orchestration: the particle bookkeeping of a
sequential Monte Carlo sampler over kernel structures, batched so that every step is ONE call
carrying all particles.  AutoGP.jl's source is not available here, so the sampler's moves are this
repository's own design ([RECALLED] where they follow what is remembered of AutoGP): data
annealing with incremental log-weights, ESS-triggered multinomial resampling, subtree-regeneration
Metropolis-Hastings over structures, HMC over the N(0,1) latents of the continuous parameters.
Python identifiers drop Julia's ``!``.
"""
from __future__ import annotations

import copy
import datetime as _dt
import hashlib
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import distributed, gp
from ._lib import PosDefException

__all__ = ["GPModel", "Schedule", "fit_smc", "add_data", "maybe_resample", "num_particles",
           "mcmc_structure", "mcmc_parameters", "predict_mvn", "MixtureMVN", "MixtureMarginals",
           "HipEngine", "decompose", "predict_components", "Component", "ComponentForecast"]


# ---------------------------------------------------------------------------------------------
# engine: the only thing that computes.  The product default is the HIP library; it raises if
# the extension or the GPU is missing (there is deliberately no CPU path in this package).
# ---------------------------------------------------------------------------------------------
class HipEngine:
    def __init__(self, device: Optional[int] = None, spec=None):
        from . import _lib
        if device is None:
            import os
            device = int(os.environ.get("LOCAL_RANK", "0"))
        self.ctx = _lib.Context(device, spec)

    def logml(self, programs, t, y):
        return self.ctx.logml_batch(programs, t, y)

    def logml_grad(self, programs, t, y):
        return self.ctx.logml_grad_batch(programs, t, y)

    def kernel_array(self, programs):
        """The C array behind a list of programs, for loops that only change parameters."""
        from ._abi import KernelArray
        return KernelArray(programs)

    def stage_grad(self, ka, t, y):
        """the inputs of ``logml_grad_flat`` resident on the device for several evaluations"""
        return self.ctx.stage_grad(ka, t, y)

    def logml_grad_flat(self, ka, t, y):
        return self.ctx.logml_grad_flat(ka, t, y)

    def predict(self, programs, t, y, t_new, noise_on_new=True):
        return self.ctx.predict_batch(programs, t, y, t_new, noise_on_new)

    def nowcast(self, programs, t, y, t_add, y_add, t_new, noise_on_new=True):
        return self.ctx.nowcast_batch(programs, t, y, t_add, y_add, t_new, noise_on_new)

    def mixture_sample(self, w, mu, sigma, draws, seed):
        """Draws from S mixtures over the same components on the device (Philox stream keyed by
        ``seed``; see include/ngp.h ``ngp_mixture_sample``)."""
        return self.ctx.mixture_sample(w, mu, sigma, draws, seed)

    def mixture_sample_indep(self, w, mu, sigma, draws, seeds):
        """Draws from S independent mixtures in one device call (``ngp_mixture_sample_indep``)."""
        return self.ctx.mixture_sample_indep(w, mu, sigma, draws, seeds)

    def mixture_path_targets(self, w, mu, sigma, draws, seed, inv, targets, probs, want_values=False):
        """Functionals of whole sample paths on the device (``ngp_mixture_path_targets``; S seeds:
        ``ngp_mixture_path_targets_indep``)."""
        return self.ctx.mixture_path_targets(w, mu, sigma, draws, seed, inv, targets, probs,
                                             want_values)

    def ensemble_scores(self, x, y, windows, scale=0, shift=0.0, fair=True):
        """Energy score / sample CRPS per window of paths x [N, m] on the device
        (``ngp_ensemble_scores``)."""
        return self.ctx.ensemble_scores(x, y, windows, scale, shift, fair)

    def mixture_path_scores(self, w, mu, sigma, draws, seed, inv, y, windows, scale=0, shift=0.0,
                            fair=True):
        """The same scores of the sampler's paths without bringing them back
        (``ngp_mixture_path_scores``)."""
        return self.ctx.mixture_path_scores(w, mu, sigma, draws, seed, inv, y, windows, scale, shift,
                                            fair)

    def mixture_cdf(self, w, mu, var, x):
        """CDF of a mixture's per-date marginals on the device (``ngp_mixture_cdf``)."""
        return self.ctx.mixture_cdf(w, mu, var, x)

    def mixture_quantiles(self, w, mu, var, probs):
        """Exact per-date quantiles on the device (``ngp_mixture_quantiles``)."""
        return self.ctx.mixture_quantiles(w, mu, var, probs)

    def mixture_crps(self, w, mu, var, y):
        """Closed-form per-date CRPS on the device (``ngp_mixture_crps``)."""
        return self.ctx.mixture_crps(w, mu, var, y)

    def mixture_crps_mapped(self, w, mu, var, inv, scale, shift, y, tol=0.0):
        """Exact CRPS and mean on the natural / log scale on the device
        (``ngp_mixture_crps_mapped``)."""
        return self.ctx.mixture_crps_mapped(w, mu, var, inv, scale, shift, y, tol)

    def factor(self, programs, t, y):
        """Factorise once, keep L on the device (``ngp_factor``): repeated forecasts of a fitted
        model only pay for their appended / forecast rows."""
        return self.ctx.factor(programs, t, y)


class _FactorCache:
    """(digest, device handle); deep copies of a model start without one."""

    def __init__(self, key, factor):
        self.key, self.factor = key, factor

    def close(self):
        if self.factor is not None:
            self.factor.close()
            self.factor = None

    def __deepcopy__(self, memo):
        return _FactorCache(None, None)


_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = HipEngine()
    return _default_engine


# ---------------------------------------------------------------------------------------------
# transforms (AutoGP rescales dates onto [0,1] — reference docs/vignettes/setting-priors.jl:71 —
# and y by its range — reference src/make_and_fit_model.jl:6-7; exact affine map [RECALLED])
# ---------------------------------------------------------------------------------------------
def to_days(ds) -> np.ndarray:
    """dates -> integer days (datetime.date / numpy datetime64 / numbers accepted)."""
    out = []
    for d in ds:
        if isinstance(d, (_dt.datetime,)):
            out.append(d.date().toordinal())
        elif isinstance(d, _dt.date):
            out.append(d.toordinal())
        elif isinstance(d, np.datetime64):
            out.append(int(d.astype("datetime64[D]").astype(np.int64)))
        else:
            out.append(d)
    return np.asarray(out, dtype=np.float64)


@dataclass
class LinearTransform:
    slope: float
    intercept: float

    def apply(self, x):
        return self.slope * np.asarray(x, dtype=np.float64) + self.intercept

    def invert(self, x):
        return (np.asarray(x, dtype=np.float64) - self.intercept) / self.slope


@dataclass
class DateTransform(LinearTransform):
    """The affine map days -> model time, applied as ``slope * (days - origin)``: the subtraction
    of two day numbers is exact, so dates that are whole days apart land on an exact lattice
    ``q * slope`` — which is what lets the library replace every transcendental of the kernel
    grammar by table lookups (``detect_lattice`` in csrc/ngp_plan.h accepts 2.5 eps of
    the span between the dates and their lattice, so the origin has to lie within the data's span).  ``slope * days + intercept`` on day numbers of ~7e5 loses eleven digits to
    cancellation and every job of a fitted model took the direct-evaluation kernels."""
    origin: float = 0.0

    def apply(self, x):
        return self.slope * (np.asarray(x, dtype=np.float64) - self.origin)

    def invert(self, x):
        return np.asarray(x, dtype=np.float64) / self.slope + self.origin


def date_transform(slope: float, intercept: float) -> DateTransform:
    """From the wire's (slope, intercept): the origin is -intercept / slope, a whole day number
    whenever the dates are (then recovered exactly by rounding)."""
    origin = -intercept / slope
    if abs(origin - round(origin)) < 1e-6:
        origin = float(round(origin))
    return DateTransform(slope, intercept, origin)


def _ds_transform(days: np.ndarray) -> DateTransform:
    lo, hi = float(days.min()), float(days.max())
    span = hi - lo if hi > lo else 1.0
    return DateTransform(1.0 / span, -lo / span, lo)


def _y_transform(y: np.ndarray) -> LinearTransform:
    lo, hi = float(y.min()), float(y.max())
    if not hi > lo:
        # the reference documents this failure as a PosDefException (issue #51,
        # src/make_and_fit_model.jl:6-8); _stabilize_for_fit jitters flat data before it gets here
        raise PosDefException(1, 0)
    slope = 2.0 / (hi - lo)
    return LinearTransform(slope, -slope * (hi + lo) / 2.0)


# ---------------------------------------------------------------------------------------------
class Schedule:
    @staticmethod
    def linear_schedule(n: int, percent: float) -> List[int]:
        """Cumulative observation counts of the data-annealing steps: step = max(1, round(p n))
        up to n (reference src/make_and_fit_model.jl:89-90 clamps p >= 1/n)."""
        if n <= 0:
            raise ValueError("n must be positive")
        step = max(1, int(round(percent * n)))
        out = list(range(step, n, step))
        out.append(n)
        return out


@dataclass
class Particle:
    tree: gp.Node
    noise: float

    def program(self):
        ops, params = gp.to_program(self.tree)
        return ops, params, self.noise


def make_streams(seed: Optional[int] = None):
    """(root, shared): the random streams of a model hang off one integer ``root``.

    ``shared`` is the SAME stream on every rank (data-annealing permutation, flat-series jitter,
    resampling ancestors, mixture draws), seeded from ``seed`` or — ``seed is None`` — from rank
    0's entropy, broadcast.  Everything that concerns ONE particle (its initial tree, its
    structure proposals, its HMC momenta and accept draws) comes from that particle's own stream,
    ``particle_stream(root, generation, global index)``: a particle therefore sees the same
    randomness whichever rank owns it, and a sharded run reproduces the single-rank run."""
    world = distributed.world()[1]
    if seed is None:
        st = np.random.SeedSequence().generate_state(2, dtype=np.uint32)
        root = (int(st[0]) | (int(st[1]) << 31)) % (2**62)
        if world > 1:
            root = distributed.broadcast_int(root)
    else:
        root = int(seed)
    return root, np.random.Generator(np.random.PCG64(np.random.SeedSequence([root, 0])))


def particle_stream(root: int, generation: int, index: int) -> np.random.Generator:
    """Stream of the particle with GLOBAL index ``index``; ``generation`` counts resamplings (the
    copies of a resampled ancestor must not share its future)."""
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence([root, 1, generation, index])))


class GPModel:
    """Ensemble of SMC particles over kernel structures.  Observable fields used by the
    reference's tests: ``config`` (identity preserved, test/test_gpconfig.jl:9), ``ds``, ``y``."""

    def __init__(self, ds=None, y=None, *, n_particles: int = 8, config: Optional[gp.GPConfig] = None,
                 engine=None, seed: Optional[int] = None, depth_cap: int = 6, _from=None,
                 _streams=None):
        if isinstance(ds, dict) and y is None:
            _from = ds
        self.engine = engine
        if _from is not None:
            self._load(_from)
            return
        ds = list(ds)
        y = np.asarray(y, dtype=np.float64)
        if len(ds) != y.size:
            raise ValueError("ds and y must have the same length")
        if n_particles < 1:
            raise ValueError("n_particles must be >= 1")
        self.config = config if config is not None else gp.GPConfig()
        self.ds = ds
        self.y = y.copy()
        self.days = to_days(ds)
        self.ds_transform = _ds_transform(self.days)
        self.y_transform = _y_transform(self.y)
        self.depth_cap = depth_cap
        self._root, self.rng_shared = _streams if _streams is not None else make_streams(seed)
        self._gen = 0
        self.n_particles_total = int(n_particles)
        sl = distributed.shard(self.n_particles_total)
        nloc = sl.stop - sl.start
        self.prng = [particle_stream(self._root, 0, i) for i in range(sl.start, sl.stop)]
        self.particles: List[Particle] = [
            Particle(gp.sample_tree(r, self.config, depth_cap=depth_cap),
                     gp.sample_noise(r, self.config)) for r in self.prng]
        self.log_weights = np.zeros(nloc)
        self.n_obs = 0                      # observations absorbed so far (data annealing)
        self._perm = np.arange(y.size)
        self._logml = np.zeros(nloc)        # log p(y[:n_obs] | particle)

    # -- engine ---------------------------------------------------------------------------------
    def _eng(self):
        if self.engine is None:
            self.engine = default_engine()
        if self.__dict__.get("_spec_checked") is False:   # loaded from a dict before it had an engine
            from . import wire
            self._spec_checked = True
            wire.check_spec(self.engine, self.__dict__.get("wire_spec"))
        return self.engine

    # -- data views -----------------------------------------------------------------------------
    def _obs(self, count: Optional[int] = None):
        """(t, y) of the first ``count`` annealed observations, in time order, on model scale."""
        count = self.n_obs if count is None else count
        idx = np.sort(self._perm[:count])
        return self.ds_transform.apply(self.days[idx]), self.y_transform.apply(self.y[idx])

    def programs(self):
        return [p.program() for p in self.particles]

    # -- cached factorisation of the current ensemble on the current data ------------------------
    def _factor(self):
        """The engine's resident factor for (particles, observed data), or None if the engine has
        none (or the training set is longer than one handle can be queried on).  The handle is
        keyed on a digest of exactly what it was built from, so any move that changes a particle
        or the data simply misses; it is never part of ``Dict(model)``."""
        make = getattr(self._eng(), "factor", None)
        if make is None:
            return None
        t, y = self._obs()
        progs = self.programs()
        h = hashlib.blake2b(digest_size=16)
        for ops, params, noise in progs:
            h.update(np.asarray(ops, dtype=np.int32).tobytes())
            h.update(np.asarray(params, dtype=np.float64).tobytes())
            h.update(np.float64(noise).tobytes())
        h.update(t.tobytes())
        h.update(y.tobytes())
        key = h.digest()
        cache = self.__dict__.get("_fcache")
        if cache is None or cache.key != key:
            if cache is not None:
                cache.close()
            try:
                fac = make(progs, t, y)
            except (RuntimeError, MemoryError):   # e.g. the ensemble does not fit: one-shot path
                fac = None
            cache = _FactorCache(key, fac)
            self.__dict__["_fcache"] = cache
        return cache.factor

    # -- Dict(model) / GPModel(dict)  (reference src/forecasting.jl:128,133) ----------------------
    def to_dict(self) -> dict:
        """The versioned, JSON-serialisable snapshot of ``nowcastautogp_amd.wire`` (plain data: a
        ``deepcopy`` is a data copy, ``json.dumps`` works, no live objects)."""
        from . import wire
        spec = None
        eng = self.engine
        if eng is not None and hasattr(eng, "ctx"):
            sp = eng.ctx.get_spec()
            spec = dict(se_form=sp.se_form, periodic_form=sp.periodic_form, cp_form=sp.cp_form,
                        jitter=sp.jitter)
        return wire.model_to_wire(self, spec)

    def _load(self, d: dict):
        from . import wire
        wire.model_from_wire(self, d)

    def clone(self, root: Optional[int] = None) -> "GPModel":
        """What ``GPModel(deepcopy(Dict(model)))`` gives (reference src/forecasting.jl:128,133),
        without the round trip through the wire dict: with a few thousand observations that trip
        is 30 ms per clone, and forecast_with_nowcasts makes one clone per scenario.  Kernel trees
        are shared between the clones — no move mutates a tree in place (a proposal works on its
        own copy, an accepted move installs a new tree) — everything else is copied.  ``root``:
        give the clone fresh random streams right away (``reseed``) instead of copies of this
        model's — what forecast_with_nowcasts wants for its scenarios."""
        m = GPModel.__new__(GPModel)
        m.engine = self.engine
        m.config = copy.deepcopy(self.config)
        m.ds = list(self.ds)
        m.y, m.days = self.y.copy(), self.days.copy()
        m.ds_transform = copy.copy(self.ds_transform)
        m.y_transform = LinearTransform(self.y_transform.slope, self.y_transform.intercept)
        m.depth_cap = self.depth_cap
        m._root, m._gen = self._root, self._gen
        m.n_particles_total = self.n_particles_total
        m.particles = [Particle(p.tree, p.noise) for p in self.particles]
        m.log_weights = self.log_weights.copy()
        m.n_obs = self.n_obs
        m._perm = self._perm.copy()
        m._logml = self._logml.copy()
        if self.__dict__.get("wire_spec") is not None:
            m.wire_spec = dict(self.wire_spec)
        if root is None:
            m.rng_shared = copy.deepcopy(self.rng_shared)
            m.prng = [copy.deepcopy(r) for r in self.prng]
        else:
            m.reseed(root)
        return m

    def reseed(self, root: int) -> None:
        """Fresh streams for a clone (forecast_with_nowcasts gives every scenario its own root)."""
        self._root, self._gen = int(root), 0
        lo = distributed.shard(self.n_particles_total).start
        self.prng = [particle_stream(self._root, 0, lo + i) for i in range(len(self.particles))]
        self.rng_shared = np.random.Generator(np.random.PCG64(np.random.SeedSequence([self._root, 0])))

    @classmethod
    def from_dict(cls, d: dict, engine=None) -> "GPModel":
        return cls(_from=d, engine=engine)


def num_particles(model: GPModel) -> int:
    return model.n_particles_total


# ---------------------------------------------------------------------------------------------
# weights / resampling — the only cross-particle (and, multi-GPU, cross-rank) step
# ---------------------------------------------------------------------------------------------
def _normalized_weights(model: GPModel):
    w, ess = distributed.normalize_log_weights(model.log_weights,
                                               P_total=model.n_particles_total)
    return w, ess


def effective_sample_size(model: GPModel) -> float:
    return _normalized_weights(model)[1]


def maybe_resample(model: GPModel, ess_threshold: float) -> bool:
    """Resample (multinomial) when ESS < ess_threshold (an absolute count, as the reference
    passes ``ess_threshold * num_particles``, src/forecasting.jl:138-141).  Weights reset to
    uniform.  Across ranks: all-gather of log-weights, identical ancestors everywhere, particle
    descriptors exchanged — no matrix moves."""
    return maybe_resample_lockstep([model], ess_threshold)[0]


def maybe_resample_lockstep(models: Sequence[GPModel], ess_threshold: float) -> List[bool]:
    """``maybe_resample`` of D models at once (the scenario clones of forecast_with_nowcasts,
    reference src/forecasting.jl:131-141): ONE all-gather of the [P_local, D] log-weights serves
    every model's normalisation and ESS, and ONE exchange of particle descriptors serves every
    model that resamples.  Model j draws its ancestors from its own shared stream, so the result
    is what D separate calls give."""
    P_total = models[0].n_particles_total
    logw = np.stack([m.log_weights for m in models], axis=1)                 # [P_local, D]
    _, ess, w_all = distributed.normalize_log_weights(logw, P_total=P_total, full=True)
    need = [j for j in range(len(models)) if ess[j] < ess_threshold]
    if not need:
        return [False] * len(models)
    ancs, descrs = [], []
    for j in need:
        m = models[j]
        seed = int(m.rng_shared.integers(0, 2**31 - 1))   # shared stream: same ancestors everywhere
        ancs.append(distributed.resample_ancestors(w_all[:, j], seed))
        descrs.append([(p.program(), float(l)) for p, l in zip(m.particles, m._logml)])
    mine = distributed.exchange_particles_many(descrs, ancs)
    lo = distributed.shard(P_total).start
    for j, got in zip(need, mine):
        m = models[j]
        m.particles = [Particle(gp.from_program(pr[0], pr[1]), float(pr[2])) for pr, _ in got]
        m._logml = np.array([l for _, l in got])
        m.log_weights = np.zeros(len(got))
        m._gen += 1      # copies of one ancestor must not share its future draws
        m.prng = [particle_stream(m._root, m._gen, lo + i) for i in range(len(got))]
    done = [False] * len(models)
    for j in need:
        done[j] = True
    return done


# ---------------------------------------------------------------------------------------------
# rejuvenation moves (all particles advance together: one engine call per proposal / leapfrog)
# ---------------------------------------------------------------------------------------------
def _valid_program(tree: gp.Node) -> bool:
    from . import _lib
    ops, params = gp.to_program(tree)
    return _lib.kernel_check((ops, params, 0.1)) == 0


def _nodes(tree: gp.Node):
    out = []

    def walk(nd, depth, parent, side):
        out.append((nd, depth, parent, side))
        if not nd.is_leaf:
            walk(nd.left, depth + 1, nd, "left")
            walk(nd.right, depth + 1, nd, "right")

    walk(tree, 1, None, None)
    return out


def _group_obs(models: Sequence[GPModel]):
    """(t, [y_j]): the observed data of models that advance in lockstep.  They must sit on the
    same dates (the scenario clones of forecast_with_nowcasts do, reference
    src/create_nowcast_data.jl:36-37); only the observations differ."""
    t, y0 = models[0]._obs()
    ys = [y0]
    m0 = models[0]
    d0 = np.sort(m0.days[m0._perm[:m0.n_obs]])
    for m in models[1:]:
        tj, yj = m._obs()
        if (m.n_obs != m0.n_obs or m.ds_transform != m0.ds_transform
                or not np.array_equal(np.sort(m.days[m._perm[:m.n_obs]]), d0)):
            raise ValueError("models advanced in lockstep must share their observation dates")
        ys.append(yj)
    return t, ys


def _item_y(ys, owner):
    """The ``y`` argument of an engine call whose item i belongs to model ``owner[i]``: the one
    shared vector for a single model, else one row per item (``ldy = n`` in include/ngp.h)."""
    if len(ys) == 1:
        return ys[0]
    own = np.asarray(owner, dtype=np.int64)
    rows = np.stack(ys)
    # the usual case — every model's items together, model after model, equally many each — is a
    # plain repeat (0.1 s for the 210 MB of 64 x 200 items; the row gather takes five times that)
    per = own.size // len(ys) if len(ys) else 0
    if per * len(ys) == own.size and np.array_equal(own, np.repeat(np.arange(len(ys)), per)):
        return np.repeat(rows, per, axis=0)
    return rows[own]


_KIND_CODE_CACHE = {}


def _kind_codes(ops) -> tuple:
    """KIND_CODES of a program's parameters followed by the noise, cached by opcode sequence."""
    key = ops.tobytes()
    got = _KIND_CODE_CACHE.get(key)
    if got is None:
        got = tuple(gp.KIND_CODES[k] for k in gp.param_kinds(ops) + [gp.NOISE_KIND])
        _KIND_CODE_CACHE[key] = got
    return got


def _all_items_y(models, ys):
    """``_item_y`` for the call that carries every particle of every model (210 MB at 64 x 200
    items of 2049 points: built once per group of moves, not once per move)."""
    return _item_y(ys, [j for j, m in enumerate(models) for _ in m.particles])


def _structure_move(models: Sequence[GPModel], t, ys):
    """Subtree-regeneration Metropolis-Hastings: pick a node uniformly, redraw its subtree from
    the prior; accept with min(1, L'/L * |T|/|T'|).  Every particle of every model proposes; ONE
    engine call evaluates all proposals."""
    props, idx = [], []
    for j, model in enumerate(models):
        cfg = model.config
        for k, p in enumerate(model.particles):
            rng = model.prng[k]
            new = gp.clone(p.tree)
            nodes = _nodes(new)
            nd, depth, parent, side = nodes[int(rng.integers(len(nodes)))]
            sub = gp.sample_tree(rng, cfg, depth=depth, depth_cap=model.depth_cap)
            if parent is None:
                new = sub
            else:
                setattr(parent, side, sub)
            if _valid_program(new):
                props.append(new)
                idx.append((j, k))
    if not props:
        return 0
    progs = [gp.to_program(tr) + (models[j].particles[k].noise,) for tr, (j, k) in zip(props, idx)]
    lm, info = models[0]._eng().logml(progs, t, _item_y(ys, [j for j, _ in idx]))
    acc = 0
    for tr, (j, k), l1, bad in zip(props, idx, lm, info):
        if bad or not np.isfinite(l1):
            continue
        model = models[j]
        log_a = (l1 - model._logml[k]) + math.log(model.particles[k].tree.size() / tr.size())
        if math.log(model.prng[k].random()) < log_a:
            model.particles[k].tree = tr
            model._logml[k] = float(l1)
            acc += 1
    return acc


def _hmc_move(models: Sequence[GPModel], t, ys, n_leapfrog: int, eps: float, Y=None,
              device: bool = False):
    """One HMC transition per particle on the N(0,1) latents z of (parameters, noise):
    U(z) = -log p(y | theta(z)) + |z|^2 / 2, gradient through the engine's logml gradient.
    All particles of all models move together: the latents live in one flat vector (``sl[i]`` is
    item i's slice), every leapfrog stage is ONE engine call of P x D items (per-item y rows when
    D > 1) and a handful of numpy operations.
    ``device`` (``hmc_config["device"]``): with an engine whose staged job has it, the whole
    trajectory is ONE library call (``ngp_grad_job_hmc``: the same arithmetic on the device, the
    latents never leave it between evaluations); momenta and accept uniforms are drawn here either
    way, from the same generators in the same order."""
    prior = models[0].config.prior
    fixed_noise = models[0].config.noise is not None
    items = [(j, k) for j, m in enumerate(models) for k in range(len(m.particles))]
    B = len(items)
    if B == 0:
        return 0
    part = [models[j].particles[k] for j, k in items]
    prng = [models[j].prng[k] for j, k in items]
    ops, theta0, codes_l, sizes = [], [], [], []
    for p in part:
        o, params = gp.to_program(p.tree)
        kc = _kind_codes(o)
        ops.append(o)
        theta0.append(params)
        theta0.append((p.noise,))
        codes_l.extend(kc)
        sizes.append(len(kc))
    sizes = np.array(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    sl = [slice(int(off[i]), int(off[i + 1])) for i in range(B)]
    seg = np.repeat(np.arange(B), sizes)                     # item of every latent
    codes = np.array(codes_l)
    z0 = gp.untransform_flat(np.concatenate(theta0), codes, prior)
    last = off[1:] - 1                                       # the noise latent of every item
    i_positive = np.flatnonzero((codes == gp.KIND_CODES["wildcard"]) | (codes == gp.KIND_CODES["period"]))
    i_gamma = np.flatnonzero(codes == gp.KIND_CODES["gamma"])
    i_unit = np.flatnonzero(codes == gp.KIND_CODES["unit"])
    to_theta = gp.FlatTransform(codes, prior)

    is_param = np.ones(codes.size, dtype=bool)
    is_param[last] = False
    i_param = np.flatnonzero(is_param)
    eng = models[0]._eng()
    if Y is None:     # the callers that make several moves on the same data pass it in
        Y = _item_y(ys, [j for j, _ in items])
    ka = job = None
    if hasattr(eng, "logml_grad_flat"):
        ka = eng.kernel_array([(ops[i], np.zeros(sizes[i] - 1), 0.0) for i in range(B)])
        # the leapfrog steps change nothing but the parameters: trees, dates and observations are
        # staged once per move (include/ngp.h ngp_grad_stage), each evaluation sends the parameters
        if hasattr(eng, "stage_grad"):
            job = eng.stage_grad(ka, t, Y)

    def sums(v):                                             # per-item sums of a flat vector
        return np.bincount(seg, weights=v, minlength=B)

    def potential(z):
        zc = z if np.isfinite(z).all() else np.nan_to_num(z, nan=0.0, posinf=50.0, neginf=-50.0)
        th, dth = to_theta(zc)
        # degenerate parameters (a diverged trajectory) would only produce a non-PD matrix and a
        # rejection; keep them inside what the kernels accept
        th = np.clip(th, -1e6, 1e6)
        if i_positive.size:
            th[i_positive] = np.maximum(th[i_positive], 1e-12)
        if i_gamma.size:
            th[i_gamma] = np.clip(th[i_gamma], 1e-9, 2.0 - 1e-9)
        if i_unit.size:
            th[i_unit] = np.clip(th[i_unit], 1e-9, 1.0 - 1e-9)
        # (the same margins as gp.clip_flat, which the accepted parameters go through)
        if ka is not None:      # same structures, new parameters: refill the C array in place
            ka.set_params(th[i_param], th[last])
            lm, g, info = job.run(ka) if job is not None else eng.logml_grad_flat(ka, t, Y)
        else:
            progs = [(ops[i], th[sl[i]][:-1], float(th[last[i]])) for i in range(B)]
            lm, grads, info = eng.logml_grad(progs, t, Y)
            g = np.concatenate(grads)
        with np.errstate(invalid="ignore", over="ignore"):
            ok = (np.asarray(info) == 0) & np.isfinite(lm) & (sums(~np.isfinite(g)) == 0)
            U = np.where(ok, -np.asarray(lm) + 0.5 * sums(z * z), np.inf)
            dU = np.where(ok[seg], -g * dth + z, 0.0)
        if fixed_noise:
            dU[last] = 0.0
        return U, dU, lm

    on_device = bool(device) and job is not None and hasattr(job, "hmc")
    try:
        if on_device:
            mom = np.concatenate([prng[i].standard_normal(int(sizes[i])) for i in range(B)])
            frozen = None
            if fixed_noise:
                mom[last] = 0.0
                frozen = np.zeros(codes.size, dtype=np.uint8)
                frozen[last] = 1
            out = job.hmc(codes, z0, mom, n_leapfrog, eps, prior, frozen=frozen)
            H0 = out["U0"] + out["K0"]
            with np.errstate(invalid="ignore", over="ignore"):
                H1 = out["U1"] + out["K1"]
            th_new, lm1 = out["theta1"], out["logml1"]
        else:
            U0, dU, _ = potential(z0)
            mom = np.concatenate([prng[i].standard_normal(int(sizes[i])) for i in range(B)])
            if fixed_noise:
                mom[last] = 0.0
            H0 = U0 + 0.5 * sums(mom * mom)
            z = z0.copy()
            pm = mom - 0.5 * eps * dU
            lm1 = U1 = None
            for step in range(n_leapfrog):
                z = z + eps * pm
                U1, dU, lm1 = potential(z)
                pm = pm - (eps if step < n_leapfrog - 1 else 0.5 * eps) * dU
    finally:
        if job is not None:   # the device arena goes back whatever a step raised
            job.close()
    if not on_device:
        with np.errstate(invalid="ignore", over="ignore"):
            H1 = U1 + 0.5 * sums(pm * pm)
        # what is installed on acceptance is what the last evaluation saw: clipped into the open domain
        # of every kind, so no particle ever carries a saturated parameter (an infinite latent)
        zc = z if np.isfinite(z).all() else np.nan_to_num(z, nan=0.0, posinf=50.0, neginf=-50.0)
        th_new = gp.clip_flat(np.clip(to_theta(zc)[0], -1e6, 1e6), codes)
    acc = 0
    for i, (j, k) in enumerate(items):
        u = prng[i].random()      # drawn for every particle: the stream does not depend on H
        if np.isfinite(H1[i]) and math.log(u) < H0[i] - H1[i]:
            th = th_new[sl[i]]
            part[i].tree = gp.from_program(ops[i], th[:-1])
            part[i].noise = float(th[-1])
            models[j]._logml[k] = float(lm1[i])
            acc += 1
    return acc


# "device": run each move's whole trajectory in one library call (ngp_grad_job_hmc) where the
# engine's staged job offers it; off by default
DEFAULT_HMC = {"n_leapfrog": 10, "eps": 0.02, "device": False}


def mcmc_parameters(model: GPModel, n_hmc: int, hmc_config: Optional[dict] = None) -> None:
    mcmc_parameters_lockstep([model], n_hmc, hmc_config)


def mcmc_structure(model: GPModel, n_mcmc: int, n_hmc: int, hmc_config: Optional[dict] = None,
                   biased: bool = False) -> None:
    mcmc_structure_lockstep([model], n_mcmc, n_hmc, hmc_config, biased)


def mcmc_parameters_lockstep(models: Sequence[GPModel], n_hmc: int,
                             hmc_config: Optional[dict] = None, _obs=None):
    """``mcmc_parameters!`` (reference src/forecasting.jl:65,148) for D models at once.
    ``_obs``: the ``(t, ys, Y)`` a previous call on the same models and data returned — the
    per-draw refinement of ``forecast`` (src/forecasting.jl:63-68) then builds the P x D
    observation rows (210 MB at 64 x 200 items of 2,049 points) once, not once per draw."""
    cfgd = {**DEFAULT_HMC, **(hmc_config or {})}
    if _obs is None:
        t, ys = _group_obs(models)
        _obs = (t, ys, _all_items_y(models, ys))
    t, ys, Y = _obs
    for _ in range(int(n_hmc)):
        _hmc_move(models, t, ys, cfgd["n_leapfrog"], cfgd["eps"], Y, cfgd["device"])
    return _obs


def mcmc_structure_lockstep(models: Sequence[GPModel], n_mcmc: int, n_hmc: int,
                            hmc_config: Optional[dict] = None, biased: bool = False) -> None:
    """``mcmc_structure!`` (reference src/forecasting.jl:146) for D models at once."""
    del biased  # accepted for signature compatibility; proposals are always drawn from the prior
    t, ys = _group_obs(models)
    cfgd = {**DEFAULT_HMC, **(hmc_config or {})}
    Y = _all_items_y(models, ys)
    for _ in range(int(n_mcmc)):
        _structure_move(models, t, ys)
        for _ in range(int(n_hmc)):
            _hmc_move(models, t, ys, cfgd["n_leapfrog"], cfgd["eps"], Y, cfgd["device"])


# ---------------------------------------------------------------------------------------------
def _refresh_logml(model: GPModel, count: int):
    t, y = model._obs(count)
    lm, info = model._eng().logml(model.programs(), t, y)
    lm = np.where((info != 0) | ~np.isfinite(lm), -np.inf, lm)
    return lm


def fit_smc(model: GPModel, *, schedule: Sequence[int], n_mcmc: int, n_hmc: int,
            hmc_config: Optional[dict] = None, biased: bool = False, shuffle: bool = True,
            adaptive_resampling: bool = True, adaptive_rejuvenation: bool = False,
            verbose: bool = False) -> None:
    """SMC over data batches (``n_mcmc`` and ``n_hmc`` are required keywords, as in the reference:
    omitting them is an error, test/test_gpconfig.jl:42)."""
    n = model.y.size
    model._perm = model.rng_shared.permutation(n) if shuffle else np.arange(n)
    P = num_particles(model)
    for count in schedule:
        count = int(min(count, n))
        if count <= model.n_obs:
            continue
        lm = _refresh_logml(model, count)
        model.log_weights = _advance_weights(model.log_weights, lm, model._logml)
        model._logml = lm
        model.n_obs = count
        resampled = maybe_resample(model, P / 2.0 if adaptive_resampling else float("inf"))
        if (not adaptive_rejuvenation) or resampled:
            mcmc_structure(model, n_mcmc, n_hmc, hmc_config, biased)
        if verbose:
            print(f"[fit_smc] n_obs={count} ess={effective_sample_size(model):.2f}")


def _advance_weights(logw, lm_new, lm_old):
    """log-weights after an incremental weight update.  A particle whose factorisation failed has
    logml = -inf; twice in a row that would be -inf - (-inf) = NaN and poison the whole ensemble
    through the normalisation, so a dead particle simply stays dead (-inf)."""
    with np.errstate(invalid="ignore"):
        inc = np.where(np.isneginf(lm_new), -np.inf, lm_new - lm_old)
        out = logw + inc
    return np.where(np.isnan(out), -np.inf, out)


def horizon_blocks(n_obs: int, d: int, m: int):
    """The library carries the appended and forecast points of a query as at most NGP_MAX_AUX
    rows beside the factor: (n mod 64) + d + m + 1 <= NGP_MAX_AUX (include/ngp.h).  The reference
    has no such limit, so longer horizons are served in several calls: returns None when the m
    dates fit one call, else the (lo, hi) blocks to query PAIRWISE (``predict_in_blocks``) — each
    block is at most half the room of a call, so any two of them fit together and every
    cross-covariance block of the joint predictive comes out of some call."""
    from ._abi import NGP_MAX_AUX
    room = NGP_MAX_AUX - (n_obs % 64) - d - 1
    if m <= room:
        return None
    blk = room // 2
    if blk < 1:
        raise ValueError(
            f"forecast horizon: with {n_obs} observations and {d} appended points no forecast "
            f"dates fit beside the factor (NGP_MAX_AUX = {NGP_MAX_AUX} rows); append fewer points "
            "per call")
    return [(lo, min(lo + blk, m)) for lo in range(0, m, blk)]


def predict_in_blocks(call, t_new: np.ndarray, blocks):
    """``call(t_sub) -> (mu [..., m_sub], sigma [P, m_sub, m_sub], info [P], extra)`` for any
    subset of the dates.  Queries every pair of blocks once and assembles the joint mean
    [..., m] and covariance [P, m, m]; ``extra`` (whatever does not depend on the dates) is the
    first call's.  The blocks of a pair are conditionally dependent given the data, which is why
    single-block calls would not do: Sigma[a, b] only exists inside a call that holds both."""
    m = t_new.size
    q = len(blocks)
    pairs = [(a, b) for a in range(q) for b in range(a + 1, q)] or [(0, 0)]
    mu = sigma = info = extra = None
    for a, b in pairs:
        idx = np.arange(*blocks[a]) if a == b else np.concatenate(
            [np.arange(*blocks[a]), np.arange(*blocks[b])])
        mu_s, sg_s, info_s, extra_s = call(t_new[idx])
        if mu is None:
            mu = np.empty(mu_s.shape[:-1] + (m,))
            sigma = np.empty((sg_s.shape[0], m, m))
            info, extra = np.array(info_s, copy=True), extra_s
        mu[..., idx] = mu_s
        sigma[:, idx[:, None], idx[None, :]] = sg_s
        info = np.where(info != 0, info, info_s)
    return mu, sigma, info, extra


def _append(model: GPModel, ds, y) -> int:
    n_old = model.y.size
    model.ds = model.ds + ds
    model.days = np.concatenate([model.days, to_days(ds)])
    model.y = np.concatenate([model.y, y])
    model._perm = np.concatenate([model._perm, np.arange(n_old, n_old + y.size)])
    return n_old + y.size


def add_data(model: GPModel, ds, y) -> None:
    """Append observations; particle log-weights move by logml(n+d) - logml(n)
    (reference src/forecasting.jl:135)."""
    ds, y = list(ds), np.asarray(y, dtype=np.float64)
    if len(ds) != y.size:
        raise ValueError("ds and y must have the same length")
    if model.n_obs != model.y.size:
        raise RuntimeError("add_data on a model that has not absorbed all of its data")
    count = _append(model, ds, y)
    lm = _refresh_logml(model, count)
    model.log_weights = _advance_weights(model.log_weights, lm, model._logml)
    model._logml = lm
    model.n_obs = count


def add_data_lockstep(models: Sequence[GPModel], ds, ys, base: Optional[GPModel] = None) -> None:
    """``add_data!`` (reference src/forecasting.jl:135) on D clones at once: model j absorbs
    ``ys[j]`` on the shared dates ``ds``.

    ``base``: the model all of them were cloned from and still equal (same particles, same
    observed data).  The appended covariance rows then do not depend on the scenario, so the D
    weight updates are ONE query of the base model's resident factor (``ngp_factor_nowcast``, or
    ``ngp_nowcast_batch`` without one): P factorisations at most, instead of P x D.  Without
    ``base`` it is one ``logml`` call of P x D items with per-item y rows."""
    ds = list(ds)
    ys = [np.asarray(y, dtype=np.float64) for y in ys]
    if len(ys) != len(models) or any(len(ds) != y.size for y in ys):
        raise ValueError("one vector of len(ds) observations per model")
    if any(m.n_obs != m.y.size for m in models):
        raise RuntimeError("add_data on a model that has not absorbed all of its data")
    eng = models[0]._eng()
    lms = None
    if base is not None and hasattr(eng, "nowcast") and len(ds) > 0:
        t, y = base._obs()
        t_add = base.ds_transform.apply(to_days(ds))
        y_add = np.stack([base.y_transform.apply(v) for v in ys])
        from ._abi import NGP_MAX_AUX
        if (t.size % 64) + t_add.size + 1 <= NGP_MAX_AUX:     # the appended rows fit one call
            fac = base._factor()
            o = (fac.nowcast(t_add, y_add, np.zeros(0), True) if fac is not None else
                 eng.nowcast(base.programs(), t, y, t_add, y_add, np.zeros(0), True))
            lf = np.asarray(o["logml_full"], dtype=np.float64)             # [P, D]
            dead = (np.asarray(o["info"]) != 0)[:, None] | ~np.isfinite(lf)
            lms = np.where(dead, -np.inf, lf)
    counts = [_append(m, ds, y) for m, y in zip(models, ys)]
    if lms is None:
        t, yy = _group_obs_count(models, counts[0])
        owner = [j for j, m in enumerate(models) for _ in m.particles]
        lm, info = eng.logml([p for m in models for p in m.programs()], t, _item_y(yy, owner))
        lm = np.where((np.asarray(info) != 0) | ~np.isfinite(lm), -np.inf, lm)
        o = np.concatenate([[0], np.cumsum([len(m.particles) for m in models])])
        lms = np.stack([lm[o[j]:o[j + 1]] for j in range(len(models))], axis=1)
    for j, m in enumerate(models):
        lm = np.array(lms[:, j])
        m.log_weights = _advance_weights(m.log_weights, lm, m._logml)
        m._logml = lm
        m.n_obs = counts[j]


def _group_obs_count(models, count):
    t, y0 = models[0]._obs(count)
    return t, [y0] + [m._obs(count)[1] for m in models[1:]]


# ---------------------------------------------------------------------------------------------
class MixtureMVN:
    """Weighted mixture of per-particle multivariate normals (what predict_mvn returns);
    ``rand(k)`` -> [m, k], ``rand()`` -> [m] (reference src/forecasting.jl:47,67)."""

    def __init__(self, means, covs, weights, rng, sampler=None):
        self.means, self.covs = np.asarray(means, float), np.asarray(covs, float)
        self.weights = np.asarray(weights, float) / np.sum(weights)
        self.rng = rng
        self.sampler = sampler     # engine.mixture_sample: many draws in one device call
        self._chol = {}

    def _factor(self, k):
        if k not in self._chol:
            try:
                self._chol[k] = np.linalg.cholesky(self.covs[k])
            except np.linalg.LinAlgError:
                raise PosDefException(1, k) from None
        return self._chol[k]

    def rand(self, draws: Optional[int] = None):
        m = self.means.shape[1]
        k = 1 if draws is None else int(draws)
        if self.sampler is not None and draws is not None and k > 1 and m > 0:
            seed = int(self.rng.integers(0, 2**63 - 1))
            out, _, info = self.sampler(self.weights[None, :], self.means[:, None, :], self.covs,
                                        k, seed)
            _raise_if_failed(info)
            return np.ascontiguousarray(out[0].T)
        comp = self.rng.choice(self.weights.size, size=k, p=self.weights)
        out = np.empty((m, k))
        for j, c in enumerate(comp):
            out[:, j] = self.means[c] + self._factor(int(c)) @ self.rng.standard_normal(m)
        return out[:, 0] if draws is None else out

    def mean(self):
        return self.weights @ self.means

    def marginals(self, engine=None) -> "MixtureMarginals":
        """The per-date marginals (means and the diagonal of every covariance)."""
        return MixtureMarginals(self.means, np.einsum("kjj->kj", self.covs), self.weights,
                                engine=engine)


_erf = np.frompyfunc(math.erf, 1, 1)
_erfc = np.frompyfunc(math.erfc, 1, 1)


def _abs_moment(d, v):
    """E|N(d, v)| = d erf(d / sqrt(2 v)) + sqrt(2 v / pi) exp(-d^2 / (2 v))"""
    s = np.sqrt(2.0 * v)
    r = d / s
    return d * _erf(r).astype(np.float64) + s * np.exp(-r * r) / math.sqrt(math.pi)


def _host_mapped(w, mu, var, inv, scale, shift, y):
    """Host stand-in for ``ngp_mixture_crps_mapped`` (small mixtures): composite Gauss-Legendre 20
    in fp64 on panels of half the smallest sd between the same breakpoints, once at that width and
    once at half of it — the difference is the error estimate.  Returns (crps, mean, err, info)."""
    from ._abi import (NGP_INFO_NOT_FINITE, NGP_INV_BOXCOX, NGP_INV_EXP, NGP_INV_IDENTITY,
                       NGP_INV_LOGISTIC100)
    kind, lam, offset = int(inv[0]), float(inv[1]), float(inv[2])
    is_exp = kind == NGP_INV_EXP or (kind == NGP_INV_BOXCOX and lam == 0.0)
    gx, gw = np.polynomial.legendre.leggauss(20)

    def g(x):
        with np.errstate(all="ignore"):
            if kind == NGP_INV_IDENTITY:
                return x
            if is_exp:
                return np.maximum(np.exp(x) - offset, 0.0)
            if kind == NGP_INV_LOGISTIC100:
                return np.maximum(100.0 / (1.0 + np.exp(-x)) - offset, 0.0)
            base = lam * x + 1.0
            if lam > 0:
                return np.maximum(np.maximum(base, 1e-10) ** (1.0 / lam) - offset, 0.0)
            safe = np.where(base > 0, base, 1.0)
            return np.maximum(np.where(base > 0, safe ** (1.0 / lam) - offset, 0.0), 0.0)

    def dpsi(x):
        with np.errstate(all="ignore"):
            if kind == NGP_INV_IDENTITY:
                d = np.ones_like(x)
            elif is_exp:
                d = np.exp(x)
            elif kind == NGP_INV_LOGISTIC100:
                sg = 1.0 / (1.0 + np.exp(-x))
                d = 100.0 * sg * (1.0 - sg)
            else:
                d = (lam * x + 1.0) ** (1.0 / lam - 1.0)
            return d / (g(x) + shift) if scale else d

    def s(v):
        with np.errstate(all="ignore"):
            return np.log(v + shift) if scale else v

    xL, xR, gmin = -np.inf, np.inf, -np.inf
    if kind == NGP_INV_IDENTITY:
        xL = -shift if scale else -np.inf
    else:
        gmin = float(g(np.float64(-np.inf)))
        if is_exp:
            xL = math.log(offset) if offset > 0 else -np.inf
        elif kind == NGP_INV_LOGISTIC100:
            xL = (np.inf if offset >= 100 else
                  math.log(offset / (100.0 - offset)) if offset > 0 else -np.inf)
        else:
            edge = (1e-10 - 1.0) / lam
            xL, xR = (edge, np.inf) if lam > 0 else (-np.inf, edge)
            if offset > 0:
                xL = max(xL, (offset ** lam - 1.0) / lam)
    m = mu.shape[1]
    out, mean, err = np.full(m, np.nan), np.full(m, np.nan), np.full(m, np.nan)
    info = np.zeros(m, dtype=np.int32)
    for j in range(m):
        mj, ij = mu[:, j], 1.0 / np.sqrt(2.0 * var[:, j])
        sd = np.sqrt(var[:, j])
        lo, hi = float(np.min(mj - 10.0 * sd)), float(np.max(mj + (10.0 + 2.0 * sd) * sd))

        def tail(x, upper):
            t = (x[None, :] - mj[:, None]) * ij[:, None]
            return w @ (0.5 * _erfc(t if upper else -t).astype(np.float64))

        if ((xR < hi and tail(np.array([xR]), True)[0] > 1e-12)
                or (scale and not gmin + shift > 0 and xL > lo)):
            info[j] = NGP_INFO_NOT_FINITE
            continue
        alo = min(max(lo, xL), hi)
        ahi = max(min(hi, xR), alo)
        v = y[j] + offset
        if kind == NGP_INV_IDENTITY:
            xy = y[j]
        elif y[j] <= gmin or not v > 0:
            xy = -np.inf
        elif is_exp:
            xy = math.log(v)
        elif kind == NGP_INV_LOGISTIC100:
            xy = np.inf if v >= 100 else math.log(v / (100.0 - v))
        else:
            xy = (v ** lam - 1.0) / lam
        x0 = min(max(xy, alo), ahi)
        psi0, yt = float(s(g(np.float64(x0)))), float(s(np.float64(y[j])))
        clip = 0.0 if alo < xy < ahi else abs(yt - psi0)
        vals = []
        for width in (0.5 * sd.min(), 0.25 * sd.min()):
            c2 = m1 = 0.0
            for a, b, upper in ((alo, x0, False), (x0, ahi, True)):
                if not b > a:
                    continue
                n = max(1, int(math.ceil((b - a) / width)))
                e = np.linspace(a, b, n + 1)
                h = 0.5 * np.diff(e)
                x = ((e[:-1] + h)[:, None] + h[:, None] * gx[None, :]).ravel()
                T = tail(x, upper)
                d = dpsi(x) * (h[:, None] * gw[None, :]).ravel()
                c2 += float(np.sum(T * T * d))
                m1 += float(np.sum(T * d)) * (1.0 if upper else -1.0)
            vals.append((c2 + clip, psi0 + m1))
        out[j], mean[j] = vals[1]
        err[j] = abs(vals[1][0] - vals[0][0])
        if not (np.isfinite(out[j]) and np.isfinite(mean[j])):
            out[j] = mean[j] = err[j] = np.nan
            info[j] = NGP_INFO_NOT_FINITE
    return out, mean, err, info


class MixtureMarginals:
    """The per-date marginals of a Gaussian mixture — ``means`` [C, m], ``variances`` [C, m],
    ``weights`` [C] — and their exact summaries, each returned date-major ([m], [m, Q]: the
    orientation of ``forecast``'s [m, draws]):

        cdf(x)        F_j(x) = sum_c w_c Phi((x - mu_cj) / sd_cj)
        quantile(p)   F_j(q) = p, to the last bits of q; ``inv_transformation`` is applied
                      elementwise to the exact quantiles — for a monotone non-decreasing map (the
                      inverses of ``nowcast.get_transformations``, clamp at 0 included) that IS the
                      quantile on the original scale
        crps(y)       E|X - y| - E|X - X'| / 2 in closed form, on the MODEL's (transformed) scale.
                      The reference's vignette scores crps(log(y), log.(X)) on draws mapped back
                      to counts: that is this number only when the fit used a log transformation.
                      For any other fit, and for the natural scale, pass ``inv_transformation``
                      (an inverse of ``nowcast.get_transformations``) and ``scale="natural"`` or
                      ``"log"`` (log(. + shift)): the exact CRPS of the transformed forecast against
                      y on the ORIGINAL scale, by quadrature in the mixture's own CDF
                      (``ngp_mixture_crps_mapped``); ``return_error=True`` adds its error estimate
        mean()        of the model's scale; with ``inv_transformation`` / ``scale`` of the mapped one
        wis(y, levels) weighted interval score from the exact quantiles, on either scale
        pit(y)        F_j(y_j)

    With an engine that has ``mixture_cdf`` / ``mixture_quantiles`` / ``mixture_crps`` (the HIP
    library, include/ngp.h) those compute; without one the same formulas run on the host with
    ``math.erf`` / ``math.erfc`` — for small mixtures only (the CRPS is C^2 terms per date)."""

    def __init__(self, means, variances, weights, engine=None):
        self.means = np.ascontiguousarray(np.asarray(means, dtype=np.float64))
        self.variances = np.ascontiguousarray(np.asarray(variances, dtype=np.float64))
        w = np.asarray(weights, dtype=np.float64)
        if (self.means.ndim != 2 or self.variances.shape != self.means.shape
                or w.shape != (self.means.shape[0],)):
            raise ValueError("MixtureMarginals: means [C, m], variances [C, m], weights [C]")
        self.weights = w / np.sum(w)
        self.engine = engine

    @classmethod
    def pool(cls, parts: Sequence["MixtureMarginals"], weights=None) -> "MixtureMarginals":
        """One mixture of several on the same dates: part d weighs ``weights[d]`` (1 / D each when
        not given — scenarios that get equal shares of the draws)."""
        parts = list(parts)
        D = len(parts)
        pw = np.full(D, 1.0 / D) if weights is None else np.asarray(weights, dtype=np.float64)
        if pw.shape != (D,):
            raise ValueError("MixtureMarginals.pool: one weight per part")
        return cls(np.concatenate([p.means for p in parts]),
                   np.concatenate([p.variances for p in parts]),
                   np.concatenate([a * p.weights for a, p in zip(pw, parts)]),
                   engine=next((p.engine for p in parts if p.engine is not None), None))

    # ---- plumbing ---------------------------------------------------------------------------
    def _device(self, name):
        return getattr(self.engine, name, None) if self.engine is not None else None

    @staticmethod
    def _check(info):
        bad = np.flatnonzero(info)
        if bad.size:      # a variance that is not positive: the covariance it came from is not either
            raise PosDefException(int(bad[0]) + 1, int(info[bad[0]]) - 1)

    def _host_info(self):
        act = self.weights > 0
        ok = np.isfinite(self.means) & np.isfinite(self.variances) & (self.variances > 0)
        bad = ~ok & act[:, None]
        return np.where(bad.any(axis=0), bad.argmax(axis=0) + 1, 0)

    def _active(self):
        act = self.weights > 0
        return self.weights[act], self.means[act], self.variances[act]

    def _host_cdf(self, x, density=False):
        """x [m, K] -> F [m, K] (and the density)"""
        w, mu, var = self._active()
        inv = 1.0 / np.sqrt(2.0 * var)                                   # [C, m]
        t = (x[None, :, :] - mu[:, :, None]) * inv[:, :, None]          # [C, m, K]
        F = np.einsum("c,cmk->mk", w, 0.5 * _erfc(-t).astype(np.float64))
        if not density:
            return F
        f = np.einsum("c,cmk->mk", w, inv[:, :, None] * np.exp(-t * t)) / math.sqrt(math.pi)
        return F, f

    # ---- summaries --------------------------------------------------------------------------
    def mean(self, inv_transformation=None, scale="model", shift=0.0, tol=None):
        if inv_transformation is None and scale == "model":
            return self.weights @ self.means
        return self._mapped(None, inv_transformation, scale, shift, tol)[1]

    # ---- scores on the natural / log scale ----------------------------------------------------
    def _mapped(self, y, inv_transformation, scale, shift, tol):
        """(crps, mean, err) of s(g(X)) per date; y None: any admissible y (the mean does not
        depend on it)"""
        from ._abi import NGP_INFO_NOT_CONVERGED, NGP_INFO_NOT_FINITE, NGP_INV_IDENTITY
        if scale not in ("natural", "log"):
            raise ValueError('scale: "model", "natural" or "log"')
        inv = (getattr(inv_transformation, "ngp_inv", None) if inv_transformation is not None
               else (NGP_INV_IDENTITY, 0.0, 0.0, 0.0))
        if inv is None:
            raise ValueError("inv_transformation: an inverse of nowcast.get_transformations")
        sc = 1 if scale == "log" else 0
        m = self.means.shape[1]
        if y is None:
            centre = self.weights @ self.means
            y = np.asarray(inv_transformation(centre) if inv_transformation is not None else centre,
                           dtype=np.float64)
            if sc:
                y = np.maximum(y, 1.0 - shift)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if y.size != m:
            raise ValueError("MixtureMarginals.crps: y [m]")
        dev = self._device("mixture_crps_mapped")
        if dev is not None:
            out, mean, err, info = dev(self.weights, self.means, self.variances, inv, sc,
                                       float(shift), y, 0.0 if tol is None else float(tol))
        else:
            self._check(self._host_info())
            out, mean, err, info = _host_mapped(*self._active(), inv, sc, float(shift), y)
        self._check(np.where(info > 0, info, 0))
        if np.any(info == NGP_INFO_NOT_FINITE):
            raise ArithmeticError("the score is infinite or the inverse is not monotone where the "
                                  f"forecast has mass (dates {np.flatnonzero(info == NGP_INFO_NOT_FINITE)})")
        if np.any(info == NGP_INFO_NOT_CONVERGED):
            import warnings
            warnings.warn("mixture_crps_mapped: panel cap reached, see the error estimate")
        return out, mean, err

    def wis(self, y, levels, inv_transformation=None, scale="model", shift=0.0):
        """Weighted interval score (Bracher et al. 2021) from the exact quantiles: ``levels`` the
        central coverage levels 1 - alpha in (0, 1);
        (|y - med| / 2 + sum_k alpha_k / 2 IS_alpha_k) / (K + 1 / 2) per date, on the model's
        scale, or with ``inv_transformation`` on the natural / log(. + shift) scale (y then on the
        original scale)."""
        lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
        if lv.ndim != 1 or not np.all((lv > 0) & (lv < 1)):
            raise ValueError("MixtureMarginals.wis: levels in (0, 1)")
        if scale not in ("model", "natural", "log"):
            raise ValueError('scale: "model", "natural" or "log"')
        alpha = 1.0 - lv
        probs = np.concatenate([[0.5], alpha / 2, 1.0 - alpha / 2])
        kw = {} if inv_transformation is None else {"inv_transformation": inv_transformation}
        q = self.quantile(probs, **kw)                                    # [m, 1 + 2 K]
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if scale == "log":
            q, y = np.log(q + shift), np.log(y + shift)
        K = lv.size
        lo, hi = q[:, 1:1 + K], q[:, 1 + K:]
        yy = y[:, None]
        score = (hi - lo) + (2.0 / alpha) * (np.maximum(lo - yy, 0.0) + np.maximum(yy - hi, 0.0))
        return (0.5 * np.abs(y - q[:, 0]) + (0.5 * alpha * score).sum(axis=1)) / (K + 0.5)

    def cdf(self, x):
        x = np.asarray(x, dtype=np.float64)
        m = self.means.shape[1]
        xs = x.reshape(m, -1) if x.ndim <= 1 else x
        if xs.shape[0] != m or (x.ndim <= 1 and x.size != m):
            raise ValueError("MixtureMarginals.cdf: x [m] or [m, K]")
        dev = self._device("mixture_cdf")
        if dev is not None:
            F, info = dev(self.weights, self.means, self.variances, np.ascontiguousarray(xs))
        else:
            info = self._host_info()
            self._check(info)
            F = self._host_cdf(xs)
        self._check(info)
        return F[:, 0] if x.ndim <= 1 else F

    def pit(self, y):
        return self.cdf(np.asarray(y, dtype=np.float64).reshape(-1))

    def quantile(self, probs, inv_transformation=lambda y: y):
        p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if p.ndim != 1 or not np.all((p > 0) & (p < 1)):
            raise ValueError("MixtureMarginals.quantile: probs in (0, 1)")
        dev = self._device("mixture_quantiles")
        if dev is not None:
            q, info = dev(self.weights, self.means, self.variances, p)
            self._check(info)
        else:
            self._check(self._host_info())
            q = self._host_quantile(p)
        from .nowcast import _apply
        return _apply(inv_transformation, q)

    def _host_quantile(self, p):
        """bisection on the host CDF until no number is left between the ends: F(lo) < p <= F(hi)"""
        w, mu, var = self._active()
        m = mu.shape[1]
        sd = np.sqrt(var)
        lo = np.repeat((mu - 40.0 * sd).min(axis=0)[:, None], p.size, axis=1)
        hi = np.repeat((mu + 40.0 * sd).max(axis=0)[:, None], p.size, axis=1)
        for _ in range(1200):
            mid = 0.5 * lo + 0.5 * hi
            live = (mid > lo) & (mid < hi)
            if not live.any():
                break
            below = self._host_cdf(mid) < p[None, :]
            lo = np.where(live & below, mid, lo)
            hi = np.where(live & ~below, mid, hi)
        return hi

    def crps(self, y, inv_transformation=None, scale="model", shift=0.0, tol=None,
             return_error=False):
        if inv_transformation is not None or scale != "model":
            out, _, err = self._mapped(y, inv_transformation, scale, shift, tol)
            return (out, err) if return_error else out
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        m = self.means.shape[1]
        if y.size != m:
            raise ValueError("MixtureMarginals.crps: y [m]")
        dev = self._device("mixture_crps")
        if dev is not None:
            out, info = dev(self.weights, self.means, self.variances, y)
            self._check(info)
            return out
        self._check(self._host_info())
        w, mu, var = self._active()
        out = np.empty(m)
        for j in range(m):
            t1 = float(w @ _abs_moment(y[j] - mu[:, j], var[:, j]))
            a = _abs_moment(mu[:, j][:, None] - mu[:, j][None, :], var[:, j][:, None] + var[:, j][None, :])
            out[j] = t1 - 0.5 * float(w @ a @ w)
        return out


def predict_mvn(model: GPModel, ds, noise_on_new: bool = True) -> MixtureMVN:
    return predict_mvn_lockstep([model], ds, noise_on_new)[0]


def _predict_marginals(model: GPModel, ds, noise_on_new: bool = True) -> "MixtureMarginals":
    """``predict_mvn(model, ds).marginals()`` without the covariances where they are not needed: on
    a horizon longer than one aux query carries, a model with a resident factor asks ONE long query
    for means and variances alone (``Factor.predict_long`` with ``want_sigma=False``)."""
    ds = list(ds)
    t, _ = _group_obs([model])
    fac = None
    if (horizon_blocks(t.size, 0, len(ds)) is not None and distributed.world()[1] == 1
            and not model.__dict__.get("_one_shot_predict", False)):
        fac = model._factor()
    if fac is None or not hasattr(fac, "predict_long"):
        return predict_mvn(model, ds, noise_on_new).marginals(engine=model._eng())
    t_new = model.ds_transform.apply(to_days(ds))
    mu, var, _, info = fac.predict_long(t_new, noise_on_new=noise_on_new, want_sigma=False)
    _raise_if_failed(info)
    w, _ = distributed.normalize_log_weights(model.log_weights[:, None],
                                             P_total=model.n_particles_total)
    sl_ = model.y_transform.slope
    return MixtureMarginals((mu[:, 0] - model.y_transform.intercept) / sl_, var / (sl_ * sl_),
                            w[:, 0], engine=model._eng())


def origin_counts(model: GPModel, origins) -> np.ndarray:
    """Forecast origins as observation counts in the factor's order: an integer is a count, a date
    means "the data up to and including that date".  Refuses (``ValueError``) observed dates that
    are not strictly increasing in that order, a count outside 1 .. n and a date before the first
    observation; a date past the last observation is the whole series."""
    idx = np.sort(model._perm[:model.n_obs])
    days = model.days[idx]
    if days.size < 1 or np.any(np.diff(days) <= 0):
        raise ValueError("predict_origins: the observed dates must be strictly increasing in the "
                         "order the model holds them, so that a prefix is what was known at a date")
    out = []
    for o in list(origins):
        if isinstance(o, (int, np.integer)) and not isinstance(o, bool):
            c = int(o)
            if not 1 <= c <= days.size:
                raise ValueError(f"predict_origins: origin {c} is not a count in 1 .. {days.size}")
        else:
            c = int(np.searchsorted(days, to_days([o])[0], side="right"))
            if c < 1:
                raise ValueError(f"predict_origins: origin {o} lies before the first observation")
        out.append(c)
    if not out:
        raise ValueError("predict_origins: at least one origin")
    return np.asarray(out, dtype=np.int32)


def origin_log_weights(log_weights, logml, logml_n):
    """log w_p(r) = log w_p + log p(y_1:c_r | p) - log p(y_1:n | p): what the fitted weights would
    have been at origin r had the particles been the same.  ``logml`` [P, R], ``logml_n`` [P]."""
    return np.stack([_advance_weights(np.asarray(log_weights, dtype=np.float64), logml[:, r], logml_n)
                     for r in range(logml.shape[1])], axis=1)


def _host_origins(model: GPModel, cuts, t_new, noise_on_new):
    """one ``engine.predict`` per origin on the prefix (in blocks of dates where one call does not
    carry them all; only the marginals are kept)"""
    from ._abi import NGP_MAX_AUX
    eng, progs = model._eng(), model.programs()
    t, y = model._obs()
    P, m = len(progs), t_new.size
    mu, var = np.empty((P, cuts.size, m)), np.empty((P, cuts.size, m))
    lm = np.empty((P, cuts.size))
    for r, c in enumerate(cuts):
        blk = max(1, NGP_MAX_AUX - (int(c) % 64) - 1)
        for lo in range(0, m, blk):
            a, sg, l, info = eng.predict(progs, t[:c], y[:c], t_new[lo:lo + blk], noise_on_new)
            _raise_if_failed(info)
            mu[:, r, lo:lo + blk] = a
            var[:, r, lo:lo + blk] = np.einsum("pjj->pj", sg)
            lm[:, r] = l
    return mu, var, lm


def predict_origins(model: GPModel, origins, ds, noise_on_new: bool = True, weights: str = "fitted"):
    """Hindcasts of a fitted model: what would it have forecast for the dates ``ds`` knowing only
    the data up to each origin (``origin_counts``)?  The particles — structures and parameters —
    are the fitted ones; only the data they are conditioned on is cut.  Returns
    ``(marginals, ess)``: a ``MixtureMarginals`` over ``ds`` per origin and the effective sample
    size per origin.

    ``weights="fitted"`` keeps the model's weights; ``"origin"`` reweights each particle by the
    evidence of the prefix (``origin_log_weights``).  A model with a resident factor asks ONE device
    query for all origins (``Factor.predict_origins``: running sums along the solved panel of the
    long query, no factorisation per origin); any other engine is asked one ``predict`` per origin
    on the prefix."""
    if weights not in ("fitted", "origin"):
        raise ValueError('predict_origins: weights "fitted" or "origin"')
    cuts = origin_counts(model, origins)
    n = model.n_obs
    # the device call wants strictly increasing cuts; the whole series rides along for "origin"
    uniq, back = np.unique(np.concatenate([cuts, [n]]) if weights == "origin" else cuts,
                           return_inverse=True)
    uniq = uniq.astype(np.int32)
    t_new = model.ds_transform.apply(to_days(list(ds)))
    fac = None
    if distributed.world()[1] == 1 and not model.__dict__.get("_one_shot_predict", False):
        fac = model._factor()
    if fac is not None and hasattr(fac, "predict_origins"):
        mu, var, lm, info = fac.predict_origins(uniq, t_new, noise_on_new)
        _raise_if_failed(info)
    else:
        mu, var, lm = _host_origins(model, uniq, t_new, noise_on_new)
    R = cuts.size
    logw = np.repeat(np.asarray(model.log_weights, dtype=np.float64)[:, None], R, axis=1)
    if weights == "origin":
        logw = origin_log_weights(model.log_weights, lm[:, back[:R]], lm[:, back[R]])
    w, ess = distributed.normalize_log_weights(logw, P_total=model.n_particles_total)
    sl_, ic = model.y_transform.slope, model.y_transform.intercept
    eng = model._eng()
    return ([MixtureMarginals((mu[:, back[r]] - ic) / sl_, var[:, back[r]] / (sl_ * sl_), w[:, r],
                              engine=eng) for r in range(R)], np.asarray(ess, dtype=np.float64))


def predict_mvn_lockstep(models: Sequence[GPModel], ds, noise_on_new: bool = True) -> List[MixtureMVN]:
    """``predict_mvn`` (reference src/forecasting.jl:46,66) of D models on the same dates: ONE
    engine call of P x D items (a single model goes through its resident factor), and in a
    sharded run ONE all-gather that carries every model's means, covariances and weights."""
    D = len(models)
    t, ys = _group_obs(models)
    t_new = models[0].ds_transform.apply(to_days(list(ds)))
    eng = models[0]._eng()
    # (a scenario clone that forecasts once asks the one-shot entry point — concurrent tasks'
    # calls are combined there, include/ngp.h "concurrent callers" — instead of building a
    # resident factor for a single query)
    fac = (models[0]._factor()
           if D == 1 and not models[0].__dict__.get("_one_shot_predict", False) else None)
    if D > 1:
        progs = [p for m in models for p in m.programs()]
        Y = _item_y(ys, [j for j, m in enumerate(models) for _ in m.particles])

    def call(ts):
        if fac is not None:
            mu_s, sg_s, _, info_s = fac.predict(ts, noise_on_new)
        elif D == 1:
            mu_s, sg_s, _, info_s = eng.predict(models[0].programs(), t, ys[0], ts, noise_on_new)
        else:
            mu_s, sg_s, _, info_s = eng.predict(progs, t, Y, ts, noise_on_new)
        return mu_s, sg_s, info_s, None

    blocks = horizon_blocks(t.size, 0, t_new.size)
    if blocks is None:
        mu, sigma, info, _ = call(t_new)
    elif fac is not None and hasattr(fac, "predict_long"):
        # longer than the aux rows carry: ONE query with the dates as the panel of a solve
        mu, _, sigma, info = fac.predict_long(t_new, noise_on_new=noise_on_new)
        mu = mu[:, 0]
    else:       # longer than one call carries: pairwise calls, joint covariance assembled
        mu, sigma, info, _ = predict_in_blocks(call, t_new, blocks)
    _raise_if_failed(info)
    m = t_new.size
    off = np.concatenate([[0], np.cumsum([len(mm.particles) for mm in models])])
    P_total = models[0].n_particles_total
    logw = np.stack([mm.log_weights for mm in models], axis=1)
    w, _ = distributed.normalize_log_weights(logw, P_total=P_total)           # [P_local, D]
    means, covs = [], []
    for j, mm in enumerate(models):
        sl_ = mm.y_transform.slope
        means.append((mu[off[j]:off[j + 1]] - mm.y_transform.intercept) / sl_)
        covs.append(sigma[off[j]:off[j + 1]] / (sl_ * sl_))
    if distributed.world()[1] > 1:   # every rank returns the full mixtures: one collective
        P_loc = w.shape[0]
        packed = np.concatenate(
            [np.stack(means, axis=1).reshape(P_loc, D * m),
             np.stack(covs, axis=1).reshape(P_loc, D * m * m), w], axis=1)
        packed = distributed.all_gather_rows(packed, sizes=distributed.block_sizes(P_total))
        mm_, cc_ = packed[:, :D * m].reshape(-1, D, m), packed[:, D * m:D * m * (m + 1)].reshape(
            -1, D, m, m)
        w = packed[:, D * m * (m + 1):]
        means = [np.ascontiguousarray(mm_[:, j]) for j in range(D)]
        covs = [np.ascontiguousarray(cc_[:, j]) for j in range(D)]
    # shared stream: the same draws on every rank; the device sampler takes at most NGP_MAX_AUX
    # dates, longer horizons are drawn on the host
    from ._abi import NGP_MAX_AUX
    sampler = getattr(eng, "mixture_sample", None) if t_new.size <= NGP_MAX_AUX else None
    return [MixtureMVN(means[j], covs[j], w[:, j], mm.rng_shared, sampler)
            for j, mm in enumerate(models)]


def rand_lockstep(mixes: Sequence[MixtureMVN], draws: int, engine=None) -> List[np.ndarray]:
    """``rand(dist, draws)`` (reference src/forecasting.jl:47) for D mixtures: with the device
    sampler ONE call (``ngp_mixture_sample_indep``: mixture j keyed by the seed its own stream
    gives, so the draws are those of D separate ``rand`` calls); otherwise mixture by mixture."""
    k = int(draws)
    if not takes_independent_form(engine, mixes, k):
        return [mx.rand(k) for mx in mixes]
    seeds = [int(mx.rng.integers(0, 2**63 - 1)) for mx in mixes]
    out, _, info = engine.mixture_sample_indep(
        np.stack([mx.weights for mx in mixes]), np.stack([mx.means for mx in mixes]),
        np.stack([mx.covs for mx in mixes]), k, seeds)
    _raise_if_failed(info)
    return [np.ascontiguousarray(out[j].T) for j in range(len(mixes))]


def _over_scenario_factors(models: Sequence[GPModel], needs: str, query):
    """Resident factors over whole scenarios of D lockstep models — items mixture-major (model
    after model, every model's particles together), per-item ``y`` rows — with as many scenarios
    per factor as the device holds: all of them first; when the factor's creation or
    ``query(factor, j0, j1)`` (the models j0 .. j1 - 1) is refused with ``NGP_ERR_TOO_LARGE`` the
    factor is closed, the count halved and the work goes on from the same scenario.  One scenario
    that does not fit is the error.  Every factor is closed behind its one query.  Returns the
    queries' results in scenario order, or None (nothing queried) where the engine has no resident
    factor with the method ``needs``."""
    D = len(models)
    P1 = len(models[0].particles)
    if any(len(mm.particles) != P1 for mm in models):
        raise ValueError("scenario factors: the models must hold equally many particles")
    t, ys = _group_obs(models)
    eng = models[0]._eng()
    if getattr(eng, "factor", None) is None:
        return None
    out, j0, per = [], 0, D
    while j0 < D:
        k = min(per, D - j0)
        sub = models[j0:j0 + k]
        fac = None
        try:
            fac = eng.factor([p for mm in sub for p in mm.programs()], t,
                             _item_y(ys[j0:j0 + k], np.repeat(np.arange(k), P1)))
            if not hasattr(fac, needs):
                return None
            out.append(query(fac, j0, j0 + k))
        except Exception as e:      # the engine's own error type: its status says what it is
            if getattr(e, "status", None) != _NGP_ERR_TOO_LARGE or k == 1:
                raise
            per = max(1, k // 2)
            continue
        finally:
            if fac is not None:
                fac.close()
        j0 += k
    return out


_NGP_ERR_TOO_LARGE = -3     # include/ngp.h


def _lockstep_weights(models: Sequence[GPModel]) -> np.ndarray:
    """[P_local, D]: every model's normalised weights, as ``predict_mvn_lockstep`` forms them"""
    logw = np.stack([mm.log_weights for mm in models], axis=1)
    return distributed.normalize_log_weights(logw, P_total=models[0].n_particles_total)[0]


def sample_long_lockstep(models: Sequence[GPModel], ds, draws: int) -> Optional[List[np.ndarray]]:
    """``rand_lockstep(predict_mvn_lockstep(models, ds), draws)`` on a horizon beyond one aux query
    without a covariance leaving the device: factors over whole scenarios
    (``_over_scenario_factors``), ONE ``Factor.sample_long_indep`` call per factor.  Mixture j is
    keyed by one ``integers(0, 2**63 - 1)`` draw of model j's shared stream, taken in model order
    where ``rand_lockstep`` takes the seeds of the device's independent form, so the streams end
    where that form leaves them.  Returns a list of [m, draws] arrays on the models' scale — or
    None, with no stream touched, where the engine's factor has no ``sample_long_indep``."""
    k = int(draws)
    t_new = models[0].ds_transform.apply(to_days(list(ds)))
    w = _lockstep_weights(models)
    seeds = []

    def query(fac, j0, j1):
        if not seeds:       # the first factor stands: only now are the streams touched
            seeds.extend(int(mm.rng_shared.integers(0, 2**63 - 1)) for mm in models)
        out, _, info, cinfo = fac.sample_long_indep(t_new, np.ascontiguousarray(w[:, j0:j1].T), k,
                                                    seeds[j0:j1])
        _raise_if_failed(info)
        _raise_if_failed(cinfo)
        return out

    parts = _over_scenario_factors(models, "sample_long_indep", query)
    if parts is None:
        return None
    out = np.concatenate(parts, axis=0)                                        # [D, draws, m]
    return [np.ascontiguousarray(((out[j] - mm.y_transform.intercept) / mm.y_transform.slope).T)
            for j, mm in enumerate(models)]


def predict_marginals_lockstep(models: Sequence[GPModel], ds,
                               noise_on_new: bool = True) -> Optional[List["MixtureMarginals"]]:
    """``[mx.marginals() for mx in predict_mvn_lockstep(models, ds)]`` without the covariances:
    ``Factor.predict_long(want_sigma=False)`` on the factors of ``sample_long_lockstep`` — no
    m x m array is formed anywhere.  None where the engine's factor has no ``predict_long``."""
    t_new = models[0].ds_transform.apply(to_days(list(ds)))
    w = _lockstep_weights(models)

    def query(fac, j0, j1):
        mu, var, _, info = fac.predict_long(t_new, noise_on_new=noise_on_new, want_sigma=False)
        _raise_if_failed(info)
        return mu[:, 0], var

    parts = _over_scenario_factors(models, "predict_long", query)
    if parts is None:
        return None
    mu = np.concatenate([p[0] for p in parts], axis=0)
    var = np.concatenate([p[1] for p in parts], axis=0)
    P1, eng, res = len(models[0].particles), models[0]._eng(), []
    for j, mm in enumerate(models):
        sl_, rows = mm.y_transform.slope, slice(j * P1, (j + 1) * P1)
        res.append(MixtureMarginals((mu[rows] - mm.y_transform.intercept) / sl_, var[rows] / (sl_ * sl_),
                                    w[:, j], engine=eng))
    return res


def takes_independent_form(engine, mixes: Sequence[MixtureMVN], draws: int) -> bool:
    """Whether ``draws`` draws from each of ``mixes`` are ONE call of the device's independent form
    (``ngp_mixture_sample_indep`` and the targets / scores over it): the engine has it, there are
    at least two mixtures and two draws, and every mixture has a sampler and the same (P, m)."""
    P, m = mixes[0].means.shape
    return (getattr(engine, "mixture_sample_indep", None) is not None and len(mixes) >= 2
            and int(draws) > 1 and m > 0
            and all(mx.sampler is not None and mx.means.shape == (P, m) for mx in mixes))


def _raise_if_failed(info) -> None:
    """``info``: a status per particle, [P] — or [S, P] from the independent forms — 0 or the pivot
    that failed.  Raises ``PosDefException`` for the first failure with its particle (the flat
    index; the last axis' for [S, P])."""
    info = np.atleast_1d(info)
    bad = np.argwhere(info != 0)
    if bad.size:
        raise PosDefException(int(info[tuple(bad[0])]), int(bad[0][-1]))


# ---------------------------------------------------------------------------------------------
# additive decomposition (AutoGP's ``decompose``; include/ngp.h "additive decomposition")
# ---------------------------------------------------------------------------------------------
@dataclass
class Component:
    """One additive part of a particle's kernel.  With ``split="plus"`` a maximal non-Plus subtree
    under the root's Plus nodes, else a sum-of-products term (``ngp_kernel_terms``).  ``kind``:
    "trend" if the part contains a Linear, "seasonal" if it contains a Periodic and no Linear,
    "other" otherwise.  ``split``: the split that was used for this particle (the one asked for, or
    a weaker one it fell back to)."""
    tree: gp.Node
    label: str
    kind: str
    split: str = "plus"


def component_kind(ops) -> str:
    ops = [int(o) for o in ops]
    if gp.LINEAR in ops:
        return "trend"
    return "seasonal" if gp.PERIODIC in ops else "other"


SPLITS = ("plus", "changepoint", "products")      # weakest first; flags of ngp_kernel_terms: 0, 1, 1 | 2
_SPLIT_FLAGS = {"plus": 0, "changepoint": 1, "products": 3}


def _zero(nd: gp.Node) -> bool:
    return nd.op == gp.CONSTANT and nd.params[0] == 0.0


def term_label(tree: gp.Node) -> str:
    """The printed sub-kernel; a windowed term (one side of a ChangePoint, the other side
    Constant(0)) names its side and the change point's location instead of printing the zero."""
    if tree.op == gp.CHANGE_POINT and _zero(tree.right) != _zero(tree.left):
        side, inner = ("before", tree.left) if _zero(tree.right) else ("after", tree.right)
        return f"{term_label(inner)} [{side} {tree.params[0]:.4g}]"
    if tree.op == gp.TIMES:
        return f"Times({term_label(tree.left)}, {term_label(tree.right)})"
    return str(tree)


def decompose(model: GPModel, split: str = "plus", max_terms: Optional[int] = None) -> List[List[Component]]:
    """Per particle, the additive parts of its kernel, left to right.

    ``split="plus"``: the maximal non-Plus subtrees under the root's Plus nodes
    (``ngp_kernel_components``); a ChangePoint or a Times is one part.  ``"changepoint"`` also
    splits a ChangePoint into its two windows (each side's terms blended against Constant(0): the
    device blend is linear in its operands), ``"products"`` in addition distributes a Times over
    the sums below it (``ngp_kernel_terms``).  A particle with more than ``max_terms`` terms
    (default: what leaves room for one forecast date beside the factor, NGP_MAX_AUX - (n mod 64) -
    2) falls back to the next weaker split; ``Component.split`` records the one used."""
    from . import _lib
    from ._abi import NGP_MAX_AUX
    if split not in _SPLIT_FLAGS:
        raise ValueError(f'decompose: split is one of {", ".join(SPLITS)}')
    if split == "plus":
        out = []
        for ops, params, noise in model.programs():
            parts = []
            for c_ops, c_par, _ in _lib.kernel_components((ops, params, noise)):
                tree = gp.from_program(c_ops, c_par)
                parts.append(Component(tree, str(tree), component_kind(c_ops)))
            out.append(parts)
        return out
    if max_terms is None:
        max_terms = NGP_MAX_AUX - (model._obs()[0].size % 64) - 2
    out = []
    for prog in model.programs():
        for used in reversed(SPLITS[:SPLITS.index(split) + 1]):
            try:
                terms = _lib.kernel_terms(prog, _SPLIT_FLAGS[used], max_terms if used != "plus" else None)
                break
            except _lib.NgpError as e:
                if e.status != -3 or used == "plus":      # NGP_ERR_TOO_LARGE: the next weaker split
                    raise
        parts = []
        for c_ops, c_par, _ in terms:
            tree = gp.from_program(c_ops, c_par)
            parts.append(Component(tree, term_label(tree), component_kind(c_ops), used))
        out.append(parts)
    return out


class AtomMixtureMarginals(MixtureMarginals):
    """A mixture whose share ``atom`` sits in a point mass at 0 (particles that have no component
    of a group contribute exactly 0 to that group); ``means`` / ``variances`` / ``weights`` are the
    continuous components, the weights summing to 1 among themselves.  The point mass is handled
    here, on the host; the continuous rest is a ``MixtureMarginals`` like any other.  The scores
    on the natural / log scale (``crps`` / ``mean`` / ``wis`` with ``inv_transformation`` or a
    ``scale`` other than "model") are NOT implemented for it: they raise ``NotImplementedError``."""

    def __init__(self, means, variances, weights, atom: float, engine=None):
        super().__init__(means, variances, weights, engine=engine)
        if not 0.0 < atom < 1.0:
            raise ValueError("AtomMixtureMarginals: 0 < atom < 1")
        self.atom = float(atom)

    def _rest(self):
        return MixtureMarginals(self.means, self.variances, self.weights, engine=self.engine)

    @staticmethod
    def _model_scale_only(inv_transformation, scale):
        if inv_transformation is not None or scale != "model":
            raise NotImplementedError("AtomMixtureMarginals: scores on the model's scale only")

    def mean(self, inv_transformation=None, scale="model", shift=0.0, tol=None):
        self._model_scale_only(inv_transformation, scale)
        return (1.0 - self.atom) * super().mean()

    def wis(self, y, levels, inv_transformation=None, scale="model", shift=0.0):
        self._model_scale_only(inv_transformation, scale)
        return super().wis(y, levels)

    def cdf(self, x):
        x = np.asarray(x, dtype=np.float64)
        m = self.means.shape[1]
        F = self._rest().cdf(x)
        step = (x.reshape(m, -1) >= 0.0).astype(np.float64).reshape(F.shape)
        return (1.0 - self.atom) * F + self.atom * step

    def quantile(self, probs, inv_transformation=lambda y: y):
        p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if p.ndim != 1 or not np.all((p > 0) & (p < 1)):
            raise ValueError("MixtureMarginals.quantile: probs in (0, 1)")
        a, rest = self.atom, self._rest()
        m = self.means.shape[1]
        F0 = (1.0 - a) * rest.cdf(np.zeros(m))                    # mass strictly below the atom
        below, above = p / (1.0 - a), (p - a) / (1.0 - a)         # levels of the rest on either side
        q = np.zeros((m, p.size))
        for levels, pick in ((below, p[None, :] < F0[:, None]), (above, p[None, :] > F0[:, None] + a)):
            ok = (levels > 0) & (levels < 1)
            if ok.any() and pick[:, ok].any():
                q[:, ok] = np.where(pick[:, ok], rest.quantile(levels[ok]), q[:, ok])
        from .nowcast import _apply
        return _apply(inv_transformation, q)

    def crps(self, y, inv_transformation=None, scale="model", shift=0.0, tol=None,
             return_error=False):
        self._model_scale_only(inv_transformation, scale)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        a, rest = self.atom, self._rest()
        c_rest = rest.crps(y)                                     # E|X - y| - E|X - X'| / 2 of the rest
        w, mu, var = rest._active()
        e_y = w @ _abs_moment(y[None, :] - mu, var)
        e_0 = w @ _abs_moment(mu, var)
        e_xx = 2.0 * (e_y - c_rest)
        return ((1.0 - a) * e_y + a * np.abs(y)
                - 0.5 * ((1.0 - a) ** 2 * e_xx + 2.0 * a * (1.0 - a) * e_0))


class ComponentForecast:
    """The joint posterior of every particle's additive parts on the forecast dates, on the
    ORIGINAL scale of y (what ``predict_components`` returns):

        means[p]  [C_p, m]          posterior mean of part c
        sigma[p]  [C_p m, C_p m]    joint covariance of the parts, row = c m + j; None when the
                                    forecast carries ``cross`` alone
        var[p]    [C_p, m]          its diagonal (always there)
        cross                       None, or per particle [C_p, C_p, m]: the covariance of parts c, c'
                                    at the SAME date (``ngp_factor_components_long``) — all that
                                    ``grouped`` reads
        weights   [P]               particle weights
        kinds[p], labels[p]         per part: "trend" / "seasonal" / "other", the printed sub-kernel
        offset                      the constant of the y-transform: it belongs to no part, the
                                    forecast without noise is  offset + sum_c part_c
        date_blocks                 None, or the (lo, hi) blocks of dates a long horizon was served
                                    in: covariances ACROSS blocks are then not formed and ``sigma`` is
                                    block-diagonal in dates (zeros elsewhere)

    The parts are the latent functions; observation noise is a part of its own (the remainder) and
    appears nowhere here."""

    def __init__(self, means, sigma, var, weights, kinds, labels, offset, date_blocks=None, engine=None,
                 cross=None):
        self.means, self.sigma, self.var, self.cross = means, sigma, var, cross
        self.weights = np.asarray(weights, dtype=np.float64)
        self.kinds, self.labels, self.offset = kinds, labels, float(offset)
        self.date_blocks, self.engine = date_blocks, engine

    def grouped(self, by: str = "kind"):
        """Per group, the weighted mixture over particles of the SUM of that group's parts: mean
        sum_{c in g} mu_c, variance per date sum_{c, c' in g} Sigma_cc'[j, j].  ``by``: "kind" or
        "label".  A particle without a part in a group contributes a point mass at 0 (an
        ``AtomMixtureMarginals``); groups are the ones at least one particle has."""
        keys = {"kind": self.kinds, "label": self.labels}.get(by)
        if keys is None:
            raise ValueError('ComponentForecast.grouped: by = "kind" or "label"')
        names = []
        for ks in keys:
            for k in ks:
                if k not in names:
                    names.append(k)
        out = {}
        for name in names:
            mus, vs, ws, atom = [], [], [], 0.0
            for p, ks in enumerate(keys):
                idx = [c for c, k in enumerate(ks) if k == name]
                if not idx:
                    atom += self.weights[p]
                    continue
                C, m = self.means[p].shape
                if self.cross is not None:
                    blocks = self.cross[p]
                else:
                    blocks = np.einsum("ajbj->abj", self.sigma[p].reshape(C, m, C, m))   # same-date entries
                mus.append(self.means[p][idx].sum(axis=0))
                vs.append(blocks[np.ix_(idx, idx)].sum(axis=(0, 1)))
                ws.append(self.weights[p])
            atom /= float(np.sum(self.weights))
            if atom > 0.0:
                out[name] = AtomMixtureMarginals(np.stack(mus), np.stack(vs), np.asarray(ws), atom,
                                                 engine=self.engine)
            else:
                out[name] = MixtureMarginals(np.stack(mus), np.stack(vs), np.asarray(ws),
                                             engine=self.engine)
        return out


def component_blocks(n_obs: int, c_max: int, m: int, d: int = 0):
    """The C m component rows of a particle share the aux block with the tail observations, the d
    appended points and the y row: (n mod 64) + d + 1 + C m <= NGP_MAX_AUX (include/ngp.h).  None
    when the m dates fit one call, else the (lo, hi) blocks of dates to query one by one."""
    from ._abi import NGP_MAX_AUX
    per = (NGP_MAX_AUX - (n_obs % 64) - d - 1) // max(c_max, 1)
    if m <= per:
        return None
    if per < 1:
        raise ValueError(f"predict_components: a kernel of {c_max} additive parts leaves no room "
                         f"for a forecast date beside the factor (NGP_MAX_AUX = {NGP_MAX_AUX} rows)")
    return [(lo, min(lo + per, m)) for lo in range(0, m, per)]


def long_component_forecast(model: GPModel, parts, o, weights) -> ComponentForecast:
    """The ``ComponentForecast`` of one ``components_long`` result ``o`` on the original scale:
    ``means[p]`` is [C_p, S, m] as the query returns it, ``var`` the c = c' planes of ``cross``,
    ``sigma`` None unless the query formed it."""
    _raise_if_failed(o["info"])
    inv = 1.0 / model.y_transform.slope           # y = (y_model - intercept) / slope
    cross = [a * (inv * inv) for a in o["cross"]]
    var = [np.ascontiguousarray(np.einsum("ccj->cj", a)) for a in cross]
    sigma = [a * (inv * inv) for a in o["sigma"]] if o["sigma"] is not None else [None] * len(parts)
    return ComponentForecast([a * inv for a in o["mu"]], sigma, var, weights,
                             [[c.kind for c in ps] for ps in parts], [[c.label for c in ps] for ps in parts],
                             -model.y_transform.intercept * inv, None, engine=model._eng(), cross=cross)


def predict_components(model: GPModel, ds, split: str = "plus", one_query: bool = False,
                       want_sigma: bool = False) -> ComponentForecast:
    """The additive decomposition of the model's forecast on the dates ``ds``: ONE query of the
    model's resident factor (``ngp_factor_components``) per block of dates — no refit on a
    sub-kernel, which would not be conditioned on the same K.  Needs an engine with resident
    factors (there is no host path).  In a sharded run every rank gets its own particles' parts,
    with their globally normalised weights.  ``split``: as ``decompose``.

    ``one_query=True`` (with a factor that has ``components_long``): ONE call whatever the horizon
    (``ngp_factor_components_long``); ``date_blocks`` is None, the forecast carries ``cross``,
    ``var`` is its diagonal planes and ``sigma`` is the full joint covariance with ``want_sigma``,
    else None per particle.  ``want_sigma`` has no effect on the default path, which always returns
    its block-diagonal ``sigma``."""
    fac = model._factor()
    if fac is None or not hasattr(fac, "components"):
        raise RuntimeError("predict_components needs the engine's resident factor (ngp_factor_components)")
    parts = decompose(model, split)
    comps = [[gp.to_program(c.tree) + (0.0,) for c in ps] for ps in parts]
    t, _ = model._obs()
    t_new = model.ds_transform.apply(to_days(list(ds)))
    m = t_new.size
    if one_query and hasattr(fac, "components_long"):
        w, _ = distributed.normalize_log_weights(model.log_weights[:, None],
                                                 P_total=model.n_particles_total)
        o = fac.components_long(comps, t_new, want_sigma=want_sigma)
        o = dict(o, mu=[a[:, 0, :] for a in o["mu"]])
        return long_component_forecast(model, parts, o, w[:, 0])
    blocks = component_blocks(t.size, max(len(ps) for ps in parts), m)
    P = len(parts)
    means = [np.empty((len(ps), m)) for ps in parts]
    var = [np.empty((len(ps), m)) for ps in parts]
    sigma = [np.zeros((len(ps) * m, len(ps) * m)) for ps in parts]
    for lo, hi in (blocks or [(0, m)]):
        o = fac.components(comps, t_new[lo:hi])
        _raise_if_failed(o["info"])
        k = hi - lo
        for p in range(P):
            C = len(parts[p])
            means[p][:, lo:hi] = o["mu"][p]
            var[p][:, lo:hi] = o["var"][p]
            sigma[p].reshape(C, m, C, m)[:, lo:hi, :, lo:hi] = o["sigma"][p].reshape(C, k, C, k)
    inv = 1.0 / model.y_transform.slope           # y = (y_model - intercept) / slope
    means = [a * inv for a in means]
    var = [a * (inv * inv) for a in var]
    sigma = [a * (inv * inv) for a in sigma]
    w, _ = distributed.normalize_log_weights(model.log_weights[:, None],
                                             P_total=model.n_particles_total)
    return ComponentForecast(means, sigma, var, w[:, 0], [[c.kind for c in ps] for ps in parts],
                             [[c.label for c in ps] for ps in parts],
                             -model.y_transform.intercept * inv, blocks, engine=model._eng())


# ---------------------------------------------------------------------------------------------
# trajectory targets (include/ngp.h "trajectory targets")
# ---------------------------------------------------------------------------------------------
TARGET_KINDS = {"sum": 0, "max": 1, "diff": 2, "argmax": 3, "exceed": 4}
REAL_TARGETS = (0, 1, 2)


def _target_tuples(targets, m: int):
    """(kind, j0, j1[, thr]) with kind a name of TARGET_KINDS or its code -> [(code, j0, j1, thr)]"""
    out = []
    for tg in targets:
        kind, j0, j1 = tg[0], int(tg[1]), int(tg[2])
        thr = float(tg[3]) if len(tg) > 3 else 0.0
        code = TARGET_KINDS[kind] if isinstance(kind, str) else int(kind)
        if code not in TARGET_KINDS.values() or not 0 <= j0 <= j1 < m or not np.isfinite(thr):
            raise ValueError(f"path target {tg!r}: kind in {sorted(TARGET_KINDS)}, 0 <= j0 <= j1 < {m}, "
                             "finite threshold")
        out.append((code, j0, j1, thr))
    if not out:
        raise ValueError("path_targets: at least one target")
    return out


def quantile_rank(p: float, N: int) -> int:
    """1-based rank of the order statistic that stands for level p among N paths:
    clamp(ceil(p N), 1, N), the product taken in float64 as the library takes it."""
    return int(min(max(int(math.ceil(float(p) * float(N))), 1), N))


def path_functionals(v: np.ndarray, targets) -> np.ndarray:
    """v [N, m] paths on the original scale, targets [(code, j0, j1, thr)] -> values [T, N], with
    the definitions of include/ngp.h (sum in ascending date order; first index of the maximum)."""
    out = np.empty((len(targets), v.shape[0]))
    for t, (code, j0, j1, thr) in enumerate(targets):
        win = v[:, j0:j1 + 1]
        if code == 0:
            acc = np.zeros(v.shape[0])
            for j in range(win.shape[1]):
                acc = acc + win[:, j]
            out[t] = acc
        elif code == 1:
            out[t] = win.max(axis=1)
        elif code == 2:
            out[t] = v[:, j1] - v[:, j0]
        elif code == 3:
            out[t] = j0 + np.argmax(win, axis=1)
        else:
            out[t] = (win.max(axis=1) > thr).astype(np.float64)
    return out + 0.0


def summarize_path_values(values: np.ndarray, targets, probs, m: int):
    """The summaries of include/ngp.h from values [T, N]: q [T, Q] (order statistics), mean, count,
    hist [T, m]."""
    T, N = values.shape
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    q = np.full((T, probs.size), np.nan)
    count, hist = np.zeros(T, dtype=np.int64), np.zeros((T, m), dtype=np.int64)
    ks = np.array([quantile_rank(p, N) for p in probs], dtype=np.int64) - 1
    for t, (code, j0, j1, thr) in enumerate(targets):
        if code in REAL_TARGETS:
            q[t] = np.sort(values[t])[ks]
            count[t] = int(np.sum(values[t] > thr))
        elif code == 3:
            hist[t] = np.bincount(values[t].astype(np.int64), minlength=m)
        else:
            count[t] = int(np.sum(values[t] > 0.5))
    return q, values.mean(axis=1), count, hist


class PathTargets:
    """Summaries of functionals of whole forecast paths (``path_targets``): per target t

        quantile(t)            the levels' order statistics among the N paths (real-valued kinds)
        mean(t)                mean over the paths (``exceed``: the probability; ``argmax``: mean index)
        prob_above(t)          share of paths above the target's threshold (``exceed``: of paths
                               that exceed it anywhere in the window)
        peak_distribution(t)   ``argmax``: share of paths whose peak is at each date, [m]
        values(t)              every path's value, if they were asked for
    """

    def __init__(self, targets, probs, q, mean, count, hist, N, values=None, device=False):
        self.targets, self.probs = list(targets), np.asarray(probs, dtype=np.float64)
        self.q, self._mean, self.count, self.hist = q, mean, count, hist
        self.N, self._values, self.device = int(N), values, bool(device)

    def quantile(self, t: int = 0):
        if self.targets[t][0] not in REAL_TARGETS:
            raise ValueError("quantile: a sum, max or diff target")
        return self.q[t].copy()

    def mean(self, t: int = 0) -> float:
        return float(self._mean[t])

    def prob_above(self, t: int = 0) -> float:
        if self.targets[t][0] == 3:
            raise ValueError("prob_above: not for an argmax target")
        return float(self.count[t]) / self.N

    def peak_distribution(self, t: int = 0):
        if self.targets[t][0] != 3:
            raise ValueError("peak_distribution: an argmax target")
        return self.hist[t] / float(self.N)

    def values(self, t: int = 0):
        if self._values is None:
            raise ValueError("values: call path_targets(..., want_values=True)")
        return self._values[t]


def _mixture_arrays(mixes_or_arrays, seed, who: str):
    """(w, mu, sigma, seed) in the sampler's layouts from one ``MixtureMVN``, a sequence of them or
    the arrays themselves (``path_targets``); seed a scalar (shared components) or a list of S."""
    if isinstance(mixes_or_arrays, MixtureMVN):
        mixes_or_arrays = [mixes_or_arrays]
    if isinstance(mixes_or_arrays[0], MixtureMVN):
        mixes = list(mixes_or_arrays)
        if seed is None:
            seed = [int(mx.rng.integers(0, 2**63 - 1)) for mx in mixes]
        elif np.isscalar(seed):
            seed = [int(seed)] if len(mixes) == 1 else None
        if seed is None or len(seed) != len(mixes):
            raise ValueError(f"{who}: one seed per mixture")
        w = np.stack([mx.weights for mx in mixes])
        mu = np.stack([mx.means for mx in mixes])
        sigma = np.stack([mx.covs for mx in mixes])
        seed = [int(v) for v in seed]
    else:
        w, mu, sigma = (np.asarray(a, dtype=np.float64) for a in mixes_or_arrays)
        if seed is None:
            raise ValueError(f"{who}: arrays need a seed")
        seed = int(seed) if np.isscalar(seed) else [int(v) for v in seed]
    return w, mu, sigma, seed


def _host_paths(engine, w, mu, sigma, draws: int, seed, inv_transformation):
    """x [N, m]: the engine's sampler (numpy without one) for the arguments of ``_mixture_arrays``,
    then the inverse transformation in numpy — the host path of ``path_targets``."""
    indep = not np.isscalar(seed)
    S, m, N = w.shape[0], mu.shape[2], w.shape[0] * int(draws)
    sampler = getattr(engine, "mixture_sample_indep" if indep else "mixture_sample", None)
    if sampler is not None:
        x, _, info = sampler(w, mu, sigma, int(draws), seed)
        _raise_if_failed(info)
    elif indep and getattr(engine, "mixture_sample", None) is not None:
        # mixture s of the independent form IS a one-mixture call keyed by seeds[s]
        x = []
        for s in range(S):
            xs, _, info = engine.mixture_sample(w[s:s + 1], np.ascontiguousarray(mu[s][:, None, :]),
                                                sigma[s], int(draws), seed[s])
            _raise_if_failed(info)
            x.append(xs[0])
        x = np.stack(x)
    elif indep:
        x = np.stack([MixtureMVN(mu[s], sigma[s], w[s], np.random.default_rng(seed[s])).rand(int(draws)).T
                      for s in range(S)])
    else:
        rng = np.random.default_rng(seed)
        x = np.stack([MixtureMVN(mu[:, s], sigma, w[s], rng).rand(int(draws)).T for s in range(S)])
    x = np.ascontiguousarray(x.reshape(N, m))
    if inv_transformation is not None:
        from .nowcast import _apply
        x = _apply(inv_transformation, x)
    return x


def path_targets(mixes_or_arrays, targets, probs, draws: int, seed=None, inv_transformation=None, *,
                 engine=None, want_values: bool = False) -> PathTargets:
    """Functionals of whole sample paths of forecast mixtures on the original scale: totals over a
    window, peak value and date, exceedance, change between two dates (include/ngp.h "trajectory
    targets").

    ``mixes_or_arrays``: one ``MixtureMVN`` or a sequence of them on the same dates (their paths
    are pooled; mixture j is keyed by ``seed[j]``, taken from its own stream when ``seed`` is None,
    as ``rand_lockstep`` takes it), or arrays ``(w [S,P], mu [P,S,m], sigma [P,m,m])`` with one
    seed — S mixtures over shared components, the layout of ``ngp_mixture_sample`` — or
    ``(w [S,P], mu [S,P,m], sigma [S,P,m,m])`` with S seeds.  The paths are those the sampler draws
    for the same arguments.  ``targets``: ``(kind, j0, j1[, thr])``, kind one of "sum", "max",
    "diff", "argmax", "exceed", window inclusive.

    ``inv_transformation`` None (identity) or a callable that carries ``ngp_inv`` (the inverses of
    ``nowcast.get_transformations``) runs wholly on the device when the engine has
    ``mixture_path_targets``; any other callable, or an engine without that entry, takes the host
    path — the engine's sampler (numpy without one), then numpy with the same definitions."""
    w, mu, sigma, seed = _mixture_arrays(mixes_or_arrays, seed, "path_targets")
    m, N = mu.shape[2], w.shape[0] * int(draws)
    tgs = _target_tuples(targets, m)
    probs = np.asarray(probs, dtype=np.float64).reshape(-1)
    if probs.size < 1 or not np.all((probs > 0.0) & (probs < 1.0)):
        raise ValueError("path_targets: levels in (0, 1)")
    inv = (0, 0.0, 0.0, 0.0) if inv_transformation is None else getattr(inv_transformation, "ngp_inv", None)
    device = getattr(engine, "mixture_path_targets", None) if engine is not None else None
    if device is not None and inv is not None:
        o = device(w, mu, sigma, int(draws), seed, inv, tgs, probs, want_values)
        _raise_if_failed(o["info"])
        return PathTargets(tgs, probs, o["q"], o["mean"], o["count"], o["hist"], N, o["values"], True)
    x = _host_paths(engine, w, mu, sigma, int(draws), seed, inv_transformation)
    values = path_functionals(x, tgs)
    q, mean, count, hist = summarize_path_values(values, tgs, probs, m)
    return PathTargets(tgs, probs, q, mean, count, hist, N, values if want_values else None, False)


# ---------------------------------------------------------------------------------------------
# scores of the paths themselves: energy score and sample CRPS (include/ngp.h "scores of the
# paths themselves"; the reference's crps / score_forecast, docs/vignettes/getting-started.jl:689-718)
# ---------------------------------------------------------------------------------------------
SCORE_SCALES = {"natural": 0, "log": 1}
NGP_INFO_NOT_FINITE = -3
_SCORE_CHUNK = 1 << 22          # numbers the numpy fallback holds per block of pairs


def _score_scale(scale) -> int:
    code = SCORE_SCALES[scale] if isinstance(scale, str) and scale in SCORE_SCALES else scale
    if isinstance(code, str) or int(code) not in SCORE_SCALES.values():
        raise ValueError(f"scale {scale!r}: one of {sorted(SCORE_SCALES)}")
    return int(code)


def _score_windows(windows, m: int):
    """None -> every single date, then the whole horizon; else [(j0, j1), ...] inclusive"""
    if windows is None:
        return [(j, j) for j in range(m)] + [(0, m - 1)], list(range(m)), [m]
    win = [(int(a), int(b)) for a, b in windows]
    if not win or any(not 0 <= a <= b < m for a, b in win):
        raise ValueError(f"windows: at least one (j0, j1) with 0 <= j0 <= j1 < {m}")
    single = [i for i, (a, b) in enumerate(win) if a == b]
    return win, single, [i for i in range(len(win)) if i not in set(single)]


def host_ensemble_scores(x, y, windows, scale: int = 0, shift: float = 0.0, fair: bool = True):
    """numpy fallback of ``ngp_ensemble_scores`` with the same definitions: x [N, m] paths, y [m],
    windows [(j0, j1)].  The pairs are worked in blocks of rows, the squared distance from
    differences date by date, so that it never holds N^2 numbers at once."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N = x.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.log(x + shift) if scale == 1 else x
        v = np.log(y + shift) if scale == 1 else y
    W = len(windows)
    es, to, tp = np.full(W, np.nan), np.full(W, np.nan), np.full(W, np.nan)
    info = np.zeros(W, dtype=np.int32)
    D = 0.5 * N * (N - 1) if fair else 0.5 * N * N
    rows = max(1, _SCORE_CHUNK // N)
    idx = np.arange(N)
    for wi, (j0, j1) in enumerate(windows):
        uw = u[:, j0:j1 + 1]
        if not np.all(np.isfinite(uw)):
            info[wi] = NGP_INFO_NOT_FINITE
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            to[wi] = np.sqrt(((uw - v[j0:j1 + 1]) ** 2).sum(axis=1)).sum() / N
        total = 0.0
        for a in range(0, N, rows):
            blk = uw[a:a + rows]
            d2 = np.zeros((blk.shape[0], N))
            for j in range(uw.shape[1]):
                df = blk[:, j][:, None] - uw[:, j][None, :]
                with np.errstate(over="ignore", invalid="ignore"):
                    d2 += df * df
            total += np.sqrt(d2)[idx[None, :] > idx[a:a + rows][:, None]].sum()      # i < k only
        if not (np.isfinite(to[wi]) and np.isfinite(total)):      # finite values, squares that overflow
            to[wi], info[wi] = np.nan, NGP_INFO_NOT_FINITE
            continue
        tp[wi] = total / D
        es[wi] = to[wi] - 0.5 * tp[wi]
    return dict(es=es, term_obs=to, term_pair=tp, info=info)


class EnsembleScores:
    """Scores of an ensemble of paths per window of dates (``ensemble_scores``):

        crps     the one-date windows' scores, in window order: the sample CRPS per date
        energy   the scores of the windows of more than one date (by default one: the horizon)
        terms    dict(term_obs = mean |X - y|, term_pair = mean |X - X'|), per window
        es, info, windows   every window's score and status (NGP_INFO_NOT_FINITE: NaN)
    """

    def __init__(self, windows, out, single, longer, device=False):
        self.windows = list(windows)
        self.es, self.info = out["es"], out["info"]
        self.terms = dict(term_obs=out["term_obs"], term_pair=out["term_pair"])
        self.crps, self.energy = self.es[single], self.es[longer]
        self.device = bool(device)


def ensemble_scores(x, y, windows=None, scale="natural", shift=0.0, fair=True, engine=None) -> EnsembleScores:
    """Energy score ES = E|X - y| - 1/2 E|X - X'| of the draws x [dates, draws] (as ``forecast``
    returns them) against y [dates], per window of dates; a one-date window is the sample CRPS the
    reference's vignette computes.  ``windows`` None: every single date plus the whole horizon.
    ``scale`` "natural" or "log" (of x + shift); ``fair`` True: pairs i < j over N (N - 1) / 2 (the
    vignette's estimator), False: over N^2 / 2 (scoringutils).  An engine with ``ensemble_scores``
    does the all-pairs work on the device; without one numpy does, in blocks of pairs."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if x.ndim != 2 or x.shape[0] != y.size or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("ensemble_scores: x [dates, draws], y [dates]")
    code = _score_scale(scale)
    if not (np.isfinite(shift) and shift >= 0.0):
        raise ValueError("ensemble_scores: shift finite and >= 0")
    if fair and x.shape[1] < 2:
        raise ValueError("ensemble_scores: fair=True needs two draws")
    if not np.all(np.isfinite(y)) or (code == 1 and not np.all(y + shift > 0.0)):
        raise ValueError("ensemble_scores: y finite, and y + shift > 0 on the log scale")
    win, single, longer = _score_windows(windows, x.shape[0])
    paths = np.ascontiguousarray(x.T)
    device = getattr(engine, "ensemble_scores", None) if engine is not None else None
    if device is not None:
        return EnsembleScores(win, device(paths, y, win, code, float(shift), bool(fair)), single, longer, True)
    return EnsembleScores(win, host_ensemble_scores(paths, y, win, code, float(shift), bool(fair)),
                          single, longer, False)


def path_scores(mixes_or_arrays, y, draws: int, seed=None, inv_transformation=None, *, windows=None,
                scale="natural", shift=0.0, fair=True, engine=None) -> EnsembleScores:
    """``ensemble_scores`` of the paths the sampler draws from forecast mixtures (the arguments of
    ``path_targets``), mapped through ``inv_transformation``.  With an engine that has
    ``mixture_path_scores`` and an inverse that carries ``ngp_inv`` the paths are drawn, mapped and
    scored on the device and never come back; otherwise the host path of ``path_targets`` draws
    them and ``ensemble_scores`` scores them."""
    w, mu, sigma, seed = _mixture_arrays(mixes_or_arrays, seed, "path_scores")
    m = mu.shape[2]
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    inv = (0, 0.0, 0.0, 0.0) if inv_transformation is None else getattr(inv_transformation, "ngp_inv", None)
    device = getattr(engine, "mixture_path_scores", None) if engine is not None else None
    if device is None or inv is None:
        x = _host_paths(engine, w, mu, sigma, int(draws), seed, inv_transformation)
        return ensemble_scores(x.T, y, windows, scale, shift, fair, engine)
    if y.size != m:
        raise ValueError("path_scores: y [dates]")
    win, single, longer = _score_windows(windows, m)
    o = device(w, mu, sigma, int(draws), seed, inv, y, win, _score_scale(scale), float(shift), bool(fair))
    _raise_if_failed(o["chol_info"])
    return EnsembleScores(win, o, single, longer, True)

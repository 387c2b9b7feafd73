"""The two call sites of the hot path, mirrored: ``make_and_fit_model`` (reference
src/make_and_fit_model.jl:78-93) and ``forecast`` / ``forecast_with_nowcasts`` (reference
src/forecasting.jl:29-167), plus the small containers their signatures need (``TData``,
``create_transformed_data``, ``create_nowcast_data``: reference src/TData.jl:46-74,
src/create_nowcast_data.jl:27-76).  Same names, argument meaning and error behaviour, so the
reference's shape / assertion tests read the same against this module (tests/test_mirror_*.py).

What is different by design: ``forecast_with_nowcasts`` does not fan scenarios out as tasks
(reference src/forecasting.jl:131-132: one ``Threads.@spawn`` per scenario).  On the default path
(``n_mcmc = n_hmc = 0``, ``forecast_n_hmc = None``) all scenarios share the appended dates and K
does not depend on y, so ONE batched call (``ngp_nowcast_batch``) factorises every particle once
and returns every scenario's weight update and predictive mean.  With refinement requested
(``mcmc_structure!`` / ``mcmc_parameters!`` after the nowcast, or HMC before every draw) the D
scenario clones advance in LOCKSTEP: every proposal / leapfrog / prediction is one engine call of
P x D items with per-item y rows — the device sees the reference's whole task fan-out as one batch
instead of D small ones.  Every clone keeps its own random streams, so the result is that of the
reference's per-scenario loop (``lockstep=False``) for the same seed — exactly on an engine whose
arithmetic does not depend on the batch (the oracle engine of the tests; the HIP engine with
``ngp_set_batch_invariant``), to rounding otherwise: by default the library picks launch shapes,
and for gradients the path, by the size of a batch, so an HMC accept decision that sits within
1e-11 of its threshold can fall the other way (include/ngp.h ``ngp_set_batch_invariant``).
``lockstep=False, threads=T`` runs the reference's own form — one task per scenario on T threads,
each making the P-item calls of its clone — and the library combines the concurrent calls
(include/ngp.h "concurrent callers").
"""
from __future__ import annotations

import copy
import warnings
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import _abi, autogp, gp
from .autogp import GPModel

GPConfig = gp.GPConfig

__all__ = ["TData", "GPModel", "GPConfig", "create_transformed_data", "make_and_fit_model",
           "forecast", "forecast_with_nowcasts", "create_nowcast_data", "forecast_mixture",
           "forecast_mixture_with_nowcasts", "get_transformations", "forecast_targets",
           "forecast_targets_with_nowcasts", "score_forecast", "forecast_scores_with_nowcasts",
           "hindcast"]


class TData:
    """(ds, y, values): dates, transformed targets, original values (reference src/TData.jl)."""

    def __init__(self, ds, values, *, transformation: Callable):
        ds, values = list(ds), list(values)
        assert len(ds) == len(values), "length of `ds` should match length of `values`"
        vals = np.asarray(values)
        y = np.asarray([transformation(v) for v in vals.tolist()])
        dtype = np.result_type(y.dtype, vals.dtype)
        self.ds = ds
        self.y = y.astype(dtype)
        self.values = vals.astype(dtype)


def create_transformed_data(ds, values, *, transformation: Callable) -> TData:
    return TData(list(ds), list(values), transformation=transformation)


def create_nowcast_data(nowcasts, dates, *, transformation: Callable = lambda y: y) -> List[TData]:
    """vector-of-vectors, or a matrix whose COLUMNS are scenarios (reference
    src/create_nowcast_data.jl:71-76)."""
    if isinstance(nowcasts, np.ndarray) and nowcasts.ndim == 2:
        nowcasts = [nowcasts[:, j] for j in range(nowcasts.shape[1])]
    nowcasts = list(nowcasts)
    dates = list(dates)
    assert all(len(v) == len(dates) for v in nowcasts), \
        "Length of each nowcast must match length of dates"
    assert len(nowcasts) > 0, "nowcasts must not be empty"
    first = len(nowcasts[0])
    assert all(len(v) == first for v in nowcasts), \
        "All vectors in nowcasts must have the same length"
    return [create_transformed_data(dates, v, transformation=transformation) for v in nowcasts]


def _get_offset(values: np.ndarray) -> float:
    """Half the smallest positive value when the data touch zero, else 0 (reference
    src/transformations.jl:51-61)."""
    assert values.size > 0, "Values array must not be empty"
    assert np.all(values >= 0), "All values must be non-negative for the selected transformations"
    return float(values[values > 0].min() / 2) if values.min() == 0 else 0.0


def _boxcox(x, lam: float):
    x = np.asarray(x, dtype=np.float64)
    return np.log(x) if lam == 0.0 else np.expm1(lam * np.log(x)) / lam


def _fit_boxcox_lambda(x: np.ndarray, lo: float = -20.0, hi: float = 20.0) -> float:
    """Maximum of the Box-Cox profile log-likelihood -(n/2) log var(bc_l(x)) + (l - 1) sum log x
    over l in [lo, hi]: a grid to find the basin, then golden-section search inside it."""
    logx = np.log(x)
    n, slog = x.size, float(np.log(x).sum())

    def nll(lam):
        with np.errstate(all="ignore"):
            z = logx if abs(lam) < 1e-12 else np.expm1(lam * logx) / lam
            v = float(np.var(z))
        if not np.isfinite(v) or v <= 0.0:
            return np.inf
        return 0.5 * n * np.log(v) - (lam - 1.0) * slog

    grid = np.linspace(lo, hi, 161)
    vals = np.array([nll(l) for l in grid])
    k = int(np.argmin(vals))
    a, b = grid[max(k - 1, 0)], grid[min(k + 1, grid.size - 1)]
    g = (np.sqrt(5.0) - 1.0) / 2.0
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = nll(c), nll(d)
    for _ in range(80):
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = nll(c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = nll(d)
    return float(0.5 * (a + b))


def _inv_boxcox(lam: float, offset: float, max_value: float) -> Callable:
    """Inverse Box-Cox that never returns a negative or non-finite value (the edge cases of
    reference src/transformations.jl:6-44): the base l y + 1 is floored at 1e-10 for l > 0; for
    l < 0 a base <= 0 is mass at zero and a tiny positive base is clamped at 1000 x the largest
    observed value."""
    big = 1000.0 * max_value

    def inv(y):
        ya = np.asarray(y, dtype=np.float64)
        base = lam * ya + 1.0
        with np.errstate(all="ignore"):
            if lam > 0:
                res = np.maximum(base, 1.0e-10) ** (1.0 / lam) - offset
            elif lam < 0:
                safe = np.where(base > 0, base, 1.0)
                powd = safe ** (1.0 / lam)
                res = np.where(base > 1.0e-10, powd - offset,
                               np.where(base <= 0, 0.0, np.minimum(powd, big) - offset))
            else:
                res = np.exp(ya) - offset
        res = np.maximum(res, 0.0)
        # (l > 0 and a huge argument: the power overflows — the largest finite number stands for it)
        res = np.where(np.isfinite(res), res, np.finfo(np.float64).max)
        return float(res) if np.ndim(y) == 0 else res

    inv.ngp_inv = (_abi.NGP_INV_BOXCOX, float(lam), float(offset), float(big))
    return inv


def _elementwise(fn: Callable, ngp_inv=None) -> Callable:
    """``ngp_inv``: (kind, lam, offset, cap) — how include/ngp.h ``ngp_inv_transform`` states an
    inverse, for the calls that apply it on the device (``autogp.path_targets``)."""
    def g(y):
        out = fn(np.asarray(y, dtype=np.float64))
        return float(out) if np.ndim(y) == 0 else out
    if ngp_inv is not None:
        g.ngp_inv = ngp_inv
    return g


def get_transformations(transform_name: str, values):
    """``(forward, inverse)`` for ``"percentage"`` (logit of y / 100), ``"positive"`` (log) and
    ``"boxcox"`` (lambda fitted by maximum likelihood), as reference src/transformations.jl:139-174
    defines them.  Data that touch zero are shifted by half their smallest positive value; every
    inverse is monotone non-decreasing (clamp at 0 included) wherever the forward map can land, so
    applied to an exact quantile of the model's scale it gives the quantile of the original scale (a
    Box-Cox inverse with lambda < 0 has a pole at y = -1 / lambda; beyond it the reference's rule,
    kept here, returns 0).  A Box-Cox fit that collapses
    (transformed values not all finite, or their range <= 1e-2 of the range of log) falls back to
    ``"positive"`` with a warning.  Both callables take scalars and numpy arrays."""
    vals = np.asarray(values, dtype=np.float64).ravel()
    offset = _get_offset(vals)
    if transform_name == "percentage":
        def fwd(y):
            pr = (y + offset) / 100.0
            with np.errstate(divide="ignore"):
                return np.log(pr) - np.log1p(-pr)
        return (_elementwise(fwd),
                _elementwise(lambda y: np.maximum(100.0 / (1.0 + np.exp(-y)) - offset, 0.0),
                             (_abi.NGP_INV_LOGISTIC100, 0.0, offset, 0.0)))
    if transform_name == "positive":
        def fwd(y):
            with np.errstate(divide="ignore"):
                return np.log(y + offset)
        return (_elementwise(fwd), _elementwise(lambda y: np.maximum(np.exp(y) - offset, 0.0),
                                                (_abi.NGP_INV_EXP, 0.0, offset, 0.0)))
    if transform_name == "boxcox":
        shifted = vals + offset
        lam = _fit_boxcox_lambda(shifted)
        with np.errstate(all="ignore"):
            transformed = _boxcox(shifted, lam)
        bc_range = float(transformed.max() - transformed.min())
        log_range = float(np.log(shifted).max() - np.log(shifted).min())
        if not np.all(np.isfinite(transformed)) or bc_range <= 1.0e-2 * log_range:
            warnings.warn(f"Box-Cox transformation degenerate (lambda = {lam}, transformed range = "
                          f"{bc_range}); falling back to log transformation (issue #51).")
            return get_transformations("positive", values)
        return (_elementwise(lambda y: _boxcox(y + offset, lam)),
                _inv_boxcox(lam, offset, float(vals.max())))
    raise AssertionError(f"Unknown transform_name: {transform_name}")


def _stabilize_for_fit(y, *, flat_threshold: float = 1.0e-3, rng=None):
    """Jitter a near-constant series so the GP covariance stays positive definite (reference
    src/make_and_fit_model.jl:17-27)."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    if n <= 1:
        return y
    scale = abs(y.sum() / n) + 1
    rel_range = (y.max() - y.min()) / scale
    if rel_range >= flat_threshold:
        return y
    sigma = flat_threshold * scale
    warnings.warn(f"Near-constant series (relative range {rel_range} < {flat_threshold}); adding "
                  f"jitter (sigma = {sigma}) so the GP covariance stays positive-definite (issue #51).")
    rng = rng or np.random.default_rng()
    return y + sigma * rng.standard_normal(n)


_REQUIRED = object()


def make_and_fit_model(data: TData, *, n_particles: int = 1, smc_data_proportion: float = 0.1,
                       flat_threshold: float = 1.0e-3, config: Optional[GPConfig] = None,
                       n_mcmc=_REQUIRED, n_hmc=_REQUIRED, engine=None, seed=None, **kwargs):
    if n_mcmc is _REQUIRED or n_hmc is _REQUIRED:
        # fit_smc! requires both (UndefKeywordError in the reference, test/test_gpconfig.jl:42)
        raise TypeError("make_and_fit_model() missing required keyword arguments n_mcmc and n_hmc "
                        "(forwarded to fit_smc)")
    config = config if config is not None else GPConfig()
    n_train = len(data.y)
    streams = autogp.make_streams(seed)
    # the jitter comes from the stream every rank shares: all ranks must fit the same series
    y_fit = _stabilize_for_fit(data.y, flat_threshold=flat_threshold, rng=streams[1])
    model = GPModel(data.ds, y_fit, n_particles=n_particles, config=config, engine=engine,
                    seed=seed, _streams=streams)
    effective = max(smc_data_proportion, 1.0 / n_train)
    schedule = autogp.Schedule.linear_schedule(n_train, effective)
    autogp.fit_smc(model, schedule=schedule, n_mcmc=n_mcmc, n_hmc=n_hmc, **kwargs)
    return model


def _apply(inv_transformation: Callable, a: np.ndarray) -> np.ndarray:
    """Elementwise ``inv_transformation.(a)`` (reference src/forecasting.jl:48).  Callables that
    already map arrays elementwise (identity, ``np.exp``, Box-Cox inverses) are applied in one go;
    scalar-only ones (``math.exp``, branches on the value) go through ``np.vectorize``."""
    try:
        out = np.asarray(inv_transformation(a), dtype=np.float64)
        if out.shape == a.shape:
            return out
    except Exception:
        pass
    return np.vectorize(inv_transformation, otypes=[np.float64])(a)


def forecast(model: GPModel, forecast_dates, forecast_draws: int, *,
             inv_transformation: Callable = lambda y: y,
             forecast_n_hmc: Optional[int] = None, hmc_config: Optional[dict] = None,
             device_paths: bool = False) -> np.ndarray:
    """Matrix (len(forecast_dates), forecast_draws) of samples (reference src/forecasting.jl:29-75).
    ``hmc_config`` (not in the reference's signature; AutoGP's default applies there): leapfrog
    count and step size of the HMC moves, ``{"n_leapfrog": ..., "eps": ...}``.
    ``device_paths`` (this module's own): a horizon beyond what one aux query carries is drawn on
    the device from the resident factor in one call (``Factor.sample_long``, S = 1 with the model's
    weights; one ``integers`` draw of the shared stream for its seed) instead of bringing every
    particle's covariance to the host.  Where that does not apply — a short horizon,
    ``forecast_n_hmc``, no resident factor with ``sample_long``, a sharded run — the existing path
    runs, as with the default."""
    dates = list(forecast_dates)
    long_x = _long_paths(model, dates, int(forecast_draws)) if device_paths and forecast_n_hmc is None else None
    if long_x is not None:
        draws = long_x
    elif forecast_n_hmc is None:
        draws = autogp.predict_mvn(model, dates).rand(int(forecast_draws))
    else:
        draws = np.empty((len(dates), int(forecast_draws)))
        for i in range(int(forecast_draws)):
            autogp.mcmc_parameters(model, forecast_n_hmc, hmc_config)
            draws[:, i] = autogp.predict_mvn(model, dates).rand()
    return _apply(inv_transformation, draws)


def _long_paths(model: GPModel, dates, draws: int) -> Optional[np.ndarray]:
    """[m, draws] on the model's scale from ONE ``Factor.sample_long`` call (S = 1, no appended
    points, the model's weights), or None where the device path does not apply."""
    t, _ = model._obs()
    t_new = model.ds_transform.apply(autogp.to_days(dates))
    fac = model._factor()
    if (autogp.horizon_blocks(t.size, 0, t_new.size) is None or fac is None
            or not hasattr(fac, "sample_long") or autogp.distributed.world()[1] > 1):
        return None
    w, _ = autogp.distributed.normalize_log_weights(model.log_weights[:, None],
                                                    P_total=model.n_particles_total)
    seed = int(model.rng_shared.integers(0, 2**63 - 1))
    out, _, info, cinfo = fac.sample_long(t_new, np.ascontiguousarray(w.T), draws, seed)
    autogp._raise_if_failed(info)
    autogp._raise_if_failed(cinfo)
    x = (out[0] - model.y_transform.intercept) / model.y_transform.slope
    return np.ascontiguousarray(x.T)


def forecast_lockstep(models: Sequence[GPModel], forecast_dates, forecast_draws: int, *,
                      inv_transformation: Callable = lambda y: y,
                      forecast_n_hmc: Optional[int] = None,
                      hmc_config: Optional[dict] = None) -> List[np.ndarray]:
    """``forecast`` (reference src/forecasting.jl:29-75) of D models on the same dates at once."""
    dates = list(forecast_dates)
    k = int(forecast_draws)
    if forecast_n_hmc is None:
        mixes = autogp.predict_mvn_lockstep(models, dates)
        out = autogp.rand_lockstep(mixes, k, models[0]._eng())
    else:
        out = [np.empty((len(dates), k)) for _ in models]
        obs = None               # the models' data does not change between the draws
        for i in range(k):       # src/forecasting.jl:63-68: HMC on the parameters before every draw
            obs = autogp.mcmc_parameters_lockstep(models, forecast_n_hmc, hmc_config, obs)
            for o, mix in zip(out, autogp.predict_mvn_lockstep(models, dates)):
                o[:, i] = mix.rand()
    return [_apply(inv_transformation, o) for o in out]


def forecast_with_nowcasts(base_model: GPModel, nowcasts: Sequence[TData], forecast_dates,
                           forecast_draws_per_nowcast: int, *,
                           inv_transformation: Callable = lambda y: y, n_mcmc: int = 0,
                           n_hmc: int = 0, ess_threshold: float = 0.0,
                           forecast_n_hmc: Optional[int] = None, verbose: bool = False,
                           lockstep: bool = True, hmc_config: Optional[dict] = None,
                           threads: Optional[int] = None, device_paths: bool = False,
                           refined_device_paths: bool = False) -> np.ndarray:
    """reference src/forecasting.jl:117-167.  Three keywords are this module's own: ``lockstep``
    (False: the reference's per-scenario loop), ``threads`` (with ``lockstep=False``: the loop's
    scenarios as concurrent tasks on that many threads — the reference's ``Threads.@spawn`` per
    scenario, src/forecasting.jl:131-132; the library combines their calls, include/ngp.h
    "concurrent callers") and ``hmc_config`` (leapfrog count / step size of the refinement moves;
    AutoGP's defaults apply in the reference).  Everything up to the draws is the scenario pipeline
    (``_Scenarios``); ``forecast_n_hmc`` and ``threads`` are this function's alone.
    ``device_paths``: a horizon beyond what one aux query carries is drawn on the device in one
    ``Factor.sample_long`` call (``_Scenarios``, "device paths"); on a short horizon, in the
    refinement modes, without a resident factor that has ``sample_long`` or with
    ``lockstep=False`` the existing path runs, as with the default.
    ``refined_device_paths``: the same for the refined ensemble (mode "lockstep" of ``_Scenarios``,
    "refined device paths"): every clone's paths of a long horizon come from
    ``Factor.sample_long_indep`` on factors over whole scenarios; where its conditions do not hold
    the existing path runs."""
    sc = _Scenarios(base_model, nowcasts, forecast_dates, n_mcmc=n_mcmc, n_hmc=n_hmc,
                    ess_threshold=ess_threshold, lockstep=lockstep, hmc_config=hmc_config,
                    forecast_n_hmc=forecast_n_hmc, device_paths=device_paths,
                    refined_device_paths=refined_device_paths)
    dates, draws, D = sc.dates, int(forecast_draws_per_nowcast), len(nowcasts)
    sc.run()
    if sc.mode == "shared":
        if sc.sampler is None:
            return _apply(inv_transformation, sc.host_matrix(draws))
        seed = sc.resample_for_device()
        smp, _, info = sc.sampler(sc.w, sc.means, sc.covs, draws, seed)      # [D, draws, m]
        autogp._raise_if_failed(info)
        return _apply(inv_transformation, np.ascontiguousarray(smp.reshape(D * draws, len(dates)).T))
    if sc.mode == "lockstep":
        paths = sc.refined_paths(draws)
        if paths is not None:
            return np.hstack([_apply(inv_transformation, o) for o in paths])
        results = forecast_lockstep(sc.models, dates, draws, inv_transformation=inv_transformation,
                                    forecast_n_hmc=forecast_n_hmc, hmc_config=hmc_config)
        if verbose:
            print(f"Nowcast scenarios: {len(results)}/{D} (lockstep)")
        return np.hstack(results)

    def task(m, nc):      # the body of the reference's per-scenario task (src/forecasting.jl:133-155)
        sc.refine(m, nc)
        return forecast(m, dates, draws, inv_transformation=inv_transformation,
                        forecast_n_hmc=forecast_n_hmc, hmc_config=hmc_config)

    if threads is not None and int(threads) > 1 and D > 1 and autogp.distributed.world()[1] == 1:
        # Threads.@spawn per scenario (src/forecasting.jl:131-132).  The clones are made in scenario
        # order first (each takes its root from the base model's shared stream), then every task
        # works on its own clone with its own streams: the result does not depend on the schedule
        # beyond the last bits the library's batching decides.  A clone forecasts ONCE, so its
        # predictive call is the one-shot entry point (combinable), not a resident factor.
        import sys
        from concurrent.futures import ThreadPoolExecutor
        models = [sc.clone() for _ in nowcasts]
        for m in models:
            m._one_shot_predict = True
        # a task that comes back from the library needs the interpreter lock to go on; with the
        # default 5 ms switch interval it can wait that long for a task that is between two calls
        old = sys.getswitchinterval()
        sys.setswitchinterval(min(old, 1e-4))
        try:
            with ThreadPoolExecutor(max_workers=int(threads)) as pool:
                results = list(pool.map(task, models, nowcasts))
        finally:
            sys.setswitchinterval(old)
        if verbose:
            print(f"Nowcast scenarios: {len(results)}/{D} ({int(threads)} threads)")
        return np.hstack(results)
    results = []
    for nc in nowcasts:   # one after another
        results.append(task(sc.clone(), nc))
        if verbose:
            print(f"Nowcast scenarios: {len(results)}/{D}")
    return np.hstack(results)


class _Scenarios:
    """The scenario pipeline: what the five ``*_with_nowcasts`` functions do before each consumes
    the scenarios' mixtures in its own way (draw, marginals, components, targets, scores).  The
    steps are written here once, in the order the random streams record them, which
    is why from one snapshot and seed the five describe the same matrix of draws.

    Construction asserts the arguments and chooses the ``mode``; it calls no engine and draws
    nothing, so a function's own refusals come between it and ``run``:

    ``"shared"`` (no refinement, the scenarios share their dates, ``lockstep``): ``run`` makes ONE
    batched query, one factorisation per particle (src/forecasting.jl:133-155 with n_mcmc = n_hmc
    = 0), and leaves the D mixtures before anything is drawn: weights ``w`` [D, P] (not yet
    resampled), ``means`` [P, D, m], ``covs`` [P, m, m] and per-date variances ``var`` [P, m]
    shared by the scenarios of a particle, ``low`` [D] (scenarios whose ESS asks for resampling),
    ``rng`` (the stream the draws come from) and ``sampler`` (the device's; None: the draws are made
    on the host).  Without ``want_sigma`` a horizon served by the long query
    (``Factor.predict_long``) forms no covariance at all and ``covs`` is None.

    Device paths (``device_paths=True``, mode "shared", a horizon beyond what one aux query carries,
    a resident factor with ``sample_long``, a single rank): ``run`` makes the query without dates
    for the weight update alone and asks ``predict_long`` for nothing; ``means``, ``covs`` and
    ``var`` are None, ``sampler`` is None and ``long_sampler`` holds the query.  ``host_matrix``
    then resamples in the device form (``resample_for_device``: the stream is used as on the
    short-horizon device path) and draws every path in ONE ``Factor.sample_long`` call.

    ``"lockstep"`` (refinement, shared dates, ``lockstep``): ``run`` leaves the D refined clones in
    ``models``, the reference's D tasks as ONE ensemble of P x D items (src/forecasting.jl:131-149).

    Refined device paths (``refined_device_paths=True``, mode "lockstep" without
    ``forecast_n_hmc``, a horizon beyond what one aux query carries, a single rank, an engine whose
    resident factor has ``sample_long_indep``): ``refined_paths`` draws every clone's paths with
    ``autogp.sample_long_lockstep`` — factors over whole scenarios, no covariance on the bus, each
    clone keyed from its own stream as the device's independent form is; ``host_matrix`` and
    ``device_input`` take the paths from it.  Otherwise it is None and today's route runs.

    ``"loop"``: the reference's per-scenario loop.  Nothing happens in ``run``; ``mixtures`` clones,
    refines and predicts scenario by scenario as it is consumed, so scenario s takes its root from
    the base model's shared stream only after scenario s - 1 has drawn."""

    def __init__(self, base_model: GPModel, nowcasts: Sequence[TData], forecast_dates, *,
                 n_mcmc: int = 0, n_hmc: int = 0, ess_threshold: float = 0.0, lockstep: bool = True,
                 hmc_config: Optional[dict] = None, forecast_n_hmc: Optional[int] = None,
                 device_paths: bool = False, refined_device_paths: bool = False):
        assert len(nowcasts) > 0, "nowcasts vector must not be empty"
        assert not (n_mcmc > 0 and n_hmc == 0), \
            "If n_mcmc > 0, n_hmc must also be > 0 for MCMC refinement"
        assert 0.0 <= ess_threshold <= 1.0, "ess_threshold must be between 0 and 1"
        assert forecast_n_hmc is None or forecast_n_hmc > 0, "forecast_n_hmc must be > 0 if specified"
        self.base, self.nowcasts, self.dates = base_model, nowcasts, list(forecast_dates)
        self.n_mcmc, self.n_hmc, self.hmc_config = n_mcmc, n_hmc, hmc_config
        self.ess_threshold = ess_threshold
        self.same_dates = all(list(nc.ds) == list(nowcasts[0].ds) for nc in nowcasts)
        if not (lockstep and self.same_dates):
            self.mode = "loop"
        elif n_mcmc == 0 and n_hmc == 0 and forecast_n_hmc is None:
            self.mode = "shared"
        else:
            self.mode = "lockstep"
        self._mixes = None
        self.device_paths, self.long_sampler = bool(device_paths), None
        self.refined_device_paths = bool(refined_device_paths) and forecast_n_hmc is None
        self._refined = None

    def run(self, want_sigma: bool = True) -> None:
        if self.mode == "shared":
            self._weigh(want_sigma)
        elif self.mode == "lockstep":
            self.models = [self.clone() for _ in self.nowcasts]
            autogp.add_data_lockstep(self.models, self.nowcasts[0].ds, [nc.y for nc in self.nowcasts],
                                     base=self.base)
            autogp.maybe_resample_lockstep(self.models,
                                           self.ess_threshold * autogp.num_particles(self.base))
            if self.n_mcmc > 0 and self.n_hmc > 0:
                autogp.mcmc_structure_lockstep(self.models, self.n_mcmc, self.n_hmc, self.hmc_config)
            elif self.n_mcmc == 0 and self.n_hmc > 0:
                autogp.mcmc_parameters_lockstep(self.models, self.n_hmc, self.hmc_config)

    # -- clones (modes "lockstep" and "loop") -------------------------------------------------------
    def clone(self) -> GPModel:
        # GPModel(deepcopy(Dict(base_model))) of the reference (src/forecasting.jl:128,133).  Every
        # scenario is its own task with its own randomness there (:131-133); a clone that kept the
        # snapshot's streams would repeat the first scenario's draws.  Splitting also advances the
        # base model's shared stream, so a second call differs from the first.
        return self.base.clone(root=int(self.base.rng_shared.integers(0, 2**62)))

    def refine(self, m: GPModel, nc: TData) -> None:
        """the body of the reference's per-scenario task up to its forecast (src/forecasting.jl:133-149)"""
        autogp.add_data(m, nc.ds, nc.y)
        autogp.maybe_resample(m, self.ess_threshold * autogp.num_particles(m))
        if self.n_mcmc > 0 and self.n_hmc > 0:
            autogp.mcmc_structure(m, self.n_mcmc, self.n_hmc, self.hmc_config)
        elif self.n_mcmc == 0 and self.n_hmc > 0:
            autogp.mcmc_parameters(m, self.n_hmc, self.hmc_config)

    # -- mode "lockstep": refined device paths ------------------------------------------------------
    def refined_on_device(self) -> bool:
        """What of the refined device route is known before a factor is made: the keyword, the mode,
        a horizon beyond one aux query, a single rank (call it after ``run``)."""
        if not (self.refined_device_paths and self.mode == "lockstep") or autogp.distributed.world()[1] > 1:
            return False
        t, _ = self.models[0]._obs()
        return autogp.horizon_blocks(t.size, 0, len(self.dates)) is not None

    def refined_paths(self, draws: int):
        """The clones' paths, a list of [m, draws] on the models' scale, from
        ``autogp.sample_long_lockstep`` (drawn once) — or None: today's route."""
        if self._refined is None and self.refined_on_device():
            self._refined = autogp.sample_long_lockstep(self.models, self.dates, draws)
        return self._refined

    def mixtures(self):
        """The scenarios' ``MixtureMVN``: a list from one ``predict_mvn_lockstep`` (made once) in
        mode "lockstep", a generator in mode "loop"."""
        if self.mode == "lockstep":
            if self._mixes is None:
                self._mixes = autogp.predict_mvn_lockstep(self.models, self.dates)
            return self._mixes
        return self._loop_mixtures()

    def _loop_mixtures(self):
        for nc in self.nowcasts:
            mdl = self.clone()
            self.refine(mdl, nc)
            yield autogp.predict_mvn(mdl, self.dates)

    # -- mode "shared": the batched query and the weight update -------------------------------------
    def _weigh(self, want_sigma: bool) -> None:
        model, nowcasts, dates = self.base, self.nowcasts, self.dates
        t, y = model._obs()
        t_add = model.ds_transform.apply(autogp.to_days(list(nowcasts[0].ds)))
        y_add = np.stack([model.y_transform.apply(np.asarray(nc.y, dtype=np.float64))
                          for nc in nowcasts])
        t_new = model.ds_transform.apply(autogp.to_days(dates))
        fac = model._factor()

        def call(ts):
            if fac is not None:
                o = fac.nowcast(t_add, y_add, ts, True)
            else:
                o = model._eng().nowcast(model.programs(), t, y, t_add, y_add, ts, True)
            return o["mu"], o["sigma"], o["info"], o

        blocks = autogp.horizon_blocks(t.size, t_add.size, t_new.size)
        if blocks is None:
            out = call(t_new)[3]
        elif (self.device_paths and fac is not None and hasattr(fac, "sample_long")
              and autogp.distributed.world()[1] == 1):
            # device paths: the weight update alone; sample_long forms the moments where it draws
            out = dict(fac.nowcast(t_add, y_add, t_new[:0], True), mu=None, sigma=None, var=None)
            self.long_sampler = (fac, t_new, t_add, y_add)
        elif fac is not None and hasattr(fac, "predict_long"):
            # longer than the aux rows carry: the weight update from a query without dates, then ONE
            # long query with the dates as the panel of a solve against the resident factor
            first = fac.nowcast(t_add, y_add, t_new[:0], True)
            mu_l, var_l, sg_l, info_l = fac.predict_long(t_new, t_add, y_add, True, want_sigma)
            out = dict(first, mu=mu_l, sigma=sg_l, var=var_l,
                       info=np.where(first["info"] != 0, first["info"], info_l))
        else:       # a horizon longer than one call carries: pairwise calls (autogp.predict_in_blocks)
            mu_all, sg_all, info_all, first = autogp.predict_in_blocks(call, t_new, blocks)
            out = dict(first, mu=mu_all, sigma=sg_all, info=info_all)
        autogp._raise_if_failed(out["info"])
        s, b = model.y_transform.slope, model.y_transform.intercept
        D = len(nowcasts)
        m = len(dates)
        P = model.n_particles_total
        self.rng = model.rng_shared     # shared stream: every rank makes the same draws
        # add_data! weight update for every scenario, normalised over ALL ranks' particles: one
        # all-gather of [P_local, D] log-weights (the only collective of the weight update)
        dist_ = autogp.distributed
        logw = model.log_weights[:, None] + (out["logml_full"] - out["logml_base"][:, None])
        _, ess, w_all = dist_.normalize_log_weights(logw, P_total=P, full=True)
        self.w = np.ascontiguousarray(w_all.T)                                    # [D, P]
        if self.long_sampler is not None:
            self.means = self.covs = self.var = self.sampler = None
            self.low = ess < self.ess_threshold * P
            return
        means = (out["mu"] - b) / s if m else np.zeros((logw.shape[0], D, 0))     # [P_local, D, m]
        covs = None
        if not m:
            covs = np.zeros((logw.shape[0], 0, 0))
        elif out["sigma"] is not None:
            covs = out["sigma"] / (s * s)
        var = out["var"] / (s * s) if out.get("var") is not None else np.einsum("pjj->pj", covs)
        if dist_.world()[1] > 1:        # the mixtures need every rank's components: one more
            second = covs if covs is not None else var
            packed = np.concatenate([means.reshape(means.shape[0], -1),
                                     second.reshape(second.shape[0], -1)], axis=1)
            packed = dist_.all_gather_rows(packed, sizes=dist_.block_sizes(P))
            means = np.ascontiguousarray(packed[:, :D * m].reshape(P, D, m))
            if covs is not None:
                covs = np.ascontiguousarray(packed[:, D * m:].reshape(P, m, m))
                var = np.einsum("pjj->pj", covs)
            else:
                var = np.ascontiguousarray(packed[:, D * m:].reshape(P, m))
        self.means, self.covs, self.var = means, covs, var
        self.low = ess < self.ess_threshold * P
        # (the device sampler takes at most NGP_MAX_AUX dates)
        self.sampler = getattr(model._eng(), "mixture_sample", None) if 0 < m <= _abi.NGP_MAX_AUX else None

    # -- mode "shared": maybe_resample! in its two recorded forms ------------------------------------
    def resample_for_device(self) -> int:
        """With a device sampler: ``maybe_resample!`` for ALL low scenarios in one multinomial
        (ancestors ~ w, weights -> ancestor counts / P), then the seed of the ONE device call that
        draws from all D mixtures.  The consumers that draw nothing (marginals, components) take
        the seed all the same: it leaves the stream where the draws would."""
        P = self.w.shape[1]
        if self.low.any():
            self.w[self.low] = self.rng.multinomial(P, self.w[self.low]) / P
        return int(self.rng.integers(0, 2**63 - 1))

    def _resampled(self, s: int) -> np.ndarray:
        """``maybe_resample!`` of scenario s on the host: ancestors ~ w, weights -> counts / P"""
        P = self.w.shape[1]
        return np.bincount(self.rng.choice(P, size=P, p=self.w[s]), minlength=P) / P

    def resample_without_draws(self) -> None:
        """What the consumers that draw nothing do where ``forecast_with_nowcasts`` would draw: the
        device form, or without a sampler the host form over the low scenarios alone (there
        ``forecast_with_nowcasts`` interleaves every scenario's draws, so only the scenarios up to
        the first resampled one have its weights)."""
        if self.sampler is not None or self.long_sampler is not None:
            self.resample_for_device()
        else:
            for s in np.flatnonzero(self.low):
                self.w[s] = self._resampled(s)

    # -- what forecast_with_nowcasts returns, where it is drawn on the host -------------------------
    def host_matrix(self, draws: int) -> np.ndarray:
        """[m, D draws] on the model's scale (column (s, d) at s draws + d).  "shared": scenario by
        scenario, each resampled just before its own draws; "lockstep": ``rand_lockstep``;
        "loop": ``rand`` of each scenario's mixture as it is made."""
        if self.mode == "lockstep":
            paths = self.refined_paths(draws)
            if paths is not None:
                return np.hstack(paths)
            return np.hstack(autogp.rand_lockstep(self.mixtures(), draws, self.base._eng()))
        if self.mode == "loop":
            return np.hstack([mx.rand(draws) for mx in self.mixtures()])
        if self.long_sampler is not None:
            fac, t_new, t_add, y_add = self.long_sampler
            seed = self.resample_for_device()
            out, _, info, cinfo = fac.sample_long(t_new, self.w, draws, seed, t_add, y_add, True)
            autogp._raise_if_failed(info)
            autogp._raise_if_failed(cinfo)
            tr = self.base.y_transform
            return np.ascontiguousarray(((out - tr.intercept) / tr.slope).reshape(-1, t_new.size).T)
        res = np.empty((len(self.dates), len(self.nowcasts) * draws))
        for s in range(len(self.nowcasts)):
            wsc = self._resampled(s) if self.low[s] else self.w[s]
            res[:, s * draws:(s + 1) * draws] = autogp.MixtureMVN(self.means[:, s, :], self.covs, wsc,
                                                                  self.rng).rand(draws)
        return res

    def device_input(self, draws: int):
        """``(mixes_or_arrays, seed)`` for ``autogp.path_targets`` / ``path_scores`` where
        ``forecast_with_nowcasts`` draws in one device call — "shared" with a sampler: the arrays
        and the seed after resampling; "lockstep" clones that take the independent form: their
        mixtures, each keyed from its own stream — else None: ``host_matrix`` has the paths (also on
        the refined device route, whose paths are drawn here)."""
        if self.mode == "lockstep" and self.refined_paths(draws) is not None:
            return None
        if self.mode == "shared" and self.sampler is not None:
            seed = self.resample_for_device()
            return (self.w, self.means, self.covs), seed
        if self.mode == "lockstep" and autogp.takes_independent_form(self.base._eng(), self.mixtures(), draws):
            return self.mixtures(), None
        return None


def forecast_mixture(model: GPModel, forecast_dates) -> "autogp.MixtureMarginals":
    """The per-date marginals of the mixture ``forecast`` draws from (``predict_mvn`` of reference
    src/forecasting.jl:46), as an ``autogp.MixtureMarginals``: exact quantiles, CDF / PIT and CRPS
    instead of draws.  Consumes nothing from the model's random streams."""
    return autogp._predict_marginals(model, list(forecast_dates))


class Hindcast:
    """Forecast skill by report date and horizon of ONE fitted model (``hindcast``).

        origins    [R] observation counts: origin r knows the first ``origins[r]`` observations
        horizons   [H] steps ahead, 1 = the next observation after the origin
        dates      [R][H] the date forecast at (origin, horizon); None past the last observation
        observed   [R, H] what was observed there, on the scale the model was given; NaN past it
        marginals  [R] ``autogp.MixtureMarginals`` of origin r over ``union_dates``
        ess        [R] effective sample size of the weights used at each origin

    ``crps()``, ``pit()`` and ``quantile(levels)`` are [R, H] ([R, H, Q]) tables from the exact
    ``MixtureMarginals`` methods, NaN where there is nothing to score.  With the
    ``inv_transformation`` the hindcast was asked with (an inverse of ``get_transformations``) the
    CRPS is the exact one on the natural scale and the quantiles are mapped back."""

    def __init__(self, origins, horizons, dates, observed, marginals, ess, union_dates, cols,
                 inv_transformation=None):
        self.origins, self.horizons, self.dates, self.observed = origins, horizons, dates, observed
        self.marginals, self.ess, self.union_dates = marginals, ess, union_dates
        self._cols, self.inv_transformation = cols, inv_transformation

    def _table(self, fn, extra=()):
        """fn(marginals over the origin's existing dates, their observations) -> [k, ...]"""
        R, H = self._cols.shape
        out = np.full((R, H) + tuple(extra), np.nan)
        for r, mix in enumerate(self.marginals):
            have = np.flatnonzero(self._cols[r] >= 0)
            if have.size:
                c = self._cols[r, have]
                sub = autogp.MixtureMarginals(mix.means[:, c], mix.variances[:, c], mix.weights,
                                              engine=mix.engine)
                out[r, have] = fn(sub, self.observed[r, have])
        return out

    def crps(self):
        inv = self.inv_transformation
        if inv is None:
            return self._table(lambda mix, y: mix.crps(y))
        return self._table(lambda mix, y: mix.crps(_apply(inv, y), inv_transformation=inv, scale="natural"))

    def pit(self):
        return self._table(lambda mix, y: mix.pit(y))

    def quantile(self, levels):
        lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
        kw = {} if self.inv_transformation is None else {"inv_transformation": self.inv_transformation}
        return self._table(lambda mix, y: mix.quantile(lv, **kw), (lv.size,))


def hindcast_columns(cuts, horizons, n: int):
    """Observation cut + h - 1 (0-based) is what origin ``cut`` forecasts h steps ahead.  Returns
    the sorted union of those below n and ``cols`` [R, H]: where each entry sits in the union, -1
    past the last observation."""
    cuts = np.asarray(cuts, dtype=np.int64).reshape(-1)
    hz = np.asarray(horizons, dtype=np.int64).reshape(-1)
    if hz.size < 1 or np.any(hz < 1):
        raise ValueError("hindcast: horizons are steps ahead, 1 or more")
    obs = cuts[:, None] + hz[None, :] - 1
    union = np.unique(obs[obs < n])
    cols = np.where(obs < n, np.searchsorted(union, np.minimum(obs, n - 1)), -1)
    return union, cols


def hindcast(model: GPModel, report_dates, horizons, *, inv_transformation: Optional[Callable] = None,
             weights: str = "fitted") -> Hindcast:
    """How good have this fitted model's forecasts been?  For every report date (an observation
    count, or a date meaning "the data up to and including") and every horizon h the forecast of
    the h-th observation after it from the data before it alone — the table of the reference's
    "forecast skill by report date" figures (docs/vignettes/setting-priors.jl:166-171) with the
    fitted particles held fixed instead of refitted.  ONE device query on the union of the dates
    (``autogp.predict_origins``), gathered to [report date, horizon]."""
    cuts = autogp.origin_counts(model, report_dates)
    n = model.n_obs
    hz = np.asarray(horizons, dtype=np.int64).reshape(-1)
    union, cols = hindcast_columns(cuts, hz, n)
    if union.size < 1:
        raise ValueError("hindcast: every (report date, horizon) lies past the last observation")
    idx = np.sort(model._perm[:n])
    union_dates = [model.ds[i] for i in idx[union]]
    mixes, ess = autogp.predict_origins(model, [int(c) for c in cuts], union_dates, weights=weights)
    y_union = np.asarray(model.y, dtype=np.float64)[idx[union]]
    observed = np.where(cols >= 0, y_union[np.maximum(cols, 0)], np.nan)
    dates = [[union_dates[c] if c >= 0 else None for c in row] for row in cols]
    return Hindcast(cuts, hz, dates, observed, mixes, ess, union_dates, cols, inv_transformation)


def forecast_mixture_with_nowcasts(base_model: GPModel, nowcasts: Sequence[TData], forecast_dates, *,
                                   n_mcmc: int = 0, n_hmc: int = 0, ess_threshold: float = 0.0,
                                   lockstep: bool = True, hmc_config: Optional[dict] = None,
                                   refined_device_paths: bool = False) -> "autogp.MixtureMarginals":
    """The mixture ``forecast_with_nowcasts`` draws from, pooled over the scenarios (every scenario
    weighs 1 / D, as its equal share of the draws does), as an ``autogp.MixtureMarginals``.

    The scenario pipeline (``_Scenarios``) up to the point where ``forecast_with_nowcasts`` draws,
    so from the same snapshot and seed the draws of that function are samples of exactly the
    mixture returned here.  One exception: on the default path with an engine that has
    no device sampler (or more forecast dates than it takes), ``forecast_with_nowcasts`` resamples
    a scenario AFTER it has drawn for the scenarios before it, so with ``ess_threshold > 0`` only
    the scenarios up to the first resampled one are the same there.  ``forecast_n_hmc`` (a new
    mixture before every draw) has no single mixture and is not taken.
    ``refined_device_paths``: on the conditions of ``forecast_with_nowcasts``' keyword the refined
    clones' marginals come from ``autogp.predict_marginals_lockstep`` (means and variances of the
    long query alone; no covariance is formed anywhere)."""
    sc = _Scenarios(base_model, nowcasts, forecast_dates, n_mcmc=n_mcmc, n_hmc=n_hmc,
                    ess_threshold=ess_threshold, lockstep=lockstep, hmc_config=hmc_config,
                    refined_device_paths=refined_device_paths)
    sc.run(want_sigma=False)
    if sc.refined_on_device():
        parts = autogp.predict_marginals_lockstep(sc.models, sc.dates)
        if parts is not None:
            return autogp.MixtureMarginals.pool(parts)
    if sc.mode != "shared":
        mixes = list(sc.mixtures())
        return autogp.MixtureMarginals.pool([mx.marginals(engine=base_model._eng()) for mx in mixes])
    sc.resample_without_draws()
    D, P = sc.w.shape
    m = len(sc.dates)
    # the scenarios of a particle share its variances: [D P, m], never the D P full matrices
    return autogp.MixtureMarginals(
        np.ascontiguousarray(sc.means.transpose(1, 0, 2)).reshape(D * P, m),
        np.broadcast_to(sc.var[None], (D, P, m)).reshape(D * P, m),
        (sc.w / D).reshape(D * P), engine=base_model._eng())


# the most terms a particle is split into for ``forecast_components_with_nowcasts(one_query=True)``:
# the long query holds C^2 m numbers per particle, not C m rows beside the factor
LONG_COMPONENT_TERMS = 256


def forecast_components_with_nowcasts(base_model: GPModel, nowcasts: Sequence[TData], forecast_dates, *,
                                      split: str = "changepoint", ess_threshold: float = 0.0,
                                      one_query: bool = False,
                                      want_sigma: bool = False) -> "autogp.ComponentForecast":
    """Which part of the nowcast-conditioned forecast is trend, which is season: the additive
    decomposition (``autogp.predict_components``) of the mixture ``forecast_mixture_with_nowcasts``
    returns on its default path.  The parts come from ONE query of the resident factor per block
    of dates (``ngp_factor_components_nowcast``); the weights come from a second one, the default
    path's own ``ngp_factor_nowcast`` query over all the forecast dates (its means and covariances
    are not used): a log evidence moves in its last bits with the number of rows swept beside the
    factor, and only that query gives the weights of ``forecast_mixture_with_nowcasts`` bit for bit.
    So a call costs about two sweeps through the factor.

    Default mode only: the scenarios share their dates and no refinement moves are made (refined
    clones no longer share particles — call ``autogp.predict_components`` per clone for those).
    Single-rank runs only (``NotImplementedError`` in a sharded run, where ``predict_components``
    per rank still works).  Weights and resampling are the scenario pipeline's (``_Scenarios``), as
    on ``forecast_mixture_with_nowcasts``' default path: from the same snapshot and seed the two
    describe one mixture.

    The entries of the returned ``ComponentForecast`` are the pairs (s, p), scenario-major, with
    weight w[s][p] / D; ``sigma`` / ``var`` of (s, p) are the same array objects as particle p's
    (the scenarios of a particle share its covariance).  Original scale of y; ``split`` as
    ``autogp.decompose``.

    ``one_query=True`` (with a factor that has ``components_long``): the parts come from ONE call
    whatever the horizon (``ngp_factor_components_long``), as in ``autogp.predict_components``:
    ``date_blocks`` is None, the forecast carries ``cross``, ``sigma`` is full with ``want_sigma``,
    else None.  The terms of a particle are then capped at ``LONG_COMPONENT_TERMS``, not at the
    rows left beside the factor."""
    sc = _Scenarios(base_model, nowcasts, forecast_dates, ess_threshold=ess_threshold)
    if not sc.same_dates:
        raise ValueError("forecast_components_with_nowcasts: the scenarios must share their dates")
    model = base_model
    fac = model._factor()
    if fac is None or not hasattr(fac, "components_nowcast"):
        raise RuntimeError("forecast_components_with_nowcasts needs the engine's resident factor "
                           "(ngp_factor_components_nowcast)")
    if autogp.distributed.world()[1] > 1:
        raise NotImplementedError("forecast_components_with_nowcasts: single-rank runs only")
    t, _ = model._obs()
    t_add = model.ds_transform.apply(autogp.to_days(list(nowcasts[0].ds)))
    # the appended points take rows beside the factor too: a particle whose terms fit without them
    # but not with them goes to the weaker split
    long_query = one_query and hasattr(fac, "components_long")
    parts = autogp.decompose(model, split, max_terms=LONG_COMPONENT_TERMS if long_query else
                             _abi.NGP_MAX_AUX - t.size % 64 - t_add.size - 2)
    comps = [[gp.to_program(c.tree) + (0.0,) for c in ps] for ps in parts]
    y_add = np.stack([model.y_transform.apply(np.asarray(nc.y, dtype=np.float64)) for nc in nowcasts])
    t_new = model.ds_transform.apply(autogp.to_days(sc.dates))
    D, m, P = len(nowcasts), t_new.size, len(parts)
    # weights, the scenarios to resample and the stream: the pipeline's own query, so the log
    # evidences are the bits of the very query the default path makes (they move in the last place
    # with the number of forecast rows beside the factor)
    sc.run()
    if long_query:
        o = fac.components_long(comps, t_new, t_add, y_add, want_sigma=want_sigma)
        sc.resample_without_draws()
        one = autogp.long_component_forecast(model, parts, o, np.ones(P))
        return autogp.ComponentForecast(
            [np.ascontiguousarray(one.means[p][:, s, :]) for s in range(D) for p in range(P)],
            [one.sigma[p] for _ in range(D) for p in range(P)], [one.var[p] for _ in range(D) for p in range(P)],
            (sc.w / D).reshape(D * P), one.kinds * D, one.labels * D, one.offset, None,
            engine=model._eng(), cross=[one.cross[p] for _ in range(D) for p in range(P)])
    blocks = autogp.component_blocks(t.size, max(len(ps) for ps in parts), m, t_add.size)
    means = [np.empty((len(ps), D, m)) for ps in parts]
    var = [np.empty((len(ps), m)) for ps in parts]
    sigma = [np.zeros((len(ps) * m, len(ps) * m)) for ps in parts]
    for lo, hi in (blocks or [(0, m)]):
        o = fac.components_nowcast(comps, t_add, y_add, t_new[lo:hi])
        autogp._raise_if_failed(o["info"])
        k = hi - lo
        for p in range(P):
            C = len(parts[p])
            means[p][:, :, lo:hi] = o["mu"][p]
            var[p][:, lo:hi] = o["var"][p]
            sigma[p].reshape(C, m, C, m)[:, lo:hi, :, lo:hi] = o["sigma"][p].reshape(C, k, C, k)
    sc.resample_without_draws()
    inv = 1.0 / model.y_transform.slope           # y = (y_model - intercept) / slope
    var = [a * (inv * inv) for a in var]
    sigma = [a * (inv * inv) for a in sigma]
    return autogp.ComponentForecast(
        [np.ascontiguousarray(means[p][:, s, :]) * inv for s in range(D) for p in range(P)],
        [sigma[p] for _ in range(D) for p in range(P)], [var[p] for _ in range(D) for p in range(P)],
        (sc.w / D).reshape(D * P),
        [[c.kind for c in parts[p]] for _ in range(D) for p in range(P)],
        [[c.label for c in parts[p]] for _ in range(D) for p in range(P)],
        -model.y_transform.intercept * inv, blocks, engine=model._eng())


def forecast_targets(model: GPModel, forecast_dates, targets, forecast_draws: int, *,
                     probs=(0.025, 0.25, 0.5, 0.75, 0.975), inv_transformation: Optional[Callable] = None,
                     want_values: bool = False, device_paths: bool = False) -> "autogp.PathTargets":
    """Summaries of functionals of the paths ``forecast`` returns — totals over a window, the peak
    and its date, exceedance, change between two dates (``autogp.path_targets``) — from the same
    snapshot and seed exactly those paths, without bringing them to the host when the engine has
    ``mixture_path_targets`` and the inverse is one of ``get_transformations``'.
    ``device_paths``: as ``forecast``; the paths of a long horizon come back from
    ``Factor.sample_long`` and are summarised by ``autogp.path_functionals`` (where it does not
    apply the existing path runs)."""
    long_x = _long_paths(model, list(forecast_dates), int(forecast_draws)) if device_paths else None
    if long_x is not None:
        x = np.ascontiguousarray(long_x.T)
        return _targets_of_paths(x if inv_transformation is None else _apply(inv_transformation, x),
                                 targets, probs, want_values)
    mix = autogp.predict_mvn(model, list(forecast_dates))
    eng = model._eng()
    if mix.sampler is None or int(forecast_draws) <= 1:    # the draws forecast() makes on the host
        x = mix.rand(int(forecast_draws)).T
        return _targets_of_paths(x if inv_transformation is None else _apply(inv_transformation, np.ascontiguousarray(x)),
                                 targets, probs, want_values)
    return autogp.path_targets(mix, targets, probs, int(forecast_draws), None, inv_transformation,
                               engine=eng, want_values=want_values)


def _targets_of_paths(v, targets, probs, want_values):
    """numpy summaries of paths v [N, m] that were drawn on the host"""
    tgs = autogp._target_tuples(targets, v.shape[1])
    values = autogp.path_functionals(np.ascontiguousarray(v), tgs)
    q, mean, count, hist = autogp.summarize_path_values(values, tgs, probs, v.shape[1])
    return autogp.PathTargets(tgs, probs, q, mean, count, hist, v.shape[0],
                              values if want_values else None, False)


def forecast_targets_with_nowcasts(base_model: GPModel, nowcasts: Sequence[TData], forecast_dates,
                                   targets, forecast_draws_per_nowcast: int, *,
                                   probs=(0.025, 0.25, 0.5, 0.75, 0.975),
                                   inv_transformation: Optional[Callable] = None, n_mcmc: int = 0,
                                   n_hmc: int = 0, ess_threshold: float = 0.0, lockstep: bool = True,
                                   hmc_config: Optional[dict] = None,
                                   want_values: bool = False, device_paths: bool = False,
                                   refined_device_paths: bool = False) -> "autogp.PathTargets":
    """``autogp.path_targets`` of the paths ``forecast_with_nowcasts`` returns.

    The scenario pipeline (``_Scenarios``) with the sampler seed ``forecast_with_nowcasts`` takes,
    so from one snapshot and seed it summarises exactly the matrix that function would return
    (column (s, d) is path s draws + d).  The default mode
    (``n_mcmc = n_hmc = 0``) is one call over the shared components; lockstep-refined clones no
    longer share particles and go through the independent form.  ``forecast_n_hmc`` (a new mixture
    before every draw) is not taken; sharded runs raise ``NotImplementedError``.
    ``device_paths``: as ``forecast_with_nowcasts`` — the paths of a long horizon are drawn in one
    ``Factor.sample_long`` call and summarised by ``autogp.path_functionals``; where the conditions
    do not hold the existing path runs.  ``refined_device_paths``: likewise for the refined
    ensemble (``Factor.sample_long_indep``)."""
    sc = _Scenarios(base_model, nowcasts, forecast_dates, n_mcmc=n_mcmc, n_hmc=n_hmc,
                    ess_threshold=ess_threshold, lockstep=lockstep, hmc_config=hmc_config,
                    device_paths=device_paths, refined_device_paths=refined_device_paths)
    if autogp.distributed.world()[1] > 1:
        raise NotImplementedError("forecast_targets_with_nowcasts: single-rank runs only")
    draws = int(forecast_draws_per_nowcast)
    eng = base_model._eng()
    sc.run()
    on_device = sc.device_input(draws)
    if on_device is not None:
        return autogp.path_targets(on_device[0], targets, probs, draws, on_device[1], inv_transformation,
                                   engine=eng, want_values=want_values)
    x = np.ascontiguousarray(sc.host_matrix(draws).T)
    return _targets_of_paths(x if inv_transformation is None else _apply(inv_transformation, x),
                             targets, probs, want_values)


def score_forecast(forecasts, y, *, horizon: Optional[int] = None, scale="log", shift: float = 0.0,
                   fair: bool = True, engine=None):
    """The vignette's ``score_forecast`` (reference docs/vignettes/getting-started.jl:689-718, with
    ``data_transform = log`` as at :746) on a draws matrix [dates, draws] from any of the five
    approaches, ``forecast_n_hmc`` included: ``(mean CRPS over the first `horizon` dates, energy
    score of those dates' paths)``, both on ``scale`` ("log": of value + shift; "natural").
    ``horizon`` None: every date.  ``fair`` True is the vignette's estimator.  ``engine``: one with
    ``ensemble_scores`` (``model._eng()``) does the all-pairs work on the device, None numpy."""
    x = np.asarray(forecasts, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    h = x.shape[0] if horizon is None else int(horizon)
    assert 1 <= h <= x.shape[0], "Not enough data to score full horizon"
    assert y.size >= h, "Not enough data to score full horizon"
    sc = autogp.ensemble_scores(x[:h], y[:h], None, scale, shift, fair, engine)
    return float(np.mean(sc.crps)), float(sc.energy[0])


def forecast_scores_with_nowcasts(base_model: GPModel, nowcasts: Sequence[TData], forecast_dates, y,
                                  forecast_draws_per_nowcast: int, *, windows=None, scale="log",
                                  shift: float = 0.0, fair: bool = True,
                                  inv_transformation: Optional[Callable] = None, n_mcmc: int = 0,
                                  n_hmc: int = 0, ess_threshold: float = 0.0, lockstep: bool = True,
                                  hmc_config: Optional[dict] = None, device_paths: bool = False,
                                  refined_device_paths: bool = False) -> "autogp.EnsembleScores":
    """``autogp.ensemble_scores`` of the paths ``forecast_with_nowcasts`` returns against ``y``
    [dates] (original scale): the sample CRPS per date and the energy score of the horizon
    (``windows`` None), or of the given windows of dates.

    The scenario pipeline (``_Scenarios``) with the sampler seed ``forecast_with_nowcasts`` takes,
    so from one snapshot and seed it scores exactly the matrix that function would return; where it goes
    through the device the paths are drawn, mapped and scored there and never come back.
    ``forecast_n_hmc`` (a new mixture before every draw) is not taken: score those draws with
    ``score_forecast``.  Sharded runs raise ``NotImplementedError``.
    ``device_paths``: as ``forecast_with_nowcasts`` — the paths of a long horizon are drawn in one
    ``Factor.sample_long`` call and scored by ``autogp.ensemble_scores``; where the conditions do
    not hold the existing path runs.  ``refined_device_paths``: likewise for the refined ensemble
    (``Factor.sample_long_indep``)."""
    sc = _Scenarios(base_model, nowcasts, forecast_dates, n_mcmc=n_mcmc, n_hmc=n_hmc,
                    ess_threshold=ess_threshold, lockstep=lockstep, hmc_config=hmc_config,
                    device_paths=device_paths, refined_device_paths=refined_device_paths)
    if autogp.distributed.world()[1] > 1:
        raise NotImplementedError("forecast_scores_with_nowcasts: single-rank runs only")
    draws = int(forecast_draws_per_nowcast)
    kw = dict(windows=windows, scale=scale, shift=shift, fair=fair, engine=base_model._eng())
    sc.run()
    on_device = sc.device_input(draws)
    if on_device is not None:
        return autogp.path_scores(on_device[0], y, draws, on_device[1], inv_transformation, **kw)
    x = np.ascontiguousarray(sc.host_matrix(draws))     # [dates, N] on the model's scale
    return autogp.ensemble_scores(x if inv_transformation is None else _apply(inv_transformation, x),
                                  y, **kw)

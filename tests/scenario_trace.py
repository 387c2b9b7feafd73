"""What the five ``*_with_nowcasts`` functions of nowcast.py ask of their engine and of the random
streams, as a record of discrete items (tests/test_scenario_trace.py holds it against
tests/golden/scenario_trace_v1.json), and the numbers they return, as hex (``--dump``).

From a fresh copy of ONE fitted snapshot (``mirror_contracts.fitted``: 10 observations, P = 4; D = 3
scenarios of 2 nowcast dates, m = 3 forecast dates, 5 draws) every function is called in every mode
of ``MODES`` on every engine of ``host_engines()``: the oracle (no sampler), the oracle with the
sampler's stand-in, one that also restates the independent sampler, the trajectory targets and the
path scores on the host (so that the device branches are walked), and that one with a resident
factor (the components need it).  A call's entry holds

    calls     the engine's (and a resident factor's) method calls in order, each with the shapes of
              its array arguments, its integers (the sampler's seeds among them) and the lengths of
              its sequences — written down by a wrapper around the engine object
    streams   the next ``integers(0, 2**62)`` of the base model's shared stream and of each of its
              particle streams, then the same of every scenario clone the call made, in the order
              it made them (the clones are seen through the base model's own ``clone``)
    raised    the exception's type name where the call raises, else null

No float goes into the record: it is the same on every machine.  The numbers are compared once per
change, between two trees on one machine:

    python -m tests.scenario_trace --dump A.txt [--package OTHER_TREE] [--hip]

writes every returned array as the hex of its bytes (``--package``: take ``nowcastautogp_amd`` from
another checkout; ``--hip``: the device engine at the shapes of the GPU mirror tests, plus one long
horizon, instead of the three host engines); ``cmp`` of two such files must be silent.
``python -m tests.scenario_trace --record FILE`` writes the record."""
import copy
import json
import sys

if __name__ == "__main__" and "--package" in sys.argv:
    sys.path.insert(0, sys.argv[sys.argv.index("--package") + 1])

import numpy as np

from nowcastautogp_amd import autogp
from nowcastautogp_amd import nowcast as nc
from tests import mirror_contracts as mc

IDENT = lambda v: v  # noqa: E731
TARGETS = [("sum", 0, 2, 30.0), ("max", 0, 2, 14.0), ("diff", 0, 2, 0.0), ("argmax", 0, 2), ("exceed", 0, 2, 13.0)]
PROBS = [0.025, 0.5, 0.975]

# keyword arguments per mode; "dates": one scenario on other dates than the rest
MODES = {
    "default": {},
    "ess_1.0": dict(ess_threshold=1.0),
    "ess_0.5": dict(ess_threshold=0.5),
    "hmc": dict(n_hmc=1),
    "mcmc_hmc": dict(n_mcmc=1, n_hmc=1),
    "hmc_loop": dict(n_hmc=1, lockstep=False),
    "differing_dates": {},
    "invalid_empty": {},
    "invalid_mcmc_without_hmc": dict(n_mcmc=1, n_hmc=0),
    "invalid_ess": dict(ess_threshold=1.5),
}
FUNCTIONS = ["forecast", "mixture", "components", "targets", "scores"]


# ---- the recording wrapper --------------------------------------------------------------------------
def _describe(v):
    if isinstance(v, np.ndarray):
        return list(v.shape)
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return "float"
    if v is None or isinstance(v, str):
        return v
    if isinstance(v, (list, tuple)):
        if v and all(isinstance(e, (int, np.integer)) and not isinstance(e, bool) for e in v):
            return [int(e) for e in v]
        return ["seq", len(v)]
    return type(v).__name__


class Recorder:
    """An engine (or its resident factor) whose method calls are written into ``log``.  What the
    wrapped object does not have, this one does not have either."""

    def __init__(self, inner, log, prefix=""):
        self.__dict__.update(_inner=inner, _log=log, _prefix=prefix)

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr):
            return attr

        def call(*args, **kw):
            self._log.append([self._prefix + name] + [_describe(a) for a in args]
                             + [[k, _describe(v)] for k, v in sorted(kw.items())])
            out = attr(*args, **kw)
            if name == "factor" and out is not None:
                return Recorder(out, self._log, "factor.")
            return out
        return call


# ---- the engines ----------------------------------------------------------------------------------
def host_engines():
    from oracle import oracle_np
    from tests import path_targets_reference as R
    from tests.engine_oracle import OracleEngine
    from tests.test_path_targets_cpu import PhiloxOracle

    class DeviceFormsOracle(PhiloxOracle):
        """PhiloxOracle plus host restatements of the independent sampler, the trajectory targets
        and the path scores, so that the device branches of the dispatch are walked without one."""

        def mixture_sample_indep(self, w, mu, sigma, draws, seeds):
            out = np.stack([oracle_np.mixture_sample(w[s:s + 1], mu[s][:, None, :], sigma[s], draws,
                                                     seeds[s])[0][0] for s in range(len(seeds))])
            return out, None, np.zeros(w.shape, dtype=np.int32)

        def mixture_path_targets(self, w, mu, sigma, draws, seed, inv, targets, probs, want_values=False):
            r = R.restate(w, mu, sigma, draws, seed, inv, targets, probs)
            return dict(q=r["q"], mean=r["mean"], count=r["count"], hist=r["hist"],
                        values=r["values"] if want_values else None,
                        info=np.zeros(w.shape if not np.isscalar(seed) else w.shape[1], dtype=np.int32))

        def mixture_path_scores(self, w, mu, sigma, draws, seed, inv, y, windows, scale=0, shift=0.0,
                                fair=True):
            x = R.inv_numpy(inv)(R.sample_paths(w, mu, sigma, draws, seed))
            o = autogp.host_ensemble_scores(x, y, windows, scale, shift, fair)
            return dict(o, chol_info=np.zeros(w.shape if not np.isscalar(seed) else w.shape[1],
                                              dtype=np.int32))

    from tests import component_nowcast_reference as cnr
    from tests.test_predict_long_cpu import FakeFactor

    class ResidentFactor(FakeFactor):
        """the oracle-backed factor of tests/test_predict_long_cpu.py plus the components query"""

        def components_nowcast(self, comps, t_add, y_add, t_new):
            refs = [cnr.evaluate(p, [c[:2] for c in cs], self.t, self.y, t_add, y_add, t_new)
                    for p, cs in zip(self.programs, comps)]
            m = np.size(t_new)
            return dict(info=np.array([r.info for r in refs], dtype=np.int32),
                        mu=[r.mu.astype(np.float64) for r in refs],
                        sigma=[r.sigma.astype(np.float64) for r in refs],
                        var=[np.diag(r.sigma).astype(np.float64).reshape(-1, m) for r in refs])

    class ResidentOracle(DeviceFormsOracle):
        """DeviceFormsOracle plus a resident factor (which is what the components need)"""

        def __init__(self):
            super().__init__()
            self.oracle, self.calls = OracleEngine(), []

        def factor(self, programs, t, y):
            return ResidentFactor(self, programs, t, y, True)

    return {"oracle": OracleEngine, "philox": PhiloxOracle, "device_forms": DeviceFormsOracle,
            "resident": ResidentOracle}


# ---- one call ---------------------------------------------------------------------------------------
def scenarios(n, mode, D=3):
    """D scenarios of 2 dates after the n observed ones (values near the series' last)"""
    nd = mc.days(n, n + 2)
    if mode == "invalid_empty":
        return []
    out = [nc.TData(nd, [12.0 + 0.5 * k, 13.0 - 0.4 * k], transformation=IDENT) for k in range(D)]
    if mode == "differing_dates":
        out[-1] = nc.TData([nd[0], mc.days(n + 2, n + 3)[0]], list(out[-1].values), transformation=IDENT)
    return out


def call(fn, base, nows, dates, draws, kw):
    y = np.linspace(12.0, 13.0, len(dates))
    if fn == "forecast":
        return nc.forecast_with_nowcasts(base, nows, dates, draws, **kw)
    if fn == "mixture":
        return nc.forecast_mixture_with_nowcasts(base, nows, dates, **kw)
    if fn == "components":
        return nc.forecast_components_with_nowcasts(base, nows, dates, **kw)
    if fn == "targets":
        m = len(dates)
        tg = [(t[0], 0, m - 1) + t[3:] for t in TARGETS]
        return nc.forecast_targets_with_nowcasts(base, nows, dates, tg, draws, probs=PROBS, want_values=True,
                                                 **kw)
    return nc.forecast_scores_with_nowcasts(base, nows, dates, y, draws, scale="natural", **kw)


def _next(rng):
    return int(rng.integers(0, 2**62))


def traced(fn, snapshot, engine, mode, n, dates, draws):
    """-> (entry of the record, what the call returned)"""
    kw = MODES[mode]
    if fn == "components":      # it takes the thresholds alone: the refinement modes are not its own
        if any(k != "ess_threshold" for k in kw):
            return None, None
        kw = dict(kw)
    log, clones = [], []
    base = nc.GPModel.from_dict(copy.deepcopy(snapshot), engine=Recorder(engine, log))
    make_clone = base.clone

    def clone(*a, **k):
        clones.append(make_clone(*a, **k))
        return clones[-1]
    base.clone = clone
    out, raised = None, None
    try:
        out = call(fn, base, scenarios(n, mode), dates, draws, kw)
    except Exception as e:      # noqa: BLE001 — the type is what is recorded
        raised = type(e).__name__
    streams = [[_next(m.rng_shared), [_next(r) for r in m.prng]] for m in [base] + clones]
    return dict(calls=log, streams=streams, raised=raised), out


def host_cases():
    """(label, entry, returned) for every function x mode x host engine"""
    from tests.engine_oracle import OracleEngine
    values = np.array([10.0, 15, 12, 18, 22, 25, 20, 16, 14, 11])
    snapshot = mc.fitted(OracleEngine(), values=values, seed=7, n_particles=4).to_dict()
    n = len(values)
    for ename, make in host_engines().items():
        for mode in MODES:
            for fn in FUNCTIONS:
                entry, out = traced(fn, snapshot, make(), mode, n, mc.days(n + 3, n + 6), 5)
                if entry is not None:
                    yield f"{ename}/{mode}/{fn}", entry, out


def hip_cases():
    """The device engine: n = 40, P = 8, D = 3, m = 6, 50 draws, and a long horizon (n = 20, P = 3,
    m = 300), in the modes default, ess_threshold = 1 and n_hmc = 1."""
    eng = autogp.HipEngine(0)
    for n, P, m, draws in ((40, 8, 6, 50), (20, 3, 300, 4)):
        rng = np.random.default_rng(n)
        values = 12.0 + 4.0 * np.sin(np.arange(n) / 5.0) + rng.random(n)
        snapshot = mc.fitted(eng, values=values, seed=11, n_particles=P).to_dict()
        for mode in ("default", "ess_1.0", "hmc"):
            for fn in FUNCTIONS:
                entry, out = traced(fn, snapshot, eng, mode, n, mc.days(n + 3, n + 3 + m), draws)
                if entry is not None:
                    yield f"hip_n{n}_m{m}/{mode}/{fn}", entry, out


def record():
    return {label: entry for label, entry, _ in host_cases()}


# ---- the numbers ------------------------------------------------------------------------------------
def _leaves(obj, path):
    if isinstance(obj, np.ndarray):
        a = np.ascontiguousarray(obj)
        yield f"{path} {a.dtype.str} {list(a.shape)} {a.tobytes().hex()}"
    elif isinstance(obj, (float, np.floating)):
        yield f"{path} {float(obj).hex()}"
    elif obj is None or isinstance(obj, (bool, int, np.integer, str)):
        yield f"{path} {obj!r}"
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            yield from _leaves(obj[k], f"{path}.{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _leaves(v, f"{path}[{i}]")
    elif hasattr(obj, "__dict__"):
        for k in sorted(vars(obj)):
            if k != "engine" and not callable(vars(obj)[k]):
                yield from _leaves(vars(obj)[k], f"{path}.{k}")
    else:
        yield f"{path} <{type(obj).__name__}>"


def dump(path, cases):
    with open(path, "w") as f:
        for label, entry, out in cases:
            f.write(f"== {label} raised={entry['raised']} streams={json.dumps(entry['streams'])}\n")
            for line in _leaves(out, "out"):
                f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    print("nowcast.py under test:", nc.__file__, file=sys.stderr)
    if "--dump" in sys.argv:
        dump(sys.argv[sys.argv.index("--dump") + 1], hip_cases() if "--hip" in sys.argv else host_cases())
    else:
        rec = record()
        with open(sys.argv[sys.argv.index("--record") + 1], "w") as f:      # one line per call
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(rec[k])}" for k in sorted(rec)) + "\n}\n")

"""The cases of ngp_factor_sample_long shared by tests/test_sample_long_cpu.py (which measures the
yardstick on the CPU) and tests/test_sample_long_gpu.py (which judges the device by it) — TEST
INFRASTRUCTURE ONLY.

Programs, ``series`` and ``query`` restate those of tests/test_predict_long_gpu.py.  The table
crosses every edge once: n = 64 (no tail) and 191 (a 63-point tail); no appended points (S = 1) and
three scenarios of three; m under, at and over one 64-wide block, odd, just past the short
sampler's 192 dates, several blocks; 1, 17 and 70 draws.  The weights leave particle 1 without any
(it is never factorised); where S = 3 and draws = 70 particle 2 is to receive 15 to 17 of the 210
paths (less than one tile of 64) and particle 0 the rest (more than one workgroup's four tiles).

A case's seed is the first one, counting up from its base, for which the long-double reference alone
says that every pick margin exceeds ``sampler_reference.PICK_MARGIN`` and (S = 3, draws = 70) that
particle 2 receives 15 to 17 paths: the picks need the stream and the weights only, no covariance.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import sampler_reference as sr
from tests import value_cases as vc
from tests.engine_oracle import OracleEngine

H = 1.0 / 200
PROGRAMS = [
    (np.array(vc.FILL_SINGLE[1][0], np.int32), np.array(vc.FILL_SINGLE[1][1], float), vc.FILL_SINGLE[1][2]),
    (np.array(vc.FILL_CHAIN[0][0], np.int32), np.array(vc.FILL_CHAIN[0][1], float), vc.FILL_CHAIN[0][2]),
    (np.array([2, 3, 7, 5, 8], np.int32),
     np.array([0.4, 0.1, 0.6, 0.2, 0.8, 0.8, 0.13, 0.7, 0.55, 0.06]), 5e-3),
]
P = 3

# (n, d, D, m, draws)
TABLE = [
    (64, 0, 1, 63, 17), (64, 0, 1, 64, 70), (64, 3, 3, 65, 70), (191, 3, 3, 129, 70),
    (191, 0, 1, 193, 17), (191, 3, 3, 300, 70), (64, 3, 3, 300, 1), (191, 0, 1, 65, 70),
    (64, 0, 1, 129, 1), (191, 3, 3, 63, 17), (64, 3, 3, 193, 70), (191, 0, 1, 64, 1),
]
# The case run once more with noise_on_new = 0.  Without noise on the dates the covariances of
# particles 1 and 2 (Linear + SqExp, the ChangePoint) are not positive definite to working precision
# at m = 65 — the long-double factorisation stops at rows 6 and 34 — and stay so for every m that
# crosses a block, so this case gives all the weight to particle 0, whose sigma factorises (cond
# 1.8e4): every sigma_k with positive weight is then one the reference can judge.
NOISE_FREE = (64, 3, 3, 65, 70)
# r64_long: the worst error of the fp64 oracle against the long-double reference over TABLE,
# measured by tests/test_sample_long_cpu.py (case (64, 3, 3, 300, 1), cond 5.5e4; 126 eps)
R64_LONG = 2.81e-14
FLOOR = 4 * R64_LONG


def series(n):
    t = np.arange(n) * H
    rng = np.random.default_rng(100 + n)
    return t, np.sin(9.0 * t) + 0.3 * t + 0.1 * rng.standard_normal(n)


def query(n, d, D, m):
    t, y = series(n)
    t_add = t[-1] + H * np.arange(1, d + 1)
    rng = np.random.default_rng(7 * n + d)
    y_add = y[-1] + 0.2 * rng.standard_normal((D, d)) if d else np.zeros((1, 0))
    t_new = t[-1] + H * (d + np.arange(1, m + 1))
    return t, y, t_add, y_add, t_new


def weights(S):
    """row s: (1 - a_s, 0, a_s), a_s = 0.066 + 0.01 s (16 of 210 paths is 0.076)"""
    a = 0.066 + 0.01 * np.arange(S)
    return np.ascontiguousarray(np.stack([1.0 - a, np.zeros(S), a], axis=1))


def weights_noise_free(S):
    return np.ascontiguousarray(np.tile([1.0, 0.0, 0.0], (S, 1)))


def picks(w, draws, seed):
    """(comp [S, draws], margin [S, draws]) of the long-double reference: stream and weights alone"""
    S = w.shape[0]
    comp, margin = np.empty((S, draws), np.int32), np.empty((S, draws))
    for s in range(S):
        u0 = sr.REFERENCE.words(seed, s, draws, 0)
        comp[s], margin[s] = sr.REFERENCE.pick(w[s], sr.REFERENCE.uniform(u0[:, 0], u0[:, 1]))
    return comp, margin


@functools.lru_cache(maxsize=None)
def seed_of(case):
    n, d, D, m, draws = case
    w = weights(D)
    seed = 1000 * n + 10 * m + draws
    while True:
        comp, margin = picks(w, draws, seed)
        got = int(np.sum(comp == 2))
        if margin.min() > sr.PICK_MARGIN and (not (D == 3 and draws == 70) or 15 <= got <= 17):
            return seed
        seed += 1


@functools.lru_cache(maxsize=None)
def oracle_moments(case, noise_on_new=True):
    """(mu [P, S, m], sigma [P, m, m]) of the CPU oracle"""
    n, d, D, m, _ = case
    t, y, t_add, y_add, t_new = query(n, d, D, m)
    eng = OracleEngine()
    if d == 0:
        mu, sg, _, info = eng.predict(PROGRAMS, t, y, t_new, noise_on_new)
        mu = mu[:, None, :]
    else:
        o = eng.nowcast(PROGRAMS, t, y, t_add, y_add, t_new, noise_on_new)
        mu, sg, info = o["mu"], o["sigma"], o["info"]
    assert not np.any(info)
    return np.ascontiguousarray(mu), np.ascontiguousarray(sg)

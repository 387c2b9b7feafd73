"""The cases of ngp_factor_sample_long_indep shared by tests/test_sample_long_indep_cpu.py and
tests/test_sample_long_indep_gpu.py — TEST INFRASTRUCTURE ONLY.

A case is (n, S, P', m, draws): S mixtures of P' items each over one series of n dates, every
mixture with observations of its own (per-item y rows, as refined scenario clones have), m forecast
dates behind the data.  The smallest shapes at which the code can still go wrong: n = 70 and 130 (one
or two main blocks plus a tail); (S, P') = (3, 2) and (2, 5); m = 65 (just past a 64-block), 193 (just
past NGP_MAX_AUX) and 200 (even, off a block edge); 1 and 70 draws (70: more than 64 paths on one
item, a second wave).  The trees are those of the grammar zoo (tests/grammar_cases.py), item i the
i-th of POOL — a ChangePoint among the first five.  A mixture of five leaves its item 1 without
weight (never factorised); every mixture gives its item 0 enough that, at 70 draws, more than 64
paths fall on it.

A mixture's seed is the first one, counting up from its base, for which the long-double reference
alone says that every pick margin exceeds ``sampler_reference.PICK_MARGIN`` and (70 draws) that item
0 of the mixture receives more than 64 paths.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

from tests import grammar_cases as gc
from tests import sampler_reference as sr
from tests.engine_oracle import OracleEngine

H = 1.0 / 200
POOL = [gc.PROGRAMS[gc.NAMES.index(k)] for k in
        ("se", "ge_gamma03", "per_third", "lin_outside", "cp_both_general", "gen15", "stat8", "per_eighth",
         "const", "cp8")]
NS, FORMS, MS, DRAWS = (70, 130), ((3, 2), (2, 5)), (65, 193, 200), (1, 70)
TABLE = [(n, S, Pm, m, dr) for n, (S, Pm), m, dr in itertools.product(NS, FORMS, MS, DRAWS)]


def programs(S, Pm):
    return [POOL[i % len(POOL)] for i in range(S * Pm)]


def series(n, S):
    """t [n] and Y [S, n]: mixture s has observations of its own"""
    t = np.arange(n) * H
    rng = np.random.default_rng(300 + n)
    base = np.sin(9.0 * t) + 0.3 * t
    return t, np.stack([base + 0.1 * rng.standard_normal(n) + 0.05 * s for s in range(S)])


def item_y(n, S, Pm):
    t, Y = series(n, S)
    return t, np.repeat(Y, Pm, axis=0)


def dates(n, m):
    return (n - 1) * H + H * np.arange(1, m + 1)


def weights(S, Pm):
    """row s: item 0 most of the weight; P' = 2: the rest on item 1; P' = 5: item 1 none, the rest
    shared among the others, descending"""
    w = np.zeros((S, Pm))
    for s in range(S):
        rest = 0.05 + 0.01 * s
        w[s, 0] = 1.0 - rest
        if Pm == 2:
            w[s, 1] = rest
        else:
            share = np.arange(Pm - 2, 0, -1, dtype=float)
            w[s, 2:] = rest * share / share.sum()
    return w


def case_weights(case):
    return weights(case[1], case[2])


def picks(wrow, draws, seed):
    """(comp [draws], margin [draws]) of the long-double reference for ONE mixture keyed by ``seed``:
    scenario counter 0, the stream and the weights alone"""
    u0 = sr.REFERENCE.words(seed, 0, draws, 0)
    return sr.REFERENCE.pick(wrow, sr.REFERENCE.uniform(u0[:, 0], u0[:, 1]))


@functools.lru_cache(maxsize=None)
def seeds_of(case):
    n, S, Pm, m, draws = case
    w = case_weights(case)
    out = []
    for s in range(S):
        seed = 100000 * n + 1000 * m + 10 * draws + 7919 * s + Pm
        while True:
            comp, margin = picks(w[s], draws, seed)
            if np.min(margin) > sr.PICK_MARGIN and (draws < 70 or int(np.sum(np.asarray(comp) == 0)) > 64):
                break
            seed += 1
        out.append(seed)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_moments(n, S, Pm, m, noise_on_new=True):
    """(mu [S P', m], sigma [S P', m, m]) of the CPU oracle's predict, item by item"""
    t, Y = item_y(n, S, Pm)
    mu, sg, _, info = OracleEngine().predict(programs(S, Pm), t, Y, dates(n, m), noise_on_new)
    assert not np.any(info)
    return np.ascontiguousarray(mu), np.ascontiguousarray(sg)

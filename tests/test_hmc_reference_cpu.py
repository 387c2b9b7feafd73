"""tests/hmc_reference.py against autogp._hmc_move on the CPU (the oracle engine), and the reference's
own clamps: the numpy restatement of ngp_grad_job_hmc's arithmetic must reproduce the host loop bit
for bit before the GPU tests hold the device to it."""
import dataclasses
import math

import numpy as np
import pytest

from nowcastautogp_amd import autogp, gp
from nowcastautogp_amd import nowcast as nc
from tests import hmc_reference as hr
from tests import mirror_contracts as mc
from tests.engine_oracle import OracleEngine

N, P, LEAP, EPS = 30, 8, 4, 0.02


def series(n, seed):
    rng = np.random.default_rng(seed)
    return 50.0 + 0.3 * np.arange(n) + 3.0 * np.sin(np.arange(n) / 3.0) + rng.standard_normal(n)


def make_model(eng, seed, config=None, **kw):
    data = nc.create_transformed_data(mc.days(0, N), series(N, seed), transformation=lambda v: v)
    extra = {} if config is None else {"config": config}
    return nc.make_and_fit_model(data, engine=eng, seed=seed, n_particles=P, n_mcmc=1, n_hmc=1,
                                 **extra, **kw)


def clone(model, eng):
    return autogp.GPModel.from_dict(model.to_dict(), engine=eng)


def state(model):
    return ([gp.to_program(p.tree)[1].copy() for p in model.particles],
            [p.noise for p in model.particles], np.array(model._logml, dtype=float))


def same_state(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]
            and np.array_equal(a[2], b[2]))


def reference_move(model, eng, n_leapfrog, eps, nudge=None):
    """autogp._hmc_move with the trajectory taken from tests/hmc_reference.py: the same draws from
    the same generators, the reference's outputs through the same accept rule."""
    t, y = model._obs()
    prior = model.config.prior
    ops, theta0, codes = [], [], []
    for p in model.particles:
        o, params = gp.to_program(p.tree)
        ops.append(o)
        theta0 += [params, (p.noise,)]
        codes += [gp.KIND_CODES[k] for k in gp.param_kinds(o) + [gp.NOISE_KIND]]
    sizes = np.array([gp.to_program(p.tree)[1].size + 1 for p in model.particles])
    off = np.concatenate([[0], np.cumsum(sizes)])
    codes = np.array(codes)
    z0 = gp.untransform_flat(np.concatenate(theta0), codes, prior)

    def evaluate(th):
        progs = [(ops[i], th[off[i]:off[i + 1] - 1], float(th[off[i + 1] - 1])) for i in range(len(ops))]
        lm, grads, info = eng.logml_grad(progs, t, y)
        return lm, np.concatenate(grads), info

    mom = np.concatenate([model.prng[i].standard_normal(int(sizes[i])) for i in range(len(ops))])
    frozen = None
    if model.config.noise is not None:
        mom[off[1:] - 1] = 0.0
        frozen = np.zeros(codes.size, dtype=bool)
        frozen[off[1:] - 1] = True
    out = hr.trajectory(evaluate, codes, sizes, z0, mom, n_leapfrog, eps, prior, frozen=frozen, sums="seq",
                        nudge=nudge)
    H0, H1 = out["U0"] + out["K0"], out["U1"] + out["K1"]
    acc = 0
    for i, p in enumerate(model.particles):
        u = model.prng[i].random()
        if np.isfinite(H1[i]) and math.log(u) < H0[i] - H1[i]:
            th = out["theta1"][off[i]:off[i + 1]]
            p.tree = gp.from_program(ops[i], th[:-1])
            p.noise = float(th[-1])
            model._logml[i] = float(out["logml1"][i])
            acc += 1
    return acc, out


@pytest.fixture(scope="module")
def eng():
    return OracleEngine()


@pytest.mark.parametrize("fixed_noise", [False, True])
def test_reference_reproduces_the_host_move_bit_for_bit(eng, fixed_noise):
    cfg = nc.GPConfig(noise=0.05) if fixed_noise else None
    base = make_model(eng, 21 if fixed_noise else 20, config=cfg)
    host, ref = clone(base, eng), clone(base, eng)
    t, y = host._obs()
    moved = 0
    for _ in range(3):
        a = autogp._hmc_move([host], t, [y], LEAP, EPS)
        b, _ = reference_move(ref, eng, LEAP, EPS)
        assert a == b
        moved += a
        assert same_state(state(host), state(ref))
    assert moved > 0 and not same_state(state(host), state(base))
    if fixed_noise:
        # (frozen: the noise only goes through log and exp again)
        assert all(abs(p.noise - 0.05) < 1e-14 for p in host.particles)


def test_device_key_falls_back_on_an_engine_without_the_call(eng):
    """the oracle engine stages no job: hmc_config={"device": True} runs today's host loop"""
    assert autogp.DEFAULT_HMC["device"] is False
    base = make_model(eng, 22)
    a, b = clone(base, eng), clone(base, eng)
    autogp.mcmc_parameters(a, 2, {"device": True, "n_leapfrog": LEAP})
    autogp.mcmc_parameters(b, 2, {"device": False, "n_leapfrog": LEAP})
    assert same_state(state(a), state(b)) and not same_state(state(a), state(base))
    # and through the fit and the lockstep moves
    fa = make_model(eng, 23, hmc_config={"device": True})
    fb = make_model(eng, 23, hmc_config={"device": False})
    assert same_state(state(fa), state(fb))
    la, lb = [clone(base, eng), clone(base, eng)], [clone(base, eng), clone(base, eng)]
    autogp.mcmc_structure_lockstep(la, 1, 1, {"device": True, "n_leapfrog": 2})
    autogp.mcmc_structure_lockstep(lb, 1, 1, {"n_leapfrog": 2})
    assert all(same_state(state(x), state(y)) for x, y in zip(la, lb))


# ---- hand-made cases: every clamp of the contract, and proof that the reference can fail ----------
PRIOR = {"gamma": {"mu": 0.3, "sigma": 1.2}, "period": {"mu": -0.5, "sigma": 0.8},
         "wildcard": {"mu": -1.0, "sigma": 1.5}}
CODES = np.array([0, 1, 2, 3, 4, 4, 2, 4])      # two items: 4 parameters + noise, 2 parameters + noise
SIZES = np.array([5, 3])


def quad_eval(calls=None, bad_info_at=None, nan_grad_at=None):
    """logml = -|theta - 1|^2 / 2 per item, an analytic gradient; failures on request"""
    n = [0]

    def evaluate(th):
        k = n[0]
        n[0] += 1
        if calls is not None:
            calls.append(th.copy())
        g = -(th - 1.0)
        lm = np.array([-0.5 * np.sum((th[:5] - 1) ** 2), -0.5 * np.sum((th[5:] - 1) ** 2)])
        info = np.zeros(2, dtype=np.int32)
        if bad_info_at == k:
            info[1] = 3
        if nan_grad_at == k:
            g[2] = np.nan
        return lm, g, info
    return evaluate


def run(z0, clamps=hr.Clamps(), sums="wave", **kw):
    mom = np.linspace(-1.0, 1.0, CODES.size)
    return hr.trajectory(quad_eval(**kw), CODES, SIZES, z0, mom, 3, 0.05, PRIOR, clamps=clamps, sums=sums)


def differs(a, b, keys=("z1", "mom1", "theta1", "U1")):
    return any(not np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def test_a_latent_at_infinity_is_cleaned_for_the_evaluation_only():
    z0 = np.full(CODES.size, 0.1)
    z0[4] = np.inf
    calls = []
    out = run(z0, calls=calls)
    a, b = hr.prior_ab(CODES, PRIOR)
    assert calls[0][4] == min(math.exp(min(a[4] + b[4] * 50.0, 300.0)), 1e6)
    assert np.isinf(out["z_trace"][0][4]) and np.isinf(out["U0"][0]) and np.isfinite(out["U0"][1])
    # (the infinite latent turns NaN after one step — inf - inf — and is evaluated as 0 from then on)
    assert np.isnan(out["z1"][4]) and out["theta_trace"][-1][4] == math.exp(a[4])
    other = run(z0, dataclasses.replace(hr.Clamps(), inf_clean=40.0, theta_clip=1e9))
    assert other["theta_trace"][0][4] != out["theta_trace"][0][4]


def test_gamma_pushed_past_two_and_the_other_margins():
    z0 = np.array([2e6, 60.0, 60.0, 0.2, -40.0, 0.1, -60.0, 400.0])
    calls = []
    out = run(z0, calls=calls)
    th = calls[0]
    assert th[0] == 1e6 and th[1] == 1.0 - 1e-9 and th[2] == 2.0 - 1e-9 and th[6] == 1e-9
    assert th[4] == 1e-12 and th[7] == 1e6
    base = hr.Clamps()
    for field, value in (("gamma_margin", 1e-8), ("unit_margin", 1e-8), ("pos_min", 1e-11),
                         ("theta_clip", 1e5), ("exp_arg", 10.0), ("sig_arg", 10.0)):
        assert differs(out, run(z0, dataclasses.replace(base, **{field: value}))), field


def test_an_item_that_fails_at_one_step_keeps_moving_and_only_the_last_evaluation_decides():
    z0 = np.full(CODES.size, 0.2)
    good, bad = run(z0), run(z0, bad_info_at=2)
    assert np.isfinite(bad["U1"]).all() and bad["info1"].tolist() == [0, 0]
    assert np.array_equal(good["z1"][:5], bad["z1"][:5]) and not np.array_equal(good["z1"][5:], bad["z1"][5:])
    last = run(z0, bad_info_at=3)
    assert np.isinf(last["U1"][1]) and last["info1"][1] == 3 and np.isfinite(last["U1"][0])


def test_a_nan_gradient_entry_fails_its_item_alone():
    z0 = np.full(CODES.size, 0.2)
    good, bad = run(z0), run(z0, nan_grad_at=3)
    assert np.isinf(bad["U1"][0]) and bad["U1"][1] == good["U1"][1]
    assert np.isfinite(bad["mom1"]).all() and np.array_equal(bad["mom1"][5:], good["mom1"][5:])
    assert not np.array_equal(bad["mom1"][:5], good["mom1"][:5])


def test_dtheta_from_theta_is_the_dtheta_that_went_with_it():
    rng = np.random.default_rng(8)
    codes = rng.integers(0, 5, 400)
    a, b = hr.prior_ab(codes, PRIOR)
    z = rng.standard_normal(400) * 2.0
    th, dth = hr.theta_of(z, codes, a, b)
    again, inside = hr.dtheta_of_theta(th, codes, b)
    assert inside.all() and np.array_equal(again, dth)
    z[:5] = 400.0                                  # saturated: flagged, not trusted
    th, _ = hr.theta_of(z, codes, a, b)
    assert not hr.dtheta_of_theta(th, codes, b)[1][:5][codes[:5] > 0].any()


def test_the_wave_order_sum():
    rng = np.random.default_rng(5)
    v = rng.standard_normal(97) ** 2
    lanes = np.zeros(128)
    lanes[:97] = v
    p = lanes[:64] + lanes[64:]
    for d in (32, 16, 8, 4, 2, 1):
        p = np.array([p[i] + p[i ^ d] for i in range(64)])
    assert hr.wave_sum(v) == p[0] == p[63]
    assert abs(hr.wave_sum(v) - hr.seq_sum(v)) <= 64 * np.finfo(float).eps * v.sum()
    z0 = np.full(CODES.size, 0.3)
    a, b = run(z0, sums="wave"), run(z0, sums="seq")
    assert np.array_equal(a["z1"], b["z1"]) and np.allclose(a["U1"], b["U1"], rtol=1e-14)

"""ngp_grad_job_hmc on the device (include/ngp.h) against
tests/hmc_reference.py: the step kernel isolated from the evaluation (recurrence, exact), the end
state against the reference driven by ``job.run`` (bound: 8 x the spread of the reference under
+-1 ulp nudges of every theta, floor 4 ulp), the structural cases, the job's state after a
trajectory, and the mirror's opt-in path."""
import math

import numpy as np
import pytest

from nowcastautogp_amd import _lib, autogp, gp
from nowcastautogp_amd import nowcast as nc
from nowcastautogp_amd._abi import KernelArray
from tests import hmc_reference as hr
from tests import mirror_contracts as mc

pytestmark = pytest.mark.gpu

LEAP, EPS = 4, 0.02
PRIOR = gp.GPConfig().prior
EPS64 = np.finfo(float).eps


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    yield c
    c.close()


class Case:
    """B trees drawn from the grammar prior on n dates, their latents, momenta and observations"""

    def __init__(self, n, B, seed, dates="weekly", mix=False):
        rng = np.random.default_rng(seed)
        if dates == "irregular":
            self.t = np.sort(rng.uniform(0.0, 1.0, n))
        else:
            self.t = np.arange(n) * 7.0 / (7.0 * max(n - 1, 1))
        self.y = np.sin(9.0 * self.t) + 0.5 * self.t + 0.1 * rng.standard_normal(n)
        cfg_s, cfg_c = gp.GPConfig(changepoints=False), gp.GPConfig(changepoints=True)
        self.ops, theta, codes = [], [], []
        while len(self.ops) < B:
            want_cp = mix and len(self.ops) % 2 == 1
            tree = gp.sample_tree(rng, cfg_c if want_cp else cfg_s)
            o, params = gp.to_program(tree)
            has = any(int(x) in (2, 8) for x in o)        # Linear / ChangePoint
            if not autogp._valid_program(tree) or o.size > 15 or (mix and has != want_cp):
                continue
            self.ops.append(o)
            theta += [params, (gp.sample_noise(rng, cfg_s),)]
            codes += [gp.KIND_CODES[k] for k in gp.param_kinds(o) + [gp.NOISE_KIND]]
        self.B = B
        self.codes = np.array(codes)
        self.sizes = np.array([len(gp.param_kinds(o)) + 1 for o in self.ops])
        self.off = np.concatenate([[0], np.cumsum(self.sizes)])
        self.last = self.off[1:] - 1
        self.z0 = gp.untransform_flat(np.concatenate(theta), self.codes, PRIOR)
        self.mom = rng.standard_normal(self.codes.size)
        self.ka = KernelArray([(o, np.zeros(s - 1), 0.0) for o, s in zip(self.ops, self.sizes)])
        self.is_param = np.ones(self.codes.size, dtype=bool)
        self.is_param[self.last] = False

    def stage(self, ctx):
        return ctx.stage_grad(self.ka, self.t, self.y)

    def evaluator(self, job):
        def evaluate(th):
            self.ka.set_params(th[self.is_param], th[self.last])
            return job.run(self.ka)
        return evaluate

    def subset(self, items):
        """the same items as a case of their own"""
        c = object.__new__(Case)
        keep = np.concatenate([np.arange(self.off[i], self.off[i + 1]) for i in items])
        c.t, c.y, c.B = self.t, self.y, len(items)
        c.ops = [self.ops[i] for i in items]
        c.codes, c.z0, c.mom = self.codes[keep], self.z0[keep], self.mom[keep]
        c.sizes = self.sizes[list(items)]
        c.off = np.concatenate([[0], np.cumsum(c.sizes)])
        c.last = c.off[1:] - 1
        c.ka = KernelArray([(o, np.zeros(s - 1), 0.0) for o, s in zip(c.ops, c.sizes)])
        c.is_param = np.ones(c.codes.size, dtype=bool)
        c.is_param[c.last] = False
        return c


def device(job, case, leap=LEAP, eps=EPS, z0=None, mom=None, **kw):
    return job.hmc(case.codes, case.z0 if z0 is None else z0, case.mom if mom is None else mom,
                   leap, eps, PRIOR, **kw)


def reference(job, case, leap=LEAP, eps=EPS, **kw):
    return hr.trajectory(case.evaluator(job), case.codes, case.sizes, kw.pop("z0", case.z0),
                         kw.pop("mom", case.mom), leap, eps, PRIOR, **kw)


KEYS = ("z1", "mom1", "theta1", "U0", "U1", "K0", "K1", "logml1")


def bound_and_diff(job, case, dev, **kw):
    """per output: (8 x the largest spread of 16 nudged reference runs, floor 4 ulp of the output's
    largest magnitude; the device's largest difference from the plain reference)"""
    ref = reference(job, case, **kw)
    rng = np.random.default_rng(99)
    spread = {k: 0.0 for k in KEYS}
    for _ in range(16):
        r = reference(job, case, nudge=hr.ulp_nudger(rng), **kw)
        for k in KEYS:
            spread[k] = max(spread[k], float(np.max(np.abs(r[k] - ref[k]))))
    out = {}
    for k in KEYS:
        floor = 4 * EPS64 * float(np.max(np.abs(ref[k])))
        out[k] = (max(8 * spread[k], floor), float(np.max(np.abs(dev[k] - ref[k]))), spread[k])
    return ref, out


def _profile(ctx, call):
    ctx.profile_enable(True)
    ctx.profile_reset()
    call()
    prof = ctx.profile_get()
    ctx.profile_enable(False)
    return prof


# (seeds: trees drawn from the prior with N(0,1) momenta can diverge within four steps — at n = 208,
# seed 208, one item reaches U1 ~ 1e13 on the CPU oracle and any bound from a spread is meaningless;
# these seeds keep |U1| below 400 there)
ROUTES = [("weekly", 21, 24, 21), ("weekly", 208, 24, 209), ("irregular", 300, 8, 300)]


@pytest.mark.parametrize("dates,n,B,seed", ROUTES)
def test_recurrence_end_state_and_job_state(ctx, dates, n, B, seed):
    case = Case(n, B, seed=seed, dates=dates)
    job, job2 = case.stage(ctx), case.stage(ctx)
    try:
        prof = _profile(ctx, lambda: device(job, case))
        info = job.info()
        assert info["general_items"] == B and info["toeplitz_items"] == 0
        assert info["general_chunk"] == B
        short = "chol_small" in prof
        assert short == (n <= 256), sorted(prof)
        # on a lattice every evaluation launches the tables kernel ahead of the fill (the kernel that
        # can fetch new parameters from the host's copy by itself); off the lattice there is none, so
        # parameters can only be uploaded.  Both are booked as "fill", like the LEAP + 2 step kernels.
        lattice = dates != "irregular"
        assert prof["fill"]["launches"] == (2 if lattice else 1) * (LEAP + 1) + LEAP + 2, prof["fill"]
        case.ka.set_params(np.full(int(case.is_param.sum()), 0.5), np.full(B, 0.1))
        prof2 = _profile(ctx, lambda: job2.run(case.ka))     # new parameters through a plain run
        assert prof2["fill"]["launches"] == (2 if lattice else 1), prof2["fill"]
        dev = device(job, case, trace=True)
        assert np.isfinite(dev["U1"]).all() and not dev["info1"].any()
        # -- job state: the job holds theta1, a run re-evaluates it bit for bit
        lm, g_last, inf = job.run()
        assert np.array_equal(lm, dev["logml1"]) and np.array_equal(inf, dev["info1"])
        # -- recurrence, exact.  Evaluation s is taken from the device itself: a trajectory cut after
        # s leapfrogs leaves the job at evaluation s (same z, bit for bit); its theta1 is the theta
        # the device evaluated, job.run() returns that evaluation's gradient bit for bit, and
        # dtheta/dz follows from theta by the contract's own operations (hr.dtheta_of_theta: exact
        # where no clamp bites — asserted).  (Re-evaluating at numpy's theta(z_s) does not isolate
        # the step kernel: numpy's exp and the device's differ in the last bit of theta, and the
        # evaluation turns that into 1e-12 on g dtheta/dz — seen: 1.9e-16 on a z of 0.16.)  With
        # these, numpy's pm is the device's at every step, so every update is held to 2 ulp of the
        # largest term of THAT step: z' = z + eps pm through the trace, pm' = pm - h dU through the
        # mom1 of the trajectory cut there (its closing half step from the same pm).
        a, b = hr.prior_ab(case.codes, PRIOR)
        ev = case.evaluator(job2)
        zt = dev["z_trace"]
        assert np.array_equal(zt[0], case.z0) and np.array_equal(zt[-1], dev["z1"])
        pm = None
        for s in range(LEAP + 1):
            cut = device(job, case, leap=max(s, 1), eps=EPS if s else 0.0, trace=True)
            assert np.array_equal(cut["z_trace"][s], zt[s])
            lm_s, g_s, info_s = job.run()
            assert not info_s.any()
            dth, inside = hr.dtheta_of_theta(cut["theta1"], case.codes, b)
            assert inside.all()
            dU = -g_s * dth + zt[s]
            prev = case.mom if s == 0 else pm
            if s > 0:     # the cut trajectory closed with half a step from the same pm
                close = prev - 0.5 * EPS * dU
                term = np.maximum.reduce([np.abs(prev), 0.5 * EPS * np.abs(g_s * dth), 0.5 * EPS * np.abs(zt[s])])
                err = np.abs(cut["mom1"] - close) / (EPS64 * term)
                print(f"n={n} step {s}: max |pm' - (pm - h dU)| / ulp(largest term) = {np.max(err):.2f}")
                assert np.all(err <= 2), (s, err.max())
            pm = prev - (0.5 * EPS if s == 0 else EPS) * dU
            if s < LEAP:
                resid = zt[s + 1] - zt[s] - EPS * pm
                big = np.maximum.reduce([np.abs(zt[s + 1]), np.abs(zt[s]), EPS * np.abs(pm)])
                err = np.abs(resid) / (EPS64 * big)
                print(f"n={n} step {s}: max |z' - z - eps pm| / ulp(largest term) = {np.max(err):.2f}")
                assert np.all(err <= 2), (s, err.max())
        assert np.array_equal(cut["mom1"], dev["mom1"])      # the cut at s = LEAP is the trajectory itself
        # -- end state against the reference driven by job.run
        ref, table = bound_and_diff(job2, case, dev)
        for k, (bound, diff, spread) in table.items():
            print(f"n={n} {k}: device-reference {diff:.3e}  spread {spread:.3e}  bound {bound:.3e}")
        for k, (bound, diff, spread) in table.items():
            assert diff <= bound, (k, diff, bound)
        assert np.array_equal(dev["info1"], ref["info1"])
        # -- evaluation 0 = job.run at theta(z0), bit for bit, through U0: eps = 0 leaves z where it
        # is, so theta1 of such a call is the theta(z0) the device evaluated
        still = device(job, case, leap=1, eps=0.0)
        assert np.array_equal(still["z1"], case.z0) and np.array_equal(still["mom1"], case.mom)
        lm0, _, _ = ev(still["theta1"])
        zz = np.array([hr.wave_sum((case.z0 ** 2)[case.off[i]:case.off[i + 1]]) for i in range(B)])
        assert np.array_equal(still["U0"], -lm0 + 0.5 * zz)
        assert np.array_equal(still["U0"], still["U1"]) and np.array_equal(dev["U0"], still["U0"])
        th0, _ = hr.theta_of(case.z0, case.codes, a, b)
        assert np.all(np.abs(still["theta1"] - th0) <= 4 * EPS64 * np.abs(th0))
    finally:
        job.close()
        job2.close()


def test_two_leaves_each_item_ends_where_it_ends_alone(ctx):
    case = Case(320, 12, seed=7, dates="regular", mix=True)
    # batch-invariant arithmetic: a mixed batch of 12 items would otherwise stay whole on the general
    # leaf (ngp_plan.h grad_batch_route splits from 256 items on), and only with it are an item's
    # bits the same whatever batch it travels in — which "ends where it ends alone" needs
    ctx.set_batch_invariant(True)
    try:
        job = case.stage(ctx)
        dev = device(job, case, trace=True)
        out5 = job.info()
        assert out5["general_items"] > 0 and out5["toeplitz_items"] > 0, out5
        lm, _, inf = job.run()
        assert np.array_equal(lm, dev["logml1"]) and np.array_equal(inf, dev["info1"])
        job.close()
        for i in range(case.B):
            one = case.subset([i])
            j1 = one.stage(ctx)
            d1 = device(j1, one, trace=True)
            j1.close()
            sl = slice(case.off[i], case.off[i + 1])
            for k in ("z1", "mom1", "theta1"):
                assert np.array_equal(d1[k], dev[k][sl]), (i, k)
            for k in ("U0", "K0", "U1", "K1", "logml1", "info1"):
                assert d1[k][0] == dev[k][i], (i, k)
            assert np.array_equal(d1["z_trace"], dev["z_trace"][:, sl])
    finally:
        ctx.set_batch_invariant(False)


def test_structural_cases(ctx):
    case = Case(62, 9, seed=3)
    job = case.stage(ctx)
    try:
        base = device(job, case)
        # frozen noise: its latent and its momentum do not move
        frozen = np.zeros(case.codes.size, dtype=np.uint8)
        frozen[case.last] = 1
        mom = case.mom.copy()
        mom[case.last] = 0.0
        fz = device(job, case, mom=mom, frozen=frozen)
        assert np.array_equal(fz["z1"][case.last], case.z0[case.last])
        assert np.array_equal(fz["mom1"][case.last], mom[case.last])
        assert not np.array_equal(fz["z1"][case.is_param], case.z0[case.is_param])
        # an item with a non-finite latent: U1 = +inf, info as a run reports it, the others untouched
        # (a frozen latent at +inf stays there: z'z = inf, U1 = +inf by the contract's own arithmetic.
        # One that moves turns NaN after a step — inf - inf, as on the host — and leaves U1 NaN:
        # not finite either, so the move is rejected all the same; checked below.)
        z0 = case.z0.copy()
        z0[case.last[4]] = np.inf
        fr4 = np.zeros(case.codes.size, dtype=np.uint8)
        fr4[case.last[4]] = 1
        mom4 = case.mom.copy()
        mom4[case.last[4]] = 0.0
        base = device(job, case, mom=mom4, frozen=fr4)
        bad = device(job, case, z0=z0, mom=mom4, frozen=fr4)
        assert np.isinf(bad["U1"][4]) and bad["U1"][4] > 0 and np.isinf(bad["U0"][4])
        assert bad["theta1"][case.last[4]] == 1e6 and np.isinf(bad["z1"][case.last[4]])
        lm, _, inf = job.run()
        assert np.array_equal(inf, bad["info1"])
        others = np.array([i for i in range(case.B) if i != 4])
        keep = np.concatenate([np.arange(case.off[i], case.off[i + 1]) for i in others])
        for k in ("z1", "mom1", "theta1"):
            assert np.array_equal(bad[k][keep], base[k][keep]), k
        for k in ("U0", "K0", "U1", "K1", "logml1", "info1"):
            assert np.array_equal(bad[k][others], base[k][others]), k
        z0 = case.z0.copy()
        z0[case.off[4]] = np.nan
        nan = device(job, case, z0=z0)
        assert not np.isfinite(nan["U1"][4]) and np.isfinite(nan["U1"][others]).all()
        assert np.array_equal(job.run()[2], nan["info1"])
    finally:
        job.close()


def test_a_combined_run_after_a_trajectory_reads_the_refreshed_host_copies(ctx):
    """After ngp_grad_job_hmc the job's one-shot form (h_params, h_k[].noise) holds theta1.  A run
    that finds company is served from THAT form — one launch sequence over all callers' items built
    from their host copies — not from the device programs a lone run evaluates.  Four jobs on the
    same dates run a trajectory each, then run together; with batch-invariant arithmetic a combined
    run gives an item the bits of its own run, so logml1 / info1 must come back bit for bit, and the
    gradient must be the one of a lone run at theta1 on a fresh job."""
    import threading
    T = 4
    cases = [Case(62, 8, seed=40 + i) for i in range(T)]
    ctx.set_batch_invariant(True)
    try:
        jobs = [c.stage(ctx) for c in cases]
        outs = [device(j, c) for j, c in zip(jobs, cases)]
        lone = []
        for c, o in zip(cases, outs):         # a fresh job given theta1 the ordinary way
            j = c.stage(ctx)
            lone.append(c.evaluator(j)(o["theta1"]))
            j.close()
        ctx.set_combining(True)
        ctx.combine_stats(reset=True)
        shared = 0
        for _ in range(3):                    # a later burst finds company announced by the first
            res = [None] * T
            gate = threading.Barrier(T)

            def work(i):
                gate.wait()
                res[i] = jobs[i].run()
            th = [threading.Thread(target=work, args=(i,)) for i in range(T)]
            [x.start() for x in th]
            [x.join() for x in th]
            shared += ctx.combine_stats(reset=True)["shared"]
            for i in range(T):
                assert np.array_equal(res[i][0], outs[i]["logml1"]), i
                assert np.array_equal(res[i][2], outs[i]["info1"]), i
                assert np.array_equal(res[i][0], lone[i][0]) and np.array_equal(res[i][1], lone[i][1]), i
        assert shared >= T, shared            # runs were combined: the host copies were what ran
        for j in jobs:
            j.close()
    finally:
        ctx.set_batch_invariant(False)


def test_validation(ctx):
    case = Case(21, 3, seed=1)
    job = case.stage(ctx)
    try:
        for kw in (dict(leap=0), dict(eps=float("nan"))):
            with pytest.raises(_lib.NgpError):
                device(job, case, **kw)
        codes = case.codes.copy()
        codes[0] = 5
        with pytest.raises(_lib.NgpError):
            job.hmc(codes, case.z0, case.mom, LEAP, EPS, PRIOR)
        bad_prior = {**PRIOR, "wildcard": {"mu": 0.0, "sigma": 0.0}}
        with pytest.raises(_lib.NgpError):
            job.hmc(case.codes, case.z0, case.mom, LEAP, EPS, bad_prior)
        assert np.isfinite(device(job, case)["U1"]).all()     # the job is still usable
    finally:
        job.close()


# ---- the mirror ------------------------------------------------------------------------------------
MIRROR_SEED = 31


def _mirror_model(eng, n=104, particles=24, seed=MIRROR_SEED):
    rng = np.random.default_rng(seed)
    vals = 100.0 + 0.2 * np.arange(n) + 5.0 * np.sin(np.arange(n) / 4.0) + rng.standard_normal(n)
    dates = [mc.D0 + mc.dt.timedelta(days=7 * i) for i in range(n)]
    data = nc.create_transformed_data(dates, vals, transformation=lambda v: v)
    return nc.make_and_fit_model(data, engine=eng, seed=seed, n_particles=particles, n_mcmc=1, n_hmc=1)


def test_mirror_move_device_against_host(ctx, monkeypatch):
    from tests.engine_oracle import OracleEngine
    eng = autogp.HipEngine(0)
    try:
        base = _mirror_model(eng)
        def clone():
            return autogp.GPModel.from_dict(base.to_dict(), engine=eng)

        # the margins of the host run's accept decisions, on the CPU with the oracle engine
        orc = autogp.GPModel.from_dict(base.to_dict(), engine=OracleEngine())
        margins = _accept_margins(orc)
        assert np.all(np.abs(margins[np.isfinite(margins)]) >= 1e-6), margins
        host, dev = clone(), clone()
        t, y = host._obs()
        calls = []
        orig = _lib.GradJob.hmc

        def spy(self, *a, **k):
            out = orig(self, *a, **k)
            calls.append(out)
            return out
        monkeypatch.setattr(_lib.GradJob, "hmc", spy)
        a = autogp._hmc_move([host], t, [y], 10, 0.02)
        assert not calls
        b = autogp._hmc_move([dev], t, [y], 10, 0.02, device=True)
        assert len(calls) == 1
        acc_h = [not np.array_equal(gp.to_program(p.tree)[1], gp.to_program(q.tree)[1])
                 for p, q in zip(host.particles, base.particles)]
        acc_d = [not np.array_equal(gp.to_program(p.tree)[1], gp.to_program(q.tree)[1])
                 for p, q in zip(dev.particles, base.particles)]
        assert a == b and acc_h == acc_d and a > 0
        assert np.allclose(np.array(host._logml, float), np.array(dev._logml, float), rtol=1e-9)
        # H0 - H1, device against host.  The host's is the reference move with the host loop's sums
        # on the same engine (bit for bit the host move: tests/test_hmc_reference_cpu.py, and the
        # accepted sets above agree with it); the bound is the one of the end-state test — 8 x the
        # largest spread of 16 such moves with every theta of every evaluation moved by +-1 ulp,
        # floor 4 ulp of the largest |H|.
        from tests import test_hmc_reference_cpu as tc
        acc_r, ref = tc.reference_move(clone(), eng, 10, 0.02)
        assert acc_r == a
        dH_host = (ref["U0"] + ref["K0"]) - (ref["U1"] + ref["K1"])
        rng = np.random.default_rng(77)
        spread = 0.0
        for _ in range(16):
            _, r = tc.reference_move(clone(), eng, 10, 0.02, nudge=hr.ulp_nudger(rng))
            spread = max(spread, float(np.max(np.abs((r["U0"] + r["K0"]) - (r["U1"] + r["K1"]) - dH_host))))
        out = calls[0]
        dH_dev = (out["U0"] + out["K0"]) - (out["U1"] + out["K1"])
        Hmax = max(float(np.max(np.abs(ref["U0"] + ref["K0"]))), float(np.max(np.abs(ref["U1"] + ref["K1"]))))
        bound = max(8 * spread, 4 * EPS64 * Hmax)
        diff = float(np.max(np.abs(dH_dev - dH_host)))
        print(f"mirror move: max |dH device - dH host| {diff:.3e}  spread {spread:.3e}  bound {bound:.3e}")
        assert np.isfinite(dH_host).all() and diff <= bound, (diff, bound)
    finally:
        eng.ctx.close()


def _accept_margins(model):
    """log u - (H0 - H1) per particle of one host move (the move's own draws, replayed)"""
    import copy
    t, y = model._obs()
    prng = copy.deepcopy(model.prng)
    sizes = [gp.to_program(p.tree)[1].size + 1 for p in model.particles]
    for r, s in zip(prng, sizes):
        r.standard_normal(int(s))
    logu = np.array([math.log(r.random()) for r in prng])
    from tests import test_hmc_reference_cpu as tc
    ref = autogp.GPModel.from_dict(model.to_dict(), engine=model._eng())
    _, out = tc.reference_move(ref, model._eng(), 10, 0.02)
    dH = (out["U0"] + out["K0"]) - (out["U1"] + out["K1"])
    return logu - dH


def test_small_fit_on_the_device_path(ctx):
    eng = autogp.HipEngine(0)
    try:
        rng = np.random.default_rng(5)
        n = 42
        vals = 20.0 + 0.1 * np.arange(n) + rng.standard_normal(n)
        dates = [mc.D0 + mc.dt.timedelta(days=7 * i) for i in range(n)]
        data = nc.create_transformed_data(dates, vals, transformation=lambda v: v)
        model = nc.make_and_fit_model(data, engine=eng, seed=9, n_particles=8, n_mcmc=2, n_hmc=2,
                                      hmc_config={"device": True})
        assert np.isfinite(model.log_weights).all()
        t, y = model._obs()
        fresh, info = eng.logml(model.programs(), t, y)
        assert not info.any() and np.allclose(model._logml, fresh, rtol=1e-9)
    finally:
        eng.ctx.close()

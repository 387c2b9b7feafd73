"""One-shot device calls that draw their blocks from each other's leavings.

A one-shot call allocates its device blocks from the context's block cache and gives them back when
it ends, so on a context that has served other calls every block a call gets is somebody else's old
one: at least as large as asked, up to twice as large, and full of that call's data.  The sampler, the
three summaries, the mapped CRPS, the trajectory targets, the covariance call, the scores of paths
handed in and of paths drawn on the device, and the long-horizon query of a resident factor (the small
shapes of tests/sanitize/oneshot_calls.h) run on ONE context in one order, again in another order, and
once each on a context of their own.  Each call's three results must be the same bytes, info arrays
included: a block handed out at the wrong size or type, or a read of a block the call did not fully
write, shows as a difference."""
import numpy as np
import pytest

from nowcastautogp_amd import _abi, _lib

pytestmark = pytest.mark.gpu

P, S, M, DRAWS = 3, 2, 5, 8
C, MM, K = 5, 7, 3
N_ENS, N_FAC, D_ADD, M_LONG = 16, 70, 2, 6


def _inputs():
    sig = np.zeros((P, M, M))
    sig_i = np.zeros((S, P, M, M))
    j = np.arange(M)
    for k in range(P):
        sig[k] = (0.04 + 0.01 * k) * np.exp(-0.5 * (j[:, None] - j[None, :]) ** 2)
    for k in range(S * P):
        sig_i[k // P, k % P] = (0.04 + 0.01 * k) * np.exp(-0.25 * (j[:, None] - j[None, :]) ** 2)
    mu = 0.5 + 0.125 * np.arange(P * S * M).reshape(P, S, M) / (P * S * M)
    w = np.array([[0.5, 0.25, 0.25], [0.2, 0.3, 0.5]])
    cw = np.array([0.3, 0.0, 0.2, 0.4, 0.1])
    c, d = np.meshgrid(np.arange(C), np.arange(MM), indexing="ij")
    cmu = 1.0 + 0.25 * c + 0.125 * d
    cvar = 0.04 + 0.01 * ((c + d) % 3)
    cvar[2, 4] = -1.0                              # component 2 (positive weight) is bad on date 4
    return dict(
        w=w, mu=mu, sigma=sig, mu_i=np.ascontiguousarray(mu.transpose(1, 0, 2)), sigma_i=sig_i,
        inv=(_abi.NGP_INV_BOXCOX, -0.3, 0.25, 1.0e4),
        # one target that has quantiles, the first date of the maximum, an exceedance
        targets=[(_abi.NGP_TARGET_SUM, 0, M - 1, 0.0), (_abi.NGP_TARGET_ARGMAX, 1, 3, 0.0),
                 (_abi.NGP_TARGET_EXCEED, 0, 2, 1.5)],
        probs=[0.45, 0.5, 0.9],                    # 16 paths: ranks 8, 8, 15
        cw=cw, cmu=cmu, cvar=cvar, x=1.0 + 0.5 * np.arange(K)[None, :] + 0.125 * np.arange(MM)[:, None],
        cprobs=[0.1, 0.5, 0.9], y=1.5 + 0.125 * np.arange(MM),
        progs=[([3], [0.3, 0.8], 0.05), ([2, 3, 7], [0.5, 0.1, 0.5, 0.2, 0.7], 0.02),
               ([3, 5, 6, 2, 7], [0.4, 0.6, 0.25, 0.2, 0.4, 0.5, 0.1, 0.5], 0.1)],
        t1=[0.0, 0.125, 0.25, 0.5, 0.75], t2=[0.0625, 0.25, 0.875, 1.0],
        # the scores: 16 paths handed in, y [M], a window of one date and one of all dates
        x_ens=0.5 + 0.125 * ((7 * np.arange(N_ENS)[:, None] + 3 * np.arange(M)[None, :]) % 11),
        y_path=0.75 + 0.25 * np.arange(M), windows=[(2, 2), (0, M - 1)],
        # the resident factor of the component entries: 2 particles, 70 points; 2 appended points in 2 scenarios
        fprogs=[([3, 5, 6], [0.3, 0.8, 0.4, 0.25, 0.5], 0.05), ([2, 3, 7], [0.5, 0.1, 0.5, 0.2, 0.7], 0.02)],
        ft=np.arange(N_FAC) / 128.0, fy=((np.arange(N_FAC) * 37) % 11) / 11.0 - 0.5,
        t_add=(N_FAC + np.arange(D_ADD)) / 128.0, y_add=(0.1 * (np.arange(2 * D_ADD) % 3)).reshape(2, D_ADD),
        t_long=(N_FAC + D_ADD + np.arange(M_LONG)) / 128.0)


def _calls(a):
    def targets(ctx, seed, mu, sigma):
        r = ctx.mixture_path_targets(a["w"], mu, sigma, DRAWS, seed, a["inv"], a["targets"], a["probs"],
                                     want_values=True)
        return [r[k] for k in ("q", "mean", "count", "hist", "values", "info")]

    def path_scores(ctx, seed, mu, sigma):
        r = ctx.mixture_path_scores(a["w"], mu, sigma, DRAWS, seed, a["inv"], a["y_path"], a["windows"])
        return [r[k] for k in ("es", "term_obs", "term_pair", "info", "chol_info")]

    def ensemble_scores(ctx, scale, shift, fair):
        r = ctx.ensemble_scores(a["x_ens"], a["y_path"], a["windows"], scale, shift, fair)
        return [r[k] for k in ("es", "term_obs", "term_pair", "info")]

    def predict_long(ctx, appended, want_sigma):
        f = ctx.factor(a["fprogs"], a["ft"], a["fy"])
        try:
            r = f.predict_long(a["t_long"], a["t_add"] if appended else None, a["y_add"] if appended else None,
                               noise_on_new=False, want_sigma=want_sigma)
        finally:
            f.close()
        return [x for x in r if x is not None]
    return {
        "sample": lambda ctx: ctx.mixture_sample(a["w"], a["mu"], a["sigma"], DRAWS, 11),
        "sample_indep": lambda ctx: ctx.mixture_sample_indep(a["w"], a["mu_i"], a["sigma_i"], DRAWS, [7, 9]),
        "cdf": lambda ctx: ctx.mixture_cdf(a["cw"], a["cmu"], a["cvar"], a["x"]),
        "quantiles": lambda ctx: ctx.mixture_quantiles(a["cw"], a["cmu"], a["cvar"], a["cprobs"]),
        "crps": lambda ctx: ctx.mixture_crps(a["cw"], a["cmu"], a["cvar"], a["y"]),
        "crps_mapped natural": lambda ctx: ctx.mixture_crps_mapped(
            a["cw"], a["cmu"], a["cvar"], (_abi.NGP_INV_IDENTITY, 0.0, 0.0, 0.0), _abi.NGP_SCORE_NATURAL, 0.0,
            a["y"]),
        "crps_mapped log": lambda ctx: ctx.mixture_crps_mapped(
            a["cw"], a["cmu"], a["cvar"], (_abi.NGP_INV_BOXCOX, 0.5, 0.25, 1.0e4), _abi.NGP_SCORE_LOG, 0.5, a["y"]),
        "path_targets": lambda ctx: targets(ctx, 11, a["mu"], a["sigma"]),
        "path_targets_indep": lambda ctx: targets(ctx, [7, 9], a["mu_i"], a["sigma_i"]),
        "cov_batch": lambda ctx: [ctx.cov_batch(a["progs"], a["t1"], a["t2"], add_diag=True)],
        "ensemble_scores natural": lambda ctx: ensemble_scores(ctx, _abi.NGP_SCORE_NATURAL, 0.0, False),
        "ensemble_scores log": lambda ctx: ensemble_scores(ctx, _abi.NGP_SCORE_LOG, 0.5, True),
        "path_scores": lambda ctx: path_scores(ctx, 11, a["mu"], a["sigma"]),
        "path_scores_indep": lambda ctx: path_scores(ctx, [7, 9], a["mu_i"], a["sigma_i"]),
        "predict_long d=0 sigma": lambda ctx: predict_long(ctx, False, True),
        "predict_long d=0": lambda ctx: predict_long(ctx, False, False),
        "predict_long d=2 sigma": lambda ctx: predict_long(ctx, True, True),
        "predict_long d=2": lambda ctx: predict_long(ctx, True, False),
    }


def _bytes(result):
    return [np.ascontiguousarray(r).tobytes() for r in result]


def test_oneshot_calls_repeat_bitwise_on_reused_blocks():
    import __graft_entry__ as ge
    ge.build()
    calls = _calls(_inputs())
    names = list(calls)
    # the second order: no call follows the call it followed in the first
    again = names[::-3] + names[-2::-3] + names[-3::-3]
    assert sorted(again) == sorted(names) and again != names
    shared = _lib.Context(0)
    try:
        first = {n: _bytes(calls[n](shared)) for n in names}
        second = {n: _bytes(calls[n](shared)) for n in again}
    finally:
        shared.close()
    for n in names:
        own = _lib.Context(0)
        try:
            fresh = _bytes(calls[n](own))
        finally:
            own.close()
        print(f"{n}: {len(fresh)} arrays, {sum(map(len, fresh))} bytes")
        assert first[n] == fresh, f"{n}: first run on the shared context differs from a fresh context"
        assert second[n] == fresh, f"{n}: second run on the shared context differs from a fresh context"

"""The leapfrog trajectory of ngp_grad_job_hmc restated in numpy (include/ngp.h; DESIGN.md section
4.23), over a callback ``evaluate(theta) -> (logml [B], grad [latents], info [B])``: ``theta`` and
``grad`` are laid out as the C call lays latents out (per item its parameters in program order, then
the noise).  TEST INFRASTRUCTURE: written from the contract, not from the library's code — it shares
nothing with ``autogp._hmc_move`` but the formulas.

``sums``: how the three per-item sums are added up.  "wave" is the device's order (a lane adds
latents l and l + 64, then a butterfly over lane distances 32 .. 1); "seq" is ``np.bincount``'s
(latent after latent), which ``autogp._hmc_move`` uses.
``clamps``: the constants of the contract, so that a test can move one and see the outputs change.
``nudge``: applied to theta just before ``evaluate`` (the +-1 ulp spread of the GPU tests)."""
import dataclasses

import numpy as np


@dataclasses.dataclass
class Clamps:
    inf_clean: float = 50.0       # +-inf in z -> +-inf_clean for the evaluation
    sig_arg: float = 700.0        # argument of the sigmoid
    exp_arg: float = 300.0        # argument of exp
    theta_clip: float = 1e6
    pos_min: float = 1e-12
    gamma_margin: float = 1e-9
    unit_margin: float = 1e-9


def wave_sum(v):
    """Sum of at most 128 values in the order of the device's wave: lanes 0..63 hold v[l] + v[l + 64],
    then v += v[lane ^ d] for d = 32, 16, 8, 4, 2, 1."""
    a = np.zeros(128)
    a[:len(v)] = v
    p = a[:64] + a[64:]
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ d]
    return p[0]


def seq_sum(v):
    return np.bincount(np.zeros(len(v), dtype=np.int64), weights=v, minlength=1)[0]


def prior_ab(codes, prior):
    a, b = np.zeros(codes.size), np.ones(codes.size)
    for code, name in ((2, "gamma"), (3, "period"), (4, "wildcard")):
        a[codes == code], b[codes == code] = prior[name]["mu"], prior[name]["sigma"]
    return a, b


def theta_of(z, codes, a, b, c=Clamps()):
    """theta(z) and d theta / dz as an evaluation sees them."""
    with np.errstate(all="ignore"):
        zc = np.where(np.isnan(z), 0.0, np.where(z == np.inf, c.inf_clean,
                                                 np.where(z == -np.inf, -c.inf_clean, z)))
        th, dth = zc.copy(), np.ones_like(zc)
        m = (codes == 1) | (codes == 2)
        x = np.minimum(np.maximum(a[m] + b[m] * zc[m], -c.sig_arg), c.sig_arg)
        e = np.exp(-np.abs(x))
        sg = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        ssg = np.where(codes[m] == 2, 2.0, 1.0) * sg
        th[m], dth[m] = ssg, ssg * (1 - sg) * b[m]
        m = codes >= 3
        v = np.exp(np.minimum(np.maximum(a[m] + b[m] * zc[m], -c.exp_arg), c.exp_arg))
        th[m], dth[m] = v, v * b[m]
        th = np.minimum(np.maximum(th, -c.theta_clip), c.theta_clip)
        m = codes >= 3
        th[m] = np.maximum(th[m], c.pos_min)
        m = codes == 2
        th[m] = np.minimum(np.maximum(th[m], c.gamma_margin), 2.0 - c.gamma_margin)
        m = codes == 1
        th[m] = np.minimum(np.maximum(th[m], c.unit_margin), 1.0 - c.unit_margin)
    return th, dth


def dtheta_of_theta(theta, codes, b, c=Clamps()):
    """d theta / dz recomputed from a theta that ``theta_of``'s arithmetic produced, by the same
    operations: exact (bit for bit the dtheta that went with it) wherever no clamp of theta bit —
    ``inside`` tells where.  exp kinds: dtheta = v b with v = theta; sigmoid kinds: sg = theta / scale
    (scale 1 or 2: exact), dtheta = (scale sg) (1 - sg) b."""
    theta = np.asarray(theta, float)
    dth = np.ones_like(theta)
    m = codes >= 3
    dth[m] = theta[m] * b[m]
    m = (codes == 1) | (codes == 2)
    scale = np.where(codes[m] == 2, 2.0, 1.0)
    sg = theta[m] / scale
    dth[m] = (scale * sg) * (1 - sg) * b[m]
    inside = np.abs(theta) < c.theta_clip
    inside &= np.where(codes >= 3, theta > c.pos_min, True)
    inside &= np.where(codes == 2, (theta > c.gamma_margin) & (theta < 2.0 - c.gamma_margin), True)
    inside &= np.where(codes == 1, (theta > c.unit_margin) & (theta < 1.0 - c.unit_margin), True)
    return dth, inside


def trajectory(evaluate, codes, sizes, z0, mom, n_leapfrog, eps, prior, frozen=None, sums="wave",
               clamps=Clamps(), nudge=None):
    """Every output of ngp_grad_job_hmc plus ``theta_trace`` (the theta of every evaluation) and
    ``grads`` / ``logmls`` / ``infos`` (what ``evaluate`` returned, per evaluation)."""
    codes = np.asarray(codes)
    sizes = np.asarray(sizes, dtype=np.int64)
    B = sizes.size
    off = np.concatenate([[0], np.cumsum(sizes)])
    seg = np.repeat(np.arange(B), sizes)
    add = wave_sum if sums == "wave" else seq_sum
    a, b = prior_ab(codes, prior)
    fr = np.zeros(codes.size, dtype=bool) if frozen is None else np.asarray(frozen).astype(bool)

    def item_sums(v):
        return np.array([add(v[off[i]:off[i + 1]]) for i in range(B)])

    rec = dict(theta_trace=[], grads=[], logmls=[], infos=[])

    def potential(z):
        th, dth = theta_of(z, codes, a, b, clamps)
        rec["theta_trace"].append(th)
        lm, g, info = evaluate(nudge(th) if nudge is not None else th)
        lm, g, info = np.asarray(lm, float), np.asarray(g, float), np.asarray(info)
        rec["grads"].append(g)
        rec["logmls"].append(lm)
        rec["infos"].append(info)
        with np.errstate(all="ignore"):
            bad = np.bincount(seg, weights=~np.isfinite(g), minlength=B) > 0
            ok = (info == 0) & np.isfinite(lm) & ~bad
            U = np.where(ok, -lm + 0.5 * item_sums(z * z), np.inf)
            dU = np.where(ok[seg], -g * dth + z, 0.0)
        dU[fr] = 0.0
        return U, dU, lm, info, th

    z0, mom = np.array(z0, float), np.array(mom, float)
    trace = [z0.copy()]
    with np.errstate(all="ignore"):
        U0, dU, lm1, info1, th = potential(z0)
        K0 = 0.5 * item_sums(mom * mom)
        z = z0.copy()
        pm = mom - 0.5 * eps * dU
        U1 = U0
        for step in range(n_leapfrog):
            z = z + eps * pm
            trace.append(z.copy())
            U1, dU, lm1, info1, th = potential(z)
            pm = pm - (eps if step < n_leapfrog - 1 else 0.5 * eps) * dU
        K1 = 0.5 * item_sums(pm * pm)
    return dict(z1=z, mom1=pm, theta1=th, U0=U0, K0=K0, U1=U1, K1=K1, logml1=lm1,
                info1=np.asarray(info1, dtype=np.int32), z_trace=np.array(trace), **rec)


def ulp_nudger(rng):
    """theta -> theta moved by one ulp up or down, at random per entry."""
    def nudge(th):
        up = rng.integers(0, 2, th.size).astype(bool)
        return np.where(up, np.nextafter(th, np.inf), np.nextafter(th, -np.inf))
    return nudge

"""Long-double reference of the device mixture sampler (TEST INFRASTRUCTURE ONLY).

A plain restatement of the contract in include/ngp.h ("mixture sampling on the device"), one step
per method of ``Sampler`` so that tests/test_sampler_reference_cpu.py can break one step at a time:

  words     Philox4x32-10 of the counter (draw, scenario, block, 0) under key = seed (low word, high
            word).  The integer core is ``oracle_np.philox4x32_10`` — 64-bit integer arithmetic, no
            rounding in it — pinned by the Random123 known-answer vectors in the CPU test.  Nothing
            else is shared with ``oracle/``.
  uniforms  (v + 0.5) 2^-53, v the top 53 bits of two words: exact in long double (54 bits).
  pick      block 0; the fp64 running sum of the weight row in index order, the first i with
            u < acc_i (strict), P - 1 when there is none.  u and acc_i are compared exactly; the
            margin min_i |u - acc_i| of every draw is returned, and a case is admitted only if every
            margin exceeds 2^-40 (tests/sampler_cases.py), so no pick depends on anybody's rounding.
  normals   Box-Muller in long double, block 1 + j / 2 gives z_j = r cos a and z_{j+1} = r sin a,
            r = sqrt(-2 log u1), a = 2 pi u2; the second normal of the last pair is dropped when
            m is odd.
  factor    ``hp_reference.cholesky_ld(sigma, pivots=True)``: L, the first failing row, the pivots.
  draw      x = mu_k + L z in long double.
Both forms: shared (mu [P][S][m], sigma [P][m][m], the scenario index in the counter) and independent
(mu [S][P][m], sigma [S][P][m][m], mixture s keyed by seeds[s] with scenario counter 0).

cond(sigma_k) = lambda_max(sigma_k) lambda_max(sigma_k^-1), the inverse formed from the long-double
factor (an fp64 eigenvalue routine finds the LARGEST eigenvalue of either to full relative accuracy,
which it does not do for the smallest), for every component whose factorisation succeeds.

The yardstick of the GPU judgement (tests/test_sampler_gpu.py) is measured with this reference, on
the CPU, against the fp64 oracle ``oracle_np.mixture_sample`` and never against the kernel: r64, the
worst |(x - mu_k)_i - (L z)_i| / (sqrt(sigma_ii) max(1, |z|_inf)) of that oracle over every case and
form of tests/sampler_cases.py, is 2.82e-12 (12,700 eps; at the SE tree of the jitter-only group,
cond 2.4e6; the synthetic shape cases, cond up to 7e4, stay under 900 eps).
The floor of the GPU test is 4 r64 = 1.128e-11 in ``tests.util.tol(floor, cond)``: summation order
and the last bits of log, cos and sin differ between the device and numpy.
"""
from __future__ import annotations

import numpy as np

from oracle.oracle_np import philox4x32_10
from tests import hp_reference as hr

LD = hr.LD
PICK_MARGIN = 2.0 ** -40


class Drawn:
    """x, dev = L z, z [S, draws, m] (long double); comp [S, draws]; u, margin [S, draws];
    info, cond [P] (shared) or [S, P] (independent); piv: the pivots of every matrix, same order"""
    __slots__ = ("x", "dev", "z", "comp", "u", "margin", "info", "cond", "piv", "indep")


def cond_ld(sigma, L):
    """lambda_max(sigma) lambda_max(sigma^-1), sigma^-1 = W'W with W = L^-1 in long double"""
    W = hr.solve_lower(L, np.eye(L.shape[0], dtype=LD))
    inv = (W.T @ W).astype(np.float64)
    return float(np.linalg.eigvalsh(np.asarray(sigma, np.float64))[-1] * np.linalg.eigvalsh(inv)[-1])


class Sampler:
    """the contract; a subclass that overrides one method is the contract with one error"""

    # ---- the stream ---------------------------------------------------------------------------------
    def counter(self, d, scen, block):
        return d, scen, block, np.zeros_like(d)

    def words(self, seed, scen, draws, block):
        d = np.arange(draws, dtype=np.uint64)
        ctr = np.stack(self.counter(d, np.full(draws, scen, np.uint64),
                                    np.full(draws, block, np.uint64)), axis=-1)
        key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint64)
        return philox4x32_10(ctr, key)

    @staticmethod
    def uniform(hi, lo):
        v = ((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(11)
        return (v.astype(LD) + LD(0.5)) * LD(2) ** -53

    # ---- the component --------------------------------------------------------------------------------
    def hit(self, u, acc):
        return u < acc

    def fallback(self, P):
        return P - 1

    def pick(self, wrow, u):
        """(component, margin) of every draw"""
        acc = np.add.accumulate(np.asarray(wrow, np.float64)).astype(LD)    # fp64, index order
        hit = self.hit(u[:, None], acc[None, :])
        k = np.where(hit.any(axis=1), hit.argmax(axis=1), self.fallback(acc.size))
        return k.astype(np.int32), np.min(np.abs(u[:, None] - acc[None, :]), axis=1).astype(np.float64)

    # ---- the normals ----------------------------------------------------------------------------------
    def pair(self, rad, ang):
        return rad * np.cos(ang), rad * np.sin(ang)

    def last_of_odd(self, z0, z1):
        return z0

    def normals(self, seed, scen, draws, m):
        z = np.empty((draws, m), dtype=LD)
        for b in range((m + 1) // 2):
            r = self.words(seed, scen, draws, 1 + b)
            u1, u2 = self.uniform(r[:, 0], r[:, 1]), self.uniform(r[:, 2], r[:, 3])
            z0, z1 = self.pair(np.sqrt(-2 * np.log(u1)), 2 * hr.PI_LD * u2)
            if 2 * b + 1 < m:
                z[:, 2 * b], z[:, 2 * b + 1] = z0, z1
            else:
                z[:, 2 * b] = self.last_of_odd(z0, z1)
        return z

    # ---- the factor and the draw ------------------------------------------------------------------
    def operator(self, L, sigma):
        """the matrix applied to z"""
        return L

    def mean(self, mu, k, s):
        """shared form: mu [P][S][m]"""
        return mu[k, s]

    def _mixture(self, out, s, wrow, mean_of, mats, draws, seed, scen):
        u0 = self.words(seed, scen, draws, 0)
        u = self.uniform(u0[:, 0], u0[:, 1])
        comp, margin = self.pick(wrow, u)
        m = out.x.shape[2]
        z = self.normals(seed, scen, draws, m)
        out.u[s], out.margin[s], out.comp[s], out.z[s] = u.astype(np.float64), margin, comp, z
        for k in np.unique(comp):
            sel = comp == k
            sigma, L = mats[k]
            if L is None:
                out.dev[s, sel] = out.x[s, sel] = np.nan
                continue
            out.dev[s, sel] = z[sel] @ self.operator(L, sigma).T
            out.x[s, sel] = mean_of(k).astype(LD)[None, :] + out.dev[s, sel]

    @staticmethod
    def _factor(sigma):
        L, info, piv = hr.cholesky_ld(np.asarray(sigma, np.float64).astype(LD), pivots=True)
        cond = cond_ld(sigma, L) if info == 0 else np.nan
        return L, info, np.asarray(piv, np.float64), cond

    @staticmethod
    def _alloc(S, draws, m, shape, indep):
        o = Drawn()
        o.x, o.dev, o.z = (np.empty((S, draws, m), dtype=LD) for _ in range(3))
        o.comp = np.empty((S, draws), np.int32)
        o.u, o.margin = np.empty((S, draws)), np.empty((S, draws))
        o.info, o.cond, o.piv, o.indep = np.zeros(shape, np.int32), np.full(shape, np.nan), [], indep
        return o

    def sample(self, w, mu, sigma, draws, seed):
        """the shared form: w [S, P], mu [P, S, m], sigma [P, m, m], one seed"""
        w, mu, sigma = (np.asarray(a, np.float64) for a in (w, mu, sigma))
        (S, P), m = w.shape, mu.shape[2]
        assert mu.shape == (P, S, m) and sigma.shape == (P, m, m)
        out = self._alloc(S, draws, m, (P,), False)
        mats = []
        for k in range(P):
            L, out.info[k], piv, out.cond[k] = self._factor(sigma[k])
            mats.append((sigma[k], L))
            out.piv.append(piv)
        for s in range(S):
            self._mixture(out, s, w[s], lambda k, s=s: self.mean(mu, k, s), mats, draws, seed, s)
        return out

    def sample_indep(self, w, mu, sigma, draws, seeds):
        """the independent form: w [S, P], mu [S, P, m], sigma [S, P, m, m], seeds [S]"""
        w, mu, sigma = (np.asarray(a, np.float64) for a in (w, mu, sigma))
        (S, P), m = w.shape, mu.shape[2]
        assert mu.shape == (S, P, m) and sigma.shape == (S, P, m, m) and len(seeds) == S
        out = self._alloc(S, draws, m, (S, P), True)
        for s in range(S):
            mats = []
            for k in range(P):
                L, out.info[s, k], piv, out.cond[s, k] = self._factor(sigma[s, k])
                mats.append((sigma[s, k], L))
                out.piv.append(piv)
            self._mixture(out, s, w[s], lambda k, s=s: mu[s, k], mats, draws, seeds[s], 0)
        return out


REFERENCE = Sampler()


def sample(w, mu, sigma, draws, seed):
    return REFERENCE.sample(w, mu, sigma, draws, seed)


def sample_indep(w, mu, sigma, draws, seeds):
    return REFERENCE.sample_indep(w, mu, sigma, draws, seeds)

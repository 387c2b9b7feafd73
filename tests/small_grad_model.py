"""numpy model of the one-launch gradient job (not the oracle): the block algebra of
chol_small_kernel, small_inverse_column and grad_kinv_small_kernel (csrc/ngp_small_kernels.h) in
fp64, in the kernels' own cut — 16 x 16 blocks, nbe = ceil(n / 16) of them, the last padded with
identity rows:

  factor   right-looking over block columns; a diagonal block is factored K_jj = Lu D Lu' with a unit
           lower triangular Lu, M_j = D^-1/2 Lu^-1 = L_jj^-1; L_ij = A_ij M_j'
  inverse  W = L^-1 by block columns: W_jj = M_j, W_ij = -M_i sum_(k = j)^(i - 1) L_ik W_kj; the
           products of a column are numbered P = 0, 1, ... stage by stage, and product P takes its
           L block from slot P mod SM_RING of a ring that was asked for it SM_RING products earlier
  K^-1     block (a, b), a >= b, = sum over the 16-groups k of [16 a, 16 nbe) of W_ka' W_kb, walked
           in chunks of four groups; past the end a chunk re-reads the last group, times zero
  alpha    from the diagonal blocks' operands: alpha_a = sum_k W_ka' z_k over the same range
  quad     sum of z_i^2 and logdet = 1/2 sum of log d_i, both over i < n
and the gradient as the contraction of (alpha alpha' - K^-1) / 2 with dK (the oracle's reverse sweep
of the tree: the contraction kernels are not what is modelled here).

``hooks`` makes the model WRONG on purpose, in the ways these kernels can be wrong about the
geometry (tests/test_small_grad_cases_cpu.py: the judge of tests/test_small_grad_gpu.py has to fail
such a model):
  inv_stop(len) -> stages       stages of an inverse column of that length that run (right: len - 1)
  ring_stale(len, P) -> bool    product P reads what its slot held before: the block of P - SM_RING
  kinv_drop(rem) -> bool        the last chunk's live groups are left out (rem = (16 nbe - 16 a) % 64)
  kinv_clamped -> True          the re-read group is multiplied in instead of zeroed
  alpha_end(n, nbe) -> columns  where alpha's sum stops (right: 16 nbe)
  logdet_padded -> True         logdet runs to 16 nbe over padding pivots that kept the filled value
  rho1_as_0 -> True             a series whose last block holds one row is treated as one point shorter
"""
import math

import numpy as np

from oracle import oracle_np

TB = 16
SM_RING = 6


def _ldl_block(A):
    """(d, M): K_jj = Lu diag(d) Lu' with unit lower Lu, M = diag(d)^-1/2 Lu^-1"""
    A = A.copy()
    Lu = np.eye(TB)
    d = np.empty(TB)
    for p in range(TB):
        d[p] = A[p, p]
        r = 1.0 / d[p]
        m = A[p + 1:, p] * r
        Lu[p + 1:, p] = m
        A[p + 1:, p + 1:] -= np.outer(m, A[p + 1:, p])
    Li = np.eye(TB)                      # Lu^-1 by forward substitution, no division
    for p in range(TB):
        Li[p + 1:, :] -= np.outer(Lu[p + 1:, p], Li[p, :])
    return d, Li / np.sqrt(d)[:, None]


def grad_job_model(program, t, y, spec=None, hooks=None):
    """(logml, gradient [npar + 1]) of one item"""
    hooks = hooks or {}
    sp = oracle_np._spec(spec)
    ops, params, noise = program
    t, y = np.asarray(t, float), np.asarray(y, float)
    if hooks.get("rho1_as_0") and t.size % TB == 1:
        t, y = t[:-1], y[:-1]
    n = t.size
    npar = len(params)
    if n == 0:
        return 0.0, np.zeros(npar + 1)
    nbe = (n + TB - 1) // TB
    N = TB * nbe
    blk = lambda i: slice(TB * i, TB * (i + 1))
    K = oracle_np.cov(program, t, t, True, spec)
    A = np.eye(N)
    A[:n, :n] = K
    pad_pivot = K[n - 1, n - 1]          # what the fill leaves on a padding row before it is reset
    # ---- factor ----------------------------------------------------------------------------------
    L = np.zeros((N, N))
    M = []
    piv = np.empty(N)
    for j in range(nbe):
        d, Mj = _ldl_block(A[blk(j), blk(j)])
        piv[blk(j)] = d
        M.append(Mj)
        for i in range(j + 1, nbe):
            L[blk(i), blk(j)] = A[blk(i), blk(j)] @ Mj.T
        for i in range(j + 1, nbe):
            for k in range(j + 1, i + 1):
                A[blk(i), blk(k)] -= L[blk(i), blk(j)] @ L[blk(k), blk(j)].T
    if not (piv > 0).all():
        raise np.linalg.LinAlgError("pivot")
    # ---- inverse: W = L^-1 by block columns --------------------------------------------------------
    small = nbe <= 16                    # (the column kernels of longer series are not modelled)
    W = np.zeros((N, N))
    for j in range(nbe):
        ln = nbe - j
        W[blk(j), blk(j)] = M[j]
        stages = hooks["inv_stop"](ln) if small and "inv_stop" in hooks else ln - 1
        ring = [None] * SM_RING
        want = [(ii, kk) for ii in range(1, ln) for kk in range(ii)]      # product P -> (ii, kk)
        for P in range(min(SM_RING, len(want))):
            ring[P] = L[blk(j + want[P][0]), blk(j + want[P][1])]
        P = 0
        for ii in range(1, stages + 1):
            s = np.zeros((TB, TB))
            for kk in range(ii):
                a = ring[P % SM_RING]
                s += a @ W[blk(j + kk), blk(j)]
                nxt = P + SM_RING
                if nxt < len(want):
                    stale = small and "ring_stale" in hooks and hooks["ring_stale"](ln, nxt)
                    if not stale:
                        ring[nxt % SM_RING] = L[blk(j + want[nxt][0]), blk(j + want[nxt][1])]
                P += 1
            W[blk(j + ii), blk(j)] = -M[j + ii] @ s
    # ---- z = W y, K^-1 = W' W, alpha = W' z, in the K^-1 kernel's cut -------------------------------
    yp = np.zeros(N)
    yp[:n] = y
    z = np.zeros(N)
    for i in range(nbe):                 # (the y' row of the main sweep: z_i = M_i (y_i - sum L_ik z_k))
        z[blk(i)] = M[i] @ (yp[blk(i)] - L[blk(i), :TB * i] @ z[:TB * i])
    Kinv = np.zeros((N, N))
    alpha = np.zeros(N)
    a_end = hooks["alpha_end"](n, nbe) if "alpha_end" in hooks else N
    for a in range(nbe):
        groups = list(range(a, nbe))
        rem = (TB * nbe - TB * a) % 64
        nchunk = (len(groups) + 3) // 4
        for b in range(a + 1):
            acc = np.zeros((TB, TB))
            for c in range(nchunk):
                for u in range(4):
                    k = a + 4 * c + u
                    live = k < nbe
                    if live and c == nchunk - 1 and "kinv_drop" in hooks and hooks["kinv_drop"](rem):
                        continue
                    if not live and not hooks.get("kinv_clamped"):
                        continue
                    k = min(k, nbe - 1)
                    acc += W[blk(k), blk(a)].T @ W[blk(k), blk(b)]
            Kinv[blk(a), blk(b)] = acc
            Kinv[blk(b), blk(a)] = acc.T
        for k in groups:
            cols = np.arange(TB * k, TB * (k + 1))
            cols = cols[cols < a_end]
            alpha[blk(a)] += W[cols, blk(a)].T @ z[cols]
    quad = float(z[:n] @ z[:n])
    if hooks.get("logdet_padded"):
        pv = piv.copy()
        pv[n:] = pad_pivot
        logdet = 0.5 * np.log(pv).sum()
    else:
        logdet = 0.5 * np.log(piv[:n]).sum()
    lm = -0.5 * quad - logdet - 0.5 * n * math.log(2 * math.pi)
    # ---- the contraction (the oracle's) ------------------------------------------------------------
    Q = 0.5 * (np.outer(alpha[:n], alpha[:n]) - Kinv[:n, :n])
    g = []
    oracle_np._eval_adjoint(oracle_np.rpn_to_tree(ops, params), t[:, None], t[None, :], sp, Q, g)
    g.append(float(np.trace(Q)))
    return float(lm), np.array(g)

"""ctypes binding of ``libngp.so`` (C-ABI: ``include/ngp.h``) — the ONLY compute path.

There is no CPU fallback: if the HIP library is missing or no device is usable the calls
raise ``NgpError`` / ``RuntimeError`` loudly.  Build with ``python -c "import __graft_entry__ as
g; g.build()"`` (hipcc --offload-arch=gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import Optional, Sequence

import numpy as np

from ._abi import (KernelArray, NgpHmcConfig, NgpInvTransform, NgpKernel, NgpPathTarget, NgpProfile, NgpSpec,
                   as_f64, c_double_p, c_int32_p, dptr, iptr)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NGP_LIB") or os.path.join(_HERE, "libngp.so")  # NGP_LIB: A/B builds

KERNEL_CLASSES = ("chol_col", "chol_diag", "gram", "epilogue", "fill", "grad_kinv", "chol_col_thin",
                  "aux_update", "diag_ahead", "chol_col_mixed", "refine", "grad_contract",
                  "chol_col_grad", "chol_small")

# every symbol include/ngp.h declares (tests/test_abi.py checks the library exports them all)
SYMBOLS = (
    "ngp_ctx_create", "ngp_ctx_destroy", "ngp_set_spec", "ngp_get_spec", "ngp_default_spec",
    "ngp_strerror", "ngp_version", "ngp_kernel_check", "ngp_cov_batch", "ngp_logml_batch",
    "ngp_predict_batch", "ngp_nowcast_batch", "ngp_logml_grad_batch", "ngp_grad_stage",
    "ngp_grad_job_set_params", "ngp_grad_job_run", "ngp_grad_job_destroy", "ngp_weights_normalize",
    "ngp_weights_normalize_cols", "ngp_mixture_sample_indep", "ngp_shard", "ngp_comm_unique_id", "ngp_comm_create",
    "ngp_comm_destroy", "ngp_weights_allgather_normalize",
    "ngp_logml_stage", "ngp_predict_stage", "ngp_nowcast_stage", "ngp_job_run", "ngp_job_fetch",
    "ngp_job_mixed_stats", "ngp_job_destroy", "ngp_factor_create", "ngp_factor_logml", "ngp_factor_nowcast",
    "ngp_factor_destroy", "ngp_mixture_sample", "ngp_set_structured_storage", "ngp_profile_enable", "ngp_profile_reset", "ngp_profile_get",
    "ngp_microbench_mfma_f64", "ngp_microbench_mfma_f64_detail", "ngp_microbench_hbm", "ngp_selftest_mfma_layout",
    "ngp_selftest_mfma_f32_layout", "ngp_set_combining", "ngp_combine_stats",
    "ngp_weights_unpad_normalize", "ngp_grad_job_info", "ngp_set_batch_invariant", "ngp_set_short_series_path",
    "ngp_mixture_cdf", "ngp_mixture_quantiles", "ngp_mixture_crps", "ngp_microbench_mixture_pairs",
    "ngp_kernel_components", "ngp_factor_components",
    "ngp_kernel_terms", "ngp_factor_components_nowcast",
    "ngp_mixture_path_targets", "ngp_mixture_path_targets_indep",
    "ngp_mixture_crps_mapped",
    "ngp_grad_job_hmc",
    "ngp_ensemble_scores", "ngp_mixture_path_scores",
    "ngp_factor_predict_long",
    "ngp_factor_sample_long",
    "ngp_factor_sample_long_indep",
    "ngp_factor_components_long",
    "ngp_factor_predict_origins",
)


class NgpError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        super().__init__(f"{where}: {_strerror(status)} (status {status})")


class PosDefException(ArithmeticError):
    """Leading minor ``k`` of a covariance matrix is not positive definite (LAPACK potrf info;
    the reference surfaces this as Julia's PosDefException, src/make_and_fit_model.jl:6-8)."""

    def __init__(self, k: int, item: int):
        self.info, self.item = k, item
        super().__init__(f"matrix is not positive definite; Cholesky failed at minor {k} "
                         f"(item {item})")


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run __graft_entry__.build()); there is no CPU fallback for the GP hot path")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f64p, i32p = C.c_void_p, C.c_int32, C.c_int64, c_double_p, c_int32_p
    KP, SP = C.POINTER(NgpKernel), C.POINTER(NgpSpec)
    sig = {
        "ngp_ctx_create": (i32, [i32, C.POINTER(vp)]),
        "ngp_ctx_destroy": (None, [vp]),
        "ngp_set_spec": (i32, [vp, SP]),
        "ngp_get_spec": (i32, [vp, SP]),
        "ngp_default_spec": (None, [SP]),
        "ngp_strerror": (C.c_char_p, [i32]),
        "ngp_version": (C.c_char_p, []),
        "ngp_kernel_check": (i32, [KP]),
        "ngp_cov_batch": (i32, [vp, i32, KP, i32, f64p, i32, f64p, i32, f64p]),
        "ngp_logml_batch": (i32, [vp, i32, KP, i32, f64p, f64p, i64, f64p, i32p]),
        "ngp_predict_batch": (i32, [vp, i32, KP, i32, f64p, f64p, i64, i32, f64p, i32, f64p, f64p,
                                    f64p, i32p]),
        "ngp_nowcast_batch": (i32, [vp, i32, KP, i32, f64p, f64p, i32, f64p, i32, f64p, i32, f64p,
                                    i32, f64p, f64p, f64p, f64p, i32p]),
        "ngp_logml_grad_batch": (i32, [vp, i32, KP, i32, f64p, f64p, i64, f64p, f64p, i32p]),
        "ngp_grad_stage": (i32, [vp, i32, KP, i32, f64p, f64p, i64, C.POINTER(vp)]),
        "ngp_grad_job_set_params": (i32, [vp, f64p, f64p]),
        "ngp_grad_job_run": (i32, [vp, f64p, f64p, i32p]),
        "ngp_grad_job_info": (i32, [vp, i32p]),
        "ngp_grad_job_hmc": (i32, [vp, vp, vp, vp, f64p, f64p, f64p, f64p, f64p, f64p, f64p, f64p,
                                   f64p, f64p, i32p, f64p]),
        "ngp_grad_job_destroy": (None, [vp]),
        "ngp_weights_normalize": (i32, [i32, f64p, f64p, f64p, f64p]),
        "ngp_weights_normalize_cols": (i32, [i32, i32, f64p, f64p, f64p, f64p]),
        "ngp_mixture_sample_indep": (i32, [vp, i32, i32, i32, f64p, f64p, f64p, i32,
                                           C.POINTER(C.c_uint64), f64p, i32p, i32p]),
        "ngp_shard": (i32, [i32, i32, i32, i32p, i32p]),
        "ngp_comm_unique_id": (i32, [vp]),
        "ngp_comm_create": (i32, [vp, vp, i32, i32, C.POINTER(vp)]),
        "ngp_comm_destroy": (None, [vp]),
        "ngp_weights_allgather_normalize": (i32, [vp, i32, i32, f64p, f64p, f64p, f64p, f64p]),
        "ngp_weights_unpad_normalize": (i32, [i32, i32, i32, f64p, f64p, f64p, f64p]),
        "ngp_logml_stage": (i32, [vp, i32, KP, i32, f64p, f64p, i64, C.POINTER(vp)]),
        "ngp_predict_stage": (i32, [vp, i32, KP, i32, f64p, f64p, i64, i32, f64p, i32,
                                    C.POINTER(vp)]),
        "ngp_nowcast_stage": (i32, [vp, i32, KP, i32, f64p, f64p, i32, f64p, i32, f64p, i32, f64p,
                                    i32, C.POINTER(vp)]),
        "ngp_job_run": (i32, [vp]),
        "ngp_job_fetch": (i32, [vp, f64p, f64p, f64p, f64p, i32p]),
        "ngp_job_mixed_stats": (i32, [vp, i32p, f64p, f64p]),
        "ngp_job_destroy": (None, [vp]),
        "ngp_factor_create": (i32, [vp, i32, KP, i32, f64p, f64p, i64, C.POINTER(vp)]),
        "ngp_factor_logml": (i32, [vp, f64p, i32p]),
        "ngp_factor_nowcast": (i32, [vp, i32, f64p, i32, f64p, i32, f64p, i32, f64p, f64p, f64p,
                                     f64p, i32p]),
        "ngp_factor_destroy": (None, [vp]),
        "ngp_factor_predict_long": (i32, [vp, i32, f64p, i32, f64p, i32, f64p, i32, f64p, f64p, f64p,
                                          i32p]),
        "ngp_factor_sample_long": (i32, [vp, i32, f64p, i32, f64p, i32, f64p, i32, f64p, i32,
                                         C.c_uint64, f64p, i32p, f64p, f64p, i32p, i32p]),
        "ngp_factor_sample_long_indep": (i32, [vp, i32, i32, f64p, i32, f64p, i32,
                                               C.POINTER(C.c_uint64), f64p, i32p, f64p, f64p, i32p,
                                               i32p]),
        "ngp_kernel_components": (i32, [KP, i32p, i32p, i32p, i32p, i32p]),
        "ngp_factor_components": (i32, [vp, i32p, KP, i32, f64p, f64p, f64p, f64p, i32p]),
        "ngp_kernel_terms": (i32, [KP, i32, i32, i32p, i32p, i32p, i32p, i32p, i32p, i32, f64p, i32]),
        "ngp_factor_components_nowcast": (i32, [vp, i32, f64p, i32, f64p, i32p, KP, i32, f64p, f64p,
                                                f64p, f64p, f64p, i32p]),
        "ngp_factor_components_long": (i32, [vp, i32, f64p, i32, f64p, i32p, KP, i32, f64p, f64p,
                                             f64p, f64p, i32p]),
        "ngp_factor_predict_origins": (i32, [vp, i32, i32p, i32, f64p, i32, f64p, f64p, f64p, i32p]),
        "ngp_mixture_sample": (i32, [vp, i32, i32, i32, f64p, f64p, f64p, i32, C.c_uint64, f64p,
                                     i32p, i32p]),
        "ngp_mixture_cdf": (i32, [vp, i32, i32, f64p, f64p, f64p, i32, f64p, f64p, i32p]),
        "ngp_mixture_quantiles": (i32, [vp, i32, i32, f64p, f64p, f64p, i32, f64p, f64p, i32p]),
        "ngp_mixture_crps": (i32, [vp, i32, i32, f64p, f64p, f64p, f64p, f64p, i32p]),
        "ngp_microbench_mixture_pairs": (i32, [vp, i32, f64p]),
        "ngp_mixture_crps_mapped": (i32, [vp, i32, i32, f64p, f64p, f64p, C.POINTER(NgpInvTransform),
                                          i32, C.c_double, f64p, C.c_double, f64p, f64p, f64p, i32p]),
        "ngp_mixture_path_targets": (i32, [vp, i32, i32, i32, f64p, f64p, f64p, i32, C.c_uint64,
                                           C.POINTER(NgpInvTransform), i32, C.POINTER(NgpPathTarget),
                                           i32, f64p, f64p, f64p, C.POINTER(i64), C.POINTER(i64),
                                           f64p, i32p]),
        "ngp_mixture_path_targets_indep": (i32, [vp, i32, i32, i32, f64p, f64p, f64p, i32,
                                                 C.POINTER(C.c_uint64), C.POINTER(NgpInvTransform),
                                                 i32, C.POINTER(NgpPathTarget), i32, f64p, f64p,
                                                 f64p, C.POINTER(i64), C.POINTER(i64), f64p, i32p]),
        "ngp_ensemble_scores": (i32, [vp, i32, i32, f64p, f64p, i32, C.c_double, i32, i32, i32p, f64p,
                                      f64p, f64p, i32p]),
        "ngp_mixture_path_scores": (i32, [vp, i32, i32, i32, f64p, f64p, f64p, i32, i32,
                                          C.POINTER(C.c_uint64), C.POINTER(NgpInvTransform), f64p, i32,
                                          C.c_double, i32, i32, i32p, f64p, f64p, f64p, i32p, i32p]),
        "ngp_set_structured_storage": (i32, [vp, i32]),
        "ngp_set_combining": (i32, [vp, i32]),
        "ngp_set_batch_invariant": (i32, [vp, i32]),
        "ngp_set_short_series_path": (i32, [vp, i32]),
        "ngp_combine_stats": (i32, [vp, C.POINTER(C.c_int64), i32]),
        "ngp_profile_enable": (i32, [vp, i32]),
        "ngp_profile_reset": (i32, [vp]),
        "ngp_profile_get": (i32, [vp, C.POINTER(NgpProfile)]),
        "ngp_microbench_mfma_f64": (i32, [vp, i32, f64p]),
        "ngp_microbench_mfma_f64_detail": (i32, [vp, i32, i32, f64p]),
        "ngp_microbench_hbm": (i32, [vp, i64, f64p, f64p]),
        "ngp_selftest_mfma_layout": (i32, [vp, f64p, f64p, f64p]),
        "ngp_selftest_mfma_f32_layout": (i32, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                               C.POINTER(C.c_float)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def _strerror(st: int) -> str:
    try:
        return load().ngp_strerror(int(st)).decode()
    except Exception:  # pragma: no cover
        return "?"


def _chk(st: int, where: str):
    if st != 0:
        raise NgpError(int(st), where)


def kernel_check(program) -> int:
    ka = KernelArray([program])
    return int(load().ngp_kernel_check(C.byref(ka.arr[0])))


def kernel_components(program):
    """The additive components of a program (``ngp_kernel_components``): the maximal non-Plus
    subtrees under the root's Plus nodes, left to right, each a program of its own —
    ``[(ops, params, noise), ...]`` with the slices of the caller's arrays."""
    from ._abi import NGP_MAX_OPS
    ka = KernelArray([program])
    cap = NGP_MAX_OPS // 2 + 1
    cnt = C.c_int32()
    of, ol, pf, pl = (np.zeros(cap, dtype=np.int32) for _ in range(4))
    _chk(load().ngp_kernel_components(C.byref(ka.arr[0]), C.byref(cnt), iptr(of), iptr(ol), iptr(pf),
                                      iptr(pl)), "ngp_kernel_components")
    ops = np.asarray(program[0], dtype=np.int32).reshape(-1)
    params = np.asarray(program[1], dtype=np.float64).reshape(-1)
    return [(ops[of[i]:of[i] + ol[i]].copy(), params[pf[i]:pf[i] + pl[i]].copy(), float(program[2]))
            for i in range(int(cnt.value))]


def kernel_terms(program, split, max_terms=None):
    """The sum-of-products terms of a program (``ngp_kernel_terms``): new programs that sum to it,
    ``[(ops, params, noise), ...]``.  ``split``: NGP_SPLIT_* flags or-ed (0: the components of
    ``kernel_components``).  More than ``max_terms`` terms (None: no limit), or a term that is no
    valid program: ``NgpError`` with status NGP_ERR_TOO_LARGE, its ``count`` the number of terms."""
    ka = KernelArray([program])
    cnt = C.c_int32()
    L = load()
    st = L.ngp_kernel_terms(C.byref(ka.arr[0]), int(split), 2**31 - 1 if max_terms is None else int(max_terms),
                            C.byref(cnt), None, None, None, None, None, 0, None, 0)
    if st != 0:
        err = NgpError(int(st), "ngp_kernel_terms")
        err.count = int(cnt.value)
        raise err
    n = int(cnt.value)
    n_ops = np.asarray(program[0]).size
    n_par = np.asarray(program[1]).size
    of, ol, pf, pl = (np.zeros(n, dtype=np.int32) for _ in range(4))
    ops, par = np.zeros(n * n_ops, dtype=np.int32), np.zeros(max(n * n_par, 1))   # a term is no longer than the tree
    st = L.ngp_kernel_terms(C.byref(ka.arr[0]), int(split), n, C.byref(cnt), iptr(of), iptr(ol), iptr(pf),
                            iptr(pl), iptr(ops), ops.size, dptr(par), n * n_par)
    if st != 0:
        err = NgpError(int(st), "ngp_kernel_terms")
        err.count = int(cnt.value)
        raise err
    return [(ops[of[i]:of[i] + ol[i]].copy(), par[pf[i]:pf[i] + pl[i]].copy(), float(program[2]))
            for i in range(n)]


def weights_normalize(logw):
    """maybe_resample! arithmetic (reference src/forecasting.jl:138-141); host-side, P doubles."""
    logw = as_f64(logw)
    w = np.empty(logw.size)
    ess, ln = C.c_double(), C.c_double()
    _chk(load().ngp_weights_normalize(logw.size, dptr(logw), dptr(w), C.byref(ess), C.byref(ln)),
         "ngp_weights_normalize")
    return w, float(ess.value), float(ln.value)


def weights_normalize_cols(logw):
    """``weights_normalize`` of every COLUMN of a [P, D] matrix in one call: (w [P, D], ess [D],
    log_norm [D])."""
    logw = as_f64(logw)
    P, D = logw.shape
    w, ess, ln = np.empty((P, D)), np.empty(D), np.empty(D)
    _chk(load().ngp_weights_normalize_cols(P, D, dptr(logw), dptr(w), dptr(ess), dptr(ln)),
         "ngp_weights_normalize_cols")
    return w, ess, ln


NGP_ERR_UNAVAILABLE = -6


def weights_unpad_normalize(padded, P_total: int, world: int):
    """``ngp_weights_unpad_normalize``: ``padded`` [world, pmax, D] (what an all-gather of
    zero-padded shards delivers) -> (w_all [P_total, D], ess [D], log_norm [D])."""
    padded = as_f64(padded)
    D = padded.shape[-1]
    w = np.empty((int(P_total), D))
    ess, ln = np.empty(D), np.empty(D)
    _chk(load().ngp_weights_unpad_normalize(int(P_total), int(world), D, dptr(padded), dptr(w),
                                            dptr(ess), dptr(ln)), "ngp_weights_unpad_normalize")
    return w, ess, ln


def shard(P_total: int, world: int, rank: int):
    """(first, rows) of ``rank`` in the block partition the library's collective uses (``ngp_shard``)."""
    a, b = C.c_int32(), C.c_int32()
    _chk(load().ngp_shard(int(P_total), int(world), int(rank), C.byref(a), C.byref(b)), "ngp_shard")
    return int(a.value), int(b.value)


def comm_unique_id() -> bytes:
    """The 128-byte id rank 0 makes for ``Comm`` (``ngp_comm_unique_id``); raises ``NgpError`` with
    status NGP_ERR_UNAVAILABLE when librccl is not installed."""
    buf = C.create_string_buffer(128)
    _chk(load().ngp_comm_unique_id(buf), "ngp_comm_unique_id")
    return buf.raw


class _Handle:
    """A handle of the C-ABI that lives inside a context (``self._h``, destroyed once by the
    function ``_destroy`` names).  The handle points into its context: where ``_needs_ctx`` is
    set, a context closed first (``self.ctx._h`` None) has already destroyed it."""
    _destroy = ""
    _needs_ctx = True

    def close(self):
        if self._h and (not self._needs_ctx or self.ctx._h is not None):
            getattr(load(), self._destroy)(self._h)
        self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class Comm(_Handle):
    """The C-ABI's own communicator over RCCL (``ngp_comm``): the one exchange of the path for
    hosts without torch.distributed.  The Python mirror itself uses torch.distributed."""
    _destroy = "ngp_comm_destroy"

    def __init__(self, ctx: "Context", uid: bytes, rank: int, world: int):
        h = C.c_void_p()
        _chk(load().ngp_comm_create(ctx._h, C.c_char_p(uid), int(rank), int(world), C.byref(h)),
             "ngp_comm_create")
        self._h, self.ctx, self.rank, self.world = h, ctx, rank, world
        ctx._children.add(self)

    def allgather_normalize(self, logw_local, P_total: int):
        """logw_local [P_local, D] -> (w_local [P_local, D], w_all [P_total, D], ess [D], log_norm [D])"""
        lw = as_f64(logw_local)
        if lw.ndim == 1:
            lw = lw[:, None]
        P_loc, D = lw.shape
        w_loc, w_all = np.empty((P_loc, D)), np.empty((int(P_total), D))
        ess, ln = np.empty(D), np.empty(D)
        _chk(load().ngp_weights_allgather_normalize(self._h, int(P_total), D, dptr(lw), dptr(w_loc),
                                                    dptr(w_all), dptr(ess), dptr(ln)),
             "ngp_weights_allgather_normalize")
        return w_loc, w_all, ess, ln


def _nullable(a: Optional[np.ndarray]):
    return dptr(a) if a is not None else None


_u64p = C.POINTER(C.c_uint64)


def _mixture_args(who, w, mu, sigma, seed, indep=None):
    """The forecast mixture the sampler and the consumers of its paths take: w [S,P] with mu [P,S,m],
    sigma [P,m,m] and one seed (shared components), or with mu [S,P,m], sigma [S,P,m,m] and S seeds
    (independent mixtures; ``indep`` None: a ``seed`` that is a sequence says so) ->
    (w, mu, sigma as float64, the seed(s) as a uint64 array, indep, S, P, m)."""
    w, mu, sigma = as_f64(w), as_f64(mu), as_f64(sigma)
    if indep is None:
        indep = not np.isscalar(seed)
        if w.ndim != 2 or mu.ndim != 3:
            raise ValueError(f"{who}: w [S,P], mu [P,S,m] ([S,P,m] with S seeds)")
    S, P = w.shape
    m = mu.shape[2]
    if indep:
        if mu.shape != (S, P, m) or sigma.shape != (S, P, m, m) or len(seed) != S:
            raise ValueError(f"{who}: w [S,P], mu [S,P,m], sigma [S,P,m,m], seeds [S]")
    elif mu.shape != (P, S, m) or sigma.shape != (P, m, m):
        raise ValueError(f"{who}: w [S,P], mu [P,S,m], sigma [P,m,m]")
    sd = np.array([int(v) & (2**64 - 1) for v in (seed if indep else [seed])], dtype=np.uint64)
    return w, mu, sigma, sd, indep, S, P, m


def _inv_transform(inv):
    """(kind, lam, offset, cap) -> NgpInvTransform"""
    return NgpInvTransform(int(inv[0]), float(inv[1]), float(inv[2]), float(inv[3]))


def _appended(t_add, y_add):
    """The appended points t_add [d] and their scenarios y_add [D, d] (d = 0: one scenario of no
    points) -> (d, D, t_add, y_add, pointer to t_add, pointer to y_add); NULL pointers for d = 0.
    The caller keeps the arrays until the call has returned."""
    t_add = as_f64(t_add)
    d = t_add.size
    y_add = as_f64(y_add).reshape(-1, d) if d else np.zeros((1, 0))
    return d, y_add.shape[0], t_add, y_add, dptr(t_add) if d else None, dptr(y_add) if d else None


def _per_particle(counts, m, mu, var, sg):
    """The flat outputs of the component queries as per-particle lists: mu and var [C_p, ...],
    sigma [C_p m, C_p m] (row = c m + j; sg None: None)."""
    first = np.concatenate([[0], np.cumsum(counts)])
    rows = counts.astype(np.int64) * m
    soff = np.concatenate([[0], np.cumsum(rows ** 2)])
    ps = range(counts.size)
    return dict(mu=[mu[first[p]:first[p + 1]] for p in ps], var=[var[first[p]:first[p + 1]] for p in ps],
                sigma=(None if sg is None else
                       [sg[soff[p]:soff[p + 1]].reshape(int(rows[p]), int(rows[p])) for p in ps]))


class GradJob(_Handle):
    """A gradient job whose trees, dates and observations stay on the device (``ngp_grad_stage``):
    ``run(ka)`` evaluates logml and gradient for the parameters ``ka`` holds NOW (the same trees —
    ``KernelArray.set_params`` between runs), sending nothing else across the bus."""
    _destroy, _needs_ctx = "ngp_grad_job_destroy", False

    def __init__(self, ctx: "Context", handle, ka: KernelArray):
        self._ctx, self._h, self.n = ctx, handle, ka.n
        ctx._children.add(self)          # closed with the context if still open (it holds a ctx pointer)
        self._ngrad = int(ka._npar.sum()) + ka.n

    def run(self, ka: Optional[KernelArray] = None):
        L = load()
        if ka is not None:
            if ka.n != self.n or int(ka._npar.sum()) + ka.n != self._ngrad:
                raise ValueError("GradJob.run: the kernel array must hold the staged trees")
            noise = np.ascontiguousarray(ka._rec["noise"][:ka.n])
            _chk(L.ngp_grad_job_set_params(self._h, dptr(ka._params), dptr(noise)),
                 "ngp_grad_job_set_params")
        grad = np.empty(self._ngrad)
        lm, info = np.empty(self.n), np.zeros(self.n, dtype=np.int32)
        _chk(L.ngp_grad_job_run(self._h, dptr(lm), dptr(grad), iptr(info)), "ngp_grad_job_run")
        return lm, grad, info

    def hmc(self, codes, z0, mom, n_leapfrog: int, eps: float, prior, frozen=None,
            trace: bool = False) -> dict:
        """``ngp_grad_job_hmc``: one whole leapfrog trajectory of every item on the device.
        ``codes`` (``gp.KIND_CODES``), ``z0``, ``mom`` and ``frozen`` are per latent, laid out as the
        gradient is (an item's parameters in program order, then its noise); ``prior`` is the
        config's ``{"gamma" | "period" | "wildcard": {"mu", "sigma"}}``.  Returns ``z1``, ``mom1``,
        ``theta1`` per latent, ``U0``, ``K0``, ``U1``, ``K1``, ``logml1``, ``info1`` per item and,
        with ``trace``, ``z_trace`` [n_leapfrog + 1][latents].  The job then holds ``theta1``."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        z0, mom = as_f64(z0), as_f64(mom)
        if codes.size != self._ngrad or z0.size != self._ngrad or mom.size != self._ngrad:
            raise ValueError("GradJob.hmc: one entry per latent (parameters and noise of every item)")
        fr = None
        if frozen is not None:
            fr = np.ascontiguousarray(frozen, dtype=np.uint8)
            if fr.size != self._ngrad:
                raise ValueError("GradJob.hmc: frozen has one entry per latent")
        cfg = NgpHmcConfig()
        cfg.n_leapfrog, cfg.eps = int(n_leapfrog), float(eps)
        for name, code in (("gamma", 2), ("period", 3), ("wildcard", 4)):
            cfg.prior_mu[code] = float(prior[name]["mu"])
            cfg.prior_sigma[code] = float(prior[name]["sigma"])
        cfg.prior_sigma[0] = cfg.prior_sigma[1] = 1.0
        out = {k: np.empty(self._ngrad) for k in ("z1", "mom1", "theta1")}
        out.update({k: np.empty(self.n) for k in ("U0", "K0", "U1", "K1", "logml1")})
        out["info1"] = np.zeros(self.n, dtype=np.int32)
        if trace:
            out["z_trace"] = np.empty((int(n_leapfrog) + 1, self._ngrad))
        _chk(load().ngp_grad_job_hmc(
            self._h, C.cast(C.pointer(cfg), C.c_void_p), codes.ctypes.data_as(C.c_void_p),
            fr.ctypes.data_as(C.c_void_p) if fr is not None else None, dptr(z0), dptr(mom),
            dptr(out["z1"]), dptr(out["mom1"]), dptr(out["theta1"]), dptr(out["U0"]), dptr(out["K0"]),
            dptr(out["U1"]), dptr(out["K1"]), dptr(out["logml1"]), iptr(out["info1"]),
            dptr(out["z_trace"]) if trace else None), "ngp_grad_job_hmc")
        return out

    def info(self) -> dict:
        """``ngp_grad_job_info``: how the batch is carried (leaves, chunk sizes of the last run)."""
        out = np.zeros(5, dtype=np.int32)
        _chk(load().ngp_grad_job_info(self._h, iptr(out)), "ngp_grad_job_info")
        return dict(general_items=int(out[0]), general_chunk=int(out[1]), toeplitz_items=int(out[2]),
                    toeplitz_chunk=int(out[3]), side_by_side=bool(out[4]))


class Job(_Handle):
    """A staged batch: inputs resident in HBM; ``run`` enqueues every kernel and waits."""
    _destroy = "ngp_job_destroy"

    def __init__(self, ctx: "Context", handle, P: int, D: int, m: int, keep):
        self.ctx, self._h, self.P, self.D, self.m = ctx, handle, P, D, m
        self._keep = keep
        ctx._children.add(self)

    def run(self):
        _chk(load().ngp_job_run(self._h), "ngp_job_run")
        return self

    def fetch(self):
        P, D, m = self.P, self.D, self.m
        lb, lf = np.empty(P), np.empty((P, D))
        mu = np.empty((P, D, m)) if m else None
        sg = np.empty((P, m, m)) if m else None
        info = np.zeros(P, dtype=np.int32)
        _chk(load().ngp_job_fetch(self._h, dptr(lb), dptr(lf), _nullable(mu), _nullable(sg),
                                  iptr(info)), "ngp_job_fetch")
        return dict(logml_base=lb, logml_full=lf, mu=mu, sigma=sg, info=info)

    def mixed_stats(self):
        """NGP_PREC_MIXED jobs: per item the refinement steps taken, the size of the last
        correction and the share of tile products that ran on the fp32 matrix cores."""
        steps = np.zeros(self.P, dtype=np.int32)
        delta, frac = np.zeros(self.P), np.zeros(self.P)
        _chk(load().ngp_job_mixed_stats(self._h, iptr(steps), dptr(delta), dptr(frac)),
             "ngp_job_mixed_stats")
        return dict(refine_steps=steps, refine_delta=delta, frac_f32=frac)


class Factor(_Handle):
    """Training covariances of P kernels factorised once and kept on the device (``ngp_factor``):
    every query sweeps only its appended / forecast rows through the resident L."""
    _destroy = "ngp_factor_destroy"

    def __init__(self, ctx: "Context", handle, P: int):
        self.ctx, self._h, self.P = ctx, handle, P
        ctx._children.add(self)

    def logml(self):
        lm, info = np.empty(self.P), np.zeros(self.P, dtype=np.int32)
        _chk(load().ngp_factor_logml(self._h, dptr(lm), iptr(info)), "ngp_factor_logml")
        return lm, info

    def nowcast(self, t_add, y_add, t_new, noise_on_new=True):
        """Same result dict as ``Context.nowcast_batch`` (``t_add`` empty: plain predict)."""
        d, D, t_add, y_add, p_t, p_y = _appended(t_add, y_add)
        t_new = as_f64(t_new)
        m, P = t_new.size, self.P
        lb, lf = np.empty(P), np.empty((P, D))
        mu = np.empty((P, D, m)) if m else None
        sg = np.empty((P, m, m)) if m else None
        info = np.zeros(P, dtype=np.int32)
        _chk(load().ngp_factor_nowcast(self._h, d, p_t, D, p_y, m, dptr(t_new) if m else None,
                                       int(noise_on_new), dptr(lb), dptr(lf), _nullable(mu),
                                       _nullable(sg), iptr(info)), "ngp_factor_nowcast")
        return dict(logml_base=lb, logml_full=lf, mu=mu, sigma=sg, info=info)

    def predict_long(self, t_new, t_add=None, y_add=None, noise_on_new=True, want_sigma=True):
        """One query for a horizon of up to ``NGP_MAX_LONG_HORIZON`` dates
        (``ngp_factor_predict_long``): the dates are the panel of a triangular solve against the
        resident L, not aux rows.  ``t_add`` [d] / ``y_add`` [D, d] as ``nowcast`` (None or empty:
        plain predict).  Returns ``(mu [P, D, m], var [P, m], sigma [P, m, m] or None, info [P])``;
        without ``want_sigma`` no m x m array is formed.  No weight update: ``nowcast`` with no
        dates gives it."""
        d, D, t_add, y_add, p_t, p_y = _appended(t_add if t_add is not None else np.zeros(0), y_add)
        t_new = as_f64(t_new)
        m, P = t_new.size, self.P
        mu, var = np.empty((P, D, m)), np.empty((P, m))
        sg = np.empty((P, m, m)) if want_sigma else None
        info = np.zeros(P, dtype=np.int32)
        _chk(load().ngp_factor_predict_long(self._h, d, p_t, D, p_y, m, dptr(t_new) if m else None,
                                            int(noise_on_new), dptr(mu), dptr(var), _nullable(sg),
                                            iptr(info)), "ngp_factor_predict_long")
        return mu, var, sg, info

    def sample_long(self, t_new, w, draws, seed, t_add=None, y_add=None, noise_on_new=True,
                    want_moments=False):
        """Paths of a horizon of up to ``NGP_MAX_LONG_HORIZON`` dates drawn on the device
        (``ngp_factor_sample_long``): the mixtures ``w`` [S, P] (S = D with appended points, else 1)
        over the components ``predict_long`` returns for the same query, under the contract of
        ``mixture_sample``.  sigma is formed, factorised and used on the device and never comes
        back.  Returns ``(out [S, draws, m], comp [S, draws], info [P], chol_info [P])``, with
        ``want_moments`` also ``mu [P, S, m]`` and ``var [P, m]`` (``predict_long``'s bits).  A path
        picked from a particle with ``info > 0`` or ``chol_info > 0`` is NaN."""
        d, D, t_add, y_add, p_t, p_y = _appended(t_add if t_add is not None else np.zeros(0), y_add)
        t_new = as_f64(t_new)
        m, P = t_new.size, self.P
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1, P))
        if w.shape[0] != D:
            raise ValueError(f"sample_long: {w.shape[0]} rows of weights for {D} scenarios")
        draws = int(draws)
        out = np.empty((D, max(draws, 0), m))
        comp = np.zeros((D, max(draws, 0)), dtype=np.int32)
        info, cinfo = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
        mu = np.empty((P, D, m)) if want_moments else None
        var = np.empty((P, m)) if want_moments else None
        _chk(load().ngp_factor_sample_long(self._h, d, p_t, D, p_y, m, dptr(t_new) if m else None,
                                           int(noise_on_new), dptr(w), draws,
                                           C.c_uint64(int(seed) & (2**64 - 1)), dptr(out),
                                           iptr(comp), _nullable(mu), _nullable(var), iptr(info),
                                           iptr(cinfo)), "ngp_factor_sample_long")
        return (out, comp, info, cinfo, mu, var) if want_moments else (out, comp, info, cinfo)

    def sample_long_indep(self, t_new, w, draws, seeds, noise_on_new=True, want_moments=False):
        """``sample_long`` for S mixtures that share no component
        (``ngp_factor_sample_long_indep``): the factor's P items are S = len(seeds) mixtures of
        P' = P / S components each, mixture-major (item s P' + k is component k of mixture s), with
        weights ``w`` [S, P'] and no appended points.  Mixture s is keyed by ``seeds[s]`` and draws
        what ``sample_long`` draws on a factor of its own items alone.  Returns ``(out [S, draws,
        m], comp [S, draws], info [P], chol_info [P])``, with ``want_moments`` also ``mu [P, m]``
        and ``var [P, m]`` (``predict_long``'s bits).  A path picked from an item with ``info > 0``
        or ``chol_info > 0`` is NaN."""
        t_new = as_f64(t_new)
        m, P = t_new.size, self.P
        seeds = np.ascontiguousarray(np.asarray([int(s) & (2**64 - 1) for s in np.asarray(seeds, dtype=object).reshape(-1)],
                                                dtype=np.uint64))
        S = seeds.size
        if S < 1 or P % S:
            raise ValueError(f"sample_long_indep: {P} items are not {S} mixtures of equal size")
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
        if w.size != P:
            raise ValueError(f"sample_long_indep: {w.size} weights for {P} items")
        draws = int(draws)
        out = np.empty((S, max(draws, 0), m))
        comp = np.zeros((S, max(draws, 0)), dtype=np.int32)
        info, cinfo = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
        mu = np.empty((P, m)) if want_moments else None
        var = np.empty((P, m)) if want_moments else None
        _chk(load().ngp_factor_sample_long_indep(
            self._h, S, m, dptr(t_new) if m else None, int(noise_on_new), dptr(w), draws,
            seeds.ctypes.data_as(C.POINTER(C.c_uint64)), dptr(out), iptr(comp), _nullable(mu),
            _nullable(var), iptr(info), iptr(cinfo)), "ngp_factor_sample_long_indep")
        return (out, comp, info, cinfo, mu, var) if want_moments else (out, comp, info, cinfo)

    def components(self, comps, t_new, want_sigma=True):
        """The joint posterior of every particle's additive parts (``ngp_factor_components``).
        ``comps``: per particle the list of its component programs (any kernels: the library does
        not check that they sum to the particle's).  Returns ``mu`` and ``var`` as lists of
        [C_p, m] arrays, ``sigma`` as a list of [C_p m, C_p m] arrays (row = c m + j; None without
        ``want_sigma``) and ``info`` [P]; the outputs of a particle with info > 0 are NaN."""
        if len(comps) != self.P:
            raise ValueError("one list of component programs per particle")
        t_new = as_f64(t_new)
        m = t_new.size
        counts = np.array([len(c) for c in comps], dtype=np.int32)
        ka = KernelArray([prog for c in comps for prog in c])
        tot = int(counts.sum())
        mu, var = np.empty((tot, m)), np.empty((tot, m))
        sizes = (counts.astype(np.int64) * m) ** 2
        sg = np.empty(int(sizes.sum())) if want_sigma else None
        info = np.zeros(self.P, dtype=np.int32)
        _chk(load().ngp_factor_components(self._h, iptr(counts), ka.arr, m, dptr(t_new) if m else None,
                                          dptr(mu), _nullable(sg), dptr(var), iptr(info)),
             "ngp_factor_components")
        return dict(**_per_particle(counts, m, mu, var, sg), info=info)

    def components_nowcast(self, comps, t_add, y_add, t_new, want_sigma=True):
        """``components`` conditioned on the appended points ``t_add`` [d] and the scenarios
        ``y_add`` [D, d] (``ngp_factor_components_nowcast``).  As ``components``, with ``mu`` a list
        of [C_p, D, m] arrays and ``logml_full`` [P, D]; ``sigma`` / ``var`` are shared by the
        scenarios of a particle."""
        if len(comps) != self.P:
            raise ValueError("one list of component programs per particle")
        d, D, t_add, y_add, p_t, p_y = _appended(t_add, y_add)
        t_new = as_f64(t_new)
        m = t_new.size
        counts = np.array([len(c) for c in comps], dtype=np.int32)
        ka = KernelArray([prog for c in comps for prog in c])
        tot = int(counts.sum())
        mu, var = np.empty((tot, D, m)), np.empty((tot, m))
        sizes = (counts.astype(np.int64) * m) ** 2
        sg = np.empty(int(sizes.sum())) if want_sigma else None
        lf = np.empty((self.P, D))
        info = np.zeros(self.P, dtype=np.int32)
        _chk(load().ngp_factor_components_nowcast(
            self._h, d, p_t, D, p_y, iptr(counts), ka.arr, m, dptr(t_new) if m else None, dptr(lf),
            dptr(mu), _nullable(sg), dptr(var), iptr(info)), "ngp_factor_components_nowcast")
        return dict(**_per_particle(counts, m, mu, var, sg), logml_full=lf, info=info)

    def components_long(self, comps, t_new, t_add=None, y_add=None, want_sigma=False):
        """The decomposition over a horizon of up to ``NGP_MAX_LONG_HORIZON`` dates in one query
        (``ngp_factor_components_long``): ``components_nowcast`` in the panel form of
        ``predict_long``.  Returns a dict of per-particle lists: ``mu`` [C_p, S, m] (S = D with
        appended points, else 1), ``cross`` [C_p, C_p, m] — the covariance of two parts at the same
        date; its c = c' planes are the variances —, ``sigma`` [C_p m, C_p m] (None without
        ``want_sigma``: nothing of that size is then formed) and ``info`` [P]."""
        if len(comps) != self.P:
            raise ValueError("one list of component programs per particle")
        d, D, t_add, y_add, p_t, p_y = _appended(t_add if t_add is not None else np.zeros(0), y_add)
        t_new = as_f64(t_new)
        m = t_new.size
        counts = np.array([len(c) for c in comps], dtype=np.int32)
        ka = KernelArray([prog for c in comps for prog in c])
        tot = int(counts.sum())
        c64 = counts.astype(np.int64)
        mu = np.empty((tot, D, m))
        cr = np.empty(int((c64 ** 2).sum()) * m)
        sg = np.empty(int(((c64 * m) ** 2).sum())) if want_sigma else None
        info = np.zeros(self.P, dtype=np.int32)
        _chk(load().ngp_factor_components_long(
            self._h, d, p_t, D, p_y, iptr(counts), ka.arr, m, dptr(t_new) if m else None, dptr(mu),
            dptr(cr), _nullable(sg), iptr(info)), "ngp_factor_components_long")
        first = np.concatenate([[0], np.cumsum(c64)])
        o_cr = np.concatenate([[0], np.cumsum(c64 ** 2 * m)])
        o_sg = np.concatenate([[0], np.cumsum((c64 * m) ** 2)])
        P = self.P
        return dict(
            mu=[mu[first[p]:first[p + 1]] for p in range(P)],
            cross=[cr[o_cr[p]:o_cr[p + 1]].reshape(counts[p], counts[p], m) for p in range(P)],
            sigma=[sg[o_sg[p]:o_sg[p + 1]].reshape(counts[p] * m, counts[p] * m) for p in range(P)]
            if want_sigma else None,
            info=info)

    def predict_origins(self, cuts, t_new, noise_on_new=True):
        """The forecasts of R forecast origins in one query (``ngp_factor_predict_origins``): origin
        r knows the first ``cuts[r]`` observations (strictly increasing, 1 .. n).  Returns
        ``(mu [P, R, m], var [P, R, m], logml [P, R], info [P])``: per origin what ``predict_long``
        and ``logml`` of a factor on that prefix give, to rounding."""
        cuts = np.ascontiguousarray(cuts, dtype=np.int32).reshape(-1)
        t_new = as_f64(t_new)
        R, m = cuts.size, t_new.size
        mu = np.empty((self.P, R, m))
        var = np.empty((self.P, R, m))
        lm = np.empty((self.P, R))
        info = np.zeros(self.P, dtype=np.int32)
        _chk(load().ngp_factor_predict_origins(
            self._h, R, iptr(cuts) if R else None, m, dptr(t_new) if m else None,
            1 if noise_on_new else 0, dptr(mu), dptr(var), dptr(lm), iptr(info)),
            "ngp_factor_predict_origins")
        return mu, var, lm, info

    def predict(self, t_new, noise_on_new=True):
        r = self.nowcast(np.zeros(0), np.zeros((1, 0)), t_new, noise_on_new)
        return r["mu"][:, 0, :], r["sigma"], r["logml_full"][:, 0], r["info"]


class Context:
    """One HIP device + stream (``ngp_ctx``).  Raises if no MI355X is usable."""

    def __init__(self, device: int = 0, spec: Optional[NgpSpec] = None):
        L = load()
        h = C.c_void_p()
        st = L.ngp_ctx_create(int(device), C.byref(h))
        if st != 0:
            raise NgpError(int(st), "ngp_ctx_create (the GP hot path has no CPU fallback)")
        self._h = h
        self.device = device
        self._children = weakref.WeakSet()
        if spec is not None:
            self.set_spec(spec)

    def close(self):
        if getattr(self, "_h", None) is not None:
            for child in list(getattr(self, "_children", ())):   # jobs / factors hold ctx pointers
                child.close()
            load().ngp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- spec ---------------------------------------------------------------------------
    def set_spec(self, spec: NgpSpec):
        _chk(load().ngp_set_spec(self._h, C.byref(spec)), "ngp_set_spec")

    def get_spec(self) -> NgpSpec:
        s = NgpSpec()
        _chk(load().ngp_get_spec(self._h, C.byref(s)), "ngp_get_spec")
        return s

    # ---- one-shot entry points ---------------------------------------------------------
    def cov_batch(self, programs: Sequence, t1, t2, add_diag=False):
        ka = KernelArray(programs)
        t1, t2 = as_f64(t1), as_f64(t2)
        out = np.empty((ka.n, t1.size, t2.size))
        _chk(load().ngp_cov_batch(self._h, ka.n, ka.arr, t1.size, dptr(t1), t2.size, dptr(t2),
                                  int(add_diag), dptr(out)), "ngp_cov_batch")
        return out

    @staticmethod
    def _ymat(y, B, n):
        y = as_f64(y)
        if y.ndim == 1:
            if y.size != n:
                raise ValueError("y has the wrong length")
            return y, 0
        if y.shape != (B, n):
            raise ValueError("y must be [n] or [B, n]")
        return y, n

    def logml_batch(self, programs, t, y):
        ka = KernelArray(programs)
        t = as_f64(t)
        y, ldy = self._ymat(y, ka.n, t.size)
        out, info = np.empty(ka.n), np.zeros(ka.n, dtype=np.int32)
        _chk(load().ngp_logml_batch(self._h, ka.n, ka.arr, t.size, dptr(t), dptr(y), ldy,
                                    dptr(out), iptr(info)), "ngp_logml_batch")
        return out, info

    def predict_batch(self, programs, t, y, t_new, noise_on_new=True):
        ka = KernelArray(programs)
        t, t_new = as_f64(t), as_f64(t_new)
        y, ldy = self._ymat(y, ka.n, t.size)
        m = t_new.size
        mu, sg = np.empty((ka.n, m)), np.empty((ka.n, m, m))
        lm, info = np.empty(ka.n), np.zeros(ka.n, dtype=np.int32)
        _chk(load().ngp_predict_batch(self._h, ka.n, ka.arr, t.size, dptr(t), dptr(y), ldy, m,
                                      dptr(t_new), int(noise_on_new), dptr(mu), dptr(sg),
                                      dptr(lm), iptr(info)), "ngp_predict_batch")
        return mu, sg, lm, info

    def nowcast_batch(self, programs, t, y, t_add, y_add, t_new, noise_on_new=True):
        ka = KernelArray(programs)
        t, y, t_new = as_f64(t), as_f64(y), as_f64(t_new)
        d, D, t_add, y_add, p_t, p_y = _appended(t_add, y_add)
        m = t_new.size
        lb, lf = np.empty(ka.n), np.empty((ka.n, D))
        mu = np.empty((ka.n, D, m)) if m else None
        sg = np.empty((ka.n, m, m)) if m else None
        info = np.zeros(ka.n, dtype=np.int32)
        _chk(load().ngp_nowcast_batch(self._h, ka.n, ka.arr, t.size, dptr(t), dptr(y), d, p_t, D, p_y, m,
                                      dptr(t_new) if m else None, int(noise_on_new), dptr(lb),
                                      dptr(lf), _nullable(mu), _nullable(sg), iptr(info)),
             "ngp_nowcast_batch")
        return dict(logml_base=lb, logml_full=lf, mu=mu, sigma=sg, info=info)

    def factor(self, programs, t, y) -> Factor:
        """Factorise once, query many times (``ngp_factor_create``)."""
        ka = KernelArray(programs)
        t = as_f64(t)
        y, ldy = self._ymat(y, ka.n, t.size)
        h = C.c_void_p()
        _chk(load().ngp_factor_create(self._h, ka.n, ka.arr, t.size, dptr(t), dptr(y), ldy,
                                      C.byref(h)), "ngp_factor_create")
        return Factor(self, h, ka.n)

    def mixture_sample(self, w, mu, sigma, draws: int, seed: int, want_comp: bool = True,
                       want_info: bool = True):
        """S mixtures over the same P components, sampled on the device (``ngp_mixture_sample``):
        w [S,P], mu [P,S,m], sigma [P,m,m] -> (out [S,draws,m], comp [S,draws], info [P]);
        want_comp / want_info = False: NULL is passed for that output and None returned."""
        w, mu, sigma, sd, _, S, P, m = _mixture_args("mixture_sample", w, mu, sigma, seed, indep=False)
        out = np.empty((S, int(draws), m))
        comp = np.zeros((S, int(draws)), dtype=np.int32) if want_comp else None
        info = np.zeros(P, dtype=np.int32) if want_info else None
        _chk(load().ngp_mixture_sample(self._h, P, S, m, dptr(w), dptr(mu), dptr(sigma),
                                       int(draws), C.c_uint64(int(sd[0])), dptr(out),
                                       iptr(comp) if want_comp else None,
                                       iptr(info) if want_info else None), "ngp_mixture_sample")
        return out, comp, info

    def mixture_sample_indep(self, w, mu, sigma, draws: int, seeds, want_comp: bool = True,
                             want_info: bool = True):
        """S independent mixtures of P components each (``ngp_mixture_sample_indep``): w [S,P],
        mu [S,P,m], sigma [S,P,m,m], seeds [S] -> (out [S,draws,m], comp [S,draws], info [S,P]);
        mixture s draws what ``mixture_sample`` with S = 1 and seed = seeds[s] draws."""
        w, mu, sigma, sd, _, S, P, m = _mixture_args("mixture_sample_indep", w, mu, sigma, seeds, indep=True)
        out = np.empty((S, int(draws), m))
        comp = np.zeros((S, int(draws)), dtype=np.int32) if want_comp else None
        info = np.zeros((S, P), dtype=np.int32) if want_info else None
        _chk(load().ngp_mixture_sample_indep(self._h, P, S, m, dptr(w), dptr(mu), dptr(sigma),
                                             int(draws), sd.ctypes.data_as(_u64p), dptr(out),
                                             iptr(comp) if want_comp else None,
                                             iptr(info) if want_info else None),
             "ngp_mixture_sample_indep")
        return out, comp, info

    def mixture_path_targets(self, w, mu, sigma, draws: int, seed, inv, targets, probs,
                             want_values: bool = False):
        """Functionals of whole sample paths (``ngp_mixture_path_targets``; with ``seed`` a
        sequence of S seeds ``ngp_mixture_path_targets_indep``): w, mu, sigma as ``mixture_sample``
        / ``mixture_sample_indep``; ``inv`` = (kind, lam, offset, cap); ``targets`` a sequence of
        (kind, j0, j1, thr); ``probs`` [Q] ->  dict(q [T,Q], mean [T], count [T], hist [T,m],
        values [T,N] or None, info)."""
        w, mu, sigma, sd, indep, S, P, m = _mixture_args("mixture_path_targets", w, mu, sigma, seed)
        probs = as_f64(probs).reshape(-1)
        T, Q, N = len(targets), probs.size, S * int(draws)
        tg = (NgpPathTarget * max(T, 1))(*[NgpPathTarget(int(k), int(j0), int(j1), float(thr))
                                           for k, j0, j1, thr in targets])
        iv = _inv_transform(inv)
        q, mean = np.empty((T, Q)), np.empty(T)
        count, hist = np.zeros(T, dtype=np.int64), np.zeros((T, m), dtype=np.int64)
        values = np.empty((T, N)) if want_values else None
        info = np.zeros((S, P) if indep else P, dtype=np.int32)
        i64p = C.POINTER(C.c_int64)
        tail = (C.byref(iv), T, tg, Q, dptr(probs), dptr(q), dptr(mean), count.ctypes.data_as(i64p),
                hist.ctypes.data_as(i64p), dptr(values) if want_values else None, iptr(info))
        head = (self._h, P, S, m, dptr(w), dptr(mu), dptr(sigma), int(draws))
        if indep:
            _chk(load().ngp_mixture_path_targets_indep(*head, sd.ctypes.data_as(_u64p), *tail),
                 "ngp_mixture_path_targets_indep")
        else:
            _chk(load().ngp_mixture_path_targets(*head, C.c_uint64(int(sd[0])), *tail),
                 "ngp_mixture_path_targets")
        return dict(q=q, mean=mean, count=count, hist=hist, values=values, info=info)

    @staticmethod
    def _windows(windows, who):
        win = np.ascontiguousarray(np.asarray(windows, dtype=np.int32).reshape(-1, 2))
        if win.shape[0] < 1:
            raise ValueError(f"{who}: at least one window (j0, j1)")
        return win

    def ensemble_scores(self, x, y, windows, scale: int = 0, shift: float = 0.0, fair: bool = True):
        """Energy score per window of dates of N paths (``ngp_ensemble_scores``): x [N,m] paths on
        the original scale (path-major), y [m], windows [(j0, j1), ...] inclusive ->
        dict(es [W], term_obs [W], term_pair [W], info [W]).  A window of one date is the sample
        CRPS of that date."""
        x, y = as_f64(x), as_f64(y)
        if x.ndim != 2 or y.shape != (x.shape[1],):
            raise ValueError("ensemble_scores: x [N,m], y [m]")
        win = self._windows(windows, "ensemble_scores")
        W = win.shape[0]
        es, to, tp = np.empty(W), np.empty(W), np.empty(W)
        info = np.zeros(W, dtype=np.int32)
        _chk(load().ngp_ensemble_scores(self._h, x.shape[0], x.shape[1], dptr(x), dptr(y), int(scale),
                                        float(shift), int(bool(fair)), W, iptr(win), dptr(es), dptr(to),
                                        dptr(tp), iptr(info)), "ngp_ensemble_scores")
        return dict(es=es, term_obs=to, term_pair=tp, info=info)

    def mixture_path_scores(self, w, mu, sigma, draws: int, seed, inv, y, windows, scale: int = 0,
                            shift: float = 0.0, fair: bool = True):
        """Energy score per window of the paths the sampler draws, scored on the device without
        bringing them back (``ngp_mixture_path_scores``): w, mu, sigma, draws and ``seed`` (a
        scalar: shared components; S seeds: independent mixtures) as ``mixture_path_targets``;
        ``inv`` = (kind, lam, offset, cap); y [m] on the original scale ->
        dict(es, term_obs, term_pair, info [W], chol_info)."""
        w, mu, sigma, sd, indep, S, P, m = _mixture_args("mixture_path_scores", w, mu, sigma, seed)
        y = as_f64(y)
        if y.shape != (m,):
            raise ValueError("mixture_path_scores: y [m]")
        win = self._windows(windows, "mixture_path_scores")
        W = win.shape[0]
        iv = _inv_transform(inv)
        es, to, tp = np.empty(W), np.empty(W), np.empty(W)
        info = np.zeros(W, dtype=np.int32)
        cinfo = np.zeros((S, P) if indep else P, dtype=np.int32)
        _chk(load().ngp_mixture_path_scores(
            self._h, P, S, m, dptr(w), dptr(mu), dptr(sigma), int(indep), int(draws),
            sd.ctypes.data_as(_u64p), C.byref(iv), dptr(y), int(scale), float(shift),
            int(bool(fair)), W, iptr(win), dptr(es), dptr(to), dptr(tp), iptr(info), iptr(cinfo)),
            "ngp_mixture_path_scores")
        return dict(es=es, term_obs=to, term_pair=tp, info=info, chol_info=cinfo)

    @staticmethod
    def _marginals(w, mu, var, who):
        w, mu, var = as_f64(w), as_f64(mu), as_f64(var)
        if w.ndim != 1 or mu.ndim != 2 or mu.shape[0] != w.size or var.shape != mu.shape:
            raise ValueError(f"{who}: w [C], mu [C,m], var [C,m]")
        return w, mu, var

    def mixture_cdf(self, w, mu, var, x):
        """F_j(x) of the per-date marginals of a mixture (``ngp_mixture_cdf``): w [C], mu [C,m],
        var [C,m], x [m,K] -> (cdf [m,K], info [m])."""
        w, mu, var = self._marginals(w, mu, var, "mixture_cdf")
        C_, m = mu.shape
        x = as_f64(x)
        if x.ndim != 2 or x.shape[0] != m:
            raise ValueError("mixture_cdf: x [m,K]")
        out, info = np.empty(x.shape), np.zeros(m, dtype=np.int32)
        _chk(load().ngp_mixture_cdf(self._h, C_, m, dptr(w), dptr(mu), dptr(var), x.shape[1],
                                    dptr(x), dptr(out), iptr(info)), "ngp_mixture_cdf")
        return out, info

    def mixture_quantiles(self, w, mu, var, probs):
        """Exact quantiles per date (``ngp_mixture_quantiles``): probs [Q] in (0, 1) ->
        (q [m,Q], info [m])."""
        w, mu, var = self._marginals(w, mu, var, "mixture_quantiles")
        C_, m = mu.shape
        probs = as_f64(probs)
        if probs.ndim != 1:
            raise ValueError("mixture_quantiles: probs [Q]")
        out, info = np.empty((m, probs.size)), np.zeros(m, dtype=np.int32)
        _chk(load().ngp_mixture_quantiles(self._h, C_, m, dptr(w), dptr(mu), dptr(var), probs.size,
                                          dptr(probs), dptr(out), iptr(info)),
             "ngp_mixture_quantiles")
        return out, info

    def mixture_crps(self, w, mu, var, y):
        """Closed-form CRPS per date (``ngp_mixture_crps``): y [m] -> (crps [m], info [m])."""
        w, mu, var = self._marginals(w, mu, var, "mixture_crps")
        C_, m = mu.shape
        y = as_f64(y)
        if y.shape != (m,):
            raise ValueError("mixture_crps: y [m]")
        out, info = np.empty(m), np.zeros(m, dtype=np.int32)
        _chk(load().ngp_mixture_crps(self._h, C_, m, dptr(w), dptr(mu), dptr(var), dptr(y),
                                     dptr(out), iptr(info)), "ngp_mixture_crps")
        return out, info

    def mixture_crps_mapped(self, w, mu, var, inv, scale: int, shift: float, y, tol: float = 0.0):
        """Exact CRPS and mean after the inverse transformation, on the natural or the log scale
        (``ngp_mixture_crps_mapped``): ``inv`` = (kind, lam, offset, cap), ``scale``
        NGP_SCORE_NATURAL / NGP_SCORE_LOG, y [m] on the original scale ->
        (crps [m], mean [m], err [m], info [m])."""
        w, mu, var = self._marginals(w, mu, var, "mixture_crps_mapped")
        C_, m = mu.shape
        y = as_f64(y)
        if y.shape != (m,):
            raise ValueError("mixture_crps_mapped: y [m]")
        iv = _inv_transform(inv)
        out, mean, err = np.empty(m), np.empty(m), np.empty(m)
        info = np.zeros(m, dtype=np.int32)
        _chk(load().ngp_mixture_crps_mapped(self._h, C_, m, dptr(w), dptr(mu), dptr(var),
                                            C.byref(iv), int(scale), float(shift), dptr(y),
                                            float(tol), dptr(out), dptr(mean), dptr(err),
                                            iptr(info)), "ngp_mixture_crps_mapped")
        return out, mean, err, info

    def logml_grad_flat(self, ka: KernelArray, t, y):
        """``ngp_logml_grad_batch`` on a prepared kernel array; the gradients come back as ONE
        vector (per program: d/d params in program order, then d/d noise), no per-program split."""
        t = as_f64(t)
        y, ldy = self._ymat(y, ka.n, t.size)
        grad = np.empty(int(ka._npar.sum()) + ka.n)
        lm, info = np.empty(ka.n), np.zeros(ka.n, dtype=np.int32)
        _chk(load().ngp_logml_grad_batch(self._h, ka.n, ka.arr, t.size, dptr(t), dptr(y), ldy,
                                         dptr(lm), dptr(grad), iptr(info)),
             "ngp_logml_grad_batch")
        return lm, grad, info

    def stage_grad(self, ka: KernelArray, t, y) -> GradJob:
        """``ngp_grad_stage``: the inputs of ``logml_grad_flat`` made resident; see GradJob."""
        t = as_f64(t)
        y, ldy = self._ymat(y, ka.n, t.size)
        h = C.c_void_p()
        _chk(load().ngp_grad_stage(self._h, ka.n, ka.arr, t.size, dptr(t), dptr(y), ldy,
                                   C.byref(h)), "ngp_grad_stage")
        return GradJob(self, h, ka)

    def logml_grad_batch(self, programs, t, y):
        ka = KernelArray(programs)
        lm, grad, info = self.logml_grad_flat(ka, t, y)
        offs = np.concatenate([[0], np.cumsum(ka._npar + 1)])
        return lm, [grad[offs[i]:offs[i + 1]] for i in range(ka.n)], info

    # ---- staged ---------------------------------------------------------------------------
    def stage_logml(self, programs, t, y) -> Job:
        ka = KernelArray(programs)
        t = as_f64(t)
        y, ldy = self._ymat(y, ka.n, t.size)
        h = C.c_void_p()
        _chk(load().ngp_logml_stage(self._h, ka.n, ka.arr, t.size, dptr(t), dptr(y), ldy,
                                    C.byref(h)), "ngp_logml_stage")
        return Job(self, h, ka.n, 1, 0, (ka, t, y))

    def stage_predict(self, programs, t, y, t_new, noise_on_new=True) -> Job:
        ka = KernelArray(programs)
        t, t_new = as_f64(t), as_f64(t_new)
        y, ldy = self._ymat(y, ka.n, t.size)
        h = C.c_void_p()
        _chk(load().ngp_predict_stage(self._h, ka.n, ka.arr, t.size, dptr(t), dptr(y), ldy,
                                      t_new.size, dptr(t_new), int(noise_on_new), C.byref(h)),
             "ngp_predict_stage")
        return Job(self, h, ka.n, 1, t_new.size, (ka, t, y, t_new))

    def stage_nowcast(self, programs, t, y, t_add, y_add, t_new, noise_on_new=True) -> Job:
        ka = KernelArray(programs)
        t, y, t_add, t_new = as_f64(t), as_f64(y), as_f64(t_add), as_f64(t_new)
        d, m = t_add.size, t_new.size
        y_add = as_f64(y_add).reshape(-1, d)
        D = y_add.shape[0]
        h = C.c_void_p()
        _chk(load().ngp_nowcast_stage(self._h, ka.n, ka.arr, t.size, dptr(t), dptr(y), d,
                                      dptr(t_add), D, dptr(y_add), m,
                                      dptr(t_new) if m else None, int(noise_on_new), C.byref(h)),
             "ngp_nowcast_stage")
        return Job(self, h, ka.n, D, m, (ka, t, y, t_add, y_add, t_new))

    # ---- measurement ----------------------------------------------------------------------
    def set_combining(self, on=True):
        """Combining of concurrent one-shot callers (include/ngp.h "concurrent callers"); on by
        default.  ``on``: False / 0 off, True / 1 on, 2 on without the bounded wait for company."""
        _chk(load().ngp_set_combining(self._h, int(on)), "ngp_set_combining")

    def set_short_series_path(self, on=True):
        """Series whose main block is at most 256 points factorised in one launch (on by default;
        include/ngp.h ``ngp_set_short_series_path``); applies to jobs staged after the call."""
        _chk(load().ngp_set_short_series_path(self._h, 1 if on else 0), "ngp_set_short_series_path")

    def set_batch_invariant(self, on=True):
        """An item's outputs no longer depend (in their last bits) on the batch it travels in
        (include/ngp.h ``ngp_set_batch_invariant``); applies to jobs staged after the call."""
        _chk(load().ngp_set_batch_invariant(self._h, 1 if on else 0), "ngp_set_batch_invariant")

    def combine_stats(self, reset=False) -> dict:
        out = (C.c_int64 * 6)()
        _chk(load().ngp_combine_stats(self._h, out, 1 if reset else 0), "ngp_combine_stats")
        return dict(requests=int(out[0]), sequences=int(out[1]), largest_group=int(out[2]),
                    shared=int(out[3]), shared_k=int(out[4]))

    def set_structured_storage(self, on=True):
        """Storage option of staged value jobs (include/ngp.h): results are bit-identical either way."""
        _chk(load().ngp_set_structured_storage(self._h, int(bool(on))), "ngp_set_structured_storage")

    def profile_enable(self, on=True):
        _chk(load().ngp_profile_enable(self._h, int(bool(on))), "ngp_profile_enable")

    def profile_reset(self):
        _chk(load().ngp_profile_reset(self._h), "ngp_profile_reset")

    def profile_get(self) -> dict:
        p = NgpProfile()
        _chk(load().ngp_profile_get(self._h, C.byref(p)), "ngp_profile_get")
        return {name: dict(ms=p.ms[i], launches=int(p.launches[i]), flops=p.flops[i],
                           bytes=p.bytes[i])
                for i, name in enumerate(KERNEL_CLASSES) if p.launches[i]}

    def microbench_mfma_f64(self, iters=20000) -> float:
        v = C.c_double()
        _chk(load().ngp_microbench_mfma_f64(self._h, iters, C.byref(v)), "ngp_microbench_mfma_f64")
        return float(v.value)

    def microbench_mfma_f64_detail(self, iters=20000, blocks_per_cu=1) -> dict:
        out = np.empty(4)
        _chk(load().ngp_microbench_mfma_f64_detail(self._h, iters, blocks_per_cu, dptr(out)),
             "ngp_microbench_mfma_f64_detail")
        return dict(tflops=out[0], cycles_per_mfma=out[1], clock_ghz=out[2],
                    waves_per_simd=int(out[3]))

    def microbench_mixture_pairs(self, iters=4096) -> float:
        """CRPS pair terms per second on registers only (``ngp_microbench_mixture_pairs``)."""
        v = C.c_double()
        _chk(load().ngp_microbench_mixture_pairs(self._h, int(iters), C.byref(v)),
             "ngp_microbench_mixture_pairs")
        return float(v.value)

    def microbench_hbm(self, nbytes=1 << 30):
        w, c = C.c_double(), C.c_double()
        _chk(load().ngp_microbench_hbm(self._h, nbytes, C.byref(w), C.byref(c)),
             "ngp_microbench_hbm")
        return float(w.value), float(c.value)

    def selftest_mfma_f32_layout(self, A, B):
        """D = A[32x2] B[2x32] through one v_mfma_f32_32x32x2_f32 (mixed-precision k-loop maps)"""
        A = np.ascontiguousarray(A, dtype=np.float32).reshape(32, 2)
        B = np.ascontiguousarray(B, dtype=np.float32).reshape(2, 32)
        D = np.empty((32, 32), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        _chk(load().ngp_selftest_mfma_f32_layout(self._h, A.ctypes.data_as(fp),
                                                 B.ctypes.data_as(fp), D.ctypes.data_as(fp)),
             "ngp_selftest_mfma_f32_layout")
        return D

    def selftest_mfma_layout(self, A, B):
        """returns (D via v_mfma_f64_16x16x4, D via 4 rotated v_mfma_f64_4x4x4 + gather)"""
        A, B = as_f64(A).reshape(16, 4), as_f64(B).reshape(4, 16)
        D = np.empty((2, 16, 16))
        _chk(load().ngp_selftest_mfma_layout(self._h, dptr(A), dptr(B), dptr(D)),
             "ngp_selftest_mfma_layout")
        return D[0], D[1]


def raise_if_not_posdef(info: np.ndarray):
    bad = np.flatnonzero(np.asarray(info) != 0)
    if bad.size:
        raise PosDefException(int(info[bad[0]]), int(bad[0]))

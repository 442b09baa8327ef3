"""
Batched fixed-point solves: many parameter vectors of one model on one grid shape.

An estimation loop (SMM, MCMC, a grid search or comparative statics over γ or ψ) solves the same grid at hundreds of
parameter vectors.  ``solve_batch`` runs them as one batch: successive approximation with the reference's semantics
(code/solvers.py:19-48), one workgroup per problem with the problem's grid in the LDS of its CU, every problem stopping on
its own (csrc/batch_kernels.hpp), or, with ``algorithm="newton"``, the reference's Newton-Krylov loop
(code/solvers.py:51-95) in the same one-workgroup-per-problem form (csrc/batch_newton.hpp).  Shapes whose grid does not fit one CU run through the single-problem device solve,
problem after problem, so the call works for every shape the package supports.

    models = [SSY(γ=g) for g in np.linspace(7.5, 10.5, 256)]
    res = solve_batch(models, (10, 10, 10, 10), tol=1e-6)
    res.w[b], res.n_iter[b], res.error[b], res.status[b], res.plan
    res = solve_batch(models, (10, 10, 10, 10), algorithm="newton", inner_rtol=1e-5, inner_atol=0.0)
    res.n_apply[b]                       # applications of T plus J.v of problem b
    sim = simulate_batch(models, (10, 10, 10, 10), res.w, 4096, 1200, burn_in=16, kappa=2.0)
    sim.moments["xd"]["mean"]["mean"][b]  # cross-path mean of member b's per-path mean excess return
"""
import ctypes as C
import weakref
from collections import namedtuple

import numpy as np

from . import _lib
from . import pricing, sensitivity as sens, simulation as sim
from ._lib import lib
from ._requests import LAYOUT, _check_n_max, _path_request, _perron_left, _weights
from .discretize import discretize_gcy, discretize_ssy
from .models import GCY, SSY
from .operators import KoopmansOperator, _as_f64

ALGORITHMS = ("successive_approx", "newton")


class BatchResult(namedtuple("BatchResult", ["w", "n_iter", "error", "status", "plan"])):
    """w: (B, *shapes) host array; n_iter, error, status: length B (status 0 converged, 1 max_iter
    reached, 2 the iterate left the finite range); plan: "batch" or "loop".  The attribute ``n_apply`` (not a field
    of the tuple) holds the applications of T plus J.v per problem of a Newton solve; None for successive approximation."""

    def __new__(cls, w, n_iter, error, status, plan, n_apply=None):
        self = super().__new__(cls, w, n_iter, error, status, plan)
        self.n_apply = n_apply
        return self


def _check_algorithm(algorithm):
    if algorithm not in ALGORITHMS:
        raise ValueError(f"algorithm {algorithm!r}: the batched solve supports \"successive_approx\" and \"newton\"")

# id, ndim, nparams, narrays
_KINDS = {k: (mid, LAYOUT[k].ndim, len(LAYOUT[k].params), LAYOUT[k].narrays)
          for k, mid in (("ssy", _lib.SDFS_MODEL_SSY), ("gcy", _lib.SDFS_MODEL_GCY))}


def batch_lds_bytes(kind, shapes):
    """Dynamic LDS in bytes the batch plan needs for ``shapes`` of model ``kind`` ("ssy" / "gcy"), or None where the grid
    does not fit one CU (sdfs_batch_lds_bytes; no device call)."""
    model = _KINDS[kind][0]
    shp = (C.c_int64 * len(shapes))(*[int(s) for s in shapes])
    n = lib.sdfs_batch_lds_bytes(model, len(shapes), shp)
    if n == _lib.SDFS_ERR_UNSUPPORTED:
        return None
    if n < 0:
        raise _lib.SdfsError(f"sdfs_batch_lds_bytes failed ({n}): {lib.sdfs_batch_last_error(None).decode()}")
    return int(n)


def batch_sim_lds_bytes(kind, shapes, records=1):
    """Dynamic LDS in bytes of the batch's path kernel for ``shapes`` with the records in LDS (``records=1``) or
    gathered from global memory (``records=2``), or None where that form does not exist for the shape
    (sdfs_batch_sim_lds_bytes; no device call)."""
    model = _KINDS[kind][0]
    shp = (C.c_int64 * len(shapes))(*[int(s) for s in shapes])
    n = lib.sdfs_batch_sim_lds_bytes(model, len(shapes), shp, int(records))
    if n == _lib.SDFS_ERR_UNSUPPORTED:
        return None
    if n < 0:
        raise _lib.SdfsError(f"sdfs_batch_sim_lds_bytes failed ({n}): {lib.sdfs_batch_last_error(None).decode()}")
    return int(n)


def batch_cdf_tables(kind, shapes, arrays):
    """(cdf (B, Σ n_a²), cdf0 (B, Σ n_a)): per member the tables of ``simulation.cdf_tables``, axis after axis (the
    cumulative rows row-major), from the batch's stacked arrays (array i: (B, size)).  ValueError when a member's chain
    does not factorise.  Host only."""
    shapes = tuple(int(s) for s in shapes)
    arrays = [np.asarray(a, dtype=np.float64) for a in arrays]
    B = arrays[0].shape[0]
    cdf = np.empty((B, int(sum(n * n for n in shapes))))
    cdf0 = np.empty((B, int(sum(shapes))))
    for b in range(B):
        o = o0 = 0
        for a, (qi, n) in enumerate(zip(LAYOUT[kind].transitions, shapes)):
            Q = arrays[qi][b].reshape(-1, n, n)
            if np.max(np.abs(Q - Q[:1])) > 1e-14:
                raise ValueError(f"member {b}, axis {a}: the conditional transition tensor differs between its slices, so "
                                 "the chain does not factorise")
            c = np.cumsum(Q[0], axis=1)
            c[:, -1] = 2.0
            c0 = np.cumsum(_perron_left(Q[0]))
            c0[-1] = 2.0
            cdf[b, o:o + n * n] = c.ravel()
            cdf0[b, o0:o0 + n] = c0
            o += n * n
            o0 += n
    return cdf, cdf0


def batch_sim_tables(kind, shapes, params, arrays, cdf, cdf0=None, start=None, kappa=None, skip=None):
    """(tab (B, words), scal (B, 4), zt (B, na3)): the table blocks ``sdfs_batch_sim_paths_dev`` uploads for a request
    (per member the cumulative rows per axis, the cumulative stationary marginals, h_λ and σ_c), its scalars θ, θ ln β, γ,
    κ, and the μ_c + z table of the records kernel in the a3 layout, formed by the library's host code from the batch's
    ``params`` (B, nparams) and stacked ``arrays`` (sdfs_batch_sim_tables; no device call)."""
    model, ndim, nparams, narrays = _KINDS[kind]
    shapes = tuple(int(n) for n in shapes)
    params = _as_f64(params)
    B = int(params.shape[0])
    arrs = [_as_f64(a).reshape(B, -1) for a in arrays]
    if params.shape != (B, nparams) or len(arrs) != narrays:
        raise ValueError(f"{kind} needs params (B, {nparams}) and {narrays} arrays")
    dp = C.POINTER(C.c_double)
    d = _lib.sdfs_batch_sim_desc()
    d.n_paths, d.n_periods = 1, 2
    keep = [np.ascontiguousarray(cdf, dtype=np.float64)]
    d.cdf = keep[0].ctypes.data_as(dp)
    if start is not None:
        d.start_fixed = 1
        for a, s0 in enumerate(start):
            d.start[a] = int(s0)
    else:
        keep.append(np.ascontiguousarray(cdf0, dtype=np.float64))
        d.cdf0 = keep[-1].ctypes.data_as(dp)
    if kappa is not None:
        keep.append(np.ascontiguousarray(kappa, dtype=np.float64))
        d.has_kappa, d.kappa = 1, keep[-1].ctypes.data_as(dp)
    if skip is not None:
        keep.append(np.ascontiguousarray(skip, dtype=np.int32))
        d.skip = keep[-1].ctypes.data_as(C.POINTER(C.c_int32))
    if keep[0].shape != (B, sum(n * n for n in shapes)) or any(k.shape[0] != B for k in keep):
        raise ValueError("cdf, cdf0, kappa and skip need one row or entry per member")
    shp = (C.c_int64 * ndim)(*shapes)
    ptrs = (dp * narrays)(*[a.ctypes.data_as(dp) for a in arrs])
    sizes = (C.c_int64 * narrays)(*[a.shape[1] for a in arrs])
    args = (model, ndim, shp, B, params.ctypes.data_as(dp), ptrs, sizes, narrays, C.byref(d))
    words = lib.sdfs_batch_sim_tables(*args, None, None, None)
    if words < 0:
        raise _lib.SdfsError(f"sdfs_batch_sim_tables failed ({words}): {lib.sdfs_batch_last_error(None).decode()}")
    na3 = shapes[2] * shapes[3] if kind == "ssy" else shapes[1] * shapes[2] * shapes[4] * shapes[0]
    tab, scal, zt = np.empty((B, words)), np.empty((B, 4)), np.empty((B, na3))
    rc = lib.sdfs_batch_sim_tables(*args, tab.ctypes.data_as(dp), scal.ctypes.data_as(dp), zt.ctypes.data_as(dp))
    if rc < 0:
        raise _lib.SdfsError(f"sdfs_batch_sim_tables failed ({rc}): {lib.sdfs_batch_last_error(None).decode()}")
    return tab, scal, zt


class BatchOperator:
    """The handle of one batch as an object: B problems of one model kind on one grid shape, device-resident.
    ``params``: (B, nparams); ``arrays``: per array of the model's discretisation, its B copies stacked problem-major."""

    def __init__(self, kind, shapes, params, arrays, device=0):
        model, ndim, nparams, narrays = _KINDS[kind]
        self.kind = kind
        self.shapes = tuple(int(s) for s in shapes)
        if len(self.shapes) != ndim:
            raise ValueError(f"{kind} grids have {ndim} axes, got shapes {self.shapes}")
        self._params = _as_f64(params)
        if self._params.ndim != 2 or self._params.shape[1] != nparams:
            raise ValueError(f"params must be (B, {nparams}), got {self._params.shape}")
        self.B = int(self._params.shape[0])
        if len(arrays) != narrays:
            raise ValueError(f"{kind} needs {narrays} arrays, got {len(arrays)}")
        self._arrays = [_as_f64(a).reshape(self.B, -1) for a in arrays]
        self.device = int(device)
        self.size = int(np.prod(self.shapes))
        shp = (C.c_int64 * ndim)(*self.shapes)
        ptrs = (C.POINTER(C.c_double) * narrays)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in self._arrays])
        sizes = (C.c_int64 * narrays)(*[a.shape[1] for a in self._arrays])
        h = C.c_void_p()
        rc = lib.sdfs_batch_create(model, ndim, shp, self.B, self._params.ctypes.data_as(C.POINTER(C.c_double)), ptrs,
                                   sizes, narrays, self.device, C.byref(h))
        if rc != 0:
            raise _lib.SdfsError(f"sdfs_batch_create failed ({rc}): {lib.sdfs_batch_last_error(None).decode()}")
        self._h = h
        self._finalizer = weakref.finalize(self, lib.sdfs_batch_destroy, h)

    @classmethod
    def from_models(cls, models, shapes, method="rouwenhorst", device=0):
        """The batch of a sequence of SSY or of GCY instances, each discretised on ``shapes``."""
        models, kind = _kind_of(models)
        shapes = tuple(int(s) for s in shapes)
        disc = discretize_ssy if kind == "ssy" else discretize_gcy
        per_model = [disc(m, shapes, method) for m in models]
        arrays = [np.stack([_as_f64(a[i]).ravel() for a in per_model]) for i in range(len(per_model[0]))]
        params = np.array([m.params for m in models], dtype=np.float64)
        return cls(kind, shapes, params, arrays, device)

    @property
    def handle(self):
        return self._h

    def close(self):
        self._finalizer()

    def _check(self, rc):
        if rc != 0:
            raise _lib.SdfsError(f"libsdfs_hip error {rc}: {lib.sdfs_batch_last_error(self._h).decode()}")

    def describe_plan(self):
        buf = C.create_string_buffer(4096)
        self._check(lib.sdfs_batch_describe(self._h, buf, len(buf)))
        return buf.value.decode()

    def set_stream(self, stream_ptr, use_own=False):
        self._check(lib.sdfs_batch_set_stream(self._h, stream_ptr, int(use_own)))

    def synchronize(self):
        self._check(lib.sdfs_batch_synchronize(self._h))

    # -- device-pointer forms: B x N doubles, problem-major ---------------------------------------------------
    def apply_dev(self, w_ptr, out_ptr, resid_ptr=None):
        """out[b] = T_b(w[b]), resid[b] = max|out[b] - w[b]|; asynchronous on the handle's stream."""
        self._check(lib.sdfs_batch_apply_T_dev(self._h, w_ptr, out_ptr, resid_ptr))

    def solve_dev(self, w_ptr, tol=1e-7, max_iter=10**6, check_every=0, algorithm="successive_approx", inner_rtol=None,
                  inner_atol=None, inner_max_iter=None, **opts):
        """Every problem from the start values at ``w_ptr`` (results in place) by successive approximation, or by
        Newton-Krylov with ``algorithm="newton"`` (inner_rtol, inner_atol, inner_max_iter: None = the reference's
        1e-5, 1e-4 and 10 N; further fields of sdfs_opts as keywords).  Returns host arrays (n_iter, error, status) of
        length B; a Newton solve returns (n_iter, error, status, n_apply)."""
        _check_algorithm(algorithm)
        o = _lib.default_opts()
        o.tol, o.max_iter, o.check_every = float(tol), int(max_iter), int(check_every)
        n_iter = np.zeros(self.B, dtype=np.int64)
        err = np.zeros(self.B, dtype=np.float64)
        status = np.zeros(self.B, dtype=np.int32)
        if algorithm == "newton":
            for k, v in dict(opts, inner_rtol=inner_rtol, inner_atol=inner_atol, inner_max_iter=inner_max_iter).items():
                if v is None:
                    continue
                if not hasattr(o, k):
                    raise TypeError(f"unknown solver option {k!r}")
                setattr(o, k, type(getattr(o, k))(v))
            n_apply = np.zeros(self.B, dtype=np.int64)
            self._check(lib.sdfs_batch_newton_dev(self._h, C.byref(o), w_ptr, n_iter.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  n_apply.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  err.ctypes.data_as(C.POINTER(C.c_double)),
                                                  status.ctypes.data_as(C.POINTER(C.c_int32))))
            return n_iter, err, status, n_apply
        if opts:
            raise TypeError(f"unknown solver option {next(iter(opts))!r}")
        self._check(lib.sdfs_batch_solve_dev(self._h, C.byref(o), w_ptr, n_iter.ctypes.data_as(C.POINTER(C.c_int64)),
                                             err.ctypes.data_as(C.POINTER(C.c_double)),
                                             status.ctypes.data_as(C.POINTER(C.c_int32))))
        return n_iter, err, status

    def adjoint_words(self):
        """Doubles per problem of the moment block: s0 s1 s2 | R[ndim] | M1[n_λ] | M2[n_c] | M3[a3 table]."""
        n = lib.sdfs_batch_adjoint_words(self._h)
        if n < 0:
            self._check(int(n))
        return int(n)

    def adjoint_dev(self, w_ptr, g_ptr, g_stride, lam_ptr, moments_ptr, rtol=1e-10, atol=0.0, inner_max_iter=None,
                    check_every=0):
        """λ[b] = (I - J_b(w[b])ᵀ)⁻¹ g[b] and the adjoint moments of every problem (sdfs_batch_adjoint_dev): ``g_stride``
        0 (one grid for all) or N; ``lam_ptr`` may be None.  Returns host arrays (n_iter, n_apply, rel_resid, resid_T,
        status) of length B."""
        o = _lib.default_opts()
        o.inner_rtol, o.inner_atol, o.check_every = float(rtol), float(atol), int(check_every)
        o.inner_max_iter = 0 if inner_max_iter is None else int(inner_max_iter)
        n_iter = np.zeros(self.B, dtype=np.int64)
        n_apply = np.zeros(self.B, dtype=np.int64)
        rel = np.zeros(self.B, dtype=np.float64)
        res_T = np.zeros(self.B, dtype=np.float64)
        status = np.zeros(self.B, dtype=np.int32)
        self._check(lib.sdfs_batch_adjoint_dev(self._h, C.byref(o), w_ptr, g_ptr, int(g_stride), lam_ptr, moments_ptr,
                                               n_iter.ctypes.data_as(C.POINTER(C.c_int64)),
                                               n_apply.ctypes.data_as(C.POINTER(C.c_int64)),
                                               rel.ctypes.data_as(C.POINTER(C.c_double)),
                                               res_T.ctypes.data_as(C.POINTER(C.c_double)),
                                               status.ctypes.data_as(C.POINTER(C.c_int32))))
        return n_iter, n_apply, rel, res_T, status

    # -- host forms ------------------------------------------------------------------------------------------
    def _to_dev(self, a):
        import torch
        dev = torch.device("cuda", self.device)
        t = torch.from_numpy(a).to(dev)
        torch.cuda.current_stream(dev).synchronize()       # (the library runs on its own stream)
        return t

    def _host_in(self, w):
        w = _as_f64(w)
        if w.shape != (self.B,) + self.shapes:
            raise ValueError(f"w has shape {w.shape}, the batch is {(self.B,) + self.shapes}")
        return w

    def __call__(self, w, return_resid=False):
        """Tw[b] = T_b(w[b]); host ndarray (B, *shapes) in, new host ndarray out."""
        import torch
        wd = self._to_dev(self._host_in(w))
        out = torch.empty_like(wd)
        res = torch.empty(self.B, dtype=torch.float64, device=wd.device)
        torch.cuda.current_stream(wd.device).synchronize()
        self.apply_dev(wd.data_ptr(), out.data_ptr(), res.data_ptr())
        self.synchronize()
        Tw = out.cpu().numpy()
        return (Tw, res.cpu().numpy()) if return_resid else Tw

    def solve(self, w0, tol=1e-7, max_iter=10**6, check_every=0, algorithm="successive_approx", inner_rtol=None,
              inner_atol=None, inner_max_iter=None, **opts):
        """Host start values (B, *shapes) in; returns (w, n_iter, error, status), and n_apply behind them for
        ``algorithm="newton"`` (the keywords of solve_dev)."""
        _check_algorithm(algorithm)
        wd = self._to_dev(self._host_in(w0).copy())
        out = self.solve_dev(wd.data_ptr(), tol, max_iter, check_every, algorithm, inner_rtol, inner_atol, inner_max_iter,
                             **opts)
        return (wd.cpu().numpy(),) + tuple(out)


    def adjoint(self, w, g, rtol=1e-10, atol=0.0, inner_max_iter=None, check_every=0, return_adjoint=False):
        """Host ``w`` (B, *shapes) and ``g`` (one grid or (B, *shapes)) in; returns (moments (B, words), n_iter, n_apply,
        rel_resid, resid_T, status, λ or None)."""
        import torch
        g = _grid_or_batch(g, self.B, self.shapes, "g")
        wd = self._to_dev(self._host_in(w))
        gd = self._to_dev(g)
        mom = torch.empty((self.B, self.adjoint_words()), dtype=torch.float64, device=wd.device)
        lam = torch.empty_like(wd) if return_adjoint else None
        torch.cuda.current_stream(wd.device).synchronize()
        out = self.adjoint_dev(wd.data_ptr(), gd.data_ptr(), 0 if g.ndim == len(self.shapes) else self.size,
                               None if lam is None else lam.data_ptr(), mom.data_ptr(), rtol, atol, inner_max_iter,
                               check_every)
        return (mom.cpu().numpy(),) + tuple(out) + (None if lam is None else lam.cpu().numpy(),)

    def _stationary_weights(self):
        """(B, Σ n_a): the stationary marginals of every member's chain, axis-major (as ``pricing.stationary_weights``)."""
        rows = []
        for b in range(self.B):                            # (a batch handle's tensors are unconditional: one matrix per axis)
            rows.append(np.concatenate([_perron_left(self._arrays[qi][b].reshape(-1, n, n)[0])
                                        for qi, n in zip(LAYOUT[self.kind].transitions, self.shapes)]))
        return np.ascontiguousarray(np.stack(rows))

    def price_dev(self, w_ptr, kappa, kappa_ts, weights, n_max, EM_ptr, EM2_ptr, pd_ptr, ER_ptr, moments_ptr, horizons_ptr,
                  rtol=1e-10, atol=0.0, inner_max_iter=None, check_every=0):
        """sdfs_batch_price_dev: ``kappa`` (B,) or None, ``kappa_ts`` (B,) (read when n_max > 0), ``weights`` (B, Σ n_a) host
        arrays; the grid pointers may be None.  Returns host arrays (n_iter, n_apply, n_horizons, rel_resid, resid_T, status)
        of length B."""
        o = _lib.default_opts()
        o.inner_rtol, o.inner_atol, o.check_every = float(rtol), float(atol), int(check_every)
        o.inner_max_iter = 0 if inner_max_iter is None else int(inner_max_iter)
        dp = C.POINTER(C.c_double)
        kap = None if kappa is None else np.ascontiguousarray(kappa, dtype=np.float64)
        kts = None if kappa_ts is None else np.ascontiguousarray(kappa_ts, dtype=np.float64)
        g = np.ascontiguousarray(weights, dtype=np.float64)
        if (kap is not None and kap.shape != (self.B,)) or (kts is not None and kts.shape != (self.B,)):
            raise ValueError(f"kappa and kappa_ts need {self.B} entries")
        if g.shape != (self.B, int(sum(self.shapes))):
            raise ValueError(f"weights has shape {g.shape}: expected {(self.B, int(sum(self.shapes)))}")
        n_iter = np.zeros(self.B, dtype=np.int64)
        n_apply = np.zeros(self.B, dtype=np.int64)
        n_hor = np.zeros(self.B, dtype=np.int64)
        rel = np.zeros(self.B, dtype=np.float64)
        res_T = np.zeros(self.B, dtype=np.float64)
        status = np.zeros(self.B, dtype=np.int32)
        i64 = C.POINTER(C.c_int64)
        self._check(lib.sdfs_batch_price_dev(self._h, C.byref(o), w_ptr, None if kap is None else kap.ctypes.data_as(dp),
                                             None if kts is None else kts.ctypes.data_as(dp), g.ctypes.data_as(dp), int(n_max),
                                             EM_ptr, EM2_ptr, pd_ptr, ER_ptr, moments_ptr, horizons_ptr,
                                             n_iter.ctypes.data_as(i64), n_apply.ctypes.data_as(i64), n_hor.ctypes.data_as(i64),
                                             rel.ctypes.data_as(dp), res_T.ctypes.data_as(dp),
                                             status.ctypes.data_as(C.POINTER(C.c_int32))))
        return n_iter, n_apply, n_hor, rel, res_T, status

    def price(self, w, kappa=None, n_max=0, kappa_ts=0.0, weights=None, rtol=1e-10, atol=0.0, inner_max_iter=None,
              check_every=0, return_grids=False):
        """Host ``w`` (B, *shapes) in.  ``kappa``: None (no claim), a scalar or B entries; ``kappa_ts`` likewise (read when
        n_max > 0); ``weights``: None (every member's stationary marginals), (B, Σ n_a) or a list of B per-axis lists of
        vectors.  Returns (moments (B, 12), horizons (B, n_max, 4), grids dict or None, n_iter, n_apply, n_horizons,
        rel_resid, resid_T, status)."""
        import torch
        n_max = _check_n_max(n_max, 0)
        rtol, atol = _check_rtol(rtol, atol)
        kap = _per_member(kappa, self.B, "kappa", optional=True)
        kts = _per_member(kappa_ts, self.B, "kappa_ts")
        g = self._stationary_weights() if weights is None else _axis_weights_array(weights, self.B, self.shapes)
        wd = self._to_dev(self._host_in(w))
        dev = wd.device
        mom = torch.empty((self.B, _lib.SDFS_BATCH_PRICE_WORDS), dtype=torch.float64, device=dev)
        hz = torch.empty((self.B, n_max, 4), dtype=torch.float64, device=dev) if n_max > 0 else None
        grids = [torch.empty_like(wd) for _ in range(4)] if return_grids else [None] * 4
        torch.cuda.current_stream(dev).synchronize()
        out = self.price_dev(wd.data_ptr(), kap, kts, g, n_max, *[None if t is None else t.data_ptr() for t in grids],
                             mom.data_ptr(), None if hz is None else hz.data_ptr(), rtol, atol, inner_max_iter, check_every)
        gd = dict(zip(("E_M", "E_M2", "pd", "expected_return"), (t.cpu().numpy() for t in grids))) if return_grids else None
        return (mom.cpu().numpy(), hz.cpu().numpy() if hz is not None else np.zeros((self.B, 0, 4)), gd) + tuple(out)


    # -- simulated paths (csrc/batch_sim.hpp) -----------------------------------------------------------------
    def simulate_dev(self, w_ptr, em_ptr, pd_ptr, records_ptr, cdf, cdf0, n_paths, n_periods, *, burn_in=0, seed=0,
                     path_offset=0, start=None, kappa=None, skip=None, records=0, lookahead=0, search=0, stats_ptr=None,
                     moments_ptr=None, idx_ptr=None, series_ptr=None):
        """sdfs_batch_sim_records_dev, then sdfs_batch_sim_paths_dev, asynchronous on the handle's stream.  Device
        pointers: ``w_ptr``, ``em_ptr`` (E_x[M]) and ``pd_ptr`` (None without a claim) of B x N doubles, ``records_ptr``
        (B x N x 8, written), ``stats_ptr`` (B x (3 nser + 1) x P, may be None), ``moments_ptr`` (B x (3 nser + 1) x 3),
        ``idx_ptr`` and ``series_ptr`` (both or neither).  Host arrays: ``cdf`` (B, Σ n_a²) and ``cdf0`` (B, Σ n_a; None
        with a fixed ``start``) as ``batch_cdf_tables`` lays them out, ``kappa`` (B,) or None, ``skip`` (B,) flags or
        None.  ``records``: 0 the shape's default, 1 LDS, 2 global; ``lookahead``: 0, 1, 2 or 4."""
        dp = C.POINTER(C.c_double)
        d = _lib.sdfs_batch_sim_desc()
        d.seed, d.path_offset, d.n_paths, d.burn_in, d.n_periods = int(seed), int(path_offset), int(n_paths), int(burn_in), int(n_periods)
        d.records, d.lookahead, d.search = int(records), int(lookahead), int(search)
        keep = []

        def host(x, shape, dtype, what):
            a = np.ascontiguousarray(x, dtype=dtype)
            if a.shape != shape:
                raise ValueError(f"{what} has shape {a.shape}: expected {shape}")
            keep.append(a)
            return a
        if (pd_ptr is None) != (kappa is None):
            raise ValueError("kappa and pd_ptr go together: both None or neither")
        if kappa is not None:
            d.has_kappa = 1
            d.kappa = host(kappa, (self.B,), np.float64, "kappa").ctypes.data_as(dp)
        d.cdf = host(cdf, (self.B, int(sum(n * n for n in self.shapes))), np.float64, "cdf").ctypes.data_as(dp)
        if start is not None:
            if len(start) != len(self.shapes):
                raise ValueError(f"start needs one state index per axis ({len(self.shapes)}), got {len(start)}")
            d.start_fixed = 1
            for a, s0 in enumerate(start):
                d.start[a] = int(s0)
        else:
            if cdf0 is None:
                raise ValueError("a stationary start needs cdf0")
            d.cdf0 = host(cdf0, (self.B, int(sum(self.shapes))), np.float64, "cdf0").ctypes.data_as(dp)
        if skip is not None:
            d.skip = host(skip, (self.B,), np.int32, "skip").ctypes.data_as(C.POINTER(C.c_int32))
        self._check(lib.sdfs_batch_sim_records_dev(self._h, w_ptr, em_ptr, pd_ptr, records_ptr))
        self._check(lib.sdfs_batch_sim_paths_dev(self._h, records_ptr, C.byref(d), stats_ptr, moments_ptr, idx_ptr, series_ptr))

    def simulate(self, w, n_paths, n_periods, *, burn_in=0, seed=0, path_offset=0, start="stationary", kappa=None,
                 rtol=1e-10, records=0, return_per_path=False, return_paths=False):
        """Host ``w`` (B, *shapes) in: ``n_paths`` paths of ``n_periods`` recorded steps per member, all members on one
        seed (common random numbers).  ``kappa``: None, a scalar or B entries; the claim's price-dividend ratio comes
        from ``price_dev`` at ``rtol``.  A member with a point of w <= 1 gets status 4, one whose pricing status is not 0
        keeps that status (3: no finite price); such members run no path and their outputs are NaN.  Returns a dict:
        "series" (names), "moments" (B, 3 nser + 1, 3) = (n, mean, se) per statistic from the device reduction, "stats"
        (B, 3 nser + 1, P) or None, "index" (B, P, T+1, d) and "paths" (B, nser, P, T) or None, "status", "n_iter" and
        "rel_resid" of the claim solve."""
        import torch
        P, T, Bn, off, sd, rtol, fixed = _path_request(self.shapes, n_paths, n_periods, burn_in, seed, path_offset, start, rtol,
                                                       return_paths, members=self.B)
        if Bn + T >= (1 << 32) - 8:
            raise ValueError(f"burn_in + n_periods = {Bn + T} >= 2^32 - 8")
        records = _check_records(records)
        w = self._host_in(w)
        kap = _per_member(kappa, self.B, "kappa", optional=True)
        if records == _lib.SDFS_BATCH_SIM_LDS and batch_sim_lds_bytes(self.kind, self.shapes, 1) is None:
            raise ValueError(f"records=1: the {self.size} records of shapes {self.shapes} do not fit the LDS of one CU")
        names = sim.SERIES_KAPPA if kap is not None else sim.SERIES
        ns, nd = len(names), len(self.shapes)
        nstat = 3 * ns + 1
        bad_w = ~np.all(w.reshape(self.B, -1) > 1.0, axis=1)
        cdf, cdf0 = batch_cdf_tables(self.kind, self.shapes, self._arrays)
        want_stats = bool(return_per_path)
        need = self.B * (self.size * (sim.REC_BYTES + 24) + (nstat * P * 8 if want_stats else 0))
        if return_paths:
            need += self.B * (P * T * ns * 8 + P * (T + 1) * nd)
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > free:
            raise ValueError(f"the per-state records and outputs need {need / 2**30:.2f} GiB, {free / 2**30:.2f} GiB of "
                             "device memory is free")
        wd = self._to_dev(w)
        dev = wd.device
        em = torch.empty_like(wd)
        pd = torch.empty_like(wd) if kap is not None else None
        pmom = torch.empty((self.B, _lib.SDFS_BATCH_PRICE_WORDS), dtype=torch.float64, device=dev)
        rec = torch.empty((self.B, self.size, 8), dtype=torch.float64, device=dev)
        mom = torch.empty((self.B, nstat, 3), dtype=torch.float64, device=dev)
        stats = torch.empty((self.B, nstat, P), dtype=torch.float64, device=dev) if want_stats else None
        idx = torch.empty((self.B, P, T + 1, nd), dtype=torch.uint8, device=dev) if return_paths else None
        ser = torch.empty((self.B, ns, P, T), dtype=torch.float64, device=dev) if return_paths else None
        torch.cuda.current_stream(dev).synchronize()
        n_iter, _, _, rel, _, status = self.price_dev(wd.data_ptr(), kap, None, self._stationary_weights(), 0, em.data_ptr(), None,
                                                      None if pd is None else pd.data_ptr(), None, pmom.data_ptr(), None, rtol, 0.0)
        status = status.copy()
        status[bad_w] = _lib.SDFS_BATCH_BAD_W
        self.simulate_dev(wd.data_ptr(), em.data_ptr(), None if pd is None else pd.data_ptr(), rec.data_ptr(), cdf,
                          None if fixed is not None else cdf0, P, T, burn_in=Bn, seed=sd, path_offset=off, start=fixed, kappa=kap,
                          skip=(status != 0).astype(np.int32), records=records,
                          stats_ptr=None if stats is None else stats.data_ptr(), moments_ptr=mom.data_ptr(),
                          idx_ptr=None if idx is None else idx.data_ptr(), series_ptr=None if ser is None else ser.data_ptr())
        self.synchronize()
        return {"series": names, "moments": mom.cpu().numpy(), "stats": None if stats is None else stats.cpu().numpy(),
                "index": None if idx is None else idx.cpu().numpy(), "paths": None if ser is None else ser.cpu().numpy(),
                "status": status, "n_iter": n_iter, "rel_resid": rel}


def _grid_or_batch(x, B, shapes, what):
    x = _as_f64(x)
    if x.shape != shapes and x.shape != (B,) + shapes:
        raise ValueError(f"{what} has shape {x.shape}: expected {shapes} or {(B,) + shapes}")
    return x


def _kind_of(models):
    try:
        models = list(models)
    except TypeError:
        raise TypeError("models must be a sequence of SSY or of GCY instances") from None
    if not models:
        raise ValueError("models is empty")
    if all(isinstance(m, SSY) for m in models):
        return models, "ssy"
    if all(isinstance(m, GCY) for m in models):
        return models, "gcy"
    raise TypeError("models must be all SSY or all GCY instances")


def _batch_request(models, shapes, *w_star):
    """What every ``*_batch`` call opens with: (models as a list, kind, shapes as a tuple of ints, ndim, B, w) with the
    axes counted and, where ``w_star`` is passed, w = w_star as a float64 array of shape (B, *shapes), else None."""
    models, kind = _kind_of(models)
    shapes = tuple(int(s) for s in shapes)
    ndim = _KINDS[kind][1]
    if len(shapes) != ndim:
        raise ValueError(f"{kind} grids have {ndim} axes, got shapes {shapes}")
    B = len(models)
    if not w_star:
        return models, kind, shapes, ndim, B, None
    w = _as_f64(w_star[0])
    if w.shape != (B,) + shapes:
        raise ValueError(f"w_star has shape {w.shape}, the batch is {(B,) + shapes}")
    return models, kind, shapes, ndim, B, w


def _start_values(w0, B, shapes):
    if w0 is None:
        return np.full((B,) + shapes, 800.0)               # the reference's drivers start from 800 everywhere
    w0 = _as_f64(w0)
    if w0.shape == shapes:
        return np.ascontiguousarray(np.broadcast_to(w0, (B,) + shapes))
    if w0.shape == (B,) + shapes:
        return w0.copy()
    raise ValueError(f"w0 has shape {w0.shape}: expected {shapes} or {(B,) + shapes}")


def solve_batch(models, shapes, w0=None, tol=1e-7, max_iter=10**6, method="rouwenhorst", device=0, check_every=0,
                algorithm="successive_approx", inner_rtol=None, inner_atol=None, inner_max_iter=None):
    """Wealth-consumption ratios of ``models`` (a sequence of SSY or of GCY instances) on one grid shape by successive
    approximation, each problem stopping on its own.  ``w0``: None (800 everywhere), one grid for all, or (B, *shapes).
    ``algorithm="newton"`` runs the reference's Newton-Krylov loop instead (inner_rtol, inner_atol, inner_max_iter:
    None = its 1e-5, 1e-4 and 10 N); the result then carries ``n_apply``.  Any other name is a ValueError.
    Returns a BatchResult; ``plan`` says whether the batch kernel ran ("batch") or the single-problem device solve,
    problem after problem ("loop": the grid does not fit the LDS of one CU)."""
    _check_algorithm(algorithm)
    newton = algorithm == "newton"
    inner = dict(inner_rtol=inner_rtol, inner_atol=inner_atol, inner_max_iter=inner_max_iter) if newton else {}
    models, kind, shapes, ndim, B, _ = _batch_request(models, shapes)
    w = _start_values(w0, B, shapes)
    disc = discretize_ssy if kind == "ssy" else discretize_gcy
    if batch_lds_bytes(kind, shapes) is not None:
        op = BatchOperator.from_models(models, shapes, method, device)
        try:
            out = op.solve(w, tol, max_iter, check_every, algorithm, **inner)
        finally:
            op.close()
        return BatchResult(out[0], out[1], out[2], out[3], "batch", out[4] if newton else None)
    n_iter = np.zeros(B, dtype=np.int64)
    n_apply = np.zeros(B, dtype=np.int64) if newton else None
    err = np.zeros(B)
    status = np.zeros(B, dtype=np.int32)
    kw = {"check_every": int(check_every)} if check_every else {}
    for b, m in enumerate(models):
        T = KoopmansOperator(kind, shapes, m.params, disc(m, shapes, method), device)
        try:
            w[b], n_iter[b], info = T.solve(w[b], algorithm, tol=tol, max_iter=max_iter, **inner, **kw)
        finally:
            T.close()
        err[b] = info["final_err"]
        if newton:
            n_apply[b] = info["n_apply"]
        if info["status"] == _lib.SDFS_ERR_NUMERIC or not np.isfinite(err[b]):
            status[b] = _lib.SDFS_BATCH_NONFINITE
        else:
            status[b] = _lib.SDFS_BATCH_CONVERGED if err[b] <= tol else _lib.SDFS_BATCH_MAX_ITER
    return BatchResult(w, n_iter, err, status, "loop", n_apply)


BatchGradient = namedtuple("BatchGradient", ["grad", "names", "n_iter", "n_apply", "rel_resid", "resid_T", "status",
                                             "plan", "lam"])
BatchGradient.__doc__ = """grad: (B, P) with grad[b, k] = d<g_b, w*_b>/d names[k]; n_iter (BiCGSTAB iterations), n_apply
(operator applications), rel_resid (|r|_2 / |g|_2 of the transposed solve), resid_T (max|T w* - w*|), status (0
converged, 1 stopped above the tolerance, 2 non-finite): length B; plan: "batch" or "loop" (the counts are -1 and the
residuals NaN there: the single-problem path does not report them); lam: (B, *shapes) or None."""


def gradient_batch(models, shapes, w_star, g, rtol=1e-10, atol=0.0, persistence=True, inner_max_iter=None, check_every=0,
                   method="rouwenhorst", device=0, return_adjoint=False):
    """Gradients of φ_b = <g_b, w*_b> with respect to the parameters of every member of ``models`` at its fixed point
    ``w_star[b]`` (normally ``solve_batch(...).w``): one transposed solve λ = (I - J(w*)ᵀ)⁻¹ g and a handful of adjoint
    moments per member, one workgroup per member (csrc/batch_adjoint.hpp), then
    ``sensitivity.adjoint_moments_to_gradient`` on the host.  ``g``: one grid for all or (B, *shapes); it is ∂L/∂w of the
    caller's objective and is treated as constant.  ``persistence=True``: all 13 / 18 parameters, else the 9 / 12 that
    leave the transition matrices alone.  Shapes beyond one CU run ``wc_ratio_gradient`` member by member
    (``plan == "loop"``).  Returns a BatchGradient."""
    if method != "rouwenhorst":
        raise ValueError(f"parameter tangents are implemented for Rouwenhorst grids only, not {method!r}")
    models, kind, shapes, ndim, B, w = _batch_request(models, shapes, w_star)
    g = _grid_or_batch(g, B, shapes, "g")
    names = tuple(LAYOUT[kind].params if persistence else LAYOUT[kind].supported)
    grad = np.zeros((B, len(names)))
    if batch_lds_bytes(kind, shapes) is not None:
        op = BatchOperator.from_models(models, shapes, method, device)
        try:
            mom, n_iter, n_apply, rel, res_T, status, lam = op.adjoint(w, g, rtol, atol, inner_max_iter, check_every,
                                                                       return_adjoint)
        finally:
            op.close()
        for b, m in enumerate(models):
            d = sens.adjoint_moments_to_gradient(m, shapes, mom[b], persistence, method)
            grad[b] = [d[nm] for nm in names]
        return BatchGradient(grad, names, n_iter, n_apply, rel, res_T, status, "batch", lam)
    for b, m in enumerate(models):
        d = sens.wc_ratio_gradient(m, shapes, w[b], g if g.ndim == ndim else g[b], rtol, atol, persistence)
        grad[b] = [d[nm] for nm in names]
    return BatchGradient(grad, names, np.full(B, -1, dtype=np.int64), np.full(B, -1, dtype=np.int64), np.full(B, np.nan),
                         np.full(B, np.nan), np.zeros(B, dtype=np.int32), "loop", None)


BatchPrices = namedtuple("BatchPrices", ["stats", "moments", "price", "yield_", "bracket", "n_horizons", "grids", "n_iter",
                                         "n_apply", "rel_resid", "resid_T", "status", "plan"])
BatchPrices.__doc__ = """stats: dict of length-B arrays (``price_words_to_stats``); moments: (B, 12), the words of
sdfs_batch_price_dev; price ⟨g, P_n⟩, yield_ ⟨g, −ln P_n⟩ / n: (B, n_max); bracket: (B, n_max, 2), min and max of
P_n / P_{n−1}; n_horizons: rows written per member (later rows are NaN); grids: {"E_M", "E_M2", "pd", "expected_return"}
of (B, *shapes) or None; n_iter (BiCGSTAB iterations of the claim solve), n_apply (operator applications), rel_resid (the
true ‖K1 − v + K v‖₂ / ‖K1‖₂), resid_T (max|T w* − w*|): length B; status: 0 done, 1 the claim solve stopped above its
tolerance, 2 non-finite, 3 no finite price (r(K) ≥ 1); plan: "batch" or "loop" (the counts are −1 and the residuals NaN
there: the single-problem path does not report them)."""

PRICE_STATS = ("log_rf_mean", "log_rf_std", "max_sharpe_mean", "log_pd_mean", "log_pd_std", "log_expected_return_mean",
               "log_premium_mean", "log_premium_std", "pd_min", "pd_max")


def price_words_to_stats(moments):
    """The statistics of the (B, 12) moment words of sdfs_batch_price_dev (host only): every sum divided by Σg (word 0),
    std = √max(m2 − m1², 0)."""
    m = np.asarray(moments, dtype=np.float64)
    if m.ndim != 2 or m.shape[1] != _lib.SDFS_BATCH_PRICE_WORDS:
        raise ValueError(f"moments must be (B, {_lib.SDFS_BATCH_PRICE_WORDS}), got {m.shape}")
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = m[:, 1:9] / m[:, :1]

        def std(m1, m2):
            return np.sqrt(np.maximum(m2 - m1 * m1, 0.0))
        return {"log_rf_mean": mean[:, 0], "log_rf_std": std(mean[:, 0], mean[:, 1]), "max_sharpe_mean": mean[:, 2],
                "log_pd_mean": mean[:, 3], "log_pd_std": std(mean[:, 3], mean[:, 4]), "log_expected_return_mean": mean[:, 5],
                "log_premium_mean": mean[:, 6], "log_premium_std": std(mean[:, 6], mean[:, 7]),
                "pd_min": m[:, 9].copy(), "pd_max": m[:, 10].copy()}


def _per_member(x, B, what, optional=False):
    """A scalar or length-B sequence of finite reals as a length-B array (None stays None where ``optional``)."""
    if x is None:
        if optional:
            return None
        raise ValueError(f"{what} must be a real number or {B} of them, got None")
    try:
        a = np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a real number or {B} of them, got {x!r}") from None
    if a.ndim == 0:
        a = np.full(B, float(a))
    if a.shape != (B,):
        raise ValueError(f"{what} has shape {a.shape}: a scalar or {B} entries")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what} must be finite, got {x!r}")
    return np.ascontiguousarray(a)


def _check_rtol(rtol, atol):
    rtol, atol = float(rtol), float(atol)
    if not (rtol >= 0.0 and np.isfinite(rtol)) or not (atol >= 0.0 and np.isfinite(atol)):
        raise ValueError(f"rtol and atol must be finite and >= 0, got {rtol!r}, {atol!r}")
    return rtol, atol


def _axis_weights_array(weights, B, shapes):
    """(B, Σ n_a) from a (B, Σ n_a) array or a list of B per-axis lists of vectors."""
    total = int(sum(shapes))
    if isinstance(weights, np.ndarray) and weights.ndim == 2:
        g = _as_f64(weights)
    else:
        if len(weights) != B:
            raise ValueError(f"weights needs one per-axis list per member ({B}), got {len(weights)}")
        rows = []
        for b, per_axis in enumerate(weights):
            if len(per_axis) != len(shapes):
                raise ValueError(f"weights[{b}] needs one vector per axis ({len(shapes)}), got {len(per_axis)}")
            vs = [np.asarray(v, dtype=np.float64).ravel() for v in per_axis]
            for a, (v, n) in enumerate(zip(vs, shapes)):
                if v.size != n:
                    raise ValueError(f"weights[{b}][{a}] has {v.size} entries, axis {a} has {n} states")
            rows.append(np.concatenate(vs))
        g = np.ascontiguousarray(np.stack(rows))
    if g.shape != (B, total):
        raise ValueError(f"weights has shape {g.shape}: expected {(B, total)}")
    if not np.all(np.isfinite(g)):
        raise ValueError("weights are not finite")
    return g


def _member_weights(models, kind, shapes, weights, method):
    """The per-axis weight vectors of every member as (B, Σ n_a): None -> the stationary marginals of each member's
    chain; one per-axis list (entries as ``term_structure`` takes them: a state index or a vector) for all; or a list
    of B such lists."""
    B = len(models)
    disc = discretize_ssy if kind == "ssy" else discretize_gcy
    if weights is None:
        per = [pricing.stationary_weights(m, shapes, disc(m, shapes, method)) for m in models]
    else:
        weights = list(weights)
        nested = len(weights) == B and all(isinstance(x, (list, tuple)) for x in weights)
        if not nested:
            if len(weights) != len(shapes):
                raise ValueError(f"weights needs one entry per axis ({len(shapes)}) or one per-axis list per member ({B}), "
                                 f"got {len(weights)} entries")
            weights = [weights] * B
        per = [_weights(kind, shapes, g, m) for g, m in zip(weights, models)]
    return np.ascontiguousarray(np.stack([np.concatenate(p) for p in per])), per


def price_batch(models, shapes, w_star, kappa=None, n_max=0, kappa_ts=0.0, weights=None, rtol=1e-10, atol=0.0,
                inner_max_iter=None, check_every=0, method="rouwenhorst", device=0, return_grids=False):
    """Asset prices of every member of ``models`` at its fixed point ``w_star[b]`` (normally ``solve_batch(...).w``), one
    workgroup per member (csrc/batch_price.hpp): the risk-free rate and the maximal Sharpe ratio from E[M] and E[M²], the
    price–dividend ratio, expected return and premium of the perpetual claim on G_c^κ (``kappa``: None for no claim, a
    scalar or B entries), and prices and yields of zero-coupon claims on G_c^κ_ts for horizons 1 … ``n_max``
    (``kappa_ts``: a scalar or B entries), each averaged with product-form weights (``weights``: None for every member's
    stationary marginals, one per-axis list for all, or a list of B such lists; an entry is a state index or a vector).
    Shapes beyond one CU run ``sdf_moments``, ``claim_prices`` and ``term_structure`` member by member
    (``plan == "loop"``).  Returns a BatchPrices."""
    models, kind, shapes, ndim, B, w = _batch_request(models, shapes, w_star)
    n_max = _check_n_max(n_max, 0)
    rtol, atol = _check_rtol(rtol, atol)
    kap = _per_member(kappa, B, "kappa", optional=True)
    kts = _per_member(kappa_ts, B, "kappa_ts")
    lds = batch_lds_bytes(kind, shapes)
    g, per_axis = _member_weights(models, kind, shapes, weights, method)
    if lds is not None:
        op = BatchOperator.from_models(models, shapes, method, device)
        try:
            mom, hz, grids, n_iter, n_apply, n_hor, rel, res_T, status = op.price(
                w, kap, n_max, kts, g, rtol, atol, inner_max_iter, check_every, return_grids)
        finally:
            op.close()
        return BatchPrices(price_words_to_stats(mom), mom, hz[:, :, 0].copy(), hz[:, :, 1].copy(), hz[:, :, 2:4].copy(), n_hor,
                           grids, n_iter, n_apply, rel, res_T, status, "batch")
    if method != "rouwenhorst":
        raise ValueError(f"shapes beyond one CU are priced by the single-problem functions, which discretise by Rouwenhorst's "
                         f"method, not {method!r}")
    if rtol <= 0.0:
        raise ValueError("the single-problem claim solve needs rtol > 0")
    # member by member through the single-problem functions, reduced on the host
    mom = np.full((B, _lib.SDFS_BATCH_PRICE_WORDS), np.nan)
    hz = np.full((B, n_max, 4), np.nan)
    n_hor = np.zeros(B, dtype=np.int64)
    status = np.zeros(B, dtype=np.int32)
    names = ("E_M", "E_M2", "pd", "expected_return")
    grids = {k: np.full((B,) + shapes, np.nan) for k in names} if return_grids else None
    for b, m in enumerate(models):
        gw = per_axis[b][0]
        for v in per_axis[b][1:]:
            gw = np.multiply.outer(gw, v)
        sm = pricing.sdf_moments(m, shapes, w[b])
        E_M = sm["E_M"]
        if not np.all(np.isfinite(E_M)) or not np.all(E_M > 0):
            status[b] = _lib.SDFS_BATCH_NONFINITE
            continue
        lr = sm["log_rf"]
        mom[b, 0:4] = gw.sum(), np.sum(gw * lr), np.sum(gw * lr * lr), np.sum(gw * sm["max_sharpe"])
        if grids is not None:
            grids["E_M"][b] = E_M
            grids["E_M2"][b] = (sm["max_sharpe"] ** 2 + 1.0) * E_M ** 2
        if kap is not None:
            try:
                cp = pricing.claim_prices(m, shapes, w[b], kap[b], rtol)
            except ValueError as e:
                if "no finite price" not in str(e):
                    raise
                status[b] = _lib.SDFS_BATCH_NO_PRICE
            else:
                v, ER, lp = cp["pd"], cp["expected_return"], cp["log_premium"]
                lv, le = np.log(v), np.log(ER)
                mom[b, 4:12] = (np.sum(gw * lv), np.sum(gw * lv * lv), np.sum(gw * le), np.sum(gw * lp), np.sum(gw * lp * lp),
                                v.min(), v.max(), 0.0)
                if grids is not None:
                    grids["pd"][b], grids["expected_return"][b] = v, ER
        if n_max > 0:
            try:
                ts = pricing.term_structure(m, shapes, w[b], n_max, kts[b], per_axis[b])
            except ValueError as e:
                if "left the positive numbers" not in str(e):
                    raise
            else:
                hz[b, :, 0], hz[b, :, 1], hz[b, :, 2:4] = ts["price"], ts["yield"], ts["bracket"]
                n_hor[b] = n_max
    return BatchPrices(price_words_to_stats(mom), mom, hz[:, :, 0].copy(), hz[:, :, 1].copy(), hz[:, :, 2:4].copy(), n_hor,
                       grids, np.full(B, -1, dtype=np.int64), np.full(B, -1, dtype=np.int64), np.full(B, np.nan),
                       np.full(B, np.nan), status, "loop")


BatchSimulation = namedtuple("BatchSimulation", ["series", "moments", "per_path", "paths", "status", "price", "plan"])
BatchSimulation.__doc__ = """series: the names (dc, m, rf, rc, xc, wc, and rd, xd, pd with a claim); moments: {name: {"mean" |
"std" | "ac1": {"n", "mean", "se"}}, "slope": {"n", "mean", "se"}}, arrays of length B over a member's paths of every
per-path statistic (n: its finite values; from the device reduction on the batch plan); per_path: None, or {name: {stat:
{"values": (B, P), "median", "p05", "p95": (B,)}}, "slope": the same}; paths: None, or {"index": (B, P, T+1, d) uint8, name:
(B, P, T)}; status per member: 0 simulated, 1 the claim solve stopped above its tolerance, 2 non-finite, 3 no finite price
(r(K) >= 1), 4 a point of w* <= 1 (members with a status other than 0 ran no path: their entries are NaN, their indices 0);
price: {"n_iter", "rel_resid"} of the claim solve (-1 and NaN on the loop plan and without a claim); plan: "batch" or
"loop"."""


def _check_records(records):
    if isinstance(records, bool) or records not in (0, _lib.SDFS_BATCH_SIM_LDS, _lib.SDFS_BATCH_SIM_GLOBAL):
        raise ValueError(f"records must be 0 (the shape's default), 1 (LDS) or 2 (global memory), got {records!r}")
    return int(records)


def _sim_fields(names, mom, stats, index, paths):
    """The fields of a BatchSimulation from (B, nstat, 3) moments, (B, nstat, P) statistics or None, and the stored paths."""
    def triple(k):
        return {"n": mom[:, k, 0].copy(), "mean": mom[:, k, 1].copy(), "se": mom[:, k, 2].copy()}

    def entry(k):
        sm = [sim._summary(row) for row in stats[:, k]]
        return {"values": stats[:, k], **{q: np.array([x[q] for x in sm]) for q in ("median", "p05", "p95")}}
    return (sim._by_statistic(names, triple), None if stats is None else sim._by_statistic(names, entry),
            None if paths is None else sim._named_paths({"index": index}, names, paths))


def simulate_batch(models, shapes, w_star, n_paths, n_periods, *, burn_in=0, seed=0, path_offset=0, start="stationary",
                   kappa=None, rtol=1e-10, records=0, return_per_path=False, return_paths=False, method="rouwenhorst",
                   device=0):
    """Simulated paths of every member of ``models`` at its fixed point ``w_star[b]`` (normally ``solve_batch(...).w``):
    ``n_paths`` paths of ``n_periods`` recorded steps after ``burn_in`` per member, one lane per path on a launch grid of
    (workgroups per member, members), all members on the one ``seed`` (common random numbers, which differences of
    simulated moments across parameter vectors want), and the cross-path moments (n, mean, se) of every per-path
    statistic reduced on the device (csrc/batch_sim.hpp).  The arguments are those of ``simulate``; ``kappa``: None, a
    scalar or B entries; ``records``: where a path-step reads its state record, 0 the shape's default, 1 LDS, 2 global
    memory (both give the same bits).  ``return_per_path`` adds the (B, P) statistics, ``return_paths`` the indices and
    series (B·P·T <= 2^25).  Shapes beyond one CU run ``simulate`` member by member (``plan == "loop"``), the moments
    formed on the host.  Returns a BatchSimulation."""
    models, kind, shapes, ndim, B, w = _batch_request(models, shapes, w_star)
    P, T, Bn, off, sd, rtol, fixed = _path_request(shapes, n_paths, n_periods, burn_in, seed, path_offset, start, rtol, return_paths,
                                                   members=B)
    records = _check_records(records)
    kap = _per_member(kappa, B, "kappa", optional=True)
    names = sim.SERIES_KAPPA if kap is not None else sim.SERIES
    if batch_lds_bytes(kind, shapes) is not None:
        op = BatchOperator.from_models(models, shapes, method, device)
        try:
            r = op.simulate(w, P, T, burn_in=Bn, seed=sd, path_offset=off, start="stationary" if fixed is None else fixed, kappa=kap,
                            rtol=rtol, records=records, return_per_path=return_per_path, return_paths=return_paths)
        finally:
            op.close()
        moments, per_path, paths = _sim_fields(names, r["moments"], r["stats"] if return_per_path else None, r["index"], r["paths"])
        return BatchSimulation(names, moments, per_path, paths, r["status"], {"n_iter": r["n_iter"], "rel_resid": r["rel_resid"]},
                               "batch")
    if records == _lib.SDFS_BATCH_SIM_LDS:
        raise ValueError(f"records=1: shapes {shapes} are beyond the batch plan")
    if method != "rouwenhorst":
        raise ValueError(f"shapes beyond one CU are simulated by ``simulate``, which discretises by Rouwenhorst's method, not "
                         f"{method!r}")
    # member by member through the single-problem function, the moments formed on the host
    ns, nd = len(names), ndim
    nstat = 3 * ns + 1
    stats = np.full((B, nstat, P), np.nan)
    index = np.zeros((B, P, T + 1, nd), dtype=np.uint8) if return_paths else None
    series = np.full((B, ns, P, T), np.nan) if return_paths else None
    status = np.zeros(B, dtype=np.int32)
    for b, m in enumerate(models):
        if not np.all(w[b] > 1.0):
            status[b] = _lib.SDFS_BATCH_BAD_W
            continue
        try:
            out = sim.simulate(m, shapes, w[b], P, T, burn_in=Bn, seed=sd, path_offset=off,
                               start="stationary" if fixed is None else fixed, kappa=None if kap is None else kap[b], rtol=rtol,
                               return_paths=return_paths)
        except ValueError as e:
            if "no finite price" not in str(e):
                raise
            status[b] = _lib.SDFS_BATCH_NO_PRICE
            continue
        for i, nm in enumerate(names):
            for j, s in enumerate(sim.STATS):
                stats[b, 3 * i + j] = out["per_path"][nm][s]
            if return_paths:
                series[b, i] = out["paths"][nm]
        stats[b, 3 * ns] = out["per_path"]["slope"]
        if return_paths:
            index[b] = out["paths"]["index"]
    mom = np.full((B, nstat, 3), np.nan)
    for b in range(B):
        if status[b] != 0:
            continue
        for k in range(nstat):
            x = stats[b, k][np.isfinite(stats[b, k])]
            mom[b, k, 0] = x.size
            if x.size > 0:
                mom[b, k, 1] = x.mean()
            if x.size > 1:
                mom[b, k, 2] = x.std(ddof=1) / np.sqrt(x.size)
    moments, per_path, paths = _sim_fields(names, mom, stats if return_per_path else None, index, series)
    return BatchSimulation(names, moments, per_path, paths, status, {"n_iter": np.full(B, -1, dtype=np.int64),
                                                                     "rel_resid": np.full(B, np.nan)}, "loop")

"""
The discretised Koopmans operator T w = 1 + β (H w^θ)^(1/θ) on MI355X.

Mirrors the reference's call shapes:
  T_ssy(w, shapes, params, arrays)  -- code/ssy/discrete/ssy_wc_ratio.py:82-151
  T_gcy(w, shapes, params, arrays)  -- code/gcy/discrete/gcy_wc_ratio.py:134-238
and the closure the drivers build from them, ``T = lambda w: T_ssy(w, shapes, params, arrays)``
(ssy_wc_ratio.py:230, gcy_wc_ratio.py:333).

``KoopmansOperator`` is that closure as an object: ``T(w)`` applies the operator,
``T.jvp(w, v)`` is the directional derivative jax.jvp gives the reference
(code/solvers.py:87), and ``sdfs_via_autodiff_amd.solvers`` recognises it and runs
the whole fixed-point loop on the device instead of calling back per iteration.
All arithmetic happens in libsdfs_hip.so (hand-written HIP, gfx950); nothing here
computes on the CPU.
"""
import contextlib
import ctypes as C
import threading
import weakref
import zlib

import numpy as np

from . import _lib
from ._lib import lib, check
from ._requests import LAYOUT


def _as_f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _inner_opts(rtol, atol, max_iter):
    """Default options with the stopping rule of a linear solve."""
    o = _lib.default_opts()
    o.inner_rtol, o.inner_atol, o.inner_max_iter = float(rtol), float(atol), int(max_iter)
    return o


def _save_list(save_at, save_ptrs):
    """(count, ctypes horizons, ctypes device pointers) of the save list of a horizon loop."""
    save_at = [int(n) for n in save_at]
    if len(save_ptrs) != len(save_at):
        raise ValueError(f"{len(save_at)} save horizons but {len(save_ptrs)} save pointers")
    ns = len(save_at)
    return ns, (C.c_int64 * max(ns, 1))(*save_at), (C.c_void_p * max(ns, 1))(*[int(p) for p in save_ptrs])


# -- call tracing -----------------------------------------------------------------------------
# The reference's drivers hand the solvers a plain closure, ``T = lambda w: T_ssy(w, shapes, params,
# arrays)`` (ssy_wc_ratio.py:230, gcy_wc_ratio.py:333), and jax.jit / jax.jvp then see through it.
# Here the solvers see through it by tracing: while a trace is open every operator application
# records (operator, input object, output object), so ``solvers._resolve_operator`` can tell that a
# foreign callable *is* one device operator applied to its argument and run the loop on the device.
_trace = threading.local()


@contextlib.contextmanager
def trace_calls():
    """Collects (operator, w_in, out) of every ``KoopmansOperator.__call__`` made in this thread while
    the context is open (nested traces each see the calls made inside them)."""
    stack = getattr(_trace, "stack", None)
    if stack is None:
        stack = _trace.stack = []
    calls = []
    stack.append(calls)
    try:
        yield calls
    finally:
        stack.pop()


def _record_call(op, w_in, out):
    for calls in getattr(_trace, "stack", None) or ():
        calls.append((op, w_in, out))


class KoopmansOperator:
    """Device-resident operator for one (model, shapes, params, arrays)."""

    def __init__(self, model, shapes, params, arrays, device=0):
        self.model = {"ssy": _lib.SDFS_MODEL_SSY, "gcy": _lib.SDFS_MODEL_GCY}[model]
        self.model_name = model
        self.shapes = tuple(int(s) for s in shapes)
        self.params = tuple(float(p) for p in params)
        self._arrays = [_as_f64(a) for a in arrays]
        self.device = int(device)
        nd = len(self.shapes)
        shp = (C.c_int64 * nd)(*self.shapes)
        par = (C.c_double * len(self.params))(*self.params)
        ptrs = (C.POINTER(C.c_double) * len(self._arrays))(
            *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in self._arrays])
        sizes = (C.c_int64 * len(self._arrays))(*[a.size for a in self._arrays])
        h = C.c_void_p()
        rc = lib.sdfs_create(self.model, nd, shp, par, len(self.params), ptrs, sizes,
                             len(self._arrays), self.device, C.byref(h))
        if rc != 0:
            raise _lib.SdfsError(f"sdfs_create failed ({rc}): {_lib.last_error(None)}")
        self._h = h
        self._finalizer = weakref.finalize(self, lib.sdfs_destroy, h)
        self.size = int(lib.sdfs_grid_size(h))

    # -- handle plumbing ------------------------------------------------------
    @property
    def handle(self):
        return self._h

    def close(self):
        self._finalizer()

    def describe_plan(self):
        buf = C.create_string_buffer(16384)
        check(lib.sdfs_describe_plan(self._h, buf, len(buf)), self._h)
        return buf.value.decode()

    def _host_in(self, w, name="w"):
        w = _as_f64(w)
        if w.shape != self.shapes:
            raise ValueError(f"{name} has shape {w.shape}, operator grid is {self.shapes}")
        return w

    # -- the reference's call shapes -----------------------------------------
    def __call__(self, w):
        """Tw = T(w); host ndarray in, new host ndarray out (inputs never mutated)."""
        w_in = w
        w = self._host_in(w)
        out = np.empty_like(w)
        check(lib.sdfs_apply_T(self._h, w.ctypes.data, out.ctypes.data), self._h)
        _record_call(self, w_in, out)
        return out

    def jvp(self, w, v):
        """dT(w)[v] -- what jax.jvp(T, (w,), (v,))[1] returns in the reference."""
        w = self._host_in(w)
        v = self._host_in(v, "v")
        out = np.empty_like(w)
        check(lib.sdfs_apply_jvp(self._h, w.ctypes.data, v.ctypes.data, out.ctypes.data), self._h)
        return out

    def vjp(self, w, u):
        """dT(w)^T[u] -- what jax.vjp(T, w)[1](u) returns (the gradient path of the reference's "gd" solver).
        Unconditional transition tensors only (Rouwenhorst / Tauchen chains)."""
        w = self._host_in(w)
        u = self._host_in(u, "u")
        out = np.empty_like(w)
        check(lib.sdfs_apply_vjp(self._h, w.ctypes.data, u.ctypes.data, out.ctypes.data), self._h)
        return out

    def residual(self):
        """max|T(w) - w| of the most recent ``T(w)`` call."""
        r = C.c_double()
        check(lib.sdfs_residual(self._h, C.byref(r)), self._h)
        return r.value

    # -- device-pointer forms (torch tensors / raw pointers) ------------------
    def apply_dev(self, w_ptr, out_ptr, resid_ptr=None):
        check(lib.sdfs_apply_T_dev(self._h, w_ptr, out_ptr, resid_ptr), self._h)

    def linearize_dev(self, w_ptr, out_ptr=None):
        check(lib.sdfs_linearize_dev(self._h, w_ptr, out_ptr), self._h)

    def jvp_dev(self, v_ptr, out_ptr, minus_identity=False):
        check(lib.sdfs_apply_jvp_dev(self._h, v_ptr, out_ptr, int(minus_identity)), self._h)

    def vjp_dev(self, u_ptr, out_ptr, minus_identity=False):
        check(lib.sdfs_apply_vjp_dev(self._h, u_ptr, out_ptr, int(minus_identity)), self._h)

    def debug_jvp_storage_dev(self, krylov_f32, w_ptr, v_ptr, out_ptr, minus_identity=False):
        """Test hook (sdfs_debug_jvp_storage_dev): linearise at w and apply J once in the storage of Newton's inner solve
        for opts.krylov_f32 = ``krylov_f32``; v and out are N floats for a non-zero storage, N doubles for 0.  Afterwards
        the cached linearisation is invalid for the fp64 device forms until the next ``linearize_dev``."""
        check(lib.sdfs_debug_jvp_storage_dev(self._h, int(krylov_f32), w_ptr, v_ptr, out_ptr, int(minus_identity)), self._h)

    def _darrays(self, darrays):
        """ctypes array of the narrays host pointers of a direction (None -> NULL), sizes checked against the arrays."""
        if darrays is None:
            return None, None
        if len(darrays) != len(self._arrays):
            raise ValueError(f"darrays has {len(darrays)} entries, the operator has {len(self._arrays)} arrays")
        keep = []
        for i, (d, a) in enumerate(zip(darrays, self._arrays)):
            if d is None:
                keep.append(None)
                continue
            d = _as_f64(d)
            if d.size != a.size:
                raise ValueError(f"darrays[{i}] has {d.size} elements, arrays[{i}] has {a.size}")
            keep.append(d)
        ptrs = (C.POINTER(C.c_double) * len(keep))(
            *[d.ctypes.data_as(C.POINTER(C.c_double)) if d is not None else None for d in keep])
        return ptrs, keep

    def _dparams(self, dparams):
        dparams = tuple(float(x) for x in dparams)
        if len(dparams) != len(self.params):
            raise ValueError(f"dparams has {len(dparams)} entries, the operator has {len(self.params)} parameters")
        return (C.c_double * len(dparams))(*dparams)

    def _dgen(self, dgen):
        """ctypes array of the per-axis generator pointers (None -> NULL), each 3 n_a doubles: sub, diag, super."""
        if len(dgen) != len(self.shapes):
            raise ValueError(f"dgen has {len(dgen)} entries, the grid has {len(self.shapes)} axes")
        keep = []
        for a, (g, n) in enumerate(zip(dgen, self.shapes)):
            if g is None:
                keep.append(None)
                continue
            g = _as_f64(g)
            if g.shape != (3, n):
                raise ValueError(f"dgen[{a}] has shape {g.shape}, axis {a} needs (3, {n})")
            keep.append(g)
        ptrs = (C.POINTER(C.c_double) * len(keep))(
            *[g.ctypes.data_as(C.POINTER(C.c_double)) if g is not None else None for g in keep])
        return ptrs, keep

    def param_tangent_dev(self, w_ptr, dparams, darrays, out_ptr, Tw_ptr=None, dgen=None):
        """out = dT(w)[dparams, darrays] on device pointers (sdfs_param_tangent_dev); linearises at w.  ``dgen``: one
        entry per axis, None or the (3, n) sub-, main and super-diagonal of a left generator G with dQ = G Q
        (sdfs_param_tangent_gen_dev); the transition entries of ``darrays`` are then what the generators state and are
        not passed on."""
        dp = self._dparams(dparams)
        if dgen is None:
            ptrs, keep = self._darrays(darrays)
            check(lib.sdfs_param_tangent_dev(self._h, w_ptr, dp, ptrs, out_ptr, Tw_ptr), self._h)
        else:
            if darrays is not None:
                layout = LAYOUT.get(getattr(self, "model_name", None))
                trans = layout.transitions if layout else ()
                darrays = [None if i in trans else d for i, d in enumerate(darrays)]
            ptrs, keep = self._darrays(darrays)
            gptrs, gkeep = self._dgen(dgen)
            check(lib.sdfs_param_tangent_gen_dev(self._h, w_ptr, dp, ptrs, gptrs, out_ptr, Tw_ptr), self._h)
            del gkeep
        del keep

    def solve_linear_dev(self, rhs_ptr, x_ptr, transpose=False, rtol=1e-10, atol=0.0, max_iter=0):
        """x = (I - J)^{-1} rhs (transpose: (I - J^T)^{-1} rhs) at the cached linearisation (sdfs_solve_linear_dev).
        Returns (iterations, relative residual)."""
        it, rel = C.c_int64(), C.c_double()
        check(lib.sdfs_solve_linear_dev(self._h, int(bool(transpose)), C.byref(_inner_opts(rtol, atol, max_iter)), rhs_ptr,
                                        x_ptr, C.byref(it), C.byref(rel)), self._h)
        return it.value, rel.value

    # -- asset pricing: the tilted expectation K (pricing.py) ------------------------------------------------------
    _TILT = (lib.sdfs_set_tilt_dev, lib.sdfs_apply_tilted_dev, lib.sdfs_solve_tilted_dev)   # (``ContinuousOperator`` has its own)

    def set_tilt_dev(self, w_ptr, sdf_power, kappa_lam, kappa_c):
        """Form K = K(sdf_power, kappa_lam, kappa_c) at w (sdfs_set_tilt_dev; w_ptr may be None for sdf_power 0).  On the
        discretised operator this linearises at w and replaces the cached linearisation; the continuous one
        (sdfs_cont_set_tilt_dev) copies w and leaves the cached linearisation as it is."""
        check(self._TILT[0](self._h, w_ptr, int(sdf_power), float(kappa_lam), float(kappa_c)), self._h)

    def apply_tilted_dev(self, f_ptr, out_ptr):
        """out = K f on device pointers, two distinct grids (sdfs_apply_tilted_dev, sdfs_cont_apply_tilted_dev)."""
        check(self._TILT[1](self._h, f_ptr, out_ptr), self._h)

    def solve_tilted_dev(self, rhs_ptr, x_ptr, rtol=1e-10, atol=0.0, max_iter=0):
        """x = (I - K)^{-1} rhs (sdfs_solve_tilted_dev, sdfs_cont_solve_tilted_dev).  Returns (iterations, relative
        residual)."""
        it, rel = C.c_int64(), C.c_double()
        check(self._TILT[2](self._h, C.byref(_inner_opts(rtol, atol, max_iter)), rhs_ptr, x_ptr, C.byref(it), C.byref(rel)),
              self._h)
        return it.value, rel.value

    def tilt_tangent_dev(self, w_ptr, dw_ptr, dtw_ptr, dparams, darrays, dgen, dkappa_lam, dkappa_c, f_ptr, df_ptr, kf_ptr,
                         out_ptr):
        """out = d(K f), the tangent of the tilt last set (sdfs_tilt_tangent_dev): along (dparams, darrays, dgen) as in
        ``param_tangent_dev``, the tilt's exponents by (dkappa_lam, dkappa_c), w by dw, T w by dtw (its total movement; dw
        and dtw may be one grid) and f by df.  w_ptr: the w of the ``set_tilt_dev``; w, dw, dtw may be None for
        sdf_power 0.  f_ptr None: f = 1; df_ptr None: df = 0; kf_ptr: K f, None to have it computed."""
        dp = self._dparams(dparams)
        gptrs, gkeep = (None, None) if dgen is None else self._dgen(dgen)
        if dgen is not None and darrays is not None:       # (the transition entries are what the generators state)
            layout = LAYOUT.get(getattr(self, "model_name", None))
            trans = layout.transitions if layout else ()
            darrays = [None if i in trans else d for i, d in enumerate(darrays)]
        ptrs, keep = self._darrays(darrays)
        check(lib.sdfs_tilt_tangent_dev(self._h, w_ptr, dw_ptr, dtw_ptr, dp, ptrs, gptrs, float(dkappa_lam), float(dkappa_c),
                                        f_ptr, df_ptr, kf_ptr, out_ptr), self._h)
        del keep, gkeep

    def tilted_horizons_dev(self, n_max, weight_axes=None, save_at=(), save_ptrs=()):
        """P_n = K P_{n-1}, P_0 = 1, for n = 1 ... n_max on the device (sdfs_tilted_horizons_dev).  weight_axes: one
        host vector per axis (product-form weights; None = uniform).  P_n lands in save_ptrs[j] at n = save_at[j].
        Returns an (n_max, 4) array: <g, P_n>, <g, -log P_n> / n, min and max of P_n / P_{n-1}."""
        n_max = int(n_max)
        ns, sat, sp = _save_list(save_at, save_ptrs)
        keep, wp = [], None
        if weight_axes is not None:
            if len(weight_axes) != len(self.shapes):
                raise ValueError(f"weight_axes has {len(weight_axes)} entries, the grid has {len(self.shapes)} axes")
            for a, (g, n) in enumerate(zip(weight_axes, self.shapes)):
                g = _as_f64(g).ravel()
                if g.size != n:
                    raise ValueError(f"weight_axes[{a}] has {g.size} entries, axis {a} has {n} states")
                keep.append(g)
            wp = (C.POINTER(C.c_double) * len(keep))(*[g.ctypes.data_as(C.POINTER(C.c_double)) for g in keep])
        out = np.empty((max(n_max, 1), 4))
        check(lib.sdfs_tilted_horizons_dev(self._h, n_max, wp, ns, sat, sp,
                                           out.ctypes.data_as(C.POINTER(C.c_double))), self._h)
        del keep
        return out

    # -- simulated paths (simulation.py) -------------------------------------------------------------------------------
    def sim_records_dev(self, w_ptr, v_ptr, rec_ptr):
        """One 64-byte record per state into rec_ptr (N x 8 doubles; sdfs_sim_records_dev).  v_ptr: the claim's
        price–dividend ratio, or None.  Leaves the tilt K(1, θ, −γ) at w set."""
        check(lib.sdfs_sim_records_dev(self._h, w_ptr, v_ptr, rec_ptr), self._h)

    def sim_paths_dev(self, rec_ptr, cdf, cdf0, seed, path_offset, n_paths, burn_in, n_periods, kappa=None,
                      start=None, stats_ptr=None, idx_ptr=None, series_ptr=None, lookahead=0, search=0):
        """Paths of the chain from the records (sdfs_sim_paths_dev).  cdf: the per-axis cumulative rows, concatenated;
        cdf0: the per-axis cumulative stationary marginals (ignored with a fixed ``start``)."""
        cdf = _as_f64(cdf).ravel()
        cdf0 = _as_f64(cdf0).ravel() if cdf0 is not None else None
        d = _lib.sdfs_sim_desc()
        d.seed, d.path_offset, d.n_paths = int(seed), int(path_offset), int(n_paths)
        d.burn_in, d.n_periods = int(burn_in), int(n_periods)
        d.has_kappa = int(kappa is not None)
        d.kappa = float(kappa) if kappa is not None else 0.0
        d.start_fixed = int(start is not None)
        if start is not None:
            for a, s in enumerate(start):
                d.start[a] = int(s)
        d.lookahead, d.search = int(lookahead), int(search)
        d.cdf = cdf.ctypes.data_as(C.POINTER(C.c_double))
        d.cdf0 = cdf0.ctypes.data_as(C.POINTER(C.c_double)) if cdf0 is not None else None
        check(lib.sdfs_sim_paths_dev(self._h, rec_ptr, C.byref(d), stats_ptr, idx_ptr, series_ptr), self._h)
        del cdf, cdf0

    def _to_dev(self, *arrays):
        import torch
        dev = torch.device("cuda", self.device)
        out = [torch.from_numpy(a).to(dev) for a in arrays]
        torch.cuda.current_stream(dev).synchronize()       # (the library runs on its own stream)
        return out

    def param_tangent(self, w, dparams, darrays, dgen=None):
        """dT(w)[dparams, darrays]: the tangent of T at a fixed w along one direction of (params, arrays), host
        ndarrays in and out (``sensitivity.discretize_ssy_tangent`` / ``discretize_gcy_tangent`` make directions;
        the ``*_persistence_tangent`` twins add the generators ``dgen`` of the transition matrices)."""
        import torch
        (wd,) = self._to_dev(self._host_in(w))
        out = torch.empty_like(wd)
        self.param_tangent_dev(wd.data_ptr(), dparams, darrays, out.data_ptr(), dgen=dgen)
        self.synchronize()
        return out.cpu().numpy()

    def solve_linear(self, w, rhs, transpose=False, rtol=1e-10, atol=0.0, max_iter=0):
        """(I - J(w))^{-1} rhs, or (I - J(w)^T)^{-1} rhs with ``transpose``; host ndarrays in and out.  Raises
        SdfsError if BiCGSTAB breaks down or stops above max(rtol |rhs|_2, atol)."""
        import torch
        wd, bd = self._to_dev(self._host_in(w), self._host_in(rhs, "rhs"))
        x = torch.empty_like(wd)
        self.linearize_dev(wd.data_ptr(), x.data_ptr())
        self.solve_linear_dev(bd.data_ptr(), x.data_ptr(), transpose, rtol, atol, max_iter)
        self.synchronize()
        return x.cpu().numpy()

    def synchronize(self):
        check(lib.sdfs_synchronize(self._h), self._h)

    def set_stream(self, stream_ptr, use_own=False):
        """Launch on a caller-owned HIP stream (0 / None = the default stream, e.g.
        ``torch.cuda.current_stream().cuda_stream``); ``use_own=True`` restores the private stream."""
        check(lib.sdfs_set_stream(self._h, stream_ptr, int(use_own)), self._h)

    # -- device-resident solve --------------------------------------------------
    @staticmethod
    def _opts(algorithm, record_errors, kw):
        algo = {"successive_approx": _lib.SDFS_ALGO_SA, "newton": _lib.SDFS_ALGO_NEWTON,
                "anderson": _lib.SDFS_ALGO_ANDERSON}[algorithm]
        o = _lib.default_opts()
        if algorithm == "anderson":
            o.max_iter = 10000               # code/solvers.py:101
        for k, v in kw.items():
            if v is None:
                continue
            if not hasattr(o, k):
                raise TypeError(f"unknown solver option {k!r}")
            setattr(o, k, type(getattr(o, k))(v))
        o.record_errors = int(record_errors)
        return algo, o

    def _solve_info(self, rc, n_apply, err, record_errors):
        check(rc, self._h, allow=(_lib.SDFS_ERR_NUMERIC,))
        errors = None
        if record_errors:
            n = lib.sdfs_error_trace(self._h, None, 0)
            errors = np.empty(n)
            lib.sdfs_error_trace(self._h, errors.ctypes.data, n)
        return dict(n_apply=n_apply.value, final_err=err.value, errors=errors, status=rc)

    def solve(self, x_init, algorithm="successive_approx", record_errors=False, **kw):
        """Run the whole fixed-point iteration on the GPU.  Returns
        (x_star, n_iter, info) with info = dict(n_apply, final_err, errors, status)."""
        algo, o = self._opts(algorithm, record_errors, kw)
        x = self._host_in(x_init, "x_init").copy()
        n_iter, n_apply, err = C.c_int64(), C.c_int64(), C.c_double()
        rc = lib.sdfs_solve(self._h, algo, C.byref(o), x.ctypes.data, C.byref(n_iter),
                            C.byref(n_apply), C.byref(err))
        return x, n_iter.value, self._solve_info(rc, n_apply, err, record_errors)

    def solve_dev(self, x_ptr, algorithm="successive_approx", record_errors=False, **kw):
        """The same loop on a grid that already lives in device memory (``x_ptr``: N doubles, start value in,
        result out; sdfs_solve_dev).  Returns (n_iter, info)."""
        algo, o = self._opts(algorithm, record_errors, kw)
        n_iter, n_apply, err = C.c_int64(), C.c_int64(), C.c_double()
        rc = lib.sdfs_solve_dev(self._h, algo, C.byref(o), x_ptr, C.byref(n_iter), C.byref(n_apply), C.byref(err))
        return n_iter.value, self._solve_info(rc, n_apply, err, record_errors)

    # -- profiling counters (bench.py) -----------------------------------------
    def stream_copy_dev(self, src_ptr, dst_ptr, n):
        """dst[0:n] = src[0:n] (device doubles) by the library's streaming copy, on the handle's stream: the ceiling of a
        pass that reads and writes every grid point once (bench.py's copy_ceiling_GBps)."""
        check(lib.sdfs_stream_copy_dev(self._h, src_ptr, dst_ptr, int(n)), self._h)

    def set_profiling(self, on):
        check(lib.sdfs_set_profiling(self._h, int(on)), self._h)

    def reset_counters(self):
        check(lib.sdfs_reset_counters(self._h), self._h)

    def counters(self):
        c = _lib.sdfs_counters()
        check(lib.sdfs_get_counters(self._h, C.byref(c)), self._h)
        out = []
        for i in range(c.nkernels):
            k = c.k[i]
            out.append(dict(name=k.name.decode(), launches=k.launches, total_ms=k.total_ms,
                            alg_bytes=k.alg_bytes, alg_flops=k.alg_flops))
        return out


def ssy_operator(shapes, params, arrays, device=0):
    return KoopmansOperator("ssy", shapes, params, arrays, device)


def gcy_operator(shapes, params, arrays, device=0):
    return KoopmansOperator("gcy", shapes, params, arrays, device)


# -- functional forms with the reference's signatures ---------------------------
_cache = {}
_CACHE_MAX = 8


def _fingerprint(a):
    """Cheap content stamp of one model array: the reference's closure re-reads its arrays at every
    call, so an array changed in place between two calls must not hit the cached device copy.  Small
    arrays are hashed whole; the two big conditional tensors (25.6 MB at 20^6) by a strided sample of 4096
    entries plus the bit pattern of their sum (bits, not the value: a NaN would never compare equal and the
    operator would be rebuilt on every call).  Limit of the sample: an in-place edit outside it that leaves
    the sum's bits unchanged goes unnoticed -- build a new arrays tuple, or a KoopmansOperator, to be sure."""
    a = np.asarray(a)
    flat = a.reshape(-1)
    if flat.size <= 65536:
        return (a.shape, zlib.crc32(np.ascontiguousarray(flat).view(np.uint8)))
    step = flat.size // 4096
    return (a.shape, zlib.crc32(np.ascontiguousarray(flat[::step]).view(np.uint8)),
            np.float64(flat.sum()).tobytes())


def _cached(model, shapes, params, arrays):
    key = (model, tuple(int(s) for s in shapes), tuple(float(p) for p in params),
           tuple(id(a) for a in arrays))
    stamp = tuple(_fingerprint(a) for a in arrays)
    hit = _cache.get(key)
    # (a replaced operator is only dropped from the cache: a running solver or the caller may still hold it, its
    # weakref finalizer frees the device memory when the last reference goes)
    if hit is not None and hit._stamp != stamp:       # same objects, new contents: rebuild
        _cache.pop(key)
        hit = None
    if hit is None:
        if len(_cache) >= _CACHE_MAX:
            _cache.pop(next(iter(_cache)))
        hit = KoopmansOperator(model, shapes, params, arrays)
        hit._keepalive = list(arrays)    # the id()-based key stays valid while these live
        hit._stamp = stamp
        _cache[key] = hit
    return hit


def T_ssy(w, shapes, params, arrays):
    """Drop-in for the reference's T_ssy: one operator application on the GPU."""
    return _cached("ssy", shapes, params, arrays)(w)


def T_gcy(w, shapes, params, arrays):
    """Drop-in for the reference's T_gcy: one operator application on the GPU."""
    return _cached("gcy", shapes, params, arrays)(w)

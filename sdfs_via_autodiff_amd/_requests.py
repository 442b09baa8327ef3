"""
What the analysis functions at w* (pricing.py, sensitivity.py, simulation.py, batch.py) share before they compute: the
layout of the two models, the argument checks that touch no device, the request of the continuous-state functions as
plain steps, and the few device-side helpers (the cached operator, a grid on the device, the two stream fences).

Nothing here imports those four modules or the operators at module level; they import from here.
"""
import math
from collections import namedtuple

import numpy as np

from .discretize import discretize_ssy, discretize_gcy
from .models import SSY, GCY

# -- the model layout ----------------------------------------------------------------------------------------------------
# params: the Greek names in the order of ``model.params``; supported: those that leave the transition matrices alone;
# persistence: {name: grid axis whose Rouwenhorst matrix it moves}; narrays: the arrays of ``discretize``; transitions:
# the transition array of each axis, in grid order (the conditional tensors carry their conditioning indices in front);
# moments: (ip_beta, ip_gamma, ip_psi, ip_mu_c), (ia_hlam, ia_sigc, ia_z), (axis of h_lam, axis of h_c), the places
# `sens_tables` of csrc/sdfs_api.hip reads.  Grid axes: SSY (h_λ, h_c, h_z, z), GCY (z, z_π, h_z, h_c, h_zπ, h_λ).
Layout = namedtuple("Layout", ["kind", "ndim", "params", "supported", "persistence", "narrays", "transitions", "moments",
                               "discretize"])

SSY_PARAMS = ("β", "γ", "ψ", "μ_c", "ρ", "φ_z", "φ_c", "ρ_z", "ρ_c", "ρ_λ", "s_z", "s_c", "s_λ")
GCY_PARAMS = ("β", "ψ", "γ", "ρ_λ", "s_λ", "μ_c", "φ_c", "ρ", "ρ_π", "φ_z", "ρ_c", "s_c", "ρ_z", "s_z",
              "ρ_ππ", "φ_zπ", "ρ_zπ", "s_zπ")
LAYOUT = {
    "ssy": Layout("ssy", 4, SSY_PARAMS, ("β", "γ", "ψ", "μ_c", "φ_z", "φ_c", "s_z", "s_c", "s_λ"),
                  {"ρ": 3, "ρ_z": 2, "ρ_c": 1, "ρ_λ": 0}, 10, (1, 3, 5, 7), ((0, 1, 2, 3), (0, 8, 6), (0, 1)), discretize_ssy),
    "gcy": Layout("gcy", 6, GCY_PARAMS, ("β", "ψ", "γ", "s_λ", "μ_c", "φ_c", "ρ_π", "φ_z", "s_c", "s_z", "φ_zπ", "s_zπ"),
                  {"ρ_λ": 5, "ρ": 0, "ρ_c": 3, "ρ_z": 2, "ρ_ππ": 1, "ρ_zπ": 4}, 15, (1, 3, 5, 8, 11, 14),
                  ((0, 2, 1, 5), (13, 9, 0), (5, 3)), discretize_gcy),
}


def _kind(model):
    """The ``Layout`` of an SSY or a GCY instance."""
    if isinstance(model, SSY):
        return LAYOUT["ssy"]
    if isinstance(model, GCY):
        return LAYOUT["gcy"]
    raise TypeError(f"model must be an SSY or a GCY instance, not {type(model).__name__}")


# -- argument checks that touch no device --------------------------------------------------------------------------------
def _shapes(model, shapes):
    kind = _kind(model).kind
    shapes = tuple(int(s) for s in shapes)
    if len(shapes) != LAYOUT[kind].ndim:
        raise ValueError(f"{kind.upper()} grids have {LAYOUT[kind].ndim} axes, got shapes {shapes}")
    if any(s < 2 or s > 32 for s in shapes):
        raise ValueError(f"every axis needs 2 ... 32 states, got shapes {shapes}")
    return kind, shapes


def _check_grid(x, shapes, what):
    shp = tuple(int(s) for s in getattr(x, "shape", np.shape(x)))
    if shp != shapes:
        raise ValueError(f"{what} has shape {shp}, the grid is {shapes}")


def _kappa(kappa):
    try:
        k = float(kappa)
    except (TypeError, ValueError):
        raise ValueError(f"kappa must be a real number, got {kappa!r}") from None
    if not math.isfinite(k):
        raise ValueError(f"kappa must be finite, got {kappa!r}")
    return k


def _count(x, name, lo, hi):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi:
        raise ValueError(f"{name} must be an integer in {lo} ... {hi}, got {x!r}")
    return int(x)


def _check_n_max(n_max, lo=1):
    if isinstance(n_max, bool) or not isinstance(n_max, (int, np.integer)) or not lo <= int(n_max) <= 1 << 24:
        raise ValueError(f"n_max must be an integer in {lo} ... 2^24, got {n_max!r}")
    return int(n_max)


def _check_save(save, n_max, wrap=False):
    """The sorted distinct save horizons in 1 ... n_max.  wrap: a ValueError, not what iterating and int() raise."""
    try:
        save = sorted({int(n) for n in save})
    except (TypeError, ValueError):
        if not wrap:
            raise
        raise ValueError(f"save must be a collection of horizons, got {save!r}") from None
    for n in save:
        if not 1 <= n <= n_max:
            raise ValueError(f"save horizon {n} lies outside 1 ... n_max = {n_max}")
    return save


def _check_rtol(rtol, wrap=False):
    """rtol > 0 of a claim solve.  wrap: as in ``_check_save``, for what float() refuses."""
    try:
        r = float(rtol)
    except (TypeError, ValueError):
        if not wrap:
            raise
        raise ValueError(f"rtol must be positive, got {rtol!r}") from None
    if not (r > 0.0 and math.isfinite(r)):
        raise ValueError(f"rtol must be positive, got {rtol!r}")
    return r


def _check_tolerance(what, v, zero_ok):
    """rtol (positive) or atol (non-negative) of a linear solve."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number, got {v!r}") from None
    if not math.isfinite(f) or f < 0.0 or (f == 0.0 and not zero_ok):
        raise ValueError(f"{what} must be {'non-negative' if zero_ok else 'positive'} and finite, got {v!r}")
    return f


def _check_w_star(w_star, why="the log return needs ln(w - 1)"):
    import torch
    if isinstance(w_star, torch.Tensor):
        w_ok = bool(torch.all(w_star > 1.0))
    else:
        w_ok = bool(np.all(np.asarray(w_star, dtype=np.float64) > 1.0))
    if not w_ok:
        raise ValueError(f"w_star must exceed 1 at every grid point ({why})")


MAX_RETURNED = 1 << 25            # path-steps of returned series


def _path_request(shapes, n_paths, n_periods, burn_in, seed, path_offset, start, rtol, return_paths, members=1, check_kappa=None):
    """The checked request of ``simulate`` (and of the batch's): (P, T, B, path_offset, seed, rtol, fixed start or None)."""
    P = _count(n_paths, "n_paths", 1, 1 << 32)
    T = _count(n_periods, "n_periods", 2, (1 << 32) - 1)
    B = _count(burn_in, "burn_in", 0, (1 << 32) - 1)
    off = _count(path_offset, "path_offset", 0, (1 << 32) - 1)
    sd = _count(seed, "seed", 0, (1 << 64) - 1)
    if off + P > 1 << 32:
        raise ValueError(f"path_offset + n_paths = {off + P} > 2^32: path numbers are 32-bit")
    if B + T >= 1 << 32:
        raise ValueError(f"burn_in + n_periods = {B + T} >= 2^32: step numbers are 32-bit")
    if check_kappa is not None:       # (where ``simulate`` has always checked its kappa: after the counts)
        check_kappa()
    rtol = _check_rtol(rtol)
    if return_paths and members * P * T > MAX_RETURNED:
        what = "n_paths * n_periods" if members == 1 else "members * n_paths * n_periods"
        raise ValueError(f"return_paths: {what} = {members * P * T} > 2^25 path-steps")
    if isinstance(start, str):
        if start != "stationary":
            raise ValueError(f"start must be 'stationary' or one state index per axis, got {start!r}")
        fixed = None
    else:
        fixed = tuple(start)
        if len(fixed) != len(shapes):
            raise ValueError(f"start needs one state index per axis ({len(shapes)}), got {len(fixed)}")
        for a, (s, n) in enumerate(zip(fixed, shapes)):
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < n:
                raise ValueError(f"start[{a}] = {s!r}: a state index of axis {a} lies in 0 ... {n - 1}")
        fixed = tuple(int(s) for s in fixed)
    return P, T, B, off, sd, rtol, fixed


def _perron_left(Q):
    """The stationary distribution π Q = π, Σ π = 1 of a stochastic matrix."""
    n = Q.shape[0]
    A = np.vstack([Q.T - np.eye(n), np.ones((1, n))])
    b = np.zeros(n + 1)
    b[-1] = 1.0
    pi = np.linalg.lstsq(A, b, rcond=None)[0]
    return pi / pi.sum()


def stationary_weights(model, shapes, arrays=None):
    """Per-axis stationary marginals (host vectors, one per grid axis) of the discretised chain of (model, shapes)
    (``arrays``: the discretisation, default ``discretize_ssy`` / ``discretize_gcy`` of the model).  Their outer
    product is the stationary distribution when the chain factorises: every conditional transition tensor must be one
    matrix repeated over its conditioning indices (Rouwenhorst and Tauchen chains are); ValueError otherwise."""
    kind, shapes = _shapes(model, shapes)
    arr = LAYOUT[kind].discretize(model, shapes) if arrays is None else arrays
    out = []
    for a, (qi, n) in enumerate(zip(LAYOUT[kind].transitions, shapes)):
        Q = np.asarray(arr[qi], dtype=np.float64).reshape(-1, n, n)
        if np.max(np.abs(Q - Q[:1])) > 1e-14:
            raise ValueError(f"axis {a}: the conditional transition tensor differs between its slices, so the chain does "
                             "not factorise and has no product-form stationary distribution")
        out.append(_perron_left(Q[0]))
    return out


def _weights(kind, shapes, weights, model):
    """Product-form weights: None -> the stationary marginals; else one entry per axis, each a state index (one-hot)
    or a vector of that axis's length."""
    if weights is None:
        return stationary_weights(model, shapes)
    if len(weights) != len(shapes):
        raise ValueError(f"weights needs one entry per axis ({len(shapes)}), got {len(weights)}")
    out = []
    for a, (g, n) in enumerate(zip(weights, shapes)):
        if isinstance(g, (int, np.integer)):
            if not 0 <= int(g) < n:
                raise ValueError(f"weights[{a}] = {g}: a state index of axis {a} lies in 0 ... {n - 1}")
            v = np.zeros(n)
            v[int(g)] = 1.0
        else:
            v = np.asarray(g, dtype=np.float64).ravel()
            if v.size != n:
                raise ValueError(f"weights[{a}] has {v.size} entries, axis {a} has {n} states")
            if not np.all(np.isfinite(v)):
                raise ValueError(f"weights[{a}] is not finite")
        out.append(v)
    return out


# -- the request of the continuous-state functions ---------------------------------------------------------
# Every ``*_continuous`` function runs these steps in this order and touches no device before the last has passed:
#     kind, nd, grids, shapes = _cont_grids(model, grids, w_star)
#     ... its own checks ...
#     d = _cont_operator_or_d(model, grids, shapes, operator, d)
#     _check_w_star(w_star)
def _cont_grids(model, grids, w_star):
    """(kind, number of state variables, grids as float64 arrays, shapes), with w_star held to the grid's shape."""
    kind, nd = _kind(model)[:2]                            # (TypeError for anything but an SSY or a GCY)
    try:
        grids = tuple(np.ascontiguousarray(np.asarray(g, dtype=np.float64)) for g in grids)
    except (TypeError, ValueError):
        raise ValueError("grids must be a sequence of 1-D axis grids") from None
    if len(grids) != nd:
        raise ValueError(f"{kind.upper()} has {nd} state variables, got {len(grids)} grids")
    for a, g in enumerate(grids):
        if g.ndim != 1 or g.size < 2 or not np.all(np.isfinite(g)) or not np.all(np.diff(g) > 0):
            raise ValueError(f"grids[{a}] must be a finite increasing 1-D grid of at least 2 points")
    shapes = tuple(g.size for g in grids)
    _check_grid(w_star, shapes, "w_star")
    return kind, nd, grids, shapes


def _cont_operator_or_d(model, grids, shapes, operator, d):
    """A given operator must be a ``ContinuousOperator`` on (model, grids); without one, d is the checked order of the
    Gauss–Hermite rule.  Returns d."""
    if operator is not None:
        from .continuous import ContinuousOperator
        if not isinstance(operator, ContinuousOperator):
            raise TypeError(f"operator must be a ContinuousOperator, not {type(operator).__name__}")
        if operator.params != tuple(float(p) for p in model.params) or operator.shapes != shapes or \
                not all(np.array_equal(a, b) for a, b in zip(operator.grids, grids)):
            raise ValueError("operator was built on other parameters or grids than (model, grids)")
        return d
    d = _count(d, "d", 1, 64)
    if d ** len(grids) > 1 << 24:
        raise ValueError(f"d = {d}: the tensor rule has {d ** len(grids)} > 2^24 nodes")
    return d


def _cont_wrt(model, wrt):
    """The parameter names a continuous-state derivative is asked for: None -> all 13 / 18 (every parameter is admitted,
    the persistences included), a name, or a sequence of names.  Returns (names, all parameter names)."""
    allp = _kind(model).params                             # (TypeError for anything but an SSY or a GCY)
    if wrt is None:
        names = allp
    elif isinstance(wrt, str):
        names = (wrt,)
    else:
        try:
            names = tuple(wrt)
        except TypeError:
            raise TypeError(f"wrt must be None, a parameter name or a sequence of names, got {wrt!r}") from None
    for nm in names:
        if nm not in allp:
            raise ValueError(f"unknown {type(model).__name__} parameter {nm!r} (one of {', '.join(allp)})")
    return names, allp


def _check_finite_grid(x, shapes, what):
    """x lives on the grid and is finite everywhere."""
    import torch
    _check_grid(x, shapes, what)
    if isinstance(x, torch.Tensor):
        ok = bool(torch.all(torch.isfinite(x)))
    else:
        try:
            ok = bool(np.all(np.isfinite(np.asarray(x, dtype=np.float64))))
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be an array of real numbers") from None
    if not ok:
        raise ValueError(f"{what} must be finite at every grid point")


# -- device-side helpers -------------------------------------------------------------------------------------------------
_ops = {}
_OPS_MAX = 4


def _operator(model, shapes):
    """(operator, arrays): the device operator of (model, shapes), built once and reused; launches on torch's current
    stream so that the torch work vectors and the library's kernels are ordered."""
    import torch
    from .operators import KoopmansOperator
    L = _kind(model)
    key = (L.kind, tuple(int(s) for s in shapes), tuple(float(p) for p in model.params))
    hit = _ops.get(key)
    if hit is None:
        if len(_ops) >= _OPS_MAX:
            _ops.pop(next(iter(_ops)))
        arr = L.discretize(model, shapes)
        hit = _ops[key] = (KoopmansOperator(L.kind, shapes, model.params, arr), arr)
    op, arr = hit
    op.set_stream(torch.cuda.current_stream(torch.device("cuda", op.device)).cuda_stream)
    return op, arr


def _cont_operator(model, grids, operator, d, device):
    """The given ``ContinuousOperator``, or one built with ``qnwnorm([d] * D)``."""
    if operator is not None:
        return operator
    from .continuous import ContinuousOperator, qnwnorm
    nodes, weights = qnwnorm([d] * len(grids))
    return ContinuousOperator(np.array(model.params), grids, np.ascontiguousarray(nodes.T), weights, device=int(device))


def _device_grid(op, x, what):
    import torch
    dev = torch.device("cuda", op.device)
    if isinstance(x, torch.Tensor):
        t = x.to(device=dev, dtype=torch.float64).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).to(dev)
    if tuple(t.shape) != op.shapes:
        raise ValueError(f"{what} has shape {tuple(t.shape)}, the grid is {op.shapes}")
    return t


class _Fence:
    """``_Fence()``: the discretised operator launches on torch's current stream, nothing to order.  ``_Fence(op)``: a
    continuous one launches on its own; torch's is drained before library calls, the operator's before torch reads."""

    def __init__(self, op=None):
        self.op = op

    def before_library(self):
        if self.op is not None:
            import torch
            torch.cuda.current_stream(torch.device("cuda", self.op.device)).synchronize()

    def before_torch(self):
        if self.op is not None:
            self.op.synchronize()

"""
Parameter sensitivities of the wealth-consumption ratio w* = T(w*; p).

The reference paper closes with the fixed point that "can potentially [be differentiated] with respect to the
parameters" (comparative statics, Jacobians for estimation).  By the implicit function theorem

    forward:  dw*/dp = (I - J(w*))^{-1} dT/dp                       one linear solve per parameter
    adjoint:  d<g, w*>/dp_k = <lambda, dT/dp_k>,  lambda = (I - J(w*)^T)^{-1} g   one transposed solve for all k

with J(w*) the Jacobian of T at the fixed point and dT/dp the tangent of T at a fixed w.  Everything after the
discretisation runs in libsdfs_hip.so (``KoopmansOperator.param_tangent_dev`` / ``solve_linear_dev``); w* and the work
vectors stay on the device.

A direction is given in the reference's own terms, (dparams, darrays): ``discretize_ssy_tangent`` /
``discretize_gcy_tangent`` differentiate ``discretize_ssy`` / ``discretize_gcy`` analytically (Rouwenhorst grids are
linear in the innovation scale and the drift; sigma = phi exp(h)).  A Rouwenhorst matrix depends on the persistence
only, so every parameter but the persistences leaves the transition matrices alone; the persistence parameters (SSY ρ,
ρ_z, ρ_c, ρ_λ; GCY ρ_λ, ρ, ρ_c, ρ_z, ρ_ππ, ρ_zπ) would need expectations with a differentiated matrix and are rejected.
"""
import numpy as np

from .discretize import _rouwenhorst_grid, discretize_ssy, discretize_gcy
from .models import SSY, GCY
from .operators import KoopmansOperator

SSY_PARAMS = ("β", "γ", "ψ", "μ_c", "ρ", "φ_z", "φ_c", "ρ_z", "ρ_c", "ρ_λ", "s_z", "s_c", "s_λ")
GCY_PARAMS = ("β", "ψ", "γ", "ρ_λ", "s_λ", "μ_c", "φ_c", "ρ", "ρ_π", "φ_z", "ρ_c", "s_c", "ρ_z", "s_z",
              "ρ_ππ", "φ_zπ", "ρ_zπ", "s_zπ")
SSY_SUPPORTED = ("β", "γ", "ψ", "μ_c", "φ_z", "φ_c", "s_z", "s_c", "s_λ")
GCY_SUPPORTED = ("β", "ψ", "γ", "s_λ", "μ_c", "φ_c", "ρ_π", "φ_z", "s_c", "s_z", "φ_zπ", "s_zπ")


def _check(names, supported, name, method, model):
    if method != "rouwenhorst":
        raise ValueError(f"parameter tangents are implemented for Rouwenhorst grids only, not {method!r}")
    if name not in names:
        raise ValueError(f"unknown {model} parameter {name!r} (one of {', '.join(names)})")
    if name not in supported:
        raise ValueError(f"{model} parameter {name!r} is a persistence parameter: it moves the transition matrices, "
                         f"which the sensitivities do not differentiate (supported: {', '.join(supported)})")


def _unit_grid(n, rho):
    """d state_values / d sigma of a Rouwenhorst grid (the grid is linear in sigma and mu)."""
    return _rouwenhorst_grid(int(n), float(rho), 1.0, 0.0)


def _zeros_for_none(d, arr):
    return tuple(np.zeros_like(a) if x is None else x for x, a in zip(d, arr))


def discretize_ssy_tangent(ssy, shapes, name, method="rouwenhorst"):
    """(dparams, darrays): the derivative of (ssy.params, discretize_ssy(ssy, shapes)) with respect to the parameter
    `name` (a Greek name of ``SSY``).  ValueError for a persistence parameter or a Tauchen grid."""
    _check(SSY_PARAMS, SSY_SUPPORTED, name, method, "SSY")
    arr = discretize_ssy(ssy, shapes)
    dparams, d = _ssy_tangent(ssy, shapes, name, arr)
    return dparams, _zeros_for_none(d, arr)


def _ssy_tangent(ssy, shapes, name, arr):
    """discretize_ssy_tangent on given arrays; None stands for a zero tangent."""
    n_h_λ, n_h_c, n_h_z, n_z = (int(s) for s in shapes)
    β, γ, ψ, μ_c, ρ, φ_z, φ_c, ρ_z, ρ_c, ρ_λ, s_z, s_c, s_λ = ssy.params
    d = [None] * len(arr)
    dparams = np.zeros(len(SSY_PARAMS))
    dparams[SSY_PARAMS.index(name)] = 1.0
    h_z, σ_c, σ_z = arr[4], arr[8], arr[9]
    g_z = _unit_grid(n_z, ρ)
    dσ_z = None
    if name == "s_λ":
        d[0] = _unit_grid(n_h_λ, ρ_λ)
    elif name == "s_c":
        d[2] = _unit_grid(n_h_c, ρ_c)
        d[8] = σ_c * d[2]
    elif name == "φ_c":
        d[8] = np.exp(arr[2])
    elif name == "s_z":
        d[4] = _unit_grid(n_h_z, ρ_z)
        dσ_z = σ_z * d[4]
    elif name == "φ_z":
        dσ_z = np.exp(h_z)
    if dσ_z is not None:
        d[9] = dσ_z
        d[6] = dσ_z[:, None] * g_z[None, :]
    return dparams, d


def discretize_gcy_tangent(gcy, shapes, name, method="rouwenhorst"):
    """(dparams, darrays): the derivative of (gcy.params, discretize_gcy(gcy, shapes)) with respect to the parameter
    `name` (a Greek name of ``GCY``).  ValueError for a persistence parameter or a Tauchen grid."""
    _check(GCY_PARAMS, GCY_SUPPORTED, name, method, "GCY")
    arr = discretize_gcy(gcy, shapes)
    dparams, d = _gcy_tangent(gcy, shapes, name, arr)
    return dparams, _zeros_for_none(d, arr)


def _gcy_tangent(gcy, shapes, name, arr):
    """discretize_gcy_tangent on given arrays; None stands for a zero tangent."""
    n_z, n_z_π, n_h_z, n_h_c, n_h_zπ, n_h_λ = (int(s) for s in shapes)
    (β, ψ, γ, ρ_λ, s_λ, μ_c, φ_c, ρ, ρ_π, φ_z, ρ_c, s_c, ρ_z, s_z,
     ρ_ππ, φ_zπ, ρ_zπ, s_zπ) = gcy.params
    z_shape = arr[0].shape
    d = [None] * len(arr)
    dparams = np.zeros(len(GCY_PARAMS))
    dparams[GCY_PARAMS.index(name)] = 1.0
    z_π, h_z, σ_z, h_c, σ_c, h_zπ, σ_zπ = arr[2], arr[4], arr[6], arr[7], arr[9], arr[10], arr[12]
    g_z = _unit_grid(n_z, ρ)                   # z_states[b, c, e, a] = σ_z[c] g_z[a] + ρ_π z_π[e, b] / (1 - ρ)
    g_zπ = _unit_grid(n_z_π, ρ_ππ)             # z_π_states[e, b] = σ_zπ[e] g_zπ[b]
    dσ_z = dσ_zπ = None
    if name == "s_λ":
        d[13] = _unit_grid(n_h_λ, ρ_λ)
    elif name == "s_c":
        d[7] = _unit_grid(n_h_c, ρ_c)
        d[9] = σ_c * d[7]
    elif name == "φ_c":
        d[9] = np.exp(h_c)
    elif name == "s_z":
        d[4] = _unit_grid(n_h_z, ρ_z)
        dσ_z = σ_z * d[4]
    elif name == "φ_z":
        dσ_z = np.exp(h_z)
    elif name == "s_zπ":
        d[10] = _unit_grid(n_h_zπ, ρ_zπ)
        dσ_zπ = σ_zπ * d[10]
    elif name == "φ_zπ":
        dσ_zπ = np.exp(h_zπ)
    elif name == "ρ_π":
        d[0] = np.broadcast_to((z_π.T / (1.0 - ρ))[:, None, :, None], z_shape).copy()
    if dσ_z is not None:
        d[6] = dσ_z
        d[0] = np.broadcast_to(dσ_z[None, :, None, None] * g_z[None, None, None, :], z_shape).copy()
    if dσ_zπ is not None:
        d[12] = dσ_zπ
        d[2] = dσ_zπ[:, None] * g_zπ[None, :]
        d[0] = np.broadcast_to((ρ_π * d[2].T / (1.0 - ρ))[:, None, :, None], z_shape).copy()
    return dparams, d


# -- fixed-point sensitivities ---------------------------------------------------------------------------------------
def _kind(model):
    if isinstance(model, SSY):
        return "ssy", SSY_SUPPORTED, discretize_ssy, _ssy_tangent, SSY_PARAMS
    if isinstance(model, GCY):
        return "gcy", GCY_SUPPORTED, discretize_gcy, _gcy_tangent, GCY_PARAMS
    raise TypeError(f"model must be an SSY or a GCY instance, not {type(model).__name__}")


_ops = {}
_OPS_MAX = 4


def _operator(model, shapes):
    """The device operator of (model, shapes), built once and reused; launches on torch's current stream so that
    the torch work vectors and the library's kernels are ordered."""
    import torch
    kind, _, disc, _, _ = _kind(model)
    key = (kind, tuple(int(s) for s in shapes), tuple(float(p) for p in model.params))
    hit = _ops.get(key)
    if hit is None:
        if len(_ops) >= _OPS_MAX:
            _ops.pop(next(iter(_ops)))
        arr = disc(model, shapes)
        hit = _ops[key] = (KoopmansOperator(kind, shapes, model.params, arr), arr)
    op, arr = hit
    op.set_stream(torch.cuda.current_stream(torch.device("cuda", op.device)).cuda_stream)
    return op, arr


def _directions(model, shapes, names, arr):
    kind, supported, _, tangent, allp = _kind(model)
    for nm in names:
        _check(allp, supported, nm, "rouwenhorst", kind.upper())
    return [tangent(model, shapes, nm, arr) for nm in names]


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


def wc_ratio_sensitivities(model, shapes, w_star, wrt=None, rtol=1e-10, atol=0.0):
    """{name: dw*/dp_name} (host arrays of the grid's shape) at a converged fixed point ``w_star`` of
    (model, shapes): one tangent of T and one BiCGSTAB solve of (I - J(w*)) x = dT/dp per parameter.  ``wrt``: the
    Greek parameter names (default: every supported one).  rtol / atol: the solve's stopping rule on |r|_2."""
    import torch
    _, supported, _, _, allp = _kind(model)
    names = supported if wrt is None else tuple([wrt] if isinstance(wrt, str) else wrt)
    for nm in names:                                               # (ValueError before any device work)
        _check(allp, supported, nm, "rouwenhorst", type(model).__name__)
    op, arr = _operator(model, shapes)
    dirs = _directions(model, shapes, names, arr)
    w = _device_grid(op, w_star, "w_star")
    rhs, x, tw = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)
    out = {}
    for nm, (dp, da) in zip(names, dirs):
        op.param_tangent_dev(w.data_ptr(), dp, da, rhs.data_ptr(), tw.data_ptr())
        op.solve_linear_dev(rhs.data_ptr(), x.data_ptr(), False, rtol, atol)
        out[nm] = x.cpu().numpy()
    return out


def wc_ratio_gradient(model, shapes, w_star, g, rtol=1e-10, atol=0.0):
    """{name: d<g, w*>/dp_name} for every supported parameter at a converged ``w_star``: one transposed solve
    lambda = (I - J(w*)^T)^{-1} g, then <lambda, dT/dp_k> per parameter (a tangent of T each, no further solve)."""
    import torch
    _, supported, _, _, _ = _kind(model)
    op, arr = _operator(model, shapes)
    dirs = _directions(model, shapes, supported, arr)
    w = _device_grid(op, w_star, "w_star")
    gd = _device_grid(op, g, "g")
    lam, rhs, tw = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)
    op.linearize_dev(w.data_ptr(), tw.data_ptr())
    op.solve_linear_dev(gd.data_ptr(), lam.data_ptr(), True, rtol, atol)
    lv = lam.view(-1)
    out = {}
    for nm, (dp, da) in zip(supported, dirs):
        op.param_tangent_dev(w.data_ptr(), dp, da, rhs.data_ptr(), tw.data_ptr())
        out[nm] = float(torch.dot(lv, rhs.view(-1)))
    return out

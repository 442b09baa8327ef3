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
only, so every parameter but the persistences leaves the transition matrices alone, and those two functions refuse
the persistence parameters (SSY ρ, ρ_z, ρ_c, ρ_λ; GCY ρ_λ, ρ, ρ_c, ρ_z, ρ_ππ, ρ_zπ).

The persistences are differentiated by ``discretize_ssy_persistence_tangent`` / ``discretize_gcy_persistence_tangent``.
The Rouwenhorst matrix is Θ_n(ρ) = exp(-½ ln ρ · L_n) with L_n the Ehrenfest generator (L[i, i-1] = i, L[i, i+1] =
n-1-i, L[i, i] = -(n-1)), hence dΘ_n/dρ = G_n Θ_n = Θ_n G_n with the tridiagonal G_n = -L_n / (2ρ)
(``rouwenhorst_generator``).  The library takes the direction of a matrix as that generator (``dgen``) and turns it
into a three-point stencil along the axis on a field the linearising pass already produces; the persistence also moves
its own grid (ψ ∝ 1/√(1-ρ²)) and the drift μ/(1-ρ), which are ordinary state-array tangents.  ``persistence=True``
opens them to ``wc_ratio_sensitivities`` / ``wc_ratio_gradient``.
"""
import numpy as np

from .discretize import _rouwenhorst_grid, discretize_ssy, discretize_gcy
from ._requests import (LAYOUT, SSY_PARAMS, GCY_PARAMS, _kind, _operator, _device_grid, _cont_grids, _cont_operator_or_d,
                        _cont_operator, _cont_wrt, _check_finite_grid, _check_w_star, _check_tolerance, _Fence)

SSY_SUPPORTED, GCY_SUPPORTED = LAYOUT["ssy"].supported, LAYOUT["gcy"].supported
SSY_PERSISTENCE, GCY_PERSISTENCE = tuple(LAYOUT["ssy"].persistence), tuple(LAYOUT["gcy"].persistence)


def _check(names, supported, name, method, model):
    if method != "rouwenhorst":
        raise ValueError(f"parameter tangents are implemented for Rouwenhorst grids only, not {method!r}")
    if name not in names:
        raise ValueError(f"unknown {model} parameter {name!r} (one of {', '.join(names)})")
    if name not in supported:
        raise ValueError(f"{model} parameter {name!r} is a persistence parameter: it moves the transition matrices, "
                         f"which the sensitivities differentiate only with persistence=True (the "
                         f"discretize_*_persistence_tangent functions; supported here: {', '.join(supported)})")


def _check_persistence(names, persistence, name, method, model):
    if method != "rouwenhorst":
        raise ValueError(f"parameter tangents are implemented for Rouwenhorst grids only, not {method!r}")
    if name not in names:
        raise ValueError(f"unknown {model} parameter {name!r} (one of {', '.join(names)})")
    if name not in persistence:
        raise ValueError(f"{model} parameter {name!r} is not a persistence parameter "
                         f"(one of {', '.join(persistence)}); use discretize_{model.lower()}_tangent")


def rouwenhorst_generator(n, rho):
    """(3, n): the sub-, main and super-diagonal, by row, of the tridiagonal G_n with dΘ_n/dρ = G_n Θ_n = Θ_n G_n for
    the Rouwenhorst matrix Θ_n(ρ) (p = q = (1 + ρ) / 2):  G_n[i, i-1] = -i / (2ρ), G_n[i, i] = (n-1) / (2ρ),
    G_n[i, i+1] = -(n-1-i) / (2ρ).  (sub[0] and super[n-1] lie outside the matrix and are zero.)"""
    n, rho = int(n), float(rho)
    if n < 2:
        raise ValueError("rouwenhorst_generator: n must be >= 2")
    if rho == 0.0 or not abs(rho) < 1.0:
        raise ValueError(f"rouwenhorst_generator: rho = {rho!r} must satisfy 0 < |rho| < 1 "
                         "(the generator is -L / (2 rho))")
    i = np.arange(n, dtype=np.float64)
    return np.stack([-i, np.full(n, n - 1.0), -(n - 1.0 - i)]) / (2.0 * rho)


def _apply_generator(gen, Q):
    """G Q over the last two axes of Q (every slice), G given by its three diagonals."""
    out = gen[1][:, None] * Q
    out[..., 1:, :] += gen[0][1:, None] * Q[..., :-1, :]
    out[..., :-1, :] += gen[2][:-1, None] * Q[..., 1:, :]
    return out


def _grid_drho(rho):
    """d ln(centred Rouwenhorst grid) / d rho: the grid scales with 1 / sqrt(1 - rho^2)."""
    return rho / (1.0 - rho * rho)


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


def discretize_ssy_persistence_tangent(ssy, shapes, name, method="rouwenhorst"):
    """(dparams, darrays, dgen): the derivative of (ssy.params, discretize_ssy(ssy, shapes)) with respect to the
    persistence parameter `name`.  ``darrays`` is the true derivative of every array, transition arrays included
    (dQ = G Q in every slice); ``dgen`` has one entry per grid axis, None or the (3, n) ``rouwenhorst_generator`` of the
    axis the parameter moves.  ValueError for any other parameter or a Tauchen grid."""
    _check_persistence(SSY_PARAMS, SSY_PERSISTENCE, name, method, "SSY")
    arr = discretize_ssy(ssy, shapes)
    dparams, d, dgen = _ssy_persistence(ssy, shapes, name, arr)
    ax = LAYOUT["ssy"].persistence[name]
    qi = LAYOUT["ssy"].transitions[ax]
    d[qi] = _apply_generator(dgen[ax], arr[qi])
    return dparams, _zeros_for_none(d, arr), dgen


def _ssy_persistence(ssy, shapes, name, arr):
    """(dparams, state-array tangents with None for zero and for the transition arrays, dgen)."""
    n_h_λ, n_h_c, n_h_z, n_z = (int(s) for s in shapes)
    β, γ, ψ, μ_c, ρ, φ_z, φ_c, ρ_z, ρ_c, ρ_λ, s_z, s_c, s_λ = ssy.params
    d = [None] * len(arr)
    dparams = np.zeros(len(SSY_PARAMS))
    dparams[SSY_PARAMS.index(name)] = 1.0
    dgen = [None] * 4
    ax = LAYOUT["ssy"].persistence[name]
    if name == "ρ_λ":
        d[0] = arr[0] * _grid_drho(ρ_λ)
        dgen[ax] = rouwenhorst_generator(n_h_λ, ρ_λ)
    elif name == "ρ_c":
        d[2] = arr[2] * _grid_drho(ρ_c)
        d[8] = arr[8] * d[2]
        dgen[ax] = rouwenhorst_generator(n_h_c, ρ_c)
    elif name == "ρ_z":                                  # h_z -> σ_z -> z
        d[4] = arr[4] * _grid_drho(ρ_z)
        d[9] = arr[9] * d[4]
        d[6] = d[9][:, None] * _unit_grid(n_z, ρ)[None, :]
        dgen[ax] = rouwenhorst_generator(n_h_z, ρ_z)
    else:                                                # ρ: the z grids (zero drift)
        d[6] = arr[6] * _grid_drho(ρ)
        dgen[ax] = rouwenhorst_generator(n_z, ρ)
    return dparams, d, dgen


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


def discretize_gcy_persistence_tangent(gcy, shapes, name, method="rouwenhorst"):
    """(dparams, darrays, dgen): the derivative of (gcy.params, discretize_gcy(gcy, shapes)) with respect to the
    persistence parameter `name`; see ``discretize_ssy_persistence_tangent``."""
    _check_persistence(GCY_PARAMS, GCY_PERSISTENCE, name, method, "GCY")
    arr = discretize_gcy(gcy, shapes)
    dparams, d, dgen = _gcy_persistence(gcy, shapes, name, arr)
    ax = LAYOUT["gcy"].persistence[name]
    qi = LAYOUT["gcy"].transitions[ax]
    d[qi] = _apply_generator(dgen[ax], arr[qi])
    return dparams, _zeros_for_none(d, arr), dgen


def _gcy_persistence(gcy, shapes, name, arr):
    """(dparams, state-array tangents with None for zero and for the transition arrays, dgen)."""
    n_z, n_z_π, n_h_z, n_h_c, n_h_zπ, n_h_λ = (int(s) for s in shapes)
    (β, ψ, γ, ρ_λ, s_λ, μ_c, φ_c, ρ, ρ_π, φ_z, ρ_c, s_c, ρ_z, s_z,
     ρ_ππ, φ_zπ, ρ_zπ, s_zπ) = gcy.params
    z_shape = arr[0].shape
    d = [None] * len(arr)
    dparams = np.zeros(len(GCY_PARAMS))
    dparams[GCY_PARAMS.index(name)] = 1.0
    dgen = [None] * 6
    ax = LAYOUT["gcy"].persistence[name]
    z_π, σ_z, σ_zπ = arr[2], arr[6], arr[12]
    g_z = _unit_grid(n_z, ρ)                   # z_states[b, c, e, a] = σ_z[c] g_z[a] + ρ_π z_π[e, b] / (1 - ρ)
    g_zπ = _unit_grid(n_z_π, ρ_ππ)             # z_π_states[e, b] = σ_zπ[e] g_zπ[b]

    def z_from_drift(dz_π):                    # d z_states through its drift ρ_π z_π / (1 - ρ)
        return np.broadcast_to((ρ_π * dz_π.T / (1.0 - ρ))[:, None, :, None], z_shape).copy()
    if name == "ρ_λ":
        d[13] = arr[13] * _grid_drho(ρ_λ)
        dgen[ax] = rouwenhorst_generator(n_h_λ, ρ_λ)
    elif name == "ρ_c":
        d[7] = arr[7] * _grid_drho(ρ_c)
        d[9] = arr[9] * d[7]
        dgen[ax] = rouwenhorst_generator(n_h_c, ρ_c)
    elif name == "ρ_z":                                  # h_z -> σ_z -> z
        d[4] = arr[4] * _grid_drho(ρ_z)
        d[6] = σ_z * d[4]
        d[0] = np.broadcast_to(d[6][None, :, None, None] * g_z[None, None, None, :], z_shape).copy()
        dgen[ax] = rouwenhorst_generator(n_h_z, ρ_z)
    elif name == "ρ_zπ":                                 # h_zπ -> σ_zπ -> z_π -> z
        d[10] = arr[10] * _grid_drho(ρ_zπ)
        d[12] = σ_zπ * d[10]
        d[2] = d[12][:, None] * g_zπ[None, :]
        d[0] = z_from_drift(d[2])
        dgen[ax] = rouwenhorst_generator(n_h_zπ, ρ_zπ)
    elif name == "ρ_ππ":                                 # z_π -> z
        d[2] = z_π * _grid_drho(ρ_ππ)
        d[0] = z_from_drift(d[2])
        dgen[ax] = rouwenhorst_generator(n_z_π, ρ_ππ)
    else:                                                # ρ: the centred z grid and the drift ρ_π z_π / (1 - ρ)
        centred = np.broadcast_to(σ_z[None, :, None, None] * g_z[None, None, None, :], z_shape)
        d[0] = centred * _grid_drho(ρ) + z_from_drift(z_π) / (1.0 - ρ)
        dgen[ax] = rouwenhorst_generator(n_z, ρ)
    return dparams, d, dgen


# -- fixed-point sensitivities ---------------------------------------------------------------------------------------
_TANGENTS = {"ssy": (_ssy_tangent, _ssy_persistence), "gcy": (_gcy_tangent, _gcy_persistence)}


def _directions(model, shapes, names, arr, persistence=False):
    """[(dparams, darrays, dgen)] of the named parameters; dgen is None for all but the persistences."""
    L = _kind(model)
    tangent, ptangent = _TANGENTS[L.kind]
    out = []
    for nm in names:
        if persistence and nm in L.persistence:
            out.append(ptangent(model, shapes, nm, arr))
        else:
            _check(L.params, L.supported, nm, "rouwenhorst", L.kind.upper())
            out.append(tangent(model, shapes, nm, arr) + (None,))
    return out


def wc_ratio_sensitivities(model, shapes, w_star, wrt=None, rtol=1e-10, atol=0.0, persistence=False):
    """{name: dw*/dp_name} (host arrays of the grid's shape) at a converged fixed point ``w_star`` of
    (model, shapes): one tangent of T and one BiCGSTAB solve of (I - J(w*)) x = dT/dp per parameter.  ``wrt``: the
    Greek parameter names (default: every supported one).  rtol / atol: the solve's stopping rule on |r|_2.
    ``persistence=True`` admits the persistence parameters (``SSY_PERSISTENCE`` / ``GCY_PERSISTENCE``) in ``wrt``
    and makes the default every parameter of the model."""
    import torch
    L = _kind(model)
    pers = L.persistence if persistence else ()
    default = L.params if persistence else L.supported
    names = default if wrt is None else tuple([wrt] if isinstance(wrt, str) else wrt)
    for nm in names:                                               # (ValueError before any device work)
        if nm not in pers:
            _check(L.params, L.supported, nm, "rouwenhorst", type(model).__name__)
    op, arr = _operator(model, shapes)
    dirs = _directions(model, shapes, names, arr, persistence)
    w = _device_grid(op, w_star, "w_star")
    rhs, x, tw = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)
    out = {}
    for nm, (dp, da, dg) in zip(names, dirs):
        op.param_tangent_dev(w.data_ptr(), dp, da, rhs.data_ptr(), tw.data_ptr(), dgen=dg)
        op.solve_linear_dev(rhs.data_ptr(), x.data_ptr(), False, rtol, atol)
        out[nm] = x.cpu().numpy()
    return out


def wc_ratio_sensitivities_continuous(model, grids, w_star, wrt=None, *, rtol=1e-10, atol=0.0, operator=None, d=5, device=0):
    """``wc_ratio_sensitivities`` for the continuous-state model: {name: dw*/dp_name} (host arrays of the grid's shape)
    at a converged fixed point ``w_star`` on ``grids`` (as ``wc_ratio_continuous`` returns them), plus
    ``"_info": {name: (BiCGSTAB iterations, final relative residual)}``.  Per parameter one tangent of T
    (``ContinuousOperator.cont_param_tangent_dev``) and one solve of (I − J(w*)) x = ∂T/∂p; ``SdfsError`` if a solve
    breaks down or stops above max(rtol |rhs|₂, atol).

    What is differentiated is the operator a ``ContinuousOperator`` represents, T(w; p) with its grids, nodes and weights
    held fixed -- ``jax.jvp`` of the reference's ``T`` with respect to the parameters, ``grids, nodes, weights`` closed
    over.  ``build_grid`` depends on the parameters too; the movement of the grid is NOT part of this derivative.  There
    is no Rouwenhorst matrix here, so every parameter is admitted, the persistences included.

    wrt: Greek names of ``SSY_PARAMS`` / ``GCY_PARAMS`` (default: all of them).  operator: a ``ContinuousOperator`` on
    these parameters and grids, whose nodes and weights define the expectation; otherwise one is built with
    ``qnwnorm([d] * D)`` on ``device``.  Every ValueError / TypeError is raised before any device work."""
    import torch
    _, _, grids, shapes = _cont_grids(model, grids, w_star)        # (TypeError for anything but an SSY or a GCY)
    names, allp = _cont_wrt(model, wrt)
    rtol, atol = _check_tolerance("rtol", rtol, False), _check_tolerance("atol", atol, True)
    d = _cont_operator_or_d(model, grids, shapes, operator, d)
    _check_w_star(w_star, "a fixed point of T is 1 + β(…)^(1/θ) > 1; the tangent takes ln of its interpolant")
    op = _cont_operator(model, grids, operator, d, device)
    w = _device_grid(op, w_star, "w_star")
    rhs, x = torch.empty_like(w), torch.empty_like(w)
    _Fence(op).before_library()
    out, info = {}, {}
    for nm in names:
        dp = np.zeros(len(allp))
        dp[allp.index(nm)] = 1.0
        op.cont_param_tangent_dev(w.data_ptr(), dp, rhs.data_ptr())
        info[nm] = op.solve_linear_dev(rhs.data_ptr(), x.data_ptr(), False, rtol, atol)   # (ends synchronised)
        out[nm] = x.cpu().numpy()
    out["_info"] = info
    return out


def wc_ratio_gradient(model, shapes, w_star, g, rtol=1e-10, atol=0.0, persistence=False):
    """{name: d<g, w*>/dp_name} for every supported parameter at a converged ``w_star``: one transposed solve
    lambda = (I - J(w*)^T)^{-1} g, then <lambda, dT/dp_k> per parameter (a tangent of T each, no further solve).
    ``persistence=True``: every parameter of the model, the persistences included."""
    import torch
    L = _kind(model)
    names = L.params if persistence else L.supported
    op, arr = _operator(model, shapes)
    dirs = _directions(model, shapes, names, arr, persistence)
    w = _device_grid(op, w_star, "w_star")
    gd = _device_grid(op, g, "g")
    lam, rhs, tw = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)
    op.linearize_dev(w.data_ptr(), tw.data_ptr())
    op.solve_linear_dev(gd.data_ptr(), lam.data_ptr(), True, rtol, atol)
    lv = lam.view(-1)
    out = {}
    for nm, (dp, da, dg) in zip(names, dirs):
        op.param_tangent_dev(w.data_ptr(), dp, da, rhs.data_ptr(), tw.data_ptr(), dgen=dg)
        out[nm] = float(torch.dot(lv, rhs.view(-1)))
    return out


def wc_ratio_gradient_continuous(model, grids, w_star, g, wrt=None, *, rtol=1e-10, atol=0.0, operator=None, d=5, device=0):
    """``wc_ratio_gradient`` for the continuous-state model: {name: d⟨g, w*⟩/dp_name} (floats) at a converged fixed point
    ``w_star`` on ``grids`` (as ``wc_ratio_continuous`` returns them), plus ``"_info": (BiCGSTAB iterations, final
    relative residual)`` of the adjoint solve and ``"_adjoint"``: λ as a host array of the grid's shape.  One
    linearisation at w*, ONE transposed solve λ = (I − J(w*)ᵀ)⁻¹ g (``ContinuousOperator.cont_solve_adjoint_dev``), then
    per parameter one tangent of T (``cont_param_tangent_dev``) and the dot product ⟨λ, ∂T/∂p⟩, no further solve --
    where ``wc_ratio_sensitivities_continuous`` takes one solve per parameter.  ``SdfsError`` if the solve breaks down
    or stops above max(rtol |g|₂, atol).

    What is differentiated is the operator a ``ContinuousOperator`` represents, T(w; p) with its grids, nodes and weights
    held fixed -- ``jax.vjp`` of the reference's ``T`` with respect to the parameters, ``grids, nodes, weights`` closed
    over.  ``build_grid`` depends on the parameters too; the movement of the grid is NOT part of this derivative.  Every
    parameter is admitted, the persistences included.

    Jᵀ is applied with hardware fp64 atomic adds whose arrival order varies: two calls on the same input agree to
    rounding (far inside the solve's tolerance), NOT bit for bit -- unlike every other analysis function here.

    g: a finite array of the grid's shape.  wrt, operator, d, device: as in ``wc_ratio_sensitivities_continuous``.  Every
    ValueError / TypeError is raised before any device work."""
    import torch
    _, _, grids, shapes = _cont_grids(model, grids, w_star)        # (TypeError for anything but an SSY or a GCY)
    names, allp = _cont_wrt(model, wrt)
    _check_finite_grid(g, shapes, "g")
    rtol, atol = _check_tolerance("rtol", rtol, False), _check_tolerance("atol", atol, True)
    d = _cont_operator_or_d(model, grids, shapes, operator, d)
    _check_w_star(w_star, "a fixed point of T is 1 + β(…)^(1/θ) > 1; the tangent takes ln of its interpolant")
    op = _cont_operator(model, grids, operator, d, device)
    w = _device_grid(op, w_star, "w_star")
    gd = _device_grid(op, g, "g")
    lam, rhs = torch.empty_like(w), torch.empty_like(w)
    fence = _Fence(op)
    fence.before_library()
    op.linearize_dev(w.data_ptr())
    info = op.cont_solve_adjoint_dev(gd.data_ptr(), lam.data_ptr(), rtol, atol)   # (ends synchronised)
    lv = lam.view(-1)
    out = {}
    for nm in names:
        dp = np.zeros(len(allp))
        dp[allp.index(nm)] = 1.0
        op.cont_param_tangent_dev(w.data_ptr(), dp, rhs.data_ptr())
        fence.before_torch()
        out[nm] = float(torch.dot(lv, rhs.view(-1)))               # (.item(): torch's stream is drained again)
    out["_info"] = info
    out["_adjoint"] = lam.cpu().numpy()
    return out


# -- gradients from adjoint moments (the batch path: csrc/batch_adjoint.hpp) -------------------------------------------
# (the places of the moment block: ``Layout.moments`` of _requests.py)


def adjoint_moments_to_gradient(model, shapes, moments, persistence=True, method="rouwenhorst"):
    """{name: d<g, w*>/dp_name} of one model from its adjoint moment block (``BatchOperator.adjoint``; layout
    s0 s1 s2 | R[ndim] | M1[n_λ] | M2[n_c] | M3[a3 table]).  Pure numpy: the directions are those of
    ``wc_ratio_gradient`` and the log-tangents restate ``sens_tables`` of the library,

        dθ = -dγ / (1 - 1/ψ) - dψ θ / (ψ (ψ - 1)),   d ln a1 = dθ h_λ + θ dh_λ,
        d ln a2 = (1 - γ) σ_c ((1 - γ) dσ_c - dγ σ_c),   d ln a3 = (1 - γ) (dμ_c + dz) - dγ (μ_c + z),

    so that  dφ/dp = dβ/β s0 - dθ/θ s1 + (<M2, d ln a2> + <M3, d ln a3>)/θ + (dθ s2 + <M1, d ln a1>)/θ
    - [p is the persistence ρ_k of axis k] R[k] / (2 ρ_k θ).  The 9 / 12 supported parameters, or all 13 / 18 with
    ``persistence=True``.  ValueError for a Tauchen grid."""
    if method != "rouwenhorst":
        raise ValueError(f"parameter tangents are implemented for Rouwenhorst grids only, not {method!r}")
    L = _kind(model)
    kind, supported, disc, allp = L.kind, L.supported, L.discretize, L.params
    shapes = tuple(int(s) for s in shapes)
    (ib, ig, ips, imu), (ia_hl, ia_sc, ia_z), (ax_l, ax_c) = L.moments
    ndim = len(shapes)
    arr = disc(model, shapes)
    n_l, n_c, na3 = shapes[ax_l], shapes[ax_c], int(np.asarray(arr[ia_z]).size)
    mom = np.asarray(moments, dtype=np.float64).ravel()
    if mom.size != 3 + ndim + n_l + n_c + na3:
        raise ValueError(f"moments has {mom.size} entries, the block of {kind} {shapes} has {3 + ndim + n_l + n_c + na3}")
    s0, s1, s2 = mom[:3]
    R = mom[3:3 + ndim]
    M1 = mom[3 + ndim:3 + ndim + n_l]
    M2 = mom[3 + ndim + n_l:3 + ndim + n_l + n_c]
    M3 = mom[3 + ndim + n_l + n_c:]
    params = np.asarray(model.params, dtype=np.float64)
    β, γ, ψ, μ_c = params[ib], params[ig], params[ips], params[imu]
    θ = (1.0 - γ) / (1.0 - 1.0 / ψ)
    h_λ, σ_c, z = (np.asarray(arr[i], dtype=np.float64).ravel() for i in (ia_hl, ia_sc, ia_z))
    names = allp if persistence else supported
    axis_of = L.persistence
    out = {}
    for nm, (dp, da, dgen) in zip(names, _directions(model, shapes, names, arr, persistence)):
        def d(i):
            return 0.0 if da[i] is None else np.asarray(da[i], dtype=np.float64).ravel()
        dγ, dψ, dμ = dp[ig], dp[ips], dp[imu]
        dθ = -dγ / (1.0 - 1.0 / ψ) - dψ * θ / (ψ * (ψ - 1.0))
        dla1 = dθ * h_λ + θ * d(ia_hl)
        dla2 = (1.0 - γ) * σ_c * ((1.0 - γ) * d(ia_sc) - dγ * σ_c)
        dla3 = (1.0 - γ) * (dμ + d(ia_z)) - dγ * (μ_c + z)
        val = dp[ib] / β * s0 - dθ / θ * s1 + (M2 @ dla2 + M3 @ dla3) / θ + (dθ * s2 + M1 @ dla1) / θ
        if dgen is not None:
            val -= R[axis_of[nm]] / (2.0 * params[allp.index(nm)] * θ)
        out[nm] = float(val)
    return out

"""
Asset prices with the stochastic discount factor at the fixed point w* of the wealth-consumption ratio.

The model's Euler equation fixes the pricing kernel

    M' = β^θ exp(θ g_λ' − γ g_c') (w(X') / (w(X) − 1))^(θ−1),    g_c' = μ_c + z + σ_c ξ',  g_λ' = h_λ'.

Every SDF-weighted or physical expectation pricing needs is the library's factorised expectation with other diagonal
scalings on its two sides.  For a power p ∈ {0, 1, 2} of the SDF and exponents (κ_λ, κ_c)

    K f (x) = [β^θ (Tw(x) − 1)^(1−θ)]^p · E_x[exp(κ_λ g_λ' + κ_c g_c') · w(X')^(p(θ−1)) · f(X')]

runs on the J·v kernels of every plan (``KoopmansOperator.set_tilt_dev`` / ``apply_tilted_dev`` / ``solve_tilted_dev``
/ ``tilted_horizons_dev``); K(1, θ, 1−γ) is J(w).  What this module computes from it, per model period:

    E_x[M] = K(1, θ, −γ)·1,  log risk-free rate = −log E_x[M]
    max Sharpe ratio (Hansen–Jagannathan) = √(E_x[M²] / E_x[M]² − 1),  E_x[M²] = K(2, 2θ, −2γ)·1
    zero-coupon claim on G_c^κ at horizon n: P_n = K(1, θ, κ−γ) P_{n−1}, P_0 = 1, yield −log P_n / n
    perpetual claim on G_c^κ: price–dividend ratio v = (I − K)⁻¹ K·1,
        expected return E_x[R] = K(0, 0, κ)(1 + v) / v, log premium log E_x[R] + log E_x[M]

K is positive, so a positive solution of (I − K) v = K·1 exists exactly when its spectral radius r(K) < 1; the
horizon loop brackets r(K) by the minimum and maximum of P_n / P_{n−1} (Collatz–Wielandt).  Everything after the
discretisation runs in libsdfs_hip.so, fp64; w* and the work vectors stay on the device.
"""
import numpy as np

from ._requests import (_shapes, _check_grid, _kappa, _check_n_max, _check_save, _check_rtol, _check_w_star, _weights,
                        _cont_grids, _cont_operator_or_d, _operator, _cont_operator, _device_grid, _Fence,
                        _check_tolerance, LAYOUT, stationary_weights)
from .sensitivity import _check, _directions
from ._lib import SdfsError, SDFS_ERR_NUMERIC


def _numeric(e):
    return f"error {SDFS_ERR_NUMERIC}:" in str(e)


def _sdf_moments(op, w, θ, γ, fence):
    """``sdf_moments`` on an operator with a tilted expectation, w on its device."""
    import torch
    one = torch.ones_like(w)
    em, em2 = torch.empty_like(w), torch.empty_like(w)
    fence.before_library()
    op.set_tilt_dev(w.data_ptr(), 1, θ, -γ)
    op.apply_tilted_dev(one.data_ptr(), em.data_ptr())
    op.set_tilt_dev(w.data_ptr(), 2, 2.0 * θ, -2.0 * γ)
    op.apply_tilted_dev(one.data_ptr(), em2.data_ptr())
    fence.before_torch()
    E_M = em.cpu().numpy()
    E_M2 = em2.cpu().numpy()
    return {"E_M": E_M, "log_rf": -np.log(E_M), "max_sharpe": np.sqrt(np.maximum(E_M2 / E_M ** 2 - 1.0, 0.0))}


def _claim_prices(op, w, θ, γ, k, rtol, fence):
    """``claim_prices`` on an operator with a tilted expectation, w on its device."""
    import torch
    one = torch.ones_like(w)
    k1, v, num, em, er = (torch.empty_like(w) for _ in range(5))
    fence.before_library()
    op.set_tilt_dev(w.data_ptr(), 1, θ, k - γ)
    op.apply_tilted_dev(one.data_ptr(), k1.data_ptr())
    try:
        op.solve_tilted_dev(k1.data_ptr(), v.data_ptr(), rtol)
    except SdfsError as e:
        if _numeric(e):
            raise ValueError(f"no finite price: r(K) ≥ 1, or (I − K) too close to singular for the solve ({e})") from None
        raise
    if not bool(torch.all(v > 0)):                       # (the solve ended with a host synchronisation)
        raise ValueError("no finite price: r(K) ≥ 1 (the solution of (I − K) v = K·1 is not strictly positive)")
    torch.add(v, 1.0, out=num)
    fence.before_library()
    op.set_tilt_dev(None, 0, 0.0, k)
    op.apply_tilted_dev(num.data_ptr(), er.data_ptr())
    op.set_tilt_dev(w.data_ptr(), 1, θ, -γ)
    op.apply_tilted_dev(one.data_ptr(), em.data_ptr())
    fence.before_torch()
    # (er and v are final: the division may stand anywhere after the product that wrote er; it used to precede E_x[M])
    ER = er.div_(v).cpu().numpy()
    return {"pd": v.cpu().numpy(), "expected_return": ER, "log_premium": np.log(ER) + np.log(em.cpu().numpy())}


def _horizons(call):
    """The result of a horizon loop, its numeric refusal as a ValueError."""
    try:
        return call()
    except SdfsError as e:
        if _numeric(e):
            raise ValueError(f"the claim prices left the positive numbers (underflow or overflow): {e}") from None
        raise


def sdf_moments(model, shapes, w_star):
    """{"E_M", "log_rf", "max_sharpe"} on the grid (host arrays) at the fixed point ``w_star``: the conditional mean of
    the SDF, the log risk-free rate −log E_x[M] and the Hansen–Jagannathan bound √(E_x[M²] / E_x[M]² − 1)."""
    _, shapes = _shapes(model, shapes)
    _check_grid(w_star, shapes, "w_star")
    op, _ = _operator(model, shapes)
    return _sdf_moments(op, _device_grid(op, w_star, "w_star"), model.θ, model.γ, _Fence())


def term_structure(model, shapes, w_star, n_max, kappa=0.0, weights=None, save=()):
    """Zero-coupon claims on G_c^κ (κ = 0: real bonds; κ = 1: consumption strips) for horizons 1 ... n_max:
    P_n = K(1, θ, κ−γ) P_{n−1}, P_0 = 1, all on the device.  ``weights``: product-form weights g over the grid, None for
    the stationary distribution, else one entry per axis (a state index or a vector).  Returns {"horizons",
    "price": ⟨g, P_n⟩, "yield": ⟨g, −log P_n⟩ / n, "bracket": (n_max, 2) min and max of P_n / P_{n−1} (they bracket
    r(K)), "grids": {n: P_n} for n in ``save``}."""
    import torch
    kind, shapes = _shapes(model, shapes)
    n_max = _check_n_max(n_max)
    k = _kappa(kappa)
    save = _check_save(save, n_max)
    g = _weights(kind, shapes, weights, model)
    _check_grid(w_star, shapes, "w_star")
    op, _ = _operator(model, shapes)
    w = _device_grid(op, w_star, "w_star")
    grids = [torch.empty_like(w) for _ in save]
    op.set_tilt_dev(w.data_ptr(), 1, model.θ, k - model.γ)
    out = _horizons(lambda: op.tilted_horizons_dev(n_max, g, save, [t.data_ptr() for t in grids]))
    return {"horizons": np.arange(1, n_max + 1), "price": out[:, 0].copy(), "yield": out[:, 1].copy(),
            "bracket": out[:, 2:4].copy(), "grids": {n: t.cpu().numpy() for n, t in zip(save, grids)}}


def claim_prices(model, shapes, w_star, kappa, rtol=1e-10):
    """The perpetual claim on G_c^κ (κ = 1: the consumption claim, whose price–dividend ratio is w* − 1): {"pd": v =
    (I − K)⁻¹ K·1 with K = K(1, θ, κ−γ), "expected_return": E_x[R] = K(0, 0, κ)(1 + v) / v, "log_premium":
    log E_x[R] + log E_x[M]} on the grid (host arrays).  ValueError ("no finite price: r(K) ≥ 1") when the solve has
    no strictly positive solution."""
    _, shapes = _shapes(model, shapes)
    k = _kappa(kappa)
    rtol = _check_rtol(rtol)
    _check_grid(w_star, shapes, "w_star")
    op, _ = _operator(model, shapes)
    return _claim_prices(op, _device_grid(op, w_star, "w_star"), model.θ, model.γ, k, rtol, _Fence())


def price_sensitivities(model, shapes, w_star, kappa=None, wrt=None, rtol=1e-10, atol=0.0, persistence=False, dw=None):
    """Parameter sensitivities of the prices at a converged fixed point ``w_star``:
    {name: {"E_M", "log_rf", "max_sharpe"[, "pd", "expected_return", "log_premium"]}}, each the derivative of that field
    of ``sdf_moments`` / ``claim_prices(kappa)`` with respect to the parameter (host arrays of the grid's shape;
    "max_sharpe" is NaN where the bound is zero), plus ``"_info": {name: (iterations of the dw* solve or None, iterations
    of the dv solve or None)}``.  ``kappa=None``: the SDF moments only.  ``wrt``, ``persistence``: as in
    ``wc_ratio_sensitivities``.  ``dw``: the result of a previous ``wc_ratio_sensitivities`` call on the same point, which
    skips those solves.  rtol / atol: the stopping rule of both solves.

    Per parameter: dw*/dp (one solve of I − J), then the tangent of each tilt along the direction that moves the
    parameter and w* together (``KoopmansOperator.tilt_tangent_dev``): dE_M = dK(1, θ, −γ)[1], dE_M² = dK(2, 2θ, −2γ)[1],
    dv = (I − K)⁻¹ dK(1, θ, κ−γ)[1 + v] (one tilted solve), dE_R = (dK(0, 0, κ)[1 + v; dv] − E_R dv) / v.  E_M, E_M², v and
    E_R are computed once.  The loops run tilt by tilt, so dw*/dp, dE_M / E_M and dv/dp of every requested parameter stay
    on the device meanwhile: three grids per parameter.  ValueError ("no finite price: r(K) ≥ 1") exactly as ``claim_prices``."""
    import torch
    kind, shapes = _shapes(model, shapes)
    L = LAYOUT[kind]
    k = None if kappa is None else _kappa(kappa)
    pers = L.persistence if persistence else ()
    default = L.params if persistence else L.supported
    names = default if wrt is None else tuple([wrt] if isinstance(wrt, str) else wrt)
    for nm in names:                                               # (ValueError before any device work)
        if nm not in pers:
            _check(L.params, L.supported, nm, "rouwenhorst", type(model).__name__)
    rtol, atol = _check_tolerance("rtol", rtol, False), _check_tolerance("atol", atol, True)
    _check_grid(w_star, shapes, "w_star")
    if dw is not None:
        if not isinstance(dw, dict):
            raise TypeError(f"dw must be the dict wc_ratio_sensitivities returns, not {type(dw).__name__}")
        for nm in names:
            if nm not in dw:
                raise ValueError(f"dw has no entry for parameter {nm!r}")
            _check_grid(dw[nm], shapes, f"dw[{nm!r}]")
    op, arr = _operator(model, shapes)
    dirs = _directions(model, shapes, names, arr, persistence)
    w = _device_grid(op, w_star, "w_star")
    θ, γ = model.θ, model.γ
    (_, ig, ips, _), _, _ = L.moments
    ψ = model.params[ips]
    dθ = [-dp[ig] / (1.0 - 1.0 / ψ) - dp[ips] * θ / (ψ * (ψ - 1.0)) for dp, _, _ in dirs]
    dγ = [dp[ig] for dp, _, _ in dirs]
    rhs, tmp = torch.empty_like(w), torch.empty_like(w)
    it_w, it_v = {}, {}

    # dw*/dp (the tangents leave the cached linearisation at w*, which every tilt below restates)
    dws = []
    for nm, (dp, da, dg) in zip(names, dirs):
        if dw is not None:
            dws.append(_device_grid(op, dw[nm], f"dw[{nm!r}]"))
            it_w[nm] = None
            continue
        x = torch.empty_like(w)
        op.param_tangent_dev(w.data_ptr(), dp, da, rhs.data_ptr(), tmp.data_ptr(), dgen=dg)
        it_w[nm] = op.solve_linear_dev(rhs.data_ptr(), x.data_ptr(), False, rtol, atol)[0]
        dws.append(x)

    def tangent(j, dkl, dkc, f, df, kf, out):
        dp, da, dg = dirs[j]
        x = dws[j].data_ptr()
        op.tilt_tangent_dev(w.data_ptr(), x, x, dp, da, dg, dkl, dkc, f, df, kf.data_ptr(), out.data_ptr())

    # The fields are formed on the device (the library launches on torch's current stream); what crosses to the host is
    # the result alone.  rel[j] = dE_M / E_M stays for the Sharpe bound and the premium.
    out = {nm: {} for nm in names}
    one = torch.ones_like(w)
    em, em2 = torch.empty_like(w), torch.empty_like(w)
    op.set_tilt_dev(w.data_ptr(), 1, θ, -γ)
    op.apply_tilted_dev(one.data_ptr(), em.data_ptr())
    rel = []
    for j, nm in enumerate(names):
        tangent(j, dθ[j], -dγ[j], None, None, em, tmp)
        out[nm]["E_M"] = tmp.cpu().numpy()
        rel.append(tmp / em)
        out[nm]["log_rf"] = (-rel[j]).cpu().numpy()
    op.set_tilt_dev(w.data_ptr(), 2, 2.0 * θ, -2.0 * γ)
    op.apply_tilted_dev(one.data_ptr(), em2.data_ptr())
    q = em2 / (em * em)
    s = torch.sqrt(torch.clamp(q - 1.0, min=0.0))
    q.div_(2.0 * s)                                                   # (inf where the bound is zero: NaN below)
    for j, nm in enumerate(names):
        tangent(j, 2.0 * dθ[j], -2.0 * dγ[j], None, None, em2, tmp)
        ms = q * (tmp / em2 - 2.0 * rel[j])
        out[nm]["max_sharpe"] = torch.where(s > 0.0, ms, torch.full_like(ms, float("nan"))).cpu().numpy()
    del em, em2, q, s
    if k is not None:
        v, num, er = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)
        op.set_tilt_dev(w.data_ptr(), 1, θ, k - γ)
        op.apply_tilted_dev(one.data_ptr(), rhs.data_ptr())
        try:
            op.solve_tilted_dev(rhs.data_ptr(), v.data_ptr(), rtol, atol)
        except SdfsError as e:
            if _numeric(e):
                raise ValueError(f"no finite price: r(K) ≥ 1, or (I − K) too close to singular for the solve ({e})") from None
            raise
        if not bool(torch.all(v > 0)):
            raise ValueError("no finite price: r(K) ≥ 1 (the solution of (I − K) v = K·1 is not strictly positive)")
        torch.add(v, 1.0, out=num)
        dvs = []
        for j, nm in enumerate(names):                                 # K(1 + v) = v: no further product for K f
            tangent(j, dθ[j], -dγ[j], num.data_ptr(), None, v, rhs)
            dv = torch.empty_like(w)
            it_v[nm] = op.solve_tilted_dev(rhs.data_ptr(), dv.data_ptr(), rtol, atol)[0]
            out[nm]["pd"] = dv.cpu().numpy()
            dvs.append(dv)
        op.set_tilt_dev(None, 0, 0.0, k)
        op.apply_tilted_dev(num.data_ptr(), er.data_ptr())
        E_R = er / v
        for j, nm in enumerate(names):
            tangent(j, 0.0, 0.0, num.data_ptr(), dvs[j].data_ptr(), er, tmp)
            dER = (tmp - E_R * dvs[j]) / v
            out[nm]["expected_return"] = dER.cpu().numpy()
            out[nm]["log_premium"] = (dER / E_R + rel[j]).cpu().numpy()
    out["_info"] = {nm: (it_w[nm], it_v.get(nm)) for nm in names}
    return out


# -- the continuous-state model -----------------------------------------------------------------------
#
# K(p, κ_λ, κ_c) f (x) = d2(x) · Σ_m W_m exp(κ_λ s_λ η_0m) · ŵ(x'_m)^(p(θ−1)) · f̂(x'_m) with the operator's nodes and
# weights, x'_m = next_state(x, η_m), ŵ and f̂ the multilinear interpolants of ``lin_interp``, and
# d2(x) = [β^θ (w(x) − 1)^(1−θ)]^p exp(κ_c (μ_c + z) + ½ κ_c² σ_c(x)² + κ_λ ρ_λ h_λ): the K above with the quadrature in
# place of the chain, and w − 1 where that one has Tw − 1 (``ContinuousOperator.set_tilt_dev`` …, which call the
# ``sdfs_cont_*`` entry points).

def _cont_states(states, nd):
    """The query states of ``term_structure_continuous`` as an (nq, nd) array; None is the zero state."""
    if states is None:
        return np.zeros((1, nd))
    try:
        st = np.ascontiguousarray(np.asarray(states, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"states must be None or an array (nq, {nd})") from None
    if st.ndim != 2 or st.shape[1] != nd or st.shape[0] < 1 or st.shape[0] > 1 << 24:
        raise ValueError(f"states has shape {st.shape}: (nq, {nd}) with 1 ... 2^24 states")
    if not np.all(np.isfinite(st)):
        raise ValueError("states must be finite")
    return st


def sdf_moments_continuous(model, grids, w_star, *, operator=None, d=5, device=0):
    """``sdf_moments`` for the continuous-state model: {"E_M", "log_rf", "max_sharpe"} on the grid (host arrays) at the
    grid function ``w_star`` (on ``grids``, as ``wc_ratio_continuous`` returns them).  operator: a ``ContinuousOperator``
    on these parameters and grids, whose nodes and weights define the expectation; otherwise one is built with
    ``qnwnorm([d] * D)`` on ``device`` (as in ``simulate_continuous``)."""
    _, _, grids, shapes = _cont_grids(model, grids, w_star)
    d = _cont_operator_or_d(model, grids, shapes, operator, d)
    _check_w_star(w_star)
    op = _cont_operator(model, grids, operator, d, device)
    return _sdf_moments(op, _device_grid(op, w_star, "w_star"), model.θ, model.γ, _Fence(op))


def term_structure_continuous(model, grids, w_star, n_max, kappa=0.0, *, states=None, save=(), operator=None, d=5, device=0):
    """``term_structure`` for the continuous-state model: zero-coupon claims on G_c^κ for horizons 1 ... n_max,
    P_n = K(1, θ, κ−γ) P_{n−1}, P_0 = 1, on the device.  states: None (the zero state) or an array (nq, D) of query
    states, at which P_n is interpolated as ``lin_interp`` does (coordinates clamped to the grid).  Returns {"horizons",
    "price": (n_max, nq), "yield": −ln price / n, "bracket": (n_max, 2) min and max of P_n / P_{n−1} over the grid (they
    bracket r(K)), "grids": {n: P_n} for n in ``save``}.  operator, d, device: as in ``sdf_moments_continuous``."""
    import torch
    _, nd, grids, shapes = _cont_grids(model, grids, w_star)
    n_max = _check_n_max(n_max)
    k = _kappa(kappa)
    save = _check_save(save, n_max, wrap=True)
    st = _cont_states(states, nd)
    d = _cont_operator_or_d(model, grids, shapes, operator, d)
    _check_w_star(w_star)
    op = _cont_operator(model, grids, operator, d, device)
    w = _device_grid(op, w_star, "w_star")
    saved = [torch.empty_like(w) for _ in save]
    _Fence(op).before_library()
    op.set_tilt_dev(w.data_ptr(), 1, model.θ, k - model.γ)
    price, bracket = _horizons(lambda: op.cont_tilted_horizons_dev(n_max, st, save, [t.data_ptr() for t in saved]))
    horizons = np.arange(1, n_max + 1)
    return {"horizons": horizons, "price": price, "yield": -np.log(price) / horizons[:, None], "bracket": bracket,
            "grids": {n: t.cpu().numpy() for n, t in zip(save, saved)}}


def claim_prices_continuous(model, grids, w_star, kappa, *, rtol=1e-10, operator=None, d=5, device=0):
    """``claim_prices`` for the continuous-state model: the perpetual claim on G_c^κ, {"pd": v = (I − K)⁻¹ K·1 with
    K = K(1, θ, κ−γ), "expected_return": E_x[R] = K(0, 0, κ)(1 + v) / v, "log_premium": log E_x[R] + log E_x[M]} on the
    grid (host arrays).  At κ = 1 and a fixed point w*, v = w* − 1.  ValueError ("no finite price: r(K) ≥ 1") when the
    solve has no strictly positive solution.  operator, d, device: as in ``sdf_moments_continuous``."""
    _, _, grids, shapes = _cont_grids(model, grids, w_star)
    k = _kappa(kappa)
    rtol = _check_rtol(rtol, wrap=True)
    d = _cont_operator_or_d(model, grids, shapes, operator, d)
    _check_w_star(w_star)
    op = _cont_operator(model, grids, operator, d, device)
    return _claim_prices(op, _device_grid(op, w_star, "w_star"), model.θ, model.γ, k, rtol, _Fence(op))


__all__ = ["stationary_weights", "sdf_moments", "term_structure", "claim_prices", "price_sensitivities", "sdf_moments_continuous",
           "term_structure_continuous", "claim_prices_continuous"]

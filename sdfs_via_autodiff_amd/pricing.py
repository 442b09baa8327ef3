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
import math

import numpy as np

from .sensitivity import _kind, _operator, _device_grid
from ._lib import SdfsError, SDFS_ERR_NUMERIC

# transition arrays of each axis, in grid order (the conditional tensors carry their conditioning indices in front)
_AXIS_Q = {"ssy": (1, 3, 5, 7), "gcy": (1, 3, 5, 8, 11, 14)}
_NDIM = {"ssy": 4, "gcy": 6}


def _shapes(model, shapes):
    kind = _kind(model)[0]
    shapes = tuple(int(s) for s in shapes)
    if len(shapes) != _NDIM[kind]:
        raise ValueError(f"{kind.upper()} grids have {_NDIM[kind]} axes, got shapes {shapes}")
    if any(s < 2 or s > 32 for s in shapes):
        raise ValueError(f"every axis needs 2 ... 32 states, got shapes {shapes}")
    return kind, shapes


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
    arr = _kind(model)[2](model, shapes) if arrays is None else arrays
    out = []
    for a, (qi, n) in enumerate(zip(_AXIS_Q[kind], shapes)):
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


def _kappa(kappa):
    try:
        k = float(kappa)
    except (TypeError, ValueError):
        raise ValueError(f"kappa must be a real number, got {kappa!r}") from None
    if not math.isfinite(k):
        raise ValueError(f"kappa must be finite, got {kappa!r}")
    return k


def _check_grid(x, shapes, what):
    shp = tuple(int(s) for s in getattr(x, "shape", np.shape(x)))
    if shp != shapes:
        raise ValueError(f"{what} has shape {shp}, the grid is {shapes}")


def _ones(w):
    import torch
    return torch.ones_like(w)


def sdf_moments(model, shapes, w_star):
    """{"E_M", "log_rf", "max_sharpe"} on the grid (host arrays) at the fixed point ``w_star``: the conditional mean of
    the SDF, the log risk-free rate −log E_x[M] and the Hansen–Jagannathan bound √(E_x[M²] / E_x[M]² − 1)."""
    import torch
    _, shapes = _shapes(model, shapes)
    _check_grid(w_star, shapes, "w_star")
    op, _ = _operator(model, shapes)
    w = _device_grid(op, w_star, "w_star")
    one = _ones(w)
    em, em2 = torch.empty_like(w), torch.empty_like(w)
    op.set_tilt_dev(w.data_ptr(), 1, model.θ, -model.γ)
    op.apply_tilted_dev(one.data_ptr(), em.data_ptr())
    op.set_tilt_dev(w.data_ptr(), 2, 2.0 * model.θ, -2.0 * model.γ)
    op.apply_tilted_dev(one.data_ptr(), em2.data_ptr())
    E_M = em.cpu().numpy()
    E_M2 = em2.cpu().numpy()
    return {"E_M": E_M, "log_rf": -np.log(E_M), "max_sharpe": np.sqrt(np.maximum(E_M2 / E_M ** 2 - 1.0, 0.0))}


def term_structure(model, shapes, w_star, n_max, kappa=0.0, weights=None, save=()):
    """Zero-coupon claims on G_c^κ (κ = 0: real bonds; κ = 1: consumption strips) for horizons 1 ... n_max:
    P_n = K(1, θ, κ−γ) P_{n−1}, P_0 = 1, all on the device.  ``weights``: product-form weights g over the grid, None for
    the stationary distribution, else one entry per axis (a state index or a vector).  Returns {"horizons",
    "price": ⟨g, P_n⟩, "yield": ⟨g, −log P_n⟩ / n, "bracket": (n_max, 2) min and max of P_n / P_{n−1} (they bracket
    r(K)), "grids": {n: P_n} for n in ``save``}."""
    import torch
    kind, shapes = _shapes(model, shapes)
    if isinstance(n_max, bool) or not isinstance(n_max, (int, np.integer)) or not 1 <= int(n_max) <= 1 << 24:
        raise ValueError(f"n_max must be an integer in 1 ... 2^24, got {n_max!r}")
    n_max = int(n_max)
    k = _kappa(kappa)
    save = sorted({int(n) for n in save})
    for n in save:
        if not 1 <= n <= n_max:
            raise ValueError(f"save horizon {n} lies outside 1 ... n_max = {n_max}")
    g = _weights(kind, shapes, weights, model)
    _check_grid(w_star, shapes, "w_star")
    op, _ = _operator(model, shapes)
    w = _device_grid(op, w_star, "w_star")
    grids = [torch.empty_like(w) for _ in save]
    op.set_tilt_dev(w.data_ptr(), 1, model.θ, k - model.γ)
    try:
        out = op.tilted_horizons_dev(n_max, g, save, [t.data_ptr() for t in grids])
    except SdfsError as e:
        if f"error {SDFS_ERR_NUMERIC}:" in str(e):
            raise ValueError(f"the claim prices left the positive numbers (underflow or overflow): {e}") from None
        raise
    return {"horizons": np.arange(1, n_max + 1), "price": out[:, 0].copy(), "yield": out[:, 1].copy(),
            "bracket": out[:, 2:4].copy(), "grids": {n: t.cpu().numpy() for n, t in zip(save, grids)}}


def claim_prices(model, shapes, w_star, kappa, rtol=1e-10):
    """The perpetual claim on G_c^κ (κ = 1: the consumption claim, whose price–dividend ratio is w* − 1): {"pd": v =
    (I − K)⁻¹ K·1 with K = K(1, θ, κ−γ), "expected_return": E_x[R] = K(0, 0, κ)(1 + v) / v, "log_premium":
    log E_x[R] + log E_x[M]} on the grid (host arrays).  ValueError ("no finite price: r(K) ≥ 1") when the solve has
    no strictly positive solution."""
    import torch
    _, shapes = _shapes(model, shapes)
    k = _kappa(kappa)
    rtol = float(rtol)
    if not (rtol > 0.0 and math.isfinite(rtol)):
        raise ValueError(f"rtol must be positive, got {rtol!r}")
    _check_grid(w_star, shapes, "w_star")
    op, _ = _operator(model, shapes)
    w = _device_grid(op, w_star, "w_star")
    one = _ones(w)
    k1, v, num, em = (torch.empty_like(w) for _ in range(4))
    op.set_tilt_dev(w.data_ptr(), 1, model.θ, k - model.γ)
    op.apply_tilted_dev(one.data_ptr(), k1.data_ptr())
    try:
        op.solve_tilted_dev(k1.data_ptr(), v.data_ptr(), rtol)
    except SdfsError as e:
        if f"error {SDFS_ERR_NUMERIC}:" in str(e):
            raise ValueError(f"no finite price: r(K) ≥ 1, or (I − K) too close to singular for the solve ({e})") from None
        raise
    if not bool(torch.all(v > 0)):
        raise ValueError("no finite price: r(K) ≥ 1 (the solution of (I − K) v = K·1 is not strictly positive)")
    torch.add(v, 1.0, out=num)
    er = torch.empty_like(w)
    op.set_tilt_dev(None, 0, 0.0, k)
    op.apply_tilted_dev(num.data_ptr(), er.data_ptr())
    er.div_(v)
    op.set_tilt_dev(w.data_ptr(), 1, model.θ, -model.γ)
    op.apply_tilted_dev(one.data_ptr(), em.data_ptr())
    ER = er.cpu().numpy()
    return {"pd": v.cpu().numpy(), "expected_return": ER, "log_premium": np.log(ER) + np.log(em.cpu().numpy())}


def _count(x, name, lo, hi):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi:
        raise ValueError(f"{name} must be an integer in {lo} ... {hi}, got {x!r}")
    return int(x)


def _check_w_star(w_star, why="the log return needs ln(w - 1)"):
    import torch
    if isinstance(w_star, torch.Tensor):
        w_ok = bool(torch.all(w_star > 1.0))
    else:
        w_ok = bool(np.all(np.asarray(w_star, dtype=np.float64) > 1.0))
    if not w_ok:
        raise ValueError(f"w_star must exceed 1 at every grid point ({why})")


# -- the continuous-state model -----------------------------------------------------------------------
#
# K(p, κ_λ, κ_c) f (x) = d2(x) · Σ_m W_m exp(κ_λ s_λ η_0m) · ŵ(x'_m)^(p(θ−1)) · f̂(x'_m) with the operator's nodes and
# weights, x'_m = next_state(x, η_m), ŵ and f̂ the multilinear interpolants of ``lin_interp``, and
# d2(x) = [β^θ (w(x) − 1)^(1−θ)]^p exp(κ_c (μ_c + z) + ½ κ_c² σ_c(x)² + κ_λ ρ_λ h_λ): the K above with the quadrature in
# place of the chain, and w − 1 where that one has Tw − 1 (``ContinuousOperator.cont_set_tilt_dev`` …).

def _cont_model_request(model, grids, w_star, operator, d, between=None, why_w=None):
    """The checks of (model, grids, w_star, operator, d) that ``simulate_continuous`` and the ``*_continuous`` pricing
    functions share, none of which touches a device: (kind, grids, shapes, d).  ``between(nd, shapes)`` runs after the
    grid and shape checks and before those of the operator -- the place of a caller's own argument checks.  ``why_w``: the caller's reason for
    w_star > 1, for the error text."""
    kind = _kind(model)[0]                                 # (TypeError for anything but an SSY or a GCY)
    nd = _NDIM[kind]
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
    if between is not None:
        between(nd, shapes)
    if operator is not None:
        from .continuous import ContinuousOperator
        if not isinstance(operator, ContinuousOperator):
            raise TypeError(f"operator must be a ContinuousOperator, not {type(operator).__name__}")
        if operator.params != tuple(float(p) for p in model.params) or operator.shapes != shapes or \
                not all(np.array_equal(a, b) for a, b in zip(operator.grids, grids)):
            raise ValueError("operator was built on other parameters or grids than (model, grids)")
    else:
        d = _count(d, "d", 1, 64)
        if d ** nd > 1 << 24:
            raise ValueError(f"d = {d}: the tensor rule has {d ** nd} > 2^24 nodes")
    if why_w is None:
        _check_w_star(w_star)
    else:
        _check_w_star(w_star, why_w)
    return kind, grids, shapes, d


def _cont_operator(model, grids, operator, d, device):
    """The given ``ContinuousOperator``, or one built with ``qnwnorm([d] * D)``."""
    if operator is not None:
        return operator
    from .continuous import ContinuousOperator, qnwnorm
    nodes, weights = qnwnorm([d] * len(grids))
    return ContinuousOperator(np.array(model.params), grids, np.ascontiguousarray(nodes.T), weights, device=int(device))


def _cont_sync(op):
    import torch
    torch.cuda.current_stream(torch.device("cuda", op.device)).synchronize()   # (the library runs on the operator's own stream)


def sdf_moments_continuous(model, grids, w_star, *, operator=None, d=5, device=0):
    """``sdf_moments`` for the continuous-state model: {"E_M", "log_rf", "max_sharpe"} on the grid (host arrays) at the
    grid function ``w_star`` (on ``grids``, as ``wc_ratio_continuous`` returns them).  operator: a ``ContinuousOperator``
    on these parameters and grids, whose nodes and weights define the expectation; otherwise one is built with
    ``qnwnorm([d] * D)`` on ``device`` (as in ``simulate_continuous``)."""
    import torch
    _, grids, _, d = _cont_model_request(model, grids, w_star, operator, d)
    op = _cont_operator(model, grids, operator, d, device)
    w = _device_grid(op, w_star, "w_star")
    one = _ones(w)
    em, em2 = torch.empty_like(w), torch.empty_like(w)
    _cont_sync(op)
    op.cont_set_tilt_dev(w.data_ptr(), 1, model.θ, -model.γ)
    op.cont_apply_tilted_dev(one.data_ptr(), em.data_ptr())
    op.cont_set_tilt_dev(w.data_ptr(), 2, 2.0 * model.θ, -2.0 * model.γ)
    op.cont_apply_tilted_dev(one.data_ptr(), em2.data_ptr())
    op.synchronize()
    E_M = em.cpu().numpy()
    E_M2 = em2.cpu().numpy()
    return {"E_M": E_M, "log_rf": -np.log(E_M), "max_sharpe": np.sqrt(np.maximum(E_M2 / E_M ** 2 - 1.0, 0.0))}


def term_structure_continuous(model, grids, w_star, n_max, kappa=0.0, *, states=None, save=(), operator=None, d=5, device=0):
    """``term_structure`` for the continuous-state model: zero-coupon claims on G_c^κ for horizons 1 ... n_max,
    P_n = K(1, θ, κ−γ) P_{n−1}, P_0 = 1, on the device.  states: None (the zero state) or an array (nq, D) of query
    states, at which P_n is interpolated as ``lin_interp`` does (coordinates clamped to the grid).  Returns {"horizons",
    "price": (n_max, nq), "yield": −ln price / n, "bracket": (n_max, 2) min and max of P_n / P_{n−1} over the grid (they
    bracket r(K)), "grids": {n: P_n} for n in ``save``}.  operator, d, device: as in ``sdf_moments_continuous``."""
    import torch
    req = {}

    def own(nd, shapes):
        if isinstance(n_max, bool) or not isinstance(n_max, (int, np.integer)) or not 1 <= int(n_max) <= 1 << 24:
            raise ValueError(f"n_max must be an integer in 1 ... 2^24, got {n_max!r}")
        req["k"] = _kappa(kappa)
        try:
            sv = sorted({int(n) for n in save})
        except (TypeError, ValueError):
            raise ValueError(f"save must be a collection of horizons, got {save!r}") from None
        for n in sv:
            if not 1 <= n <= int(n_max):
                raise ValueError(f"save horizon {n} lies outside 1 ... n_max = {int(n_max)}")
        req["save"] = sv
        if states is None:
            st = np.zeros((1, nd))
        else:
            try:
                st = np.ascontiguousarray(np.asarray(states, dtype=np.float64))
            except (TypeError, ValueError):
                raise ValueError(f"states must be None or an array (nq, {nd})") from None
            if st.ndim != 2 or st.shape[1] != nd or st.shape[0] < 1 or st.shape[0] > 1 << 24:
                raise ValueError(f"states has shape {st.shape}: (nq, {nd}) with 1 ... 2^24 states")
            if not np.all(np.isfinite(st)):
                raise ValueError("states must be finite")
        req["states"] = st

    _, grids, _, d = _cont_model_request(model, grids, w_star, operator, d, own)
    n_max, k, save, st = int(n_max), req["k"], req["save"], req["states"]
    op = _cont_operator(model, grids, operator, d, device)
    w = _device_grid(op, w_star, "w_star")
    saved = [torch.empty_like(w) for _ in save]
    _cont_sync(op)
    op.cont_set_tilt_dev(w.data_ptr(), 1, model.θ, k - model.γ)
    try:
        price, bracket = op.cont_tilted_horizons_dev(n_max, st, save, [t.data_ptr() for t in saved])
    except SdfsError as e:
        if f"error {SDFS_ERR_NUMERIC}:" in str(e):
            raise ValueError(f"the claim prices left the positive numbers (underflow or overflow): {e}") from None
        raise
    horizons = np.arange(1, n_max + 1)
    return {"horizons": horizons, "price": price, "yield": -np.log(price) / horizons[:, None], "bracket": bracket,
            "grids": {n: t.cpu().numpy() for n, t in zip(save, saved)}}


def claim_prices_continuous(model, grids, w_star, kappa, *, rtol=1e-10, operator=None, d=5, device=0):
    """``claim_prices`` for the continuous-state model: the perpetual claim on G_c^κ, {"pd": v = (I − K)⁻¹ K·1 with
    K = K(1, θ, κ−γ), "expected_return": E_x[R] = K(0, 0, κ)(1 + v) / v, "log_premium": log E_x[R] + log E_x[M]} on the
    grid (host arrays).  At κ = 1 and a fixed point w*, v = w* − 1.  ValueError ("no finite price: r(K) ≥ 1") when the
    solve has no strictly positive solution.  operator, d, device: as in ``sdf_moments_continuous``."""
    import torch
    req = {}

    def own(nd, shapes):
        req["k"] = _kappa(kappa)
        try:
            r = float(rtol)
        except (TypeError, ValueError):
            raise ValueError(f"rtol must be positive, got {rtol!r}") from None
        if not (r > 0.0 and math.isfinite(r)):
            raise ValueError(f"rtol must be positive, got {rtol!r}")
        req["rtol"] = r

    _, grids, _, d = _cont_model_request(model, grids, w_star, operator, d, own)
    k, rtol = req["k"], req["rtol"]
    op = _cont_operator(model, grids, operator, d, device)
    w = _device_grid(op, w_star, "w_star")
    one = _ones(w)
    k1, v, num, em, er = (torch.empty_like(w) for _ in range(5))
    _cont_sync(op)
    op.cont_set_tilt_dev(w.data_ptr(), 1, model.θ, k - model.γ)
    op.cont_apply_tilted_dev(one.data_ptr(), k1.data_ptr())
    try:
        op.cont_solve_tilted_dev(k1.data_ptr(), v.data_ptr(), rtol)
    except SdfsError as e:
        if f"error {SDFS_ERR_NUMERIC}:" in str(e):
            raise ValueError(f"no finite price: r(K) ≥ 1, or (I − K) too close to singular for the solve ({e})") from None
        raise
    if not bool(torch.all(v > 0)):                       # (the solve ended with a host synchronisation)
        raise ValueError("no finite price: r(K) ≥ 1 (the solution of (I − K) v = K·1 is not strictly positive)")
    torch.add(v, 1.0, out=num)
    _cont_sync(op)
    op.cont_set_tilt_dev(None, 0, 0.0, k)
    op.cont_apply_tilted_dev(num.data_ptr(), er.data_ptr())
    op.cont_set_tilt_dev(w.data_ptr(), 1, model.θ, -model.γ)
    op.cont_apply_tilted_dev(one.data_ptr(), em.data_ptr())
    op.synchronize()
    ER = (er / v).cpu().numpy()
    return {"pd": v.cpu().numpy(), "expected_return": ER, "log_premium": np.log(ER) + np.log(em.cpu().numpy())}


__all__ = ["stationary_weights", "sdf_moments", "term_structure", "claim_prices", "sdf_moments_continuous",
           "term_structure_continuous", "claim_prices_continuous"]

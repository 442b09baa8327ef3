"""
The numpy twin of the price sensitivities (sdfs_tilt_tangent_dev, ``price_sensitivities``), on ``folded_K``
and ``pieces`` of tests/test_pricing_cpu.py:

  ``tilt_tangent``              d(K f) along a direction that moves the parameters, the state arrays, the transition
                                matrices (dQ_k = G_k Q_k), the tilt's exponents, w, Tw and f, and its "abs companion"
                                |u2| |Kf| + K(|u1 f| + |df|) + the generator with absolute values (the scale of the rounding
                                of any evaluation of the formula);
  ``param_tangent``             the tangent of T at a fixed w along the same direction;
  ``price_sensitivities_dense`` the whole chain with dense matrices: dw* = (I − J)⁻¹ ∂T, then the price formulas with
                                ``numpy.linalg.solve`` on I − K;
  ``prices_dense``              the prices themselves, and ``newton_dense`` the dense Newton solve of w*, for difference
                                quotients of the whole pipeline.
"""
import numpy as np

from test_pricing_cpu import folded_K, oracle_T, pieces

# the places of (β, γ, ψ, μ_c) in params and of (h_λ, σ_c, z) in arrays
PLACES = {"ssy": ((0, 1, 2, 3), (0, 8, 6)), "gcy": ((0, 2, 1, 5), (13, 9, 0))}


def direction_pieces(kind, shapes, direction):
    """(dβ, dγ, dψ, dμ_c, dh_λ, dσ_c, dz) of a direction (dparams, darrays, dgen), the arrays broadcast as ``pieces``."""
    dp, da = direction[0], direction[1]
    (ib, ig, ips, imu), (il, ic, iz) = PLACES[kind]

    def arr(i):
        return None if da is None or da[i] is None else np.asarray(da[i], dtype=np.float64)
    dhl, dsc, dz = arr(il), arr(ic), arr(iz)
    if kind == "ssy":
        dhl = 0.0 if dhl is None else dhl[:, None, None, None]
        dsc = 0.0 if dsc is None else dsc[None, :, None, None]
        dz = 0.0 if dz is None else dz[None, None, :, :]
    else:
        dhl = 0.0 if dhl is None else dhl[None, None, None, None, None, :]
        dsc = 0.0 if dsc is None else dsc[None, None, None, :, None, None]
        dz = 0.0 if dz is None else np.transpose(dz, (3, 0, 1, 2))[:, :, :, None, :, None]
    return dp[ib], dp[ig], dp[ips], dp[imu], dhl, dsc, dz


def dtheta_of(kind, model, direction):
    (_, ig, ips, _), _ = PLACES[kind]
    psi = model.params[ips]
    dp = direction[0]
    return -dp[ig] / (1.0 - 1.0 / psi) - dp[ips] * model.θ / (psi * (psi - 1.0))


def along_axis(gen, x, axis, absolute=False):
    """G x along one axis, G by its (3, n) sub-, main and super-diagonal (by row)."""
    g = np.abs(gen) if absolute else gen
    x = np.moveaxis(np.abs(x) if absolute else x, axis, -1)
    out = g[1] * x
    out[..., 1:] += g[0][1:] * x[..., :-1]
    out[..., :-1] += g[2][:-1] * x[..., 1:]
    return np.moveaxis(out, -1, axis)


def row_factor(kind, shapes, model, arrays, Tw, p, kc):
    """R = [β^θ (Tw − 1)^(1−θ)]^p exp(½ κ_c² σ_c² + κ_c (μ_c + z)) on the grid."""
    beta, theta, _, mu_c, _, sc, zz, _ = pieces(kind, model, arrays)
    return (beta ** theta * (Tw - 1.0) ** (1.0 - theta)) ** p * np.broadcast_to(
        np.exp(0.5 * kc * kc * sc * sc + kc * (mu_c + zz)), shapes)


def tilt_tangent(kind, shapes, model, arrays, w, Tw, f, p, kl, kc, direction, dkl, dkc, dw, dTw, df):
    """(d(K f), abs companion) of K = K(p, κ_λ, κ_c) at (w, Tw) along ``direction`` = (dparams, darrays, dgen), with the
    exponents moved by (dkl, dkc), w by dw, Tw by dTw and f by df."""
    beta, theta, _, mu_c, hl, sc, zz, _ = pieces(kind, model, arrays)
    dbeta, _, _, dmu, dhl, dsc, dz = direction_pieces(kind, shapes, direction)
    dth = dtheta_of(kind, model, direction)
    u1 = dkl * hl + kl * dhl + np.zeros(shapes)
    u2 = kc * dkc * sc * sc + kc * kc * sc * dsc + dkc * (mu_c + zz) + kc * (dmu + dz) + np.zeros(shapes)
    if p:
        u1 = u1 + p * (dth * np.log(w) + (theta - 1.0) * dw / w)
        u2 = u2 + p * (theta * dbeta / beta + dth * np.log(beta) - dth * np.log(Tw - 1.0) + (1.0 - theta) * dTw / (Tw - 1.0))

    def K(x):
        return folded_K(kind, shapes, model, arrays, w, x, p, kl, kc, Tw=Tw)
    Kf = K(f)
    val = u2 * Kf + K(u1 * f + df)
    comp = np.abs(u2) * np.abs(Kf) + K(np.abs(u1 * f) + np.abs(df))
    dgen = direction[2] if len(direction) > 2 else None
    if dgen is not None:
        R = row_factor(kind, shapes, model, arrays, Tw, p, kc)
        for a, g in enumerate(dgen):
            if g is not None:
                val = val + R * along_axis(g, Kf / R, a)
                comp = comp + R * along_axis(g, Kf / R, a, absolute=True)
    return val, comp


def param_tangent(kind, shapes, model, arrays, w, Tw, jv, direction):
    """∂T at a fixed w along ``direction`` (the formula of csrc/sens_kernels.hpp); jv(x) = J(w) x."""
    beta, theta, gamma, mu_c, hl, sc, zz, _ = pieces(kind, model, arrays)
    dbeta, dg, _, dmu, dhl, dsc, dz = direction_pieces(kind, shapes, direction)
    dth = dtheta_of(kind, model, direction)
    og = 1.0 - gamma
    dla1 = dth * hl + theta * dhl
    dla2 = og * sc * (og * dsc - dg * sc)
    dla3 = og * (dmu + dz) - dg * (mu_c + zz)
    e = Tw - 1.0
    out = e * (dbeta / beta - dth / theta * np.log(e / beta) + (dla2 + dla3) / theta) + jv(w * (dth * np.log(w) + dla1)) / theta
    dgen = direction[2] if len(direction) > 2 else None
    if dgen is not None:
        E = (e / beta) ** theta / np.exp(0.5 * (og * sc) ** 2 + og * (mu_c + zz))
        for a, g in enumerate(dgen):
            if g is not None:
                out = out + e / theta * along_axis(g, E, a) / E
    return out


def dense_of(apply, shapes):
    """The N × N matrix of a linear map on the grid, from unit vectors."""
    N = int(np.prod(shapes))
    M = np.empty((N, N))
    for k in range(N):
        e = np.zeros(N)
        e[k] = 1.0
        M[:, k] = apply(e.reshape(shapes)).ravel()
    return M


def dense_tilt(kind, shapes, model, arrays, w, Tw, p, kl, kc):
    return dense_of(lambda x: folded_K(kind, shapes, model, arrays, w, x, p, kl, kc, Tw=Tw), shapes)


def newton_dense(kind, shapes, model, arrays, w, iters=8):
    """w* by Newton with the dense I − J(w), J = K(1, θ, 1−γ)."""
    N = w.size
    for _ in range(iters):
        Tw = oracle_T(kind, shapes, model, arrays, w)
        r = Tw - w
        if np.max(np.abs(r)) <= 1e-13 * np.max(np.abs(w)):
            break
        J = dense_tilt(kind, shapes, model, arrays, w, Tw, 1, model.θ, 1.0 - model.γ)
        w = w + np.linalg.solve(np.eye(N) - J, r.ravel()).reshape(shapes)
    return w


def prices_dense(kind, shapes, model, arrays, w, kappa=None):
    """The fields of ``sdf_moments`` (and of ``claim_prices(kappa)``) with dense matrices, plus "_K": the dense
    K(1, θ, κ−γ)."""
    th, g = model.θ, model.γ
    N = w.size
    one = np.ones(shapes)
    Tw = oracle_T(kind, shapes, model, arrays, w)
    E_M = folded_K(kind, shapes, model, arrays, w, one, 1, th, -g, Tw=Tw)
    E_M2 = folded_K(kind, shapes, model, arrays, w, one, 2, 2 * th, -2 * g, Tw=Tw)
    out = {"E_M": E_M, "log_rf": -np.log(E_M), "max_sharpe": np.sqrt(np.maximum(E_M2 / E_M ** 2 - 1.0, 0.0))}
    if kappa is not None:
        K = dense_tilt(kind, shapes, model, arrays, w, Tw, 1, th, kappa - g)
        v = np.linalg.solve(np.eye(N) - K, K @ np.ones(N)).reshape(shapes)
        E_R = folded_K(kind, shapes, model, arrays, w, 1.0 + v, 0, 0.0, kappa, Tw=Tw) / v
        out.update({"pd": v, "expected_return": E_R, "log_premium": np.log(E_R) + np.log(E_M), "_K": K})
    return out


def price_sensitivities_dense(kind, shapes, model, arrays, w, kappa, directions):
    """{name: {field: derivative}} for ``directions`` = {name: (dparams, darrays, dgen or None)} at the fixed point w:
    dw* from the dense (I − J)⁻¹ on the twin's ∂T, the price formulas of DESIGN §4.19 with ``numpy.linalg.solve``.  Also
    "_dw": {name: dw*} and, with a kappa, "_K": the dense K(1, θ, κ−γ)."""
    th, g = model.θ, model.γ
    N = w.size
    one = np.ones(shapes)
    zero = np.zeros(shapes)
    Tw = oracle_T(kind, shapes, model, arrays, w)
    J = dense_tilt(kind, shapes, model, arrays, w, Tw, 1, th, 1.0 - g)
    A = np.eye(N) - J
    base = prices_dense(kind, shapes, model, arrays, w, kappa)
    E_M = base["E_M"]
    E_M2 = folded_K(kind, shapes, model, arrays, w, one, 2, 2 * th, -2 * g, Tw=Tw)
    q = E_M2 / E_M ** 2
    S = np.sqrt(np.maximum(q - 1.0, 0.0))
    out = {"_dw": {}}
    if kappa is not None:
        K, v, E_R = base["_K"], base["pd"], base["expected_return"]
        out["_K"] = K
    (_, ig, _, _), _ = PLACES[kind]
    for name, d in directions.items():
        d = tuple(d) + (None,) * (3 - len(d))
        dT = param_tangent(kind, shapes, model, arrays, w, Tw, lambda x: (J @ x.ravel()).reshape(shapes), d)
        dw = np.linalg.solve(A, dT.ravel()).reshape(shapes)
        out["_dw"][name] = dw
        dth, dg = dtheta_of(kind, model, d), d[0][ig]

        def dK(p, kl, kc, dkl, dkc, f, df):
            return tilt_tangent(kind, shapes, model, arrays, w, Tw, f, p, kl, kc, d, dkl, dkc, dw, dw, df)[0]
        dEM = dK(1, th, -g, dth, -dg, one, zero)
        dEM2 = dK(2, 2 * th, -2 * g, 2 * dth, -2 * dg, one, zero)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = {"E_M": dEM, "log_rf": -dEM / E_M,
                 "max_sharpe": np.where(S > 0, q / (2 * S) * (dEM2 / E_M2 - 2 * dEM / E_M), np.nan)}
        if kappa is not None:
            b = dK(1, th, kappa - g, dth, -dg, 1.0 + v, zero)
            dv = np.linalg.solve(np.eye(N) - K, b.ravel()).reshape(shapes)
            dER = dK(0, 0.0, kappa, 0.0, 0.0, 1.0 + v, dv) / v - E_R * dv / v
            r.update({"pd": dv, "expected_return": dER, "log_premium": dER / E_R + dEM / E_M})
        out[name] = r
    return out

"""
Numpy twin of the continuous-state simulation (sdfs_via_autodiff_amd/simulation.py ``simulate_continuous``):
Philox4x32-10 with counter (t, p, b, 1) and Box–Muller normals, the reference's ``next_state`` (oracle/continuous.py),
``lin_interp`` of w and of −ln E_x[M] along the states, the series, and the per-path statistics computed two-pass from
the stored series.  E_x[M] on the grid is the formula of DESIGN §4.14 on ``next_state`` and ``lin_interp``.

``dtype=np.longdouble`` runs the normals, the state recursion and the series in extended precision (the interpolation
itself stays scipy's fp64 ``map_coordinates``, at the extended states rounded to fp64): the distance between the two
twins measures how far rounding alone moves these series.
"""
import numpy as np

from oracle import continuous as OC
import sim_oracle as so

SERIES = ("dc", "m", "rf", "rc", "xc", "wc")


def pieces(kind, params):
    """(theta, beta, gamma, mu_c, phi_c, index of z, index of h_c, rho_lambda, s_lambda, next_state)."""
    p = tuple(float(q) for q in params)
    if kind == "ssy":
        beta, gamma, psi, mu_c, phi_c, rho_l, s_l = p[0], p[1], p[2], p[3], p[6], p[9], p[12]
        iz, nxt = 3, OC.next_state_ssy
    else:
        beta, psi, gamma, rho_l, s_l, mu_c, phi_c = p[0], p[1], p[2], p[3], p[4], p[5], p[6]
        iz, nxt = 4, OC.next_state_gcy
    theta = (1 - gamma) / (1 - 1 / psi)
    return theta, beta, gamma, mu_c, phi_c, iz, 1, rho_l, s_l, nxt


def two_pi(dtype):
    return dtype(8) * np.arctan(dtype(1)) if dtype is np.longdouble else dtype(2.0 * np.pi)


def normals(seed, t, paths, ndim, dtype=np.float64, with_xi=True):
    """(eta (ndim, P), xi (P,) or None) of step t: block b's words r0 … r3 give n_4b … n_4b+3."""
    key = (seed & 0xFFFFFFFF, seed >> 32)
    p = np.asarray(paths, dtype=np.uint64)
    r = so.philox4x32_10((t, p, 0, 1), key) + so.philox4x32_10((t, p, 1, 1), key)
    need = ndim + (1 if with_xi else 0)
    n = []
    for k in range(need):
        a, b = r[2 * (k // 2)], r[2 * (k // 2) + 1]
        u = (a.astype(dtype) + dtype(0.5)) * dtype(2.0 ** -32)
        phi = two_pi(dtype) * (b.astype(dtype) * dtype(2.0 ** -32))
        rad = np.sqrt(dtype(-2.0) * np.log(u))
        n.append(rad * (np.cos(phi) if k % 2 == 0 else np.sin(phi)))
    return np.stack(n[:ndim]), (n[ndim] if with_xi else None)


def state_paths(kind, params, ndim, seed, path_offset, n_paths, burn_in, n_periods, step_offset=0, start=None,
                dtype=np.float64):
    """(x (P, T+1, D) for t = B … B+T, xi (P, T)), both of ``dtype``."""
    nxt = pieces(kind, params)[-1]
    par = tuple(float(q) for q in params)
    paths = np.arange(path_offset, path_offset + n_paths, dtype=np.uint64)
    if start is None:
        x = np.zeros((ndim, n_paths), dtype=dtype)
    else:
        st = np.asarray(start, dtype=dtype)
        x = np.ascontiguousarray(np.broadcast_to(st, (n_paths, ndim)).T) if st.ndim == 1 else np.ascontiguousarray(st.T)
    X = np.empty((n_paths, n_periods + 1, ndim), dtype=dtype)
    xi = np.empty((n_paths, n_periods), dtype=dtype)
    for k in range(1, burn_in + n_periods + 1):
        if k == burn_in + 1:
            X[:, 0, :] = x.T
        eta, z = normals(seed, step_offset + k, paths, ndim, dtype, with_xi=k > burn_in)
        x = nxt(par, x, eta)
        if k > burn_in:
            X[:, k - burn_in, :] = x.T
            xi[:, k - burn_in - 1] = z
    return X, xi


def sdf_mean(kind, params, grids, w, nodes, weights=None):
    """E_x[M] on the grid: nodes (D, M) as the reference passes them, weights None = Monte Carlo (1 / M)."""
    theta, beta, gamma, mu_c, phi_c, iz, ihc, _, _, nxt = pieces(kind, params)
    par = tuple(float(q) for q in params)
    w = np.asarray(w, dtype=np.float64)
    nodes = np.asarray(nodes, dtype=np.float64)
    M = nodes.shape[1]
    wts = np.full(M, 1.0 / M) if weights is None else np.asarray(weights, dtype=np.float64)
    mesh = np.meshgrid(*grids, indexing="ij")
    X = np.stack([m.ravel() for m in mesh], axis=1)
    out = np.empty(X.shape[0])
    wf = w.ravel()
    for i, x in enumerate(X):
        nx = nxt(par, x, nodes)
        g = OC.lin_interp(nx, w, grids)
        sig_c = phi_c * np.exp(x[ihc])
        c = np.exp(-gamma * (mu_c + x[iz]) + 0.5 * gamma ** 2 * sig_c ** 2)
        with np.errstate(invalid="ignore"):
            out[i] = beta ** theta * (wf[i] - 1.0) ** (1.0 - theta) * c * np.dot(wts * np.exp(theta * nx[0]), g ** (theta - 1.0))
    return out.reshape(w.shape)


def sdf_mean_constant_w(kind, params, grids, c):
    """The closed form of E_x[M] for w ≡ c (exact under the normal law of the h_λ shock)."""
    theta, beta, gamma, mu_c, phi_c, iz, ihc, rho_l, s_l, _ = pieces(kind, params)
    mesh = np.meshgrid(*grids, indexing="ij")
    sig_c = phi_c * np.exp(mesh[ihc])
    return beta ** theta * (c - 1.0) ** (1.0 - theta) * c ** (theta - 1.0) * np.exp(
        -gamma * (mu_c + mesh[iz]) + 0.5 * gamma ** 2 * sig_c ** 2 + theta * rho_l * mesh[0] + 0.5 * theta ** 2 * s_l ** 2)


def interp_along(X, f, grids):
    """lin_interp of the grid function f at the states X (P, T+1, D) -> (P, T+1), fp64."""
    P, T1, D = X.shape
    pts = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(P * T1, D).T)
    return OC.lin_interp(pts, np.asarray(f, dtype=np.float64), grids).reshape(P, T1)


def series(kind, params, grids, X, xi, w, em, dtype=np.float64):
    """The series of DESIGN §4.14 along states X (P, T+1, D) with draws xi (P, T): ({name: (P, T)}, slope regressor)."""
    theta, beta, gamma, mu_c, phi_c, iz, ihc, _, _, _ = pieces(kind, params)
    wh = interp_along(X, w, grids).astype(dtype)
    rf = interp_along(X, -np.log(np.asarray(em, dtype=np.float64)), grids).astype(dtype)
    X = np.asarray(X, dtype=dtype)
    th, gm = dtype(theta), dtype(gamma)
    lw, lw1 = np.log(wh[:, 1:]), np.log(wh[:, :-1] - dtype(1.0))
    dc = dtype(mu_c) + X[:, :-1, iz] + dtype(phi_c) * np.exp(X[:, :-1, ihc]) * np.asarray(xi, dtype=dtype)
    rl = lw - lw1
    out = {"dc": dc,
           "m": th * np.log(dtype(beta)) + th * X[:, 1:, 0] - gm * dc + (th - dtype(1.0)) * rl,
           "rf": rf[:, :-1],
           "rc": dc + rl}
    out["xc"] = out["rc"] - out["rf"]
    out["wc"] = wh[:, 1:]
    return out, lw1


def outside(grids, X, rel=1e-12):
    """(outside (P, T+1): some coordinate of the state lies outside the grid; near (P, T+1): some coordinate lies
    within rel × the grid's span of an edge, where rounding decides the side)."""
    X = np.asarray(X, dtype=np.float64)
    out = np.zeros(X.shape[:2], dtype=bool)
    near = np.zeros(X.shape[:2], dtype=bool)
    for d, g in enumerate(grids):
        c = (X[..., d] - g[0]) / (g[1] - g[0])
        out |= (c < 0.0) | (c > len(g) - 1)
        span = g[-1] - g[0]
        near |= (np.abs(X[..., d] - g[0]) <= rel * span) | (np.abs(X[..., d] - g[-1]) <= rel * span)
    return out, near


def statistics(ser, xr):
    out = {}
    for nm, s in ser.items():
        m, sd, a = so.two_pass(np.asarray(s, dtype=np.float64))
        out[nm] = {"mean": m, "std": sd, "ac1": a}
    out["slope"] = so.ols_slope(np.asarray(xr, dtype=np.float64), np.asarray(ser["xc"], dtype=np.float64))
    return out


def simulate(kind, params, grids, w, em, seed=0, path_offset=0, n_paths=1, burn_in=0, n_periods=2, step_offset=0,
             start=None, dtype=np.float64):
    """{"state" (P, T+1, D), "series", "stats", "clamped" (P,) counts over the recorded steps, "near_edge" (P, T) mask,
    "final_state"} of the numpy twin."""
    X, xi = state_paths(kind, params, len(grids), seed, path_offset, n_paths, burn_in, n_periods, step_offset, start, dtype)
    ser, xr = series(kind, params, grids, X, xi, w, em, dtype)
    out, near = outside(grids, X)
    return {"state": X, "series": ser, "stats": statistics(ser, xr), "outside": out[:, 1:],
            "clamped": out[:, 1:].sum(axis=1), "near_edge": near[:, 1:], "final_state": X[:, -1, :]}


def close(a, b, tol):
    """sim_oracle's measure of test_hip_simulation.py: max |a − b| / max(|b|, tol), NaN against NaN counting as equal."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    err = np.abs(a - b) / np.maximum(np.abs(b), tol)
    err[both_nan] = 0.0
    return float(np.max(err))

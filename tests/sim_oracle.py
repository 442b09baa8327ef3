"""
Numpy twin of the simulation (sdfs_via_autodiff_amd/simulation.py): Philox4x32-10 vectorised over paths
on uint64 arrays, the inverse-CDF index draws on the same host tables, the series, and the per-path statistics computed
two-pass from the stored series.  Index paths agree with the device bit for bit; series up to libm's log and cos.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two.  Returns the four output words (uint64 arrays)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in counter)
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = M0 * c0
        p1 = M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + W0) & MASK
        k1 = (k1 + W1) & MASK
    return c0, c1, c2, c3


def unit(r):
    """u = (r + 0.5) 2^-32: exact in fp64, in (0, 1)."""
    return (np.asarray(r, dtype=np.float64) + 0.5) * 2.0 ** -32


def words(t, paths, seed):
    """The eight words r0 ... r7 of step t for every path number in ``paths``."""
    key = (seed & 0xFFFFFFFF, seed >> 32)
    p = np.asarray(paths, dtype=np.uint64)
    a = philox4x32_10((t, p, 0, 0), key)
    b = philox4x32_10((t, p, 1, 0), key)
    return a + b


def draw(rows, u):
    """Least j with u < rows[:, j] (rows: one cumulative row per path)."""
    return np.sum(rows[:, :-1] <= u[:, None], axis=1)


def index_paths(cdf, cdf0, seed, path_offset, n_paths, burn_in, n_periods, start=None):
    """(idx (P, T+1, d) for t = B ... B+T, xi (P, T) for t = B+1 ... B+T)."""
    d = len(cdf)
    paths = np.arange(path_offset, path_offset + n_paths, dtype=np.uint64)
    if start is None:
        r = words(0, paths, seed)
        ix = [draw(np.broadcast_to(cdf0[a], (n_paths, cdf0[a].size)), unit(r[a])) for a in range(d)]
    else:
        ix = [np.full(n_paths, s, dtype=np.int64) for s in start]
    idx = np.empty((n_paths, n_periods + 1, d), dtype=np.uint8)
    xi = np.empty((n_paths, n_periods))
    for t in range(1, burn_in + n_periods + 1):
        if t == burn_in + 1:
            idx[:, 0, :] = np.stack(ix, axis=1)
        r = words(t, paths, seed)
        ix = [draw(cdf[a][ix[a]], unit(r[a])) for a in range(d)]
        if t > burn_in:
            idx[:, t - burn_in, :] = np.stack(ix, axis=1)
            u, u2 = unit(r[6]), np.asarray(r[7], dtype=np.float64) * 2.0 ** -32
            xi[:, t - burn_in - 1] = np.sqrt(-2.0 * np.log(u)) * np.cos(2 * np.pi * u2)
    if burn_in + n_periods == 0:
        idx[:, 0, :] = np.stack(ix, axis=1)
    return idx, xi


def model_pieces(kind, params, arrays, shapes):
    """(theta, beta, gamma, h_lam axis values and axis, sigma_c values and axis, mu_c + z on the grid)."""
    if kind == "ssy":
        beta, gamma, psi, mu_c = params[0], params[1], params[2], params[3]
        hl, ax_l, sc, ax_c = np.asarray(arrays[0]), 0, np.asarray(arrays[8]), 1
        z = np.asarray(arrays[6]).reshape(shapes[2], shapes[3])
        muz = np.broadcast_to((mu_c + z)[None, None, :, :], shapes)
    else:
        beta, psi, gamma, mu_c = params[0], params[1], params[2], params[5]
        hl, ax_l, sc, ax_c = np.asarray(arrays[13]), 5, np.asarray(arrays[9]), 3
        z = np.asarray(arrays[0]).reshape(shapes[1], shapes[2], shapes[4], shapes[0])      # [z_pi, h_z, h_zpi, z]
        zg = np.transpose(z, (3, 0, 1, 2))                                                  # [z, z_pi, h_z, h_zpi]
        muz = np.broadcast_to((mu_c + zg)[:, :, :, None, :, None], shapes)
    theta = (1 - gamma) / (1 - 1 / psi)
    return theta, beta, gamma, hl, ax_l, sc, ax_c, np.ascontiguousarray(muz)


def series(kind, params, arrays, shapes, idx, xi, w, em, v=None, kappa=None):
    """The series of DESIGN §4.8 along index paths idx (P, T+1, d) with normal draws xi (P, T): {name: (P, T)}, and
    the slope regressor x_{t-1} (P, T)."""
    th, beta, gamma, hl, ax_l, sc, ax_c, muz = model_pieces(kind, params, arrays, shapes)
    flat = np.ravel_multi_index(tuple(idx[..., a].astype(np.int64) for a in range(idx.shape[-1])), shapes)
    prev, nxt = flat[:, :-1], flat[:, 1:]
    w = np.asarray(w, dtype=np.float64).ravel()
    lw, lw1, nlem, mz = np.log(w), np.log(w - 1.0), -np.log(np.asarray(em, dtype=np.float64).ravel()), muz.ravel()
    dc = mz[prev] + sc[idx[:, :-1, ax_c]] * xi
    rl = lw[nxt] - lw1[prev]
    out = {"dc": dc,
           "m": th * np.log(beta) + th * hl[idx[:, 1:, ax_l]] - gamma * dc + (th - 1.0) * rl,
           "rf": nlem[prev],
           "rc": dc + rl}
    out["xc"] = out["rc"] - out["rf"]
    out["wc"] = w[nxt]
    xr = lw1[prev]
    if kappa is not None:
        lv = np.log(np.asarray(v, dtype=np.float64).ravel())
        l1v = np.log(1.0 + np.asarray(v, dtype=np.float64).ravel())
        out["rd"] = kappa * dc + l1v[nxt] - lv[prev]
        out["xd"] = out["rd"] - out["rf"]
        out["pd"] = lv[nxt]
        xr = lv[prev]
    return out, xr


def two_pass(s):
    """Per-row mean, std = √(Σ(s−mean)²/T), ac1 = Σ_{t≥2}(s_t−mean)(s_{t−1}−mean) / Σ(s_t−mean)² (NaN for a zero
    denominator), each two-pass on the row shifted by its first value."""
    s = np.asarray(s, dtype=np.float64)
    d = s - s[:, :1]
    md = d.mean(axis=1)
    e = d - md[:, None]
    den = np.sum(e * e, axis=1)
    num = np.sum(e[:, 1:] * e[:, :-1], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ac1 = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)
    return s[:, 0] + md, np.sqrt(den / s.shape[1]), ac1


def ols_slope(x, y):
    """Per-row OLS slope of y on x (NaN for a regressor without variation), two-pass on shifted rows."""
    dx = x - x[:, :1]
    dy = y - y[:, :1]
    ex = dx - dx.mean(axis=1)[:, None]
    ey = dy - dy.mean(axis=1)[:, None]
    sxx = np.sum(ex * ex, axis=1)
    sxy = np.sum(ex * ey, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(sxx > 0, sxy / np.where(sxx > 0, sxx, 1.0), np.nan)


def statistics(ser, xr, kappa=None):
    """{name: {"mean", "std", "ac1"}, "slope"} of the series dict ``ser``."""
    out = {}
    for nm, s in ser.items():
        m, sd, a = two_pass(s)
        out[nm] = {"mean": m, "std": sd, "ac1": a}
    out["slope"] = ols_slope(xr, ser["xd" if kappa is not None else "xc"])
    return out


def simulate(kind, params, arrays, shapes, cdf, cdf0, w, em, v=None, kappa=None, seed=0, path_offset=0, n_paths=1,
             burn_in=0, n_periods=2, start=None):
    """(idx, series, stats) of the numpy twin."""
    idx, xi = index_paths(cdf, cdf0, seed, path_offset, n_paths, burn_in, n_periods, start)
    ser, xr = series(kind, params, arrays, shapes, idx, xi, w, em, v, kappa)
    return idx, ser, statistics(ser, xr, kappa)

"""
Numpy twin of the continuous-state pricing operator (sdfs_via_autodiff_amd/pricing.py ``*_continuous``, csrc/cont_price.hpp,
the C_K0 / C_K1 / C_K2 forms of csrc/cont_kernel.hpp), built on the reference restatement
oracle/continuous.py (``next_state``, ``lin_interp``) and on tests/cont_sim_oracle.py (``pieces``):

    K(p, κ_λ, κ_c) f (x) = d2(x) · Σ_m W_m exp(κ_λ s_λ η_0m) · ŵ(x'_m)^(p(θ−1)) · f̂(x'_m)
    d2(x) = [β^θ (w(x) − 1)^(1−θ)]^p · exp(κ_c (μ_c + z) + ½ κ_c² σ_c(x)² + κ_λ ρ_λ h_λ)

``apply`` is the one-application twin: one pass over the grid points, every setting from the same ``next_state`` and
``lin_interp`` calls.  ``dense`` assembles the N × N matrix of K from the corner weights of the multilinear interpolant
(interpolation is linear in f), which gives K^n·1, the perpetual claim, r(K) and cond₂(I − K) by dense linear algebra.
"""
import itertools

import numpy as np

from oracle import continuous as OC
import cont_sim_oracle as co


def weights_of(nodes, weights):
    M = np.asarray(nodes).shape[1]
    return np.full(M, 1.0 / M) if weights is None else np.asarray(weights, dtype=np.float64)


def d2(kind, params, grids, w, p, kl, kc):
    """The per-point factor on the grid (NaN where p > 0 and w <= 1)."""
    theta, beta, _, mu_c, phi_c, iz, ihc, rho_l, _, _ = co.pieces(kind, params)
    mesh = np.meshgrid(*grids, indexing="ij")
    sig_c = phi_c * np.exp(mesh[ihc])
    e = np.exp(kc * (mu_c + mesh[iz]) + 0.5 * kc ** 2 * sig_c ** 2 + kl * rho_l * mesh[0])
    if p == 0:
        return e
    with np.errstate(invalid="ignore"):
        return (beta ** theta * (np.asarray(w, dtype=np.float64) - 1.0) ** (1.0 - theta)) ** p * e


def apply(kind, params, grids, w, fs, nodes, weights, settings):
    """[K(p, κ_λ, κ_c) f for (p, κ_λ, κ_c), f in zip(settings, fs)]; ``fs`` may be one grid function for every setting."""
    theta, _, _, _, _, _, _, _, s_l, nxt = co.pieces(kind, params)
    par = tuple(float(q) for q in params)
    w = np.asarray(w, dtype=np.float64)
    nodes = np.asarray(nodes, dtype=np.float64)
    if isinstance(fs, np.ndarray):
        fs = [fs] * len(settings)
    fs = [np.asarray(f, dtype=np.float64) for f in fs]
    uniq = []
    for f in fs:
        if not any(f is u for u in uniq):
            uniq.append(f)
    which = [next(i for i, u in enumerate(uniq) if u is f) for f in fs]
    W = weights_of(nodes, weights)
    wt = [W * np.exp(kl * s_l * nodes[0]) for _, kl, _ in settings]
    D2 = [d2(kind, params, grids, w, p, kl, kc).ravel() for p, kl, kc in settings]
    mesh = np.meshgrid(*grids, indexing="ij")
    X = np.stack([m.ravel() for m in mesh], axis=1)
    out = [np.empty(X.shape[0]) for _ in settings]
    for i, x in enumerate(X):
        nx = nxt(par, x, nodes)
        g = OC.lin_interp(nx, w, grids)
        fi = [OC.lin_interp(nx, f, grids) for f in uniq]
        for s, (p, _, _) in enumerate(settings):
            gp = g ** (p * (theta - 1.0)) if p else 1.0
            out[s][i] = D2[s][i] * np.dot(wt[s], gp * fi[which[s]])
    return [o.reshape(w.shape) for o in out]


def corner_weights(grids, nx):
    """(flat indices (2^D, M), weights (2^D, M)) of the multilinear interpolant with clamped coordinates at the points nx
    (D, M): map_coordinates(order=1, mode='nearest') equals interpolation at the coordinate clipped to the grid."""
    D = len(grids)
    n = [len(g) for g in grids]
    stride = [int(np.prod(n[d + 1:])) for d in range(D)]
    c = OC.vals_to_coords(grids, nx)
    i0, t = [], []
    for d in range(D):
        cc = np.clip(c[d], 0.0, n[d] - 1.0)
        lo = np.minimum(np.floor(cc).astype(np.int64), n[d] - 2)
        i0.append(lo)
        t.append(cc - lo)
    idx, wgt = [], []
    for bits in itertools.product((0, 1), repeat=D):
        k = np.zeros(nx.shape[1], dtype=np.int64)
        v = np.ones(nx.shape[1])
        for d, b in enumerate(bits):
            k += (i0[d] + b) * stride[d]
            v = v * (t[d] if b else 1.0 - t[d])
        idx.append(k)
        wgt.append(v)
    return np.stack(idx), np.stack(wgt)


def dense(kind, params, grids, w, nodes, weights, settings):
    """[the N × N matrix of K(p, κ_λ, κ_c) for each setting], rows and columns in C order of the grid."""
    theta, _, _, _, _, _, _, _, s_l, nxt = co.pieces(kind, params)
    par = tuple(float(q) for q in params)
    w = np.asarray(w, dtype=np.float64)
    nodes = np.asarray(nodes, dtype=np.float64)
    W = weights_of(nodes, weights)
    wt = [W * np.exp(kl * s_l * nodes[0]) for _, kl, _ in settings]
    D2 = [d2(kind, params, grids, w, p, kl, kc).ravel() for p, kl, kc in settings]
    mesh = np.meshgrid(*grids, indexing="ij")
    X = np.stack([m.ravel() for m in mesh], axis=1)
    N = X.shape[0]
    wf = w.ravel()
    out = [np.zeros((N, N)) for _ in settings]
    for i, x in enumerate(X):
        nx = nxt(par, x, nodes)
        idx, wgt = corner_weights(grids, nx)
        g = np.sum(wgt * wf[idx], axis=0)
        for s, (p, _, _) in enumerate(settings):
            coef = wt[s] * (g ** (p * (theta - 1.0)) if p else 1.0)
            out[s][i] = D2[s][i] * np.bincount(idx.ravel(), weights=(wgt * coef).ravel(), minlength=N)
    return out


def spectral_radius(K):
    return float(np.max(np.abs(np.linalg.eigvals(K))))


def powers_of_one(K, n_max):
    """[K^n·1 for n = 1 … n_max] (each of length N)."""
    out, p = [], np.ones(K.shape[0])
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(n_max):
            p = K @ p
            out.append(p)
    return out


def brackets(Ps):
    """(n_max, 2): min and max of P_n / P_{n−1} over the grid, P_0 = 1."""
    prev = np.ones_like(Ps[0])
    out = np.empty((len(Ps), 2))
    for n, p in enumerate(Ps):
        r = p / prev
        out[n] = r.min(), r.max()
        prev = p
    return out


def claim(K, K0, EM):
    """The perpetual claim from the dense K = K(1, θ, κ−γ), K0 = K(0, 0, κ) and E_x[M] (length N): (pd, expected
    return, log premium)."""
    N = K.shape[0]
    v = np.linalg.solve(np.eye(N) - K, K @ np.ones(N))
    er = (K0 @ (1.0 + v)) / v
    with np.errstate(invalid="ignore"):
        return v, er, np.log(er) + np.log(EM)


def closed_form_constant_w(kind, params, grids, c, nodes1, weights1, p, kl, kc):
    """K(p, κ_λ, κ_c)·1 at w ≡ c: [β^θ (c−1)^(1−θ)]^p c^(p(θ−1)) exp(κ_c(μ_c+z) + ½κ_c²σ_c² + κ_λρ_λh_λ) Σ_j W_j exp(κ_λ s_λ η_j)
    with the sum over the 1-D nodes."""
    theta, beta, _, mu_c, phi_c, iz, ihc, rho_l, s_l, _ = co.pieces(kind, params)
    mesh = np.meshgrid(*grids, indexing="ij")
    sig_c = phi_c * np.exp(mesh[ihc])
    e = np.exp(kc * (mu_c + mesh[iz]) + 0.5 * kc ** 2 * sig_c ** 2 + kl * rho_l * mesh[0])
    s = np.dot(np.asarray(weights1, dtype=np.float64), np.exp(kl * s_l * np.asarray(nodes1, dtype=np.float64)))
    return (beta ** theta * (c - 1.0) ** (1.0 - theta)) ** p * c ** (p * (theta - 1.0)) * e * s


# -- the operator cases of the issue's table: one per gather path and dimension -----------------------------------------
# (name, model, sizes, num_std_devs, rule, class, staged blocks, unstaged blocks)
CASES = [
    ("A4", "ssy", (4, 4, 4, 8), 1.0, ("gh", 3), "A", 512, 0),
    ("A6", "gcy", (2, 2, 2, 2, 6, 6), 1.0, ("gh", 3), "A", 576, 0),
    ("B4", "ssy", (4, 4, 4, 8), 1.0, ("mc", 100), "B", 512, 0),
    ("B6", "gcy", (2, 2, 2, 2, 6, 6), 0.3, ("mc", 100), "B", 576, 0),
    ("C4", "ssy", (8, 8, 8, 8), 0.2, ("gh", 3), "C", 3584, 512),
    ("C6", "gcy", (4, 4, 4, 4, 4, 4), 0.1, ("mc", 100), "C", 2048, 2048),
    ("D4", "ssy", (8, 8, 8, 8), 0.1, ("gh", 3), "D", 0, 4096),
]
CASE_IDS = [c[0] for c in CASES]


def settings_of(kind, params):
    """The three settings of the operator tests: (0, 0, 2), (1, θ, 2−γ), (2, 2θ, −2γ)."""
    theta, _, gamma = co.pieces(kind, params)[:3]
    return [(0, 0.0, 2.0), (1, theta, 2.0 - gamma), (2, 2.0 * theta, -2.0 * gamma)]


# -- the (grid, κ) pairs of the claim tests, on the grids of cont_sim_cases.GRIDS with the Gauss–Hermite rule QUAD_D -----
# tests/test_cont_pricing_cpu.py pins r(K(1, θ, κ−γ)) of the dense twin on each: below 0.9998 where a price is asked
# for, above 1.002 where a refusal is
def claim_pairs():
    import cont_sim_cases as CC
    fixed = [g for g in CC.GRIDS if g not in CC.NO_FIXED_POINT]
    return ([(g, 1.0) for g in fixed] + [(g, 0.0) for g in CC.GRIDS if g[2] == 1.0] +
            [(g, 2.0) for g in CC.GRIDS if g[0] == "ssy" and g[2] == 3.2])


def refused_pairs():
    import cont_sim_cases as CC
    return [(g, 6.0) for g in CC.GRIDS] + [(g, k) for g in CC.NO_FIXED_POINT for k in (0.0, 1.0)]


_DENSE = {}


def dense_at_golden(grid, kappas):
    """{κ: dense K(1, θ, κ−γ)} on one grid of cont_sim_cases.GRIDS at its golden w (Gauss–Hermite QUAD_D), cached."""
    import cont_sim_cases as CC
    kind, sizes, sd = grid
    par = CC.params_of(kind)
    theta, _, gamma = co.pieces(kind, par)[:3]
    have = _DENSE.setdefault(grid, {})
    need = [k for k in kappas if k not in have]
    if need:
        grids = CC.grids_of(kind, sizes, sd)
        nodes, weights = OC.qnwnorm([CC.QUAD_D] * len(sizes))
        Ks = dense(kind, par, grids, CC.golden_wstar(kind, sizes, sd), np.ascontiguousarray(nodes.T), weights,
                   [(1, theta, k - gamma) for k in need])
        have.update(zip(need, Ks))
    return {k: have[k] for k in kappas}

"""
Numpy twin of the parameter tangent of the continuous-state operator (csrc/cont_sens.hpp, the C_PTAN form of
csrc/cont_kernel.hpp, ``sensitivity.wc_ratio_sensitivities_continuous``).

What is differentiated: T(w; p) of oracle/continuous.py ``T_fun_factory`` with ``grids, nodes, weights`` held fixed.

``tangent``       the analytic tangent for every unit direction from one pass over the nodes, with its abs companion (the
                  same expression with every signed term replaced by its absolute value), dtype float64 or longdouble;
``complex_step``  an independent tangent, Im T(p + i h e_j) / h with h = 1e-30: T restated on complex parameters with its
                  own multilinear interpolation, the cell chosen by the real part of the coordinate;
``dense_jacobian`` / ``dense_sensitivities``  J(w) from the corner weights of the interpolant (as
                  cont_pricing_oracle.dense assembles K) and dw*/dp = solve(I − J, ∂T/∂p).

The derivative of ``map_coordinates(order=1, mode='nearest')``: the floor has none, and where the coordinate is clamped
(c < 0 or c ≥ n − 1) both clipped corners coincide, so the tangent of the coordinate is zero there.
"""
import numpy as np

import cont_pricing_oracle as cp

# parameter places: (β, γ, ψ, μ_c, φ_c), then per dimension (ρ, s or None, φ or None, voldim, ξ or None, xdim); z, h_c dims
PLACES = {
    "ssy": dict(np=13, beta=0, gamma=1, psi=2, mu_c=3, phi_c=6, iz=3, ihc=1,
                dims=[(9, 12, None, -1, None, -1), (8, 11, None, -1, None, -1), (7, 10, None, -1, None, -1),
                      (4, None, 5, 2, None, -1)]),
    "gcy": dict(np=18, beta=0, gamma=2, psi=1, mu_c=5, phi_c=6, iz=4, ihc=1,
                dims=[(3, 4, None, -1, None, -1), (10, 11, None, -1, None, -1), (12, 13, None, -1, None, -1),
                      (16, 17, None, -1, None, -1), (7, None, 9, 2, 8, 5), (14, None, 15, 3, None, -1)]),
}
H = 1e-30

# The operator cases of the tangent tests: the seven of cont_pricing_oracle.CASES and one more.  In the two 4-D cases with
# unstaged blocks (C4, D4: Gauss–Hermite order 3 on narrow grids) every shocked node of z clips, so the tangent of φ_z is
# identically zero on the global-gather path; E4 has Monte-Carlo draws on D4's grid, some of which stay inside.
EXTRA_CASES = [("E4", "ssy", (8, 8, 8, 8), 0.1, ("mc", 100), "D", 0, 4096)]
CASES = list(cp.CASES) + EXTRA_CASES
CASE_IDS = [c[0] for c in CASES]


def _points(grids):
    mesh = np.meshgrid(*grids, indexing="ij")
    return np.stack([m.ravel() for m in mesh], axis=1)


def _strides(n):
    return [int(np.prod(n[d + 1:])) for d in range(len(n))]


def _cells(c_real, n):
    """Per dimension: (lower corner (M,), clipped coordinate (M,), in range (M,)) from the real coordinate."""
    out = []
    for d, cr in enumerate(c_real):
        cc = np.clip(cr, 0.0, n[d] - 1.0)
        i0 = np.minimum(np.floor(cc).astype(np.int64), n[d] - 2)
        out.append((i0, cc, (cr >= 0.0) & (cr < n[d] - 1.0)))
    return out


def _corner_values(wf, cells, stride):
    """w at the 2^D corners of every node's cell: shape (2,) * D + (M,)."""
    D = len(cells)
    idx = np.zeros((1,) * D + cells[0][0].shape, dtype=np.int64)
    for d, (i0, _, _) in enumerate(cells):
        bit = np.arange(2, dtype=np.int64).reshape((1,) * d + (2,) + (1,) * (D - d - 1) + (1,))
        idx = idx + (i0 + bit) * stride[d]
    return wf[idx]


def _contract(V, pairs):
    """Σ over the corner axes of V (2, …, 2, M) with the per-dimension weights pairs[d] = (weight of corner 0, of 1),
    each (M,) or (P, M): (M,) if every weight is, else (P, M)."""
    V = V[..., None, :]
    for a0, a1 in pairs:
        V = V[0] * a0 + V[1] * a1
    return V[0] if all(a0.ndim == 1 for a0, _ in pairs) else V


def next_coords(kind, p, x, nodes, grids):
    """(D, …) coordinates of the next states, p a sequence of scalars or of (P, 1) arrays (complex allowed); the division
    by the spacing as oracle.continuous.vals_to_coords has it."""
    out = []
    for d, (ir, isc, iph, vd, ix, xd) in enumerate(PLACES[kind]["dims"]):
        mean = p[ir] * x[d]
        if ix is not None:
            mean = mean + p[ix] * x[xd]
        vol = p[isc] if isc is not None else p[iph] * np.exp(x[vd])
        out.append((mean + vol * nodes[d] - grids[d][0]) / (grids[d][1] - grids[d][0]))
    return out


def complex_step(kind, params, grids, w, nodes, weights, which=None):
    """{j: Im T(p + i h e_j) / h on the grid} for the parameter indices ``which`` (default: all)."""
    pl = PLACES[kind]
    which = list(range(pl["np"])) if which is None else list(which)
    P = len(which)
    p = np.tile(np.asarray(params, dtype=np.complex128), (P, 1))
    for r, j in enumerate(which):
        p[r, j] += 1j * H
    p = [p[:, j].reshape(P, 1) for j in range(pl["np"])]
    beta, gamma, psi, mu_c, phi_c = (p[pl[k]] for k in ("beta", "gamma", "psi", "mu_c", "phi_c"))
    theta = (1.0 - gamma) / (1.0 - 1.0 / psi)
    rho_l, s_l = p[pl["dims"][0][0]], p[pl["dims"][0][1]]
    n = [len(g) for g in grids]
    stride = _strides(n)
    wf = np.asarray(w, dtype=np.float64).ravel()
    nodes = np.asarray(nodes, dtype=np.float64)
    W = cp.weights_of(nodes, weights)
    X = _points(grids)
    out = np.empty((P, X.shape[0]))
    for i, x in enumerate(X):
        c = next_coords(kind, p, x, nodes, grids)                    # D × (P, M) complex
        cells = _cells([np.broadcast_to(cd.real, (P, nodes.shape[1]))[0] for cd in c], n)
        V = _corner_values(wf, cells, stride)
        pairs = []
        for cd, (i0, cc, inr) in zip(c, cells):
            t = np.where(inr, cd - i0, cc - i0)                      # clamped: the real, constant coordinate
            pairs.append((1.0 - t, t))
        g = _contract(V, pairs)                                      # (P, M)
        e = np.sum(W * np.exp(theta * s_l * nodes[0]) * g ** theta, axis=1, keepdims=True)
        sig_c = phi_c * np.exp(x[pl["ihc"]])
        C = np.exp((1.0 - gamma) * (mu_c + x[pl["iz"]]) + 0.5 * (1.0 - gamma) ** 2 * sig_c ** 2 + theta * rho_l * x[0])
        out[:, i] = (1.0 + beta * (C * e) ** (1.0 / theta)).imag[:, 0] / H
    shape = tuple(n)
    return {j: out[r].reshape(shape) for r, j in enumerate(which)}


def tangent(kind, params, grids, w, nodes, weights, dtype=np.float64, points=None):
    """(dT (np, *shape), abs companion (np, *shape), T w (*shape)): row j is the tangent along the unit direction e_j.
    ``points``: flat (C-order) indices of the grid points to evaluate; the results then have shape (np, len(points)) and
    (len(points),)."""
    pl = PLACES[kind]
    npar = pl["np"]
    q = [dtype(v) for v in params]
    beta, gamma, psi, mu_c, phi_c = (q[pl[k]] for k in ("beta", "gamma", "psi", "mu_c", "phi_c"))
    one = dtype(1.0)
    theta = (one - gamma) / (one - one / psi)
    dtheta = np.zeros(npar, dtype=dtype)
    dtheta[pl["gamma"]] = -psi / (psi - one)
    dtheta[pl["psi"]] = -(one - gamma) / (psi - one) ** 2
    i_rl, i_sl = pl["dims"][0][0], pl["dims"][0][1]
    rho_l, s_l = q[i_rl], q[i_sl]
    unit = np.eye(npar, dtype=dtype)
    grids = [np.asarray(g, dtype=dtype) for g in grids]
    n = [len(g) for g in grids]
    D = len(n)
    stride = _strides(n)
    wf = np.asarray(w, dtype=dtype).ravel()
    nodes = np.asarray(nodes, dtype=dtype)
    M = nodes.shape[1]
    W = np.asarray(cp.weights_of(nodes, weights), dtype=dtype)
    X = _points(grids)
    if points is not None:
        X = X[np.asarray(points, dtype=np.int64)]
    N = X.shape[0]
    dT, aT, Tw = np.empty((npar, N), dtype=dtype), np.empty((npar, N), dtype=dtype), np.empty(N, dtype=dtype)
    ones = (np.ones(M, dtype=dtype), np.ones(M, dtype=dtype))
    for i, x in enumerate(X):
        c = next_coords(kind, q, x, nodes, grids)
        cells = _cells(c, n)
        V = _corner_values(wf, cells, stride)
        pairs = [((one - (cc - i0)), (cc - i0)) for (i0, cc, _) in cells]
        g = _contract(V, pairs)
        gdot = np.zeros((npar, M), dtype=dtype)
        gabs = np.zeros((npar, M), dtype=dtype)
        for d, (ir, isc, iph, vd, ix, xd) in enumerate(pl["dims"]):
            inv = one / (grids[d][1] - grids[d][0])
            am = unit[ir] * x[d]
            if ix is not None:
                am = am + unit[ix] * x[xd]
            kv = unit[isc] if isc is not None else unit[iph] * np.exp(x[vd])
            inr = cells[d][2]
            a_k = (am * inv)[:, None], (kv * inv)[:, None] * nodes[d][None, :]
            cdot = (a_k[0] + a_k[1]) * inr[None, :]
            cabs = (np.abs(a_k[0]) + np.abs(a_k[1])) * inr[None, :]
            slope = _contract(V, pairs[:d] + [(-ones[0], ones[1])] + pairs[d + 1:])      # ∂ŵ/∂c_d in this cell
            sabs = _contract(V, pairs[:d] + [ones] + pairs[d + 1:])                       # (w > 0: the sum of |terms|)
            gdot += slope[None, :] * cdot
            gabs += np.abs(sabs)[None, :] * cabs
        eta0 = nodes[0]
        lg = np.log(g)
        omega = W * np.exp(theta * s_l * eta0) * g ** theta
        e = np.sum(omega)
        L = dtheta[:, None] * (s_l * eta0 + lg)[None, :] + theta * (unit[i_sl][:, None] * eta0[None, :] + gdot / g)
        La = np.abs(dtheta)[:, None] * (np.abs(s_l * eta0) + np.abs(lg))[None, :] + \
            np.abs(theta) * (unit[i_sl][:, None] * np.abs(eta0)[None, :] + gabs / g)
        ee, eea = (L @ omega) / e, (La @ omega) / e
        z, h0 = x[pl["iz"]], x[0]
        eh = np.exp(x[pl["ihc"]])
        sig_c = phi_c * eh
        omg = one - gamma
        lnC_terms = (omg * (mu_c + z), dtype(0.5) * omg * omg * sig_c * sig_c, theta * rho_l * h0)
        dl = (-unit[pl["gamma"]] * (mu_c + z) + unit[pl["mu_c"]] * omg - unit[pl["gamma"]] * omg * sig_c * sig_c +
              unit[pl["phi_c"]] * omg * omg * sig_c * eh + dtheta * rho_l * h0 + unit[i_rl] * theta * h0)
        dla = (unit[pl["gamma"]] * np.abs(mu_c + z) + unit[pl["mu_c"]] * np.abs(omg) +
               unit[pl["gamma"]] * np.abs(omg * sig_c * sig_c) + unit[pl["phi_c"]] * np.abs(omg * omg * sig_c * eh) +
               np.abs(dtheta * rho_l * h0) + unit[i_rl] * np.abs(theta * h0))
        lnKg = sum(lnC_terms) + np.log(e)
        lnKg_abs = sum(np.abs(t) for t in lnC_terms) + np.abs(np.log(e))
        u = np.exp(lnKg / theta)
        Tw[i] = one + beta * u
        dT[:, i] = unit[pl["beta"]] * u + beta * u * ((dl + ee) / theta - dtheta * lnKg / theta ** 2)
        aT[:, i] = unit[pl["beta"]] * u + beta * u * ((dla + eea) / np.abs(theta) + np.abs(dtheta) * lnKg_abs / theta ** 2)
    if points is not None:
        return dT, aT, Tw
    shape = tuple(n)
    return dT.reshape((npar,) + shape), aT.reshape((npar,) + shape), Tw.reshape(shape)


def min_line_distance(kind, params, grids, nodes):
    """The smallest distance, in cells, of any in-range next-state coordinate to a grid line, over all grid points, nodes
    and dimensions (the tangent is one-sided on a line; which side is a matter of the coordinate's last bit)."""
    q = [float(v) for v in params]
    n = [len(g) for g in grids]
    nodes = np.asarray(nodes, dtype=np.float64)
    best = np.inf
    for x in _points(grids):
        for d, c in enumerate(next_coords(kind, q, x, nodes, grids)):
            c = np.broadcast_to(c, nodes[d].shape)
            c = c[(c > -0.5) & (c < n[d] - 0.5)]                     # (the lines 0 and n − 1 included, from both sides)
            if c.size:
                best = min(best, float(np.min(np.abs(c - np.rint(c)))))
    return best


def dense_jacobian(kind, params, grids, w, nodes, weights):
    """The N × N matrix of J(w) = ∂T/∂w, rows and columns in C order, from the corner weights of the interpolant."""
    import cont_sim_oracle as co
    theta, beta, gamma, mu_c, phi_c, iz, ihc, rho_l, s_l, nxt = co.pieces(kind, params)
    par = tuple(float(v) for v in params)
    w = np.asarray(w, dtype=np.float64)
    nodes = np.asarray(nodes, dtype=np.float64)
    W = cp.weights_of(nodes, weights)
    X = _points(grids)
    N = X.shape[0]
    wf = w.ravel()
    J = np.zeros((N, N))
    for i, x in enumerate(X):
        nx = nxt(par, x, nodes)
        idx, wgt = cp.corner_weights(grids, nx)
        g = np.sum(wgt * wf[idx], axis=0)
        pf = W * np.exp(theta * nx[0])
        sig_c = phi_c * np.exp(x[ihc])
        C = np.exp((1 - gamma) * (mu_c + x[iz]) + 0.5 * (1 - gamma) ** 2 * sig_c ** 2)
        Kg = C * np.dot(pf, g ** theta)
        coef = beta * Kg ** (1.0 / theta - 1.0) * C * pf * g ** (theta - 1.0)
        J[i] = np.bincount(idx.ravel(), weights=(wgt * coef).ravel(), minlength=N)
    return J


def dense_sensitivities(kind, params, grids, w, nodes, weights):
    """(dw/dp (np, *shape) = solve(I − J, ∂T/∂p) for every parameter, cond₂(I − J))."""
    J = dense_jacobian(kind, params, grids, w, nodes, weights)
    dT = tangent(kind, params, grids, w, nodes, weights)[0]
    A = np.eye(J.shape[0]) - J
    x = np.linalg.solve(A, dT.reshape(dT.shape[0], -1).T).T
    return x.reshape(dT.shape), float(np.linalg.cond(A, 2))

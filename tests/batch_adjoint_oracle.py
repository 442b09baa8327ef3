"""
Helper of tests/test_batch_gradient_cpu.py and tests/test_hip_batch_gradient.py (not a test module): the adjoint moments
of csrc/batch_adjoint.hpp restated in numpy from (w, lambda) with the oracle's pieces (``_pieces``, ``expect_*``,
``vjp_*``, ``kfactor_gcy``), a dense lambda from N columns of the oracle's J.v, and the truth of a gradient,
<lambda, complex-step dT/dp>.

The moment block is  s0 s1 s2 | R[ndim] | M1[n_lam] | M2[n_c] | M3[a3 table]  (include/sdfs_hip.h).  E = H0(a1 w^theta)
comes from ``expect_*`` directly (the kernel divides its contraction by a2 along h_c instead), ln((T w - 1)/beta) from
ln(K E) / theta (the kernel takes the logarithm of c_out S / beta), so the two sides reach R and s1 by different routes.
"""
import numpy as np

from oracle import gcy as ogcy
from oracle import models as omodels
from oracle import ssy as ossy
from persistence_oracle import complex_step_tangent

# (axis of h_lam, axis of h_c)
AXES = {"ssy": (0, 1), "gcy": (5, 3)}


def oracle_inputs(kind, shapes, over):
    """(params, arrays) of the oracle for the overrides of a family member."""
    if kind == "ssy":
        p = omodels.ssy_params(**over)
        return p, ossy.discretize_ssy(p, tuple(shapes))
    p = omodels.gcy_params(**over)
    return p, ogcy.discretize_gcy(p, tuple(shapes))


def T(kind, shapes, params, arrays, w):
    f = ossy.T_ssy_factorised if kind == "ssy" else ogcy.T_gcy_factorised
    return f(w, shapes, params, arrays)


def jvp(kind, shapes, params, arrays, w, v):
    return (ossy.jvp_ssy if kind == "ssy" else ogcy.jvp_gcy)(w, v, shapes, params, arrays)


def vjp(kind, shapes, params, arrays, w, u):
    return (ossy.vjp_ssy if kind == "ssy" else ogcy.vjp_gcy)(w, u, shapes, params, arrays)


def dense_jacobian(kind, shapes, params, arrays, w):
    """J(w) as an N x N matrix: N columns of the oracle's J.v."""
    N = int(np.prod(shapes))
    J = np.empty((N, N))
    e = np.zeros(N)
    for c in range(N):
        e[c] = 1.0
        J[:, c] = jvp(kind, shapes, params, arrays, w, e.reshape(shapes)).ravel()
        e[c] = 0.0
    return J


def dense_lambda(kind, shapes, params, arrays, w, g):
    """lambda = (I - J(w)^T)^(-1) g by a dense solve."""
    J = dense_jacobian(kind, shapes, params, arrays, w)
    return np.linalg.solve(np.eye(J.shape[0]) - J.T, np.asarray(g, dtype=np.float64).ravel()).reshape(shapes)


def dense_fixed_point(kind, shapes, params, arrays, steps=8):
    """w* by Newton with the dense Jacobian from 800 (small grids)."""
    w = np.full(shapes, 800.0)
    for _ in range(steps):
        J = dense_jacobian(kind, shapes, params, arrays, w)
        r = (T(kind, shapes, params, arrays, w) - w).ravel()
        w = w - np.linalg.solve(J - np.eye(J.shape[0]), r).reshape(shapes)
    return w


def _fields(kind, params, arrays, w):
    """beta, theta, E = H0(a1 w^theta), K = a2 a3 on the grid."""
    if kind == "ssy":
        beta, theta, a1, a2, a3, Ql, Qc, Qz, zQ = ossy._pieces(params, arrays)
        E = ossy.expect_ssy(a1[:, None, None, None] * w ** theta, (Ql, Qc, Qz, zQ))
        K = a2[None, :, None, None] * a3[None, None, :, :]
    else:
        beta, theta, a1, a2, a3, zQ, zpQ, Qhz, Qhc, Qhzp, Qhl = ogcy._pieces(params, arrays)
        E = ogcy.expect_gcy(a1 * w ** theta, (zQ, zpQ, Qhz, Qhc, Qhzp, Qhl))
        K = ogcy.kfactor_gcy(a2, a3) * np.ones_like(w)
    return beta, theta, E, K


def _marginals(kind, m, mu):
    if kind == "ssy":
        return mu.sum(axis=(1, 2, 3)), m.sum(axis=(0, 2, 3)), m.sum(axis=(0, 1)).ravel()
    m3 = np.transpose(m.sum(axis=(3, 5)), (1, 2, 3, 0))          # [a, b, c, e] -> the a3 table's [b, c, e, a]
    return mu.sum(axis=(0, 1, 2, 3, 4)), m.sum(axis=(0, 1, 2, 4, 5)), m3.ravel()


def moments(kind, shapes, params, arrays, w, lam):
    """(block, scale): the moment block of (w, lambda) and, entry by entry, the sum of the absolute values of its terms."""
    shapes = tuple(shapes)
    w = np.asarray(w, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    beta, theta, E, K = _fields(kind, params, arrays, w)
    tm1 = beta * (K * E) ** (1.0 / theta)
    m = lam * tm1
    mu = vjp(kind, shapes, params, arrays, w, lam) * w
    lnu = np.log(K * E) / theta
    lnw = np.log(w)
    head = [m.sum(), (m * lnu).sum(), (mu * lnw).sum()]
    head_s = [np.abs(m).sum(), np.abs(m * lnu).sum(), np.abs(mu * lnw).sum()]
    R, R_s = [], []
    for k, n in enumerate(shapes):
        i = np.arange(n, dtype=np.float64).reshape([n if a == k else 1 for a in range(len(shapes))])
        Ek = np.moveaxis(E, k, 0)
        down = np.zeros_like(Ek)
        up = np.zeros_like(Ek)
        down[1:] = Ek[:-1] / Ek[1:] - 1.0
        up[:-1] = Ek[1:] / Ek[:-1] - 1.0
        down, up = np.moveaxis(down, 0, k), np.moveaxis(up, 0, k)
        R.append((m * (i * down + (n - 1.0 - i) * up)).sum())
        R_s.append((np.abs(m) * (i * np.abs(down) + (n - 1.0 - i) * np.abs(up))).sum())
    block = np.concatenate([head, R, *_marginals(kind, m, mu)])
    scale = np.concatenate([head_s, R_s, *_marginals(kind, np.abs(m), np.abs(mu))])
    return block, scale


def split(kind, shapes, block):
    """{"s": 3, "R": ndim, "M1", "M2", "M3"} views of a moment block."""
    ndim = len(shapes)
    ax_l, ax_c = AXES[kind]
    o1 = 3 + ndim
    o2 = o1 + shapes[ax_l]
    o3 = o2 + shapes[ax_c]
    return {"s": block[:3], "R": block[3:o1], "M1": block[o1:o2], "M2": block[o2:o3], "M3": block[o3:]}


def truth_gradient(S, kind, shapes, model, params, arrays, w, lam):
    """{name: <lambda, complex-step dT/dp_name at w>} for every parameter of the model, with the true tangents of the
    discretisation (transition arrays included)."""
    from sdfs_via_autodiff_amd import sensitivity as sens
    names = sens.SSY_PARAMS if kind == "ssy" else sens.GCY_PARAMS
    pers = sens.SSY_PERSISTENCE if kind == "ssy" else sens.GCY_PERSISTENCE
    tan = S.discretize_ssy_tangent if kind == "ssy" else S.discretize_gcy_tangent
    ptan = S.discretize_ssy_persistence_tangent if kind == "ssy" else S.discretize_gcy_persistence_tangent
    out = {}
    for nm in names:
        dp, da = ptan(model, shapes, nm)[:2] if nm in pers else tan(model, shapes, nm)
        dT = complex_step_tangent(kind, tuple(shapes), params, arrays, dp, da, w)
        out[nm] = float(np.sum(lam * dT))
    return out

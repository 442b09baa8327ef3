"""
Numpy twin of the transposed Jacobian of the continuous-state operator and of the adjoint gradient built on it (the C_VJP
form of csrc/cont_kernel.hpp, csrc/cont_adjoint.hpp, ``sensitivity.wc_ratio_gradient_continuous``), from the
dense J(w) and the tangent of tests/cont_sens_oracle.py:

``jacobian``   J(w), N × N, rows and columns in C order (``so.dense_jacobian``);
``vjp``        Jᵀu and its abs companion Jᵀ|u| -- J is entrywise non-negative (node weights, hat weights and the powers of a
               positive interpolant), so the companion is the sum of the magnitudes of the terms of Jᵀu;
``adjoint``    λ_ref = solve(I − Jᵀ, g) and cond₂(I − J), which is cond₂ of the transpose too;
``gradient``   d⟨g, w*⟩/dp_k = ⟨λ_ref, ∂T/∂p_k⟩ for every parameter, with the companion Σ|λ_ref|·aT_k (aT the abs companion
               of the tangent) and Σ|∂T/∂p_k|.
"""
import numpy as np

import cont_sens_oracle as so


def jacobian(kind, params, grids, w, nodes, weights):
    J = so.dense_jacobian(kind, params, grids, w, nodes, weights)
    assert np.all(J >= 0.0)
    return J


def vjp(J, u):
    """(Jᵀu, Jᵀ|u|) as flat vectors."""
    u = np.asarray(u, dtype=np.float64).ravel()
    return J.T @ u, J.T @ np.abs(u)


def adjoint(J, g):
    """(λ_ref = solve(I − Jᵀ, g) flat, cond₂(I − J))."""
    A = np.eye(J.shape[0]) - J
    lam = np.linalg.solve(A.T, np.asarray(g, dtype=np.float64).ravel())
    return lam, float(np.linalg.cond(A, 2))


def gradient(dT, aT, lam):
    """(⟨λ, ∂T/∂p_k⟩, Σ|λ|·aT_k, Σ|∂T/∂p_k|), each (np,), from the tangent and its abs companion (np, *shape)."""
    npar = dT.shape[0]
    d, a = dT.reshape(npar, -1), aT.reshape(npar, -1)
    return d @ lam, a @ np.abs(lam), np.sum(np.abs(d), axis=1)

"""
NumPy restatements behind the persistence-tangent tests (test_persistence_cpu.py, test_hip_persistence.py).

  rouwenhorst_matrix_complex   oracle.rouwenhorst.rouwenhorst_matrix on a complex p, for complex-step derivatives
  dense_generator              the (3, n) diagonals of ``rouwenhorst_generator`` as an n x n matrix
  complex_step_tangent         dT(w) along (dparams, darrays) by the complex step of the oracle's factorised T
  stencil_tangent              the same tangent as  states part + generator stencil on the oracle's T w
"""
import numpy as np

from oracle import gcy as ogcy, ssy as ossy
from oracle.models import theta_of

TRANSITION = {"ssy": (1, 3, 5, 7), "gcy": (1, 3, 5, 8, 11, 14)}      # transition array of each grid axis


def rouwenhorst_matrix_complex(n, p):
    """oracle.rouwenhorst.rouwenhorst_matrix(n, p, p), statement for statement, in complex arithmetic.  (The oracle
    accumulates into a float array and so cannot take a complex p above n = 2; the matrix is a polynomial in p.)"""
    q = p
    theta = np.array([[p, 1.0 - p], [1.0 - q, q]], dtype=np.complex128)
    for m in range(3, n + 1):
        prev = theta
        theta = np.zeros((m, m), dtype=np.complex128)
        theta[: m - 1, : m - 1] += p * prev
        theta[: m - 1, 1:] += (1.0 - p) * prev
        theta[1:, : m - 1] += (1.0 - q) * prev
        theta[1:, 1:] += q * prev
        theta[1 : m - 1, :] /= 2.0
    return theta


def dense_generator(gen):
    gen = np.asarray(gen)
    n = gen.shape[1]
    G = np.diag(gen[1])
    G[np.arange(1, n), np.arange(n - 1)] = gen[0][1:]
    G[np.arange(n - 1), np.arange(1, n)] = gen[2][:-1]
    return G


def oracle_T(kind):
    return ossy.T_ssy_factorised if kind == "ssy" else ogcy.T_gcy_factorised


def complex_step_tangent(kind, shapes, params, arrays, dparams, darrays, w, h=1e-30):
    """Im T(p + i h dp, arrays + i h darrays)(w) / h: exact to rounding, transition tangents included."""
    pc = tuple(complex(p, h * d) for p, d in zip(params, dparams))
    ac = tuple(np.asarray(a, dtype=np.complex128) + 1j * h * np.asarray(d) for a, d in zip(arrays, darrays))
    return np.imag(oracle_T(kind)(w, shapes, pc, ac)) / h


def _k_factor(kind, params, arrays):
    if kind == "ssy":
        _, _, _, a2, a3, *_ = ossy._pieces(params, arrays)
        return a2[None, :, None, None] * a3[None, None, :, :]
    _, _, _, a2, a3, *_ = ogcy._pieces(params, arrays)
    return ogcy.kfactor_gcy(a2, a3)


def stencil_tangent(kind, shapes, params, arrays, dparams, darrays, dgen, w):
    """dT(w) of a persistence direction as the library forms it: the state-array part (complex step with the transition
    tangents set to zero) plus, per axis with a generator G,  (T w - 1) / theta . (G E) / E  along that axis, with
    E = ((T w - 1) / beta)^theta / (a2 a3)."""
    states = [np.zeros_like(a) if i in TRANSITION[kind] else d for i, (a, d) in enumerate(zip(arrays, darrays))]
    out = complex_step_tangent(kind, shapes, params, arrays, dparams, states, w)
    beta = params[0]
    theta = theta_of(params[1], params[2]) if kind == "ssy" else theta_of(params[2], params[1])
    Tw = oracle_T(kind)(w, shapes, params, arrays)
    E = ((Tw - 1.0) / beta) ** theta / _k_factor(kind, params, arrays)
    for ax, gen in enumerate(dgen):
        if gen is None:
            continue
        GE = np.moveaxis(np.tensordot(dense_generator(gen), E, axes=([1], [ax])), 0, ax)
        out = out + (Tw - 1.0) / theta * GE / E
    return out

"""The oracle's vector-Jacobian product dT(w)^T[u] (oracle/ssy.py vjp_ssy, oracle/gcy.py vjp_gcy, the C twin's mode 2),
the reference the GPU tests of the library's VJP (tests/test_hip_vjp.py) and of its transposed solve are held to.

 (1) numpy vjp_* against the transpose of a dense Jacobian built column by column from the oracle's jvp_*,
     on Rouwenhorst tensors (centrosymmetric), random unconditional tensors and random conditional ones;
 (2) the C VJP against numpy, conditional tensors included;
 (3) the adjoint identity <u, J v> = <J^T u, v> on both.
"""
import numpy as np
import pytest

from oracle import models, ssy, gcy
from oracle.c_oracle import COperator

# transition tensors in each model's arrays tuple (SSY z_Q and GCY z_Q / z_pi_Q are conditional)
SSY_Q = (1, 3, 5, 7)
GCY_Q = (1, 3, 5, 8, 11, 14)


def random_stochastic(rng, shape):
    """Strictly positive, row-stochastic along the last axis, every slice different (and not centrosymmetric)."""
    q = rng.random(shape) + 0.05
    return q / q.sum(axis=-1, keepdims=True)


def model_arrays(model, shapes, kind, seed=0):
    """(params, arrays, jvp, vjp) with the transition tensors of `kind`: "rouwenhorst" (the discretisation's own),
    "unconditional" (one random matrix per axis, copied into every conditioning slice) or "conditional" (a random
    matrix per slice)."""
    rng = np.random.default_rng(seed)
    if model == "ssy":
        p = models.ssy_params(); arr = list(ssy.discretize_ssy(p, shapes))
        qi, jvp, vjp = SSY_Q, ssy.jvp_ssy, ssy.vjp_ssy
    else:
        p = models.gcy_params(); arr = list(gcy.discretize_gcy(p, shapes))
        qi, jvp, vjp = GCY_Q, gcy.jvp_gcy, gcy.vjp_gcy
    if kind != "rouwenhorst":
        for i in qi:
            n = arr[i].shape[-1]
            if kind == "conditional":
                arr[i] = random_stochastic(rng, arr[i].shape)
            else:
                arr[i] = np.broadcast_to(random_stochastic(rng, (n, n)), arr[i].shape).copy()
    return p, arr, jvp, vjp


def is_centrosymmetric(q):
    return np.allclose(q, q[..., ::-1, ::-1], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("kind", ["rouwenhorst", "unconditional", "conditional"])
@pytest.mark.parametrize("model,shapes", [("ssy", (3, 2, 4, 3)), ("gcy", (2, 3, 2, 3, 2, 3))])
def test_numpy_vjp_is_transpose_of_dense_jacobian(model, shapes, kind):
    p, arr, jvp, vjp = model_arrays(model, shapes, kind, seed=11)
    qi = SSY_Q if model == "ssy" else GCY_Q
    if kind == "rouwenhorst":
        assert all(is_centrosymmetric(arr[i]) for i in qi)
    else:
        assert not any(is_centrosymmetric(arr[i]) for i in qi)
    rng = np.random.default_rng(12)
    w = 300 + 600 * rng.random(shapes)
    n = w.size
    J = np.stack([jvp(w, e.reshape(shapes), shapes, p, arr).ravel() for e in np.eye(n)], axis=1)   # J[:, j] = J e_j
    for _ in range(3):
        u = rng.standard_normal(shapes)
        want = J.T @ u.ravel()
        got = vjp(w, u, shapes, p, arr).ravel()
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.max(np.abs(want)))
    # every column of J^T: the unit vectors as u
    JT = np.stack([vjp(w, e.reshape(shapes), shapes, p, arr).ravel() for e in np.eye(n)], axis=1)
    np.testing.assert_allclose(JT, J.T, rtol=1e-12, atol=1e-12 * np.max(np.abs(J)))


@pytest.mark.parametrize("kind", ["rouwenhorst", "unconditional", "conditional"])
@pytest.mark.parametrize("model,shapes", [("ssy", (4, 7, 6, 5)), ("ssy", (10, 10, 10, 10)),
                                          ("gcy", (2, 3, 4, 5, 6, 7)), ("gcy", (5,) * 6)])
def test_c_vjp_matches_numpy_vjp(model, shapes, kind):
    p, arr, jvp, vjp = model_arrays(model, shapes, kind, seed=3)
    op = COperator(model, shapes, p, arr)
    rng = np.random.default_rng(4)
    w = 300 + 600 * rng.random(shapes)
    u = rng.standard_normal(shapes)
    v = rng.standard_normal(shapes)
    want = vjp(w, u, shapes, p, arr)
    got = op.vjp(w, u)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-13 * np.max(np.abs(want)))
    # adjoint identity, numpy and C
    jv = jvp(w, v, shapes, p, arr)
    lhs = float(np.vdot(u, jv))
    for jtu in (want, got):
        assert abs(lhs - float(np.vdot(jtu, v))) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(jv)
    np.testing.assert_allclose(op.jvp(w, v), jv, rtol=1e-11, atol=1e-13 * np.max(np.abs(jv)))
    # (mode 2 leaves the other modes alone: T after a VJP is still T)
    T = ssy.T_ssy_factorised if model == "ssy" else gcy.T_gcy_factorised
    np.testing.assert_allclose(op(w), T(w, shapes, p, arr), rtol=1e-13)


@pytest.mark.parametrize("model,shapes", [("ssy", (3, 2, 4, 3)), ("gcy", (2, 3, 2, 3, 2, 3))])
def test_vjp_is_not_the_forward_form(model, shapes):
    """The checks above can tell J^T from J, and from an adjoint that uses Q instead of Q^T or the forward axis
    order: each of those differs from the true J^T by far more than the tolerance on conditional tensors."""
    p, arr, jvp, vjp = model_arrays(model, shapes, "conditional", seed=5)
    rng = np.random.default_rng(6)
    w = 300 + 600 * rng.random(shapes)
    u = rng.standard_normal(shapes)
    want = vjp(w, u, shapes, p, arr)
    scale = np.max(np.abs(want))
    assert np.max(np.abs(jvp(w, u, shapes, p, arr) - want)) > 1e-6 * scale
    if model == "ssy":
        beta, theta, a1, a2, a3, Ql, Qc, Qz, zQ = ssy._pieces(p, arr)
        A1 = a1[:, None, None, None]
        K = a2[None, :, None, None] * a3[None, None, :, :]
        S = ssy.expect_ssy(A1 * w ** theta, (Ql, Qc, Qz, zQ))
        y = beta * (K * S) ** (1 / theta - 1) * K * u
        untransposed = A1 * w ** (theta - 1) * ssy.expect_ssy_T(
            y, tuple(np.swapaxes(q, -1, -2) for q in (Ql, Qc, Qz, zQ)))
        # forward order with transposed matrices: z's adjoint after h_z's (its slice index is then a next-state index)
        x = np.einsum("iI,LKiJ->LKIJ", Qz, np.einsum("kK,Lkij->LKij", Qc, np.einsum("lL,lkij->Lkij", Ql, y)))
        wrong_order = A1 * w ** (theta - 1) * np.einsum("ijJ,LKij->LKiJ", zQ, x)
    else:
        beta, theta, a1, a2, a3, zQ, zpQ, Qhz, Qhc, Qhzp, Qhl = gcy._pieces(p, arr)
        Qs = (zQ, zpQ, Qhz, Qhc, Qhzp, Qhl)
        K = gcy.kfactor_gcy(a2, a3)
        S = gcy.expect_gcy(a1 * w ** theta, Qs)
        y = beta * (K * S) ** (1 / theta - 1) * K * u
        untransposed = a1 * w ** (theta - 1) * gcy.expect_gcy_T(y, tuple(np.swapaxes(q, -1, -2) for q in Qs))
        # expect_gcy's order with the adjoint contractions: z_pi and z conditioned on next-state indices
        x = np.einsum("fF,abcdef->abcdeF", Qhl, y)
        x = np.einsum("eE,abcdeF->abcdEF", Qhzp, x)
        x = np.einsum("dD,abcdEF->abcDEF", Qhc, x)
        x = np.einsum("cC,abcDEF->abCDEF", Qhz, x)
        x = np.einsum("EbB,abCDEF->aBCDEF", zpQ, x)
        wrong_order = a1 * w ** (theta - 1) * np.einsum("BCEaA,aBCDEF->ABCDEF", zQ, x)
    for bad in (untransposed, wrong_order):
        assert np.max(np.abs(bad - want)) > 1e-6 * scale

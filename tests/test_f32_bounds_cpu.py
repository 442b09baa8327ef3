"""
The error bound of the reduced-precision J.v products (tests/f32_bound.py), pinned on the CPU before the GPU tests
(tests/test_hip_f32_forms.py) rely on it: a numpy emulation of each storage form meets it, and four deliberate faults of
the kind a kernel could make each violate it -- so the bound is tight enough to catch them, and loose enough for the
legitimate rounding.

The emulation follows the kernels' structure: c1 and c2 computed in fp64 and stored as floats (times 2^k and 2^-k, as
the library stores them, k from the mid-grid point), the contraction two axes per pass with each pass's result stored as floats, the last pass
multiplying by c2 (and subtracting v) before its float store.  Inputs: the discretisation's Rouwenhorst tensors
(centrosymmetric) and one random row-stochastic, non-centrosymmetric matrix per axis; 4-D and 6-D grids with a 20-wide
axis for the dropped-row fault.
"""
import numpy as np
import pytest

import f32_bound as fb
from oracle import gcy, models, ssy

SSY_Q = (1, 3, 5, 7)
GCY_Q = (1, 3, 5, 8, 11, 14)
CASES = [("ssy", (20, 6, 5, 7), 1), ("ssy", (6, 7, 5, 20), 7), ("gcy", (4, 3, 5, 20, 3, 4), 8),
         ("gcy", (20, 4, 3, 3, 4, 5), 1)]        # (model, shapes, index into arrays of the transition tensor of the 20-wide axis)
INPUTS = ["rouwenhorst", "random"]


def f32(a):
    with np.errstate(over="ignore"):          # (the "scale" fault overflows: inf is a violation too)
        return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def bf16(a):
    """Round to bfloat16 (nearest, ties to even) through float32, as k_round_bf16 does."""
    b = np.asarray(a, np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def setup(model, shapes, inputs, seed=0):
    if model == "ssy":
        p = models.ssy_params(); arr = list(ssy.discretize_ssy(p, shapes)); qi = SSY_Q
    else:
        p = models.gcy_params(); arr = list(gcy.discretize_gcy(p, shapes)); qi = GCY_Q
    if inputs == "random":
        rng = np.random.default_rng(100 + seed)
        for i in qi:
            n = arr[i].shape[-1]
            q = rng.random((n, n)) + 0.05
            q /= q.sum(axis=1, keepdims=True)
            assert not np.allclose(q, q[::-1, ::-1])
            arr[i] = np.ascontiguousarray(np.broadcast_to(q, arr[i].shape))
    return p, arr


def passes(model, Qs, contract):
    """The per-axis contractions of oracle/{ssy,gcy}.py expect_*, grouped two axes per pass."""
    if model == "ssy":
        Ql, Qc, Qz, zQ = Qs
        return [[lambda x: contract("iI,LKIJ->LKiJ", Qz, x), lambda x: contract("ijJ,LKiJ->LKij", zQ, x)],
                [lambda x: contract("kK,LKij->Lkij", Qc, x), lambda x: contract("lL,Lkij->lkij", Ql, x)]]
    zQ, zpQ, Qhz, Qhc, Qhzp, Qhl = Qs
    return [[lambda x: contract("fF,ABCDEF->ABCDEf", Qhl, x), lambda x: contract("eE,ABCDEf->ABCDef", Qhzp, x)],
            [lambda x: contract("dD,ABCDef->ABCdef", Qhc, x), lambda x: contract("cC,ABCdef->ABcdef", Qhz, x)],
            [lambda x: contract("ebB,ABcdef->Abcdef", zpQ, x), lambda x: contract("bceaA,Abcdef->abcdef", zQ, x)]]


def scalings(model, w, p, arr):
    """c1 = a1 w^(theta-1), c2 = beta (K S)^(1/theta-1) K in fp64, and the transition tensors in expect_* order."""
    if model == "ssy":
        beta, theta, a1, a2, a3, Ql, Qc, Qz, zQ = ssy._pieces(p, arr)
        Qs = (Ql, Qc, Qz, zQ)
        A1 = a1[:, None, None, None]
        K = a2[None, :, None, None] * a3[None, None, :, :]
        S = ssy.expect_ssy(A1 * w ** theta, Qs)
    else:
        beta, theta, a1, a2, a3, *Qs = gcy._pieces(p, arr)
        Qs = tuple(Qs)
        A1 = a1
        K = gcy.kfactor_gcy(a2, a3)
        S = gcy.expect_gcy(a1 * w ** theta, Qs)
    return A1 * w ** (theta - 1), beta * (K * S) ** (1 / theta - 1) * K, Qs


def emulate(model, w, v, p, arr, m, store=f32, mid=None, fp32_math=False, fault=None, q_index=None):
    """One J.v product in reduced storage.  store: rounding of c1, c2 and the output; mid: of the intermediates
    (default: store); fp32_math: contractions in float32 (the fp32-MFMA form).  fault: None, "transpose" (one axis's
    matrix transposed), "drop_row" (the last row of the 20-wide axis's contraction left out), "scale" (c1 stored times
    2^k, c2 not divided by it), "scale_by_2" (c2 divided by 2^(k-1): one factor 2 left over), "bf16_mid" (intermediates
    rounded to bfloat16)."""
    mid = mid or store
    c1, c2, Qs = scalings(model, w, p, arr)
    if fault in ("transpose", "drop_row"):            # (c1, c2 from the true tensors: only the contraction is wrong)
        Qs = list(Qs)
        j = (SSY_Q if model == "ssy" else GCY_Q).index(q_index)      # (Qs is in the arrays tuple's order)
        q = np.array(Qs[j], dtype=np.float64)
        if fault == "transpose":
            q = np.swapaxes(q, -1, -2)
        else:
            q[..., -1, :] = 0.0
        Qs[j] = q
    # the library's power of two (fast_kernels.hpp, lin_scale_of): k = -ilogb(c1 at the mid-grid point)
    scale = 2.0 ** -(np.frexp(c1[tuple(n // 2 for n in w.shape)])[1] - 1)
    c1s = store(c1 * scale)
    c2s = store(c2) if fault == "scale" else store(c2 / scale * (2.0 if fault == "scale_by_2" else 1.0))
    if fault == "bf16_mid":
        mid = bf16
    if fp32_math:
        def contract(sub, q, x):
            return np.einsum(sub, np.asarray(q, np.float32), np.asarray(x, np.float32)).astype(np.float64)
    else:
        contract = np.einsum
    x = c1s * v
    ps = passes(model, Qs, contract)
    for k, steps in enumerate(ps):
        for f in steps:
            x = f(x)
        if k < len(ps) - 1:
            x = mid(x)
    return store(c2s * x - (v if m else 0.0))


def reference(model, w, v, p, arr, m):
    jvp = ssy.jvp_ssy if model == "ssy" else gcy.jvp_gcy
    shapes = w.shape
    want = jvp(w, v, shapes, p, arr) - (v if m else 0.0)
    return want, jvp(w, np.abs(v), shapes, p, arr)


def inputs_wv(shapes, seed):
    rng = np.random.default_rng(seed)
    w = 300 + 600 * rng.random(shapes)
    v = rng.standard_normal(shapes).astype(np.float32).astype(np.float64)
    return w, v


def prepare(model, shapes, inputs):
    p, arr = setup(model, shapes, inputs)
    w, v = inputs_wv(shapes, 5)
    return p, arr, w, v


@pytest.mark.parametrize("m", [0, 1])
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("model,shapes,qi", CASES)
def test_storage_emulations_meet_the_bound(model, shapes, qi, inputs, m):
    p, arr, w, v = prepare(model, shapes, inputs)
    want, jabs = reference(model, w, v, p, arr, m)
    r1 = fb.check(emulate(model, w, v, p, arr, m), want, jabs, v, m, fb.constant(1, shapes, False), fb.U[1], "fp32 storage")
    r2 = fb.check(emulate(model, w, v, p, arr, m, store=bf16), want, jabs, v, m, fb.constant(2, shapes, False), fb.U[2],
                  "bf16 storage")
    r3 = fb.check(emulate(model, w, v, p, arr, m, fp32_math=True), want, jabs, v, m, fb.constant(3, shapes, True), fb.U[3],
                  "fp32 storage + fp32 arithmetic")
    # the rounding is there (the emulation is not fp64 in disguise) and well inside the bound
    assert 0 < r1 < 1 and 0 < r2 < 1 and 0 < r3 < 1


@pytest.mark.parametrize("fault", ["transpose", "drop_row", "scale", "scale_by_2", "bf16_mid"])
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("model,shapes,qi", CASES)
def test_each_fault_violates_the_bound(model, shapes, qi, inputs, fault):
    p, arr, w, v = prepare(model, shapes, inputs)
    for m in (0, 1):
        want, jabs = reference(model, w, v, p, arr, m)
        got = emulate(model, w, v, p, arr, m, fault=fault, q_index=qi)
        assert fb.ratio(got, want, jabs, v, m, fb.constant(1, shapes, False), fb.U[1]) > 1, (fault, m)
        # ... and the fp32-MFMA form's wider bound still catches it
        assert fb.ratio(got, want, jabs, v, m, fb.constant(3, shapes, True), fb.U[3]) > 1, (fault, m)


def test_bf16_rounding_helper():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9, -3.0e-5])
    y = bf16(x)
    assert y[0] == 1.0 and y[1] == 1.0 and y[2] == 1.0 + 4 * 2.0 ** -8 and y[3] == 1.0  # (ties to even)
    assert np.all((y.astype(np.float32).view(np.uint32) & 0xFFFF) == 0)
    assert np.all(np.abs(y - x) <= 2.0 ** -8 * np.abs(x))


def test_constant_follows_the_form():
    assert fb.constant(1, (20,) * 6, True) == 8
    assert fb.constant(2, (16,) * 4, True) == 8
    assert fb.constant(3, (20,) * 6, True) == 128
    assert fb.constant(3, (20,) * 6, False) == 8          # mode 3 on a plan without fp32-MFMA kernels runs as mode 1

"""
GPU tests of the vector-Jacobian product u -> dT(w)^T u (sdfs_apply_vjp / sdfs_apply_vjp_dev) on every kernel plan,
of the transposed linear solve built on it (sdfs_solve_linear_dev, transpose = 1), of the adjoint gradient
(wc_ratio_gradient) and of the "gd" solver, all against the oracle's own VJP (oracle/ssy.py vjp_ssy, oracle/gcy.py
vjp_gcy, its C twin's mode 2; tests/test_oracle_vjp.py pins those to a dense J^T).

The VJP has no kernels of its own: each plan runs its J.v kernels with the transposed matrices and the two diagonal
scalings swapped.  Every case runs on two sets of inputs:
  (a) the discretisation's Rouwenhorst tensors, which are centrosymmetric (Q[i, j] = Q[n-1-i, n-1-j]);
  (b) the same arrays with every transition tensor replaced by one random, strictly positive, row-stochastic matrix
      that is not centrosymmetric, copied into every conditioning slice (identical slices keep the handle on the
      unconditional path the VJP needs) -- a kernel that reverses an index on both sides, or reads the wrong one of
      two mirrored tiles, passes (a) and fails (b).
Bound: max|got - want| <= 1e-11 max|want|, the same as the J.v tests.  Each case asserts the plan it is meant to run
on from describe_plan().  Every test runs under its own time limit (SIGALRM).
"""
import contextlib
import os
import signal

import numpy as np
import pytest

from test_hip_pad_plan import SHAPES as PAD_SHAPES
from test_hip_small_plan import CASES as SMALL_CASES
from test_hip_pair_plan import SSY_SHAPES as PAIR_SSY_SHAPES

pytestmark = pytest.mark.gpu

VJP_RTOL = 1e-11
QIDX = {"ssy": (1, 3, 5, 7), "gcy": (1, 3, 5, 8, 11, 14)}      # transition tensors in each model's arrays tuple
INPUTS = ["rouwenhorst", "random"]

SMALL = "small-grid plan pass"
PAIR = "pair plan pass"
PADDED = "padded pair plan pass"
STREAMED_MID = "persistent, next tile in flight"


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


@pytest.fixture(autouse=True)
def time_limit(request):
    seconds = getattr(request.function, "time_limit_s", 240)

    def expire(signum, frame):
        raise TimeoutError(f"test exceeded its {seconds} s limit")
    old = signal.signal(signal.SIGALRM, expire)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def limit(seconds):
    def mark(fn):
        fn.time_limit_s = seconds
        return fn
    return mark


@contextlib.contextmanager
def env(**kw):
    """Create-time knobs: set (or, for None, unset) while an operator is built, restored afterwards."""
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def random_transition(rng, n):
    """Strictly positive, row-stochastic, not centrosymmetric."""
    q = rng.random((n, n)) + 0.05
    q /= q.sum(axis=1, keepdims=True)
    assert not np.allclose(q, q[::-1, ::-1], rtol=1e-6, atol=0.0)
    return q


def model_inputs(S, model, shapes, inputs, seed=0):
    """(params, arrays) of the library's discretisation; inputs = "random": every transition tensor replaced by one
    random matrix per axis, the same in every conditioning slice."""
    m = S.SSY() if model == "ssy" else S.GCY()
    arr = list((S.discretize_ssy if model == "ssy" else S.discretize_gcy)(m, shapes))
    if inputs == "random":
        rng = np.random.default_rng(1000 + seed)
        for i in QIDX[model]:
            q = random_transition(rng, arr[i].shape[-1])
            arr[i] = np.ascontiguousarray(np.broadcast_to(q, arr[i].shape))
    return m.params, arr


def build(S, model, shapes, params, arrays, **knobs):
    with env(**knobs):
        return S.KoopmansOperator(model, shapes, params, arrays)


def oracle(model, shapes, params, arrays):
    from oracle.c_oracle import COperator
    return COperator(model, shapes, params, arrays)


def assert_plan(op, marker):
    """marker: SMALL, PAIR (not padded), PADDED, or None for the generic tiles (none of the plans)."""
    desc = op.describe_plan()
    if marker is None:
        assert SMALL not in desc and PAIR not in desc, desc
    elif marker == PAIR:
        assert PAIR in desc and PADDED not in desc, desc
    else:
        assert marker in desc, desc
    return desc


def inputs_wu(shapes, seed):
    rng = np.random.default_rng(seed)
    return 300 + 600 * rng.random(shapes), rng.standard_normal(shapes)


def assert_close(got, want, what):
    err = float(np.max(np.abs(got - want)))
    scale = float(np.max(np.abs(want)))
    assert err <= VJP_RTOL * scale, f"{what}: max|got - want| = {err:.3e}, {err / scale:.3e} of max|want|"


def check_vjp(op, ref, shapes, seed, what):
    w, u = inputs_wu(shapes, seed)
    w0, u0 = w.copy(), u.copy()
    got = op.vjp(w, u)
    np.testing.assert_array_equal(w, w0)                      # inputs never mutated
    np.testing.assert_array_equal(u, u0)
    assert_close(got, ref.vjp(w, u), what)


def vjp_cases(S, model, shapes, inputs, marker, seed=0, **knobs):
    params, arr = model_inputs(S, model, shapes, inputs, seed)
    op = build(S, model, shapes, params, arr, **knobs)
    assert_plan(op, marker)
    ref = oracle(model, shapes, params, arr)
    check_vjp(op, ref, shapes, seed + 7, f"{model} {shapes} {inputs} {knobs}")
    op.close()


# -- the small-grid plan (fast_kernels.hpp: small_tile_kernel) ----------------------------------------------------------
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("wpt", [1, 4])
@pytest.mark.parametrize("run", [0, 4])
@pytest.mark.parametrize("model,shapes", SMALL_CASES)
def test_vjp_small_plan(S, model, shapes, run, wpt, inputs):
    vjp_cases(S, model, shapes, inputs, SMALL, SDFS_PLAN=None, SDFS_SMALL_R=run if run else None, SDFS_SMALL_WPT=wpt)


# -- the generic tiles (pass_kernel.hpp) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("model,shapes", [("ssy", (4, 7, 6, 5)), ("ssy", (20, 5, 3, 17)), ("ssy", (2, 2, 2, 2)),
                                          ("gcy", (3, 4, 2, 3, 2, 4))])
def test_vjp_generic_tiles(S, model, shapes, inputs):
    vjp_cases(S, model, shapes, inputs, None, SDFS_PLAN="classic")


# -- the pair plan (fast_kernels.hpp: slice_kernel + line_kernel) --------------------------------------------------------
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("shapes", PAIR_SSY_SHAPES)
def test_vjp_pair_plan_4d(S, shapes, inputs):
    vjp_cases(S, "ssy", shapes, inputs, PAIR, SDFS_PLAN="pair")


@limit(300)
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("shapes", [(16,) * 6, (16, 16, 20, 20, 16, 16), (24, 24, 16, 16, 16, 16), (16, 16, 16, 16, 32, 32)])
def test_vjp_pair_plan_6d(S, shapes, inputs):
    """A slice pass and two line passes, the middle one in its one-tile-per-workgroup form (SDFS_LINE_STREAM=0)."""
    params, arr = model_inputs(S, "gcy", shapes, inputs)
    op = build(S, "gcy", shapes, params, arr, SDFS_PLAN="pair", SDFS_LINE_STREAM=0)
    assert "streamed" not in assert_plan(op, PAIR)
    check_vjp(op, oracle("gcy", shapes, params, arr), shapes, 7, f"gcy {shapes} {inputs}")
    op.close()


# -- the streamed persistent middle pass (stream_kernels.hpp) ------------------------------------------------------------
@limit(900)
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("shapes,knobs", [((20, 20, 20, 20, 16, 16), dict(SDFS_PLAN="pair", SDFS_LINE_STREAM=None)),
                                          ((16,) * 6, dict(SDFS_PLAN="pair", SDFS_LINE_STREAM=7)),
                                          ((20,) * 6, dict(SDFS_PLAN=None, SDFS_LINE_STREAM=None))],
                         ids=["gcy20x4-16x2", "gcy16-forced", "gcy20"])
def test_vjp_streamed_middle_pass(S, shapes, knobs, inputs):
    """The persistent middle pass hands out its tiles by ticket; the ticket words must be back at zero after a launch,
    so the VJP runs twice in a row on one handle, at the same w and with a different u (the second result cannot
    be the first one's stale output)."""
    params, arr = model_inputs(S, "gcy", shapes, inputs)
    op = build(S, "gcy", shapes, params, arr, **knobs)
    assert STREAMED_MID in assert_plan(op, PAIR), op.describe_plan()
    ref = oracle("gcy", shapes, params, arr)
    w, u = inputs_wu(shapes, 31)
    u2 = np.random.default_rng(32).standard_normal(shapes)
    for k, uu in enumerate((u, u2)):
        assert_close(op.vjp(w, uu), ref.vjp(w, uu), f"gcy {shapes} {inputs} application {k}")
    op.close()


# -- the padded pair plan (pad_kernels.hpp) ------------------------------------------------------------------------------
@limit(300)
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("shapes", PAD_SHAPES)
def test_vjp_padded_plan(S, shapes, inputs):
    model = "gcy" if len(shapes) == 6 else "ssy"
    wide = max(shapes) > 16 and min(shapes) <= 16           # (as tests/test_hip_pad_plan.py builds them)
    params, arr = model_inputs(S, model, shapes, inputs)
    op = build(S, model, shapes, params, arr, SDFS_PAD_PLAN=2 if wide else 1)
    assert assert_plan(op, PADDED).count(PADDED) == len(shapes) // 2, op.describe_plan()
    check_vjp(op, oracle(model, shapes, params, arr), shapes, 7, f"{model} {shapes} {inputs}")
    op.close()


# -- the "- u" form the transposed BiCGSTAB launches ---------------------------------------------------------------------
FAMILIES = [("ssy", (15,) * 4, dict(SDFS_PLAN=None), SMALL),
            ("ssy", (4, 7, 6, 5), dict(SDFS_PLAN="classic"), None),
            ("ssy", (16,) * 4, dict(SDFS_PLAN="pair"), PAIR),
            ("gcy", (16,) * 6, dict(SDFS_PLAN="pair", SDFS_LINE_STREAM=0), PAIR),
            ("gcy", (20, 20, 20, 20, 16, 16), dict(SDFS_PLAN="pair"), STREAMED_MID),
            ("gcy", (10,) * 6, dict(SDFS_PLAN=None), PADDED)]
FAMILY_IDS = ["small", "generic", "pair4d", "pair6d", "streamed", "padded"]


@limit(300)
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("model,shapes,knobs,marker", FAMILIES, ids=FAMILY_IDS)
def test_vjp_minus_identity_on_device(S, model, shapes, knobs, marker, inputs):
    """vjp_dev(..., minus_identity=True) after linearize_dev: out = J(w)^T u - u, device pointers in and out."""
    import torch
    params, arr = model_inputs(S, model, shapes, inputs)
    op = build(S, model, shapes, params, arr, **knobs)
    if marker == STREAMED_MID:
        assert STREAMED_MID in assert_plan(op, PAIR)
    else:
        assert_plan(op, marker)
    w, u = inputs_wu(shapes, 41)
    wd, ud = op._to_dev(w, u)
    tw, out = torch.empty_like(wd), torch.empty_like(wd)
    op.linearize_dev(wd.data_ptr(), tw.data_ptr())
    op.vjp_dev(ud.data_ptr(), out.data_ptr(), minus_identity=True)
    op.synchronize()
    got = out.cpu().numpy()
    np.testing.assert_array_equal(ud.cpu().numpy(), u)        # the input vector is left alone
    ref = oracle(model, shapes, params, arr)
    assert_close(got, ref.vjp(w, u) - u, f"{model} {shapes} {inputs} minus identity")
    # the plain form on the same linearisation
    op.vjp_dev(ud.data_ptr(), out.data_ptr(), minus_identity=False)
    op.synchronize()
    assert_close(out.cpu().numpy(), ref.vjp(w, u), f"{model} {shapes} {inputs}")
    op.close()


# -- handle state ------------------------------------------------------------------------------------------------------
@limit(300)
@pytest.mark.parametrize("model,shapes,marker", [("gcy", (16,) * 6, PAIR), ("ssy", (15,) * 4, SMALL)], ids=["gcy16", "ssy15"])
def test_vjp_is_fp64_after_an_fp32_newton_solve(S, model, shapes, marker):
    """A Newton solve with fp32 Krylov storage and fp32 MFMA J.v (krylov_f32 = 3) on the same handle leaves the VJP on
    its fp64 kernels: sdfs_apply_vjp_dev clears the handle's fp32 flag for the application and restores it."""
    params, arr = model_inputs(S, model, shapes, "rouwenhorst")
    op = build(S, model, shapes, params, arr, SDFS_PLAN=None)
    assert_plan(op, marker)
    ref = oracle(model, shapes, params, arr)
    x, _, info = op.solve(np.full(shapes, 800.0), "newton", tol=1e-8, inner_rtol=1e-6, inner_atol=0.0, krylov_f32=3)
    assert info["status"] == 0
    check_vjp(op, ref, shapes, 51, f"{model} {shapes} after an fp32 solve")
    # at the fixed point too, and a second fp32 solve after the VJP still converges to the same point
    u = np.random.default_rng(52).standard_normal(shapes)
    assert_close(op.vjp(x, u), ref.vjp(x, u), f"{model} {shapes} at the fixed point")
    x2, _, info2 = op.solve(np.full(shapes, 800.0), "newton", tol=1e-8, inner_rtol=1e-6, inner_atol=0.0, krylov_f32=3)
    assert info2["status"] == 0
    assert np.max(np.abs(x2 - x)) <= 1e-9 * np.max(np.abs(x))
    op.close()


# -- the transposed solve, with the residual computed by the oracle ----------------------------------------------------
SOLVE_CASES = [("ssy", (15,) * 4, SMALL), ("ssy", (4, 7, 6, 5), None), ("gcy", (10,) * 6, PADDED),
               ("gcy", (16,) * 6, PAIR), ("gcy", (20,) * 6, STREAMED_MID)]
SOLVE_IDS = ["ssy15-small", "ssy4765-generic", "gcy10-padded", "gcy16-pair", "gcy20-streamed"]


def default_operator(S, model, shapes, marker, inputs="rouwenhorst"):
    """The operator the library builds by default (SSY (4, 7, 6, 5): on the generic tiles under SDFS_PLAN=classic)."""
    params, arr = model_inputs(S, model, shapes, inputs)
    op = build(S, model, shapes, params, arr, SDFS_PLAN="classic" if marker is None else None)
    if marker == STREAMED_MID:
        assert STREAMED_MID in assert_plan(op, PAIR)
    else:
        assert_plan(op, marker)
    return op, params, arr


@limit(600)
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("model,shapes,marker", SOLVE_CASES, ids=SOLVE_IDS)
def test_transposed_solve_residual_by_the_oracle(S, model, shapes, marker, inputs):
    """y = (I - J(w)^T)^{-1} b at a Newton fixed point: |y - J_oracle(w)^T y - b|_2 <= 1e-9 |b|_2.  (The self-residual
    of tests/test_hip_sensitivity.py uses the library's own VJP, which a wrong VJP would pass.)"""
    op, params, arr = default_operator(S, model, shapes, marker, inputs)
    w, _, info = op.solve(np.full(shapes, 800.0), "newton", tol=1e-8)
    assert info["status"] == 0
    b = np.random.default_rng(3).standard_normal(shapes)
    y = op.solve_linear(w, b, transpose=True, rtol=1e-12)
    r = y - oracle(model, shapes, params, arr).vjp(w, y) - b
    rel = np.linalg.norm(r) / np.linalg.norm(b)
    assert rel <= 1e-9, f"{model} {shapes}: oracle residual {rel:.3e}"
    op.close()


# -- the adjoint gradient against the forward sensitivities ------------------------------------------------------------
GRAD_CASES = [("ssy", (15,) * 4, SMALL), ("ssy", (16,) * 4, SMALL), ("gcy", (10,) * 6, PADDED),
              ("gcy", (16,) * 6, PAIR), ("gcy", (20,) * 6, STREAMED_MID)]


@limit(900)
@pytest.mark.parametrize("model,shapes,marker", GRAD_CASES, ids=["ssy15", "ssy16", "gcy10", "gcy16", "gcy20"])
def test_gradient_equals_forward_sensitivities(S, model, shapes, marker):
    """wc_ratio_gradient (one transposed solve, on the VJP) against sum(g * wc_ratio_sensitivities[name]) (J.v only,
    checked against the oracle and finite differences elsewhere), every supported parameter, on the default plan."""
    from sdfs_via_autodiff_amd import sensitivity as sens
    op, params, arr = default_operator(S, model, shapes, marker)
    w, _, info = op.solve(np.full(shapes, 800.0), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
    assert info["status"] == 0
    op.close()
    m = S.SSY() if model == "ssy" else S.GCY()
    with env(SDFS_PLAN=None):
        g = np.random.default_rng(7).random(shapes)
        fwd = S.wc_ratio_sensitivities(m, shapes, w, rtol=1e-12)
        adj = S.wc_ratio_gradient(m, shapes, w, g, rtol=1e-12)
    supported = sens.SSY_SUPPORTED if model == "ssy" else sens.GCY_SUPPORTED
    assert set(adj) == set(supported) == set(fwd)
    for name in supported:
        want = float(np.sum(g * fwd[name]))
        assert abs(adj[name] - want) <= 1e-8 * abs(want), f"{model} {shapes} {name}: {adj[name]!r} vs {want!r}"


# -- "gd" on a non-generic plan against the oracle's restatement fed with the oracle's VJP -----------------------------
@limit(300)
def test_gd_on_the_small_grid_plan_matches_oracle(S):
    from oracle import solvers as osol, ssy as ossy
    shapes = (15,) * 4
    params, arr = model_inputs(S, "ssy", shapes, "rouwenhorst")
    op = build(S, "ssy", shapes, params, arr, SDFS_PLAN=None)
    assert_plan(op, SMALL)
    w0 = np.full(shapes, 800.0)
    xg, st = S.fixed_point_via_gradient_decent(op, w0, maxiter=25)
    oT = lambda x: ossy.T_ssy_factorised(x, shapes, params, arr)
    oV = lambda x, r: ossy.vjp_ssy(x, r, shapes, params, arr)
    xo, no = osol.fixed_point_via_gradient_decent(oT, w0, oV, maxiter=25)
    assert st["iter_num"] == no == 25
    np.testing.assert_allclose(xg, xo, rtol=1e-9)
    np.testing.assert_allclose(st["errors"], osol.fixed_point_via_gradient_decent.last_errors, rtol=1e-6)
    r0, rg = oT(w0) - w0, oT(xg) - xg
    assert np.vdot(rg, rg) < np.vdot(r0, r0)
    op.close()

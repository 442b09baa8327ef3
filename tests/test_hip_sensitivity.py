"""
GPU tests of the parameter sensitivities of the wealth-consumption ratio (sdfs_param_tangent_dev,
sdfs_solve_linear_dev, sdfs_via_autodiff_amd/sensitivity.py):

 (1) the tangent of T at a fixed w against Richardson-extrapolated central differences of the oracle's T, every
     supported parameter, one shape on each kernel plan;
 (2) dw*/dp at 3^4 / 3^6 against a dense solve of (I - J(w*)) with numpy, the right-hand side by complex-step
     differentiation of the oracle's T (exact to rounding);
 (3) dw*/dp for beta and gamma against central differences of two tight GPU Newton solves (GCY 16^6, 20^6);
 (4) the adjoint gradient against the forward sensitivities;
 (5) the linear solves' true residual, plain and transposed;
 (6) the refusals.
Every test runs under its own time limit (SIGALRM).
"""
import contextlib
import ctypes as C
import os
import signal

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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
def plan_env(which):
    old = os.environ.get("SDFS_PLAN")
    if which is None:
        os.environ.pop("SDFS_PLAN", None)
    else:
        os.environ["SDFS_PLAN"] = which
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SDFS_PLAN", None)
        else:
            os.environ["SDFS_PLAN"] = old


def model_of(S, kind, **over):
    from sdfs_via_autodiff_amd import sensitivity as sens
    cls, names = (S.SSY, sens.SSY_PARAMS) if kind == "ssy" else (S.GCY, sens.GCY_PARAMS)
    d = dict(zip(names, cls().params))
    d.update(over)
    return cls(**d)


def supported(kind):
    from sdfs_via_autodiff_amd import sensitivity as sens
    return sens.SSY_SUPPORTED if kind == "ssy" else sens.GCY_SUPPORTED


def names_of(kind):
    from sdfs_via_autodiff_amd import sensitivity as sens
    return sens.SSY_PARAMS if kind == "ssy" else sens.GCY_PARAMS


def disc(S, kind):
    return S.discretize_ssy if kind == "ssy" else S.discretize_gcy


def tangent_fn(S, kind):
    return S.discretize_ssy_tangent if kind == "ssy" else S.discretize_gcy_tangent


def oracle_T(kind, shapes, params, arrays, c_oracle=False):
    if c_oracle:
        from oracle.c_oracle import COperator
        return COperator(kind, shapes, params, arrays)
    from oracle import ssy, gcy
    f = ssy.T_ssy_factorised if kind == "ssy" else gcy.T_gcy_factorised
    return lambda w: f(w, shapes, params, arrays)


def oracle_jvp(kind, shapes, params, arrays):
    from oracle import ssy, gcy
    f = ssy.jvp_ssy if kind == "ssy" else gcy.jvp_gcy
    return lambda w, v: f(w, v, shapes, params, arrays)


# -- (1) tangent of T at a fixed w ------------------------------------------------------------------------------------
# (model, shapes, SDFS_PLAN, text the plan description must hold, C oracle)
PLAN_CASES = [
    ("ssy", (15, 15, 15, 15), None, "small-grid plan", False),
    ("ssy", (4, 7, 6, 5), "classic", None, False),
    ("gcy", (10,) * 6, None, "padded pair plan", False),
    ("gcy", (16,) * 6, None, "pair plan pass", True),
]


@limit(600)
@pytest.mark.parametrize("kind,shapes,plan,marker,c_oracle", PLAN_CASES,
                         ids=["ssy15-small", "ssy4765-generic", "gcy10-padded", "gcy16-pair"])
def test_param_tangent_vs_richardson_central_differences(S, kind, shapes, plan, marker, c_oracle):
    m = model_of(S, kind)
    arr = disc(S, kind)(m, shapes)
    with plan_env(plan):
        op = S.KoopmansOperator(kind, shapes, m.params, arr)
    desc = op.describe_plan()
    if marker:
        assert marker in desc, desc
        if marker == "pair plan pass":
            assert "padded" not in desc, desc
    else:
        assert "pair plan" not in desc and "small-grid plan" not in desc, desc
    w = 500.0 + 200.0 * np.random.default_rng(sum(shapes)).random(shapes)   # a non-constant w, not a fixed point
    p0 = dict(zip(names_of(kind), m.params))
    for name in supported(kind):
        dp, da = tangent_fn(S, kind)(m, shapes, name)
        got = op.param_tangent(w, dp, da)
        h = 1e-4 * abs(p0[name])

        def cd(step):
            mp, mm = model_of(S, kind, **{name: p0[name] + step}), model_of(S, kind, **{name: p0[name] - step})
            Tp = oracle_T(kind, shapes, mp.params, disc(S, kind)(mp, shapes), c_oracle)(w)
            Tm = oracle_T(kind, shapes, mm.params, disc(S, kind)(mm, shapes), c_oracle)(w)
            return (Tp - Tm) / (2.0 * step)
        want = (4.0 * cd(h / 2) - cd(h)) / 3.0
        scale = np.max(np.abs(want))
        err = np.max(np.abs(got - want)) / scale
        assert err <= 1e-7, f"{kind} {shapes} {name}: {err:.3e} relative to max|dT/dp| = {scale:.3e}"
    op.close()


# -- (2) exact small grids --------------------------------------------------------------------------------------------
def complex_step_tangent(kind, shapes, params, arrays, dparams, darrays, w, h=1e-30):
    """dT(w)/dp along (dparams, darrays) by the complex step: Im T(p + i h d) / h, exact to rounding."""
    pc = tuple(complex(p, h * d) for p, d in zip(params, dparams))
    ac = tuple(np.asarray(a, dtype=np.complex128) + 1j * h * np.asarray(d) for a, d in zip(arrays, darrays))
    return np.imag(oracle_T(kind, shapes, pc, ac)(w)) / h


@limit(300)
@pytest.mark.parametrize("kind,shapes", [("ssy", (3,) * 4), ("gcy", (3,) * 6)])
def test_sensitivities_match_dense_implicit_function_theorem(S, kind, shapes):
    from oracle.solvers import newton_polish
    m = model_of(S, kind)
    arr = disc(S, kind)(m, shapes)
    op = S.KoopmansOperator(kind, shapes, m.params, arr)
    x0, _, _ = op.solve(np.full(shapes, 800.0), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
    f, jv = oracle_T(kind, shapes, m.params, arr), oracle_jvp(kind, shapes, m.params, arr)
    w = newton_polish(f, jv, x0)
    assert np.max(np.abs(f(w) - w)) < 1e-10
    N = w.size
    J = np.empty((N, N))
    for k in range(N):
        e = np.zeros(N); e[k] = 1.0
        J[:, k] = jv(w, e.reshape(shapes)).ravel()
    A = np.eye(N) - J
    got = S.wc_ratio_sensitivities(m, shapes, w, rtol=1e-13)
    assert set(got) == set(supported(kind))
    for name in supported(kind):
        dp, da = tangent_fn(S, kind)(m, shapes, name)
        rhs = complex_step_tangent(kind, shapes, m.params, arr, dp, da, w)
        want = np.linalg.solve(A, rhs.ravel()).reshape(shapes)
        err = np.max(np.abs(got[name] - want)) / np.max(np.abs(want))
        assert got[name].shape == shapes
        assert err <= 1e-9, f"{kind} {name}: {err:.3e}"
    op.close()


# -- (3) finite differences of the fixed point -------------------------------------------------------------------------
NEWTON_TOL = 1e-10          # sup-norm Newton step at which the solves stop
FD_STEP = 1e-6              # central-difference step, relative to |p|


def newton_fixed_point(S, kind, shapes, model, x_init):
    op = S.KoopmansOperator(kind, shapes, model.params, disc(S, kind)(model, shapes))
    x, _, info = op.solve(x_init, "newton", tol=NEWTON_TOL, inner_rtol=1e-12, inner_atol=0.0)
    assert info["status"] == 0
    op.close()
    return x


@limit(600)
@pytest.mark.parametrize("shapes", [(16,) * 6, (20,) * 6], ids=["gcy16", "gcy20"])
def test_sensitivities_vs_central_differences_of_newton_solves(S, shapes):
    """Newton to a sup-norm step of 1e-10 at p and at p +- 1e-6 |p|; the central difference is then accurate to
    ~(1e-6 / (1 - beta))^2 ~ 1e-6 relative (truncation) -- the bound below is 2e-5."""
    m = model_of(S, "gcy")
    w = newton_fixed_point(S, "gcy", shapes, m, np.full(shapes, 800.0))
    got = S.wc_ratio_sensitivities(m, shapes, w, wrt=("β", "γ"), rtol=1e-11)
    p0 = dict(zip(names_of("gcy"), m.params))
    for name in ("β", "γ"):
        h = FD_STEP * abs(p0[name])
        wp = newton_fixed_point(S, "gcy", shapes, model_of(S, "gcy", **{name: p0[name] + h}), w)
        wm = newton_fixed_point(S, "gcy", shapes, model_of(S, "gcy", **{name: p0[name] - h}), w)
        fd = (wp - wm) / (2.0 * h)
        err = np.max(np.abs(got[name] - fd)) / np.max(np.abs(fd))
        assert err <= 2e-5, f"{shapes} {name}: {err:.3e}"


# -- (4) adjoint against forward ---------------------------------------------------------------------------------------
@limit(300)
@pytest.mark.parametrize("kind,shapes", [("ssy", (7, 6, 5, 4)), ("gcy", (4, 3, 5, 3, 4, 6))])
def test_adjoint_gradient_equals_forward_sensitivities(S, kind, shapes):
    m = model_of(S, kind)
    w = newton_fixed_point(S, kind, shapes, m, np.full(shapes, 800.0))
    g = np.random.default_rng(7).random(shapes)
    fwd = S.wc_ratio_sensitivities(m, shapes, w, rtol=1e-12)
    adj = S.wc_ratio_gradient(m, shapes, w, g, rtol=1e-12)
    assert set(adj) == set(supported(kind)) == set(fwd)
    for name in supported(kind):
        want = float(np.sum(g * fwd[name]))
        assert abs(adj[name] - want) <= 1e-8 * abs(want), f"{kind} {name}: {adj[name]!r} vs {want!r}"


# -- (5) linear solves --------------------------------------------------------------------------------------------------
@limit(300)
@pytest.mark.parametrize("kind,shapes", [("ssy", (15,) * 4), ("ssy", (4, 7, 6, 5)), ("gcy", (10,) * 6), ("gcy", (16,) * 6)])
def test_linear_solve_residuals_plain_and_transposed(S, kind, shapes):
    m = model_of(S, kind)
    op = S.KoopmansOperator(kind, shapes, m.params, disc(S, kind)(m, shapes))
    w, _, _ = op.solve(np.full(shapes, 800.0), "newton", tol=1e-8)
    b = np.random.default_rng(3).standard_normal(shapes)
    x = op.solve_linear(w, b, rtol=1e-12)
    r = x - op.jvp(w, x) - b
    assert np.linalg.norm(r) / np.linalg.norm(b) <= 1e-10
    y = op.solve_linear(w, b, transpose=True, rtol=1e-12)
    r = y - op.vjp(w, y) - b
    assert np.linalg.norm(r) / np.linalg.norm(b) <= 1e-10
    op.close()


# -- (6) refusals -----------------------------------------------------------------------------------------------------
def test_transposed_solve_refused_on_conditional_tensors_plain_solve_works(S):
    rng = np.random.default_rng(5)
    shapes = (4, 5, 6, 7)
    m = S.SSY()
    arr = list(S.discretize_ssy(m, shapes))
    q = rng.random(arr[7].shape) + 0.05
    arr[7] = q / q.sum(axis=-1, keepdims=True)        # every z_Q[i] slice differs: no transposed product
    op = S.KoopmansOperator("ssy", shapes, m.params, arr)
    w, _, _ = op.solve(np.full(shapes, 800.0), "newton", tol=1e-8)
    b = rng.standard_normal(shapes)
    with pytest.raises(S.SdfsError, match="unconditional"):
        op.solve_linear(w, b, transpose=True)
    x = op.solve_linear(w, b, rtol=1e-12)
    assert np.linalg.norm(x - op.jvp(w, x) - b) / np.linalg.norm(b) <= 1e-10
    # the tangent itself works on such a handle (it needs no transposed product)
    dp, da = S.discretize_ssy_tangent(m, shapes, "β")
    da = list(da); da[7] = np.zeros_like(arr[7])
    Tw = op(w)
    np.testing.assert_allclose(op.param_tangent(w, dp, da), (Tw - 1.0) / m.β, rtol=1e-13)


def test_transition_tangents_and_unsupported_handles_are_refused(S):
    import torch
    from sdfs_via_autodiff_amd import _lib
    shapes = (3, 4, 2, 3, 5, 4)
    m = S.GCY()
    arr = S.discretize_gcy(m, shapes)
    op = S.KoopmansOperator("gcy", shapes, m.params, arr)
    w = np.full(shapes, 700.0)
    dp, da = S.discretize_gcy_tangent(m, shapes, "s_c")
    for i in (1, 3, 5, 8, 11, 14):
        bad = list(da); bad[i] = np.full(arr[i].shape, 1e-3)
        with pytest.raises(S.SdfsError, match="transition"):
            op.param_tangent(w, dp, bad)
    op.param_tangent(w, dp, da)                      # (the handle still works)
    # fp32 Krylov storage is refused by the linear solve
    wd = torch.from_numpy(w).cuda(); xd = torch.empty_like(wd)
    torch.cuda.synchronize()
    op.linearize_dev(wd.data_ptr())
    o = _lib.default_opts(); o.krylov_f32 = 1
    assert _lib.lib.sdfs_solve_linear_dev(op.handle, 0, C.byref(o), wd.data_ptr(), xd.data_ptr(), None, None) == _lib.SDFS_ERR_ARG
    op.synchronize()

    # dense
    D = S.DenseOperator(0.5 * np.full((4, 4), 0.25), 0.99, -10.0)
    with pytest.raises(S.SdfsError, match="unsharded discretised"):
        D.param_tangent(np.full(4, 2.0), np.zeros(len(D.params)), None)
    # continuous
    ssy = S.SSY()
    grids = S.build_grid(ssy, 3, 3, 3, 4)
    nodes, weights = S.qnwnorm([3] * 4)
    Tc = S.T_fun_factory((np.array(ssy.params), grids, nodes.T.copy(), weights), "quadrature", 3 * 3 * 3 * 4)
    with pytest.raises(S.SdfsError, match="unsharded discretised"):
        Tc.param_tangent(np.full(Tc.shapes, 800.0), np.zeros(len(Tc.params)), None)
    # sharded (one rank owning every index of its two axes)
    nd = len(shapes)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in arr]
    h = C.c_void_p()
    rc = _lib.lib.sdfs_create_sharded(
        _lib.SDFS_MODEL_GCY, nd, (C.c_int64 * nd)(*shapes), (C.c_double * 18)(*m.params), 18,
        (C.POINTER(C.c_double) * 15)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs]),
        (C.c_int64 * 15)(*[a.size for a in arrs]), 15, 0, 3, 0, shapes[3], 5, 0, shapes[5], C.byref(h))
    assert rc == 0, _lib.last_error(None)
    try:
        par = (C.c_double * 18)(*dp)
        assert _lib.lib.sdfs_param_tangent_dev(h, wd.data_ptr(), par, None, xd.data_ptr(), None) == _lib.SDFS_ERR_UNSUPPORTED
        assert _lib.lib.sdfs_solve_linear_dev(h, 0, None, wd.data_ptr(), xd.data_ptr(), None, None) == _lib.SDFS_ERR_UNSUPPORTED
    finally:
        _lib.lib.sdfs_destroy(h)
    op.close()

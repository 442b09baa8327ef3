"""
GPU tests of the persistence tangents (sdfs_param_tangent_gen_dev, k_sens_generator, sensitivity.py's persistence=True):

 (5) the device tangent of T at a fixed w against the complex step of the oracle's T along the true direction (dQ = G Q
     included), every persistence parameter: generic tiles, the edge extents 2 and 32, a 6-D grid, and a grid of more
     than one grid-stride sweep;
 (6) dw*/dρ and every other sensitivity against a dense solve of (I - J(w*)) with numpy;
 (7) the adjoint gradient of all 13 / 18 parameters against the forward sensitivities;
 (8) the C ABI: dgen = NULL is sdfs_param_tangent_dev bit for bit, and the refusals.
Every test runs under its own time limit (SIGALRM).
"""
import contextlib
import ctypes as C
import os
import signal

import numpy as np
import pytest

import persistence_oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


@pytest.fixture(autouse=True)
def time_limit(request):
    seconds = getattr(request.function, "time_limit_s", 120)

    def expire(signum, frame):
        raise TimeoutError(f"test exceeded its {seconds} s limit")
    old = signal.signal(signal.SIGALRM, expire)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


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


def model_of(S, kind):
    return S.SSY() if kind == "ssy" else S.GCY()


def all_names(kind):
    from sdfs_via_autodiff_amd import sensitivity as sens
    return sens.SSY_PARAMS if kind == "ssy" else sens.GCY_PARAMS


def persistence_names(kind):
    from sdfs_via_autodiff_amd import sensitivity as sens
    return sens.SSY_PERSISTENCE if kind == "ssy" else sens.GCY_PERSISTENCE


def disc(S, kind):
    return S.discretize_ssy if kind == "ssy" else S.discretize_gcy


def direction(S, kind, m, shapes, name):
    """(dparams, darrays, dgen) of any parameter; dgen is None for the ones that leave the matrices alone."""
    if name in persistence_names(kind):
        f = S.discretize_ssy_persistence_tangent if kind == "ssy" else S.discretize_gcy_persistence_tangent
        return f(m, shapes, name)
    f = S.discretize_ssy_tangent if kind == "ssy" else S.discretize_gcy_tangent
    return f(m, shapes, name) + (None,)


def oracle_jvp(kind, shapes, params, arrays):
    from oracle import ssy, gcy
    f = ssy.jvp_ssy if kind == "ssy" else gcy.jvp_gcy
    return lambda w, v: f(w, v, shapes, params, arrays)


# -- (5) tangent of T at a fixed w ------------------------------------------------------------------------------------
TANGENT_CASES = [
    ("ssy", (4, 7, 6, 5), "classic"),
    ("ssy", (2, 32, 3, 17), None),
    ("gcy", (3, 4, 2, 3, 5, 4), None),
    ("gcy", (13, 12, 11, 10, 12, 14), None),
]


@pytest.mark.parametrize("kind,shapes,plan", TANGENT_CASES, ids=["ssy4765-generic", "ssy2-32-3-17", "gcy342354", "gcy2.9M"])
def test_persistence_tangent_vs_complex_step_of_oracle_T(S, kind, shapes, plan):
    m = model_of(S, kind)
    arr = disc(S, kind)(m, shapes)
    with plan_env(plan):
        op = S.KoopmansOperator(kind, shapes, m.params, arr)
    if plan == "classic":
        desc = op.describe_plan()
        assert "pair plan" not in desc and "small-grid plan" not in desc, desc
    w = 500.0 + 200.0 * np.random.default_rng(sum(shapes)).random(shapes)   # a non-constant w, not a fixed point
    for name in persistence_names(kind):
        dp, da, dgen = direction(S, kind, m, shapes, name)
        got = op.param_tangent(w, dp, da, dgen=dgen)
        want = po.complex_step_tangent(kind, shapes, m.params, arr, dp, da, w)
        scale = np.max(np.abs(want))
        err = np.max(np.abs(got - want)) / scale
        print(f"{kind} {shapes} {name}: {err:.3e} relative to max|dT/dρ| = {scale:.3e}")
        assert err <= 1e-7, f"{kind} {shapes} {name}: {err:.3e} relative to max|dT/dρ| = {scale:.3e}"
    op.close()


# -- (6) exact small grids --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shapes", [("ssy", (3,) * 4), ("ssy", (4, 3, 5, 2)), ("gcy", (3,) * 6), ("gcy", (2, 3, 2, 3, 2, 3))])
def test_persistence_sensitivities_match_dense_implicit_function_theorem(S, kind, shapes):
    from oracle.solvers import newton_polish
    m = model_of(S, kind)
    arr = disc(S, kind)(m, shapes)
    op = S.KoopmansOperator(kind, shapes, m.params, arr)
    x0, _, _ = op.solve(np.full(shapes, 800.0), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
    op.close()
    f, jv = (lambda w: po.oracle_T(kind)(w, shapes, m.params, arr)), oracle_jvp(kind, shapes, m.params, arr)
    w = newton_polish(f, jv, x0)
    assert np.max(np.abs(f(w) - w)) < 1e-10
    N = w.size
    J = np.empty((N, N))
    for k in range(N):
        e = np.zeros(N); e[k] = 1.0
        J[:, k] = jv(w, e.reshape(shapes)).ravel()
    A = np.eye(N) - J
    got = S.wc_ratio_sensitivities(m, shapes, w, rtol=1e-13, persistence=True)
    assert set(got) == set(all_names(kind)) and len(got) == (13 if kind == "ssy" else 18)
    for name in all_names(kind):
        dp, da, _ = direction(S, kind, m, shapes, name)
        rhs = po.complex_step_tangent(kind, shapes, m.params, arr, dp, da, w)
        want = np.linalg.solve(A, rhs.ravel()).reshape(shapes)
        err = np.max(np.abs(got[name] - want)) / np.max(np.abs(want))
        print(f"{kind} {shapes} {name}: {err:.3e}")
        assert got[name].shape == shapes
        assert err <= 1e-8, f"{kind} {name}: {err:.3e}"
    # named persistences alone, and the default path keeps its keys
    one = persistence_names(kind)[0]
    sub = S.wc_ratio_sensitivities(m, shapes, w, wrt=[one, "β"], rtol=1e-13, persistence=True)
    assert list(sub) == [one, "β"]
    np.testing.assert_allclose(sub[one], got[one], rtol=0.0, atol=1e-10 * np.max(np.abs(got[one])))


# -- (7) adjoint against forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shapes", [("ssy", (7, 6, 5, 4)), ("gcy", (4, 3, 5, 3, 4, 6))])
def test_persistence_adjoint_gradient_equals_forward_sensitivities(S, kind, shapes):
    m = model_of(S, kind)
    op = S.KoopmansOperator(kind, shapes, m.params, disc(S, kind)(m, shapes))
    w, _, info = op.solve(np.full(shapes, 800.0), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
    assert info["status"] == 0
    op.close()
    g = np.random.default_rng(7).random(shapes)
    fwd = S.wc_ratio_sensitivities(m, shapes, w, rtol=1e-12, persistence=True)
    adj = S.wc_ratio_gradient(m, shapes, w, g, rtol=1e-12, persistence=True)
    assert set(adj) == set(all_names(kind)) == set(fwd)
    for name in all_names(kind):
        want = float(np.sum(g * fwd[name]))
        print(f"{kind} {name}: {adj[name]!r} vs {want!r}")
        assert abs(adj[name] - want) <= 1e-8 * abs(want), f"{kind} {name}: {adj[name]!r} vs {want!r}"
    # the default path is untouched by the keyword's existence
    from sdfs_via_autodiff_amd import sensitivity as sens
    supported = sens.SSY_SUPPORTED if kind == "ssy" else sens.GCY_SUPPORTED
    plain = S.wc_ratio_gradient(m, shapes, w, g, rtol=1e-12)
    assert tuple(plain) == supported
    for name in supported:
        assert abs(plain[name] - adj[name]) <= 1e-10 * abs(adj[name]), name


# -- (8) the C ABI -------------------------------------------------------------------------------------------------------
def _ptrs(arrs):
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in arrs]
    p = (C.POINTER(C.c_double) * len(keep))(
        *[a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None for a in keep])
    return p, keep


def test_null_generator_is_the_plain_tangent_bit_for_bit(S):
    import torch
    from sdfs_via_autodiff_amd import _lib
    shapes = (3, 4, 2, 3, 5, 4)
    m = S.GCY()
    arr = S.discretize_gcy(m, shapes)
    op = S.KoopmansOperator("gcy", shapes, m.params, arr)
    w = 500.0 + 200.0 * np.random.default_rng(1).random(shapes)
    wd = torch.from_numpy(w).cuda()
    a, b, c = torch.empty_like(wd), torch.empty_like(wd), torch.empty_like(wd)
    torch.cuda.synchronize()
    for name in ("γ", "s_c", "ρ_π"):
        dp, da = S.discretize_gcy_tangent(m, shapes, name)
        par = (C.c_double * 18)(*dp)
        ptr, keep = _ptrs(da)
        assert _lib.lib.sdfs_param_tangent_dev(op.handle, wd.data_ptr(), par, ptr, a.data_ptr(), None) == 0
        assert _lib.lib.sdfs_param_tangent_gen_dev(op.handle, wd.data_ptr(), par, ptr, None, b.data_ptr(), None) == 0
        gnull = (C.POINTER(C.c_double) * 6)()                       # six NULL entries: no generator either
        assert _lib.lib.sdfs_param_tangent_gen_dev(op.handle, wd.data_ptr(), par, ptr, gnull, c.data_ptr(), None) == 0
        op.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c), name
        # and through the wrapper
        np.testing.assert_array_equal(op.param_tangent(w, dp, da), op.param_tangent(w, dp, da, dgen=[None] * 6))
        np.testing.assert_array_equal(op.param_tangent(w, dp, da), a.cpu().numpy())
    op.close()


def test_generator_refused_on_conditional_tensors_and_handle_still_works(S):
    rng = np.random.default_rng(5)
    shapes = (4, 5, 6, 7)
    m = S.SSY()
    arr = list(S.discretize_ssy(m, shapes))
    q = rng.random(arr[7].shape) + 0.05
    arr[7] = q / q.sum(axis=-1, keepdims=True)        # every z_Q[i] slice differs
    op = S.KoopmansOperator("ssy", shapes, m.params, arr)
    w = 500.0 + 200.0 * rng.random(shapes)
    for name in ("ρ_z", "ρ"):
        dp, da, dgen = S.discretize_ssy_persistence_tangent(m, shapes, name)
        with pytest.raises(S.SdfsError, match="unconditional"):
            op.param_tangent(w, dp, da, dgen=dgen)
    dp, da = S.discretize_ssy_tangent(m, shapes, "β")
    Tw = op(w)
    np.testing.assert_allclose(op.param_tangent(w, dp, da), (Tw - 1.0) / m.β, rtol=1e-13)
    np.testing.assert_allclose(op.param_tangent(w, dp, da, dgen=[None] * 4), (Tw - 1.0) / m.β, rtol=1e-13)
    op.close()


def test_generator_argument_errors(S):
    import torch
    from sdfs_via_autodiff_amd import _lib
    shapes = (3, 4, 2, 3, 5, 4)
    m = S.GCY()
    arr = S.discretize_gcy(m, shapes)
    op = S.KoopmansOperator("gcy", shapes, m.params, arr)
    w = np.full(shapes, 700.0)
    wd = torch.from_numpy(w).cuda(); xd = torch.empty_like(wd)
    torch.cuda.synchronize()
    dp, da, dgen = S.discretize_gcy_persistence_tangent(m, shapes, "ρ_c")
    par = (C.c_double * 18)(*dp)
    states = [None if i in po.TRANSITION["gcy"] else d for i, d in enumerate(da)]
    sptr, skeep = _ptrs(states)
    # a NaN or an infinity inside a generator: SDFS_ERR_ARG; in the two ignored corners: accepted
    for k, bad in ((1, np.nan), (2, np.inf)):
        g = dgen[3].copy(); g[k, 1] = bad
        gptr, gkeep = _ptrs([None, None, None, g, None, None])
        rc = _lib.lib.sdfs_param_tangent_gen_dev(op.handle, wd.data_ptr(), par, sptr, gptr, xd.data_ptr(), None)
        assert rc == _lib.SDFS_ERR_ARG, rc
        with pytest.raises(S.SdfsError, match="finite"):
            op.param_tangent(w, dp, da, dgen=[None, None, None, g, None, None])
    g = dgen[3].copy(); g[0, 0] = np.nan; g[2, -1] = np.nan
    np.testing.assert_array_equal(op.param_tangent(w, dp, da, dgen=[None, None, None, g, None, None]),
                                  op.param_tangent(w, dp, da, dgen=dgen))
    # a non-zero transition tangent is refused without a generator (wrapper) and with one (C ABI)
    with pytest.raises(S.SdfsError, match="transition"):
        op.param_tangent(w, dp, da)
    aptr, akeep = _ptrs(da)
    gptr, gkeep = _ptrs(dgen)
    rc = _lib.lib.sdfs_param_tangent_gen_dev(op.handle, wd.data_ptr(), par, aptr, gptr, xd.data_ptr(), None)
    assert rc == _lib.SDFS_ERR_UNSUPPORTED and "transition" in _lib.last_error(op.handle)
    rc = _lib.lib.sdfs_param_tangent_gen_dev(op.handle, wd.data_ptr(), par, aptr, None, xd.data_ptr(), None)
    assert rc == _lib.SDFS_ERR_UNSUPPORTED and "transition" in _lib.last_error(op.handle)
    # wrong shapes are caught on the host
    with pytest.raises(ValueError):
        op.param_tangent(w, dp, da, dgen=dgen[:5])
    with pytest.raises(ValueError):
        op.param_tangent(w, dp, da, dgen=[None, None, None, dgen[3][:, :2], None, None])
    op.param_tangent(w, dp, da, dgen=dgen)           # (the handle still works)
    # dense, continuous and sharded handles refuse as sdfs_param_tangent_dev does
    D = S.DenseOperator(0.5 * np.full((4, 4), 0.25), 0.99, -10.0)
    with pytest.raises(S.SdfsError, match="unsharded discretised"):
        D.param_tangent(np.full(4, 2.0), np.zeros(len(D.params)), None, dgen=[None])
    op.close()

"""
GPU tests of the batch gradient (csrc/batch_adjoint.hpp, sdfs_batch_adjoint_dev, ``BatchOperator.adjoint``,
``gradient_batch``): one workgroup per member, checked per member against the oracle's transposed product (the true
residual of the solve), against the numpy restatement of the moments (tests/batch_adjoint_oracle.py), against the dense
truth <lambda, complex-step dT/dp>, against central differences of Newton solves through the discretisation, against the
single-problem path, and for independence of a member's bits from the batch, its place in it and the budget of a launch.
Every test runs under its own time limit (SIGALRM).

The shapes hit every form of the kernel:
    SSY (3,4,3,5)  180 points  registers, K = 1        GCY 4^6          4 096  global, K = 8
    SSY 5^4        625         K = 4                   SSY (7,13,11,9)  9 009  global, K = 20, row classes 8/16/12/12
    GCY 3^6        729         K = 4                   SSY 10^4        10 000  global, K = 20
    GCY (3,4,5,2,3,4) 1 440    K = 8                   GCY 5^6         15 625  global, K = 32
"""
import signal

import numpy as np
import pytest

import batch_adjoint_oracle as bao
from batch_family import member, package_model

pytestmark = pytest.mark.gpu

SHAPES = [("ssy", (3, 4, 3, 5)), ("ssy", (5,) * 4), ("gcy", (3,) * 6), ("gcy", (3, 4, 5, 2, 3, 4)), ("gcy", (4,) * 6),
          ("ssy", (7, 13, 11, 9)), ("ssy", (10,) * 4), ("gcy", (5,) * 6)]
NEWTON = dict(algorithm="newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)


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


def family(S, kind, count, start=0):
    return [package_model(S, kind, member(kind, b)) for b in range(start, start + count)]


_solved = {}
_adjoint = {}


def solved(S, kind, shapes, members):
    """w* of the first `members` family members by the batch Newton solve from 800 (once per module)."""
    key = (kind, shapes, members)
    if key not in _solved:
        res = S.solve_batch(family(S, kind, members), shapes, **NEWTON)
        assert np.all(res.status == 0), res.status
        _solved[key] = res.w
    return _solved[key]


def positive_g(shapes, B, seed=5):
    return 0.5 + np.random.default_rng(seed).random((B,) + shapes)


def adjoint3(S, kind, shapes):
    """B = 3, a random positive g per member, rtol 1e-12: (w, g, the outputs of BatchOperator.adjoint), once per module."""
    key = (kind, shapes)
    if key not in _adjoint:
        w = solved(S, kind, shapes, 3)
        g = positive_g(shapes, 3)
        op = S.BatchOperator.from_models(family(S, kind, 3), shapes)
        try:
            out = op.adjoint(w, g, rtol=1e-12, return_adjoint=True)
        finally:
            op.close()
        _adjoint[key] = (w, g, out)
    return _adjoint[key]


# ---------------------------------------------------------------- 1: the true residual of the transposed solve
@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_true_residual(S, kind, shapes):
    """|g - (lambda - J^T lambda)|_2 / |g|_2 <= 1e-10 with J^T by the oracle (the bound of
    test_linear_solve_residuals_plain_and_transposed); max|T w - w| <= 1e-9."""
    w, g, (mom, n_iter, n_apply, rel, res_T, status, lam) = adjoint3(S, kind, shapes)
    assert np.all(status == 0), status
    assert mom.shape == (3, 3 + len(shapes) + shapes[bao.AXES[kind][0]] + shapes[bao.AXES[kind][1]]
                         + int(np.prod(shapes)) // (shapes[bao.AXES[kind][0]] * shapes[bao.AXES[kind][1]]))
    for b in range(3):
        params, arrays = bao.oracle_inputs(kind, shapes, member(kind, b))
        r = g[b] - (lam[b] - bao.vjp(kind, shapes, params, arrays, w[b], lam[b]))
        true = np.linalg.norm(r) / np.linalg.norm(g[b])
        print(f"{kind} {shapes} member {b}: {n_iter[b]} iterations, {n_apply[b]} applications, true residual {true:.3e}, "
              f"recurrence {rel[b]:.3e}, resid_T {res_T[b]:.3e}")
        assert true <= 1e-10, (b, true)
        assert res_T[b] <= 1e-9, (b, res_T[b])
        # L, two per full iteration (one where it ends on |s|^2), one J^T per sweep (at most two restarts), the last H
        assert n_iter[b] > 0 and 2 * n_iter[b] <= n_apply[b] <= 2 * n_iter[b] + 5


# ---------------------------------------------------------------- 2: the moments of the device's own lambda
@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_moments_against_numpy_restatement(S, kind, shapes):
    """Entry by entry: s0 .. M3 within 1e-11 sum|terms| (worst-case fixed-order summation of <= 16 384 terms is 2e-12;
    a few ulp per term with a margin of about 5), R within 1e-10 sum|terms| (a difference of neighbours that differ by
    per cent, reached by different routes, with |theta| ~ 16-36 magnifying a power's rounding)."""
    w, g, (mom, _, _, _, _, status, lam) = adjoint3(S, kind, shapes)
    assert np.all(status == 0), status
    for b in range(3):
        params, arrays = bao.oracle_inputs(kind, shapes, member(kind, b))
        want, scale = bao.moments(kind, shapes, params, arrays, w[b], lam[b])
        got, want, scale = (bao.split(kind, shapes, x) for x in (mom[b], want, scale))
        for part, bound in (("s", 1e-11), ("M1", 1e-11), ("M2", 1e-11), ("M3", 1e-11), ("R", 1e-10)):
            gap = np.max(np.abs(got[part] - want[part]) / scale[part])
            print(f"{kind} {shapes} member {b} {part}: worst gap {gap:.3e} of sum|terms| (bound {bound:.0e})")
            assert np.all(np.abs(got[part] - want[part]) <= bound * scale[part]), (b, part, gap)


# ---------------------------------------------------------------- 3: the gradient against the dense truth
@pytest.mark.parametrize("kind,shapes", [("ssy", (3, 4, 3, 5)), ("ssy", (5,) * 4), ("gcy", (3,) * 6)])
def test_gradient_against_dense_truth(S, kind, shapes):
    """<lambda_dense, complex-step dT/dp> linearised at the device's w, all 13 / 18 parameters, within 1e-8 |want|."""
    w = solved(S, kind, shapes, 3)[:2]
    g = positive_g(shapes, 2, seed=9)
    models = family(S, kind, 2)
    res = S.gradient_batch(models, shapes, w, g, rtol=1e-12)
    assert res.plan == "batch" and np.all(res.status == 0) and res.lam is None
    assert res.grad.shape == (2, 13 if kind == "ssy" else 18)
    b = 1
    params, arrays = bao.oracle_inputs(kind, shapes, member(kind, b))
    lam = bao.dense_lambda(kind, shapes, params, arrays, w[b], g[b])
    truth = bao.truth_gradient(S, kind, shapes, models[b], params, arrays, w[b], lam)
    for k, nm in enumerate(res.names):
        want = truth[nm]
        print(f"{kind} {shapes} {nm}: {res.grad[b, k]!r} vs {want!r}, relative gap {abs(res.grad[b, k] - want) / abs(want):.2e}")
        assert abs(res.grad[b, k] - want) <= 1e-8 * abs(want), (nm, res.grad[b, k], want)


# ---------------------------------------------------------------- 4: end to end through the discretisation
@pytest.mark.parametrize("kind,shapes", [("ssy", (5,) * 4), ("gcy", (3,) * 6)])
def test_gradient_against_central_differences_of_newton_solves(S, kind, shapes):
    """One batch Newton solve of the 2P members p_k +- 1e-6 |p_k| (a sup-norm step of 1e-10); the central difference of
    <g, w*> is accurate to ~(1e-6 / (1 - beta))^2 ~ 1e-6 relative (truncation) -- the bound is 2e-5, as in
    test_sensitivities_vs_central_differences_of_newton_solves.  A persistence whose perturbed value would leave (0, 1)
    is stepped relative to 1 - rho."""
    from sdfs_via_autodiff_amd import sensitivity as sens
    names = sens.SSY_PARAMS if kind == "ssy" else sens.GCY_PARAMS
    pers = sens.SSY_PERSISTENCE if kind == "ssy" else sens.GCY_PERSISTENCE
    cls = S.SSY if kind == "ssy" else S.GCY
    base = package_model(S, kind, member(kind, 2))
    p0 = dict(zip(names, base.params))
    g = positive_g(shapes, 1, seed=13)[0]
    steps, models = [], []
    for nm in names:
        h = 1e-6 * abs(p0[nm])
        if nm in pers and not (0.0 < p0[nm] - h and p0[nm] + h < 1.0):
            h = 1e-6 * (1.0 - p0[nm])
        steps.append(h)
        models += [cls(**dict(p0, **{nm: p0[nm] + h})), cls(**dict(p0, **{nm: p0[nm] - h}))]
    res = S.solve_batch([base] + models, shapes, **NEWTON)
    assert np.all(res.status == 0), res.status
    phi = np.tensordot(res.w, g, axes=len(shapes))
    out = S.gradient_batch([base], shapes, res.w[:1], g, rtol=1e-12)
    assert np.all(out.status == 0)
    for k, nm in enumerate(names):
        fd = (phi[1 + 2 * k] - phi[2 + 2 * k]) / (2.0 * steps[k])
        gap = abs(out.grad[0, k] - fd) / abs(fd)
        print(f"{kind} {shapes} {nm}: {out.grad[0, k]!r} vs central difference {fd!r}, relative gap {gap:.2e}")
        assert gap <= 2e-5, (nm, out.grad[0, k], fd)


# ---------------------------------------------------------------- 5: the single-problem path (a cross-check, not the truth)
@pytest.mark.parametrize("kind,shapes", [("ssy", (10,) * 4), ("gcy", (5,) * 6)])
def test_consistent_with_single_problem_gradient(S, kind, shapes):
    """Against ``wc_ratio_gradient`` (the code this feature is built beside), within 1e-8 |want|."""
    w = solved(S, kind, shapes, 3)[:2]
    g = positive_g(shapes, 2, seed=17)
    models = family(S, kind, 2)
    res = S.gradient_batch(models, shapes, w, g, rtol=1e-12)
    assert res.plan == "batch" and np.all(res.status == 0)
    for b in range(2):
        want = S.wc_ratio_gradient(models[b], shapes, w[b], g[b], rtol=1e-12, persistence=True)
        for k, nm in enumerate(res.names):
            print(f"{kind} {shapes} member {b} {nm}: {res.grad[b, k]!r} vs {want[nm]!r}")
            assert abs(res.grad[b, k] - want[nm]) <= 1e-8 * abs(want[nm]), (b, nm, res.grad[b, k], want[nm])


# ---------------------------------------------------------------- 6: a member's bits are its own
def run_adjoint(S, models, shapes, w, g, check_every):
    op = S.BatchOperator.from_models(models, shapes)
    try:
        return op.adjoint(w, g, rtol=1e-10, check_every=check_every, return_adjoint=True)
    finally:
        op.close()


def same_bits(a, ia, b, ib):
    return (np.array_equal(a[6][ia], b[6][ib]) and np.array_equal(a[0][ia], b[0][ib]) and a[1][ia] == b[1][ib]
            and a[2][ia] == b[2][ib] and a[5][ia] == b[5][ib])


@pytest.mark.parametrize("kind,shapes", [("ssy", (5,) * 4), ("gcy", (4,) * 6)])
def test_member_independent_of_batch_and_budget(S, kind, shapes):
    w12 = solved(S, kind, shapes, 12)
    fam = family(S, kind, 12)
    g = positive_g(shapes, 1, seed=21)[0]
    ref = run_adjoint(S, fam, shapes, w12, g, 0)
    assert np.all(ref[5] == 0) and ref[1][5] > 0
    big = [fam[b % 12] for b in range(300)]
    wbig = np.stack([w12[b % 12] for b in range(300)])
    for check_every in (8, 64, 0):
        alone = run_adjoint(S, [fam[5]], shapes, w12[5:6], g, check_every)
        assert same_bits(alone, 0, ref, 5), check_every
        three = run_adjoint(S, [fam[5], fam[1], fam[2]], shapes, w12[[5, 1, 2]], g, check_every)
        assert same_bits(three, 0, ref, 5), check_every
        twelve = run_adjoint(S, fam, shapes, w12, g, check_every)
        assert same_bits(twelve, 5, ref, 5), check_every
        many = run_adjoint(S, big, shapes, wbig, g, check_every)
        assert same_bits(many, 137, ref, 5), check_every


# ---------------------------------------------------------------- 7: statuses
def test_zero_g_nan_w_and_iteration_limit(S):
    kind, shapes = "ssy", (5,) * 4
    w = solved(S, kind, shapes, 3)
    models = family(S, kind, 3)
    g = positive_g(shapes, 3, seed=23)
    clean = S.gradient_batch(models, shapes, w, g, return_adjoint=True)
    assert np.all(clean.status == 0)
    # g = 0 for member 1
    g0 = g.copy()
    g0[1] = 0.0
    res = S.gradient_batch(models, shapes, w, g0, return_adjoint=True)
    assert res.status[1] == 0 and res.n_iter[1] == 0 and res.rel_resid[1] == 0.0
    assert np.all(res.grad[1] == 0.0) and np.all(res.lam[1] == 0.0)
    for b in (0, 2):
        assert np.array_equal(res.grad[b], clean.grad[b]) and np.array_equal(res.lam[b], clean.lam[b])
    # a NaN in the w of member 1
    wn = w.copy()
    wn[1].flat[17] = np.nan
    res = S.gradient_batch(models, shapes, wn, g, return_adjoint=True)
    assert list(res.status) == [0, 2, 0], res.status
    assert np.all(np.isnan(res.grad[1])) and np.all(np.isnan(res.lam[1]))
    for b in (0, 2):
        assert np.array_equal(res.grad[b], clean.grad[b]) and np.array_equal(res.lam[b], clean.lam[b])
        assert res.n_iter[b] == clean.n_iter[b] and res.n_apply[b] == clean.n_apply[b]
    # one iteration
    res = S.gradient_batch(models, shapes, w, g, rtol=1e-10, inner_max_iter=1)
    assert np.all(res.status == 1) and np.all(res.n_iter == 1), (res.status, res.n_iter)
    assert np.all(np.isfinite(res.rel_resid)) and np.all(res.rel_resid > 1e-10), res.rel_resid
    assert np.all(np.isfinite(res.grad))


def test_fp32_krylov_vectors_are_refused(S):
    import ctypes as C
    import torch
    from sdfs_via_autodiff_amd import _lib
    shapes = (3, 4, 3, 5)
    op = S.BatchOperator.from_models(family(S, "ssy", 1), shapes)
    try:
        o = _lib.default_opts()
        o.krylov_f32 = 1
        t = torch.ones(op.size + op.adjoint_words(), dtype=torch.float64, device="cuda")
        z = np.zeros(1, dtype=np.int64)
        d = np.zeros(1)
        s = np.zeros(1, dtype=np.int32)
        rc = _lib.lib.sdfs_batch_adjoint_dev(op.handle, C.byref(o), t.data_ptr(), t.data_ptr(), 0, None,
                                             t.data_ptr() + 8 * op.size, z.ctypes.data_as(C.POINTER(C.c_int64)),
                                             z.ctypes.data_as(C.POINTER(C.c_int64)), d.ctypes.data_as(C.POINTER(C.c_double)),
                                             d.ctypes.data_as(C.POINTER(C.c_double)), s.ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc == _lib.SDFS_ERR_ARG
    finally:
        op.close()


# ---------------------------------------------------------------- 8: shapes beyond one CU
def test_loop_plan_equals_direct_gradients(S):
    kind, shapes = "ssy", (12,) * 4
    models = family(S, kind, 2)
    sol = S.solve_batch(models, shapes, **NEWTON)
    assert sol.plan == "loop" and np.all(sol.status == 0)
    g = positive_g(shapes, 2, seed=29)
    res = S.gradient_batch(models, shapes, sol.w, g)
    assert res.plan == "loop" and res.lam is None and res.grad.shape == (2, 13)
    for b in range(2):
        want = S.wc_ratio_gradient(models[b], shapes, sol.w[b], g[b], persistence=True)
        assert [want[nm] for nm in res.names] == list(res.grad[b])


# ---------------------------------------------------------------- 9: the plan says where the vectors live
def test_describe_plan_names_the_adjoint_form(S):
    for shapes, where in (((3, 4, 3, 5), "in registers"), ((10,) * 4, "in global memory")):
        op = S.BatchOperator.from_models(family(S, "ssy", 2), shapes)
        try:
            lines = [ln for ln in op.describe_plan().splitlines() if ln.startswith("adjoint:")]
        finally:
            op.close()
        assert len(lines) == 1 and where in lines[0] and "budget" in lines[0], lines

"""
GPU tests of the batched Newton-Krylov solve (csrc/batch_newton.hpp, sdfs_batch_newton_dev, ``solve_batch(...,
algorithm="newton")``): one workgroup per problem, checked per member against the oracle's operator, its J.v and its
own Newton solve (oracle/solvers.py), against the single-problem device solve on the fallback, and for independence of
a problem's bits from the batch, its place in it and the budget of a launch.  The oracle-side preconditions of the
bounds are tests/test_batch_newton_cpu.py.
"""
import numpy as np
import pytest

from batch_family import member, package_model
from batch_newton_family import CASES, INNER_RTOL, TOL, first_step_residual, oracle_newton, oracle_ops

pytestmark = pytest.mark.gpu

OPTS = dict(algorithm="newton", tol=TOL, inner_rtol=INNER_RTOL, inner_atol=0.0)


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


def family(S, kind, count, start=0):
    return [package_model(S, kind, member(kind, b)) for b in range(start, start + count)]


_solved = {}


def solved(S, kind, shapes, members):
    """The batch of the first `members` family members solved by Newton from 800 (once per module)."""
    key = (kind, shapes, members)
    if key not in _solved:
        _solved[key] = S.solve_batch(family(S, kind, members), shapes, **OPTS)
    return _solved[key]


def same_bits(a, b, ia, ib):
    return (np.array_equal(a.w[ia], b.w[ib]) and a.n_iter[ia] == b.n_iter[ib] and a.n_apply[ia] == b.n_apply[ib]
            and a.error[ia] == b.error[ib] and a.status[ia] == b.status[ib])


# ---------------------------------------------------------------- 1: the fixed point
@pytest.mark.parametrize("kind,shapes,members", CASES)
def test_newton_fixed_point(S, kind, shapes, members):
    res = solved(S, kind, shapes, members)
    assert res.plan == "batch"
    assert np.all(res.status == 0), res.status
    for b in range(members):
        T, _ = oracle_ops(kind, shapes, member(kind, b))
        wo, no, errs, nmv, wstar = oracle_newton(kind, shapes, b)
        dist = np.max(np.abs(res.w[b] - wstar))
        resid = np.max(np.abs(T(res.w[b]) - res.w[b]))
        print(f"{kind} {shapes} member {b}: {res.n_iter[b]} steps (oracle {no}), {res.n_apply[b]} applications (oracle "
              f"{nmv} + {no}), error {res.error[b]:.3e}, max|w - w*| {dist:.3e}, residual {resid:.3e}")
        assert dist <= 1e-8, (b, dist)
        assert resid <= 1e-9, (b, resid)
        assert abs(int(res.n_iter[b]) - no) <= 1, (b, res.n_iter[b], no)
        assert res.n_apply[b] <= 2 * (nmv + no), (b, res.n_apply[b], nmv, no)
        assert res.n_apply[b] > res.n_iter[b]


# ---------------------------------------------------------------- 2: one inner solve, tightly
@pytest.mark.parametrize("kind,shapes,members", CASES)
def test_newton_one_inner_solve(S, kind, shapes, members):
    res = S.solve_batch(family(S, kind, members), shapes, algorithm="newton", tol=TOL, max_iter=1, inner_rtol=1e-10,
                        inner_atol=0.0)
    assert res.plan == "batch"
    assert np.all(res.n_iter == 1) and np.all(res.status == 1), (res.n_iter, res.status)
    for b in range(members):
        rel = first_step_residual(kind, shapes, b, 800.0 - res.w[b])
        print(f"{kind} {shapes} member {b}: {res.n_apply[b]} applications, true relative residual of the step {rel:.3e}")
        assert rel <= 1e-9, (b, rel)


# ---------------------------------------------------------------- 3: max_iter is exact
@pytest.mark.parametrize("kind,shapes,members", [("ssy", (5,) * 4, 12), ("gcy", (3,) * 6, 12), ("ssy", (10,) * 4, 3)])
def test_newton_k_steps(S, kind, shapes, members):
    models = family(S, kind, members)
    prev = np.full((members,) + shapes, 800.0)
    res0 = S.solve_batch(models, shapes, max_iter=0, **OPTS)
    assert np.all(res0.status == 1) and np.all(res0.n_iter == 0) and np.all(res0.n_apply == 0)
    assert np.array_equal(res0.w, prev)
    for k in (1, 2, 3):
        res = S.solve_batch(models, shapes, max_iter=k, **OPTS)
        assert np.all(res.n_iter == k) and np.all(res.status == 1), (k, res.n_iter, res.status)
        for b in range(members):
            step = np.max(np.abs(res.w[b] - prev[b]))
            print(f"{kind} {shapes} member {b} step {k}: error {res.error[b]:.6e}, max|w_k - w_k-1| {step:.6e}")
            assert abs(res.error[b] - step) <= 1e-10, (k, b, res.error[b], step)
        prev = res.w


# ---------------------------------------------------------------- 4: the reference's defaults
@pytest.mark.parametrize("kind,shapes,members", [("ssy", (5,) * 4, 12), ("gcy", (3,) * 6, 12), ("ssy", (10,) * 4, 3)])
def test_newton_reference_defaults(S, kind, shapes, members):
    res = S.solve_batch(family(S, kind, members), shapes, algorithm="newton")
    assert res.plan == "batch"
    assert np.all(res.status == 0), res.status
    for b in range(members):
        T, _ = oracle_ops(kind, shapes, member(kind, b))
        wo, no, errs, nmv, _ = oracle_newton(kind, shapes, b, 1e-7, 1e-5, 1e-4, polish=False)
        resid = np.max(np.abs(T(res.w[b]) - res.w[b]))
        print(f"{kind} {shapes} member {b}: {res.n_iter[b]} steps (oracle {no}), residual {resid:.3e}, error {res.error[b]:.3e}")
        assert no in (5, 6), (b, no)
        assert resid <= 1e-4, (b, resid)
        assert abs(int(res.n_iter[b]) - no) <= 1, (b, res.n_iter[b], no)


# ---------------------------------------------------------------- 5: a problem's bits are its own
def test_newton_member_independent_of_batch_and_budget(S):
    shapes = (5,) * 4
    ref = solved(S, "ssy", shapes, 12)
    m5 = package_model(S, "ssy", member("ssy", 5))
    for check_every in (8, 64, 1000, 0):
        alone = S.solve_batch([m5], shapes, check_every=check_every, **OPTS)
        assert same_bits(alone, ref, 0, 5), check_every
        three = S.solve_batch([m5] + family(S, "ssy", 2, start=1), shapes, check_every=check_every, **OPTS)
        assert same_bits(three, ref, 0, 5), check_every
        twelve = S.solve_batch(family(S, "ssy", 12), shapes, check_every=check_every, **OPTS)
        for b in range(12):
            assert same_bits(twelve, ref, b, b), (check_every, b)
        big = S.solve_batch(family(S, "ssy", 300), shapes, check_every=check_every, **OPTS)
        assert np.all(big.status == 0)
        for b in range(12):
            assert same_bits(big, ref, b, b), (check_every, b)


def test_newton_member_independent_where_the_vectors_leave_the_registers(S):
    shapes = (10,) * 4
    ref = S.solve_batch(family(S, "ssy", 12), shapes, **OPTS)
    assert np.all(ref.status == 0)
    m1 = package_model(S, "ssy", member("ssy", 1))
    op = S.BatchOperator.from_models([m1], shapes)
    assert "in global memory" in op.describe_plan()
    op.close()
    # an inner solve takes 60 to 80 J.v here: budgets of 8 and 64 applications end inside one
    for check_every in (8, 64, 1000, 0):
        alone = S.solve_batch([m1], shapes, check_every=check_every, **OPTS)
        assert same_bits(alone, ref, 0, 1), check_every
        three = S.solve_batch([m1] + family(S, "ssy", 2, start=2), shapes, check_every=check_every, **OPTS)
        assert same_bits(three, ref, 0, 1), check_every
        twelve = S.solve_batch(family(S, "ssy", 12), shapes, check_every=check_every, **OPTS)
        for b in range(12):
            assert same_bits(twelve, ref, b, b), (check_every, b)


# ---------------------------------------------------------------- 6: every problem stops on its own
def test_newton_per_problem_stopping(S):
    shapes = (5,) * 4
    ref = solved(S, "ssy", shapes, 12)
    models = [package_model(S, "ssy", member("ssy", 5)), package_model(S, "ssy", member("ssy", 0)), S.SSY(β=1.05)]
    res = S.solve_batch(models, shapes, max_iter=50, **OPTS)
    assert list(res.status) == [0, 0, 2], res.status
    assert same_bits(res, ref, 0, 5) and same_bits(res, ref, 1, 0)
    print(f"beta = 1.05: error {res.error[2]}, {res.n_iter[2]} steps, min w {np.nanmin(res.w[2])}")
    assert (not np.isfinite(res.error[2])) or res.error[2] <= 0.0
    assert res.n_iter[2] <= 50


# ---------------------------------------------------------------- 7: warm starts, honoured per member
def test_newton_warm_start(S):
    kind, shapes, B = "ssy", (5,) * 4, 12
    ref = solved(S, kind, shapes, B)
    models = family(S, kind, B)
    res = S.solve_batch(models, shapes, w0=ref.w + 1e-3, **OPTS)
    assert np.all(res.status == 0)
    assert np.all(res.n_iter <= 3) and np.all(res.n_iter < ref.n_iter), (res.n_iter, ref.n_iter)
    pair = (5, 11)
    w0 = ref.w + 1e-3
    w0[list(pair)] = w0[list(pair[::-1])]
    res = S.solve_batch(models, shapes, w0=w0, **OPTS)
    assert np.all(res.status == 0)
    assert np.max(np.abs(ref.w[pair[0]] - ref.w[pair[1]])) > 10.0
    for b in pair:
        wstar = oracle_newton(kind, shapes, b)[4]
        d = np.max(np.abs(res.w[b] - wstar))
        print(f"member {b} from the other's w*: {res.n_iter[b]} steps, max|w - w*| {d:.3e}")
        assert d <= 1e-8, (b, d)


# ---------------------------------------------------------------- 8: fallback and device forms
def test_newton_fallback_loop(S):
    shapes = (15,) * 4
    models = family(S, "ssy", 2)
    res = S.solve_batch(models, shapes, **OPTS)
    assert res.plan == "loop"
    for b, m in enumerate(models):
        T = S.ssy_operator(shapes, m.params, S.discretize_ssy(m, shapes))
        x, n, info = T.solve(np.full(shapes, 800.0), "newton", tol=TOL, inner_rtol=INNER_RTOL, inner_atol=0.0)
        T.close()
        assert np.array_equal(res.w[b], x) and res.n_iter[b] == n and res.error[b] == info["final_err"]
        assert res.n_apply[b] == info["n_apply"] and res.status[b] == 0


def test_newton_operator_device_forms(S):
    import torch
    shapes, B = (5,) * 4, 4
    ref = solved(S, "ssy", shapes, 12)
    op = S.BatchOperator.from_models(family(S, "ssy", B), shapes)
    assert "newton" in op.describe_plan() and "in registers" in op.describe_plan()
    w = torch.full((B,) + shapes, 800.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    n_iter, err, status, n_apply = op.solve_dev(w.data_ptr(), **OPTS)
    for b in range(B):
        assert np.array_equal(w[b].cpu().numpy(), ref.w[b]) and n_iter[b] == ref.n_iter[b] and err[b] == ref.error[b]
        assert n_apply[b] == ref.n_apply[b] and status[b] == 0
    wh, n2, e2, s2, a2 = op.solve(np.full((B,) + shapes, 800.0), **OPTS)
    assert np.array_equal(wh, w.cpu().numpy()) and np.array_equal(n2, n_iter) and np.array_equal(a2, n_apply)
    with pytest.raises(S.SdfsError):
        op.solve(np.full((B,) + shapes, 800.0), krylov_f32=1, **OPTS)
    with pytest.raises(TypeError):
        op.solve(np.full((B,) + shapes, 800.0), no_such_option=1, **OPTS)
    op.close()
    m = S.SSY()
    arr = [np.asarray(a, dtype=np.float64) for a in S.discretize_ssy(m, shapes)]
    q = np.random.default_rng(3).random(arr[7].shape) + 0.05
    arr[7] = q / q.sum(axis=-1, keepdims=True)                           # a conditional z tensor
    with pytest.raises(S.SdfsError):
        S.BatchOperator("ssy", shapes, np.array([m.params]), [a[None] for a in arr])


# ---------------------------------------------------------------- 9: the SA path is untouched
def test_successive_approximation_path_untouched(S):
    shapes = (5,) * 4
    models = family(S, "ssy", 4)
    a = S.solve_batch(models, shapes, tol=1e-6)
    b = S.solve_batch(models, shapes, tol=1e-6, algorithm="successive_approx")
    assert a.plan == b.plan == "batch"
    assert np.array_equal(a.w, b.w) and np.array_equal(a.n_iter, b.n_iter) and np.array_equal(a.error, b.error)
    assert np.array_equal(a.status, b.status)
    assert a.n_apply is None and b.n_apply is None

"""
GPU tests of the batched successive approximation (csrc/batch_kernels.hpp, sdfs_batch_*, ``solve_batch``): one
workgroup per problem, checked per member against the oracle's operator and the oracle's own solve, against the
single-problem device solve, against the committed golden solves, and for independence of a problem's bits from the
batch, its place in it and the chunk length.  Tolerances are those of tests/test_hip_small_plan.py.
"""
import numpy as np
import pytest

from batch_family import COUNT_CASES, member, oracle_T, oracle_apply, oracle_solve, package_model
from conftest import load_golden

pytestmark = pytest.mark.gpu

APPLY_RTOL = 1e-12
TOL = 1e-6


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


def family(S, kind, count, start=0):
    return [package_model(S, kind, member(kind, b)) for b in range(start, start + count)]


_solved = {}


def solved(S, kind, shapes, members):
    """The batch of the first `members` family members solved to TOL from 800 (once per module)."""
    key = (kind, shapes, members)
    if key not in _solved:
        _solved[key] = S.solve_batch(family(S, kind, members), shapes, tol=TOL)
    return _solved[key]


# ---------------------------------------------------------------- 4: one application per problem
@pytest.mark.parametrize("kind,shapes", [
    ("ssy", (5,) * 4), ("ssy", (10,) * 4), ("ssy", (11,) * 4), ("ssy", (7, 13, 11, 9)), ("ssy", (2, 2, 2, 2)),
    ("gcy", (3,) * 6), ("gcy", (5,) * 6), ("gcy", (3, 4, 5, 2, 3, 4)), ("gcy", (2,) * 6)])
def test_batch_apply_T_vs_oracle(S, kind, shapes):
    B = 12
    op = S.BatchOperator.from_models(family(S, kind, B), shapes)
    assert "batch plan" in op.describe_plan()
    w = 400 + 500 * np.random.default_rng(0).random((B,) + shapes)
    keep = w.copy()
    got, resid = op(w, return_resid=True)
    for b in range(B):
        want = oracle_T(kind, shapes, member(kind, b))(w[b])
        np.testing.assert_allclose(got[b], want, rtol=APPLY_RTOL, err_msg=f"member {b}")
        r = np.max(np.abs(want - w[b]))
        assert abs(resid[b] - r) <= 1e-12 * r + 1e-9, (b, resid[b], r)
    np.testing.assert_array_equal(w, keep)                               # inputs never mutated
    op.close()


# ---------------------------------------------------------------- 5: max_iter is exact
@pytest.mark.parametrize("k", [1, 2, 3, 7])
@pytest.mark.parametrize("kind,shapes,B", [("ssy", (5,) * 4, 12), ("gcy", (3,) * 6, 12), ("ssy", (7, 13, 11, 9), 3)])
def test_batch_k_iterations(S, kind, shapes, B, k):
    res = S.solve_batch(family(S, kind, B), shapes, tol=0.0, max_iter=k)
    assert res.plan == "batch"
    assert np.all(res.n_iter == k) and np.all(res.status == 1)
    for b in range(B):
        want = oracle_apply(kind, shapes, member(kind, b), np.full(shapes, 800.0), k)
        np.testing.assert_allclose(res.w[b], want, rtol=1e-11, err_msg=f"member {b}")


# ---------------------------------------------------------------- 6: counts, iterates and errors of whole solves
@pytest.mark.parametrize("kind,shapes,members", COUNT_CASES)
def test_batch_solve_counts_match_oracle_and_single_solve(S, kind, shapes, members):
    res = solved(S, kind, shapes, members)
    assert res.plan == "batch"
    disc = S.discretize_ssy if kind == "ssy" else S.discretize_gcy
    for b, m in enumerate(family(S, kind, members)):
        wo, no, errs = oracle_solve(kind, shapes, member(kind, b), TOL)
        print(f"{kind} {shapes} member {b}: batch {res.n_iter[b]} oracle {no} error {res.error[b]:.6e} oracle {errs[-1]:.6e} "
              f"max|w - w_oracle| {np.max(np.abs(res.w[b] - wo)):.3e}")
        assert res.n_iter[b] == no, (b, res.n_iter[b], no)
        assert np.max(np.abs(res.w[b] - wo)) <= 1e-9
        np.testing.assert_allclose(res.error[b], errs[-1], rtol=1e-9, atol=1e-11)
        assert res.status[b] == 0
        T = S.KoopmansOperator(kind, shapes, m.params, disc(m, shapes))
        xs, ns, _ = T.solve(np.full(shapes, 800.0), "successive_approx", tol=TOL)
        T.close()
        assert ns == res.n_iter[b], (b, ns, res.n_iter[b])
        np.testing.assert_allclose(xs, res.w[b], rtol=0, atol=1e-9)


# ---------------------------------------------------------------- 6b: pinned to the reference's recorded solves
def test_batch_reproduces_golden_solves(S):
    shapes = (3, 3, 3, 3)
    g = load_golden("sa_ssy_3x3x3x3.npz")
    res = S.solve_batch([S.SSY()] + family(S, "ssy", 2, start=1), shapes, tol=1e-8)
    assert res.plan == "batch" and res.status[0] == 0
    assert res.n_iter[0] == int(g["n_1e8"]) == 12253
    np.testing.assert_allclose(res.w[0], g["w_1e8"], rtol=0, atol=1e-9)
    shapes = (3,) * 6
    g = load_golden("sa_gcy_3x3x3x3x3x3.npz")
    res = S.solve_batch(family(S, "gcy", 2, start=1) + [S.GCY()], shapes)         # the reference's default tol 1e-7
    assert res.plan == "batch" and res.status[2] == 0
    assert res.n_iter[2] == int(g["n_1e7"]) == 7520
    np.testing.assert_allclose(res.w[2], g["w_1e7"], rtol=0, atol=1e-9)


# ---------------------------------------------------------------- 7: a problem's bits are its own
def same_bits(a, b, ia, ib):
    return (np.array_equal(a.w[ia], b.w[ib]) and a.n_iter[ia] == b.n_iter[ib] and a.error[ia] == b.error[ib]
            and a.status[ia] == b.status[ib])


def test_batch_member_independent_of_batch_and_chunk(S):
    shapes = (5,) * 4
    ref = solved(S, "ssy", shapes, 12)
    m5 = package_model(S, "ssy", member("ssy", 5))
    for check_every in (64, 1000, 0):
        alone = S.solve_batch([m5], shapes, tol=TOL, check_every=check_every)
        assert same_bits(alone, ref, 0, 5), check_every
        three = S.solve_batch([m5] + family(S, "ssy", 2, start=1), shapes, tol=TOL, check_every=check_every)
        assert same_bits(three, ref, 0, 5), check_every
        twelve = S.solve_batch(family(S, "ssy", 12), shapes, tol=TOL, check_every=check_every)
        for b in range(12):
            assert same_bits(twelve, ref, b, b), (check_every, b)


def test_batch_larger_than_the_chip(S):
    shapes = (5,) * 4
    ref = solved(S, "ssy", shapes, 12)
    big = S.solve_batch(family(S, "ssy", 300), shapes, tol=TOL)
    assert np.all(big.status == 0)
    for b in range(12):
        assert same_bits(big, ref, b, b), b


# ---------------------------------------------------------------- 8: every problem stops on its own
def test_batch_per_problem_stopping(S):
    shapes = (5,) * 4
    ref = solved(S, "ssy", shapes, 12)
    models = [package_model(S, "ssy", member("ssy", 5)), package_model(S, "ssy", member("ssy", 0)), S.SSY(β=1.05)]
    assert oracle_solve("ssy", shapes, member("ssy", 5), TOL)[1] == 5562
    assert oracle_solve("ssy", shapes, member("ssy", 0), TOL)[1] == 9317
    res = S.solve_batch(models, shapes, tol=TOL, max_iter=7000)
    assert list(res.status) == [0, 1, 2], res.status
    assert same_bits(res, ref, 0, 5)
    assert res.n_iter[1] == 7000
    want = oracle_apply("ssy", shapes, member("ssy", 0), np.full(shapes, 800.0), 7000)
    np.testing.assert_allclose(res.w[1], want, rtol=0, atol=1e-9)
    assert not np.isfinite(res.error[2]) and res.n_iter[2] <= 7000
    res = S.solve_batch(models, shapes, tol=TOL, max_iter=700)
    assert list(res.status) == [1, 1, 1] and list(res.n_iter) == [700, 700, 700]


# ---------------------------------------------------------------- 9: warm starts, honoured per member
def test_batch_warm_start(S):
    kind, shapes, B = "ssy", (5,) * 4, 12
    ref = solved(S, kind, shapes, B)
    models = family(S, kind, B)
    res = S.solve_batch(models, shapes, w0=ref.w + 1e-3, tol=TOL)
    assert np.all(res.status == 0)
    assert np.all(res.n_iter < ref.n_iter), (res.n_iter, ref.n_iter)
    for b in range(B):
        r = np.max(np.abs(oracle_T(kind, shapes, member(kind, b))(res.w[b]) - res.w[b]))
        assert r <= TOL, (b, r)
    # Two members start from each other's solution and still return their own fixed points.  Which two: a start from
    # the other member's w* approaches from the other side for one of them, and an iterate stopped at a step <= tol lies
    # within tol rho / (1 - rho) of w* (rho: the member's contraction rate, the ratio of the oracle's last two errors),
    # so two stopped iterates of one member can differ by twice that.  Members 5 and 11 are the family's fastest
    # contractions (3.9e-4 and 4.1e-4 one-sided on the oracle): atol 1e-3 holds for them on the oracle itself, while for
    # members 3 and 4 the oracle alone gives 1.09e-3 between its two stopped iterates.
    pair = (5, 11)
    for b in pair:
        errs = oracle_solve(kind, shapes, member(kind, b), TOL)[2]
        rho = errs[-1] / errs[-2]
        assert 2 * TOL * rho / (1 - rho) < 1e-3, (b, rho)
    w0 = ref.w + 1e-3
    w0[list(pair)] = w0[list(pair[::-1])]
    res = S.solve_batch(models, shapes, w0=w0, tol=TOL)
    assert np.all(res.status == 0)
    assert np.max(np.abs(ref.w[pair[0]] - ref.w[pair[1]])) > 10.0
    for b in pair:
        print(f"member {b} from the other's w*: {res.n_iter[b]} iterations, max|w - w_ref| {np.max(np.abs(res.w[b] - ref.w[b])):.3e}")
        np.testing.assert_allclose(res.w[b], ref.w[b], rtol=0, atol=1e-3)
    one = S.solve_batch(models, shapes, w0=np.full(shapes, 800.0), tol=TOL)     # one grid for all = the default start
    for b in range(B):
        assert same_bits(one, ref, b, b)


# ---------------------------------------------------------------- 10: shapes that do not fit one CU
def test_batch_fallback_loop(S):
    shapes = (15,) * 4
    models = family(S, "ssy", 3)
    res = S.solve_batch(models, shapes, tol=TOL)
    assert res.plan == "loop"
    for b, m in enumerate(models):
        T = S.ssy_operator(shapes, m.params, S.discretize_ssy(m, shapes))
        x, n, info = T.solve(np.full(shapes, 800.0), "successive_approx", tol=TOL)
        T.close()
        assert np.array_equal(res.w[b], x) and res.n_iter[b] == n and res.error[b] == info["final_err"]
        assert res.status[b] == 0
    assert solved(S, "ssy", (10,) * 4, 3).plan == "batch"


def test_batch_operator_device_forms(S):
    """``apply_dev`` / ``solve_dev`` on caller-owned device memory, conditional tensors refused."""
    import torch
    shapes, B = (5,) * 4, 4
    op = S.BatchOperator.from_models(family(S, "ssy", B), shapes)
    w = torch.full((B,) + shapes, 800.0, dtype=torch.float64, device="cuda")
    out = torch.empty_like(w)
    torch.cuda.synchronize()
    op.apply_dev(w.data_ptr(), out.data_ptr())
    op.synchronize()
    for b in range(B):
        np.testing.assert_allclose(out[b].cpu().numpy(), oracle_T("ssy", shapes, member("ssy", b))(np.full(shapes, 800.0)),
                                   rtol=APPLY_RTOL)
    n_iter, err, status = op.solve_dev(w.data_ptr(), tol=TOL)
    ref = solved(S, "ssy", shapes, 12)
    for b in range(B):
        assert np.array_equal(w[b].cpu().numpy(), ref.w[b]) and n_iter[b] == ref.n_iter[b] and err[b] == ref.error[b]
    op.close()
    m = S.SSY()
    arr = [np.asarray(a, dtype=np.float64) for a in S.discretize_ssy(m, shapes)]
    q = np.random.default_rng(3).random(arr[7].shape) + 0.05
    arr[7] = q / q.sum(axis=-1, keepdims=True)                           # a conditional z tensor
    with pytest.raises(S.SdfsError):
        S.BatchOperator("ssy", shapes, np.array([m.params]), [a[None] for a in arr])

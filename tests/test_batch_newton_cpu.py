"""
CPU tests of the batched Newton-Krylov solve: the algorithm argument of ``solve_batch`` (checked before any device
work), the binding of ``sdfs_batch_newton_dev``, and the preconditions of tests/test_hip_batch_newton.py on the oracle
alone.
"""
import numpy as np
import pytest

from batch_family import member
from batch_newton_family import CASES, INNER_RTOL, TOL, first_step_residual, oracle_newton, oracle_ops
from oracle import solvers as osolvers


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


@pytest.mark.parametrize("name", ["bogus", "anderson"])
def test_solve_batch_refuses_other_algorithms(S, name):
    with pytest.raises(ValueError) as e:
        S.solve_batch([S.SSY()], (5, 5, 5, 5), algorithm=name)
    assert "successive_approx" in str(e.value) and "newton" in str(e.value)


def test_newton_symbol_is_bound(S):
    from sdfs_via_autodiff_amd import _lib
    assert "sdfs_batch_newton_dev" in _lib.SYMBOLS
    fn = _lib.lib.sdfs_batch_newton_dev
    assert fn.argtypes is not None and len(fn.argtypes) == 7


def test_batch_result_keeps_its_fields(S):
    assert S.BatchResult._fields == ("w", "n_iter", "error", "status", "plan")
    r = S.BatchResult(1, 2, 3, 4, "batch")
    assert tuple(r) == (1, 2, 3, 4, "batch") and r.n_apply is None
    assert S.BatchResult(1, 2, 3, 4, "batch", 5).n_apply == 5


@pytest.mark.parametrize("kind,shapes,members", CASES)
def test_newton_preconditions_on_the_oracle(kind, shapes, members):
    """What the GPU tests lean on: the oracle's Newton solve (tol 1e-7, inner rtol 1e-5, atol 0) ends at a residual
    <= 1e-12 in 6 or 7 steps, and its BiCGSTAB at rtol 1e-10 leaves a true relative residual <= 1e-10 on the first step."""
    for b in range(members):
        T, jvp = oracle_ops(kind, shapes, member(kind, b))
        w, n, errors, nmv, _ = oracle_newton(kind, shapes, b, TOL, INNER_RTOL, 0.0, polish=False)
        resid = np.max(np.abs(T(w) - w))
        w0 = np.full(shapes, 800.0)
        g = T(w0) - w0
        step = osolvers.bicgstab(lambda v: jvp(w0, v) - v, g, tol=1e-10, atol=0.0)
        rel = first_step_residual(kind, shapes, b, step)
        print(f"{kind} {shapes} member {b}: {n} steps, {nmv} J.v, residual {resid:.2e}, first step rel. residual {rel:.3e}")
        assert resid <= 1e-12, (b, resid)
        assert n in (6, 7), (b, n)
        assert rel <= 1.0e-10, (b, rel)

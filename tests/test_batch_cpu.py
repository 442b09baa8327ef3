"""
CPU tests of the batched solve: argument checks of ``solve_batch`` (before any device work), the host-only LDS budget
``sdfs_batch_lds_bytes``, and the precondition of the GPU count test on the oracle alone.
"""
import ctypes as C

import numpy as np
import pytest

from batch_family import COUNT_CASES, member, oracle_solve


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


def test_solve_batch_argument_checks(S):
    shapes = (5, 5, 5, 5)
    with pytest.raises(TypeError):
        S.solve_batch([S.SSY(), S.GCY()], shapes)
    with pytest.raises(TypeError):
        S.solve_batch([S.SSY(), "ssy"], shapes)
    with pytest.raises(ValueError):
        S.solve_batch([], shapes)
    with pytest.raises(ValueError):
        S.solve_batch([S.SSY(), S.SSY()], shapes, w0=np.full((3, 5, 5, 5, 5), 800.0))
    with pytest.raises(ValueError):
        S.solve_batch([S.SSY(), S.SSY()], shapes, w0=np.full((5, 5, 5), 800.0))
    with pytest.raises(ValueError):
        S.solve_batch([S.GCY()], shapes)                      # a 4-D shape for a 6-D model


FITS = [("ssy", (5,) * 4), ("ssy", (10,) * 4), ("ssy", (11,) * 4), ("ssy", (7, 13, 11, 9)),
        ("gcy", (3,) * 6), ("gcy", (4,) * 6), ("gcy", (5,) * 6), ("gcy", (3, 4, 5, 2, 3, 4))]
TOO_LARGE = [("ssy", (15,) * 4), ("ssy", (16,) * 4), ("gcy", (6,) * 6)]


def _lds_bytes(S, kind, shapes):
    from sdfs_via_autodiff_amd import _lib
    model = _lib.SDFS_MODEL_SSY if kind == "ssy" else _lib.SDFS_MODEL_GCY
    return _lib.lib.sdfs_batch_lds_bytes(model, len(shapes), (C.c_int64 * len(shapes))(*shapes))


@pytest.mark.parametrize("kind,shapes", FITS)
def test_batch_lds_bytes_fits(S, kind, shapes):
    n = _lds_bytes(S, kind, shapes)
    assert 8 * int(np.prod(shapes)) <= n <= 163840
    assert S.batch_lds_bytes(kind, shapes) == n


@pytest.mark.parametrize("kind,shapes", TOO_LARGE + [("ssy", (33, 2, 2, 2))])
def test_batch_lds_bytes_unsupported(S, kind, shapes):
    from sdfs_via_autodiff_amd import _lib
    assert _lds_bytes(S, kind, shapes) == _lib.SDFS_ERR_UNSUPPORTED
    assert S.batch_lds_bytes(kind, shapes) is None


def test_batch_lds_bytes_bad_arguments(S):
    from sdfs_via_autodiff_amd import _lib
    assert _lds_bytes(S, "ssy", (5,) * 6) == _lib.SDFS_ERR_ARG
    assert _lds_bytes(S, "gcy", (5,) * 4) == _lib.SDFS_ERR_ARG
    assert _lds_bytes(S, "ssy", (5, 1, 5, 5)) == _lib.SDFS_ERR_ARG


@pytest.mark.parametrize("kind,shapes,members", COUNT_CASES)
def test_count_test_precondition_on_the_oracle(kind, shapes, members):
    """No entry of the oracle's error trace lies within 1e-5 tol of tol, for any member the GPU count test uses: a
    device trace that agrees with the oracle's to atol 1e-11 (at tol 1e-6) then stops at the same iteration."""
    tol = 1e-6
    for b in range(members):
        w, n, errors = oracle_solve(kind, shapes, member(kind, b), tol)
        assert n == len(errors) and errors[-1] <= tol < errors[-2]
        gap = np.min(np.abs(errors - tol))
        assert gap > 1e-5 * tol, (kind, shapes, b, n, gap)

"""
CPU tests of the batch gradient's host half (no GPU): ``adjoint_moments_to_gradient`` on moments restated in numpy
(tests/batch_adjoint_oracle.py) against <lambda, complex-step dT/dp> with a dense lambda, for every parameter, and the
refusals of ``gradient_batch`` that come before any device call.
"""
import numpy as np
import pytest

import batch_adjoint_oracle as bao
from batch_family import member, package_model

CASES = [("ssy", (3, 4, 3, 5)), ("gcy", (3, 2, 3, 2, 2, 3))]


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


_cache = {}


def setting(S, kind, shapes):
    """Member 1 at its dense fixed point: model, oracle inputs, w*, g, the dense lambda, its moments and the truth."""
    key = (kind, shapes)
    if key not in _cache:
        over = member(kind, 1)
        model = package_model(S, kind, over)
        params, arrays = bao.oracle_inputs(kind, shapes, over)
        w = bao.dense_fixed_point(kind, shapes, params, arrays)
        assert np.max(np.abs(bao.T(kind, shapes, params, arrays, w) - w)) <= 1e-9
        g = 0.5 + np.random.default_rng(11).random(shapes)
        lam = bao.dense_lambda(kind, shapes, params, arrays, w, g)
        block, _ = bao.moments(kind, shapes, params, arrays, w, lam)
        truth = bao.truth_gradient(S, kind, shapes, model, params, arrays, w, lam)
        _cache[key] = (model, block, truth)
    return _cache[key]


@pytest.mark.parametrize("kind,shapes", CASES)
def test_moments_to_gradient_equals_lambda_dot_complex_step_tangent(S, kind, shapes):
    """Bound 1e-8 |want|, that of test_adjoint_gradient_equals_forward_sensitivities; the worst gaps are on γ and ψ,
    whose terms cancel."""
    model, block, truth = setting(S, kind, shapes)
    got = S.adjoint_moments_to_gradient(model, shapes, block, persistence=True)
    assert len(got) == (13 if kind == "ssy" else 18) and set(got) == set(truth)
    for nm, want in truth.items():
        gap = abs(got[nm] - want) / abs(want)
        print(f"{kind} {shapes} {nm}: {got[nm]!r} vs {want!r}, relative gap {gap:.2e}")
        assert abs(got[nm] - want) <= 1e-8 * abs(want), (nm, got[nm], want)


@pytest.mark.parametrize("kind,shapes", CASES)
def test_without_persistence_the_other_values_are_unchanged(S, kind, shapes):
    from sdfs_via_autodiff_amd import sensitivity as sens
    model, block, _ = setting(S, kind, shapes)
    full = S.adjoint_moments_to_gradient(model, shapes, block, persistence=True)
    part = S.adjoint_moments_to_gradient(model, shapes, block, persistence=False)
    pers = sens.SSY_PERSISTENCE if kind == "ssy" else sens.GCY_PERSISTENCE
    supported = sens.SSY_SUPPORTED if kind == "ssy" else sens.GCY_SUPPORTED
    assert tuple(part) == tuple(supported) and len(part) == (9 if kind == "ssy" else 12)
    assert not set(part) & set(pers)
    for nm in part:
        assert part[nm] == full[nm], nm


def test_refusals_come_before_any_device_call(S):
    shapes = (3, 4, 3, 5)
    ssy = [package_model(S, "ssy", member("ssy", b)) for b in range(2)]
    w = np.full((2,) + shapes, 800.0)
    g = np.ones(shapes)
    model, block, _ = setting(S, "ssy", shapes)
    with pytest.raises(ValueError, match="Rouwenhorst"):
        S.adjoint_moments_to_gradient(model, shapes, block, method="tauchen")
    with pytest.raises(ValueError, match="Rouwenhorst"):
        S.gradient_batch(ssy, shapes, w, g, method="tauchen")
    with pytest.raises(TypeError, match="all SSY or all GCY"):
        S.gradient_batch([ssy[0], S.GCY()], shapes, w, g)
    with pytest.raises(ValueError, match="w_star has shape"):
        S.gradient_batch(ssy, shapes, w[0], g)
    with pytest.raises(ValueError, match="w_star has shape"):
        S.gradient_batch(ssy, shapes, np.full((3,) + shapes, 800.0), g)
    with pytest.raises(ValueError, match="g has shape"):
        S.gradient_batch(ssy, shapes, w, np.ones((3,) + shapes))
    with pytest.raises(ValueError, match="g has shape"):
        S.gradient_batch(ssy, shapes, w, np.ones(shapes[:-1]))
    with pytest.raises(ValueError, match="moments has"):
        S.adjoint_moments_to_gradient(model, shapes, block[:-1])

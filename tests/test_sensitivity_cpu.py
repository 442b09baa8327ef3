"""
CPU tests of the discretisation tangents behind the parameter sensitivities (sdfs_via_autodiff_amd/sensitivity.py):
(dparams, darrays) = d (params, discretize_*(model, shapes)) / dp, held to Richardson-extrapolated central differences
of discretize_ssy / discretize_gcy for every supported parameter; persistence parameters and Tauchen grids are refused.
"""
import numpy as np
import pytest

import sdfs_via_autodiff_amd as S
from sdfs_via_autodiff_amd import sensitivity as sens

SSY_SHAPES = (3, 4, 5, 6)
GCY_SHAPES = (4, 3, 5, 3, 4, 2)


def _model(kind, **over):
    cls, names = (S.SSY, sens.SSY_PARAMS) if kind == "ssy" else (S.GCY, sens.GCY_PARAMS)
    base = dict(zip(names, cls().params))
    base.update(over)
    return cls(**base)


def _fd(kind, shapes, name):
    """Richardson-extrapolated central differences of (params, arrays) along one parameter (step 1e-4 |p|)."""
    disc = S.discretize_ssy if kind == "ssy" else S.discretize_gcy
    names = sens.SSY_PARAMS if kind == "ssy" else sens.GCY_PARAMS
    p0 = dict(zip(names, (_model(kind)).params))[name]
    h = 1e-4 * abs(p0)

    def d(step):
        hi = disc(_model(kind, **{name: p0 + step}), shapes)
        lo = disc(_model(kind, **{name: p0 - step}), shapes)
        return [(a - b) / (2 * step) for a, b in zip(hi, lo)]
    d1, d2 = d(h), d(h / 2)
    return [(4 * b - a) / 3 for a, b in zip(d1, d2)]


@pytest.mark.parametrize("kind,shapes,name",
                         [("ssy", SSY_SHAPES, n) for n in sens.SSY_SUPPORTED] +
                         [("gcy", GCY_SHAPES, n) for n in sens.GCY_SUPPORTED])
def test_discretisation_tangent_vs_central_differences(kind, shapes, name):
    tangent = S.discretize_ssy_tangent if kind == "ssy" else S.discretize_gcy_tangent
    names = sens.SSY_PARAMS if kind == "ssy" else sens.GCY_PARAMS
    dparams, darrays = tangent(_model(kind), shapes, name)
    want_p = np.zeros(len(names)); want_p[names.index(name)] = 1.0
    np.testing.assert_array_equal(dparams, want_p)
    want = _fd(kind, shapes, name)
    arrays = (S.discretize_ssy if kind == "ssy" else S.discretize_gcy)(_model(kind), shapes)
    assert len(darrays) == len(arrays)
    scale = max(np.max(np.abs(w)) for w in want)
    assert scale > 0.0 or name in ("β", "γ", "ψ", "μ_c")
    for i, (got, w, a) in enumerate(zip(darrays, want, arrays)):
        assert got.shape == a.shape, i
        err = np.max(np.abs(got - w))
        assert err <= 1e-7 * max(np.max(np.abs(w)), 1e-300) or err <= 1e-12 * max(scale, 1.0), (name, i, err)


@pytest.mark.parametrize("name", ["ρ", "ρ_z", "ρ_c", "ρ_λ"])
def test_ssy_persistence_parameters_are_refused(name):
    with pytest.raises(ValueError, match="persistence"):
        S.discretize_ssy_tangent(S.SSY(), SSY_SHAPES, name)


@pytest.mark.parametrize("name", ["ρ_λ", "ρ", "ρ_c", "ρ_z", "ρ_ππ", "ρ_zπ"])
def test_gcy_persistence_parameters_are_refused(name):
    with pytest.raises(ValueError, match="persistence"):
        S.discretize_gcy_tangent(S.GCY(), GCY_SHAPES, name)


def test_tauchen_and_unknown_names_are_refused():
    with pytest.raises(ValueError, match="Rouwenhorst"):
        S.discretize_ssy_tangent(S.SSY(), SSY_SHAPES, "β", method="tauchen")
    with pytest.raises(ValueError, match="Rouwenhorst"):
        S.discretize_gcy_tangent(S.GCY(), GCY_SHAPES, "γ", method="tauchen")
    with pytest.raises(ValueError, match="unknown"):
        S.discretize_ssy_tangent(S.SSY(), SSY_SHAPES, "beta")


def test_sensitivities_refuse_before_device_work():
    # (checked on the host before any operator is built: runs without a GPU)
    with pytest.raises(ValueError, match="persistence"):
        S.wc_ratio_sensitivities(S.GCY(), GCY_SHAPES, np.ones(GCY_SHAPES), wrt=["β", "ρ_ππ"])
    with pytest.raises(TypeError):
        S.wc_ratio_gradient(object(), GCY_SHAPES, np.ones(GCY_SHAPES), np.ones(GCY_SHAPES))


def test_supported_parameter_sets():
    assert len(sens.SSY_SUPPORTED) == 9 and len(sens.GCY_SUPPORTED) == 12
    assert set(sens.SSY_SUPPORTED) <= set(sens.SSY_PARAMS) and set(sens.GCY_SUPPORTED) <= set(sens.GCY_PARAMS)

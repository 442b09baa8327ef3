"""
CPU tests of the persistence tangents (sdfs_via_autodiff_amd/sensitivity.py):

 (1) the generator identity  G Θ = Θ G = dΘ/dρ  of the Rouwenhorst matrix against the complex step of the oracle's
     recursion;
 (2) (dparams, darrays, dgen) of every persistence parameter against Richardson-extrapolated central differences of
     discretize_ssy / discretize_gcy (the scheme, shapes and bounds of test_sensitivity_cpu.py), the transition slices
     against G Q;
 (3) the stencil formula the library implements, restated in numpy (tests/persistence_oracle.py), against the complex
     step of the oracle's T along the true direction, dQ included;
 (4) the refusals.
"""
import numpy as np
import pytest

import sdfs_via_autodiff_amd as S
from sdfs_via_autodiff_amd import sensitivity as sens
from oracle.rouwenhorst import rouwenhorst_matrix

import persistence_oracle as po

SSY_SHAPES = (3, 4, 5, 6)
GCY_SHAPES = (4, 3, 5, 3, 4, 2)
SSY_AXIS = {"ρ_λ": 0, "ρ_c": 1, "ρ_z": 2, "ρ": 3}
GCY_AXIS = {"ρ": 0, "ρ_ππ": 1, "ρ_z": 2, "ρ_c": 3, "ρ_zπ": 4, "ρ_λ": 5}


def _model(kind, **over):
    cls, names = (S.SSY, sens.SSY_PARAMS) if kind == "ssy" else (S.GCY, sens.GCY_PARAMS)
    base = dict(zip(names, cls().params))
    base.update(over)
    return cls(**base)


def _tangent(kind):
    return S.discretize_ssy_persistence_tangent if kind == "ssy" else S.discretize_gcy_persistence_tangent


def _disc(kind):
    return S.discretize_ssy if kind == "ssy" else S.discretize_gcy


def _fd(kind, shapes, name):
    """Richardson-extrapolated central differences of the arrays along one parameter (step 1e-4 |p|)."""
    names = sens.SSY_PARAMS if kind == "ssy" else sens.GCY_PARAMS
    p0 = dict(zip(names, (_model(kind)).params))[name]
    h = 1e-4 * abs(p0)

    def d(step):
        hi = _disc(kind)(_model(kind, **{name: p0 + step}), shapes)
        lo = _disc(kind)(_model(kind, **{name: p0 - step}), shapes)
        return [(a - b) / (2 * step) for a, b in zip(hi, lo)]
    d1, d2 = d(h), d(h / 2)
    return [(4 * b - a) / 3 for a, b in zip(d1, d2)]


PERSISTENCE_CASES = ([("ssy", n) for n in ("ρ", "ρ_z", "ρ_c", "ρ_λ")] +
                     [("gcy", n) for n in ("ρ_λ", "ρ", "ρ_c", "ρ_z", "ρ_ππ", "ρ_zπ")])


# -- (1) generator identity ---------------------------------------------------------------------------------------------
def test_complex_restatement_is_the_oracle_matrix():
    for n in (2, 3, 5, 16, 32):
        for rho in (-0.3, 0.1, 0.5, 0.987):
            p = (1.0 + rho) / 2.0
            got = po.rouwenhorst_matrix_complex(n, complex(p, 0.0))
            assert np.array_equal(got.real, rouwenhorst_matrix(n, p, p)) and not got.imag.any()


@pytest.mark.parametrize("n", [2, 3, 5, 16, 32])
@pytest.mark.parametrize("rho", [-0.3, 0.1, 0.5, 0.987])
def test_generator_identity(n, rho):
    gen = S.rouwenhorst_generator(n, rho)
    assert gen.shape == (3, n)
    G = po.dense_generator(gen)
    theta = rouwenhorst_matrix(n, (1.0 + rho) / 2.0, (1.0 + rho) / 2.0)
    h = 1e-30
    dtheta = np.imag(po.rouwenhorst_matrix_complex(n, complex((1.0 + rho) / 2.0, h / 2.0))) / h    # dp/dρ = 1/2
    scale = np.max(np.abs(dtheta))
    assert np.max(np.abs(G @ theta - dtheta)) <= 1e-12 * scale
    assert np.max(np.abs(theta @ G - dtheta)) <= 1e-12 * scale


def test_generator_entries_and_refusals():
    n, rho = 5, 0.4
    sub, diag, sup = S.rouwenhorst_generator(n, rho)
    i = np.arange(n)
    np.testing.assert_allclose(sub, -i / (2 * rho), rtol=1e-15)
    np.testing.assert_allclose(diag, np.full(n, (n - 1) / (2 * rho)), rtol=1e-15)
    np.testing.assert_allclose(sup, -(n - 1 - i) / (2 * rho), rtol=1e-15)
    for bad in (0.0, 1.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            S.rouwenhorst_generator(4, bad)


def test_persistence_name_sets():
    assert sens.SSY_PERSISTENCE == ("ρ", "ρ_z", "ρ_c", "ρ_λ")
    assert sens.GCY_PERSISTENCE == ("ρ_λ", "ρ", "ρ_c", "ρ_z", "ρ_ππ", "ρ_zπ")
    assert set(sens.SSY_PERSISTENCE) | set(sens.SSY_SUPPORTED) == set(sens.SSY_PARAMS)
    assert set(sens.GCY_PERSISTENCE) | set(sens.GCY_SUPPORTED) == set(sens.GCY_PARAMS)
    assert not set(sens.SSY_PERSISTENCE) & set(sens.SSY_SUPPORTED)
    assert not set(sens.GCY_PERSISTENCE) & set(sens.GCY_SUPPORTED)


# -- (2) discretisation tangents ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", PERSISTENCE_CASES)
def test_persistence_tangent_vs_central_differences(kind, name):
    shapes = SSY_SHAPES if kind == "ssy" else GCY_SHAPES
    names = sens.SSY_PARAMS if kind == "ssy" else sens.GCY_PARAMS
    m = _model(kind)
    dparams, darrays, dgen = _tangent(kind)(m, shapes, name)
    want_p = np.zeros(len(names)); want_p[names.index(name)] = 1.0
    np.testing.assert_array_equal(dparams, want_p)
    want = _fd(kind, shapes, name)
    arrays = _disc(kind)(m, shapes)
    assert len(darrays) == len(arrays)
    scale = max(np.max(np.abs(w)) for w in want)
    assert scale > 0.0
    for i, (got, w, a) in enumerate(zip(darrays, want, arrays)):
        assert got.shape == a.shape, i
        err = np.max(np.abs(got - w))
        assert err <= 1e-7 * max(np.max(np.abs(w)), 1e-300) or err <= 1e-12 * max(scale, 1.0), (name, i, err)
    # one generator, on the stated axis, and the transition slices are G Q
    axis = (SSY_AXIS if kind == "ssy" else GCY_AXIS)[name]
    assert len(dgen) == len(shapes)
    assert [g is not None for g in dgen] == [a == axis for a in range(len(shapes))]
    rho = dict(zip(names, m.params))[name]
    np.testing.assert_array_equal(dgen[axis], S.rouwenhorst_generator(shapes[axis], rho))
    G = po.dense_generator(dgen[axis])
    for ax, it in enumerate(po.TRANSITION[kind]):
        Q = arrays[it]
        if ax != axis:
            assert not darrays[it].any()
            continue
        wantQ = np.einsum("ij,...jk->...ik", G, Q)
        assert np.max(np.abs(darrays[it] - wantQ)) <= 1e-14 * np.max(np.abs(wantQ))
        assert np.max(np.abs(darrays[it].sum(axis=-1))) <= 1e-13 * np.max(np.abs(wantQ))    # rows of Q keep summing to 1


# -- (3) the stencil formula --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", PERSISTENCE_CASES)
def test_stencil_formula_vs_complex_step_of_T(kind, name):
    shapes = (4, 7, 6, 5) if kind == "ssy" else (3, 4, 2, 3, 5, 4)
    m = _model(kind)
    arrays = _disc(kind)(m, shapes)
    dp, da, dgen = _tangent(kind)(m, shapes, name)
    w = 500.0 + 200.0 * np.random.default_rng(sum(shapes)).random(shapes)
    want = po.complex_step_tangent(kind, shapes, m.params, arrays, dp, da, w)
    got = po.stencil_tangent(kind, shapes, m.params, arrays, dp, da, dgen, w)
    scale = np.max(np.abs(want))
    err = np.max(np.abs(got - want)) / scale
    assert err <= 1e-10, f"{kind} {name}: {err:.3e} relative to max|dT/dρ| = {scale:.3e}"


# -- (4) refusals -------------------------------------------------------------------------------------------------------
def test_persistence_tangent_refusals():
    with pytest.raises(ValueError, match="Rouwenhorst"):
        S.discretize_ssy_persistence_tangent(S.SSY(), SSY_SHAPES, "ρ", method="tauchen")
    with pytest.raises(ValueError, match="Rouwenhorst"):
        S.discretize_gcy_persistence_tangent(S.GCY(), GCY_SHAPES, "ρ_ππ", method="tauchen")
    with pytest.raises(ValueError, match="unknown"):
        S.discretize_ssy_persistence_tangent(S.SSY(), SSY_SHAPES, "rho")
    with pytest.raises(ValueError, match="unknown"):
        S.discretize_gcy_persistence_tangent(S.GCY(), GCY_SHAPES, "ρ_q")
    for name in sens.SSY_SUPPORTED:
        with pytest.raises(ValueError, match="not a persistence"):
            S.discretize_ssy_persistence_tangent(S.SSY(), SSY_SHAPES, name)
    for name in sens.GCY_SUPPORTED:
        with pytest.raises(ValueError, match="not a persistence"):
            S.discretize_gcy_persistence_tangent(S.GCY(), GCY_SHAPES, name)


def test_sensitivities_still_refuse_unknown_names_with_persistence():
    # (checked on the host before any operator is built: runs without a GPU)
    with pytest.raises(ValueError, match="unknown"):
        S.wc_ratio_sensitivities(S.GCY(), GCY_SHAPES, np.ones(GCY_SHAPES), wrt=["ρ_ππ", "rho"], persistence=True)
    with pytest.raises(ValueError, match="persistence"):
        S.wc_ratio_sensitivities(S.SSY(), SSY_SHAPES, np.ones(SSY_SHAPES), wrt="ρ_z", persistence=False)

"""
CPU tests of the adjoint gradient of the continuous-state model: the numpy twin tests/cont_adjoint_oracle.py
against the forward twin of tests/cont_sens_oracle.py, and the argument checks of ``wc_ratio_gradient_continuous``, none of
which needs a device.

BOUND.  ⟨λ_ref, ∂T/∂p_k⟩ = ⟨g, dw/dp_k⟩ to 1e-9 × Σ|g| · max|dw/dp_k|: the two sides are one dense solve each of the same
matrix (its transpose on one side), so their distance is cond₂(I − J) roundings of a sum of that size (cond₂ is printed;
about 5e2 on these cases, the distance about 3e-15 of that scale).
"""
import numpy as np
import pytest

import cont_adjoint_oracle as ao
import cont_boxes as CB
import cont_sens_oracle as so
import cont_sim_cases as CC

TWIN_RTOL = 1e-9


@pytest.mark.parametrize("name", ["A4", "A6"])
def test_adjoint_gradient_is_the_forward_one(name):
    kind, params, grids, nodes, weights = CB.make_case(so.CASES[so.CASE_IDS.index(name)])
    par = tuple(float(q) for q in params)
    w = CC.smooth_w(grids)
    J = ao.jacobian(kind, par, grids, w, nodes, weights)
    dT, aT, _ = so.tangent(kind, par, grids, w, nodes, weights)
    sens, cond = so.dense_sensitivities(kind, par, grids, w, nodes, weights)
    rng = np.random.default_rng(31)
    worst = 0.0
    for g in (np.full(w.size, 1.0 / w.size), rng.standard_normal(w.size)):
        lam, cond_t = ao.adjoint(J, g)
        assert cond_t == cond
        grad, comp, _ = ao.gradient(dT, aT, lam)
        assert np.all(np.abs(grad) <= comp * (1 + 1e-12))
        for k in range(dT.shape[0]):
            fwd = float(g @ sens[k].ravel())
            scale = np.sum(np.abs(g)) * np.max(np.abs(sens[k]))
            assert scale > 0
            worst = max(worst, abs(grad[k] - fwd) / scale)
            assert abs(grad[k] - fwd) <= TWIN_RTOL * scale, (name, k, grad[k], fwd)
    print(f"{name}: cond2(I - J) = {cond:.3e}, worst |adjoint - forward| / (sum|g| max|dw/dp|) = {worst:.3e}")


def test_vjp_twin_is_the_transpose():
    kind, params, grids, nodes, weights = CB.make_case(so.CASES[so.CASE_IDS.index("A4")])
    w = CC.smooth_w(grids)
    J = ao.jacobian(kind, tuple(float(q) for q in params), grids, w, nodes, weights)
    rng = np.random.default_rng(32)
    u, v = rng.standard_normal(w.size), rng.standard_normal(w.size)
    jtu, comp = ao.vjp(J, u)
    assert np.all(np.abs(jtu) <= comp * (1 + 1e-12))
    assert abs(u @ (J @ v) - jtu @ v) <= 1e-13 * (np.abs(u) @ (J @ np.abs(v)))


# -- the public interface, before any device work --------------------------------------------------------------------------
def _request():
    import sdfs_via_autodiff_amd as S
    kind, sizes, sd = CC.GRIDS[0]
    model = S.SSY()
    grids = CC.grids_of(kind, sizes, sd)
    w = CC.golden_wstar(kind, sizes, sd)
    return S, model, grids, w, np.full(w.shape, 1.0 / w.size)


def test_exports():
    import sdfs_via_autodiff_amd as S
    assert "wc_ratio_gradient_continuous" in S.__all__ and callable(S.wc_ratio_gradient_continuous)
    for m in ("cont_vjp_dev", "cont_vjp", "cont_solve_adjoint_dev"):
        assert callable(getattr(S.ContinuousOperator, m)), m
    from sdfs_via_autodiff_amd import _lib
    assert _lib.lib.sdfs_cont_apply_vjp_dev and _lib.lib.sdfs_cont_solve_adjoint_dev


def test_argument_checks_need_no_device():
    S, model, grids, w, g = _request()
    f = S.wc_ratio_gradient_continuous
    with pytest.raises(TypeError, match="SSY or a GCY"):
        f(object(), grids, w, g)
    with pytest.raises(ValueError, match="unknown SSY parameter"):
        f(model, grids, w, g, wrt=["β", "ρ_ππ"])
    with pytest.raises(ValueError, match="unknown SSY parameter"):
        f(model, grids, w, g, wrt="nope")
    with pytest.raises(TypeError):
        f(model, grids, w, g, wrt=3)
    with pytest.raises(ValueError, match="g has shape"):
        f(model, grids, w, g[:-1])
    with pytest.raises(ValueError, match="g has shape"):
        f(model, grids, w, g.ravel())
    for bad in (float("nan"), float("inf")):
        gb = g.copy()
        gb[0, 1, 2, 3] = bad
        with pytest.raises(ValueError, match="g must be finite"):
            f(model, grids, w, gb)
    with pytest.raises(ValueError, match="rtol"):
        f(model, grids, w, g, rtol=0.0)
    with pytest.raises(ValueError, match="rtol"):
        f(model, grids, w, g, rtol="tight")
    with pytest.raises(ValueError, match="atol"):
        f(model, grids, w, g, atol=float("nan"))
    with pytest.raises(ValueError, match="atol"):
        f(model, grids, w, g, atol=-1.0)
    with pytest.raises(ValueError, match="w_star must exceed 1"):
        f(model, grids, np.ones_like(w), g)
    wb = w.copy()
    wb[1, 1, 1, 1] = 1.0
    with pytest.raises(ValueError, match="w_star must exceed 1"):
        f(model, grids, wb, g)
    # ... and what it shares with its forward twin, with the twin's messages
    with pytest.raises(ValueError, match="4 state variables"):
        f(model, grids[:3], w, g)
    with pytest.raises(ValueError, match="w_star has shape"):
        f(model, grids, w[:-1], g)
    with pytest.raises(TypeError, match="ContinuousOperator"):
        f(model, grids, w, g, operator=object())
    with pytest.raises(ValueError, match="d must be"):
        f(model, grids, w, g, d=0)

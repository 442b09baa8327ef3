"""
CPU tests of the continuous-state parameter sensitivities: the numpy twin tests/cont_sens_oracle.py against
itself (analytic tangent against the complex step), the input conditions of tests/test_hip_cont_sensitivity.py, and the
argument checks of ``wc_ratio_sensitivities_continuous``, none of which needs a device.

BOUND.  analytic = complex step to 1e-10 × the abs companion: the two share no derivative code, so the distance is their
rounding (measured: ≤ 3e-15 × abs on every case below).
"""
import numpy as np
import pytest

import cont_boxes as CB
import cont_pricing_oracle as cp
import cont_sens_oracle as so
import cont_sim_cases as CC
from oracle import continuous as OC

TWIN_RTOL = 1e-10
MIN_LINE_DISTANCE = 1e-6
FIXED_POINT_GRIDS = [g for g in CC.GRIDS if g not in CC.NO_FIXED_POINT]
SENS_QUAD_D = 4                  # the end-to-end operator's Gauss–Hermite order: an odd order puts its zero node on grid lines
# A6: θ's two (ψ, γ), a persistence (ρ_λ), ρ_π, a φ (φ_z), and s_zπ, ρ_zπ, ρ
A6_PARAMS = (1, 2, 3, 8, 9, 17, 16, 7)

_CASE = {}


def case_inputs(name):
    if name not in _CASE:
        kind, params, grids, nodes, weights = CB.make_case(so.CASES[so.CASE_IDS.index(name)])
        _CASE[name] = (kind, tuple(float(q) for q in params), grids, nodes, weights, CC.smooth_w(grids))
    return _CASE[name]


_TAN = {}


def twin_tangent(name):
    if name not in _TAN:
        kind, par, grids, nodes, weights, w = case_inputs(name)
        _TAN[name] = so.tangent(kind, par, grids, w, nodes, weights)
    return _TAN[name]


@pytest.mark.parametrize("name,which", [("A4", None), ("B4", None), ("D4", None), ("A6", A6_PARAMS)])
def test_analytic_tangent_is_the_complex_step(name, which):
    kind, par, grids, nodes, weights, w = case_inputs(name)
    dT, aT, Tw = twin_tangent(name)
    np.testing.assert_allclose(Tw, OC.T_fun_factory(kind, par, grids, nodes, weights)(w), rtol=1e-12, atol=0)
    cs = so.complex_step(kind, par, grids, w, nodes, weights, which)
    assert len(cs) == (so.PLACES[kind]["np"] if which is None else len(which))
    worst = 0.0
    for j, v in cs.items():
        err = np.abs(v - dT[j])
        assert np.all(err <= TWIN_RTOL * aT[j]), (name, j)
        assert np.all(np.abs(dT[j]) <= aT[j] * (1 + 1e-12))
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(aT[j] > 0, err / aT[j], 0.0))))
    print(f"{name}: analytic vs complex step, worst |Δ| / abs = {worst:.3e}")


def test_longdouble_twin_agrees():
    kind, par, grids, nodes, weights, w = case_inputs("A4")
    dT, aT, _ = twin_tangent("A4")
    dL = so.tangent(kind, par, grids, w, nodes, weights, dtype=np.longdouble)[0]
    assert np.all(np.abs(dL.astype(np.float64) - dT) <= 1e-13 * aT)


@pytest.mark.parametrize("name", so.CASE_IDS)
def test_no_node_of_the_operator_cases_lies_on_a_grid_line(name):
    kind, par, grids, nodes, _, _ = case_inputs(name)
    dist = so.min_line_distance(kind, par, grids, nodes)
    print(f"{name}: smallest distance of an in-range node coordinate to a grid line = {dist:.3e} cells")
    assert dist > MIN_LINE_DISTANCE


@pytest.mark.parametrize("grid", FIXED_POINT_GRIDS, ids=[CC.tag(*g) for g in FIXED_POINT_GRIDS])
def test_no_node_of_the_fixed_point_grids_lies_on_a_grid_line_at_order_4(grid):
    kind, sizes, sd = grid
    grids = CC.grids_of(kind, sizes, sd)
    nodes, _ = OC.qnwnorm([SENS_QUAD_D] * len(sizes))
    dist = so.min_line_distance(kind, CC.params_of(kind), grids, np.ascontiguousarray(nodes.T))
    print(f"{CC.tag(*grid)}: {dist:.3e} cells")
    assert dist > MIN_LINE_DISTANCE
    # ... and the odd order does put nodes exactly on lines there, which is why the end-to-end test avoids it
    nodes3, _ = OC.qnwnorm([3] * len(sizes))
    assert so.min_line_distance(kind, CC.params_of(kind), grids, np.ascontiguousarray(nodes3.T)) == 0.0


def test_every_parameter_moves_t_on_every_gather_path():
    """Per dimension count and gather path (1 pre-contracted, 2 staged, 3 global gather, by cont_boxes.classify), every
    parameter has a non-zero tangent at some block of that path in at least one case."""
    hit = {}
    assert so.CASE_IDS[:7] == cp.CASE_IDS
    for name in so.CASE_IDS:
        kind, par, grids, nodes, _, _ = case_inputs(name)
        info = CB.classify(kind, par, grids, nodes)
        case = so.CASES[so.CASE_IDS.index(name)]
        assert (info["cls"], info["n_staged"], info["n_unstaged"]) == case[5:8], name
        dT = twin_tangent(name)[0]
        masks = {3: ~info["staged"]}
        masks[1 if info["precontract"] else 2] = info["staged"]
        for path, mask in masks.items():
            if not mask.any():
                continue
            moved = hit.setdefault((len(grids), path), np.zeros(dT.shape[0], dtype=bool))
            moved |= np.array([np.any(dT[j][mask] != 0.0) for j in range(dT.shape[0])])
    assert set(hit) == {(D, path) for D in (4, 6) for path in (1, 2, 3)}, sorted(hit)
    for key, moved in hit.items():
        assert moved.all(), (key, np.flatnonzero(~moved))


# -- the public interface, before any device work --------------------------------------------------------------------------
def _request():
    import sdfs_via_autodiff_amd as S
    kind, sizes, sd = CC.GRIDS[0]
    model = S.SSY()
    grids = CC.grids_of(kind, sizes, sd)
    return S, model, grids, CC.golden_wstar(kind, sizes, sd)


def test_exports():
    import sdfs_via_autodiff_amd as S
    assert "wc_ratio_sensitivities_continuous" in S.__all__ and callable(S.wc_ratio_sensitivities_continuous)
    assert callable(S.ContinuousOperator.cont_param_tangent_dev) and callable(S.ContinuousOperator.cont_param_tangent)
    assert len(S.SSY_PARAMS) == 13 and len(S.GCY_PARAMS) == 18


def test_argument_checks_need_no_device():
    S, model, grids, w = _request()
    f = S.wc_ratio_sensitivities_continuous
    with pytest.raises(ValueError, match="unknown SSY parameter"):
        f(model, grids, w, wrt=["β", "ρ_ππ"])
    with pytest.raises(ValueError, match="unknown SSY parameter"):
        f(model, grids, w, wrt="nope")
    with pytest.raises(TypeError):
        f(model, grids, w, wrt=3)
    with pytest.raises(ValueError, match="4 state variables"):
        f(model, grids[:3], w)
    with pytest.raises(ValueError, match="w_star"):
        f(model, grids, w[:-1])
    with pytest.raises(ValueError, match="w_star"):
        f(model, grids, np.ones_like(w))
    with pytest.raises(TypeError, match="ContinuousOperator"):
        f(model, grids, w, operator=object())
    with pytest.raises(TypeError):
        f(object(), grids, w)
    with pytest.raises(ValueError, match="rtol"):
        f(model, grids, w, rtol=0.0)
    with pytest.raises(ValueError, match="atol"):
        f(model, grids, w, atol=float("nan"))
    with pytest.raises(ValueError, match="d must be"):
        f(model, grids, w, d=0)

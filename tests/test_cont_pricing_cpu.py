"""
CPU tests of continuous-state pricing (sdfs_via_autodiff_amd/pricing.py ``sdf_moments_continuous``,
``term_structure_continuous``, ``claim_prices_continuous``): the numpy twin tests/cont_pricing_oracle.py
against the quantities it must reduce to, the input conditions the GPU file (tests/test_hip_cont_pricing.py) relies on,
and the request errors.  No GPU.

 (1) ``cont_boxes.classify`` puts the operator cases on the gather paths their names say;
 (2) the twin's K(1, θ, −γ)·1 is ``cont_sim_oracle.sdf_mean``;
 (3) at the golden fixed points K(1, θ, 1−γ) is J(w*) up to |θ−1| |Tw − w| / (w − 1);
 (4) the closed form at a constant w;
 (5) the spectral radii and condition numbers behind the claim tests;
 (6) the overflow behind the term-structure refusal;
 (7) every request error of the three public functions raises before a device is touched.
"""
import numpy as np
import pytest

import sdfs_via_autodiff_amd as S
from sdfs_via_autodiff_amd import _lib

import cont_boxes as CB
import cont_pricing_oracle as cp
import cont_sim_cases as CC
import cont_sim_oracle as co
from oracle import continuous as OC

GRID_IDS = [CC.tag(*g) for g in CC.GRIDS]
FIXED = [g for g in CC.GRIDS if g not in CC.NO_FIXED_POINT]


def quad(kind):
    nodes, weights = OC.qnwnorm([CC.QUAD_D] * (4 if kind == "ssy" else 6))
    return np.ascontiguousarray(nodes.T), weights


def test_exports():
    for name in ("sdf_moments_continuous", "term_structure_continuous", "claim_prices_continuous"):
        assert name in S.__all__ and callable(getattr(S, name))
    for name in ("sdfs_cont_set_tilt_dev", "sdfs_cont_apply_tilted_dev", "sdfs_cont_solve_tilted_dev",
                 "sdfs_cont_tilted_horizons_dev"):
        assert name in _lib.SYMBOLS
    for name in ("cont_set_tilt_dev", "cont_apply_tilted_dev", "cont_solve_tilted_dev", "cont_tilted_horizons_dev"):
        assert callable(getattr(S.ContinuousOperator, name))


# -- (1) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cp.CASES, ids=cp.CASE_IDS)
def test_operator_cases_take_the_gather_paths_of_their_names(case):
    model, params, grids, nodes, _ = CB.make_case(case)
    c = CB.classify(model, params, grids, nodes)
    assert (c["cls"], c["n_staged"], c["n_unstaged"]) == case[5:8]
    M = nodes.shape[1]
    assert M in (81, 100, 729) and (M % 256 != 0)          # idle lanes in the last 256-lane trip of every case


# -- (2) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", CC.GRIDS, ids=GRID_IDS)
def test_twin_k1_of_one_is_the_sdf_mean(grid):
    kind, sizes, sd = grid
    par, grids = CC.params_of(kind), CC.grids_of(kind, sizes, sd)
    theta, _, gamma = co.pieces(kind, par)[:3]
    nodes, weights = quad(kind)
    w = CC.golden_wstar(kind, sizes, sd)
    want = co.sdf_mean(kind, par, grids, w, nodes, weights)
    setting = [(1, theta, -gamma)]
    got = cp.apply(kind, par, grids, w, np.ones(sizes), nodes, weights, setting)[0]
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    K = cp.dense(kind, par, grids, w, nodes, weights, setting)[0]
    np.testing.assert_allclose((K @ np.ones(K.shape[0])).reshape(sizes), want, rtol=1e-13, atol=0)


# -- (3) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", FIXED, ids=[CC.tag(*g) for g in FIXED])
def test_twin_k1_at_one_minus_gamma_is_the_jacobian_at_a_fixed_point(grid):
    kind, sizes, sd = grid
    par, grids = CC.params_of(kind), CC.grids_of(kind, sizes, sd)
    theta, _, gamma = co.pieces(kind, par)[:3]
    nodes, weights = quad(kind)
    w = CC.golden_wstar(kind, sizes, sd)
    f = np.random.default_rng(7).standard_normal(sizes)
    Tw = OC.T_fun_factory(kind, par, grids, nodes, weights)(w)
    J = OC.jvp_factory(kind, par, grids, nodes, weights)
    got = cp.apply(kind, par, grids, w, f, nodes, weights, [(1, theta, 1.0 - gamma)])[0]
    bound = (2.0 * abs(theta - 1.0) * np.max(np.abs(Tw - w)) / (np.min(w) - 1.0) + 1e-12) * J(w, np.abs(f))
    assert np.all(np.abs(got - J(w, f)) <= bound)


# -- (4) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A4", "A6"])
def test_twin_at_a_constant_w_is_the_closed_form(name):
    case = cp.CASES[cp.CASE_IDS.index(name)]
    kind, par, grids, nodes, weights = CB.make_case(case)
    par = tuple(float(q) for q in par)
    sizes = case[2]
    n1, w1 = OC.qnwnorm([case[4][1]])
    c = 650.0
    settings = cp.settings_of(kind, par)
    got = cp.apply(kind, par, grids, np.full(sizes, c), np.ones(sizes), nodes, weights, settings)
    for g, (p, kl, kc) in zip(got, settings):
        np.testing.assert_allclose(g, cp.closed_form_constant_w(kind, par, grids, c, n1[:, 0], w1, p, kl, kc), rtol=1e-13, atol=0)


# -- (5) ------------------------------------------------------------------------------------------------------------------
def test_spectral_radii_behind_the_claim_tests():
    rows = []
    for grid, k in cp.claim_pairs():
        K = cp.dense_at_golden(grid, [k])[k]
        r, cond = cp.spectral_radius(K), np.linalg.cond(np.eye(K.shape[0]) - K)
        rows.append((CC.tag(*grid), k, r, cond))
        assert r < 0.9998, rows[-1]
        assert cond <= 2.7e3, rows[-1]
    for grid, k in cp.refused_pairs():
        r = cp.spectral_radius(cp.dense_at_golden(grid, [k])[k])
        rows.append((CC.tag(*grid), k, r, None))
        assert r > 1.002, rows[-1]
    print(rows)


# -- (6) ------------------------------------------------------------------------------------------------------------------
def test_twin_prices_overflow_where_the_term_structure_is_refused():
    (grid,) = CC.NO_FIXED_POINT
    K = cp.dense_at_golden(grid, [0.0])[0.0]
    Ps = cp.powers_of_one(K, 999)
    assert not all(np.all(np.isfinite(p) & (p > 0)) for p in Ps)


# -- (7) ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def request_case():
    m = S.SSY()
    grids = S.build_grid(m, 2, 3, 4, 5)
    return m, grids, np.full((2, 3, 4, 5), 700.0)


def no_device(monkeypatch):
    """Any attempt to open the device fails the test."""
    import torch
    from sdfs_via_autodiff_amd import _requests, pricing

    def boom(*a, **k):
        raise AssertionError("a bad request reached the device")
    monkeypatch.setattr(torch.cuda, "current_stream", boom)
    for module in (_requests, pricing):             # (where it lives, and the name the pricing functions call)
        monkeypatch.setattr(module, "_device_grid", boom)
    monkeypatch.setattr(S.ContinuousOperator, "__init__", boom)


def call(fn, m, grids, w, **kw):
    if fn is S.term_structure_continuous:
        return fn(m, grids, w, kw.pop("n_max", 8), **kw)
    if fn is S.claim_prices_continuous:
        return fn(m, grids, w, kw.pop("kappa", 1.0), **kw)
    return fn(m, grids, w, **kw)


FUNCTIONS = [S.sdf_moments_continuous, S.term_structure_continuous, S.claim_prices_continuous]


@pytest.mark.parametrize("fn", FUNCTIONS, ids=[f.__name__ for f in FUNCTIONS])
def test_shared_request_errors_raise_before_any_device_call(monkeypatch, request_case, fn):
    no_device(monkeypatch)
    m, grids, w = request_case
    with pytest.raises(ValueError, match="w_star has shape"):
        call(fn, m, grids, w[:, :, :, :4])
    bad = w.copy()
    bad[1, 2, 0, 4] = 1.0
    with pytest.raises(ValueError, match="exceed 1"):
        call(fn, m, grids, bad)
    with pytest.raises(ValueError, match="4 state variables, got 3 grids"):
        call(fn, m, grids[:3], w[..., 0])
    with pytest.raises(ValueError, match="6 state variables, got 4 grids"):
        call(fn, S.GCY(), grids, w)
    with pytest.raises(ValueError, match="increasing"):
        call(fn, m, (grids[0][::-1],) + tuple(grids[1:]), w)
    with pytest.raises(TypeError, match="SSY or a GCY"):
        call(fn, object(), grids, w)
    with pytest.raises(ValueError, match="d must be"):
        call(fn, m, grids, w, d=0)
    with pytest.raises(ValueError, match="2\\^24 nodes"):
        call(fn, S.GCY(), S.build_grid(S.GCY(), 2, 2, 2, 2, 2, 2), np.full((2,) * 6, 700.0), d=17)
    with pytest.raises(TypeError, match="ContinuousOperator"):
        call(fn, m, grids, w, operator=object())


BAD_TERM = [
    (dict(n_max=0), "n_max"),
    (dict(n_max=(1 << 24) + 1), "n_max"),
    (dict(n_max=2.0), "n_max"),
    (dict(n_max=True), "n_max"),
    (dict(kappa=float("nan")), "kappa must be finite"),
    (dict(kappa="x"), "kappa must be a real number"),
    (dict(save=(0,)), "save horizon 0"),
    (dict(save=(9,)), "save horizon 9"),
    (dict(states=np.zeros(4)), "states has shape"),
    (dict(states=np.zeros((2, 3))), "states has shape"),
    (dict(states=np.zeros((0, 4))), "states has shape"),
    (dict(states=np.array([[0.0, np.inf, 0.0, 0.0]])), "finite"),
]


@pytest.mark.parametrize("kw,msg", BAD_TERM, ids=[f"{i}:{sorted(k)[0]}" for i, (k, _) in enumerate(BAD_TERM)])
def test_term_structure_request_errors_raise_before_any_device_call(monkeypatch, request_case, kw, msg):
    no_device(monkeypatch)
    m, grids, w = request_case
    with pytest.raises(ValueError, match=msg):
        call(S.term_structure_continuous, m, grids, w, **kw)


BAD_CLAIM = [
    (dict(kappa=float("inf")), "kappa must be finite"),
    (dict(kappa=None), "kappa must be a real number"),
    (dict(rtol=0.0), "rtol must be positive"),
    (dict(rtol=-1e-8), "rtol must be positive"),
    (dict(rtol=float("nan")), "rtol must be positive"),
]


@pytest.mark.parametrize("kw,msg", BAD_CLAIM, ids=[f"{i}:{sorted(k)[0]}" for i, (k, _) in enumerate(BAD_CLAIM)])
def test_claim_prices_request_errors_raise_before_any_device_call(monkeypatch, request_case, kw, msg):
    no_device(monkeypatch)
    m, grids, w = request_case
    with pytest.raises(ValueError, match=msg):
        call(S.claim_prices_continuous, m, grids, w, **kw)


def test_simulate_continuous_shares_the_request_checks():
    """The same request steps serve both callers (the errors of ``simulate_continuous`` themselves:
    tests/test_cont_simulation_cpu.py)."""
    from sdfs_via_autodiff_amd import _requests, pricing, simulation
    for step in ("_cont_grids", "_cont_operator_or_d", "_check_w_star"):
        assert getattr(simulation, step) is getattr(pricing, step) is getattr(_requests, step)

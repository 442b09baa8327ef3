"""
CPU tests of the price sensitivities (sdfs_via_autodiff_amd/pricing.py ``price_sensitivities``):

 (a) the numpy twin of the tilt's tangent (tests/price_sens_oracle.py ``tilt_tangent``) against Richardson-extrapolated
     central differences of ``folded_K`` with the model, the arrays, the exponents, w, Tw and f all moved, every parameter
     (the persistences included) at p = 0, 1, 2;
 (b) ``price_sensitivities_dense`` against central differences of the whole numpy pipeline (a dense Newton re-solve of w*
     at p ± h, then the prices);
 (c) the argument checks of ``price_sensitivities``, which run before any device work (this machine has no GPU to reach).
"""
import numpy as np
import pytest

import sdfs_via_autodiff_amd as S
from sdfs_via_autodiff_amd._requests import LAYOUT
from sdfs_via_autodiff_amd.sensitivity import _directions

from conftest import load_golden
from price_sens_oracle import tilt_tangent, price_sensitivities_dense, prices_dense, newton_dense
from test_pricing_cpu import folded_K

SHAPES = [("ssy", (3, 3, 3, 5)), ("gcy", (2, 3, 2, 3, 2, 3))]


def model_of(kind, **over):
    cls = S.SSY if kind == "ssy" else S.GCY
    d = dict(zip(LAYOUT[kind].params, cls().params))
    d.update(over)
    return cls(**d)


def disc(kind):
    return S.discretize_ssy if kind == "ssy" else S.discretize_gcy


# -- (a) the tangent of K against differences ---------------------------------------------------------------------------
TANGENT_BOUND = 1e-7        # of max|reference|: the project's bound for a tangent against Richardson central differences
                            # (tests/test_hip_sensitivity.py); it belongs to the difference quotient's truncation


@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_twin_tangent_vs_richardson_central_differences(kind, shapes):
    m = model_of(kind)
    arr = disc(kind)(m, shapes)
    names = LAYOUT[kind].params
    p0 = dict(zip(names, m.params))
    rng = np.random.default_rng(11)
    w = 500.0 + 400.0 * rng.random(shapes)
    Tw = w * (1.0 + 0.01 * rng.random(shapes))
    f = 0.5 + rng.random(shapes)
    dw, dTw, df = (rng.standard_normal(shapes) for _ in range(3))
    dkl, dkc = 0.7, -0.4
    th, g = m.θ, m.γ
    worst = {}
    for name, d in zip(names, _directions(m, shapes, names, arr, persistence=True)):
        # a persistence moves its grid like 1 / sqrt(1 - rho^2): the step is taken relative to 1 - rho there
        h = 1e-3 * (1.0 - p0[name]) if name in LAYOUT[kind].persistence else 1e-4 * abs(p0[name])
        for p, kl, kc in [(0, 0.3, 1.0), (1, th, 2.0 - g), (2, 2 * th, -2 * g)]:
            got, _ = tilt_tangent(kind, shapes, m, arr, w, Tw, f, p, kl, kc, d, dkl, dkc, dw, dTw, df)

            def F(t):
                mt = model_of(kind, **{name: p0[name] + t})
                return folded_K(kind, shapes, mt, disc(kind)(mt, shapes), w + t * dw, f + t * df, p, kl + t * dkl, kc + t * dkc,
                                Tw=Tw + t * dTw)

            def cd(step):
                return (F(step) - F(-step)) / (2.0 * step)
            want = (4.0 * cd(h / 2) - cd(h)) / 3.0
            err = np.max(np.abs(got - want)) / np.max(np.abs(want))
            worst[name] = max(worst.get(name, 0.0), err)
    print(kind, {k: f"{v:.1e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= TANGENT_BOUND}
    assert not bad, f"{kind} {shapes}: {bad}"


# -- (b) the whole chain against differences of a re-solve ---------------------------------------------------------------
FIXTURES = {"ssy": ((2, 3, 4, 5), "sa_ssy_2x3x4x5.npz", "w_1e8"), "gcy": ((3,) * 6, "sa_gcy_3x3x3x3x3x3.npz", "w_1e7")}
# γ, μ_c, one φ, one s and one persistence per model (β and ψ: w* curves like 1 / (1 − β)², so that with this step the
# difference quotient, not the formula, is off; test (a) holds them at tangent level)
WRT = {"ssy": ("γ", "μ_c", "φ_c", "s_z", "ρ_c"), "gcy": ("γ", "μ_c", "φ_z", "s_c", "ρ_zπ")}
FD_STEP = 1e-4              # relative to |p|
PIPELINE_BOUND = 1e-6       # ten times the agreement measured on the CPU with step 1e-4 |p| (<= 1.1e-7): the truncation of the
                            # reference side
FIELDS0 = ("E_M", "log_rf", "max_sharpe")
FIELDS = FIELDS0 + ("pd", "expected_return", "log_premium")


@pytest.fixture(scope="module", params=["ssy", "gcy"])
def fixed_point(request):
    kind = request.param
    shapes, file, key = FIXTURES[kind]
    m = model_of(kind)
    arr = disc(kind)(m, shapes)
    w = newton_dense(kind, shapes, m, arr, np.array(load_golden(file)[key], dtype=np.float64))
    p0 = dict(zip(LAYOUT[kind].params, m.params))
    moved = {}
    for name in WRT[kind]:
        h = FD_STEP * abs(p0[name])
        for s in (+1.0, -1.0, +0.5, -0.5):
            mt = model_of(kind, **{name: p0[name] + s * h})
            at = disc(kind)(mt, shapes)
            moved[name, s] = (mt, at, newton_dense(kind, shapes, mt, at, w), s * h)
    return kind, shapes, m, arr, w, moved


@pytest.mark.parametrize("kappa", [0.0, 2.0])
def test_dense_sensitivities_vs_central_differences_of_a_resolve(fixed_point, kappa):
    kind, shapes, m, arr, w, moved = fixed_point
    names = WRT[kind]
    dirs = dict(zip(names, _directions(m, shapes, names, arr, persistence=True)))
    got = price_sensitivities_dense(kind, shapes, m, arr, w, kappa, dirs)
    K = got["_K"]
    r = np.max(np.abs(np.linalg.eigvals(K)))
    base = prices_dense(kind, shapes, m, arr, w, kappa)
    assert r < 1.0 and np.all(base["pd"] > 0), (r, base["pd"].min())
    print(kind, "kappa", kappa, f"r(K) = {r:.4f}, cond2(I - K) = {np.linalg.cond(np.eye(w.size) - K):.1e}")
    for name in names:
        P = {s: prices_dense(kind, shapes, *moved[name, s][:3], kappa) for s in (+1.0, -1.0, +0.5, -0.5)}
        h = moved[name, +1.0][3]
        for fld in FIELDS:
            want = (P[+1.0][fld] - P[-1.0][fld]) / (2.0 * h)
            if name in LAYOUT[kind].persistence:
                # a persistence moves its grid like 1 / sqrt(1 - rho^2): with this step the plain quotient's truncation
                # is 2e-4 of the derivative (SSY rho_c), so the quotients at h and h / 2 are Richardson-extrapolated.
                # (Elsewhere the extrapolation would only triple the quotient's rounding, which is what is left of
                # d log premium / d mu_c, a derivative that nearly vanishes.)
                want = (4.0 * (P[+0.5][fld] - P[-0.5][fld]) / h - want) / 3.0
            err = np.max(np.abs(got[name][fld] - want)) / np.max(np.abs(want))
            print(f"  {name} {fld}: {err:.2e}")
            assert err <= PIPELINE_BOUND, f"{kind} kappa {kappa} {name} {fld}: {err:.3e}"


# -- (c) the argument checks ---------------------------------------------------------------------------------------------
def test_argument_checks_before_device_work():
    m = S.SSY()
    shapes = (3, 3, 3, 5)
    w = np.full(shapes, 800.0)
    with pytest.raises(TypeError):
        S.price_sensitivities(object(), shapes, w)
    with pytest.raises(ValueError, match="4 axes"):
        S.price_sensitivities(m, (3, 3, 3), w)
    with pytest.raises(ValueError, match="kappa"):
        S.price_sensitivities(m, shapes, w, kappa=float("inf"))
    with pytest.raises(ValueError, match="kappa"):
        S.price_sensitivities(m, shapes, w, kappa="two")
    with pytest.raises(ValueError, match="unknown SSY parameter"):
        S.price_sensitivities(m, shapes, w, wrt=("β", "nope"))
    with pytest.raises(ValueError, match="persistence=True"):
        S.price_sensitivities(m, shapes, w, wrt="ρ_c")
    with pytest.raises(ValueError, match="unknown SSY parameter"):
        S.price_sensitivities(m, shapes, w, wrt="ρ_π", persistence=True)
    with pytest.raises(ValueError, match="rtol"):
        S.price_sensitivities(m, shapes, w, rtol=0.0)
    with pytest.raises(ValueError, match="atol"):
        S.price_sensitivities(m, shapes, w, atol=-1.0)
    with pytest.raises(ValueError, match="w_star has shape"):
        S.price_sensitivities(m, shapes, w[:2])
    with pytest.raises(TypeError, match="dw must be"):
        S.price_sensitivities(m, shapes, w, wrt="γ", dw=w)
    with pytest.raises(ValueError, match="no entry"):
        S.price_sensitivities(m, shapes, w, wrt=("γ", "β"), dw={"γ": w})
    with pytest.raises(ValueError, match="has shape"):
        S.price_sensitivities(m, shapes, w, wrt="γ", dw={"γ": w[:2]})
    g = S.GCY()
    with pytest.raises(ValueError, match="6 axes"):
        S.price_sensitivities(g, shapes, w)
    with pytest.raises(ValueError, match="unknown GCY parameter"):
        S.price_sensitivities(g, (2, 3, 2, 3, 2, 3), np.full((2, 3, 2, 3, 2, 3), 800.0), wrt="φ")

"""
CPU tests of the batch pricing layer (``price_batch``, ``price_words_to_stats``, tests/batch_pricing_oracle.py):

 (1) the numpy restatement of the stages of csrc/batch_price.hpp (on ``folded_K``) against dense matrices from the literal
     SDF (``dense_K``: Gauss–Hermite quadrature over the consumption shock) on SSY 3×3×3×5 and a ragged GCY grid;
 (2) ``price_words_to_stats`` against direct numpy;
 (3) the batch kernels' form of the tilted operator, K = d2 ⊙ H(d1 ⊙ ·) with d1 = c_in^p t1, d2 = c_out^p t2 t3, against
     ``folded_K`` for the four tilts of ``tilts(model)`` and for (1, θ, 1−γ), where it is J;
 (4) the refusals of ``price_batch``, all before any device call (this machine has no GPU to reach).
"""
import numpy as np
import pytest

import sdfs_via_autodiff_amd as S
import batch_family as bf
import batch_pricing_oracle as bpo
from test_pricing_cpu import SHAPES, dense_K, folded_K, grid_w, model_of, oracle_T, tilts
from oracle import ssy as ossy, gcy as ogcy

KAPPA = 2.0


def family_member(kind, shapes):
    """Member 0 of the batch family at its fixed point by the oracle's successive approximation (tol 1e-6): there the
    claim's K at κ = 2 is a contraction (the test checks that it is)."""
    over = bf.member(kind, 0)
    m = bf.package_model(S, kind, over)
    w, _, _ = bf.oracle_solve(kind, shapes, over, tol=1e-6)
    return m, bpo.discretize(S, kind, m, shapes), w


@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_restatement_against_literal_dense_sdf(kind, shapes):
    m, arr, w = family_member(kind, shapes)
    mem = bpo.Member(kind, shapes, m, arr, w)
    N = int(np.prod(shapes))
    one = np.ones(N)
    th, ga = m.θ, m.γ
    D = lambda p, kl, kc: dense_K(kind, shapes, m, arr, w, p, kl, kc)      # noqa: E731
    Kc = D(1, th, KAPPA - ga)
    radius = np.max(np.abs(np.linalg.eigvals(Kc)))
    assert radius < 1.0, radius
    inv_norm = np.linalg.norm(np.linalg.inv(np.eye(N) - Kc), np.inf)
    want = {"E_M": D(1, th, -ga) @ one, "E_M2": D(2, 2 * th, -2 * ga) @ one, "pd": np.linalg.solve(np.eye(N) - Kc, Kc @ one)}
    want["expected_return"] = D(0, 0.0, KAPPA) @ (1.0 + want["pd"]) / want["pd"]
    got = bpo.stages(mem, KAPPA)
    assert np.all(got["pd"] > 0)
    # the two forms of K agree to 1e-13 entry by entry (test_folded_K_matches_literal_dense_sdf); a solve magnifies that
    # by at most ‖(I − K)⁻¹‖∞ (‖K‖∞ + 1) relative to max v
    tol = {"E_M": 1e-13, "E_M2": 1e-13, "pd": 1e-13 * inv_norm * 4.0, "expected_return": 1e-13 * inv_norm * 8.0}
    for k, ref in want.items():
        rel = np.max(np.abs(got[k].reshape(-1) - ref)) / np.max(np.abs(ref))
        assert rel <= tol[k], (k, rel, tol[k])
    # the residual the GPU tests measure is at rounding level for the dense solution
    r, k1 = mem.claim_residual(got["pd"], KAPPA)
    assert np.linalg.norm(r) <= 1e-12 * inv_norm * np.linalg.norm(k1)
    # horizons: matrix powers of the dense K
    gw = bpo.point_weights(S.stationary_weights(m, shapes))
    rows = mem.horizons(0.0, 12, gw)
    Kt = D(1, th, -ga)
    P = one.copy()
    for n in range(1, 13):
        Pn = Kt @ P
        ref = np.array([gw.reshape(-1) @ Pn, gw.reshape(-1) @ -np.log(Pn) / n, (Pn / P).min(), (Pn / P).max()])
        # (dense_K takes T w from oracle_T in fp64: its yields carry the offset of
        # test_extended_Tw_and_the_bias_of_fp64_yields, at most (1 − θ) 2e-15, which the restatement does not)
        np.testing.assert_allclose(rows[n - 1, [0, 2, 3]], ref[[0, 2, 3]], rtol=1e-12 * n)
        np.testing.assert_allclose(rows[n - 1, 1], ref[1], rtol=1e-12 * n, atol=(1.0 - th) * 2e-15)
        P = Pn
    # the words: against direct sums over the dense grids
    wd, scale = bpo.words(gw, got["E_M"], got["E_M2"], got["pd"], got["expected_return"])
    g1 = gw.reshape(-1)
    lr, lv, le = -np.log(want["E_M"]), np.log(want["pd"]), np.log(want["expected_return"])
    lp = le - lr
    ref = np.array([g1.sum(), g1 @ lr, g1 @ lr ** 2, g1 @ np.sqrt(np.maximum(want["E_M2"] / want["E_M"] ** 2 - 1, 0)),
                    g1 @ lv, g1 @ lv ** 2, g1 @ le, g1 @ lp, g1 @ lp ** 2, want["pd"].min(), want["pd"].max(), 0.0])
    assert np.all(np.abs(wd - ref) <= 1e-12 * inv_norm * (scale + np.abs(ref)) + 1e-300)
    assert np.all(scale[:9] >= np.abs(wd[:9])) and np.all(scale[9:] == 0)


@pytest.mark.parametrize("kind,shapes", SHAPES + [("gcy", (3,) * 6)])
def test_extended_Tw_and_the_bias_of_fp64_yields(kind, shapes):
    """``extended_Tw`` is ``oracle_T`` to a few ulp of T w − 1, and yet the yields of repeated ``folded_K`` move by up to
    1e-14 between the two at GCY: the offset is the same at every horizon (a bias, not noise), which is why the oracle of
    the horizon tests takes T w from extended precision."""
    m, arr, w = family_member(kind, shapes)
    Tx = bpo.extended_Tw(kind, shapes, m, arr, w)
    Td = oracle_T(kind, shapes, m, arr, w)
    assert np.max(np.abs((Td - 1.0) / (Tx - 1.0) - 1.0)) <= 2e-15
    gw = bpo.point_weights(S.stationary_weights(m, shapes))
    mem = bpo.Member(kind, shapes, m, arr, w)
    assert np.array_equal(mem.Tw, Tx)
    yx = mem.horizons(0.0, 20, gw)[:, 1]
    mem.Tw = Td
    yd = mem.horizons(0.0, 20, gw)[:, 1]
    diff = yd - yx
    print(f"{kind} {shapes}: yields with fp64 T w minus yields with extended T w: {diff.min():.3e} ... {diff.max():.3e}")
    assert np.max(np.abs(diff)) <= (1.0 - m.θ) * 2e-15           # the power's amplification of the few ulp above
    assert np.max(np.abs(diff - diff.mean())) <= 2e-15           # ... and it is an offset: the same at every horizon


def test_words_without_a_claim_and_without_a_price():
    rng = np.random.default_rng(0)
    shp = (3, 4)
    gw = rng.random(shp)
    E_M, E_M2 = 0.9 + 0.1 * rng.random(shp), 1.0 + rng.random(shp)
    wd, scale = bpo.words(gw, E_M, E_M2)
    assert np.all(np.isfinite(wd[:4])) and np.all(np.isnan(wd[4:]))
    v = rng.random(shp) + 0.5
    v[1, 2] = -0.25
    wd, _ = bpo.words(gw, E_M, E_M2, v, None)
    assert np.all(np.isnan(wd[4:9]))
    assert wd[9] == -0.25 and wd[10] == v.max() and wd[11] == 1.0


def test_price_words_to_stats_against_direct_numpy():
    rng = np.random.default_rng(3)
    B, shp = 4, (3, 5, 2)
    mom = np.empty((B, 12))
    want = {k: np.empty(B) for k in ("log_rf_mean", "log_rf_std", "max_sharpe_mean", "log_pd_mean", "log_pd_std",
                                      "log_expected_return_mean", "log_premium_mean", "log_premium_std", "pd_min", "pd_max")}
    for b in range(B):
        gw = rng.random(shp) * (1.0 + b)                 # (not normalised: the statistics divide by Σg)
        E_M, E_M2 = 0.9 + 0.1 * rng.random(shp), 1.0 + rng.random(shp)
        v, ER = 50.0 + 100.0 * rng.random(shp), 1.0 + 0.01 * rng.random(shp)
        mom[b], _ = bpo.words(gw, E_M, E_M2, v, ER)
        pr = gw / gw.sum()
        lr, hj, lv, le = -np.log(E_M), np.sqrt(np.maximum(E_M2 / E_M ** 2 - 1, 0)), np.log(v), np.log(ER)
        lp = le + np.log(E_M)
        mean = lambda x: float(np.sum(pr * x))           # noqa: E731
        std = lambda x: float(np.sqrt(np.sum(pr * (x - mean(x)) ** 2)))      # noqa: E731
        for k, val in (("log_rf_mean", mean(lr)), ("log_rf_std", std(lr)), ("max_sharpe_mean", mean(hj)),
                       ("log_pd_mean", mean(lv)), ("log_pd_std", std(lv)), ("log_expected_return_mean", mean(le)),
                       ("log_premium_mean", mean(lp)), ("log_premium_std", std(lp)), ("pd_min", v.min()),
                       ("pd_max", v.max())):
            want[k][b] = val
    got = S.price_words_to_stats(mom)
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == (B,)
        # a standard deviation from m2 − m1² loses the digits of m1² / var: about 1e-16 · 30 / 1e-3 here
        np.testing.assert_allclose(got[k], want[k], rtol=1e-9 if k.endswith("_std") else 1e-13, err_msg=k)
    # a member without a claim: NaN statistics of the claim, finite ones of the SDF; a negative variance by rounding is 0
    mom[1, 4:] = np.nan
    mom[2, 2] = mom[2, 1] ** 2 / mom[2, 0] * (1 - 1e-16)
    got = S.price_words_to_stats(mom)
    assert np.isnan(got["log_pd_mean"][1]) and np.isnan(got["pd_min"][1]) and np.isfinite(got["log_rf_std"][1])
    assert got["log_rf_std"][2] == 0.0
    with pytest.raises(ValueError, match="moments must be"):
        S.price_words_to_stats(np.zeros((3, 11)))


@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_batch_form_of_the_tilted_operator(kind, shapes):
    m = model_of(kind)
    arr = bpo.discretize(S, kind, m, shapes)
    w = grid_w(shapes)
    f = 0.5 + np.random.default_rng(1).random(shapes)
    for p, kl, kc in tilts(m) + [(1, m.θ, 1 - m.γ)]:
        got = bpo.batch_form_K(kind, shapes, m, arr, w, f, p, kl, kc)
        want = folded_K(kind, shapes, m, arr, w, f, p, kl, kc)
        rel = np.max(np.abs(got - want) / np.abs(want))
        # two routes through powers with |θ| of 16-36: a few hundred ulp
        assert rel < 1e-12, f"tilt {(p, kl, kc)}: relative difference {rel:.2e}"
    v = np.random.default_rng(3).standard_normal(shapes)
    jvp = ossy.jvp_ssy if kind == "ssy" else ogcy.jvp_gcy
    want = jvp(w, v, shapes, m.params, arr)
    got = bpo.batch_form_K(kind, shapes, m, arr, w, v, 1, m.θ, 1 - m.γ)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def test_refusals_before_any_device_call():
    shapes = (3, 3, 3, 5)
    models = [S.SSY(), S.SSY(γ=9.0)]
    w = np.full((2,) + shapes, 800.0)
    ok = dict(kappa=2.0)
    with pytest.raises(ValueError, match="4 axes"):
        S.price_batch(models, (3, 3, 3), w, **ok)
    with pytest.raises(ValueError, match="w_star has shape"):
        S.price_batch(models, shapes, w[:1], **ok)
    with pytest.raises(ValueError, match="w_star has shape"):
        S.price_batch(models, shapes, w[0], **ok)
    with pytest.raises(TypeError):
        S.price_batch([S.SSY(), S.GCY()], shapes, w, **ok)
    with pytest.raises(ValueError, match="models is empty"):
        S.price_batch([], shapes, w, **ok)
    with pytest.raises(ValueError, match="kappa"):
        S.price_batch(models, shapes, w, kappa=[2.0, float("nan")])
    with pytest.raises(ValueError, match="kappa"):
        S.price_batch(models, shapes, w, kappa=[2.0, 2.0, 2.0])
    with pytest.raises(ValueError, match="kappa"):
        S.price_batch(models, shapes, w, kappa="two")
    with pytest.raises(ValueError, match="kappa_ts"):
        S.price_batch(models, shapes, w, n_max=4, kappa_ts=float("inf"))
    with pytest.raises(ValueError, match="kappa_ts"):
        S.price_batch(models, shapes, w, n_max=4, kappa_ts=None)
    for bad in (-1, 2.5, True, (1 << 24) + 1):
        with pytest.raises(ValueError, match="n_max"):
            S.price_batch(models, shapes, w, n_max=bad, **ok)
    with pytest.raises(ValueError, match="rtol"):
        S.price_batch(models, shapes, w, rtol=-1.0, **ok)
    with pytest.raises(ValueError, match="rtol"):
        S.price_batch(models, shapes, w, rtol=float("nan"), **ok)
    with pytest.raises(ValueError, match="one entry per axis"):
        S.price_batch(models, shapes, w, weights=[np.ones(3)] * 3, **ok)
    with pytest.raises(ValueError, match="state index"):
        S.price_batch(models, shapes, w, weights=[0, 0, 3, 0], **ok)
    with pytest.raises(ValueError, match="weights\\[3\\] has"):
        S.price_batch(models, shapes, w, weights=[0, 0, 0, np.ones(4)], **ok)
    with pytest.raises(ValueError, match="not finite"):
        S.price_batch(models, shapes, w, weights=[0, 0, 0, np.array([1.0, np.nan, 1.0, 1.0, 1.0])], **ok)
    with pytest.raises(ValueError, match="one entry per axis"):
        S.price_batch(models, shapes, w, weights=[[0, 0, 0, 0], [0, 0, 0]], **ok)
    # a shape beyond one CU takes the member-by-member path: its checks run before a device is touched as well
    big = (12,) * 4
    assert S.batch_lds_bytes("ssy", big) is None
    wb = np.full((2,) + big, 800.0)
    with pytest.raises(ValueError, match="n_max"):
        S.price_batch(models, big, wb, n_max=-3, **ok)
    with pytest.raises(ValueError, match="w_star has shape"):
        S.price_batch(models, big, w, **ok)
    with pytest.raises(ValueError, match="Rouwenhorst"):
        S.price_batch(models, big, wb, method="tauchen", **ok)

"""
CPU tests of the simulation layer (sdfs_via_autodiff_amd/simulation.py) and its numpy twin (tests/sim_oracle.py):

 (1) Philox4x32-10 against the Random123 known-answer vectors, and the unit map u = (r + 0.5) 2^-32 at its ends;
 (2) the twin's index draws: per-axis state frequencies along long stationary paths against ``stationary_weights``;
 (3) the twin's two-pass statistics against direct numpy formulas, including NaN for a zero denominator;
 (4) the cumulative tables, and every argument check of ``simulate`` that runs before any device work (this machine
     needs no GPU for them).
"""
import numpy as np
import pytest

import sdfs_via_autodiff_amd as S
from sdfs_via_autodiff_amd.simulation import cdf_tables

import sim_oracle as so


# -- (1) Philox ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = tuple(int(x) for x in so.philox4x32_10(counter, key))
    assert got == want, [hex(x) for x in got]


def test_philox_vectorised_equals_scalar():
    paths = np.arange(5, 5 + 64, dtype=np.uint64)
    vec = so.philox4x32_10((17, paths, 1, 0), (0x1234, 0x5678))
    for i, p in enumerate(paths):
        one = so.philox4x32_10((17, int(p), 1, 0), (0x1234, 0x5678))
        assert tuple(int(v[i]) for v in vec) == tuple(int(x) for x in one)


def test_unit_interval_ends():
    lo, hi = so.unit(0), so.unit(2 ** 32 - 1)
    assert lo == 2.0 ** -33 and 0.0 < lo
    assert hi == 1.0 - 2.0 ** -33 and hi < 1.0


# -- (2) index draws -----------------------------------------------------------------------------------------------------
def test_index_frequencies_match_stationary_weights():
    shapes = (3, 4, 5, 6)
    m = S.SSY()
    cdf, cdf0 = cdf_tables(m, shapes)
    pis = S.stationary_weights(m, shapes)
    idx, xi = so.index_paths(cdf, cdf0, seed=20240917, path_offset=0, n_paths=512, burn_in=0, n_periods=4096)
    for a, (n, pi) in enumerate(zip(shapes, pis)):
        freq = np.bincount(idx[:, :, a].ravel(), minlength=n) / idx[:, :, a].size
        assert np.max(np.abs(freq - pi)) < 0.01, (a, freq, pi)
    assert abs(xi.mean()) < 0.01 and abs(xi.std() - 1.0) < 0.01


def test_draw_is_least_index_above_u():
    rows = np.array([[0.2, 0.5, 0.5, 2.0]] * 5)
    u = np.array([0.1, 0.2, 0.3, 0.5, 0.9])
    assert so.draw(rows, u).tolist() == [0, 1, 1, 3, 3]


# -- (3) statistics ------------------------------------------------------------------------------------------------------
def test_two_pass_statistics_against_numpy():
    rng = np.random.default_rng(3)
    s = rng.standard_normal((6, 50)) * 0.01 + 7.0
    s[2] = 5.0                                          # constant: ac1 has a zero denominator
    x = rng.standard_normal((6, 50))
    x[4] = 1.5                                          # regressor without variation
    mean, std, ac1 = so.two_pass(s)
    np.testing.assert_allclose(mean, s.mean(axis=1), rtol=1e-14)
    np.testing.assert_allclose(std, s.std(axis=1), rtol=1e-9, atol=1e-15)
    for i in range(6):
        if i == 2:
            assert np.isnan(ac1[i]) and std[i] == 0.0 and mean[i] == 5.0
            continue
        e = s[i] - s[i].mean()
        np.testing.assert_allclose(ac1[i], np.dot(e[1:], e[:-1]) / np.dot(e, e), rtol=1e-9)
    slope = so.ols_slope(x, s)
    for i in range(6):
        if i == 4:
            assert np.isnan(slope[i])
            continue
        np.testing.assert_allclose(slope[i], np.polyfit(x[i], s[i], 1)[0], rtol=1e-8, atol=1e-12)


def test_series_timing_on_a_hand_made_path():
    """One SSY path by hand: dc, m, rf, rc against the DESIGN §4.8 formulas evaluated state by state."""
    shapes = (2, 3, 2, 3)
    m = S.SSY()
    arr = S.discretize_ssy(m, shapes)
    rng = np.random.default_rng(1)
    w = 500.0 + 100.0 * rng.random(shapes)
    em = 0.99 + 0.001 * rng.random(shapes)
    idx = np.array([[[0, 1, 0, 2], [1, 2, 1, 0], [1, 0, 0, 1]]], dtype=np.uint8)
    xi = np.array([[0.3, -1.2]])
    ser, xr = so.series("ssy", m.params, arr, shapes, idx, xi, w, em)
    for t in range(2):
        x0, x1 = tuple(idx[0, t]), tuple(idx[0, t + 1])
        z = arr[6].reshape(2, 3)[x0[2], x0[3]]
        dc = m.μ_c + z + arr[8][x0[1]] * xi[0, t]
        assert ser["dc"][0, t] == pytest.approx(dc, rel=1e-14)
        mm = m.θ * np.log(m.β) + m.θ * arr[0][x1[0]] - m.γ * dc + (m.θ - 1) * (np.log(w[x1]) - np.log(w[x0] - 1))
        assert ser["m"][0, t] == pytest.approx(mm, rel=1e-12)
        assert ser["rf"][0, t] == -np.log(em[x0])
        assert ser["rc"][0, t] == pytest.approx(dc + np.log(w[x1]) - np.log(w[x0] - 1), rel=1e-12)
        assert ser["wc"][0, t] == w[x1]
        assert xr[0, t] == np.log(w[x0] - 1)


# -- (4) tables and argument checks --------------------------------------------------------------------------------------
def test_cdf_tables():
    shapes = (3, 4, 3, 5, 2, 4)
    m = S.GCY()
    cdf, cdf0 = cdf_tables(m, shapes)
    for c, c0, n in zip(cdf, cdf0, shapes):
        assert c.shape == (n, n) and c0.shape == (n,)
        assert np.all(c[:, -1] == 2.0) and c0[-1] == 2.0
        assert np.all(np.diff(c, axis=1) >= 0.0)
    arr = list(S.discretize_ssy(S.SSY(), (3, 3, 3, 4)))
    zQ = arr[7].reshape(3, 4, 4).copy()
    zQ[1] = np.eye(4)
    arr[7] = zQ
    with pytest.raises(ValueError, match="does not factorise"):
        cdf_tables(S.SSY(), (3, 3, 3, 4), arr)


def _args(**kw):
    shapes = (3, 3, 3, 4)
    a = dict(model=S.SSY(), shapes=shapes, w_star=np.full(shapes, 700.0), n_paths=8, n_periods=16)
    a.update(kw)
    return a


@pytest.mark.parametrize("kw,match", [
    (dict(w_star=np.full((3, 3, 3, 5), 700.0)), "shape"),
    (dict(w_star=np.where(np.arange(108).reshape(3, 3, 3, 4) == 5, 1.0, 700.0)), "exceed 1"),
    (dict(w_star=np.full((3, 3, 3, 4), np.nan)), "exceed 1"),
    (dict(n_periods=1), "n_periods"),
    (dict(n_paths=0), "n_paths"),
    (dict(path_offset=2 ** 32 - 4), "2\\^32"),
    (dict(burn_in=2 ** 32 - 16), "2\\^32"),
    (dict(seed=-1), "seed"),
    (dict(seed=2 ** 64), "seed"),
    (dict(start=(0, 0, 3, 0)), "start\\[2\\]"),
    (dict(start=(0, 0, 0)), "one state index per axis"),
    (dict(start="uniform"), "stationary"),
    (dict(kappa=float("inf")), "finite"),
    (dict(kappa=float("nan")), "finite"),
    (dict(return_paths=True, n_paths=1 << 20, n_periods=64), "2\\^25"),
    (dict(rtol=0.0), "rtol"),
])
def test_argument_checks(kw, match):
    a = _args(**kw)
    with pytest.raises(ValueError, match=match):
        S.simulate(a.pop("model"), a.pop("shapes"), a.pop("w_star"), a.pop("n_paths"), a.pop("n_periods"), **a)

"""
CPU tests of the claim series of the continuous-state simulation (``simulate_continuous`` with ``kappa``);
no device call is made here:

 (1) the exports; (2) every bad claim request raises before a device call; (3) ``smooth_v`` is positive on the six grids
 of tests/cont_sim_cases.py; (4) at κ = 1 with v = w − 1 the twin (tests/cont_sim_claim_oracle.py) gives rd = rc, xd = xc
 and pd = ln(ŵ − 1); (5) the rounding amplification A of rd, xd, pd on the GPU test cases: the largest
 ``close(fp64 twin, longdouble twin, 1.0)``.

Measured (5), κ = 2, v = ``smooth_v``, every grid with burn-in 0 and 7 and the zero and the vector start: A = 2.3e-15
(rd of gcy_2x3x2x3x4x3_sd1.0 from the vector start; xd 2.3e-15, pd 3.7e-16).  The three series carry no factor θ − 1, so
they amplify rounding far less than m (7.7e-14, tests/test_cont_simulation_cpu.py), which stays the A of the nine series
together.
"""
import numpy as np
import pytest

import sdfs_via_autodiff_amd as S
from sdfs_via_autodiff_amd import simulate_continuous, simulation, _lib

import cont_sim_cases as CC
import cont_sim_oracle as co
import cont_sim_claim_oracle as cc
from test_cont_simulation_cpu import twin_inputs, no_device

GRID_IDS = [CC.tag(*g) for g in CC.GRIDS]


# -- (1) ------------------------------------------------------------------------------------------------------------------
def test_exports():
    for name in ("sdfs_cont_sim_claim_records_dev", "sdfs_cont_sim_claim_paths_dev"):
        assert name in _lib.SYMBOLS
    for name in ("cont_sim_claim_records_dev", "cont_sim_claim_paths_dev"):
        assert callable(getattr(S.ContinuousOperator, name))
    assert cc.SERIES == simulation.SERIES_KAPPA


# -- (2) ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def request_case():
    m = S.SSY()
    grids = S.build_grid(m, 2, 3, 4, 5)
    return m, grids, np.full((2, 3, 4, 5), 700.0), cc.smooth_v(grids)


def bad_pd(v, how):
    v = v.copy()
    if how == "zero":
        v[1, 2, 0, 4] = 0.0
    elif how == "negative":
        v[0, 0, 0, 0] = -3.0
    elif how == "nan":
        v[1, 0, 3, 2] = np.nan
    elif how == "inf":
        v[1, 0, 3, 2] = np.inf
    elif how == "shape":
        v = v[:, :, :, :4]
    return v


@pytest.mark.parametrize("how,msg", [("zero", "pd must be positive"), ("negative", "pd must be positive"),
                                     ("nan", "pd must be finite"), ("inf", "pd must be finite"), ("shape", "pd has shape")])
def test_bad_pd_raises_before_any_device_call(monkeypatch, request_case, how, msg):
    no_device(monkeypatch)
    m, grids, w, v = request_case
    with pytest.raises(ValueError, match=msg):
        simulate_continuous(m, grids, w, 16, 8, kappa=2.0, pd=bad_pd(v, how))


def test_bad_claim_requests_raise_before_any_device_call(monkeypatch, request_case):
    no_device(monkeypatch)
    m, grids, w, v = request_case
    with pytest.raises(ValueError, match="needs kappa"):
        simulate_continuous(m, grids, w, 16, 8, pd=v)
    for kappa in (np.nan, np.inf, "two"):
        with pytest.raises(ValueError, match="kappa must be"):
            simulate_continuous(m, grids, w, 16, 8, kappa=kappa)
    for rtol in (0.0, -1e-3, np.nan):
        with pytest.raises(ValueError, match="rtol must be positive"):
            simulate_continuous(m, grids, w, 16, 8, kappa=1.0, rtol=rtol)
    # the established order: the counts before kappa, kappa before pd, pd before the start and the operator
    with pytest.raises(ValueError, match="n_paths"):
        simulate_continuous(m, grids, w, 0, 8, kappa=np.nan)
    with pytest.raises(ValueError, match="kappa must be"):
        simulate_continuous(m, grids, w, 16, 8, kappa=np.nan, pd=bad_pd(v, "zero"))
    with pytest.raises(ValueError, match="pd must be positive"):
        simulate_continuous(m, grids, w, 16, 8, kappa=2.0, pd=bad_pd(v, "zero"), start=np.zeros(3))
    with pytest.raises(ValueError, match="start has shape"):
        simulate_continuous(m, grids, w, 16, 8, kappa=2.0, pd=v, start=np.zeros(3), operator=object())


# -- (3) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS, ids=GRID_IDS)
def test_smooth_v_is_positive(kind, sizes, sd):
    v = cc.smooth_v(CC.grids_of(kind, sizes, sd))
    assert v.shape == tuple(sizes) and np.all(np.isfinite(v))
    assert v.min() >= 60.0 - 8.0 * len(sizes) >= 12.0


# -- (4) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS, ids=GRID_IDS)
def test_the_consumption_claim_is_the_twins_own_return(kind, sizes, sd):
    """κ = 1, v = w − 1: the interpolant of w − 1 is ŵ − 1 up to rounding, so rd = rc, xd = xc and pd = ln(ŵ − 1)."""
    par, grids, w, em = twin_inputs(kind, sizes, sd)
    tw = cc.simulate(kind, par, grids, w, em, w - 1.0, 1.0, seed=CC.SEED, path_offset=CC.PATH_OFFSET, n_paths=CC.P,
                     burn_in=7, n_periods=CC.T, start=CC.start_of(grids, "vector"))
    ser = tw["series"]
    assert tuple(ser) == cc.SERIES
    assert co.close(ser["rd"], ser["rc"], 1.0) <= 1e-13
    assert co.close(ser["xd"], ser["xc"], 1.0) <= 1e-13
    wh = co.interp_along(tw["state"], w, grids)
    assert co.close(ser["pd"], np.log(wh[:, 1:] - 1.0), 1.0) <= 1e-13
    # the base series are cont_sim_oracle's
    base = co.simulate(kind, par, grids, w, em, seed=CC.SEED, path_offset=CC.PATH_OFFSET, n_paths=CC.P, burn_in=7,
                       n_periods=CC.T, start=CC.start_of(grids, "vector"))
    for nm in co.SERIES:
        assert np.array_equal(ser[nm], base["series"][nm]), nm
    assert np.array_equal(tw["clamped"], base["clamped"])


# -- (5) ------------------------------------------------------------------------------------------------------------------
def test_rounding_amplification_of_the_claim_series():
    """A of rd, xd, pd over the cases of the GPU file's (1): see the figures at the top of this file."""
    A, worst = 0.0, None
    per = {}
    for kind, sizes, sd in CC.GRIDS:
        par, grids, w, em = twin_inputs(kind, sizes, sd)
        v = cc.smooth_v(grids)
        for burn_in in CC.BURN_INS:
            for start in CC.STARTS:
                kw = dict(seed=CC.SEED, path_offset=CC.PATH_OFFSET, n_paths=CC.P, burn_in=burn_in, n_periods=CC.T,
                          start=CC.start_of(grids, start))
                lo = cc.simulate(kind, par, grids, w, em, v, 2.0, dtype=np.float64, **kw)
                hi = cc.simulate(kind, par, grids, w, em, v, 2.0, dtype=np.longdouble, **kw)
                for nm in ("rd", "xd", "pd"):
                    e = co.close(lo["series"][nm], hi["series"][nm], 1.0)
                    per[nm] = max(per.get(nm, 0.0), e)
                    if e > A:
                        A, worst = e, (CC.tag(kind, sizes, sd), burn_in, start, nm)
    print(f"rounding amplification of the claim series: A = {A:.3e} at {worst}; per series "
          + ", ".join(f"{nm} {e:.3e}" for nm, e in per.items()))
    assert A <= 1e-9

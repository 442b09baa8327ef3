"""
GPU tests of the continuous-state simulation (csrc/cont_sim.hpp, the C_EM form of csrc/cont_kernel.hpp,
sdfs_via_autodiff_amd/simulation.py ``simulate_continuous``) on the cases of tests/cont_sim_cases.py:

 (1) E_x[M] against the numpy twin (tests/cont_sim_oracle.py), quadrature and Monte Carlo, and against the closed form
     at a constant w, to the RTOL of tests/test_hip_continuous.py;
 (2) states, series and statistics against the twin; (3) the interpolated series against ``lin_interp`` at the device's
 own states; (4) a start far outside the grid; (5) purity: rerun, split by path_offset, continuation by step_offset;
 (6) the distribution of the simulated states; (7) mid-size grids; (8) the refusals.

BOUND.  States and series are compared by ``close(device, twin, 1.0)``.  The fp64 twin and the device differ by libm
(log, exp, sin, cos, sqrt: a few ulp per call) and by the fused multiply-adds of the device's interpolation.  On the
cases of (2) the twin's own sensitivity to such rounding is A = 7.7e-14 (tests/test_cont_simulation_cpu.py: fp64 against
longdouble twin) and the worst device-vs-twin value measured on the MI355X is 9.9e-14 (m on the GCY grids; 6.1e-14 on
the SSY grids; states 8.9e-16).  BOUND = 32 max(A, measured) = 3.2e-12, rounded up to a power of ten: 1e-11.

The far-outside start of (4) is held to the same bound.  There the twins themselves are 1.7e-10 apart on the GCY 3.2 grid
(2.5e-11 on the SSY 3.2 grids; the decaying z keeps the absolute rounding error of its first, large steps), which by
the same rule would ask for 1e-8, more than the 1e-9 such a bound may be; the device is 7.4e-12 from the fp64 twin there
(4.6e-13 on the SSY 3.2 grids, below 1e-13 on the 1.0 grids), inside 1e-11 with a margin of 1.35.

One case departs from "w* is a Newton fixed point": GCY 2x3x2x3x4x3 at num_std_devs = 3.2 has none (cont_sim_cases.py),
the solve is asserted to diverge and the case runs at a smooth synthetic w.
"""
import signal

import numpy as np
import pytest

import cont_sim_cases as CC
import cont_sim_oracle as co
import sim_oracle as so
from test_hip_continuous import RTOL
from test_hip_simulation import rel_err

pytestmark = pytest.mark.gpu

BOUND = 1e-11


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


@pytest.fixture(autouse=True)
def time_limit():
    def expire(signum, frame):
        raise TimeoutError("test exceeded its 120 s limit")
    old = signal.signal(signal.SIGALRM, expire)
    signal.alarm(120)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def model_of(S, kind):
    return S.SSY() if kind == "ssy" else S.GCY()


def quad_operator(S, kind, grids, d):
    nodes, weights = S.qnwnorm([d] * len(grids))
    return S.ContinuousOperator(np.array(model_of(S, kind).params), grids, np.ascontiguousarray(nodes.T), weights)


def newton_fixed_point(op, w0):
    """Successive approximation into Newton's basin, as the reference's drivers do, then a tight Newton solve."""
    xs, _, _ = op.solve(w0, "successive_approx", tol=1e-2, max_iter=50000)
    x, _, info = op.solve(xs, "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
    assert info["status"] == 0, info
    assert np.all(x > 1.0) and np.max(np.abs(op(x) - x)) < 1e-8
    return x


_FP = {}


def _lib_numeric(S):
    from sdfs_via_autodiff_amd import _lib
    return _lib.SDFS_ERR_NUMERIC


def fixed_point(S, kind, sizes, sd):
    """(model, params, grids, operator (Gauss–Hermite d = 3), w*, the twin's E_x[M] at w*), cached per grid.  Where the
    grid has no fixed point (cont_sim_cases.NO_FIXED_POINT) w is ``smooth_w``."""
    key = CC.tag(kind, sizes, sd)
    if key not in _FP:
        grids = CC.grids_of(kind, sizes, sd)
        for a, b in zip(grids, S.build_grid(model_of(S, kind), *sizes, num_std_devs=sd)):
            assert np.array_equal(a, b)
        op = quad_operator(S, kind, grids, CC.QUAD_D)
        if (kind, sizes, sd) in CC.NO_FIXED_POINT:
            _, _, info = op.solve(np.ones(sizes), "successive_approx", tol=1e-2, max_iter=50000)
            assert info["status"] == _lib_numeric(S) and not np.isfinite(info["final_err"]), info   # it does diverge
            w = CC.smooth_w(grids)
        else:
            w = newton_fixed_point(op, np.ones(sizes))
            np.testing.assert_allclose(w, CC.golden_wstar(kind, sizes, sd), rtol=0, atol=1e-7)   # what the CPU file runs at
        par = CC.params_of(kind)
        em = co.sdf_mean(kind, par, grids, w, op.nodes, op.weights)
        _FP[key] = (model_of(S, kind), par, grids, op, w, em)
    return _FP[key]


def device_sdf_mean(op, w):
    import torch
    wd = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(torch.device("cuda", op.device))
    em = torch.empty_like(wd)
    torch.cuda.synchronize()
    op.cont_sdf_mean_dev(wd.data_ptr(), em.data_ptr())
    op.synchronize()
    return em.cpu().numpy()


def device_records(op, w, em):
    """The records {w, −ln E_M} (grid shape + (2,)) sdfs_cont_sim_records_dev writes."""
    import torch
    dev = torch.device("cuda", op.device)
    wd = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(dev)
    ed = torch.from_numpy(np.ascontiguousarray(em, dtype=np.float64)).to(dev)
    rec = torch.empty(tuple(w.shape) + (2,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    op.cont_sim_records_dev(wd.data_ptr(), ed.data_ptr(), rec.data_ptr())
    op.synchronize()
    return rec.cpu().numpy()


GRID_IDS = [CC.tag(*g) for g in CC.GRIDS]


# -- (1) E_x[M] -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS, ids=GRID_IDS)
def test_sdf_mean_matches_the_twin(S, kind, sizes, sd):
    m, par, grids, op, w, em = fixed_point(S, kind, sizes, sd)
    got = device_sdf_mean(op, w)
    print(f"E_M quadrature: max rel {np.max(np.abs(got / em - 1)):.3e}")
    np.testing.assert_allclose(got, em, rtol=RTOL)
    draws = np.random.default_rng(11).standard_normal((len(grids), 64))
    mc = S.ContinuousOperator(np.array(m.params), grids, draws, None)
    got = device_sdf_mean(mc, w)
    want = co.sdf_mean(kind, par, grids, w, draws, None)
    print(f"E_M Monte Carlo: max rel {np.max(np.abs(got / want - 1)):.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL)
    # w <= 1 at one point: NaN there (its own value enters as (w - 1)^(1 - theta)), finite elsewhere around it
    bad = w.copy()
    bad.flat[5] = 1.0
    assert np.isnan(device_sdf_mean(op, bad).flat[5])


@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS[1::2], ids=GRID_IDS[1::2])
def test_sdf_mean_of_a_constant_w_is_the_closed_form(S, kind, sizes, sd):
    grids = CC.grids_of(kind, sizes, sd)
    op = quad_operator(S, kind, grids, 5)
    got = device_sdf_mean(op, np.full(sizes, 650.0))
    want = co.sdf_mean_constant_w(kind, CC.params_of(kind), grids, 650.0)
    print(f"E_M constant w: max rel {np.max(np.abs(got / want - 1)):.3e}")
    np.testing.assert_allclose(got, want, rtol=RTOL)


# -- (2) against the twin ---------------------------------------------------------------------------------------------------
def run_pair(S, kind, sizes, sd, burn_in, start):
    m, par, grids, op, w, em = fixed_point(S, kind, sizes, sd)
    st = CC.start_of(grids, start)
    out = S.simulate_continuous(m, grids, w, CC.P, CC.T, burn_in=burn_in, seed=CC.SEED, path_offset=CC.PATH_OFFSET,
                                start=st, operator=op, return_paths=True)
    tw = co.simulate(kind, par, grids, w, em, seed=CC.SEED, path_offset=CC.PATH_OFFSET, n_paths=CC.P, burn_in=burn_in,
                     n_periods=CC.T, start=st)
    return grids, w, out, tw


def check_against_twin(S, grids, w, out, tw):
    """States, series, statistics and clamped counts of a device run against the twin's; returns the largest measured
    device-vs-twin value of the states and of the series."""
    got = out["paths"]
    D = len(grids)
    assert out["series"] == co.SERIES
    assert got["state"].shape == (CC.P, CC.T + 1, D) and got["state"].dtype == np.float64
    worst = {"state": co.close(got["state"], tw["state"], 1.0), "series": 0.0}
    for nm in co.SERIES:
        assert got[nm].shape == (CC.P, CC.T)
        worst["series"] = max(worst["series"], co.close(got[nm], tw["series"][nm], 1.0))
    print(f"device vs twin: states {worst['state']:.3e}, series {worst['series']:.3e}")
    assert worst["state"] <= BOUND, worst
    for nm in co.SERIES:
        assert co.close(got[nm], tw["series"][nm], 1.0) <= BOUND, (nm, co.close(got[nm], tw["series"][nm], 1.0))
    # statistics: the one-pass sums against the two-pass formulas on the device's own series (test_hip_simulation.py's
    # bound and floors)
    for nm in co.SERIES:
        mean, sd_, ac1 = so.two_pass(got[nm])
        pp = out["per_path"][nm]
        floor_mean = 1e-3 * np.max(np.abs(got[nm]), axis=1)
        for a, b, floor, what in ((pp["mean"], mean, floor_mean, "mean"), (pp["std"], sd_, 0.0, "std"),
                                  (pp["ac1"], ac1, 1e-2, "ac1")):
            assert rel_err(a, b, floor) <= 1e-10, (nm, what, rel_err(a, b, floor))
    # ... the slope's regressor ln(ŵ(x_{t−1}) − 1) from lin_interp at the device's own states
    prv = np.ascontiguousarray(got["state"][:, :-1, :].reshape(-1, D).T)
    xr = np.log(S.lin_interp(prv, w, grids).reshape(CC.P, CC.T) - 1.0)
    assert rel_err(out["per_path"]["slope"], so.ols_slope(xr, got["xc"]), 1e-2) <= 1e-10
    # clamped: the twin's count, except at steps whose state lies within 1e-12 of an edge
    dev = np.rint(out["clamped"]["per_path"] * CC.T).astype(np.int64)
    sure = (tw["outside"] & ~tw["near_edge"]).sum(axis=1)
    maybe = tw["near_edge"].sum(axis=1)
    assert np.all(dev >= sure) and np.all(dev <= sure + maybe), int(np.sum((dev < sure) | (dev > sure + maybe)))
    assert np.array_equal(out["final_state"], got["state"][:, -1, :])
    assert set(out["clamped"]["summary"]) == {"mean", "median", "p05", "p95"}
    return worst


@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("start", CC.STARTS)
@pytest.mark.parametrize("burn_in", CC.BURN_INS)
def test_states_series_and_statistics_match_the_twin(S, kind, sizes, sd, burn_in, start):
    grids, w, out, tw = run_pair(S, kind, sizes, sd, burn_in, start)
    check_against_twin(S, grids, w, out, tw)


@pytest.mark.parametrize("kind,sizes,sd", [CC.GRIDS[0], CC.GRIDS[5]], ids=[GRID_IDS[0], GRID_IDS[5]])
@pytest.mark.parametrize("n_periods", [2, 3, 9])
def test_every_lookahead_and_group_gives_the_default_forms_bits(S, kind, sizes, sd, n_periods):
    """sdfs_cont_sim_paths_dev with look-ahead 1, 2, 4 and groups of 4, 8 and (6-D, look-ahead <= 2) 16 corners, at 300
    paths (a partial block) and runs shorter than, as long as and no multiple of the look-ahead.  These forms store no
    path; cont_sim.hpp promises that the copies of a step round alike, so their statistics, clamped counts and final
    states are the default form's bit for bit.  The default form, which stores, is held against the twin with the bound
    of the test above (states and series), and its statistics against the two-pass values of its own series (1e-10)."""
    import torch
    m, par, grids, op, w, em = fixed_point(S, kind, sizes, sd)
    Pn, Bn, D = 300, 3, len(grids)
    st0 = CC.start_of(grids, "vector")
    kw = dict(burn_in=Bn, seed=CC.SEED, path_offset=CC.PATH_OFFSET, start=st0)
    out = S.simulate_continuous(m, grids, w, Pn, n_periods, operator=op, return_paths=True, **kw)
    tw = co.simulate(kind, par, grids, w, em, n_paths=Pn, n_periods=n_periods, **kw)
    worst = {"state": co.close(out["paths"]["state"], tw["state"], 1.0),
             "series": max(co.close(out["paths"][nm], tw["series"][nm], 1.0) for nm in co.SERIES)}
    print(f"device vs twin: states {worst['state']:.3e}, series {worst['series']:.3e}")
    assert worst["state"] <= BOUND and worst["series"] <= BOUND, worst
    for nm in co.SERIES:
        mean, sd_, ac1 = so.two_pass(out["paths"][nm])
        pp = out["per_path"][nm]
        floor_mean = 1e-3 * np.max(np.abs(out["paths"][nm]), axis=1)
        for a, b, floor in ((pp["mean"], mean, floor_mean), (pp["std"], sd_, 0.0), (pp["ac1"], ac1, 1e-2)):
            assert rel_err(a, b, floor) <= 1e-10, nm
    # ... and the slope against the two-pass OLS value at the device's own states (check_against_twin's bound and floor)
    prv = np.ascontiguousarray(out["paths"]["state"][:, :-1, :].reshape(-1, D).T)
    xr = np.log(S.lin_interp(prv, w, grids).reshape(Pn, n_periods) - 1.0)
    slope = rel_err(out["per_path"]["slope"], so.ols_slope(xr, out["paths"]["xc"]), 1e-2)
    print(f"slope vs two-pass OLS: {slope:.3e}")
    assert slope <= 1e-10, slope
    default = np.stack([out["per_path"][nm][s] for nm in co.SERIES for s in ("mean", "std", "ac1")] + [out["per_path"]["slope"]])
    dev = torch.device("cuda", op.device)
    wd = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(dev)
    ed = torch.empty_like(wd)
    rec = torch.empty((wd.numel(), 2), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    op.cont_sdf_mean_dev(wd.data_ptr(), ed.data_ptr())
    op.cont_sim_records_dev(wd.data_ptr(), ed.data_ptr(), rec.data_ptr())
    forms = [(k, g) for k in (1, 2, 4) for g in (4, 8)] + ([(1, 16), (2, 16)] if D == 6 else [])
    for k, g in forms:
        st = torch.full((19, Pn), -7.0, dtype=torch.float64, device=dev)
        cl = torch.full((Pn,), -7, dtype=torch.int32, device=dev)
        fin = torch.full((Pn, D), -7.0, dtype=torch.float64, device=dev)
        op.cont_sim_paths_dev(rec.data_ptr(), CC.SEED, CC.PATH_OFFSET, Pn, Bn, n_periods, st.data_ptr(), cl.data_ptr(), fin.data_ptr(),
                              start=st0, lookahead=k, group=g)
        op.synchronize()
        assert np.array_equal(st.cpu().numpy(), default, equal_nan=True), (k, g)
        assert np.array_equal(cl.cpu().numpy() / n_periods, out["clamped"]["per_path"]), (k, g)
        assert np.array_equal(fin.cpu().numpy(), out["final_state"]), (k, g)


# -- (3) interpolation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS, ids=GRID_IDS)
def test_series_are_lin_interp_at_the_device_states(S, kind, sizes, sd):
    grids, w, out, _ = run_pair(S, kind, sizes, sd, 7, "vector")
    st = out["paths"]["state"]
    D = len(grids)
    nxt = np.ascontiguousarray(st[:, 1:, :].reshape(-1, D).T)
    prv = np.ascontiguousarray(st[:, :-1, :].reshape(-1, D).T)
    np.testing.assert_allclose(out["paths"]["wc"].ravel(), S.lin_interp(nxt, w, grids), rtol=1e-13)
    # rf interpolates the record field −ln E_M as the device formed it: on the 3.2 grids that field changes sign, and
    # an interpolant near zero of the host's −ln E_M (one ulp of a corner away) is 1e-10 relative from the device's
    m, par, _, op, _, _ = fixed_point(S, kind, sizes, sd)
    rec = device_records(op, w, out["E_M"])
    assert np.array_equal(rec[..., 0], w)
    np.testing.assert_allclose(rec[..., 1], -np.log(out["E_M"]), rtol=1e-14)
    np.testing.assert_allclose(out["paths"]["rf"].ravel(), S.lin_interp(prv, rec[..., 1], grids), rtol=1e-13)


# -- (4) far outside --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS, ids=GRID_IDS)
def test_start_far_outside_the_grid(S, kind, sizes, sd):
    grids, w, out, tw = run_pair(S, kind, sizes, sd, 0, "far")
    for nm in co.SERIES:
        assert np.all(np.isfinite(out["paths"][nm])), nm
        for s in ("mean", "std"):
            assert np.all(np.isfinite(out["per_path"][nm][s])), (nm, s)
    assert np.all(np.isfinite(out["paths"]["state"])) and np.all(np.isfinite(out["final_state"]))
    outside, _ = co.outside(grids, out["paths"]["state"])
    assert np.all(outside[:, :4])                              # x_0 and the first steps: every path outside
    assert np.all(out["clamped"]["per_path"] >= 3.0 / CC.T)
    check_against_twin(S, grids, w, out, tw)


# -- (5) purity -------------------------------------------------------------------------------------------------------------
def same(a, b):
    for nm in co.SERIES:
        for s in ("mean", "std", "ac1"):
            assert np.array_equal(a["per_path"][nm][s], b["per_path"][nm][s], equal_nan=True), (nm, s)
        assert np.array_equal(a["paths"][nm], b["paths"][nm]), nm
    assert np.array_equal(a["per_path"]["slope"], b["per_path"]["slope"], equal_nan=True)
    assert np.array_equal(a["paths"]["state"], b["paths"]["state"])
    assert np.array_equal(a["clamped"]["per_path"], b["clamped"]["per_path"])
    assert np.array_equal(a["final_state"], b["final_state"])


def joined(a, b):
    out = {"per_path": {nm: {s: np.concatenate([a["per_path"][nm][s], b["per_path"][nm][s]]) for s in ("mean", "std", "ac1")}
                        for nm in co.SERIES},
           "paths": {nm: np.concatenate([a["paths"][nm], b["paths"][nm]]) for nm in co.SERIES + ("state",)},
           "clamped": {"per_path": np.concatenate([a["clamped"]["per_path"], b["clamped"]["per_path"]])},
           "final_state": np.concatenate([a["final_state"], b["final_state"]])}
    out["per_path"]["slope"] = np.concatenate([a["per_path"]["slope"], b["per_path"]["slope"]])
    return out


@pytest.mark.parametrize("kind,sizes,sd", [CC.GRIDS[0], CC.GRIDS[5]], ids=[GRID_IDS[0], GRID_IDS[5]])
def test_rerun_split_and_continuation_are_bit_identical(S, kind, sizes, sd):
    m, par, grids, op, w, em = fixed_point(S, kind, sizes, sd)
    kw = dict(burn_in=5, seed=77, operator=op, return_paths=True, start=CC.start_of(grids, "vector"))
    full = S.simulate_continuous(m, grids, w, 3000, 100, **kw)
    same(full, S.simulate_continuous(m, grids, w, 3000, 100, **kw))
    a = S.simulate_continuous(m, grids, w, 1100, 100, path_offset=0, **kw)
    b = S.simulate_continuous(m, grids, w, 1900, 100, path_offset=1100, **kw)
    same(full, joined(a, b))
    # 100 steps = 40 steps, then 60 from where they ended with the step numbers carried on
    first = S.simulate_continuous(m, grids, w, 3000, 40, **kw)
    rest = S.simulate_continuous(m, grids, w, 3000, 60, **dict(kw, burn_in=0, start=first["final_state"], step_offset=45))
    assert np.array_equal(full["paths"]["state"][:, :41], first["paths"]["state"])
    assert np.array_equal(full["paths"]["state"][:, 40:], rest["paths"]["state"])
    for nm in co.SERIES:
        assert np.array_equal(full["paths"][nm], np.concatenate([first["paths"][nm], rest["paths"][nm]], axis=1)), nm
    assert np.array_equal(full["final_state"], rest["final_state"])
    other = S.simulate_continuous(m, grids, w, 3000, 100, **dict(kw, seed=78))
    assert not np.array_equal(other["paths"]["state"], full["paths"]["state"])
    assert not np.array_equal(other["per_path"]["dc"]["mean"], full["per_path"]["dc"]["mean"])


# -- (6) distribution -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,sd", [CC.GRIDS[3], CC.GRIDS[5]], ids=[GRID_IDS[3], GRID_IDS[5]])
def test_distribution_of_the_simulated_states(S, kind, sizes, sd):
    m, par, grids, op, w, em = fixed_point(S, kind, sizes, sd)
    P, T = 1 << 16, 32
    out = S.simulate_continuous(m, grids, w, P, T, seed=2024, operator=op, return_paths=True)
    st = out["paths"]["state"]
    rho_l, s_l = co.pieces(kind, par)[7:9]
    rho_c, s_c = (par[8], par[11]) if kind == "ssy" else (par[10], par[11])
    h = st[:, -1, 0]
    var = s_l ** 2 * (1 - rho_l ** (2 * T)) / (1 - rho_l ** 2)
    assert abs(h.mean()) <= 5.0 * np.sqrt(var / P), (h.mean(), var)
    assert abs(h.var(ddof=1) - var) <= 5.0 * np.sqrt(2.0 * var ** 2 / (P - 1)), (h.var(ddof=1), var)
    e_l = (st[:, 1:, 0] - rho_l * st[:, :-1, 0]) / s_l
    e_c = (st[:, 1:, 1] - rho_c * st[:, :-1, 1]) / s_c
    corr = np.corrcoef(e_l.ravel(), e_c.ravel())[0, 1]
    assert abs(corr) <= 5.0 / np.sqrt(P * T), corr
    assert abs(e_l.std() - 1.0) < 0.01 and abs(e_c.std() - 1.0) < 0.01


# -- (7) mid-size grids -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes", [("ssy", (10, 10, 10, 20)), ("gcy", (6, 6, 6, 6, 8, 8))], ids=["ssy", "gcy"])
def test_mid_size_grids(S, kind, sizes):
    m = model_of(S, kind)
    grids = S.build_grid(m, *sizes)
    op = quad_operator(S, kind, grids, 3)
    w = newton_fixed_point(op, np.ones(sizes)) if kind == "ssy" else CC.smooth_w(grids)
    a = S.simulate_continuous(m, grids, w, 5000, 64, burn_in=16, seed=5, operator=op)
    b = S.simulate_continuous(m, grids, w, 5000, 64, burn_in=16, seed=5, operator=op)
    for nm in a["series"]:
        for s in ("mean", "std", "ac1"):
            assert np.all(np.isfinite(a["per_path"][nm][s])), (nm, s)
            assert np.array_equal(a["per_path"][nm][s], b["per_path"][nm][s]), (nm, s)
    assert np.all(np.isfinite(a["per_path"]["slope"])) and np.array_equal(a["per_path"]["slope"], b["per_path"]["slope"])
    assert np.array_equal(a["final_state"], b["final_state"]) and a["E_M"].shape == tuple(sizes)
    assert set(a["clamped"]["summary"]) == {"mean", "median", "p05", "p95"} and "paths" not in a
    assert 0.0 <= a["clamped"]["summary"]["mean"] < 0.2


# -- (8) refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(S):
    import ctypes as C
    import torch
    from sdfs_via_autodiff_amd import _lib
    ssy = S.SSY()
    shapes = (3, 3, 3, 4)
    disc = S.ssy_operator(shapes, ssy.params, S.discretize_ssy(ssy, shapes))
    dense = S.DenseOperator(S.compute_H_single_index(ssy, (2, 2, 2, 3)), ssy.params[0], ssy.θ)
    for op, n in ((disc, 108), (dense, 24)):
        wd = torch.full((n,), 700.0, dtype=torch.float64, device="cuda")
        em = torch.empty_like(wd)
        rec = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        st = torch.empty((19, 4), dtype=torch.float64, device="cuda")
        cl = torch.empty((4,), dtype=torch.int32, device="cuda")
        fs = torch.empty((4, 4), dtype=torch.float64, device="cuda")
        d = _lib.sdfs_cont_sim_desc()
        d.n_paths, d.n_periods = 4, 8
        h = op._h
        assert _lib.lib.sdfs_cont_sdf_mean_dev(h, wd.data_ptr(), em.data_ptr()) == _lib.SDFS_ERR_UNSUPPORTED
        assert _lib.lib.sdfs_cont_sim_records_dev(h, wd.data_ptr(), em.data_ptr(), rec.data_ptr()) == _lib.SDFS_ERR_UNSUPPORTED
        assert _lib.lib.sdfs_cont_sim_paths_dev(h, rec.data_ptr(), C.byref(d), st.data_ptr(), cl.data_ptr(), fs.data_ptr(),
                                                None, None) == _lib.SDFS_ERR_UNSUPPORTED
    m, par, grids, op, w, em = fixed_point(S, *CC.GRIDS[1])
    bad = w.copy()
    bad[1, 2, 0, 4] = 0.5
    with pytest.raises(ValueError, match="exceed 1"):
        S.simulate_continuous(m, grids, bad, 16, 8, operator=op)
    # the C layer's own request checks
    d = _lib.sdfs_cont_sim_desc()
    d.n_paths, d.n_periods, d.lookahead = 4, 8, 3
    rec = torch.ones((w.size, 2), dtype=torch.float64, device="cuda")
    st = torch.empty((19, 4), dtype=torch.float64, device="cuda")
    cl = torch.empty((4,), dtype=torch.int32, device="cuda")
    fs = torch.empty((4, 4), dtype=torch.float64, device="cuda")
    call = lambda: _lib.lib.sdfs_cont_sim_paths_dev(op._h, rec.data_ptr(), C.byref(d), st.data_ptr(), cl.data_ptr(),
                                                    fs.data_ptr(), None, None)
    assert call() == _lib.SDFS_ERR_ARG
    d.lookahead, d.group = 4, 16
    assert call() == _lib.SDFS_ERR_ARG
    d.group, d.step_offset = 0, (1 << 32) - 8
    assert call() == _lib.SDFS_ERR_ARG

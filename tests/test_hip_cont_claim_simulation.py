"""
GPU tests of the claim series rd, xd, pd of the continuous-state simulation (k_cont_sim_claim_paths of csrc/cont_sim.hpp,
``simulate_continuous(..., kappa=, pd=)``) on the cases of tests/cont_sim_cases.py:

 (1) states, the nine series, the 28 statistics, slope, clamped counts and final state against the numpy twin
     (tests/cont_sim_claim_oracle.py) with ``pd = smooth_v`` and κ = 2; (2) the six base series of a claim run are those of
     the plain run, bit for bit; (3) pd is ``log(lin_interp(state, v))`` at the device's own states; (4) the solved v;
 (5) the refusals; (6) purity: rerun, split by path_offset, continuation by step_offset; (7) both group sizes give the
 default's bits; (8) mid-size grids.

BOUND.  The rule of tests/test_hip_cont_simulation.py: states and series are compared by ``close(device, twin, 1.0)``, and
the bound is 32 max(A, measured), rounded up to a power of ten and never above 1e-9.  The rounding amplification of the
nine series is A = 7.7e-14 (m; tests/test_cont_simulation_cpu.py); that of rd, xd, pd alone is 2.3e-15
(tests/test_cont_claim_simulation_cpu.py).  The worst device-vs-twin value measured on the MI355X over the 24 cases of (1)
is 9.9e-14 (m on the GCY grids, as without a claim; rd 3.0e-15, xd 5.2e-15, pd 4.4e-16, states 8.9e-16).
BOUND = 32 max(7.7e-14, 9.9e-14) = 3.2e-12, rounded up to a power of ten: 1e-11, the bound of the plain simulation's file.

(4) at κ = 1: the solved v was 4.7e-12 … 1.5e-11 (relative) from w* − 1 on the five grids with a fixed point, and rd was
1.0e-13 … 2.8e-13 from rc, inside the 1.3e-11 of DESIGN §4.15 plus BOUND that the test allows.
"""
import ctypes as C
import signal

import numpy as np
import pytest

import cont_sim_cases as CC
import cont_sim_oracle as co
import cont_sim_claim_oracle as cc
import sim_oracle as so
from test_hip_cont_simulation import fixed_point, model_of, quad_operator, newton_fixed_point
from test_hip_simulation import rel_err

pytestmark = pytest.mark.gpu

BOUND = 1e-11
KAPPA = 2.0
GRID_IDS = [CC.tag(*g) for g in CC.GRIDS]


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


_RUN = {}


def run_pair(S, kind, sizes, sd, burn_in, start):
    """(grids, w, v, device result, twin) of one case with pd = smooth_v and κ = 2, computed once."""
    key = (CC.tag(kind, sizes, sd), burn_in, start)
    if key not in _RUN:
        m, par, grids, op, w, em = fixed_point(S, kind, sizes, sd)
        v = cc.smooth_v(grids)
        st = CC.start_of(grids, start)
        out = S.simulate_continuous(m, grids, w, CC.P, CC.T, burn_in=burn_in, seed=CC.SEED, path_offset=CC.PATH_OFFSET,
                                    start=st, operator=op, return_paths=True, kappa=KAPPA, pd=v)
        tw = cc.simulate(kind, par, grids, w, em, v, KAPPA, seed=CC.SEED, path_offset=CC.PATH_OFFSET, n_paths=CC.P,
                         burn_in=burn_in, n_periods=CC.T, start=st)
        _RUN[key] = (grids, w, v, out, tw)
    return _RUN[key]


def check_statistics(S, grids, v, out, P, T):
    """The 28 statistics against the two-pass values of the device's own series (1e-10, the floors of
    tests/test_hip_simulation.py), the slope against the two-pass OLS of xd on ln v̂(x_{t−1}) from lin_interp."""
    got = out["paths"]
    D = len(grids)
    for nm in cc.SERIES:
        mean, sd_, ac1 = so.two_pass(got[nm])
        pp = out["per_path"][nm]
        floor_mean = 1e-3 * np.max(np.abs(got[nm]), axis=1)
        for a, b, floor, what in ((pp["mean"], mean, floor_mean, "mean"), (pp["std"], sd_, 0.0, "std"),
                                  (pp["ac1"], ac1, 1e-2, "ac1")):
            assert rel_err(a, b, floor) <= 1e-10, (nm, what, rel_err(a, b, floor))
    prv = np.ascontiguousarray(got["state"][:, :-1, :].reshape(-1, D).T)
    xr = np.log(S.lin_interp(prv, v, grids).reshape(P, T))
    slope = rel_err(out["per_path"]["slope"], so.ols_slope(xr, got["xd"]), 1e-2)
    print(f"slope vs two-pass OLS: {slope:.3e}")
    assert slope <= 1e-10, slope


# -- (1) against the twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("start", CC.STARTS)
@pytest.mark.parametrize("burn_in", CC.BURN_INS)
def test_states_series_and_statistics_match_the_twin(S, kind, sizes, sd, burn_in, start):
    grids, w, v, out, tw = run_pair(S, kind, sizes, sd, burn_in, start)
    got = out["paths"]
    D = len(grids)
    assert out["series"] == cc.SERIES and set(out["per_path"]) == set(cc.SERIES) | {"slope"}
    assert np.array_equal(out["pd"], v)
    assert got["state"].shape == (CC.P, CC.T + 1, D) and got["state"].dtype == np.float64
    worst = {nm: co.close(got[nm], tw["series"][nm], 1.0) for nm in cc.SERIES}
    worst["state"] = co.close(got["state"], tw["state"], 1.0)
    print("device vs twin: " + ", ".join(f"{nm} {e:.3e}" for nm, e in worst.items()))
    for nm in cc.SERIES:
        assert got[nm].shape == (CC.P, CC.T)
    for nm, e in worst.items():
        assert e <= BOUND, (nm, e)
    check_statistics(S, grids, v, out, CC.P, CC.T)
    for nm in cc.SERIES:                       # ... and the twin's own statistics, as far as the series agree
        for s in ("mean", "std"):
            assert rel_err(out["per_path"][nm][s], tw["stats"][nm][s], 1e-3 * np.max(np.abs(got[nm]))) <= 1e-8, (nm, s)
    dev = np.rint(out["clamped"]["per_path"] * CC.T).astype(np.int64)
    sure = (tw["outside"] & ~tw["near_edge"]).sum(axis=1)
    maybe = tw["near_edge"].sum(axis=1)
    assert np.all(dev >= sure) and np.all(dev <= sure + maybe), int(np.sum((dev < sure) | (dev > sure + maybe)))
    assert np.array_equal(out["final_state"], got["state"][:, -1, :])
    assert co.close(out["final_state"], tw["final_state"], 1.0) <= BOUND


# -- (2) the base series ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS, ids=GRID_IDS)
def test_base_series_are_the_plain_runs_bit_for_bit(S, kind, sizes, sd):
    grids, w, v, out, _ = run_pair(S, kind, sizes, sd, 7, "vector")
    m, par, _, op, _, _ = fixed_point(S, kind, sizes, sd)
    plain = S.simulate_continuous(m, grids, w, CC.P, CC.T, burn_in=7, seed=CC.SEED, path_offset=CC.PATH_OFFSET,
                                  start=CC.start_of(grids, "vector"), operator=op, return_paths=True)
    assert plain["series"] == co.SERIES and "pd" not in plain
    for nm in co.SERIES:
        assert np.array_equal(out["paths"][nm], plain["paths"][nm]), nm
        for s in ("mean", "std", "ac1"):
            assert np.array_equal(out["per_path"][nm][s], plain["per_path"][nm][s], equal_nan=True), (nm, s)
    assert np.array_equal(out["paths"]["state"], plain["paths"]["state"])
    assert np.array_equal(out["clamped"]["per_path"], plain["clamped"]["per_path"])
    assert np.array_equal(out["final_state"], plain["final_state"])
    assert np.array_equal(out["E_M"], plain["E_M"])


# -- (3) interpolation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS, ids=GRID_IDS)
def test_pd_is_lin_interp_at_the_device_states(S, kind, sizes, sd):
    grids, w, v, out, _ = run_pair(S, kind, sizes, sd, 7, "vector")
    st = out["paths"]["state"]
    D = len(grids)
    nxt = np.ascontiguousarray(st[:, 1:, :].reshape(-1, D).T)
    np.testing.assert_allclose(out["paths"]["pd"].ravel(), np.log(S.lin_interp(nxt, v, grids)), rtol=1e-13)
    np.testing.assert_allclose(out["paths"]["wc"].ravel(), S.lin_interp(nxt, w, grids), rtol=1e-13)


# -- (4) the solved v -------------------------------------------------------------------------------------------------------
# the (grid, κ) pairs for which DESIGN §4.15 records r(K) < 0.9998
SOLVED = [(g, 1.0) for g in CC.GRIDS if g not in CC.NO_FIXED_POINT] + \
         [(g, 2.0) for g in CC.GRIDS if g[0] == "ssy" and g[2] == 3.2] + [(g, 0.0) for g in CC.GRIDS if g[2] == 1.0]


@pytest.mark.parametrize("grid,kappa", SOLVED, ids=[f"{CC.tag(*g)}-k{k:g}" for g, k in SOLVED])
def test_solved_v_is_claim_prices_continuous(S, grid, kappa):
    kind, sizes, sd = grid
    m, par, grids, op, w, em = fixed_point(S, kind, sizes, sd)
    out = S.simulate_continuous(m, grids, w, CC.P, CC.T, burn_in=7, seed=CC.SEED, path_offset=CC.PATH_OFFSET,
                                start=CC.start_of(grids, "vector"), operator=op, return_paths=True, kappa=kappa)
    want = S.claim_prices_continuous(m, grids, w, kappa, operator=op)["pd"]
    assert out["series"] == cc.SERIES and np.array_equal(out["pd"], want)
    for nm in cc.SERIES:
        assert np.all(np.isfinite(out["paths"][nm])), nm
    check_statistics(S, grids, out["pd"], out, CC.P, CC.T)
    if kappa == 1.0:
        # the consumption claim: v = w* − 1 up to the solve, so rd is rc up to that distance (§4.15: 3.1e-12 … 1.3e-11)
        dist = float(np.max(np.abs(out["pd"] / (w - 1.0) - 1.0)))
        err = co.close(out["paths"]["rd"], out["paths"]["rc"], 1.0)
        print(f"v against w* − 1: {dist:.3e} relative; rd against rc: {err:.3e}")
        assert err <= 1.3e-11 + BOUND, err
        assert co.close(out["paths"]["xd"], out["paths"]["xc"], 1.0) <= 1.3e-11 + BOUND


# -- (5) refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(S):
    import torch
    from sdfs_via_autodiff_amd import _lib
    lib = _lib.lib
    m, par, grids, op, w, em = fixed_point(S, *CC.GRIDS[1])
    v = cc.smooth_v(grids)
    with pytest.raises(ValueError, match="no finite price"):
        S.simulate_continuous(m, grids, w, 16, 8, operator=op, kappa=6.0)
    for bad, msg in ((np.where(v > v.mean(), v, 0.0), "positive"), (np.where(v > v.mean(), v, np.nan), "finite"),
                     (v[:, :, :, :4], "pd has shape")):
        with pytest.raises(ValueError, match=msg):
            S.simulate_continuous(m, grids, w, 16, 8, operator=op, kappa=KAPPA, pd=bad)
    with pytest.raises(ValueError, match="needs kappa"):
        S.simulate_continuous(m, grids, w, 16, 8, operator=op, pd=v)

    def buffers(n, D):
        return (torch.full((n,), 700.0, dtype=torch.float64, device="cuda"), torch.full((n,), 0.99, dtype=torch.float64, device="cuda"),
                torch.full((n,), 50.0, dtype=torch.float64, device="cuda"), torch.ones((n, 4), dtype=torch.float64, device="cuda"),
                torch.empty((28, 4), dtype=torch.float64, device="cuda"), torch.empty((4,), dtype=torch.int32, device="cuda"),
                torch.empty((4, D), dtype=torch.float64, device="cuda"))

    # a discretised and a dense handle
    ssy = S.SSY()
    shapes = (3, 3, 3, 4)
    disc = S.ssy_operator(shapes, ssy.params, S.discretize_ssy(ssy, shapes))
    dense = S.DenseOperator(S.compute_H_single_index(ssy, (2, 2, 2, 3)), ssy.params[0], ssy.θ)
    for o, n in ((disc, 108), (dense, 24)):
        wd, ed, vd, rec, st, cl, fs = buffers(n, 4)
        d = _lib.sdfs_cont_sim_desc()
        d.n_paths, d.n_periods = 4, 8
        assert lib.sdfs_cont_sim_claim_records_dev(o._h, wd.data_ptr(), ed.data_ptr(), vd.data_ptr(), rec.data_ptr()) == _lib.SDFS_ERR_UNSUPPORTED
        assert lib.sdfs_cont_sim_claim_paths_dev(o._h, rec.data_ptr(), C.byref(d), 2.0, st.data_ptr(), cl.data_ptr(), fs.data_ptr(),
                                                 None, None) == _lib.SDFS_ERR_UNSUPPORTED
    # the argument checks of the continuous handle, each before any launch
    wd, ed, vd, rec, st, cl, fs = buffers(w.size, 4)
    h = op._h
    for args in ((None, ed.data_ptr(), vd.data_ptr(), rec.data_ptr()), (wd.data_ptr(), None, vd.data_ptr(), rec.data_ptr()),
                 (wd.data_ptr(), ed.data_ptr(), None, rec.data_ptr()), (wd.data_ptr(), ed.data_ptr(), vd.data_ptr(), None)):
        assert lib.sdfs_cont_sim_claim_records_dev(h, *args) == _lib.SDFS_ERR_ARG
    d = _lib.sdfs_cont_sim_desc()
    d.n_paths, d.n_periods = 4, 8
    states = torch.empty((4, 9, 4), dtype=torch.float64, device="cuda")
    series = torch.empty((9, 4, 8), dtype=torch.float64, device="cuda")

    def call(rec_p=rec.data_ptr(), desc=d, kappa=2.0, st_p=st.data_ptr(), cl_p=cl.data_ptr(), fs_p=fs.data_ptr(), states_p=None,
             series_p=None):
        return lib.sdfs_cont_sim_claim_paths_dev(h, rec_p, C.byref(desc) if desc is not None else None, kappa, st_p, cl_p, fs_p,
                                                 states_p, series_p)
    sentinel = torch.full_like(st, -7.0)
    st.copy_(sentinel)
    for kw in (dict(rec_p=None), dict(desc=None), dict(st_p=None), dict(cl_p=None), dict(fs_p=None), dict(kappa=float("nan")),
               dict(kappa=float("inf")), dict(states_p=states.data_ptr()), dict(series_p=series.data_ptr())):
        assert call(**kw) == _lib.SDFS_ERR_ARG, kw
    for field, value in (("lookahead", 2), ("lookahead", 4), ("group", 16), ("group", 2), ("n_periods", 1), ("n_paths", 0),
                         ("burn_in", -1), ("step_offset", (1 << 32) - 8), ("path_offset", 1 << 32), ("start_mode", 2)):
        d2 = _lib.sdfs_cont_sim_desc()
        d2.n_paths, d2.n_periods = 4, 8
        setattr(d2, field, value)
        assert call(desc=d2) == _lib.SDFS_ERR_ARG, (field, value)
    d3 = _lib.sdfs_cont_sim_desc()                      # stored paths: the default group only
    d3.n_paths, d3.n_periods, d3.group = 4, 8, 4
    assert call(desc=d3, states_p=states.data_ptr(), series_p=series.data_ptr()) == _lib.SDFS_ERR_ARG
    op.synchronize()
    assert torch.equal(st, sentinel)                    # nothing was launched
    assert call() == 0 and call(states_p=states.data_ptr(), series_p=series.data_ptr()) == 0
    op.synchronize()


# -- (6) purity -------------------------------------------------------------------------------------------------------------
def same(a, b, stats=True):
    for nm in cc.SERIES:
        for s in ("mean", "std", "ac1"):
            assert not stats or np.array_equal(a["per_path"][nm][s], b["per_path"][nm][s], equal_nan=True), (nm, s)
        assert np.array_equal(a["paths"][nm], b["paths"][nm]), nm
    assert not stats or np.array_equal(a["per_path"]["slope"], b["per_path"]["slope"], equal_nan=True)
    assert np.array_equal(a["paths"]["state"], b["paths"]["state"])
    assert np.array_equal(a["clamped"]["per_path"], b["clamped"]["per_path"])
    assert np.array_equal(a["final_state"], b["final_state"])


def joined(a, b):
    out = {"per_path": {nm: {s: np.concatenate([a["per_path"][nm][s], b["per_path"][nm][s]]) for s in ("mean", "std", "ac1")}
                        for nm in cc.SERIES},
           "paths": {nm: np.concatenate([a["paths"][nm], b["paths"][nm]]) for nm in cc.SERIES + ("state",)},
           "clamped": {"per_path": np.concatenate([a["clamped"]["per_path"], b["clamped"]["per_path"]])},
           "final_state": np.concatenate([a["final_state"], b["final_state"]])}
    out["per_path"]["slope"] = np.concatenate([a["per_path"]["slope"], b["per_path"]["slope"]])
    return out


@pytest.mark.parametrize("kind,sizes,sd", [CC.GRIDS[0], CC.GRIDS[5]], ids=[GRID_IDS[0], GRID_IDS[5]])
def test_rerun_split_and_continuation_are_bit_identical(S, kind, sizes, sd):
    m, par, grids, op, w, em = fixed_point(S, kind, sizes, sd)
    kw = dict(burn_in=5, seed=77, operator=op, return_paths=True, start=CC.start_of(grids, "vector"), kappa=KAPPA,
              pd=cc.smooth_v(grids))
    Pn = 1200
    full = S.simulate_continuous(m, grids, w, Pn, 64, **kw)
    same(full, S.simulate_continuous(m, grids, w, Pn, 64, **kw))
    a = S.simulate_continuous(m, grids, w, 500, 64, path_offset=0, **kw)
    b = S.simulate_continuous(m, grids, w, 700, 64, path_offset=500, **kw)
    same(full, joined(a, b))
    # 64 steps = 24 steps, then 40 from where they ended with the step numbers carried on
    first = S.simulate_continuous(m, grids, w, Pn, 24, **kw)
    rest = S.simulate_continuous(m, grids, w, Pn, 40, **dict(kw, burn_in=0, start=first["final_state"], step_offset=29))
    assert np.array_equal(full["paths"]["state"][:, :25], first["paths"]["state"])
    assert np.array_equal(full["paths"]["state"][:, 24:], rest["paths"]["state"])
    for nm in cc.SERIES:
        assert np.array_equal(full["paths"][nm], np.concatenate([first["paths"][nm], rest["paths"][nm]], axis=1)), nm
    assert np.array_equal(full["final_state"], rest["final_state"])
    # the storing form reads its sums back from its own series; the form without the stores keeps them in registers
    quiet = S.simulate_continuous(m, grids, w, Pn, 64, **dict(kw, return_paths=False))
    for nm in cc.SERIES:
        for s in ("mean", "std", "ac1"):
            assert np.array_equal(quiet["per_path"][nm][s], full["per_path"][nm][s], equal_nan=True), (nm, s)
    assert np.array_equal(quiet["per_path"]["slope"], full["per_path"]["slope"], equal_nan=True)
    assert np.array_equal(quiet["final_state"], full["final_state"]) and "paths" not in quiet


# -- (7) group sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes,sd", [CC.GRIDS[0], CC.GRIDS[5]], ids=[GRID_IDS[0], GRID_IDS[5]])
@pytest.mark.parametrize("n_periods", [2, 9])
def test_both_groups_give_the_default_forms_bits(S, kind, sizes, sd, n_periods):
    """sdfs_cont_sim_claim_paths_dev with groups of 4 and of 8 corners at 300 paths (a partial block); these calls store no
    path, and their statistics, clamped counts and final states are those of the default (storing) run bit for bit."""
    import torch
    m, par, grids, op, w, em = fixed_point(S, kind, sizes, sd)
    v = cc.smooth_v(grids)
    Pn, Bn, D = 300, 3, len(grids)
    st0 = CC.start_of(grids, "vector")
    out = S.simulate_continuous(m, grids, w, Pn, n_periods, burn_in=Bn, seed=CC.SEED, path_offset=CC.PATH_OFFSET, start=st0,
                                operator=op, return_paths=True, kappa=KAPPA, pd=v)
    default = np.stack([out["per_path"][nm][s] for nm in cc.SERIES for s in ("mean", "std", "ac1")] + [out["per_path"]["slope"]])
    dev = torch.device("cuda", op.device)
    wd = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(dev)
    vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
    ed = torch.empty_like(wd)
    rec = torch.empty((wd.numel(), 4), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    op.cont_sdf_mean_dev(wd.data_ptr(), ed.data_ptr())
    op.cont_sim_claim_records_dev(wd.data_ptr(), ed.data_ptr(), vd.data_ptr(), rec.data_ptr())
    op.synchronize()
    r = rec.cpu().numpy().reshape(tuple(sizes) + (4,))
    assert np.array_equal(r[..., 0], w) and np.array_equal(r[..., 2], v) and np.all(r[..., 3] == 0.0)
    np.testing.assert_allclose(r[..., 1], -np.log(out["E_M"]), rtol=1e-14)
    for g in (0, 4, 8):
        st = torch.full((28, Pn), -7.0, dtype=torch.float64, device=dev)
        cl = torch.full((Pn,), -7, dtype=torch.int32, device=dev)
        fin = torch.full((Pn, D), -7.0, dtype=torch.float64, device=dev)
        op.cont_sim_claim_paths_dev(rec.data_ptr(), KAPPA, CC.SEED, CC.PATH_OFFSET, Pn, Bn, n_periods, st.data_ptr(), cl.data_ptr(),
                                    fin.data_ptr(), start=st0, group=g)
        op.synchronize()
        assert np.array_equal(st.cpu().numpy(), default, equal_nan=True), g
        assert np.array_equal(cl.cpu().numpy() / n_periods, out["clamped"]["per_path"]), g
        assert np.array_equal(fin.cpu().numpy(), out["final_state"]), g


# -- (8) mid-size grids -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes", [("ssy", (10, 10, 10, 20)), ("gcy", (6, 6, 6, 6, 8, 8))], ids=["ssy", "gcy"])
def test_mid_size_grids(S, kind, sizes):
    m = model_of(S, kind)
    grids = S.build_grid(m, *sizes)
    op = quad_operator(S, kind, grids, 3)
    w = newton_fixed_point(op, np.ones(sizes)) if kind == "ssy" else CC.smooth_w(grids)
    v = cc.smooth_v(grids)
    kw = dict(burn_in=16, seed=5, operator=op, kappa=KAPPA, pd=v)
    a = S.simulate_continuous(m, grids, w, 5000, 64, **kw)
    b = S.simulate_continuous(m, grids, w, 5000, 64, **kw)
    plain = S.simulate_continuous(m, grids, w, 5000, 64, burn_in=16, seed=5, operator=op)
    assert a["series"] == cc.SERIES and "paths" not in a and np.array_equal(a["pd"], v)
    for nm in a["series"]:
        for s in ("mean", "std", "ac1"):
            assert np.all(np.isfinite(a["per_path"][nm][s])), (nm, s)
            assert np.array_equal(a["per_path"][nm][s], b["per_path"][nm][s]), (nm, s)
            if nm in co.SERIES:
                assert np.array_equal(a["per_path"][nm][s], plain["per_path"][nm][s]), (nm, s)
    assert np.all(np.isfinite(a["per_path"]["slope"])) and np.array_equal(a["per_path"]["slope"], b["per_path"]["slope"])
    assert np.array_equal(a["final_state"], b["final_state"]) and np.array_equal(a["final_state"], plain["final_state"])
    assert np.array_equal(a["clamped"]["per_path"], plain["clamped"]["per_path"])
    # pd_t = ln v̂(x_t) lies between the logarithms of the extremes of v; xd = rd − rf in the means
    for s, lo, hi in (("mean", np.log(v.min()), np.log(v.max())),):
        assert np.all(a["per_path"]["pd"][s] >= lo) and np.all(a["per_path"]["pd"][s] <= hi)
    np.testing.assert_allclose(a["per_path"]["xd"]["mean"], a["per_path"]["rd"]["mean"] - a["per_path"]["rf"]["mean"], rtol=0, atol=1e-12)

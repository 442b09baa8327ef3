"""
GPU tests of simulated paths at w* (sdfs_sim_records_dev, sdfs_sim_paths_dev; sdfs_via_autodiff_amd/simulation.py):

 (1) index paths bit-identical to the numpy twin (tests/sim_oracle.py) on SSY and GCY grids, stationary and fixed
     starts, burn-in 0 and 7, with and without a claim;
 (2) the series against the twin to 1e-12 (up to libm's log and cos), the per-path statistics against the two-pass
     values of the returned series to 1e-10 relative;
 (3) a run split by path_offset and a rerun are bit-identical, another seed is not;
 (4) with κ = 1 the claim is the consumption claim: rd = rc and pd = ln(w* − 1) to the claim solve's tolerance;
 (5) the Euler equation along stationary paths: the pooled means of exp(m + rc), exp(m + rf), exp(m + rd) are 1 within
     5 standard errors, and (6) the pooled means of rf and wc are ⟨π, log_rf⟩ and ⟨π, w*⟩;
 (7) the same at GCY 20^6, with a bit-identical rerun of the per-path statistics of 2^18 paths;
 (8) the refusals.
Every test runs under its own time limit (SIGALRM).
"""
import math
import signal

import numpy as np
import pytest

import sim_oracle as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


@pytest.fixture(autouse=True)
def time_limit(request):
    seconds = getattr(request.function, "time_limit_s", 240)

    def expire(signum, frame):
        raise TimeoutError(f"test exceeded its {seconds} s limit")
    old = signal.signal(signal.SIGALRM, expire)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def limit(seconds):
    def mark(fn):
        fn.time_limit_s = seconds
        return fn
    return mark


def model_of(S, kind):
    return S.SSY() if kind == "ssy" else S.GCY()


_W = {}


def fixed_point(S, kind, shapes, m=None, tag=None):
    """A tight Newton fixed point on the operator simulation.py uses (cached per grid; m, tag: another model than the
    default and its name in the cache)."""
    import torch
    from sdfs_via_autodiff_amd import _requests
    key = (kind, tuple(shapes)) if m is None else (kind, tuple(shapes), tag)
    if key not in _W:
        m = m or model_of(S, kind)
        op, _ = _requests._operator(m, shapes)
        w = torch.full(shapes, 800.0, dtype=torch.float64, device="cuda")
        _, info = op.solve_dev(w.data_ptr(), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
        assert info["status"] == 0, info
        if len(_W) > 4:
            _W.clear()
        _W[key] = w.cpu().numpy()
    return _W[key]


def twin(S, kind, shapes, w, kappa, m=None, **kw):
    from sdfs_via_autodiff_amd.simulation import cdf_tables
    m = m or model_of(S, kind)
    arr = (S.discretize_ssy if kind == "ssy" else S.discretize_gcy)(m, shapes)
    cdf, cdf0 = cdf_tables(m, shapes, arr)
    em = S.sdf_moments(m, shapes, w)["E_M"]
    v = S.claim_prices(m, shapes, w, kappa)["pd"] if kappa is not None else None
    return so.simulate(kind, m.params, arr, shapes, cdf, cdf0, w, em, v, kappa, **kw)


def close(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    both_nan = np.isnan(a) & np.isnan(b)
    err = np.abs(a - b) / np.maximum(np.abs(b), 1.0)
    err[both_nan] = 0.0
    return float(np.max(err))


GRIDS = [("ssy", (3, 4, 5, 6)), ("ssy", (15, 15, 15, 15)), ("ssy", (5, 4, 6, 7)),
         ("gcy", (3, 4, 3, 5, 2, 4)), ("gcy", (8, 8, 8, 8, 8, 8))]


# -- (1), (2) against the twin --------------------------------------------------------------------------------------------
@limit(300)
@pytest.mark.parametrize("kind,shapes", GRIDS, ids=lambda x: x if isinstance(x, str) else "x".join(map(str, x)))
@pytest.mark.parametrize("start", ["stationary", "fixed"])
@pytest.mark.parametrize("burn_in", [0, 7])
@pytest.mark.parametrize("kappa", [None, 2.0])
def test_paths_series_and_statistics_match_the_twin(S, kind, shapes, start, burn_in, kappa):
    paths_series_and_statistics_case(S, kind, shapes, start, burn_in, kappa)


def paths_series_and_statistics_case(S, kind, shapes, start, burn_in, kappa, m=None, tag=None):
    """The body of test_paths_series_and_statistics_match_the_twin; m, tag: another model than the default."""
    w = fixed_point(S, kind, shapes, m, tag)
    m = m or model_of(S, kind)
    st = None if start == "stationary" else tuple(n // 2 for n in shapes)
    P, T, seed = 1000, 64, 0x9E3779B97F4A7C15
    out = S.simulate(m, shapes, w, P, T, burn_in=burn_in, seed=seed, path_offset=123,
                     start="stationary" if st is None else st, kappa=kappa, return_paths=True)
    idx, ser, stats = twin(S, kind, shapes, w, kappa, m=m, seed=seed, path_offset=123, n_paths=P, burn_in=burn_in,
                           n_periods=T, start=st)
    got = out["paths"]
    assert got["index"].shape == (P, T + 1, len(shapes)) and got["index"].dtype == np.uint8
    assert np.array_equal(got["index"], idx), f"{np.sum(got['index'] != idx)} index entries differ"
    assert out["series"] == tuple(ser)
    worst = {"series": 0.0, "statistics, two-pass": 0.0, "statistics, twin": 0.0}
    for nm in out["series"]:
        worst["series"] = max(worst["series"], close(got[nm], ser[nm], 1.0))
        assert close(got[nm], ser[nm], 1.0) <= 1e-12, (nm, close(got[nm], ser[nm], 1.0))
    # statistics: the device's one-pass sums against the two-pass formulas on the device's own series (relative
    # error; a mean is measured against 1e-3 of the path's largest |value|, an ac1 or a slope against at least 0.01)
    for nm in out["series"]:
        mean, sd, ac1 = so.two_pass(got[nm])
        pp = out["per_path"][nm]
        floor_mean = 1e-3 * np.max(np.abs(got[nm]), axis=1)
        for a, b, floor, what in ((pp["mean"], mean, floor_mean, "mean"), (pp["std"], sd, 0.0, "std"),
                                  (pp["ac1"], ac1, 1e-2, "ac1")):
            worst["statistics, two-pass"] = max(worst["statistics, two-pass"], rel_err(a, b, floor))
            worst["statistics, twin"] = max(worst["statistics, twin"], close(a, stats[nm][what], 1.0))
            assert rel_err(a, b, floor) <= 1e-10, (nm, what, rel_err(a, b, floor))
            assert close(a, stats[nm][what], 1.0) <= 1e-9, (nm, what)     # and the twin's (its own series)
    worst["statistics, twin"] = max(worst["statistics, twin"], close(out["per_path"]["slope"], stats["slope"], 1.0))
    assert close(out["per_path"]["slope"], stats["slope"], 1.0) <= 1e-9
    return worst          # largest measured value of each of the three bounds (1e-12, 1e-10, 1e-9)


def rel_err(a, b, floor):
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN patterns differ"
    ok = ~np.isnan(b)
    if not ok.any():
        return 0.0
    den = np.maximum(np.abs(b), floor)[ok] if np.ndim(floor) else np.maximum(np.abs(b[ok]), floor)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(den, 1e-300)))


# -- (2b) every look-ahead and search, and runs shorter than the ring ----------------------------------------------------------
@pytest.mark.parametrize("kind,shapes", [("ssy", (5, 4, 6, 7)), ("gcy", (3, 4, 3, 5, 2, 4))], ids=["ssy", "gcy"])
@pytest.mark.parametrize("n_periods", [2, 3, 9])
@pytest.mark.parametrize("kappa", [None, 2.0])
def test_every_lookahead_and_search_matches_the_twin(S, kind, shapes, n_periods, kappa):
    """sdfs_sim_paths_dev with look-ahead 1 and 4 and both searches, with and without a claim, at 300 paths (a partial block) and runs shorter
    than, as long as and no multiple of the ring: these forms store no path, so their statistics are held against the
    twin's (1e-9, the bound of the test above), and against the default form's bit for bit (the forms agree in every
    bit at the parent commit too).  The default form, which stores, gives the indices (exact) and series (1e-12) of
    these run lengths."""
    import torch
    from sdfs_via_autodiff_amd import _requests
    from sdfs_via_autodiff_amd.simulation import cdf_tables
    m = model_of(S, kind)
    w = fixed_point(S, kind, shapes)
    P, B, seed, off = 300, 3, 0x9E3779B97F4A7C15, 123
    idx, ser, stats = twin(S, kind, shapes, w, kappa, seed=seed, path_offset=off, n_paths=P, burn_in=B, n_periods=n_periods)
    out = S.simulate(m, shapes, w, P, n_periods, burn_in=B, seed=seed, path_offset=off, kappa=kappa, return_paths=True)
    assert np.array_equal(out["paths"]["index"], idx)
    for nm in out["series"]:
        assert close(out["paths"][nm], ser[nm], 1.0) <= 1e-12, nm
    op, _ = _requests._operator(m, shapes)
    dev = torch.device("cuda", 0)
    wd = torch.from_numpy(w).to(dev)
    vd = torch.from_numpy(S.claim_prices(m, shapes, w, kappa)["pd"]).to(dev) if kappa is not None else None
    rec = torch.empty((op.size, 8), dtype=torch.float64, device=dev)
    op.sim_records_dev(wd.data_ptr(), None if vd is None else vd.data_ptr(), rec.data_ptr())
    cdf, cdf0 = cdf_tables(m, shapes)
    cdf, cdf0 = np.concatenate([c.ravel() for c in cdf]), np.concatenate(cdf0)
    names = out["series"]
    default = np.stack([out["per_path"][nm][s] for nm in names for s in ("mean", "std", "ac1")] + [out["per_path"]["slope"]])
    want = np.stack([stats[nm][s] for nm in names for s in ("mean", "std", "ac1")] + [stats["slope"]])
    for k in (1, 4):
        for search in (1, 2):
            st = torch.full((3 * len(names) + 1, P), -7.0, dtype=torch.float64, device=dev)
            op.sim_paths_dev(rec.data_ptr(), cdf, cdf0, seed, off, P, B, n_periods, kappa=kappa, stats_ptr=st.data_ptr(),
                             lookahead=k, search=search)
            torch.cuda.synchronize()
            got = st.cpu().numpy()
            print(f"lookahead {k} search {search}: statistics vs twin {close(got, want, 1.0):.3e}")
            assert close(got, want, 1.0) <= 1e-9, (k, search)
            assert np.array_equal(got, default, equal_nan=True), (k, search)


# -- (3) determinism and splits -------------------------------------------------------------------------------------------
@limit(300)
@pytest.mark.parametrize("kind,shapes", [("ssy", (5, 4, 6, 7)), ("gcy", (3, 4, 3, 5, 2, 4))], ids=["ssy", "gcy"])
def test_split_and_rerun_are_bit_identical(S, kind, shapes):
    m = model_of(S, kind)
    w = fixed_point(S, kind, shapes)
    kw = dict(burn_in=5, seed=77, kappa=2.0, return_paths=True)
    full = S.simulate(m, shapes, w, 3000, 100, **kw)
    again = S.simulate(m, shapes, w, 3000, 100, **kw)
    a = S.simulate(m, shapes, w, 1100, 100, path_offset=0, **kw)
    b = S.simulate(m, shapes, w, 1900, 100, path_offset=1100, **kw)
    for nm in full["series"]:
        for s in ("mean", "std", "ac1"):
            x = full["per_path"][nm][s]
            assert np.array_equal(x, again["per_path"][nm][s], equal_nan=True)
            assert np.array_equal(x, np.concatenate([a["per_path"][nm][s], b["per_path"][nm][s]]), equal_nan=True)
        assert np.array_equal(full["paths"][nm], np.concatenate([a["paths"][nm], b["paths"][nm]]))
    assert np.array_equal(full["paths"]["index"], np.concatenate([a["paths"]["index"], b["paths"]["index"]]))
    assert np.array_equal(full["per_path"]["slope"], again["per_path"]["slope"], equal_nan=True)
    other = S.simulate(m, shapes, w, 3000, 100, **dict(kw, seed=78))
    assert not np.array_equal(other["paths"]["index"], full["paths"]["index"])
    assert not np.array_equal(other["per_path"]["dc"]["mean"], full["per_path"]["dc"]["mean"])


# -- (4) the consumption claim --------------------------------------------------------------------------------------------
@limit(300)
@pytest.mark.parametrize("kind,shapes", [("ssy", (15,) * 4), ("gcy", (8,) * 6)], ids=["ssy15", "gcy8"])
def test_kappa_one_is_the_consumption_claim(S, kind, shapes):
    m = model_of(S, kind)
    w = fixed_point(S, kind, shapes)
    out = S.simulate(m, shapes, w, 2000, 64, kappa=1.0, rtol=1e-12, return_paths=True)
    p = out["paths"]
    assert np.max(np.abs(p["rd"] - p["rc"])) <= 1e-8
    flat = np.ravel_multi_index(tuple(p["index"][:, 1:, a].astype(np.int64) for a in range(len(shapes))), shapes)
    assert np.max(np.abs(p["pd"] - np.log(w - 1.0).ravel()[flat])) <= 1e-8
    assert np.max(np.abs(p["wc"] - w.ravel()[flat])) == 0.0


# -- (5), (6) the Euler equation and the unconditional means ----------------------------------------------------------------
def euler_checks(S, kind, shapes, P, T, w):
    m = model_of(S, kind)
    out = S.simulate(m, shapes, w, P, T, seed=2024, kappa=2.0, return_paths=True)
    p = out["paths"]
    n = P * T
    report = {}
    for r in ("rc", "rf", "rd"):
        e = np.exp(p["m"] + p[r])
        mean, se = float(e.mean()), float(e.std() / math.sqrt(n))
        report[r] = (mean, se)
        assert abs(mean - 1.0) <= 5.0 * se, (r, mean, se)
    return out, report


@limit(600)
@pytest.mark.parametrize("kind,shapes", [("ssy", (15,) * 4), ("gcy", (16,) * 6)], ids=["ssy15", "gcy16"])
def test_euler_equation_and_unconditional_means(S, kind, shapes):
    m = model_of(S, kind)
    w = fixed_point(S, kind, shapes)
    out, report = euler_checks(S, kind, shapes, 1 << 14, 512, w)
    pis = S.stationary_weights(m, shapes)
    pi = pis[0]
    for g in pis[1:]:
        pi = np.multiply.outer(pi, g)
    log_rf = S.sdf_moments(m, shapes, w)["log_rf"]
    for nm, want in (("rf", float(np.sum(pi * log_rf))), ("wc", float(np.sum(pi * w)))):
        got = out["pooled"][nm]
        assert abs(got["mean"] - want) <= 5.0 * got["se"], (nm, got, want)


# -- (7) full size ----------------------------------------------------------------------------------------------------------
@limit(900)
def test_gcy20_euler_and_rerun(S):
    shapes = (20,) * 6
    m = S.GCY()
    w = fixed_point(S, "gcy", shapes)
    euler_checks(S, "gcy", shapes, 1 << 15, 256, w)
    a = S.simulate(m, shapes, w, 1 << 18, 240, seed=5, burn_in=16)
    b = S.simulate(m, shapes, w, 1 << 18, 240, seed=5, burn_in=16)
    for nm in a["series"]:
        for s in ("mean", "std", "ac1"):
            assert np.array_equal(a["per_path"][nm][s], b["per_path"][nm][s], equal_nan=True), (nm, s)
    assert np.array_equal(a["per_path"]["slope"], b["per_path"]["slope"], equal_nan=True)
    _W.clear()


# -- (8) refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(S):
    import ctypes as C
    import torch
    from sdfs_via_autodiff_amd import _lib
    ssy = S.SSY()
    grids = S.build_grid(ssy, 3, 3, 3, 4)
    nodes, weights = S.qnwnorm([3] * 4)
    Tc = S.T_fun_factory((np.array(ssy.params), grids, nodes.T.copy(), weights), "quadrature", 3 * 3 * 3 * 4)
    wd = torch.full((3, 3, 3, 4), 700.0, dtype=torch.float64, device="cuda")
    rec = torch.empty((108, 8), dtype=torch.float64, device="cuda")
    st = torch.empty((19, 4), dtype=torch.float64, device="cuda")
    assert _lib.lib.sdfs_sim_records_dev(Tc._h, wd.data_ptr(), None, rec.data_ptr()) == _lib.SDFS_ERR_UNSUPPORTED
    d = _lib.sdfs_sim_desc()
    d.n_paths, d.n_periods = 4, 8
    cdf = np.full(3 * 9 + 3 * 9 + 16, 2.0)
    d.cdf = cdf.ctypes.data_as(C.POINTER(C.c_double))
    d.cdf0 = d.cdf
    assert _lib.lib.sdfs_sim_paths_dev(Tc._h, rec.data_ptr(), C.byref(d), st.data_ptr(), None, None) == \
        _lib.SDFS_ERR_UNSUPPORTED
    # a claim without a finite price, and a w* with a point <= 1
    shapes = (3, 3, 3, 5)
    w = fixed_point(S, "ssy", shapes)
    with pytest.raises(ValueError, match="no finite price"):
        S.simulate(ssy, shapes, w, 16, 8, kappa=8.0)
    bad = w.copy()
    bad[1, 2, 0, 4] = 0.5
    with pytest.raises(ValueError, match="exceed 1"):
        S.simulate(ssy, shapes, bad, 16, 8)

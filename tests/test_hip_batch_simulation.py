"""
GPU tests of the batch simulation (csrc/batch_sim.hpp, sdfs_batch_sim_records_dev, sdfs_batch_sim_paths_dev,
``BatchOperator.simulate``, ``simulate_batch``): B = 6 members of tests/batch_family.py at their Newton fixed points,
P = 1000 paths (a ragged last workgroup) of T = 64 steps unless stated.

 (1) every member against the numpy twin (tests/sim_oracle.py) fed with that member's tables, w and the E_M and pd grids
     of ``op.price`` on the same handle: indices bit for bit, series to 1e-12, per-path statistics to 1e-10 against the
     two-pass values of the device's own series and to 1e-9 against the twin's;
 (2) against ``simulate`` member by member: identical indices, dc, m, rc, wc within 1e-12;
 (3) records in LDS and gathered from global memory give identical bits; the LDS form is refused where it does not fit;
 (4) a member's bits do not depend on B or its place, equal members are equal, a rerun and a path_offset split are
     bit-identical, another seed is not;
 (5) the device's (n, mean, se) against numpy on the returned per-path arrays, with NaN statistics among them;
 (6) statuses 3 (no finite price) and 4 (a point of w <= 1) with untouched neighbours;
 (7) the "loop" plan at SSY 12^4;  (8) the Euler equation at SSY 5^4.
Shapes: SSY (3,4,3,5) mixed extents; GCY (3,2,3,2,2,3) six axes (the second Philox block feeds axes 4 and 5); SSY 5^4
LDS records of real size; SSY 8^4 = 4 096 points, the global form only.  Every test runs under its own time limit.
"""
import math
import signal

import numpy as np
import pytest

import sim_oracle as so
from batch_family import member, package_model
from test_hip_simulation import close, rel_err

pytestmark = pytest.mark.gpu

SMALL = [("ssy", (3, 4, 3, 5)), ("gcy", (3, 2, 3, 2, 2, 3)), ("ssy", (5, 5, 5, 5))]
BIG = ("ssy", (8, 8, 8, 8))
SHAPES = SMALL + [BIG]
IDS = (0, 1, 2, 3, 4, 5)
P, T, SEED = 1000, 64, 0x9E3779B97F4A7C15
STATS = ("mean", "std", "ac1")


def sid(x):
    return x if isinstance(x, str) else "x".join(map(str, x))


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


@pytest.fixture(autouse=True)
def time_limit(request):
    seconds = getattr(request.function, "time_limit_s", 120)

    def expire(signum, frame):
        raise TimeoutError(f"test exceeded its {seconds} s limit")
    old = signal.signal(signal.SIGALRM, expire)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def family(S, kind, ids=IDS):
    return [package_model(S, kind, member(kind, b)) for b in ids]


_solved = {}
_sims = {}


def solved(S, kind, shapes, ids=IDS):
    """w* of the family members ``ids`` by the batch Newton solve from 800 (once per module)."""
    key = (kind, shapes, tuple(ids))
    if key not in _solved:
        res = S.solve_batch(family(S, kind, ids), shapes, algorithm="newton", tol=1e-10)
        assert np.all(res.status == 0), res.status
        _solved[key] = res.w
    return _solved[key]


def run(S, kind, shapes, ids=IDS, **kw):
    """simulate_batch of the family members ``ids`` (cached per request; the results are not modified)."""
    key = (kind, shapes, tuple(ids), tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _sims:
        if len(_sims) > 12:
            _sims.clear()
        args = dict(dict(n_paths=P, n_periods=T, seed=SEED), **kw)
        _sims[key] = S.simulate_batch(family(S, kind, ids), shapes, solved(S, kind, shapes, ids), args.pop("n_paths"),
                                      args.pop("n_periods"), **args)
    return _sims[key]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def assert_same_member(x, bx, y, by, per_path=True, paths=True):
    """Member bx of result x and member by of result y carry the same bits."""
    assert x.series == y.series
    names = list(x.series) + ["slope"]
    for nm in names:
        for s in (STATS if nm != "slope" else (None,)):
            mx, my = (x.moments[nm][s], y.moments[nm][s]) if s else (x.moments[nm], y.moments[nm])
            for q in ("n", "mean", "se"):
                assert same(mx[q][bx], my[q][by]), (nm, s, q)
            if per_path:
                px, py = (x.per_path[nm][s], y.per_path[nm][s]) if s else (x.per_path[nm], y.per_path[nm])
                assert same(px["values"][bx], py["values"][by]), (nm, s)
    if paths:
        for nm in ("index",) + tuple(x.series):
            assert same(x.paths[nm][bx], y.paths[nm][by]), nm


# -- (1) against the twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shapes", SHAPES, ids=sid)
@pytest.mark.parametrize("start", ["stationary", "fixed"])
@pytest.mark.parametrize("burn_in", [0, 7])
@pytest.mark.parametrize("kappa", [None, 2.0])
def test_every_member_matches_the_twin(S, kind, shapes, start, burn_in, kappa):
    every_member_matches_the_twin(S, kind, shapes, start, burn_in, kappa, family(S, kind), solved(S, kind, shapes))


def every_member_matches_the_twin(S, kind, shapes, start, burn_in, kappa, models, w):
    """The body of test_every_member_matches_the_twin on any batch of models at their fixed points w; returns what
    BatchOperator.simulate returned and the largest measured value of each of the three bounds (1e-12, 1e-10, 1e-9)."""
    from sdfs_via_autodiff_amd.simulation import cdf_tables
    st = None if start == "stationary" else tuple(n // 2 for n in shapes)
    disc = S.discretize_ssy if kind == "ssy" else S.discretize_gcy
    op = S.BatchOperator.from_models(models, shapes)
    try:
        grids = op.price(w, kappa, return_grids=True)[2]
        r = op.simulate(w, P, T, burn_in=burn_in, seed=SEED, path_offset=123, start="stationary" if st is None else st,
                        kappa=kappa, return_per_path=True, return_paths=True)
    finally:
        op.close()
    assert np.all(r["status"] == 0), r["status"]
    names = r["series"]
    ns = len(names)
    worst = {"series": 0.0, "statistics, two-pass": 0.0, "statistics, twin": 0.0}
    assert r["index"].shape == (len(models), P, T + 1, len(shapes)) and r["index"].dtype == np.uint8
    for b, m in enumerate(models):
        arr = disc(m, shapes)
        cdf, cdf0 = cdf_tables(m, shapes, arr)
        idx, ser, stats = so.simulate(kind, m.params, arr, shapes, cdf, cdf0, w[b], grids["E_M"][b],
                                      grids["pd"][b] if kappa is not None else None, kappa, seed=SEED, path_offset=123,
                                      n_paths=P, burn_in=burn_in, n_periods=T, start=st)
        assert np.array_equal(r["index"][b], idx), (b, int(np.sum(r["index"][b] != idx)))
        assert names == tuple(ser)
        for i, nm in enumerate(names):
            got = r["paths"][b, i]
            worst["series"] = max(worst["series"], close(got, ser[nm], 1.0))
            assert close(got, ser[nm], 1.0) <= 1e-12, (b, nm, close(got, ser[nm], 1.0))
            # the device's one-pass sums against the two-pass formulas on the device's own series (a mean is measured
            # against 1e-3 of the path's largest |value|, an ac1 against at least 0.01), then against the twin's
            mean, sd, ac1 = so.two_pass(got)
            floor_mean = 1e-3 * np.max(np.abs(got), axis=1)
            for j, (ref, floor) in enumerate(((mean, floor_mean), (sd, 0.0), (ac1, 1e-2))):
                a = r["stats"][b, 3 * i + j]
                worst["statistics, two-pass"] = max(worst["statistics, two-pass"], rel_err(a, ref, floor))
                worst["statistics, twin"] = max(worst["statistics, twin"], close(a, stats[nm][STATS[j]], 1.0))
                assert rel_err(a, ref, floor) <= 1e-10, (b, nm, STATS[j], rel_err(a, ref, floor))
                assert close(a, stats[nm][STATS[j]], 1.0) <= 1e-9, (b, nm, STATS[j])
        worst["statistics, twin"] = max(worst["statistics, twin"], close(r["stats"][b, 3 * ns], stats["slope"], 1.0))
        assert close(r["stats"][b, 3 * ns], stats["slope"], 1.0) <= 1e-9, b
    return r, worst


# -- (1b) every look-ahead of the global form, and runs shorter than the ring -------------------------------------------------
@pytest.mark.parametrize("kind,shapes", SMALL[:2], ids=sid)
@pytest.mark.parametrize("n_periods", [2, 3, 9])
@pytest.mark.parametrize("kappa", [None, 2.0])
def test_every_lookahead_matches_the_twin(S, kind, shapes, n_periods, kappa):
    """``simulate_dev`` with the records gathered at look-ahead 1 and 4, with and without a claim, 300 paths (a partial workgroup) and runs shorter
    than, as long as and no multiple of the ring.  These forms store no path: their per-path statistics are held against
    the twin's (1e-9) and their statistics and moments against the default form's bit for bit (the forms agree in every
    bit at the parent commit too, as tools/batch_simulation_times.py asserts of the moments); the default form, which
    stores, gives the indices (exact) and series (1e-12) of these run lengths."""
    import torch
    from sdfs_via_autodiff_amd.batch import batch_cdf_tables
    from sdfs_via_autodiff_amd.simulation import cdf_tables
    ids, Pn, Bn, off = IDS[:3], 300, 3, 123
    models, w = family(S, kind, ids), solved(S, kind, shapes)[:3]
    disc = S.discretize_ssy if kind == "ssy" else S.discretize_gcy
    op = S.BatchOperator.from_models(models, shapes)
    try:
        grids = op.price(w, kappa, return_grids=True)[2]
        wd, em = (op._to_dev(np.ascontiguousarray(x, dtype=np.float64)) for x in (w, grids["E_M"]))
        pd = op._to_dev(np.ascontiguousarray(grids["pd"], dtype=np.float64)) if kappa is not None else None
        dev = wd.device
        rec = torch.empty((3, op.size, 8), dtype=torch.float64, device=dev)
        cdf, cdf0 = batch_cdf_tables(kind, shapes, op._arrays)
        ns, nd = 9 if kappa is not None else 6, len(shapes)

        def run_form(k, store):
            st = torch.full((3, 3 * ns + 1, Pn), -7.0, dtype=torch.float64, device=dev)
            mom = torch.full((3, 3 * ns + 1, 3), -7.0, dtype=torch.float64, device=dev)
            idx = torch.empty((3, Pn, n_periods + 1, nd), dtype=torch.uint8, device=dev) if store else None
            ser = torch.empty((3, ns, Pn, n_periods), dtype=torch.float64, device=dev) if store else None
            torch.cuda.synchronize()
            op.simulate_dev(wd.data_ptr(), em.data_ptr(), None if pd is None else pd.data_ptr(), rec.data_ptr(), cdf, cdf0, Pn, n_periods, burn_in=Bn,
                            seed=SEED, path_offset=off, kappa=None if kappa is None else np.full(3, kappa), records=2, lookahead=k, stats_ptr=st.data_ptr(),
                            moments_ptr=mom.data_ptr(), idx_ptr=None if idx is None else idx.data_ptr(),
                            series_ptr=None if ser is None else ser.data_ptr())
            op.synchronize()
            return st.cpu().numpy(), mom.cpu().numpy(), None if idx is None else idx.cpu().numpy(), None if ser is None else ser.cpu().numpy()
        st0, mom0, idx0, ser0 = run_form(0, True)
        forms = {k: run_form(k, False) for k in (1, 4)}
    finally:
        op.close()
    for b, m in enumerate(models):
        arr = disc(m, shapes)
        c, c0 = cdf_tables(m, shapes, arr)
        idx, ser, stats = so.simulate(kind, m.params, arr, shapes, c, c0, w[b], grids["E_M"][b], grids["pd"][b] if kappa is not None else None, kappa,
                                      seed=SEED, path_offset=off, n_paths=Pn, burn_in=Bn, n_periods=n_periods)
        assert np.array_equal(idx0[b], idx), b
        for i, nm in enumerate(ser):
            assert close(ser0[b, i], ser[nm], 1.0) <= 1e-12, (b, nm)
        want = np.stack([stats[nm][s] for nm in ser for s in STATS] + [stats["slope"]])
        for k, (st, mom, _, _) in forms.items():
            print(f"member {b} lookahead {k}: statistics vs twin {close(st[b], want, 1.0):.3e}")
            assert close(st[b], want, 1.0) <= 1e-9, (b, k)
            assert same(st[b], st0[b]) and same(mom[b], mom0[b]), (b, k)


# -- (2) against simulate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shapes", SMALL[:2] + [BIG], ids=sid)
def test_members_match_simulate(S, kind, shapes):
    models = family(S, kind)
    w = solved(S, kind, shapes)
    kw = dict(burn_in=7, path_offset=5, kappa=2.0)
    res = run(S, kind, shapes, return_per_path=True, return_paths=True, **kw)
    assert res.plan == "batch" and np.all(res.status == 0)
    for b, m in enumerate(models):
        one = S.simulate(m, shapes, w[b], P, T, seed=SEED, return_paths=True, **kw)
        assert one["series"] == res.series
        assert np.array_equal(res.paths["index"][b], one["paths"]["index"]), b
        for nm in ("dc", "m", "rc", "wc"):
            assert close(res.paths[nm][b], one["paths"][nm], 1.0) <= 1e-12, (b, nm)


# -- (3) the two record forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shapes", SMALL, ids=sid)
@pytest.mark.parametrize("kappa", [None, 2.0])
def test_lds_and_global_records_give_the_same_bits(S, kind, shapes, kappa):
    assert S.batch_sim_lds_bytes(kind, shapes, 1) is not None
    kw = dict(burn_in=7, kappa=kappa, return_per_path=True, return_paths=True)
    a = run(S, kind, shapes, records=1, **kw)
    g = run(S, kind, shapes, records=2, **kw)
    d = run(S, kind, shapes, **kw)
    for b in range(6):
        assert_same_member(a, b, g, b)
        assert_same_member(a, b, d, b)


def test_lds_records_above_64_kib(S):
    # SSY 7^4: 2 401 records = 153 664 B, the largest LDS form there is (the kernel's dynamic LDS limit has to be raised)
    kind, shapes = "ssy", (7, 7, 7, 7)
    assert S.batch_sim_lds_bytes(kind, shapes, 1) > 64 * 1024
    kw = dict(ids=(0, 1), n_paths=300, burn_in=3, kappa=2.0, return_per_path=True, return_paths=True)
    a = run(S, kind, shapes, records=1, **kw)
    g = run(S, kind, shapes, records=2, **kw)
    assert np.all(a.status == 0)
    for b in range(2):
        assert_same_member(a, b, g, b)


def test_lds_records_are_refused_where_they_do_not_fit(S):
    import torch
    from sdfs_via_autodiff_amd.batch import batch_cdf_tables
    kind, shapes = BIG
    assert S.batch_sim_lds_bytes(kind, shapes, 1) is None and S.batch_sim_lds_bytes(kind, shapes, 2) is not None
    models = family(S, kind, (0, 1))
    w = solved(S, kind, shapes)[:2]
    with pytest.raises(ValueError, match="do not fit"):
        S.simulate_batch(models, shapes, w, 8, 4, records=1)
    # the library's own refusal (SDFS_ERR_ARG), reached through the pointer form
    op = S.BatchOperator.from_models(models, shapes)
    try:
        N = int(np.prod(shapes))
        g = torch.full((2, N), 2.0, dtype=torch.float64, device="cuda")
        rec = torch.empty((2, N, 8), dtype=torch.float64, device="cuda")
        mom = torch.empty((2, 19, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        cdf, cdf0 = batch_cdf_tables(kind, shapes, op._arrays)
        with pytest.raises(S.SdfsError, match="records = 1"):
            op.simulate_dev(g.data_ptr(), g.data_ptr(), None, rec.data_ptr(), cdf, cdf0, 8, 4, records=1, moments_ptr=mom.data_ptr())
        assert "simulation:" in op.describe_plan() and "does not fit" in op.describe_plan()
    finally:
        op.close()


# -- (4) independence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shapes", SMALL[:2] + [BIG], ids=sid)
def test_a_member_does_not_depend_on_the_batch(S, kind, shapes):
    kw = dict(burn_in=7, kappa=2.0, return_per_path=True, return_paths=True)
    full = run(S, kind, shapes, **kw)
    rev = run(S, kind, shapes, ids=IDS[::-1], **kw)
    for b in (1, 4):
        alone = run(S, kind, shapes, ids=(b,), **kw)
        assert_same_member(full, b, alone, 0)
        assert_same_member(full, b, rev, 5 - b)
    twice = run(S, kind, shapes, ids=(2, 0, 2), **kw)
    assert_same_member(twice, 0, twice, 2)
    assert_same_member(twice, 0, full, 2)


@pytest.mark.parametrize("kind,shapes", SMALL[:2], ids=sid)
def test_rerun_split_and_seed(S, kind, shapes):
    models = family(S, kind)
    w = solved(S, kind, shapes)
    kw = dict(burn_in=5, kappa=2.0, return_per_path=True, return_paths=True)
    full = run(S, kind, shapes, **kw)
    again = S.simulate_batch(models, shapes, w, P, T, seed=SEED, **kw)
    a = S.simulate_batch(models, shapes, w, 300, T, seed=SEED, path_offset=0, **kw)
    c = S.simulate_batch(models, shapes, w, 700, T, seed=SEED, path_offset=300, **kw)
    for b in range(6):
        assert_same_member(full, b, again, b)
    for nm in full.series:
        for s in STATS:
            assert same(full.per_path[nm][s]["values"],
                        np.concatenate([a.per_path[nm][s]["values"], c.per_path[nm][s]["values"]], axis=1)), (nm, s)
        assert same(full.paths[nm], np.concatenate([a.paths[nm], c.paths[nm]], axis=1)), nm
    assert same(full.per_path["slope"]["values"], np.concatenate([a.per_path["slope"]["values"], c.per_path["slope"]["values"]], axis=1))
    assert same(full.paths["index"], np.concatenate([a.paths["index"], c.paths["index"]], axis=1))
    other = S.simulate_batch(models, shapes, w, P, T, seed=SEED + 1, **kw)
    assert not np.array_equal(other.paths["index"], full.paths["index"])
    assert not np.array_equal(other.moments["dc"]["mean"]["mean"], full.moments["dc"]["mean"]["mean"])


# -- (5) the moments --------------------------------------------------------------------------------------------------------
def check_moments(res):
    """The device's (n, mean, se) of every statistic against numpy on the returned per-path values over their finite
    entries: n exact, mean and se to 1e-10 relative.  One exception: where numpy's own se is below 1e-13 of the largest
    |value| the spread is rounding noise of the values (the ac1 of a T = 2 series is -0.5 for every path) and no relative
    bound can hold; the device's se must then lie within 4 ulp of that largest |value| (2^-50) of numpy's.
    Returns the number of non-finite entries met."""
    holes = 0
    for nm in list(res.series) + ["slope"]:
        for s in (STATS if nm != "slope" else (None,)):
            mo = res.moments[nm][s] if s else res.moments[nm]
            vals = res.per_path[nm][s]["values"] if s else res.per_path[nm]["values"]
            for b in range(vals.shape[0]):
                x = vals[b][np.isfinite(vals[b])]
                holes += vals[b].size - x.size
                assert mo["n"][b] == x.size, (nm, s, b, mo["n"][b], x.size)
                top = np.max(np.abs(x))
                mean, se = x.mean(), x.std(ddof=1) / math.sqrt(x.size)
                em = abs(mo["mean"][b] - mean) / abs(mean)
                noise = se < 1e-13 * top
                es = abs(mo["se"][b] - se) / (top * 2.0 ** -50 if noise else se)
                print(f"moments {nm} {s} member {b}: n {x.size} mean err {em:.2e} se err {es:.2e}{' (ulp of max|x|, noise)' if noise else ''}")
                assert em <= 1e-10, (nm, s, b, em)
                assert es <= (1.0 if noise else 1e-10), (nm, s, b, es, noise)
    return holes


@pytest.mark.parametrize("kind,shapes", SHAPES, ids=sid)
def test_moments_match_numpy(S, kind, shapes):
    check_moments(run(S, kind, shapes, burn_in=7, kappa=2.0, return_per_path=True))


def test_moments_leave_nan_statistics_out(S):
    # T = 2 from a fixed start: a path that stays where it started has constant series, so zero denominators
    kind, shapes = SMALL[0]
    res = run(S, kind, shapes, n_periods=2, start=tuple(n // 2 for n in shapes), kappa=2.0, return_per_path=True)
    holes = check_moments(res)
    assert holes > 0, "the case was meant to have NaN statistics"
    assert np.all(res.moments["rf"]["ac1"]["n"] < P) and np.all(res.moments["dc"]["mean"]["n"] == P)


def test_five_paths(S):
    kind, shapes = SMALL[1]
    res = run(S, kind, shapes, n_paths=5, kappa=2.0, return_per_path=True, return_paths=True)
    big = run(S, kind, shapes, kappa=2.0, return_per_path=True, return_paths=True)
    check_moments(res)
    assert np.array_equal(res.paths["index"], big.paths["index"][:, :5])
    assert same(res.per_path["xd"]["ac1"]["values"], big.per_path["xd"]["ac1"]["values"][:, :5])


# -- (6) statuses -----------------------------------------------------------------------------------------------------------
def all_nan_member(res, b):
    for nm in list(res.series) + ["slope"]:
        for s in (STATS if nm != "slope" else (None,)):
            mo = res.moments[nm][s] if s else res.moments[nm]
            pp = res.per_path[nm][s] if s else res.per_path[nm]
            assert all(np.isnan(mo[q][b]) for q in ("n", "mean", "se")), (nm, s)
            assert np.all(np.isnan(pp["values"][b])) and all(np.isnan(pp[q][b]) for q in ("median", "p05", "p95")), (nm, s)
    for nm in res.series:
        assert np.all(np.isnan(res.paths[nm][b])), nm
    assert not res.paths["index"][b].any()


def test_statuses_leave_the_neighbours_alone(S):
    shapes = (3, 3, 3, 5)
    fam = family(S, "ssy")
    models = fam[:2] + [S.SSY()] + fam[3:]               # the default calibration has no finite price at kappa = 8
    sol = S.solve_batch(models, shapes, algorithm="newton", tol=1e-10)
    assert np.all(sol.status == 0)
    w = sol.w
    kap = np.array([2.0, 2.0, 8.0, 2.0, 2.0, 2.0])
    op = S.BatchOperator.from_models(models, shapes)
    try:
        assert list(op.price(w, kap)[-1]) == [0, 0, 3, 0, 0, 0]          # (confirmed on the batch handle)
    finally:
        op.close()
    kw = dict(burn_in=7, seed=SEED, return_per_path=True, return_paths=True)
    res = S.simulate_batch(models, shapes, w, P, T, kappa=kap, **kw)
    assert list(res.status) == [0, 0, 3, 0, 0, 0]
    all_nan_member(res, 2)
    keep = [0, 1, 3, 4, 5]
    ref = S.simulate_batch([models[b] for b in keep], shapes, w[keep], P, T, kappa=2.0, **kw)
    assert np.all(ref.status == 0)
    for i, b in enumerate(keep):
        assert_same_member(res, b, ref, i)
    bad = w.copy()
    bad[4, 1, 2, 0, 4] = 0.5
    res4 = S.simulate_batch(models, shapes, bad, P, T, kappa=2.0, **kw)
    assert res4.status[4] == 4 and np.all(np.delete(res4.status, [2, 4]) == 0)
    all_nan_member(res4, 4)
    for i, b in enumerate(keep):
        if b != 4:
            assert_same_member(res4, b, ref, i)


# -- (7) the loop plan ------------------------------------------------------------------------------------------------------
def test_loop_plan_returns_the_same_fields(S):
    kind, shapes = "ssy", (12, 12, 12, 12)
    assert S.batch_lds_bytes(kind, shapes) is None
    models = family(S, kind, (0, 1))
    w = solved(S, kind, shapes, (0, 1))
    res = S.simulate_batch(models, shapes, w, 500, T, burn_in=3, seed=SEED, kappa=2.0, return_per_path=True, return_paths=True)
    small = run(S, *SMALL[0], kappa=2.0, return_per_path=True, return_paths=True)
    assert res.plan == "loop" and small.plan == "batch" and res._fields == small._fields
    assert res.series == small.series and set(res.moments) == set(small.moments) and set(res.per_path) == set(small.per_path)
    assert set(res.paths) == set(small.paths) and set(res.price) == set(small.price)
    assert set(res.per_path["dc"]["mean"]) == set(small.per_path["dc"]["mean"])
    assert list(res.status) == [0, 0]
    for b, m in enumerate(models):
        one = S.simulate(m, shapes, w[b], 500, T, burn_in=3, seed=SEED, kappa=2.0)
        for nm in res.series:
            assert np.array_equal(res.per_path[nm]["mean"]["values"][b], one["per_path"][nm]["mean"]), (b, nm)
            x = one["per_path"][nm]["mean"]
            assert res.moments[nm]["mean"]["n"][b] == 500
            assert abs(res.moments[nm]["mean"]["mean"][b] - x.mean()) <= 1e-12 * max(abs(x.mean()), 1.0)


# -- (8) the Euler equation -------------------------------------------------------------------------------------------------
def test_euler_equation(S):
    kind, shapes = "ssy", (5, 5, 5, 5)
    Pn, Tn = 4096, 256
    res = run(S, kind, shapes, n_paths=Pn, n_periods=Tn, seed=2024, kappa=2.0, return_paths=True)
    assert np.all(res.status == 0)
    for b in range(6):
        for r in ("rc", "rf", "rd"):
            e = np.exp(res.paths["m"][b] + res.paths[r][b])
            mean, se = float(e.mean()), float(e.std() / math.sqrt(Pn * Tn))
            print(f"euler member {b} {r}: mean {mean:.6f} se {se:.2e}")
            assert abs(mean - 1.0) <= 5.0 * se, (b, r, mean, se)

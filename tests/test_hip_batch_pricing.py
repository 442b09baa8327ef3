"""
GPU tests of batch pricing (csrc/batch_price.hpp, sdfs_batch_price_dev, ``BatchOperator.price``, ``price_batch``): one
workgroup per member, checked per member against the numpy oracle (``folded_K`` of tests/test_pricing_cpu.py through
tests/batch_pricing_oracle.py), against dense numpy, against the single-problem path, and for independence of a member's
bits from the batch, its place in it and the budget of a launch.  Every test runs under its own time limit (SIGALRM).

B = 3, κ = 2, rtol 1e-12 unless stated.  The shapes hit every form of the kernel:
    SSY (3,4,3,5)  180 points  registers, K = 1        GCY 4^6          4 096  global, K = 8
    SSY 5^4        625         K = 4                   SSY (7,13,11,9)  9 009  global, K = 20, row classes 8/16/12/12
    GCY 3^6        729         K = 4                   SSY 10^4        10 000  global, K = 20
    GCY (3,4,5,2,3,4) 1 440    K = 8                   GCY 5^6         15 625  global, K = 32
"""
import signal

import numpy as np
import pytest

import batch_pricing_oracle as bpo
from batch_family import member, package_model

pytestmark = pytest.mark.gpu

SHAPES = [("ssy", (3, 4, 3, 5)), ("ssy", (5,) * 4), ("gcy", (3,) * 6), ("gcy", (3, 4, 5, 2, 3, 4)), ("gcy", (4,) * 6),
          ("ssy", (7, 13, 11, 9)), ("ssy", (10,) * 4), ("gcy", (5,) * 6)]
SMALL = SHAPES[:4]                                       # N <= 1 440: dense numpy is cheap
NEWTON = dict(algorithm="newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
KAPPA = 2.0
GRIDS = ("E_M", "E_M2", "pd", "expected_return")
# A yield is <g, -ln P_n> / n with P_n near 1: a relative error e of P_n is an absolute error e of ln P_n, so a yield of
# 1e-3 cannot hold a relative bound.  test_term_structure_vs_dense_matrix_powers therefore pairs its rtol of 1e-12 with
# this absolute term (the 1e-12 on the price alone would allow 1e-12 / n), and so do the yields here.
# The oracle takes T w from extended precision (batch_pricing_oracle.extended_Tw): with oracle_T's fp64 T w, folded_K's
# power 1 - theta turns a bias of a few ulp into an offset of 1.1e-14 ... 1.4e-14 on every GCY yield (measured against the
# device on an MI355X, and against an extended-precision restatement in tests/test_batch_pricing_cpu.py), above this term.
YIELD_ATOL = 1e-14


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


def n_max_of(shapes):
    return 50 if int(np.prod(shapes)) <= 1440 else 8


def family(S, kind, ids):
    return [package_model(S, kind, member(kind, b)) for b in ids]


_solved = {}
_priced = {}
_members = {}
_dense = {}


def solved(S, kind, shapes, ids=(0, 1, 2)):
    """w* of the family members ``ids`` by the batch Newton solve from 800 (once per module)."""
    key = (kind, shapes, tuple(ids))
    if key not in _solved:
        res = S.solve_batch(family(S, kind, ids), shapes, **NEWTON)
        assert np.all(res.status == 0), res.status
        _solved[key] = res.w
    return _solved[key]


def priced3(S, kind, shapes):
    """B = 3, κ = 2, κ_ts = 0, stationary weights, rtol 1e-12, with grids: (w, BatchPrices), once per module."""
    key = (kind, shapes)
    if key not in _priced:
        w = solved(S, kind, shapes)
        _priced[key] = (w, S.price_batch(family(S, kind, range(3)), shapes, w, kappa=KAPPA, n_max=n_max_of(shapes),
                                         rtol=1e-12, return_grids=True))
    return _priced[key]


def oracle_member(S, kind, shapes, b, w):
    """The oracle's view of family member b at w (``w`` is part of the key by identity of the module's caches)."""
    key = (kind, shapes, b)
    if key not in _members:
        m = package_model(S, kind, member(kind, b))
        _members[key] = bpo.Member(kind, shapes, m, bpo.discretize(S, kind, m, shapes), w)
    assert _members[key].w is w or np.array_equal(_members[key].w, w)
    return _members[key]


def dense_claim(mem, key):
    """(v, ‖(I − K)⁻¹‖∞) of the dense K_κ: K ≥ 0 with r(K) < 1, so (I − K)⁻¹ = Σ Kⁿ ≥ 0 and its ∞-norm is the
    largest entry of (I − K)⁻¹·1: two right-hand sides of one LU."""
    if key not in _dense:
        Kd = mem.dense(1, mem.theta, KAPPA - mem.gamma)
        N = Kd.shape[0]
        sol = np.linalg.solve(np.eye(N) - Kd, np.stack([Kd.sum(axis=1), np.ones(N)], axis=1))
        assert np.all(sol > 0), "K is not a contraction here"
        _dense[key] = (sol[:, 0].reshape(mem.shapes), float(sol[:, 1].max()))
    return _dense[key]


def rel_err(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


# ---------------------------------------------------------------- 1: E_M and E_M2
@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_sdf_moment_grids(S, kind, shapes):
    """E_M and E_M2 against folded_K·1 per member: max relative error <= 1e-12 (the bound test_hip_pricing.py holds the
    tilted product to)."""
    w, res = priced3(S, kind, shapes)
    assert res.plan == "batch" and np.all(res.status == 0), (res.plan, res.status)
    for b in range(3):
        mem = oracle_member(S, kind, shapes, b, w[b])
        e1, e2 = rel_err(res.grids["E_M"][b], mem.E_M()), rel_err(res.grids["E_M2"][b], mem.E_M2())
        print(f"{kind} {shapes} member {b}: E_M {e1:.2e}, E_M2 {e2:.2e}")
        assert e1 <= 1e-12 and e2 <= 1e-12, (b, e1, e2)


# ---------------------------------------------------------------- 2: the claim's true residual
@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_claim_true_residual(S, kind, shapes):
    """|K1 - (v - K v)|_2 / |K1|_2 <= 1e-10 with K by the oracle (the bound of test_true_residual for the same
    BiCGSTAB); max|T w - w| <= 1e-9; v > 0; status 0; and the applications the stage list implies."""
    w, res = priced3(S, kind, shapes)
    assert np.all(res.status == 0), res.status
    for b in range(3):
        mem = oracle_member(S, kind, shapes, b, w[b])
        v = res.grids["pd"][b]
        r, k1 = mem.claim_residual(v, KAPPA)
        true = np.linalg.norm(r) / np.linalg.norm(k1)
        print(f"{kind} {shapes} member {b}: {res.n_iter[b]} iterations, {res.n_apply[b]} applications, true residual "
              f"{true:.3e}, reported {res.rel_resid[b]:.3e}, resid_T {res.resid_T[b]:.3e}, {res.n_horizons[b]} horizons")
        assert true <= 1e-10, (b, true)
        assert res.resid_T[b] <= 1e-9, (b, res.resid_T[b])
        assert np.all(v > 0) and res.moments[b, 11] == 0.0
        # stage 0: L, K1, the iterations (two applications each, one where a sweep ends on |s|^2), K1 and K v per
        # residual check (one plus at most two restarts); stages 1-3: L and one application; stage 4: L and the horizons
        assert res.n_horizons[b] == n_max_of(shapes)
        rest = res.n_apply[b] - 2 - 6 - (1 + res.n_horizons[b])
        n = res.n_iter[b]
        assert n > 0 and any(2 * n - s <= rest - 2 * s <= 2 * n for s in (1, 2, 3)), (b, n, res.n_apply[b])


# ---------------------------------------------------------------- 3: against dense numpy
@pytest.mark.parametrize("kind,shapes", SMALL)
def test_claim_against_dense_solve(S, kind, shapes):
    """v against np.linalg.solve(I - K, K1): (I - K)(v - v_dense) = -r_true, so |v - v_dense| <= |(I - K)^-1|_inf
    |r_true|_inf; the test allows 4 times that plus 1e-12 max v for the rounding of the dense side.  ER = K0(1 + v) / v
    with K0 = K(0, 0, kappa) then moves by at most dv (|K0 1|_inf + max ER) / min v, plus 1e-12 max ER for the product's
    own rounding (test 1's bound); lp = ln ER + ln E_M by at most dER / min ER plus 2e-12."""
    w, res = priced3(S, kind, shapes)
    for b in range(3):
        mem = oracle_member(S, kind, shapes, b, w[b])
        v_ref, inv_norm = dense_claim(mem, (kind, shapes, b))
        v, ER = res.grids["pd"][b], res.grids["expected_return"][b]
        r, _ = mem.claim_residual(v, KAPPA)
        dv = 4.0 * inv_norm * np.max(np.abs(r)) + 1e-12 * v_ref.max()
        err_v = np.max(np.abs(v - v_ref))
        ER_ref = mem.ER(v_ref, KAPPA)
        k0 = mem.K(np.ones(shapes), 0, 0.0, KAPPA)
        dER = dv * (k0.max() + ER_ref.max()) / v_ref.min() + 1e-12 * ER_ref.max()
        err_ER = np.max(np.abs(ER - ER_ref))
        gw = bpo.point_weights(S.stationary_weights(mem.model, shapes))
        lp_ref = np.sum(gw * (np.log(ER_ref) + np.log(mem.E_M()))) / gw.sum()
        dlp = dER / ER_ref.min() + 2e-12
        err_lp = abs(res.stats["log_premium_mean"][b] - lp_ref)
        print(f"{kind} {shapes} member {b}: |inv| {inv_norm:.1f}, v {err_v:.2e} (bound {dv:.2e}), ER {err_ER:.2e} "
              f"(bound {dER:.2e}), lp {err_lp:.2e} (bound {dlp:.2e})")
        assert err_v <= dv, (b, err_v, dv)
        assert err_ER <= dER, (b, err_ER, dER)
        assert err_lp <= dlp, (b, err_lp, dlp)


# ---------------------------------------------------------------- 4: the words of the device's own grids
@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_words_against_numpy_restatement(S, kind, shapes):
    """The 12 words against the restatement evaluated on the device's own grids: within 1e-11 sum|terms| per word (the
    gradient tests' bound for fixed-order sums of <= 16 384 terms); words 9-11 exactly."""
    w, res = priced3(S, kind, shapes)
    for b in range(3):
        m = package_model(S, kind, member(kind, b))
        gw = bpo.point_weights(S.stationary_weights(m, shapes))
        g = res.grids
        want, scale = bpo.words(gw, g["E_M"][b], g["E_M2"][b], g["pd"][b], g["expected_return"][b])
        got = res.moments[b]
        err = np.abs(got[:9] - want[:9]) / scale[:9]
        print(f"{kind} {shapes} member {b}: worst word {int(np.argmax(err))} at {err.max():.2e} of sum|terms|")
        assert np.all(err <= 1e-11), (b, err)
        assert np.array_equal(got[9:], want[9:]), (b, got[9:], want[9:])
    stats = S.price_words_to_stats(res.moments)
    for k in stats:
        assert np.array_equal(stats[k], res.stats[k]), k


# ---------------------------------------------------------------- 5: horizons
def check_horizons(S, kind, shapes, res, w, kappa_ts, per_axis_of):
    n_max = res.price.shape[1]
    assert np.all(res.n_horizons == n_max), res.n_horizons
    for b in range(3):
        mem = oracle_member(S, kind, shapes, b, w[b])
        rows = mem.horizons(float(np.broadcast_to(kappa_ts, 3)[b]), n_max, bpo.point_weights(per_axis_of(mem.model)))
        np.testing.assert_allclose(res.price[b], rows[:, 0], rtol=1e-12)
        np.testing.assert_allclose(res.yield_[b], rows[:, 1], rtol=1e-12, atol=YIELD_ATOL)
        np.testing.assert_allclose(res.bracket[b], rows[:, 2:4], rtol=1e-12)


@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_horizons_stationary_weights(S, kind, shapes):
    """n_max = 50 at the small shapes, 8 at the larger ones, real bonds, against repeated folded_K: rtol 1e-12 on price,
    yield and bracket, the yield with the absolute term of test_term_structure_vs_dense_matrix_powers (YIELD_ATOL)."""
    w, res = priced3(S, kind, shapes)
    check_horizons(S, kind, shapes, res, w, 0.0, lambda m: S.stationary_weights(m, shapes))


@pytest.mark.parametrize("kind,shapes", SMALL)
def test_horizons_one_hot_weights_and_strips(S, kind, shapes):
    """One-hot weights (a state index per axis), and kappa_ts per member in {0, 1} (bonds and consumption strips)."""
    w = solved(S, kind, shapes)
    models = family(S, kind, range(3))
    state = [n // 2 for n in shapes]
    res = S.price_batch(models, shapes, w, n_max=50, weights=state)
    assert np.all(res.status == 0) and np.all(res.n_iter == 0) and np.all(np.isnan(res.moments[:, 4:]))

    def one_hot(m):
        return [np.eye(n)[i] for n, i in zip(shapes, state)]
    check_horizons(S, kind, shapes, res, w, 0.0, one_hot)
    assert np.all(res.moments[:, 0] == 1.0)
    kts = np.array([0.0, 1.0, 1.0])
    res = S.price_batch(models, shapes, w, n_max=50, kappa_ts=kts)
    check_horizons(S, kind, shapes, res, w, kts, lambda m: S.stationary_weights(m, shapes))


# ---------------------------------------------------------------- 6: the single-problem path
@pytest.mark.parametrize("kind,shapes", [("ssy", (5,) * 4), ("gcy", (4,) * 6)])
def test_against_single_problem_path(S, kind, shapes):
    """E_M within 1e-12 of sdf_moments, prices and yields within 1e-12 of term_structure, pd against
    claim_prices(rtol=1e-12) within the sum of the two solves' bounds of test 3."""
    w, res = priced3(S, kind, shapes)
    n_max = n_max_of(shapes)
    for b in range(3):
        m = package_model(S, kind, member(kind, b))
        sm = S.sdf_moments(m, shapes, w[b])
        assert rel_err(res.grids["E_M"][b], sm["E_M"]) <= 1e-12
        ts = S.term_structure(m, shapes, w[b], n_max)
        np.testing.assert_allclose(res.price[b], ts["price"], rtol=1e-12)
        np.testing.assert_allclose(res.yield_[b], ts["yield"], rtol=1e-12, atol=YIELD_ATOL)
        cp = S.claim_prices(m, shapes, w[b], KAPPA, rtol=1e-12)
        mem = oracle_member(S, kind, shapes, b, w[b])
        v_ref, inv_norm = dense_claim(mem, (kind, shapes, b))
        bound = 0.0
        for v in (res.grids["pd"][b], cp["pd"]):
            r, _ = mem.claim_residual(v, KAPPA)
            bound += 4.0 * inv_norm * np.max(np.abs(r)) + 1e-12 * v_ref.max()
        err = np.max(np.abs(res.grids["pd"][b] - cp["pd"]))
        print(f"{kind} {shapes} member {b}: pd differs by {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (b, err, bound)


# ---------------------------------------------------------------- 7: independence, bit for bit
def same_member(a, i, b, j, grids=True):
    ok = (np.array_equal(a.moments[i], b.moments[j], equal_nan=True) and np.array_equal(a.price[i], b.price[j])
          and np.array_equal(a.yield_[i], b.yield_[j]) and np.array_equal(a.bracket[i], b.bracket[j])
          and a.n_iter[i] == b.n_iter[j] and a.n_apply[i] == b.n_apply[j] and a.n_horizons[i] == b.n_horizons[j]
          and a.rel_resid[i] == b.rel_resid[j] and a.resid_T[i] == b.resid_T[j] and a.status[i] == b.status[j])
    if grids:
        ok = ok and all(np.array_equal(a.grids[k][i], b.grids[k][j]) for k in GRIDS)
    return ok


@pytest.mark.parametrize("kind,shapes", [("ssy", (5,) * 4), ("gcy", (4,) * 6)])
def test_member_bits_do_not_depend_on_the_batch(S, kind, shapes):
    """Member 1's grids, words, horizons and counts: B = 3 at place 1, B = 1, B = 5 at place 3; check_every 1, 3 and the
    default; with and without the grids; two identical calls."""
    w, ref = priced3(S, kind, shapes)
    kw = dict(kappa=KAPPA, n_max=n_max_of(shapes), rtol=1e-12)
    one = S.price_batch(family(S, kind, [1]), shapes, w[1:2], return_grids=True, **kw)
    assert same_member(ref, 1, one, 0)
    ids = [3, 4, 0, 1, 2]
    w5 = np.concatenate([solved(S, kind, shapes, (3, 4)), w])
    five = S.price_batch(family(S, kind, ids), shapes, w5, return_grids=True, **kw)
    assert same_member(ref, 1, five, 3) and same_member(ref, 0, five, 2) and same_member(ref, 2, five, 4)
    for ce in (1, 3):
        res = S.price_batch(family(S, kind, range(3)), shapes, w, return_grids=True, check_every=ce, **kw)
        assert all(same_member(ref, b, res, b) for b in range(3)), ce
    bare = S.price_batch(family(S, kind, range(3)), shapes, w, **kw)
    assert bare.grids is None and all(same_member(ref, b, bare, b, grids=False) for b in range(3))
    again = S.price_batch(family(S, kind, range(3)), shapes, w, return_grids=True, **kw)
    assert all(same_member(ref, b, again, b) for b in range(3))


# ---------------------------------------------------------------- 8: a member without a finite price
def test_member_without_a_finite_price(S):
    """kappa = 8 has r(K) of 1.003-1.006 for every family member at SSY (3,4,3,5): status 3 for that member alone."""
    kind, shapes = "ssy", (3, 4, 3, 5)
    w, ref = priced3(S, kind, shapes)
    models = family(S, kind, range(3))
    res = S.price_batch(models, shapes, w, kappa=[2.0, 8.0, 2.0], n_max=n_max_of(shapes), rtol=1e-12, return_grids=True)
    assert list(res.status) == [0, S._lib.SDFS_BATCH_NO_PRICE, 0] and S._lib.SDFS_BATCH_NO_PRICE == 3
    assert np.all(np.isnan(res.moments[1, 4:9])) and np.all(np.isfinite(res.moments[1, :4]))
    assert res.moments[1, 11] >= 1 and res.moments[1, 9] <= 0.0 and np.isfinite(res.moments[1, 10])
    assert np.array_equal(res.grids["E_M"][1], ref.grids["E_M"][1]) and np.all(np.isfinite(res.grids["E_M"][1]))
    assert np.all(np.isnan(res.grids["expected_return"][1])) and np.sum(~(res.grids["pd"][1] > 0)) == res.moments[1, 11]
    assert res.n_horizons[1] == n_max_of(shapes) and np.array_equal(res.price[1], ref.price[1])
    assert np.isnan(res.stats["log_pd_mean"][1]) and np.isfinite(res.stats["log_rf_mean"][1])
    assert same_member(ref, 0, res, 0) and same_member(ref, 2, res, 2)
    none = S.price_batch(models, shapes, w, kappa=None, n_max=n_max_of(shapes), rtol=1e-12, return_grids=True)
    assert np.all(none.status == 0) and np.all(none.n_iter == 0) and np.all(np.isnan(none.moments[:, 4:]))
    assert np.array_equal(none.grids["E_M"], ref.grids["E_M"]) and np.array_equal(none.moments[:, :4], ref.moments[:, :4])
    assert np.all(np.isnan(none.grids["pd"])) and np.all(np.isnan(none.rel_resid))
    assert np.array_equal(none.price, ref.price)


# ---------------------------------------------------------------- 9: the loop plan
def test_loop_plan_beyond_one_cu(S):
    """SSY 12^4 (20 736 points) does not fit one CU: the three single-problem functions member by member, reduced on the
    host.  The horizons price the claim's own strips (kappa_ts = kappa), so their last bracket bounds r(K) of the solve."""
    kind, shapes, n_max = "ssy", (12,) * 4, 400
    assert S.batch_lds_bytes(kind, shapes) is None
    models = family(S, kind, range(2))
    w = S.solve_batch(models, shapes, **NEWTON).w
    res = S.price_batch(models, shapes, w, kappa=KAPPA, n_max=n_max, kappa_ts=KAPPA, rtol=1e-12, return_grids=True)
    assert res.plan == "loop" and np.all(res.status == 0)
    assert np.all(res.n_iter == -1) and np.all(res.n_apply == -1) and np.all(np.isnan(res.rel_resid))
    assert np.all(res.n_horizons == n_max)
    assert np.all(res.bracket[:, -1, 1] < 1.0), res.bracket[:, -1]
    stats = S.price_words_to_stats(res.moments)
    assert all(np.array_equal(stats[k], res.stats[k]) and np.all(np.isfinite(stats[k])) for k in stats)
    for b, m in enumerate(models):
        gw = bpo.point_weights(S.stationary_weights(m, shapes))
        sm = S.sdf_moments(m, shapes, w[b])
        cp = S.claim_prices(m, shapes, w[b], KAPPA, rtol=1e-12)
        ts = S.term_structure(m, shapes, w[b], n_max, KAPPA)
        E_M2 = (sm["max_sharpe"] ** 2 + 1.0) * sm["E_M"] ** 2
        want, scale = bpo.words(gw, sm["E_M"], E_M2, cp["pd"], cp["expected_return"])
        assert np.all(np.abs(res.moments[b, :9] - want[:9]) <= 1e-12 * scale[:9])
        assert np.array_equal(res.moments[b, 9:], want[9:])
        assert np.array_equal(res.price[b], ts["price"]) and np.array_equal(res.yield_[b], ts["yield"])
        assert np.array_equal(res.bracket[b], ts["bracket"])
        assert np.array_equal(res.grids["pd"][b], cp["pd"])


# ---------------------------------------------------------------- 10: the handle's state
@pytest.mark.parametrize("kind,shapes", [("ssy", (5,) * 4), ("gcy", (4,) * 6)])
def test_price_leaves_the_handle_alone(S, kind, shapes):
    """solve, adjoint and apply on a BatchOperator give identical bits before and after price, also after a price whose
    launches ran out of budget mid-solve (check_every = 1)."""
    w = solved(S, kind, shapes)
    g = 0.5 + np.random.default_rng(5).random((3,) + shapes)
    w0 = np.full((3,) + shapes, 800.0)
    op = S.BatchOperator.from_models(family(S, kind, range(3)), shapes)

    def snapshot():
        out = list(op.solve(w0, **NEWTON)) + list(op.adjoint(w, g, rtol=1e-12, return_adjoint=True)) + list(op(w, True))
        return [np.asarray(x) for x in out]
    try:
        before = snapshot()
        first = op.price(w, KAPPA, 8, rtol=1e-12)
        mid = snapshot()
        second = op.price(w, KAPPA, 8, rtol=1e-12, check_every=1)
        after = snapshot()
    finally:
        op.close()
    for a, b in zip(first, second):
        assert a is None and b is None or np.array_equal(a, b, equal_nan=True)
    for x, y, z in zip(before, mid, after):
        assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True)

"""
GPU tests of continuous-state pricing (csrc/cont_price.hpp, the C_K0 / C_K1 / C_K2 forms of csrc/cont_kernel.hpp,
sdfs_via_autodiff_amd/pricing.py ``sdf_moments_continuous`` / ``term_structure_continuous`` /
``claim_prices_continuous``) against the numpy twin tests/cont_pricing_oracle.py.  The input conditions
(gather paths of the operator cases, spectral radii and condition numbers of the claim cases) are pinned on the CPU by
tests/test_cont_pricing_cpu.py.

BOUNDS.  One application: rtol 1e-12 for a positive f, |got − want| ≤ 1e-11 · K|f| for a signed one -- what
tests/test_hip_continuous_paths.py holds T and J·v to; the sums have the same length and one factor more.  n
applications: n times that.  The perpetual claim at rtol = 1e-12: max|Δ| / max|v| ≤ 10 · cond₂(I − K_twin) · rtol, the
perturbation bound of the solve with a factor 10 for the last-bit differences of the two matrices; cond₂ is computed
here.  ``expected_return`` is held to that bound plus 1e-12 by the same measure; ``log_premium`` = log E_x[R] + log E_x[M]
is a sum of logs of numbers near 1, where the absolute error of a log is the relative error of its argument, so it is
held to that bound plus 1e-12 absolutely (relative to max|ref| where that exceeds 1).
"""
import ctypes as C
import signal

import numpy as np
import pytest

import cont_boxes as CB
import cont_pricing_oracle as cp
import cont_sim_cases as CC
import cont_sim_oracle as co
from oracle import continuous as OC
from test_hip_cont_simulation import fixed_point, device_sdf_mean

pytestmark = pytest.mark.gpu

RTOL_POS, RTOL_SIGNED = 1e-12, 1e-11
SOLVE_RTOL = 1e-12
KAPPAS = (0.0, 1.0, 2.0, 6.0)
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


def to_dev(op, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.device("cuda", op.device))


def k_apply(op, w, setting, f):
    """K(p, κ_λ, κ_c) f on the device, host arrays in and out (w may be None for p = 0)."""
    import torch
    p, kl, kc = setting
    wd = None if w is None else to_dev(op, w)
    fd = to_dev(op, f)
    out = torch.empty_like(fd)
    torch.cuda.synchronize()
    op.cont_set_tilt_dev(None if wd is None else wd.data_ptr(), p, kl, kc)
    op.cont_apply_tilted_dev(fd.data_ptr(), out.data_ptr())
    op.synchronize()
    return out.cpu().numpy()


# -- the operator cases --------------------------------------------------------------------------------------------------
_CASE = {}


def operator_case(S, name):
    """(operator, kind, params, grids, w, settings, f_pos, f_signed, twin: {(setting index, "pos" | "signed" | "abs")})."""
    if name not in _CASE:
        case = cp.CASES[cp.CASE_IDS.index(name)]
        kind, params, grids, nodes, weights = CB.make_case(case)
        par = tuple(float(q) for q in params)
        op = S.ContinuousOperator(np.array(par), grids, nodes, weights)
        w = CC.smooth_w(grids)
        rng = np.random.default_rng(500 + cp.CASE_IDS.index(name))
        fs = {"pos": 0.5 + rng.random(case[2]), "signed": rng.standard_normal(case[2])}
        fs["abs"] = np.abs(fs["signed"])
        settings = cp.settings_of(kind, par)
        keys = [(s, k) for s in range(3) for k in ("pos", "signed", "abs")]
        outs = cp.apply(kind, par, grids, w, [fs[k] for _, k in keys], nodes, weights, [settings[s] for s, _ in keys])
        _CASE[name] = (op, kind, par, grids, w, settings, fs, dict(zip(keys, outs)))
    return _CASE[name]


@pytest.mark.parametrize("name", cp.CASE_IDS)
def test_operator_matches_the_twin_on_every_gather_path(S, name):
    op, _, _, _, w, settings, fs, twin = operator_case(S, name)
    for s, setting in enumerate(settings):
        got = k_apply(op, w if setting[0] else None, setting, fs["pos"])
        want = twin[(s, "pos")]
        err = np.max(np.abs(got - want) / np.abs(want))
        print(f"{name} p = {setting[0]}: positive f rel err {err:.3e}")
        assert np.all(want > 0) and err <= RTOL_POS, (name, setting, err)
        got = k_apply(op, w, setting, fs["signed"])
        ratio = np.max(np.abs(got - twin[(s, "signed")]) / twin[(s, "abs")])
        print(f"{name} p = {setting[0]}: signed f |err| / K|f| {ratio:.3e}")
        assert ratio <= RTOL_SIGNED, (name, setting, ratio)


@pytest.mark.parametrize("name", ["A4", "A6"])
def test_operator_at_a_constant_w_is_the_closed_form(S, name):
    op, kind, par, grids, w, settings, _, _ = operator_case(S, name)
    case = cp.CASES[cp.CASE_IDS.index(name)]
    n1, w1 = OC.qnwnorm([case[4][1]])
    c = 650.0
    for setting in settings:
        got = k_apply(op, np.full(w.shape, c), setting, np.ones(w.shape))
        want = cp.closed_form_constant_w(kind, par, grids, c, n1[:, 0], w1, *setting)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_apply_is_deterministic(S):
    for name in ("A4", "C6"):
        op, _, _, _, w, settings, fs, _ = operator_case(S, name)
        for setting in settings:
            a, b = k_apply(op, w, setting, fs["signed"]), k_apply(op, w, setting, fs["signed"])
            assert np.array_equal(a, b)


# -- the fixed points of cont_sim_cases ---------------------------------------------------------------------------------
_TWIN = {}


def grid_twin(S, grid):
    """The dense twin at the device's own w of one grid: {"K1": {κ: K(1, θ, κ−γ)}, "K0": {κ: K(0, 0, κ)}, "EM"}."""
    if grid not in _TWIN:
        model, par, grids, op, w, em = fixed_point(S, *grid)
        theta, _, gamma = co.pieces(grid[0], par)[:3]
        settings = [(1, theta, k - gamma) for k in KAPPAS] + [(0, 0.0, k) for k in KAPPAS]
        Ks = cp.dense(grid[0], par, grids, w, op.nodes, op.weights, settings)
        _TWIN[grid] = {"K1": dict(zip(KAPPAS, Ks[:4])), "K0": dict(zip(KAPPAS, Ks[4:])), "EM": em}
    return _TWIN[grid]


@pytest.mark.parametrize("grid", CC.GRIDS, ids=GRID_IDS)
def test_sdf_moments_against_the_sdf_mean_of_the_same_operator(S, grid):
    model, par, grids, op, w, em = fixed_point(S, *grid)
    out = S.sdf_moments_continuous(model, grids, w, operator=op)
    np.testing.assert_allclose(out["E_M"], device_sdf_mean(op, w), rtol=1e-13, atol=0)
    np.testing.assert_allclose(out["log_rf"], -np.log(out["E_M"]), rtol=0, atol=0)
    theta, _, gamma = co.pieces(grid[0], par)[:3]
    em2 = cp.apply(grid[0], par, grids, w, np.ones(w.shape), op.nodes, op.weights, [(2, 2 * theta, -2 * gamma)])[0]
    assert np.all(em2 / em ** 2 > 1.0)
    np.testing.assert_allclose(out["max_sharpe"] ** 2 + 1.0, em2 / em ** 2, rtol=4e-12, atol=0)   # two applications and a square


@pytest.mark.parametrize("grid", [g for g in CC.GRIDS if g not in CC.NO_FIXED_POINT],
                         ids=[CC.tag(*g) for g in CC.GRIDS if g not in CC.NO_FIXED_POINT])
def test_k1_at_one_minus_gamma_is_the_handles_jacobian(S, grid):
    model, par, grids, op, w, _ = fixed_point(S, *grid)
    theta, _, gamma = co.pieces(grid[0], par)[:3]
    f = np.random.default_rng(7).standard_normal(w.shape)
    got = k_apply(op, w, (1, theta, 1.0 - gamma), f)
    resid = np.max(np.abs(op(w) - w))
    bound = (2.0 * abs(theta - 1.0) * resid / (np.min(w) - 1.0) + 1e-12) * op.jvp(w, np.abs(f))
    assert np.all(np.abs(got - op.jvp(w, f)) <= bound)


def test_set_tilt_leaves_the_cached_linearisation_alone(S):
    import torch
    model, par, grids, op, w, _ = fixed_point(S, *CC.GRIDS[0])
    theta, _, gamma = co.pieces(CC.GRIDS[0][0], par)[:3]
    wd, vd = to_dev(op, w), to_dev(op, np.random.default_rng(3).standard_normal(w.shape))
    other = to_dev(op, CC.smooth_w(grids))
    a, b, tmp = torch.empty_like(wd), torch.empty_like(wd), torch.empty_like(wd)
    torch.cuda.synchronize()
    op.linearize_dev(wd.data_ptr())
    op.jvp_dev(vd.data_ptr(), a.data_ptr())
    for p, kl, kc in ((1, theta, 1.5 - gamma), (2, 2 * theta, -2 * gamma), (0, 0.0, 1.0)):
        op.cont_set_tilt_dev(other.data_ptr(), p, kl, kc)
        op.cont_apply_tilted_dev(vd.data_ptr(), tmp.data_ptr())
    op.jvp_dev(vd.data_ptr(), b.data_ptr())
    op.synchronize()
    assert torch.equal(a, b)
    # set_tilt copies w: the caller's buffer is free afterwards
    op.cont_set_tilt_dev(wd.data_ptr(), 1, theta, -gamma)
    op.synchronize()
    keep = wd.clone()
    wd.fill_(float("nan"))
    torch.cuda.synchronize()
    one = torch.ones_like(wd)
    op.cont_apply_tilted_dev(one.data_ptr(), tmp.data_ptr())
    op.synchronize()
    np.testing.assert_allclose(tmp.cpu().numpy(), device_sdf_mean(op, keep.cpu().numpy()), rtol=1e-13, atol=0)


# -- the C ABI's refusals --------------------------------------------------------------------------------------------------
def test_c_abi_refusals(S):
    import torch
    from sdfs_via_autodiff_amd import _lib
    lib = _lib.lib
    ARG, UNSUP = _lib.SDFS_ERR_ARG, _lib.SDFS_ERR_UNSUPPORTED
    nan, inf = float("nan"), float("inf")
    dp = C.POINTER(C.c_double)
    price, bracket = np.empty((4, 1)), np.empty((4, 2))
    xq = np.zeros((4, 1))
    no_i64, no_ptr = (C.c_int64 * 1)(0), (C.c_void_p * 1)(0)

    def horizons(h, n_max, ns=0, sat=no_i64, sp=no_ptr):
        return lib.sdfs_cont_tilted_horizons_dev(h, n_max, xq.ctypes.data_as(dp), 1, ns, sat, sp, price.ctypes.data_as(dp),
                                                 bracket.ctypes.data_as(dp))

    # a discretised handle
    ssy = S.SSY()
    shapes = (2, 3, 4, 5)
    disc = S.ssy_operator(shapes, ssy.params, S.discretize_ssy(ssy, shapes))
    g = torch.ones(shapes, dtype=torch.float64, device="cuda")
    o = torch.empty_like(g)
    torch.cuda.synchronize()
    assert lib.sdfs_cont_set_tilt_dev(disc._h, g.data_ptr(), 1, 1.0, 1.0) == UNSUP
    assert "continuous-state handles only" in _lib.last_error(disc._h)
    assert lib.sdfs_cont_apply_tilted_dev(disc._h, g.data_ptr(), o.data_ptr()) == UNSUP
    assert lib.sdfs_cont_solve_tilted_dev(disc._h, None, g.data_ptr(), o.data_ptr(), None, None) == UNSUP
    assert horizons(disc._h, 4) == UNSUP

    # a continuous handle before any set_tilt
    grids = S.build_grid(ssy, *shapes)
    nodes, weights = S.qnwnorm([2] * 4)
    op = S.ContinuousOperator(np.array(ssy.params), grids, np.ascontiguousarray(nodes.T), weights)
    h = op._h
    w = 700.0 * g
    torch.cuda.synchronize()
    assert lib.sdfs_cont_apply_tilted_dev(h, g.data_ptr(), o.data_ptr()) == ARG
    assert "before sdfs_cont_set_tilt_dev" in _lib.last_error(h)
    assert lib.sdfs_cont_solve_tilted_dev(h, None, g.data_ptr(), o.data_ptr(), None, None) == ARG
    assert horizons(h, 4) == ARG
    # set_tilt's own arguments; a refused set_tilt leaves no tilt behind
    for p in (-1, 3):
        assert lib.sdfs_cont_set_tilt_dev(h, w.data_ptr(), p, 1.0, 1.0) == ARG
    for p in (1, 2):
        assert lib.sdfs_cont_set_tilt_dev(h, None, p, 1.0, 1.0) == ARG
    for kl, kc in ((nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, -inf)):
        assert lib.sdfs_cont_set_tilt_dev(h, w.data_ptr(), 1, kl, kc) == ARG
    assert lib.sdfs_cont_apply_tilted_dev(h, g.data_ptr(), o.data_ptr()) == ARG
    # with a tilt
    assert lib.sdfs_cont_set_tilt_dev(h, w.data_ptr(), 1, ssy.θ, -ssy.γ) == 0
    assert lib.sdfs_cont_apply_tilted_dev(h, g.data_ptr(), g.data_ptr()) == ARG
    assert lib.sdfs_cont_apply_tilted_dev(h, None, o.data_ptr()) == ARG
    assert lib.sdfs_cont_apply_tilted_dev(h, g.data_ptr(), None) == ARG
    assert lib.sdfs_cont_solve_tilted_dev(h, None, None, o.data_ptr(), None, None) == ARG
    for n_max in (0, -1, (1 << 24) + 1):
        assert horizons(h, n_max) == ARG
    sp = (C.c_void_p * 2)(o.data_ptr(), g.data_ptr())
    for sat in ((0, 1), (2, 2), (3, 2), (1, 5)):
        assert horizons(h, 4, 2, (C.c_int64 * 2)(*sat), sp) == ARG
    assert horizons(h, 4, 2, (C.c_int64 * 2)(1, 2), (C.c_void_p * 2)(o.data_ptr(), None)) == ARG
    assert horizons(h, 4, 1, None, sp) == ARG
    assert horizons(h, 4, -1) == ARG
    assert horizons(h, 4) == 0 and np.all(price > 0)
    op.synchronize()


# -- the perpetual claim ---------------------------------------------------------------------------------------------------
PAIRS = cp.claim_pairs()


@pytest.mark.parametrize("grid,kappa", PAIRS, ids=[f"{CC.tag(*g)}-kappa{k:g}" for g, k in PAIRS])
def test_claim_prices_against_the_dense_twin(S, grid, kappa):
    model, par, grids, op, w, _ = fixed_point(S, *grid)
    tw = grid_twin(S, grid)
    K = tw["K1"][kappa]
    r = cp.spectral_radius(K)
    assert r < 0.9998, r
    v, er, lp = cp.claim(K, tw["K0"][kappa], tw["EM"].ravel())
    bound = 10.0 * np.linalg.cond(np.eye(K.shape[0]) - K) * SOLVE_RTOL
    out = S.claim_prices_continuous(model, grids, w, kappa, rtol=SOLVE_RTOL, operator=op)
    again = S.claim_prices_continuous(model, grids, w, kappa, rtol=SOLVE_RTOL, operator=op)
    for key in ("pd", "expected_return", "log_premium"):
        assert np.array_equal(out[key], again[key]), key          # two runs, identical bits
    vmax = np.max(np.abs(v))
    e_pd = np.max(np.abs(out["pd"].ravel() - v)) / vmax
    e_er = np.max(np.abs(out["expected_return"].ravel() - er)) / np.max(np.abs(er))
    e_lp = np.max(np.abs(out["log_premium"].ravel() - lp)) / max(1.0, np.max(np.abs(lp)))
    print(f"{CC.tag(*grid)} kappa {kappa:g}: r(K) {r:.5f} bound {bound:.2e} pd {e_pd:.2e} E[R] {e_er:.2e} log premium {e_lp:.2e}")
    assert np.all(out["pd"] > 0)
    assert e_pd <= bound
    assert e_er <= bound + 1e-12
    assert e_lp <= bound + 1e-12
    if kappa == 1.0:
        twin_dev = np.max(np.abs(v - (w.ravel() - 1.0))) / vmax
        print(f"    the twin's own distance from w* - 1: {twin_dev:.2e}")
        assert np.max(np.abs(out["pd"] - (w - 1.0))) / vmax <= twin_dev + bound


REFUSED = cp.refused_pairs()


@pytest.mark.parametrize("grid,kappa", REFUSED, ids=[f"{CC.tag(*g)}-kappa{k:g}" for g, k in REFUSED])
def test_claim_prices_refuse_where_the_radius_exceeds_one(S, grid, kappa):
    model, par, grids, op, w, _ = fixed_point(S, *grid)
    assert cp.spectral_radius(grid_twin(S, grid)["K1"][kappa]) > 1.002
    with pytest.raises(ValueError, match="no finite price"):
        S.claim_prices_continuous(model, grids, w, kappa, rtol=SOLVE_RTOL, operator=op)


# -- the term structure ----------------------------------------------------------------------------------------------------
N_MAX, SAVE = 16, (1, 7, 16)


@pytest.mark.parametrize("kappa", [0.0, 1.0])
@pytest.mark.parametrize("grid", CC.GRIDS, ids=GRID_IDS)
def test_term_structure_against_the_dense_twin(S, grid, kappa):
    model, par, grids, op, w, _ = fixed_point(S, *grid)
    K = grid_twin(S, grid)["K1"][kappa]
    Ps = cp.powers_of_one(K, N_MAX)
    states = np.stack([np.zeros(len(grids)), CC.start_of(grids, "vector"), np.array([g[-1] if d % 2 else g[0] for d, g in enumerate(grids)])])
    out = S.term_structure_continuous(model, grids, w, N_MAX, kappa, states=states, save=SAVE, operator=op)
    again = S.term_structure_continuous(model, grids, w, N_MAX, kappa, states=states, save=SAVE, operator=op)
    for key in ("price", "yield", "bracket"):
        assert np.array_equal(out[key], again[key]), key          # two runs, identical bits
    for n in SAVE:
        assert np.array_equal(out["grids"][n], again["grids"][n])
    assert np.array_equal(out["horizons"], np.arange(1, N_MAX + 1))
    assert out["price"].shape == (N_MAX, 3) and out["bracket"].shape == (N_MAX, 2)
    xq = np.ascontiguousarray(states.T)
    rk = cp.spectral_radius(K)
    br = cp.brackets(Ps)
    for n in range(1, N_MAX + 1):
        want = OC.lin_interp(xq, Ps[n - 1].reshape(w.shape), grids)
        np.testing.assert_allclose(out["price"][n - 1], want, rtol=n * 1e-12, atol=0)
        np.testing.assert_allclose(out["bracket"][n - 1], br[n - 1], rtol=2 * n * 1e-12, atol=0)
        lo, hi = out["bracket"][n - 1]
        assert lo * (1 - 1e-10) <= rk <= hi * (1 + 1e-10), (n, lo, rk, hi)
    for n in SAVE:
        np.testing.assert_allclose(out["grids"][n], Ps[n - 1].reshape(w.shape), rtol=n * 1e-12, atol=0)
    np.testing.assert_allclose(out["yield"], -np.log(out["price"]) / np.arange(1, N_MAX + 1)[:, None], rtol=0, atol=0)
    # the default query state is the zero state
    zero = S.term_structure_continuous(model, grids, w, 3, kappa, operator=op)
    assert np.array_equal(zero["price"][:, 0], out["price"][:3, 0]) and zero["grids"] == {}


def test_term_structure_refuses_prices_that_leave_the_positive_numbers(S):
    (grid,) = CC.NO_FIXED_POINT
    model, par, grids, op, w, _ = fixed_point(S, *grid)
    with pytest.raises(ValueError, match="left the positive numbers"):
        S.term_structure_continuous(model, grids, w, 1000, 0.0, operator=op)


def test_public_functions_build_their_own_operator(S):
    """operator=None: the Gauss–Hermite rule of order d, as in ``simulate_continuous``."""
    grid = CC.GRIDS[0]
    model, par, grids, op, w, em = fixed_point(S, *grid)
    out = S.sdf_moments_continuous(model, grids, w, d=CC.QUAD_D)
    np.testing.assert_allclose(out["E_M"], em, rtol=1e-12, atol=0)
    a = S.claim_prices_continuous(model, grids, w, 1.0, rtol=SOLVE_RTOL, d=CC.QUAD_D)
    b = S.claim_prices_continuous(model, grids, w, 1.0, rtol=SOLVE_RTOL, operator=op)
    assert np.array_equal(a["pd"], b["pd"])

"""
GPU tests of asset pricing with the SDF at w* (sdfs_set_tilt_dev, sdfs_apply_tilted_dev, sdfs_solve_tilted_dev,
sdfs_tilted_horizons_dev; sdfs_via_autodiff_amd/pricing.py):

 (1) the tilted product K(p, κ_λ, κ_c) f against the oracle on every kernel plan: the numpy folded form of
     tests/test_pricing_cpu.py at small and medium grids; at GCY 16^6 and 20^6 the C oracle with its scale tables
     replaced by the tilted ones and θ = β = 1, so that T f − 1 = H_κ f;
 (2) J·v and the (1, θ, 1−γ) product are bit-identical;
 (3) the perpetual consumption claim's price–dividend ratio is w* − 1;
 (4) the term structure against dense matrix powers, the strip sandwich of w* − 1 at GCY 16^6, bit-identical reruns;
 (5) claim prices against dense numpy, the Euler equation, and the refusal when r(K) > 1;
 (6) the handle's own state (J·v, Newton, fp32 solve settings) is untouched by pricing calls;
 (7) the refusals.
Every test runs under its own time limit (SIGALRM).
"""
import contextlib
import ctypes as C
import os
import signal

import numpy as np
import pytest

from test_pricing_cpu import folded_K, oracle_T, pieces

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


@contextlib.contextmanager
def plan_env(which):
    old = os.environ.get("SDFS_PLAN")
    if which is None:
        os.environ.pop("SDFS_PLAN", None)
    else:
        os.environ["SDFS_PLAN"] = which
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SDFS_PLAN", None)
        else:
            os.environ["SDFS_PLAN"] = old


def model_of(S, kind):
    return S.SSY() if kind == "ssy" else S.GCY()


def disc(S, kind):
    return S.discretize_ssy if kind == "ssy" else S.discretize_gcy


def tilts(m):
    th, g = m.θ, m.γ
    return [(1, th, -g), (2, 2 * th, -2 * g), (1, th, 2 - g), (0, 0.0, 1.0)]


def dev(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    return t


def make_op(S, kind, shapes, m, arr, plan=None):
    import torch
    with plan_env(plan):
        op = S.KoopmansOperator(kind, shapes, m.params, arr)
    op.set_stream(torch.cuda.current_stream().cuda_stream)
    return op


def tilted(op, w, f, p, kl, kc):
    import torch
    wd, fd = dev(w), dev(f)
    out = torch.empty_like(fd)
    op.set_tilt_dev(wd.data_ptr() if w is not None else None, p, kl, kc)
    op.apply_tilted_dev(fd.data_ptr(), out.data_ptr())
    return out.cpu().numpy()


def c_oracle_K(kind, shapes, m, arr, w, Tw, f, p, kl, kc):
    """K f by the C oracle: H_κ u = T(u) − 1 with a1 = exp(κ_λ h_λ), a2 = exp(½κ_c²σ_c²), a3 = exp(κ_c(μ_c + z)) and
    θ = β = 1; u = c1^p f, scaled so that H_κ u >> 1 (no cancellation in the − 1)."""
    from oracle.c_oracle import COperator
    beta, theta, gamma, mu_c, _, _, _, _ = pieces(kind, m, arr)
    o = COperator(kind, shapes, m.params, arr)
    if kind == "ssy":
        hl, sc, z = arr[0], arr[8], arr[6]
    else:
        hl, sc, z = arr[13], arr[9], arr[0]
    o.a1 = np.ascontiguousarray(np.exp(kl * np.asarray(hl)))
    o.a2 = np.ascontiguousarray(np.exp(0.5 * kc * kc * np.asarray(sc) ** 2))
    o.a3 = np.ascontiguousarray(np.exp(kc * (mu_c + np.asarray(z))))
    o.theta, o.beta = 1.0, 1.0
    u = w ** (p * (theta - 1.0)) * f
    s = 1e6 / np.mean(u)
    Hu = (o(s * u) - 1.0) / s
    return (beta ** theta * (Tw - 1.0) ** (1.0 - theta)) ** p * Hu


# -- (1) the tilted product on every plan -------------------------------------------------------------------------------
PLAN_CASES = [
    ("ssy", (15, 15, 15, 15), None, "small-grid plan", False),
    ("ssy", (4, 7, 6, 5), "classic", None, False),
    ("gcy", (10,) * 6, None, "padded pair plan", False),
    ("gcy", (16,) * 6, None, "pair plan pass", True),
]
PLAN_IDS = ["ssy15-small", "ssy4765-generic", "gcy10-padded", "gcy16-pair"]


def assert_plan(op, marker):
    desc = op.describe_plan()
    if marker:
        assert marker in desc, desc
        if marker == "pair plan pass":
            assert "padded" not in desc, desc
    else:
        assert "pair plan" not in desc and "small-grid plan" not in desc, desc


@limit(900)
@pytest.mark.parametrize("kind,shapes,plan,marker,c_oracle", PLAN_CASES, ids=PLAN_IDS)
def test_tilted_product_vs_oracle(S, kind, shapes, plan, marker, c_oracle):
    tilted_product_case(S, kind, shapes, plan, marker, c_oracle)


def tilted_product_case(S, kind, shapes, plan, marker, c_oracle, m=None):
    """The body of test_tilted_product_vs_oracle; m: another model than the default.  Returns the worst relative error."""
    m = m or model_of(S, kind)
    arr = disc(S, kind)(m, shapes)
    worst = 0.0
    op = make_op(S, kind, shapes, m, arr, plan)
    assert_plan(op, marker)
    rng = np.random.default_rng(sum(shapes))
    w = 500.0 + 200.0 * rng.random(shapes)           # a non-constant w, not a fixed point
    f = 0.5 + rng.random(shapes)
    if c_oracle:
        from oracle.c_oracle import COperator
        Tw = COperator(kind, shapes, m.params, arr)(w)
    else:
        Tw = oracle_T(kind, shapes, m, arr, w)
    for p, kl, kc in tilts(m):
        got = tilted(op, w, f, p, kl, kc)
        if c_oracle:
            want = c_oracle_K(kind, shapes, m, arr, w, Tw, f, p, kl, kc)
        else:
            want = folded_K(kind, shapes, m, arr, w, f, p, kl, kc, Tw=Tw)
        rel = np.max(np.abs(got - want) / np.abs(want))
        assert rel <= 1e-12, f"{kind} {shapes} tilt {(p, kl, kc)}: {rel:.3e}"
        worst = max(worst, float(rel))
    op.close()
    return worst


@limit(900)
def test_tilted_product_gcy20_vs_c_oracle(S):
    shapes = (20,) * 6
    m = S.GCY()
    arr = S.discretize_gcy(m, shapes)
    op = make_op(S, "gcy", shapes, m, arr)
    assert "pair plan" in op.describe_plan()
    rng = np.random.default_rng(20)
    w = 500.0 + 200.0 * rng.random(shapes)
    f = 0.5 + rng.random(shapes)
    from oracle.c_oracle import COperator
    Tw = COperator("gcy", shapes, m.params, arr)(w)
    p, kl, kc = 1, m.θ, -m.γ
    got = tilted(op, w, f, p, kl, kc)
    want = c_oracle_K("gcy", shapes, m, arr, w, Tw, f, p, kl, kc)
    rel = np.max(np.abs(got - want) / np.abs(want))
    assert rel <= 1e-12, f"{rel:.3e}"
    op.close()


# -- (2) J.v is K(1, θ, 1−γ) bit for bit ----------------------------------------------------------------------------------
@limit(600)
@pytest.mark.parametrize("kind,shapes,plan,marker,c_oracle", PLAN_CASES, ids=PLAN_IDS)
def test_jvp_equals_consumption_tilt_bitwise(S, kind, shapes, plan, marker, c_oracle):
    import torch
    m = model_of(S, kind)
    arr = disc(S, kind)(m, shapes)
    op = make_op(S, kind, shapes, m, arr, plan)
    rng = np.random.default_rng(3)
    wd = dev(500.0 + 200.0 * rng.random(shapes))
    vd = dev(rng.standard_normal(shapes))
    a, b = torch.empty_like(wd), torch.empty_like(wd)
    op.set_tilt_dev(wd.data_ptr(), 1, m.θ, 1 - m.γ)          # (linearises at w)
    op.jvp_dev(vd.data_ptr(), a.data_ptr())
    op.apply_tilted_dev(vd.data_ptr(), b.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(a, b), f"max diff {float((a - b).abs().max()):.3e}"
    op.close()


# -- (3) the perpetual consumption claim -----------------------------------------------------------------------------------
def fixed_point(S, kind, shapes, m):
    """A tight Newton fixed point, computed on the operator pricing.py will use."""
    import torch
    from sdfs_via_autodiff_amd import _requests
    op, _ = _requests._operator(m, shapes)
    w = torch.full(shapes, 800.0, dtype=torch.float64, device="cuda")
    _, info = op.solve_dev(w.data_ptr(), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
    assert info["status"] == 0, info
    return w.cpu().numpy()


@limit(600)
@pytest.mark.parametrize("kind,shapes", [("ssy", (15,) * 4), ("gcy", (10,) * 6), ("gcy", (16,) * 6)],
                         ids=["ssy15", "gcy10", "gcy16"])
def test_consumption_claim_pd_is_w_star_minus_one(S, kind, shapes):
    m = model_of(S, kind)
    w = fixed_point(S, kind, shapes, m)
    out = S.claim_prices(m, shapes, w, 1.0, rtol=1e-12)
    rel = np.max(np.abs(out["pd"] - (w - 1.0)) / (w - 1.0))
    assert rel <= 1e-9, f"{rel:.3e}"
    assert np.all(np.isfinite(out["expected_return"])) and np.all(out["expected_return"] > 0)


# -- (4) term structure ----------------------------------------------------------------------------------------------------
def dense_of(kind, shapes, m, arr, w, p, kl, kc):
    N = int(np.prod(shapes))
    Tw = oracle_T(kind, shapes, m, arr, w)
    K = np.empty((N, N))
    for j in range(N):
        e = np.zeros(N)
        e[j] = 1.0
        K[:, j] = folded_K(kind, shapes, m, arr, w, e.reshape(shapes), p, kl, kc, Tw=Tw).reshape(N)
    return K


@limit(300)
@pytest.mark.parametrize("kappa", [0.0, 1.0])
def test_term_structure_vs_dense_matrix_powers(S, kappa):
    kind, shapes = "ssy", (3, 3, 3, 5)
    m = S.SSY()
    arr = S.discretize_ssy(m, shapes)
    w = fixed_point(S, kind, shapes, m)
    K = dense_of(kind, shapes, m, arr, w, 1, m.θ, kappa - m.γ)
    r = float(np.max(np.abs(np.linalg.eigvals(K))))
    for weights in (None, [1, 0, 2, 4]):
        gax = S.stationary_weights(m, shapes) if weights is None else \
            [np.eye(n)[i] for n, i in zip(shapes, weights)]
        g = gax[0]
        for x in gax[1:]:
            g = np.multiply.outer(g, x)
        g = g.reshape(-1)
        out = S.term_structure(m, shapes, w, 50, kappa=kappa, weights=weights, save=(1, 17, 50))
        P = np.ones(K.shape[0])
        for n in range(1, 51):
            Pn = K @ P
            ratio = Pn / P
            np.testing.assert_allclose(out["price"][n - 1], g @ Pn, rtol=1e-12)
            np.testing.assert_allclose(out["yield"][n - 1], g @ -np.log(Pn) / n, rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(out["bracket"][n - 1], [ratio.min(), ratio.max()], rtol=1e-12)
            if n in out["grids"]:
                np.testing.assert_allclose(out["grids"][n].reshape(-1), Pn, rtol=1e-12)
            P = Pn
        assert out["bracket"][-1, 0] <= r * (1 + 1e-12) and r <= out["bracket"][-1, 1] * (1 + 1e-12)
        assert list(out["horizons"]) == list(range(1, 51))


@limit(600)
def test_strip_sandwich_of_the_consumption_claim_gcy16(S):
    shapes = (16,) * 6
    m = S.GCY()
    w = fixed_point(S, "gcy", shapes, m)
    gax = S.stationary_weights(m, shapes)
    g = gax[0]
    for x in gax[1:]:
        g = np.multiply.outer(g, x)
    target = float(np.sum(g * (w - 1.0)))
    out = S.term_structure(m, shapes, w, 1000, kappa=1.0)
    widths = []
    for N in (200, 1000):
        S_N = float(np.sum(out["price"][:N]))
        PN = out["price"][N - 1]
        lo_r, hi_r = out["bracket"][N - 1]
        assert 0 < lo_r <= hi_r < 1, (N, lo_r, hi_r)
        lo = S_N + lo_r / (1 - lo_r) * PN
        hi = S_N + hi_r / (1 - hi_r) * PN
        assert lo <= target * (1 + 1e-9) and target <= hi * (1 + 1e-9), (N, lo, target, hi)
        widths.append(hi - lo)
    assert widths[1] < widths[0], widths
    # two identical runs give identical bits
    a = S.term_structure(m, shapes, w, 50, kappa=1.0, save=(50,))
    b = S.term_structure(m, shapes, w, 50, kappa=1.0, save=(50,))
    for k in ("price", "yield", "bracket"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["grids"][50], b["grids"][50])
    assert np.array_equal(a["price"], out["price"][:50])


# -- (5) claim prices --------------------------------------------------------------------------------------------------------
@limit(300)
def test_claim_prices_vs_dense_and_euler_equation(S):
    import torch
    kind, shapes = "ssy", (3, 3, 3, 5)
    m = S.SSY()
    arr = S.discretize_ssy(m, shapes)
    w = fixed_point(S, kind, shapes, m)
    kappa = 3.0
    K = dense_of(kind, shapes, m, arr, w, 1, m.θ, kappa - m.γ)
    K0 = dense_of(kind, shapes, m, arr, w, 0, 0.0, kappa)
    one = np.ones(K.shape[0])
    v = np.linalg.solve(np.eye(K.shape[0]) - K, K @ one)
    er = K0 @ (1 + v) / v
    out = S.claim_prices(m, shapes, w, kappa, rtol=1e-13)
    np.testing.assert_allclose(out["pd"].reshape(-1), v, rtol=1e-8)
    np.testing.assert_allclose(out["expected_return"].reshape(-1), er, rtol=1e-8)
    # Euler: K (1 + v) / v = 1 with the device's own K
    from sdfs_via_autodiff_amd import _requests
    op, _ = _requests._operator(m, shapes)
    wd, vd = dev(w), dev(out["pd"])
    num, res = torch.add(vd, 1.0), torch.empty_like(vd)
    op.set_tilt_dev(wd.data_ptr(), 1, m.θ, kappa - m.γ)
    op.apply_tilted_dev(num.data_ptr(), res.data_ptr())
    euler = (res / vd).cpu().numpy()
    assert np.max(np.abs(euler - 1.0)) <= 1e-10
    em = S.sdf_moments(m, shapes, w)
    np.testing.assert_allclose(out["log_premium"], np.log(out["expected_return"]) + np.log(em["E_M"]), rtol=1e-13)
    assert np.all(em["max_sharpe"] > 0) and np.all(np.isfinite(em["log_rf"]))
    with pytest.raises(ValueError, match="no finite price"):
        S.claim_prices(m, shapes, w, 8.0)


# -- (6) the handle's own state -----------------------------------------------------------------------------------------------
def pricing_calls(op, m, wd):
    """Every pricing entry point once; returns what they computed."""
    import torch
    f = torch.ones_like(wd)
    a, x = torch.empty_like(wd), torch.empty_like(wd)
    op.set_tilt_dev(wd.data_ptr(), 2, 2 * m.θ, -2 * m.γ)
    op.apply_tilted_dev(f.data_ptr(), a.data_ptr())
    op.set_tilt_dev(wd.data_ptr(), 1, m.θ, 1 - m.γ)
    op.solve_tilted_dev(a.data_ptr(), x.data_ptr(), 1e-10)
    op.set_tilt_dev(wd.data_ptr(), 1, m.θ, -m.γ)
    hz = op.tilted_horizons_dev(20, None)
    return a.cpu().numpy(), x.cpu().numpy(), hz


@limit(600)
@pytest.mark.parametrize("kind,shapes", [("ssy", (15,) * 4), ("gcy", (16,) * 6)], ids=["ssy15", "gcy16"])
def test_pricing_leaves_jvp_and_newton_bitwise_unchanged(S, kind, shapes):
    import torch
    m = model_of(S, kind)
    arr = disc(S, kind)(m, shapes)
    op = make_op(S, kind, shapes, m, arr)
    w0 = dev(np.full(shapes, 800.0))
    wa = w0.clone()
    op.solve_dev(wa.data_ptr(), "newton")
    v = dev(np.random.default_rng(1).standard_normal(shapes))
    ja, jb = torch.empty_like(v), torch.empty_like(v)
    op.linearize_dev(wa.data_ptr())
    op.jvp_dev(v.data_ptr(), ja.data_ptr())
    pricing_calls(op, m, wa)
    op.set_tilt_dev(wa.data_ptr(), 0, 0.0, 1.0)     # (last: a tilt at the linearisation point)
    op.jvp_dev(v.data_ptr(), jb.data_ptr())
    wb = w0.clone()
    op.solve_dev(wb.data_ptr(), "newton")
    torch.cuda.synchronize()
    assert torch.equal(ja, jb)
    assert torch.equal(wa, wb)
    op.close()


@limit(600)
def test_pricing_is_fp64_whatever_the_solve_settings(S):
    import torch
    kind, shapes = "gcy", (16,) * 6
    m = S.GCY()
    arr = S.discretize_gcy(m, shapes)
    a_op = make_op(S, kind, shapes, m, arr)
    b_op = make_op(S, kind, shapes, m, arr)
    w = dev(np.full(shapes, 800.0))
    b_op.solve_dev(w.data_ptr(), "newton", tol=1e-9)
    w32 = dev(np.full(shapes, 800.0))
    a_op.solve_dev(w32.data_ptr(), "newton", krylov_f32=3)
    wt = dev(np.full(shapes, 800.0))
    a_op.solve_dev(wt.data_ptr(), "successive_approx", t_f32=1, max_iter=5)
    ra = pricing_calls(a_op, m, w)
    rb = pricing_calls(b_op, m, w)
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    # the fp32 solves still give what they gave before
    w32b = dev(np.full(shapes, 800.0))
    a_op.solve_dev(w32b.data_ptr(), "newton", krylov_f32=3)
    wtb = dev(np.full(shapes, 800.0))
    a_op.solve_dev(wtb.data_ptr(), "successive_approx", t_f32=1, max_iter=5)
    torch.cuda.synchronize()
    assert torch.equal(w32, w32b) and torch.equal(wt, wtb)
    a_op.close()
    b_op.close()


# -- (7) refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(S):
    import torch
    from sdfs_via_autodiff_amd import _lib
    shapes = (3, 4, 2, 3, 5, 4)
    m = S.GCY()
    arr = S.discretize_gcy(m, shapes)
    op = make_op(S, "gcy", shapes, m, arr)
    wd = dev(np.full(shapes, 700.0))
    xd = torch.empty_like(wd)
    with pytest.raises(S.SdfsError, match="before sdfs_set_tilt_dev"):
        op.apply_tilted_dev(wd.data_ptr(), xd.data_ptr())
    with pytest.raises(S.SdfsError, match="before sdfs_set_tilt_dev"):
        op.solve_tilted_dev(wd.data_ptr(), xd.data_ptr())
    with pytest.raises(S.SdfsError, match="before sdfs_set_tilt_dev"):
        op.tilted_horizons_dev(3)
    assert _lib.lib.sdfs_set_tilt_dev(op.handle, wd.data_ptr(), 3, 0.0, 0.0) == _lib.SDFS_ERR_ARG
    assert _lib.lib.sdfs_set_tilt_dev(op.handle, None, 1, m.θ, -m.γ) == _lib.SDFS_ERR_ARG
    op.set_tilt_dev(None, 0, 0.0, 1.0)
    op.apply_tilted_dev(wd.data_ptr(), xd.data_ptr())
    with pytest.raises(S.SdfsError, match="save_at"):
        op.tilted_horizons_dev(3, None, [2, 2], [xd.data_ptr(), xd.data_ptr()])
    with pytest.raises(S.SdfsError, match="save_at"):
        op.tilted_horizons_dev(3, None, [4], [xd.data_ptr()])
    assert _lib.lib.sdfs_tilted_horizons_dev(op.handle, 0, None, 0, None, None, None) == _lib.SDFS_ERR_ARG
    op.synchronize()
    # dense
    D = S.DenseOperator(0.5 * np.full((4, 4), 0.25), 0.99, -10.0)
    with pytest.raises(S.SdfsError, match="unsharded discretised"):
        D.set_tilt_dev(None, 0, 0.0, 1.0)
    # continuous
    ssy = S.SSY()
    grids = S.build_grid(ssy, 3, 3, 3, 4)
    nodes, weights = S.qnwnorm([3] * 4)
    Tc = S.T_fun_factory((np.array(ssy.params), grids, nodes.T.copy(), weights), "quadrature", 3 * 3 * 3 * 4)
    # (``ContinuousOperator.set_tilt_dev`` is the tilt of the continuous-state model; the discrete entry point refuses its handle)
    assert _lib.lib.sdfs_set_tilt_dev(Tc.handle, None, 0, 0.0, 1.0) == _lib.SDFS_ERR_UNSUPPORTED
    assert "unsharded discretised" in _lib.last_error(Tc.handle)
    # sharded (one rank owning every index of its two axes)
    nd = len(shapes)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in arr]
    h = C.c_void_p()
    rc = _lib.lib.sdfs_create_sharded(
        _lib.SDFS_MODEL_GCY, nd, (C.c_int64 * nd)(*shapes), (C.c_double * 18)(*m.params), 18,
        (C.POINTER(C.c_double) * 15)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs]),
        (C.c_int64 * 15)(*[a.size for a in arrs]), 15, 0, 3, 0, shapes[3], 5, 0, shapes[5], C.byref(h))
    assert rc == 0, _lib.last_error(None)
    try:
        assert _lib.lib.sdfs_set_tilt_dev(h, wd.data_ptr(), 1, m.θ, -m.γ) == _lib.SDFS_ERR_UNSUPPORTED
        assert _lib.lib.sdfs_apply_tilted_dev(h, wd.data_ptr(), xd.data_ptr()) == _lib.SDFS_ERR_UNSUPPORTED
        assert _lib.lib.sdfs_solve_tilted_dev(h, None, wd.data_ptr(), xd.data_ptr(), None, None) == _lib.SDFS_ERR_UNSUPPORTED
    finally:
        _lib.lib.sdfs_destroy(h)
    op.close()

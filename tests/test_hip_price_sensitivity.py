"""
GPU tests of the price sensitivities (sdfs_tilt_tangent_dev, ``price_sensitivities``):

 (1) ``tilt_tangent_dev`` against the numpy twin (tests/price_sens_oracle.py) at two ragged shapes: every parameter, the
     persistences on every axis, p = 0, 1, 2, with K f given and not, f = 1 and df = 0 as NULL pointers;
 (2) the same comparison where the products run on the small-grid plan and on the padded pair plan (at 10^6 points the
     grid-stride loops of the streaming kernels take a second trip);
 (3) ``price_sensitivities`` against the dense twin at two small fixed points;
 (4) its consistency: ``dw=`` given or computed, two runs, κ = 1 (pd = w* − 1), ``sdf_moments`` untouched;
 (5) the refusals of the entry point.

BOUNDS.  The tangent: |device − twin| ≤ 1e-11 × the abs companion at every grid point, the bound the continuous tangent's
test uses for the same comparison (the companion is the sum of the absolute values of the terms; both sides round each
term to ~1e-16 of it, the logarithms and the products to a few 1e-15).  The solves: max|Δ| / max|ref| ≤ 10 · cond₂(I − K_twin) ·
rtol per field, the perturbation rule of tests/test_hip_cont_sensitivity.py; cond₂ is computed here.
The twin takes T w from the device (``op(w)``): the entry point has no argument for it, the tilt's linearisation fixes it.
Every test runs under its own time limit (SIGALRM).
"""
import contextlib
import ctypes as C
import os
import signal

import numpy as np
import pytest

from conftest import load_golden
from price_sens_oracle import tilt_tangent, price_sensitivities_dense

pytestmark = pytest.mark.gpu

RTOL_TANGENT = 1e-11
SOLVE_RTOL = 1e-12


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


def layout(kind):
    from sdfs_via_autodiff_amd._requests import LAYOUT
    return LAYOUT[kind]


def directions(m, shapes, names, arr):
    from sdfs_via_autodiff_amd.sensitivity import _directions
    return _directions(m, shapes, names, arr, persistence=True)


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


def tilts(m):
    th, g = m.θ, m.γ
    return [(0, 0.3, 1.0), (1, th, 2.0 - g), (2, 2 * th, -2 * g)]


class Case:
    """Random data of one tangent comparison, on the host and on the device."""

    def __init__(self, op, shapes, seed):
        rng = np.random.default_rng(seed)
        self.w = 500.0 + 400.0 * rng.random(shapes)
        self.f = 0.5 + rng.random(shapes)
        self.dw, self.dTw, self.df = (rng.standard_normal(shapes) for _ in range(3))
        self.Tw = op(self.w)
        self.d = {k: dev(getattr(self, k)) for k in ("w", "f", "dw", "dTw", "df")}


def compare(op, kind, shapes, m, arr, c, p, kl, kc, d, dkl, dkc, variant, kf_dev):
    """max over the grid of |device − twin| / abs companion for one direction.  variant: 0 everything given, 1 K f not
    given, 2 f = 1 as NULL (K f not given either), 3 df = 0 as NULL, 4 f and df NULL with K f given."""
    import torch
    f_null, df_null, kf_null = variant in (2, 4), variant in (3, 4), variant in (1, 2)
    out = torch.empty_like(c.d["w"])
    f = np.ones(shapes) if f_null else c.f
    df = np.zeros(shapes) if df_null else c.df
    if not kf_null and f_null:                     # K 1 for the given-K f form
        one = torch.ones_like(out)
        kf_dev = torch.empty_like(out)
        op.apply_tilted_dev(one.data_ptr(), kf_dev.data_ptr())
    op.tilt_tangent_dev(c.d["w"].data_ptr(), c.d["dw"].data_ptr(), c.d["dTw"].data_ptr(), d[0], d[1], d[2], dkl, dkc,
                        None if f_null else c.d["f"].data_ptr(), None if df_null else c.d["df"].data_ptr(),
                        None if kf_null else kf_dev.data_ptr(), out.data_ptr())
    got = out.cpu().numpy()
    want, comp = tilt_tangent(kind, shapes, m, arr, c.w, c.Tw, f, p, kl, kc, d, dkl, dkc, c.dw, c.dTw, df)
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(got - want) / comp))


# -- (1) every parameter at two ragged shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shapes,plan", [("ssy", (4, 7, 6, 5), "classic"), ("gcy", (3, 2, 4, 2, 3, 5), None)],
                         ids=["ssy4765", "gcy324235"])
def test_tilt_tangent_matches_the_twin_every_parameter(S, kind, shapes, plan):
    import torch
    m = model_of(S, kind)
    arr = disc(S, kind)(m, shapes)
    op = make_op(S, kind, shapes, m, arr, plan)
    names = layout(kind).params
    dirs = directions(m, shapes, names, arr)
    assert {a for d in dirs if d[2] is not None for a, g in enumerate(d[2]) if g is not None} == set(range(len(shapes)))
    c = Case(op, shapes, 5)
    kf = torch.empty_like(c.d["w"])
    worst, seen = 0.0, set()
    for ip, (p, kl, kc) in enumerate(tilts(m)):
        op.set_tilt_dev(c.d["w"].data_ptr(), p, kl, kc)
        op.apply_tilted_dev(c.d["f"].data_ptr(), kf.data_ptr())
        for j, (name, d) in enumerate(zip(names, dirs)):
            variant = (j + ip) % 5
            seen.add((p, variant))
            r = compare(op, kind, shapes, m, arr, c, p, kl, kc, d, 0.7, -0.4, variant, kf)
            worst = max(worst, r)
            assert r <= RTOL_TANGENT, f"{kind} {shapes} p = {p} {name} variant {variant}: {r:.3e} of the abs companion"
    assert seen == {(p, v) for p in (0, 1, 2) for v in range(5)}
    print(f"{kind} {shapes}: max |device - twin| / abs companion = {worst:.3e}")
    op.close()


# -- (2) the other plans ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shapes,marker,names", [("ssy", (15,) * 4, "small-grid plan", ("γ", "s_c", "ρ_c")),
                                                      ("gcy", (10,) * 6, "padded pair plan", ("γ", "s_c", "ρ_zπ"))],
                         ids=["ssy15-small", "gcy10-padded"])
def test_tilt_tangent_matches_the_twin_on_the_other_plans(S, kind, shapes, marker, names):
    import torch
    m = model_of(S, kind)
    arr = disc(S, kind)(m, shapes)
    op = make_op(S, kind, shapes, m, arr)
    assert marker in op.describe_plan(), op.describe_plan()
    dirs = directions(m, shapes, names, arr)
    c = Case(op, shapes, 6)
    kf = torch.empty_like(c.d["w"])
    th, g = m.θ, m.γ
    worst = 0.0
    for j, (name, d) in enumerate(zip(names, dirs)):            # one tilt per parameter: p = 1, 2, 0
        p, kl, kc = [(1, th, 2.0 - g), (2, 2 * th, -2 * g), (0, 0.3, 1.0)][j]
        op.set_tilt_dev(c.d["w"].data_ptr(), p, kl, kc)
        op.apply_tilted_dev(c.d["f"].data_ptr(), kf.data_ptr())
        r = compare(op, kind, shapes, m, arr, c, p, kl, kc, d, 0.7, -0.4, j % 2, kf)
        worst = max(worst, r)
        assert r <= RTOL_TANGENT, f"{kind} {shapes} p = {p} {name}: {r:.3e} of the abs companion"
    print(f"{kind} {shapes}: max |device - twin| / abs companion = {worst:.3e}")
    op.close()


# -- (3) the whole chain against the dense twin -------------------------------------------------------------------------
FIXTURES = {"ssy": ((2, 3, 4, 5), "sa_ssy_2x3x4x5.npz", "w_1e8"), "gcy": ((3,) * 6, "sa_gcy_3x3x3x3x3x3.npz", "w_1e7")}
FIELDS0 = ("E_M", "log_rf", "max_sharpe")
FIELDS = FIELDS0 + ("pd", "expected_return", "log_premium")


@pytest.fixture(scope="module")
def fixed_points(S):
    """{kind: (shapes, model, arrays, w*)}: the committed fixtures polished by a device Newton solve."""
    out = {}
    for kind, (shapes, file, key) in FIXTURES.items():
        m = model_of(S, kind)
        arr = disc(S, kind)(m, shapes)
        op = S.KoopmansOperator(kind, shapes, m.params, arr)
        w, _, info = op.solve(np.array(load_golden(file)[key], dtype=np.float64), "newton", tol=1e-10, inner_rtol=1e-12,
                              inner_atol=0.0)
        assert info["status"] == 0
        op.close()
        out[kind] = (shapes, m, arr, w)
    return out


@pytest.fixture(scope="module")
def dense(fixed_points):
    """{(kind, kappa): the dense twin of every parameter}, computed once."""
    memo = {}

    def get(kind, kappa):
        if (kind, kappa) not in memo:
            shapes, m, arr, w = fixed_points[kind]
            names = layout(kind).params
            memo[kind, kappa] = price_sensitivities_dense(kind, shapes, m, arr, w, kappa,
                                                          dict(zip(names, directions(m, shapes, names, arr))))
        return memo[kind, kappa]
    return get


def solve_bound(ref, n):
    cond = float(np.linalg.cond(np.eye(n) - ref["_K"]))
    return cond, 10.0 * cond * SOLVE_RTOL


@pytest.mark.parametrize("kappa", [0.0, 2.0])
@pytest.mark.parametrize("kind", ["ssy", "gcy"])
def test_price_sensitivities_match_the_dense_twin(S, fixed_points, dense, kind, kappa):
    shapes, m, arr, w = fixed_points[kind]
    names = layout(kind).params
    ref = dense(kind, kappa)
    cond, bound = solve_bound(ref, w.size)
    got = S.price_sensitivities(m, shapes, w, kappa=kappa, persistence=True, rtol=SOLVE_RTOL)
    assert set(got) == set(names) | {"_info"}
    worst = 0.0
    for name in names:
        assert set(got[name]) == set(FIELDS)
        itw, itv = got["_info"][name]
        assert itw > 0 and itv > 0
        for fld in FIELDS:
            assert got[name][fld].shape == shapes
            err = np.max(np.abs(got[name][fld] - ref[name][fld])) / np.max(np.abs(ref[name][fld]))
            worst = max(worst, err)
            assert err <= bound, f"{kind} kappa {kappa} {name} {fld}: {err:.3e} > {bound:.3e}"
    print(f"{kind} kappa {kappa}: cond2(I - K) = {cond:.3e}, bound {bound:.3e}, worst {worst:.3e}")


# -- (4) consistency ----------------------------------------------------------------------------------------------------
def same(a, b):
    assert set(a) == set(b)
    for nm in a:
        if nm == "_info":
            continue
        for fld in a[nm]:
            assert np.array_equal(a[nm][fld], b[nm][fld], equal_nan=True), (nm, fld)


def test_given_dw_two_runs_consumption_claim_and_moments_untouched(S, fixed_points, dense):
    kind = "ssy"
    shapes, m, arr, w = fixed_points[kind]
    wrt = ("γ", "ψ", "s_c", "ρ_z")
    before = S.sdf_moments(m, shapes, w)
    a = S.price_sensitivities(m, shapes, w, kappa=1.0, wrt=wrt, persistence=True, rtol=SOLVE_RTOL)
    b = S.price_sensitivities(m, shapes, w, kappa=1.0, wrt=wrt, persistence=True, rtol=SOLVE_RTOL)
    same(a, b)                                                         # two runs: identical bits
    after = S.sdf_moments(m, shapes, w)
    for fld in FIELDS0:
        assert np.array_equal(before[fld], after[fld]), fld
    dws = S.wc_ratio_sensitivities(m, shapes, w, wrt=wrt, persistence=True, rtol=SOLVE_RTOL)
    c = S.price_sensitivities(m, shapes, w, kappa=1.0, wrt=wrt, persistence=True, rtol=SOLVE_RTOL, dw=dws)
    same(a, c)
    assert all(c["_info"][nm][0] is None and c["_info"][nm][1] > 0 for nm in wrt)
    # the consumption claim's pd is w* - 1: d pd = dw*, to the bound of (3) (K(1, theta, 1 - gamma) = J)
    ref = dense(kind, 1.0)
    _, bound = solve_bound(ref, w.size)
    for nm in wrt:
        err = np.max(np.abs(a[nm]["pd"] - dws[nm])) / np.max(np.abs(dws[nm]))
        assert err <= bound, f"{nm}: d pd differs from dw* by {err:.3e} > {bound:.3e}"
    # the SDF moments alone
    d = S.price_sensitivities(m, shapes, w, wrt="γ", rtol=SOLVE_RTOL)
    assert set(d["γ"]) == set(FIELDS0) and d["_info"]["γ"][1] is None
    for fld in FIELDS0:
        assert np.array_equal(d["γ"][fld], a["γ"][fld], equal_nan=True)


# -- (5) refusals -------------------------------------------------------------------------------------------------------
def test_refusals(S):
    import torch
    from sdfs_via_autodiff_amd import _lib
    lib = _lib.lib
    shapes = (4, 5, 6, 7)
    m = S.SSY()
    arr = S.discretize_ssy(m, shapes)
    op = make_op(S, "ssy", shapes, m, arr)
    wd = dev(np.full(shapes, 700.0))
    x, out = torch.randn_like(wd), torch.empty_like(wd)
    torch.cuda.synchronize()
    dp, da = S.discretize_ssy_tangent(m, shapes, "s_c")
    par = (C.c_double * len(dp))(*dp)
    P = lambda t: t.data_ptr()                                         # noqa: E731

    def call(h, w=wd, dkl=0.0, dkc=0.0):
        return lib.sdfs_tilt_tangent_dev(h, P(w) if w is not None else None, P(x), P(x), par, None, None, dkl, dkc, None, None,
                                         None, P(out))
    assert call(op.handle) == _lib.SDFS_ERR_ARG                        # before a set_tilt
    assert "before sdfs_set_tilt_dev" in _lib.last_error(op.handle)
    op.set_tilt_dev(P(wd), 1, m.θ, -m.γ)
    assert call(op.handle) == 0
    assert call(op.handle, w=None) == _lib.SDFS_ERR_ARG                # power 1 without w
    assert call(op.handle, dkl=float("nan")) == _lib.SDFS_ERR_ARG
    assert call(op.handle, dkc=float("inf")) == _lib.SDFS_ERR_ARG
    assert lib.sdfs_tilt_tangent_dev(op.handle, P(wd), P(x), P(x), par, None, None, 0.0, 0.0, None, None, P(out), P(out)) \
        == _lib.SDFS_ERR_ARG                                           # out is an input
    for i in (1, 3, 5, 7):                                             # a transition-array tangent without a generator
        bad = list(da); bad[i] = np.full(arr[i].shape, 1e-3)
        with pytest.raises(S.SdfsError, match="transition"):
            op.tilt_tangent_dev(P(wd), P(x), P(x), dp, bad, None, 0.0, 0.0, None, None, None, P(out))
    op.set_tilt_dev(None, 0, 0.0, 1.0)
    assert call(op.handle, w=None) == 0                                # power 0 reads no w
    op.synchronize()
    op.close()

    # a generator on a handle with a conditional transition tensor
    rng = np.random.default_rng(5)
    carr = list(arr)
    q = rng.random(carr[7].shape) + 0.05
    carr[7] = q / q.sum(axis=-1, keepdims=True)
    cop = make_op(S, "ssy", shapes, m, carr)
    cop.set_tilt_dev(P(wd), 1, m.θ, -m.γ)
    dpp, dap, dgp = S.discretize_ssy_persistence_tangent(m, shapes, "ρ_c")
    with pytest.raises(S.SdfsError, match="unconditional"):
        cop.tilt_tangent_dev(P(wd), P(x), P(x), dpp, dap, dgp, 0.0, 0.0, None, None, None, P(out))
    cop.tilt_tangent_dev(P(wd), P(x), P(x), dp, da, None, 0.0, 0.0, None, None, None, P(out))     # (no generator: fine)
    cop.synchronize()
    cop.close()

    # dense, continuous, sharded
    D = S.DenseOperator(0.5 * np.full((4, 4), 0.25), 0.99, -10.0)
    assert call(D.handle) == _lib.SDFS_ERR_UNSUPPORTED
    ssy = S.SSY()
    grids = S.build_grid(ssy, 3, 3, 3, 4)
    nodes, weights = S.qnwnorm([3] * 4)
    Tc = S.T_fun_factory((np.array(ssy.params), grids, nodes.T.copy(), weights), "quadrature", 3 * 3 * 3 * 4)
    assert call(Tc.handle) == _lib.SDFS_ERR_UNSUPPORTED
    assert "unsharded discretised" in _lib.last_error(Tc.handle)
    g = S.GCY()
    gs = (3, 4, 2, 3, 5, 4)
    garr = [np.ascontiguousarray(a, dtype=np.float64) for a in S.discretize_gcy(g, gs)]
    h = C.c_void_p()
    rc = lib.sdfs_create_sharded(
        _lib.SDFS_MODEL_GCY, 6, (C.c_int64 * 6)(*gs), (C.c_double * 18)(*g.params), 18,
        (C.POINTER(C.c_double) * 15)(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in garr]),
        (C.c_int64 * 15)(*[a.size for a in garr]), 15, 0, 3, 0, gs[3], 5, 0, gs[5], C.byref(h))
    assert rc == 0, _lib.last_error(None)
    try:
        gpar = (C.c_double * 18)(*([0.0] * 18))
        assert lib.sdfs_tilt_tangent_dev(h, P(wd), P(x), P(x), gpar, None, None, 0.0, 0.0, None, None, None, P(out)) \
            == _lib.SDFS_ERR_UNSUPPORTED
    finally:
        lib.sdfs_destroy(h)

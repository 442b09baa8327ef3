"""
GPU tests of the continuous-state parameter sensitivities (csrc/cont_sens.hpp, the C_PTAN form of csrc/cont_kernel.hpp,
``ContinuousOperator.cont_param_tangent_dev``, ``sensitivity.wc_ratio_sensitivities_continuous``) against
the numpy twin tests/cont_sens_oracle.py.  The twin's own consistency (analytic against complex step) and the input
conditions (no node within 1e-6 cells of a grid line; every parameter moves T on every gather path) are pinned on the
CPU by tests/test_cont_sensitivity_cpu.py.

BOUNDS.  The tangent: |got − want| ≤ 1e-11 × the abs companion at every grid point -- the signed-sum bound of
tests/test_hip_continuous_paths.py and tests/test_hip_cont_pricing.py.  The sensitivities at rtol = 1e-12:
max|Δ| / max|ref| ≤ 10 · cond₂(I − J_twin) · rtol, the perturbation bound of the solve DESIGN §4.15 uses; cond₂ is computed
here.  The operator of the end-to-end test is Gauss–Hermite order 4: an odd order puts its zero node exactly on grid lines,
where the tangent is one-sided and the side a matter of the coordinate's last bit.
"""
import ctypes as C
import signal

import numpy as np
import pytest

import cont_boxes as CB
import cont_sens_oracle as so
import cont_sim_cases as CC
from test_hip_cont_simulation import model_of, newton_fixed_point, quad_operator

pytestmark = pytest.mark.gpu

RTOL_TANGENT = 1e-11
SOLVE_RTOL = 1e-12
QUAD_D = 4
FIXED_POINT_GRIDS = [g for g in CC.GRIDS if g not in CC.NO_FIXED_POINT]
LONGDOUBLE_STRIDE = {"C6": 16}       # C6 (4096 points x 64 corners): every 16th grid point in long double, a quarter minute


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


_CASE = {}


def operator_case(S, name):
    """(operator, kind, params, grids, w, twin dT (np, *shape), twin abs companion, twin T w)."""
    if name not in _CASE:
        kind, params, grids, nodes, weights = CB.make_case(so.CASES[so.CASE_IDS.index(name)])
        par = tuple(float(q) for q in params)
        op = S.ContinuousOperator(np.array(par), grids, nodes, weights)
        w = CC.smooth_w(grids)
        _CASE[name] = (op, kind, par, grids, w) + so.tangent(kind, par, grids, w, nodes, weights)
    return _CASE[name]


def mixed_direction(npar, seed):
    return np.random.default_rng(seed).standard_normal(npar)


def device_tangent(op, w, dp):
    """(tangent, T w, J·v after the tangent for a fixed v) as host arrays, through the device entry points."""
    import torch
    wd = to_dev(op, w)
    vd = to_dev(op, np.random.default_rng(11).standard_normal(w.shape))
    out, tw, jv = torch.empty_like(wd), torch.empty_like(wd), torch.empty_like(wd)
    torch.cuda.synchronize()
    op.cont_param_tangent_dev(wd.data_ptr(), dp, out.data_ptr(), tw.data_ptr())
    op.jvp_dev(vd.data_ptr(), jv.data_ptr())
    op.synchronize()
    return out.cpu().numpy(), tw.cpu().numpy(), jv.cpu().numpy()


@pytest.mark.parametrize("name", so.CASE_IDS)
def test_tangent_matches_the_twin_on_every_gather_path(S, name):
    import torch
    op, kind, par, grids, w, dT, aT, Tw = operator_case(S, name)
    npar = len(par)
    worst = 0.0
    dirs = [np.eye(npar)[j] for j in range(npar)] + [mixed_direction(npar, 900 + so.CASE_IDS.index(name))]
    for dp in dirs:
        got = op.cont_param_tangent(w, dp)
        want, bound = np.tensordot(dp, dT, 1), np.tensordot(np.abs(dp), aT, 1)
        err = np.abs(got - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.max(np.where(bound > 0, err / bound, 0.0))))
        assert np.all(err <= RTOL_TANGENT * bound), (name, dp, float(np.max(err)))
    print(f"{name}: worst |got − want| / abs companion over {len(dirs)} directions = {worst:.3e}")
    case = so.CASES[so.CASE_IDS.index(name)]
    _, _, _, nodes, weights = CB.make_case(case)
    pts = np.arange(0, w.size, LONGDOUBLE_STRIDE.get(name, 1))
    dL = so.tangent(kind, par, grids, w, nodes, weights, dtype=np.longdouble, points=pts)[0].astype(np.float64)
    d64, a64 = dT.reshape(npar, -1)[:, pts], aT.reshape(npar, -1)[:, pts]
    with np.errstate(invalid="ignore", divide="ignore"):
        twin = float(np.max(np.where(a64 > 0, np.abs(dL - d64) / a64, 0.0)))
    print(f"{name}: float64 twin against long-double twin at {pts.size} of {w.size} points, worst |Δ| / abs companion = {twin:.3e}")
    assert twin <= RTOL_TANGENT / 10          # (the twin's own rounding stays a factor 10 inside the bound)

    # T w, the linearisation the call leaves behind, and determinism, along the mixed direction
    dp = dirs[-1]
    got, tw, jv = device_tangent(op, w, dp)
    np.testing.assert_allclose(tw, op(w), rtol=1e-13, atol=0)
    np.testing.assert_allclose(tw, Tw, rtol=1e-12, atol=0)
    wd = to_dev(op, w)
    vd = to_dev(op, np.random.default_rng(11).standard_normal(w.shape))
    ref = torch.empty_like(wd)
    torch.cuda.synchronize()
    op.linearize_dev(wd.data_ptr())
    op.jvp_dev(vd.data_ptr(), ref.data_ptr())
    op.synchronize()
    assert np.array_equal(jv, ref.cpu().numpy())
    again, tw2, jv2 = device_tangent(op, w, dp)
    assert np.array_equal(got, again) and np.array_equal(tw, tw2) and np.array_equal(jv, jv2)
    assert np.array_equal(got, op.cont_param_tangent(w, dp))          # (with and without the T w output)


@pytest.mark.parametrize("from_pow", [0, 1])
@pytest.mark.parametrize("name", ["A4", "A6", "C6", "E4"])
def test_both_sources_of_the_logarithm_meet_the_bound(S, name, from_pow, monkeypatch):
    """SDFS_PTAN_LOG_FROM_POW (read at every call): libm's log (C_PTAN) and ln 2 times the power's own log2 (C_PTANL)."""
    op, kind, par, grids, w, dT, aT, _ = operator_case(S, name)
    monkeypatch.setenv("SDFS_PTAN_LOG_FROM_POW", str(from_pow))
    dp = mixed_direction(len(par), 55)
    got = op.cont_param_tangent(w, dp)
    err, bound = np.abs(got - np.tensordot(dp, dT, 1)), np.tensordot(np.abs(dp), aT, 1)
    print(f"{name}: log from {'the power' if from_pow else 'libm'}, worst ratio {float(np.max(err / bound)):.3e}")
    assert np.all(err <= RTOL_TANGENT * bound)
    assert np.array_equal(got, op.cont_param_tangent(w, dp))


@pytest.mark.parametrize("name", ["B4", "B6", "C6"])
def test_tangent_of_the_monte_carlo_rule(S, name):
    op, kind, par, grids, w, dT, aT, _ = operator_case(S, name)
    assert op.weights is None
    dp = mixed_direction(len(par), 77)
    got = op.cont_param_tangent(w, dp)
    err, bound = np.abs(got - np.tensordot(dp, dT, 1)), np.tensordot(np.abs(dp), aT, 1)
    print(f"{name}: Monte-Carlo rule, worst ratio {float(np.max(err / bound)):.3e}")
    assert np.all(err <= RTOL_TANGENT * bound)


@pytest.mark.parametrize("grid", FIXED_POINT_GRIDS, ids=[CC.tag(*g) for g in FIXED_POINT_GRIDS])
def test_sensitivities_against_the_dense_twin(S, grid):
    kind, sizes, sd = grid
    model, par, grids = model_of(S, kind), CC.params_of(kind), CC.grids_of(kind, sizes, sd)
    op = quad_operator(S, kind, grids, QUAD_D)
    w = newton_fixed_point(op, np.ones(sizes))
    names = S.SSY_PARAMS if kind == "ssy" else S.GCY_PARAMS
    out = S.wc_ratio_sensitivities_continuous(model, grids, w, rtol=SOLVE_RTOL, operator=op)
    assert set(out) == set(names) | {"_info"}
    ref, cond = so.dense_sensitivities(kind, par, grids, w, op.nodes, op.weights)
    bound = 10.0 * cond * SOLVE_RTOL
    print(f"{CC.tag(*grid)}: cond2(I - J) = {cond:.3e}, bound {bound:.3e}")
    for j, nm in enumerate(names):
        its, rel = out["_info"][nm]
        scale = np.max(np.abs(ref[j]))
        err = np.max(np.abs(out[nm] - ref[j]))
        print(f"  {nm}: {its} iterations, residual {rel:.2e}, max|Δ| / max|ref| = {err / scale if scale else err:.3e}")
        assert out[nm].shape == tuple(sizes) and its >= 0 and rel <= SOLVE_RTOL
        assert scale > 0 and err / scale <= bound, (nm, err, scale)
    # the default path builds the same operator
    dflt = S.wc_ratio_sensitivities_continuous(model, grids, w, rtol=SOLVE_RTOL, d=QUAD_D)
    for nm in names:
        assert np.array_equal(dflt[nm], out[nm]), nm
    one = S.wc_ratio_sensitivities_continuous(model, grids, w, wrt=names[3], rtol=SOLVE_RTOL, operator=op)
    assert set(one) == {names[3], "_info"} and np.array_equal(one[names[3]], out[names[3]])


def test_c_abi_refusals(S):
    import torch
    from sdfs_via_autodiff_amd import _lib
    lib = _lib.lib
    ARG, UNSUP = _lib.SDFS_ERR_ARG, _lib.SDFS_ERR_UNSUPPORTED
    ssy = S.SSY()
    shapes = (2, 3, 4, 5)
    dp13 = (C.c_double * 13)(*([0.0] * 12 + [1.0]))
    g = torch.full(shapes, 700.0, dtype=torch.float64, device="cuda")
    o, t = torch.empty_like(g), torch.empty_like(g)
    torch.cuda.synchronize()
    # a discretised and a dense handle
    disc = S.ssy_operator(shapes, ssy.params, S.discretize_ssy(ssy, shapes))
    assert lib.sdfs_cont_param_tangent_dev(disc._h, g.data_ptr(), dp13, o.data_ptr(), None) == UNSUP
    assert "continuous-state handles only" in _lib.last_error(disc._h)
    H = np.full((6, 6), 1.0 / 6)
    dense = S.DenseOperator(H, 0.99, -30.0)
    g6 = torch.full((6,), 700.0, dtype=torch.float64, device="cuda")
    o6 = torch.empty_like(g6)
    torch.cuda.synchronize()
    assert lib.sdfs_cont_param_tangent_dev(dense._h, g6.data_ptr(), dp13, o6.data_ptr(), None) == UNSUP
    # a continuous handle
    grids = S.build_grid(ssy, *shapes)
    nodes, weights = S.qnwnorm([2] * 4)
    op = S.ContinuousOperator(np.array(ssy.params), grids, np.ascontiguousarray(nodes.T), weights)
    h = op._h
    assert lib.sdfs_cont_param_tangent_dev(h, None, dp13, o.data_ptr(), None) == ARG
    assert lib.sdfs_cont_param_tangent_dev(h, g.data_ptr(), None, o.data_ptr(), None) == ARG
    assert lib.sdfs_cont_param_tangent_dev(h, g.data_ptr(), dp13, None, None) == ARG
    assert lib.sdfs_cont_param_tangent_dev(h, g.data_ptr(), dp13, g.data_ptr(), None) == ARG
    assert "distinct" in _lib.last_error(h)
    assert lib.sdfs_cont_param_tangent_dev(h, g.data_ptr(), dp13, o.data_ptr(), o.data_ptr()) == ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        d = (C.c_double * 13)(*([0.0] * 5 + [bad] + [0.0] * 7))
        assert lib.sdfs_cont_param_tangent_dev(h, g.data_ptr(), d, o.data_ptr(), None) == ARG
        assert "not finite" in _lib.last_error(h)
    with pytest.raises(ValueError, match="13 parameters"):
        op.cont_param_tangent_dev(g.data_ptr(), [1.0] * 18, o.data_ptr())
    # sdfs_param_tangent_dev keeps refusing a continuous handle
    assert lib.sdfs_param_tangent_dev(h, g.data_ptr(), dp13, None, o.data_ptr(), None) == UNSUP
    # the handle still applies T, and the tangent itself works
    want = op(np.full(shapes, 700.0))
    op.apply_dev(g.data_ptr(), t.data_ptr())
    op.synchronize()
    assert np.array_equal(t.cpu().numpy(), want)
    assert lib.sdfs_cont_param_tangent_dev(h, g.data_ptr(), dp13, o.data_ptr(), t.data_ptr()) == 0
    op.synchronize()
    np.testing.assert_allclose(t.cpu().numpy(), want, rtol=1e-13, atol=0)
    assert bool(torch.all(torch.isfinite(o)))

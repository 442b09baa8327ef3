"""
GPU tests of the transposed Jacobian of the continuous-state operator, the adjoint solve on it and the adjoint gradient
(the C_VJP form of csrc/cont_kernel.hpp, csrc/cont_vjp.hip, csrc/cont_adjoint.hpp, ``ContinuousOperator.cont_vjp_dev`` /
``cont_solve_adjoint_dev``, ``sensitivity.wc_ratio_gradient_continuous``) against the numpy twin
tests/cont_adjoint_oracle.py.  The twin's own consistency is pinned on the CPU by tests/test_cont_gradient_cpu.py.

The new calls accumulate with hardware atomic adds whose arrival order varies, so NOTHING here asserts bit equality of
their results; everything else on the handle is held to its bits.

BOUNDS.  The project's own:
  Jᵀu          |got − want| ≤ 1e-11 × the abs companion Jᵀ|u| at every grid point (J is entrywise non-negative), the
               signed-sum bound of tests/test_hip_continuous_paths.py; where the companion is zero the result is exactly 0;
  two runs     each within 1e-11 × companion of the exact sum, hence within 2e-11 × companion of each other;
  ⟨u, J v⟩     = ⟨Jᵀu, v⟩ to 1e-11 × ⟨|u|, J|v|⟩, the companion of either side, computed on the device;
  solves       at rtol = 1e-12: max|Δ| / max|ref| ≤ 10 · cond₂(I − J_twin) · rtol, the perturbation bound of the solve DESIGN
               §4.15 uses (cond₂ of the transpose is the same number);
  gradient     |got_k − ref_k| ≤ 10 · cond₂ · rtol · max|λ_ref| · Σ|∂T/∂p_k| + 1e-11 · Σ|λ_ref| · aT_k: the solve's bound on λ
               carried through the dot product, plus the signed-sum bound of the tangent (aT its abs companion).
The operator of the solves is Gauss–Hermite order 4, for the reason the docstring of tests/test_hip_cont_sensitivity.py
gives: an odd order puts its zero node exactly on grid lines, where the tangent is one-sided.
"""
import ctypes as C
import signal

import numpy as np
import pytest

import cont_adjoint_oracle as ao
import cont_boxes as CB
import cont_sens_oracle as so
import cont_sim_cases as CC
from test_hip_cont_simulation import model_of, newton_fixed_point, quad_operator

pytestmark = pytest.mark.gpu

RTOL_SUM = 1e-11
SOLVE_RTOL = 1e-12
QUAD_D = 4
EPS = 2.0 ** -52
FIXED_POINT_GRIDS = [g for g in CC.GRIDS if g not in CC.NO_FIXED_POINT]


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


def directions(shape, seed):
    """{"normal": standard normal u, "unit": one unit vector at an interior point}."""
    unit = np.zeros(shape)
    unit[tuple(n // 2 for n in shape)] = 1.0
    return {"normal": np.random.default_rng(seed).standard_normal(shape), "unit": unit}


_CASE = {}


def operator_case(S, name):
    """(operator, w, {direction name: (u, twin Jᵀu, twin Jᵀ|u|)}), the twin computed once per case; J itself is not kept."""
    if name not in _CASE:
        kind, params, grids, nodes, weights = CB.make_case(so.CASES[so.CASE_IDS.index(name)])
        par = tuple(float(q) for q in params)
        op = S.ContinuousOperator(np.array(par), grids, nodes, weights)
        w = CC.smooth_w(grids)
        J = ao.jacobian(kind, par, grids, w, nodes, weights)
        twin = {}
        for nm, u in directions(w.shape, 300 + so.CASE_IDS.index(name)).items():
            jtu, comp = ao.vjp(J, u)
            twin[nm] = (u, jtu.reshape(w.shape), comp.reshape(w.shape))
        _CASE[name] = (op, w, twin)
    return _CASE[name]


def device_vjp(op, w, u, minus_identity=False, linearize=True):
    import torch
    wd, ud = to_dev(op, w), to_dev(op, u)
    out = torch.full_like(wd, float("nan"))              # (the call initialises its output itself)
    torch.cuda.synchronize()
    if linearize:
        op.linearize_dev(wd.data_ptr())
    op.cont_vjp_dev(ud.data_ptr(), out.data_ptr(), minus_identity)
    op.synchronize()
    return out.cpu().numpy()


def device_jvp(op, v):
    import torch
    vd = to_dev(op, v)
    out = torch.empty_like(vd)
    torch.cuda.synchronize()
    op.jvp_dev(vd.data_ptr(), out.data_ptr())
    op.synchronize()
    return out.cpu().numpy()


# -- 1. the transposed application on every gather path --------------------------------------------------------------------
@pytest.mark.parametrize("name", so.CASE_IDS)
def test_vjp_matches_the_twin_on_every_gather_path(S, name):
    op, w, twin = operator_case(S, name)
    for nm, (u, want, comp) in twin.items():
        got = device_vjp(op, w, u)
        err = np.abs(got - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = float(np.max(np.where(comp > 0, err / comp, 0.0)))
        print(f"{name} {nm}: worst |got − Jᵀu| / Jᵀ|u| = {worst:.3e}, {int(np.sum(comp > 0))} of {comp.size} points reached")
        assert np.all(np.isfinite(got))
        assert np.all(err <= RTOL_SUM * comp), (name, nm, float(np.max(err)))
        # out = Jᵀu − u: another run of the sum, then one subtraction.  Its difference to the plain call is u within the
        # bound of the sum plus one rounding of that subtraction and one of the subtraction here (half an ulp each of a
        # number no larger than |u| + companion)
        mi = device_vjp(op, w, u, minus_identity=True)
        d = np.abs((got - mi) - u)
        assert np.all(d <= RTOL_SUM * comp + EPS * (np.abs(u) + comp)), (name, nm, float(np.max(d)))
        assert np.all(np.abs(mi - (want - u)) <= RTOL_SUM * comp + EPS * (np.abs(u) + comp))
        assert np.all(np.abs(op.cont_vjp(w, u) - want) <= RTOL_SUM * comp)    # (the host form: the same call)


# -- 2. the exact transpose of the device J·v ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", so.CASE_IDS)
def test_vjp_is_the_transpose_of_the_device_jvp(S, name):
    import torch
    op, w, _ = operator_case(S, name)
    rng = np.random.default_rng(700 + so.CASE_IDS.index(name))
    for trial in range(2):
        u, v = rng.standard_normal(w.shape), rng.standard_normal(w.shape)
        wd, ud, vd = to_dev(op, w), to_dev(op, u), to_dev(op, v)
        au, av = ud.abs(), vd.abs()
        jv, jtu, jav = torch.empty_like(wd), torch.empty_like(wd), torch.empty_like(wd)
        torch.cuda.synchronize()
        op.linearize_dev(wd.data_ptr())
        op.jvp_dev(vd.data_ptr(), jv.data_ptr())
        op.cont_vjp_dev(ud.data_ptr(), jtu.data_ptr())
        op.jvp_dev(av.data_ptr(), jav.data_ptr())
        op.synchronize()
        lhs, rhs = float(torch.dot(ud.view(-1), jv.view(-1))), float(torch.dot(jtu.view(-1), vd.view(-1)))
        comp = float(torch.dot(au.view(-1), jav.view(-1)))
        print(f"{name}: <u, Jv> = {lhs:.15e}, <Jᵀu, v> = {rhs:.15e}, |Δ| / <|u|, J|v|> = {abs(lhs - rhs) / comp:.3e}")
        assert comp > 0 and abs(lhs - rhs) <= RTOL_SUM * comp


# -- 3. nothing else moves --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", so.CASE_IDS)
def test_the_linearisation_and_jvp_keep_their_bits(S, name):
    import torch
    from sdfs_via_autodiff_amd import _lib
    op, w, twin = operator_case(S, name)
    u, _, comp = twin["normal"]
    v = np.random.default_rng(11).standard_normal(w.shape)
    wd = to_dev(op, w)
    torch.cuda.synchronize()
    op.linearize_dev(wd.data_ptr())
    op.synchronize()
    before = device_jvp(op, v)
    first = device_vjp(op, w, u, linearize=False)
    assert np.array_equal(device_jvp(op, v), before)
    second = device_vjp(op, w, u, linearize=False)
    d = np.abs(first - second)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{name}: two runs of Jᵀu, worst |Δ| / Jᵀ|u| = {float(np.max(np.where(comp > 0, d / comp, 0.0))):.3e}, "
              f"{int(np.sum(d != 0))} of {d.size} points differ")
    assert np.all(d <= 2 * RTOL_SUM * comp)
    # an adjoint solve at this linearisation (w is no fixed point here: it may stop unconverged, which is not the subject)
    gd, xd = to_dev(op, u), to_dev(op, np.zeros(w.shape))
    o = _lib.default_opts()
    o.inner_rtol, o.inner_atol, o.inner_max_iter = 1e-10, 0.0, 40
    it, rel = C.c_int64(), C.c_double()
    torch.cuda.synchronize()
    rc = _lib.lib.sdfs_cont_solve_adjoint_dev(op._h, C.byref(o), gd.data_ptr(), xd.data_ptr(), C.byref(it), C.byref(rel))
    op.synchronize()
    assert rc in (0, _lib.SDFS_ERR_NUMERIC), _lib.last_error(op._h)
    print(f"{name}: adjoint solve at smooth w: rc {rc}, {it.value} iterations, residual {rel.value:.2e}")
    assert np.array_equal(device_jvp(op, v), before)
    assert np.array_equal(op(w), op(w))


# -- 4., 5. the adjoint solve and the gradient at a fixed point -----------------------------------------------------------
_FP = {}


def fixed_point_case(S, grid):
    """(model, operator, grids, w*, names, J, dT, aT, dw/dp twin, cond₂(I − J)) of one grid, solved and assembled once."""
    if grid not in _FP:
        kind, sizes, sd = grid
        model, par, grids = model_of(S, kind), CC.params_of(kind), CC.grids_of(kind, sizes, sd)
        op = quad_operator(S, kind, grids, QUAD_D)
        w = newton_fixed_point(op, np.ones(sizes))
        J = ao.jacobian(kind, par, grids, w, op.nodes, op.weights)
        dT, aT, _ = so.tangent(kind, par, grids, w, op.nodes, op.weights)
        A = np.eye(J.shape[0]) - J
        sens = np.linalg.solve(A, dT.reshape(dT.shape[0], -1).T).T
        names = S.SSY_PARAMS if kind == "ssy" else S.GCY_PARAMS
        _FP[grid] = (model, op, grids, w, names, J, dT, aT, sens, float(np.linalg.cond(A, 2)))
    return _FP[grid]


def rhs_vectors(shape):
    n = int(np.prod(shape))
    return {"mean": np.full(shape, 1.0 / n), "normal": np.random.default_rng(41).standard_normal(shape)}


@pytest.mark.parametrize("grid", FIXED_POINT_GRIDS, ids=[CC.tag(*g) for g in FIXED_POINT_GRIDS])
def test_adjoint_solve_against_the_dense_twin(S, grid):
    import torch
    model, op, grids, w, names, J, dT, aT, sens, cond = fixed_point_case(S, grid)
    bound = 10.0 * cond * SOLVE_RTOL
    print(f"{CC.tag(*grid)}: cond2(I - J) = {cond:.3e}, bound {bound:.3e}")
    wd = to_dev(op, w)
    for nm, g in rhs_vectors(w.shape).items():
        lam_ref, _ = ao.adjoint(J, g)
        gd, lam = to_dev(op, g), torch.empty_like(wd)
        torch.cuda.synchronize()
        op.linearize_dev(wd.data_ptr())
        its, rel = op.cont_solve_adjoint_dev(gd.data_ptr(), lam.data_ptr(), SOLVE_RTOL)
        err = float(np.max(np.abs(lam.cpu().numpy().ravel() - lam_ref)) / np.max(np.abs(lam_ref)))
        print(f"  g = {nm}: {its} iterations, residual {rel:.2e}, max|λ − λ_ref| / max|λ_ref| = {err:.3e}")
        assert its >= 1 and rel <= SOLVE_RTOL
        assert err <= bound


@pytest.mark.parametrize("grid", FIXED_POINT_GRIDS, ids=[CC.tag(*g) for g in FIXED_POINT_GRIDS])
def test_gradient_end_to_end(S, grid):
    model, op, grids, w, names, J, dT, aT, sens, cond = fixed_point_case(S, grid)
    kind, sizes, sd = grid
    fwd = S.wc_ratio_sensitivities_continuous(model, grids, w, rtol=SOLVE_RTOL, operator=op)
    solve = 10.0 * cond * SOLVE_RTOL
    for gname, g in rhs_vectors(w.shape).items():
        lam_ref, _ = ao.adjoint(J, g)
        ref, comp, sum_dT = ao.gradient(dT, aT, lam_ref)
        out = S.wc_ratio_gradient_continuous(model, grids, w, g, rtol=SOLVE_RTOL, operator=op)
        assert set(out) == set(names) | {"_info", "_adjoint"}
        its, rel = out["_info"]
        assert its >= 1 and rel <= SOLVE_RTOL
        assert out["_adjoint"].shape == tuple(sizes)
        assert np.max(np.abs(out["_adjoint"].ravel() - lam_ref)) <= solve * np.max(np.abs(lam_ref))
        lam_max = float(np.max(np.abs(lam_ref)))
        print(f"{CC.tag(*grid)}, g = {gname}: {its} iterations, residual {rel:.2e}")
        for k, nm in enumerate(names):
            assert isinstance(out[nm], float)
            adj_bound = solve * lam_max * sum_dT[k]
            bound = adj_bound + RTOL_SUM * comp[k]
            print(f"  {nm}: got {out[nm]:.12e}, twin {ref[k]:.12e}, |Δ| = {abs(out[nm] - ref[k]):.2e}, bound {bound:.2e}")
            assert abs(out[nm] - ref[k]) <= bound, (nm, out[nm], ref[k])
            # the forward twin on the same operator: one solve per parameter, each within its own bound
            fwd_bound = np.sum(np.abs(g)) * solve * np.max(np.abs(sens[k]))
            via_fwd = float(np.sum(g * fwd[nm]))
            assert abs(out[nm] - via_fwd) <= adj_bound + fwd_bound, (nm, out[nm], via_fwd)
    # a subset; operator= and d= build the same operator (compared within the bound: the call is not bit-reproducible)
    g = rhs_vectors(w.shape)["normal"]
    lam_ref, _ = ao.adjoint(J, g)
    ref, comp, sum_dT = ao.gradient(dT, aT, lam_ref)
    lam_max = float(np.max(np.abs(lam_ref)))
    sub = (names[3], names[0])
    one = S.wc_ratio_gradient_continuous(model, grids, w, g, wrt=sub, rtol=SOLVE_RTOL, operator=op)
    assert set(one) == set(sub) | {"_info", "_adjoint"}
    single = S.wc_ratio_gradient_continuous(model, grids, w, g, wrt=names[1], rtol=SOLVE_RTOL, operator=op)
    assert set(single) == {names[1], "_info", "_adjoint"}
    dflt = S.wc_ratio_gradient_continuous(model, grids, w, g, rtol=SOLVE_RTOL, d=QUAD_D)
    for k, nm in enumerate(names):
        bound = solve * lam_max * sum_dT[k] + RTOL_SUM * comp[k]
        assert abs(dflt[nm] - ref[k]) <= bound, nm
        if nm in sub:
            assert abs(one[nm] - ref[k]) <= bound, nm


# -- 6. the C ABI -----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals(S):
    import torch
    from sdfs_via_autodiff_amd import _lib
    lib = _lib.lib
    ARG, UNSUP = _lib.SDFS_ERR_ARG, _lib.SDFS_ERR_UNSUPPORTED
    ssy = S.SSY()
    shapes = (2, 3, 4, 5)
    g = torch.full(shapes, 700.0, dtype=torch.float64, device="cuda")
    o, t = torch.empty_like(g), torch.empty_like(g)
    it, rel = C.c_int64(), C.c_double()
    torch.cuda.synchronize()
    # a discretised and a dense handle, linearised: both new symbols refuse them
    disc = S.ssy_operator(shapes, ssy.params, S.discretize_ssy(ssy, shapes))
    disc.linearize_dev(g.data_ptr())
    assert lib.sdfs_cont_apply_vjp_dev(disc._h, g.data_ptr(), o.data_ptr(), 0) == UNSUP
    assert "continuous-state handles only" in _lib.last_error(disc._h)
    assert lib.sdfs_cont_solve_adjoint_dev(disc._h, None, g.data_ptr(), o.data_ptr(), C.byref(it), C.byref(rel)) == UNSUP
    assert "continuous-state handles only" in _lib.last_error(disc._h)
    dense = S.DenseOperator(np.full((6, 6), 1.0 / 6), 0.99, -30.0)
    g6 = torch.full((6,), 700.0, dtype=torch.float64, device="cuda")
    o6 = torch.empty_like(g6)
    torch.cuda.synchronize()
    dense.linearize_dev(g6.data_ptr())
    assert lib.sdfs_cont_apply_vjp_dev(dense._h, g6.data_ptr(), o6.data_ptr(), 0) == UNSUP
    assert lib.sdfs_cont_solve_adjoint_dev(dense._h, None, g6.data_ptr(), o6.data_ptr(), None, None) == UNSUP
    # a continuous handle
    grids = S.build_grid(ssy, *shapes)
    nodes, weights = S.qnwnorm([2] * 4)
    op = S.ContinuousOperator(np.array(ssy.params), grids, np.ascontiguousarray(nodes.T), weights)
    h = op._h
    # before any linearisation
    assert lib.sdfs_cont_apply_vjp_dev(h, g.data_ptr(), o.data_ptr(), 0) == ARG
    assert "before a linearisation" in _lib.last_error(h)
    assert lib.sdfs_cont_solve_adjoint_dev(h, None, g.data_ptr(), o.data_ptr(), None, None) == ARG
    assert "before a linearisation" in _lib.last_error(h)
    assert lib.sdfs_cont_apply_vjp_dev(h, None, o.data_ptr(), 0) == ARG
    assert lib.sdfs_cont_apply_vjp_dev(h, g.data_ptr(), g.data_ptr(), 0) == ARG
    want = op(np.full(shapes, 700.0))
    op.linearize_dev(g.data_ptr())
    assert lib.sdfs_cont_apply_vjp_dev(h, None, o.data_ptr(), 0) == ARG
    assert lib.sdfs_cont_apply_vjp_dev(h, g.data_ptr(), None, 0) == ARG
    assert lib.sdfs_cont_apply_vjp_dev(h, g.data_ptr(), g.data_ptr(), 0) == ARG
    assert "in place" in _lib.last_error(h)
    assert lib.sdfs_cont_solve_adjoint_dev(h, None, None, o.data_ptr(), None, None) == ARG
    assert lib.sdfs_cont_solve_adjoint_dev(h, None, g.data_ptr(), None, None, None) == ARG
    bad = _lib.default_opts()
    bad.krylov_f32 = 1
    assert lib.sdfs_cont_solve_adjoint_dev(h, C.byref(bad), g.data_ptr(), o.data_ptr(), None, None) == ARG
    # the discretised operator's names keep refusing a continuous handle
    assert lib.sdfs_apply_vjp_dev(h, g.data_ptr(), o.data_ptr(), 0) == UNSUP
    assert "discretised operator only" in _lib.last_error(h)
    assert lib.sdfs_solve_linear_dev(h, 1, None, g.data_ptr(), o.data_ptr(), None, None) == UNSUP
    assert "discretised operator only" in _lib.last_error(h)
    hw, ho = np.full(shapes, 700.0), np.empty(shapes)
    assert lib.sdfs_apply_vjp(h, hw.ctypes.data, hw.ctypes.data, ho.ctypes.data) == UNSUP
    with pytest.raises(_lib.SdfsError):
        op.vjp_dev(g.data_ptr(), o.data_ptr())
    with pytest.raises(_lib.SdfsError):
        op.solve_linear_dev(g.data_ptr(), o.data_ptr(), True)
    # the handle still applies T bit for bit, and the new calls themselves work
    op.apply_dev(g.data_ptr(), t.data_ptr())
    op.synchronize()
    assert np.array_equal(t.cpu().numpy(), want)
    assert lib.sdfs_cont_apply_vjp_dev(h, g.data_ptr(), o.data_ptr(), 1) == 0
    op.synchronize()
    assert bool(torch.all(torch.isfinite(o)))
    assert lib.sdfs_cont_solve_adjoint_dev(h, None, g.data_ptr(), o.data_ptr(), C.byref(it), C.byref(rel)) == 0
    assert it.value >= 1 and rel.value <= _lib.default_opts().inner_rtol and bool(torch.all(torch.isfinite(o)))   # (opts NULL)
    op.apply_dev(g.data_ptr(), t.data_ptr())
    op.synchronize()
    assert np.array_equal(t.cpu().numpy(), want)

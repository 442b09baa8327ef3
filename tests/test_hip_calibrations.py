"""
GPU tests of every kernel plan and precision form away from the default calibration.

Every kernel raises the grid to a power fixed per launch -- theta = (1 - gamma) / (1 - 1 / psi), 1 / theta, theta - 1,
1 / theta - 1 -- and the handle builds its pre-scaled power tables, beta^theta, the range test of the fast power, the
power-of-two scales of the fp32 forms, the split of a3, the tilt and tangent tables and the batch kernels' per-member
blocks from theta, gamma and beta when it is created.  The rest of the GPU suite runs at the default calibration
(theta = -16 for SSY, -36 for GCY); here the same checks run at the calibrations of tests/calibrations.py: theta = -38
(steep), -6.2 (shallow), +20 (positive), +0.4 (fractional), exactly 1 (linear), and the default theta with every other
field of the model moved (shifted).  tests/test_oracle_calibrations.py pins the oracle to the reference at these.

Part 2 (the operator on every plan): T with its residual, the linearising T, J.v and J^T.u with their minus-identity
device forms and the device SA loop for k = 1, 2, 3, against the C oracle built from the oracle's own parameters and
discretisation, at w = level (0.6 + 0.8 U) with level 600 and level 5 (below the range the fast power routine takes
without its range test at large |theta|).  Bounds as the plan tests': T and residual 1e-12 relative, J.v and J^T.u
1e-11 of their maximum, SA iterates 1e-11, final_err 1e-9.  Each case asserts the plan it runs on from
describe_plan(), the padded cases also the tile width of every pass (16, 20, 24 and 32 wide all occur).  At `linear` J.v does not depend on w; at `steep` and `positive` the full-range power path is taken.

Part 3 (the reduced-precision forms): krylov_f32 = 1, 2, 3 through the storage hook and one application of T with
t_f32, under the derived bounds of tests/f32_bound.py, at `steep`, `positive` and `fractional`.

Part 4 (what is built on the operator): the parameter tangents against the oracle's complex step, the tilted products,
simulate at the fixed point of `positive`, and the batch kernels (SA, Newton, gradient, prices, simulation) on one
batch of eight members with theta from -38 to +20, forwards and reversed.  Each is the body of an existing test, run
with another model, with that test's oracle and bound.

Every figure is printed before it is held to its bound (lines starting with CALSWEEP / F32-MEASURED under pytest -s;
tools/calibration_sweep_profile.py makes profiles/calibration_sweep_errors.txt from them).  Every test runs under its own time limit (SIGALRM).
"""
import signal

import numpy as np
import pytest

import calibrations as C
from test_hip_vjp import env, assert_plan, SMALL, PAIR, PADDED, STREAMED_MID
from test_hip_last_pass_streams import NEW_LINE, OLD_LINE

pytestmark = pytest.mark.gpu

APPLY_RTOL = 1e-12
JV_RTOL = 1e-11
SA_RTOL = 1e-11
ERR_RTOL = 1e-9
LEVELS = (600.0, 5.0)


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


def limit(seconds):
    def mark(fn):
        fn.time_limit_s = seconds
        return fn
    return mark


# -- the families: (model, shapes, create-time knobs, plan marker) -----------------------------------------------------
LAST_PASS = "last pass, both side-stream forms"
FAMILIES = {
    "small": ("ssy", (15,) * 4, dict(SDFS_PLAN=None), SMALL),
    "generic": ("ssy", (4, 7, 6, 5), dict(SDFS_PLAN="classic"), None),
    "pair4d": ("ssy", (16,) * 4, dict(SDFS_PLAN="pair"), PAIR),
    "lastpass": ("ssy", (20,) * 4, dict(SDFS_PLAN="pair", SDFS_LINE_STREAM=7), LAST_PASS),
    "pad20": ("ssy", (20,) * 4, dict(SDFS_PLAN=None, SDFS_PAD_PLAN=1), PADDED),
    "pad16": ("gcy", (10,) * 6, dict(SDFS_PLAN=None), PADDED),
    "pad32": ("ssy", (25, 18, 32, 7), dict(SDFS_PLAN=None, SDFS_PAD_PLAN=2), PADDED),
    "pad24_32": ("ssy", (22, 18, 32, 7), dict(SDFS_PLAN=None, SDFS_PAD_PLAN=2), PADDED),
    "pair6d": ("gcy", (16,) * 6, dict(SDFS_PLAN="pair", SDFS_LINE_STREAM=0), PAIR),
    "streamed": ("gcy", (16,) * 6, dict(SDFS_PLAN="pair", SDFS_LINE_STREAM=7), STREAMED_MID),
}
# Tile width of each pass of the padded families, first pass first, as describe_plan() labels them ("... on NxN]"): the
# width is the class of the larger extent of the pass's axis pair (<= 16, <= 20, <= 24, <= 32), and a 4-D grid pairs axes
# (2, 3) then (0, 1).  SSY (25, 18, 32, 7) is 32 wide on both passes (25 > 24), so the 24-wide tiles have a shape of their
# own, (22, 18, 32, 7): 32 wide on (32, 7), 24 wide on (22, 18).
PAD_WIDTHS = {"pad16": (16, 16, 16), "pad20": (20, 20), "pad32": (32, 32), "pad24_32": (32, 24)}
# (lastpass and pad20 share the oracle results of SSY 20^4: they are neighbours)
SMALL_FAMILIES = ["small", "generic", "pair4d", "lastpass", "pad20", "pad16", "pad32", "pad24_32"]
BIG_FAMILIES = ["pair6d", "streamed"]
BIG_CALIBRATIONS = ["steep", "positive", "fractional"]


def disc(S, kind):
    return S.discretize_ssy if kind == "ssy" else S.discretize_gcy


def build(S, family, cal):
    """The library's operator of a family at a calibration, on the plan the family names."""
    kind, shapes, knobs, marker = FAMILIES[family]
    m = C.package_model(S, kind, cal)
    with env(**knobs):
        op = S.KoopmansOperator(kind, shapes, m.params, disc(S, kind)(m, shapes))
    if marker == LAST_PASS:
        # 20 wide: a T that reads the side stream (a residual is asked for) runs the form with its loads in flight with
        # the tile's, a T without one and every linearising T the form that loads it behind the tile or not at all
        desc = assert_plan(op, PAIR)
        assert "streamed" in desc and NEW_LINE in desc and OLD_LINE not in desc, desc
    elif marker == STREAMED_MID:
        assert STREAMED_MID in assert_plan(op, PAIR)
    elif marker == PADDED:
        lines = [ln for ln in assert_plan(op, PADDED).splitlines() if ln.startswith(PADDED)]
        assert len(lines) == len(shapes) // 2, lines
        for ln, nt in zip(lines, PAD_WIDTHS[family]):
            assert f" on {nt}x{nt}]" in ln, lines
    elif family == "pair6d":
        assert "streamed" not in assert_plan(op, PAIR)
    else:
        assert_plan(op, marker)
    return op


# -- the oracle side: the results of one (model, shapes, calibration) are kept at a time, both levels of a grid below
# 10^7 points and one level above (16^6: 8 arrays of 134 MB); families that share a shape are neighbours in the
# parametrisations below
_REF = {}
_REF_GROUP = [None]


def inputs(shapes, level):
    """w = level (0.6 + 0.8 U); v and u standard normal, the same at every level."""
    w = level * (0.6 + 0.8 * np.random.default_rng(11).random(shapes))
    v = np.random.default_rng(12).standard_normal(shapes)
    u = np.random.default_rng(13).standard_normal(shapes)
    return w, v, u


def oracle_operator(kind, shapes, cal):
    """The C oracle on the oracle's own parameter tuple and discretisation (nothing of the library's host side)."""
    from oracle import ssy, gcy
    from oracle.c_oracle import COperator
    p = C.oracle_params(kind, cal)
    arr = (ssy.discretize_ssy if kind == "ssy" else gcy.discretize_gcy)(p, shapes)
    return COperator(kind, shapes, p, arr)


def reference(kind, shapes, cal, level):
    key = (kind, shapes, cal, level)
    group = key if int(np.prod(shapes)) > 10 ** 7 else key[:3]
    if group != _REF_GROUP[0]:
        _REF.clear()
        _REF_GROUP[0] = group
    if key not in _REF:
        oc = oracle_operator(kind, shapes, cal)
        w, v, u = inputs(shapes, level)
        r = dict(w=w, v=v, u=u, Jv=oc.jvp(w, v), JTu=oc.vjp(w, u))
        x, sa = w, []
        for _ in range(3):
            x = oc(x)
            sa.append(x)
        r["sa"] = sa
        for a in [w, v, u, r["Jv"], r["JTu"]] + sa:
            assert np.all(np.isfinite(a))
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def note(family, cal, what, err, bound):
    """Print the figure (profiles/calibration_sweep_errors.txt is made from these lines), then hold it to its bound."""
    print(f"CALSWEEP {family} {cal} {what} {err:.3e} {bound:.1e}")
    assert err <= bound, f"{family} {cal} {what}: {err:.3e} > {bound:.1e}"


def check_operator(S, family, cal, level):
    import torch
    kind, shapes, _, _ = FAMILIES[family]
    op = build(S, family, cal)
    r = reference(kind, shapes, cal, level)
    w, v, u, Tw, Jv, JTu = r["w"], r["v"], r["u"], r["sa"][0], r["Jv"], r["JTu"]
    tag = f"L{level:g}"
    # T with its residual (on 20^4: the form that reads the side stream with the tile)
    got = op(w)
    note(family, cal, f"T {tag}", np.max(np.abs(got - Tw) / np.abs(Tw)), APPLY_RTOL)
    res = float(np.max(np.abs(Tw - w)))
    note(family, cal, f"residual {tag}", abs(op.residual() - res) / res, APPLY_RTOL)
    # T without a residual, then the linearising T and the four device products on that linearisation
    wd, vd, ud = op._to_dev(w, v, u)
    out = torch.empty_like(wd)
    op.apply_dev(wd.data_ptr(), out.data_ptr(), None)
    op.synchronize()
    note(family, cal, f"T no residual {tag}", np.max(np.abs(out.cpu().numpy() - Tw) / np.abs(Tw)), APPLY_RTOL)
    op.linearize_dev(wd.data_ptr(), out.data_ptr())
    op.synchronize()
    note(family, cal, f"T linearising {tag}", np.max(np.abs(out.cpu().numpy() - Tw) / np.abs(Tw)), APPLY_RTOL)
    for name, fn, xd, x, want in (("J.v", op.jvp_dev, vd, v, Jv), ("J^T.u", op.vjp_dev, ud, u, JTu)):
        scale = float(np.max(np.abs(want)))
        fn(xd.data_ptr(), out.data_ptr(), minus_identity=False)
        op.synchronize()
        note(family, cal, f"{name} {tag}", np.max(np.abs(out.cpu().numpy() - want)) / scale, JV_RTOL)
        fn(xd.data_ptr(), out.data_ptr(), minus_identity=True)
        op.synchronize()
        note(family, cal, f"{name} - identity {tag}", np.max(np.abs(out.cpu().numpy() - (want - x))) / scale, JV_RTOL)
        np.testing.assert_array_equal(xd.cpu().numpy(), x)
    # the device SA loop
    prev = w
    for k in (1, 2, 3):
        x = r["sa"][k - 1]
        xk, n, info = op.solve(w, "successive_approx", tol=0.0, max_iter=k)
        assert n == k
        note(family, cal, f"SA iterate {tag}", np.max(np.abs(xk - x) / np.abs(x)), SA_RTOL)
        err = float(np.max(np.abs(x - prev)))
        note(family, cal, f"SA final_err {tag}", abs(info["final_err"] - err) / err, ERR_RTOL)
        prev = x
    op.close()


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("family", SMALL_FAMILIES)
@pytest.mark.parametrize("cal", C.NAMES)
def test_operator_on_every_plan(S, cal, family, level):
    check_operator(S, family, cal, level)


@limit(600)
@pytest.mark.parametrize("family", BIG_FAMILIES)
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("cal", BIG_CALIBRATIONS)
def test_operator_on_the_6d_pair_plan(S, cal, level, family):
    """GCY 16^6, the middle pass in its one-tile-per-workgroup and its persistent form: both families share one set of
    oracle results per calibration and level (the family varies fastest; the oracle is the slow side at this size)."""
    check_operator(S, family, cal, level)


@pytest.mark.parametrize("family", SMALL_FAMILIES)
def test_linear_calibration_jacobian_does_not_depend_on_w(S, family):
    """theta = 1: T is affine in w, so J.v linearised at two different w is the same vector, to 1e-13 of its maximum
    (w^(theta-1) and (K S)^(1/theta-1) are both a zeroth power)."""
    import torch
    kind, shapes, _, _ = FAMILIES[family]
    op = build(S, family, "linear")
    wa, v, _ = inputs(shapes, 600.0)
    wb = 5.0 * (0.6 + 0.8 * np.random.default_rng(21).random(shapes))
    res = []
    for w in (wa, wb):
        wd, vd = op._to_dev(w, v)
        out = torch.empty_like(wd)
        op.linearize_dev(wd.data_ptr(), None)
        op.jvp_dev(vd.data_ptr(), out.data_ptr(), minus_identity=False)
        op.synchronize()
        res.append(out.cpu().numpy())
    scale = np.max(np.abs(res[0]))
    assert scale > 0
    note(family, "linear", "J.v at two w", np.max(np.abs(res[0] - res[1])) / scale, 1e-13)
    op.close()


@pytest.mark.parametrize("family", ["pair4d", "pad20"])
@pytest.mark.parametrize("cal", ["steep", "positive"])
def test_full_range_power_path(S, cal, family):
    """tests/test_hip_pair_plan.py's full-range case at theta = -38 and +20: values that leave the straight-line power
    routine, put in one after the other because each swamps the ones before (the Rouwenhorst matrices have no zero
    entry, so every point reaches every other):
      a 1e12        theta < 0: 1e12^theta underflows; theta > 0: 1e240, far beyond the fast range but finite -- T w is
                    finite everywhere and depends on theta;
      then          theta < 0: a 1e300 (underflows as well); theta > 0: a 0 (0^theta = 0) -- T w still finite;
      then          theta < 0: a 0, 0^theta = +inf, S = +inf and T w = 1 at every point, residual finite (about 1e300);
                    theta > 0: a 1e300, which overflows, T w = +inf everywhere, residual +inf;
      then a -1     NaN where the oracle has it and nowhere else, residual +inf.
    No NaN before the negative w goes in; everything that is not NaN to 1e-12 each time."""
    from oracle import ssy
    kind, shapes, _, _ = FAMILIES[family]
    op = build(S, family, cal)
    p = C.oracle_params(kind, cal)
    arr = ssy.discretize_ssy(p, shapes)
    w = inputs(shapes, 600.0)[0].copy()
    zero, huge = ((0, 0, 0, 0), 0.0), ((9, 9, 9, 9), 1e300)
    stages = [((5, 6, 7, 8), 1e12)] + ([huge, zero] if C.theta(kind, cal) < 0 else [zero, huge]) + [((3, 4, 5, 6), -1.0)]
    for stage, (at, value) in enumerate(stages):
        w[at] = value
        with np.errstate(all="ignore"):
            want = ssy.T_ssy_factorised(w, shapes, p, arr)
        got = op(w)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert bool(np.isnan(want).any()) == (stage == 3)
        assert np.all(np.isfinite(want)) == (stage < 2 or (stage == 2 and C.theta(kind, cal) < 0))
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
        ok = np.isfinite(want)
        if ok.any():
            note(family, cal, f"full range, stage {stage} (w = {value:g} added)",
                 np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok])), APPLY_RTOL)
        if np.all(ok):
            r = float(np.max(np.abs(want - w)))
            note(family, cal, f"full range residual, stage {stage}", abs(op.residual() - r) / r, APPLY_RTOL)
        else:
            assert op.residual() == np.inf
    op.close()


# ======================================================================================================================
# Part 3: the reduced-precision forms at theta = -38, +20 and +0.4 (bounds: tests/f32_bound.py, derived, unchanged)
# ======================================================================================================================
F32_CALIBRATIONS = ["steep", "positive", "fractional"]
# (shapes, knobs, what jvp_forms expects, plan marker): the fp32-MFMA kernels; the generic fp32 passes behind the
# small-grid plan and behind the padded plan
F32_FAMILIES = {"mfma": ((16, 16, 24, 24), dict(SDFS_PLAN="pair"), "mfma", PAIR),
                "small": ((15,) * 4, dict(SDFS_PLAN=None), "generic", SMALL),
                "pad20": ((20,) * 4, dict(SDFS_PLAN=None, SDFS_PAD_PLAN=1), "generic", PADDED)}


@pytest.mark.parametrize("family", list(F32_FAMILIES))
@pytest.mark.parametrize("cal", F32_CALIBRATIONS)
def test_krylov_f32_forms(S, cal, family):
    """krylov_f32 = 1, 2, 3 with m = 0 and 1 through the storage hook at w = wbench (no Newton solve first):
    |got - want| <= C u (J|v| + m|v|) and err > 0, the plan and the counters as tests/test_hip_f32_forms.py names them."""
    from test_hip_f32_forms import jvp_forms
    shapes, knobs, expect, marker = F32_FAMILIES[family]
    m = C.package_model(S, "ssy", cal)
    desc = jvp_forms(S, "ssy", shapes, f"calibration {cal}", expect, knobs,
                     tensors=(m.params, list(S.discretize_ssy(m, shapes))), fixed_point=False)
    if marker == PAIR:
        assert PAIR in desc and PADDED not in desc and "mfma32 none" not in desc, desc
    else:
        assert marker in desc, desc
    if family == "pad20":
        assert desc.count(" on 20x20]") == 2, desc


@pytest.mark.parametrize("shapes", [(16, 16, 24, 24), (32, 32, 16, 16), (20, 20, 20, 20)])
@pytest.mark.parametrize("cal", F32_CALIBRATIONS)
def test_t_f32_one_application(S, cal, shapes):
    """One application of T with fp32 intermediates on the 4-D shapes of T32_SHAPES, held to t32_bound(T, theta) with
    the model's own theta (at theta = 0.4 the bound is 40 times the default's: a relative error of S is divided by
    theta on its way to T - 1)."""
    from test_hip_f32_forms import T32_SHAPES, t32_one_application
    assert ("ssy", shapes) in T32_SHAPES
    m = C.package_model(S, "ssy", cal)
    assert m.θ == C.theta("ssy", cal)
    used = t32_one_application(S, "ssy", shapes, f"calibration {cal}",
                               tensors=(m.params, list(S.discretize_ssy(m, shapes))), theta=m.θ)
    print(f"CALSWEEP t_f32-ssy{'x'.join(map(str, shapes))} {cal} fraction of t32_bound {used:.3e} 1.0e+00")


# ======================================================================================================================
# Part 4: what is built on the operator
# ======================================================================================================================
# The Richardson test of tests/test_hip_sensitivity.py holds the tangents to 1e-7 of max|dT/dp|, the truncation error of
# its differences.  The complex step has none: the worst case measured on an MI355X over every calibration, family and
# parameter is 6.33e-12 (gamma at `fractional` on the generic tiles), so the bound here is ten times that.
TANGENT_RTOL = 6.4e-11


@pytest.mark.parametrize("family", ["small", "generic"])
@pytest.mark.parametrize("cal", ["steep", "positive", "fractional", "shifted"])
def test_parameter_tangents_vs_complex_step(S, cal, family):
    """dT(w)/dp at a fixed w for every parameter -- the supported ones through sdfs_param_tangent_dev, the persistences
    with their generators through sdfs_param_tangent_gen_dev -- against the complex step of the oracle's T along the
    same direction, within TANGENT_RTOL of max|dT/dp|."""
    import persistence_oracle as po
    from test_hip_persistence import all_names, direction, persistence_names
    kind, shapes, _, _ = FAMILIES[family]
    op = build(S, family, cal)
    m = C.package_model(S, kind, cal)
    arr = disc(S, kind)(m, shapes)
    w = 500.0 + 200.0 * np.random.default_rng(sum(shapes)).random(shapes)
    names = all_names(kind)
    assert len(names) == 13 and set(persistence_names(kind)) < set(names)
    for name in names:
        dp, da, dgen = direction(S, kind, m, shapes, name)
        assert (dgen is not None) == (name in persistence_names(kind))
        got = op.param_tangent(w, dp, da, dgen=dgen)
        want = po.complex_step_tangent(kind, shapes, m.params, arr, dp, da, w)
        scale = float(np.max(np.abs(want)))
        assert scale > 0 and np.all(np.isfinite(want))
        note(family, cal, f"tangent {name}", np.max(np.abs(got - want)) / scale, TANGENT_RTOL)
    op.close()


@limit(300)
@pytest.mark.parametrize("cal", ["positive", "steep"])
def test_tilted_product_and_sdf_expectation(S, cal):
    """The first case of test_tilted_product_vs_oracle (SSY 15^4, small-grid plan) with its four tilts -- (1, theta,
    -gamma) is E_x[M] -- and its bound, 1e-12 relative."""
    from test_hip_pricing import PLAN_CASES, tilted_product_case
    kind, shapes, plan, marker, c_oracle = PLAN_CASES[0]
    worst = tilted_product_case(S, kind, shapes, plan, marker, c_oracle, m=C.package_model(S, kind, cal))
    print(f"CALSWEEP small {cal} tilted product {worst:.3e} 1.0e-12")


SIM_BOUNDS = (1e-12, 1e-10, 1e-9)       # series, statistics against the two-pass formulas, statistics against the twin


@limit(300)
@pytest.mark.parametrize("kappa", [None, 2.0])
def test_simulate_at_the_positive_calibration(S, kappa):
    """simulate at the fixed point of `positive` on SSY (5, 4, 6, 7): index paths, series and per-path statistics
    against tests/sim_oracle.py with the bounds of tests/test_hip_simulation.py (theta - 1 > 0 in the log SDF)."""
    from test_hip_simulation import GRIDS, paths_series_and_statistics_case
    kind, shapes = "ssy", (5, 4, 6, 7)
    assert (kind, shapes) in GRIDS
    worst = paths_series_and_statistics_case(S, kind, shapes, "stationary", 7, kappa,
                                             m=C.package_model(S, kind, "positive"), tag="positive")
    for (what, value), bound in zip(worst.items(), SIM_BOUNDS):         # (asserted by the body; printed here)
        note("simulate", "positive", f"{what}, kappa {kappa}", value, bound)


# -- the batch kernels: one batch of eight members, theta from -38 to +20 -----------------------------------------------
BATCH_SHAPES = [("ssy", (5,) * 4), ("gcy", (3,) * 6)]
BATCH_IDS = ["ssy5", "gcy3"]
TIGHT_NEWTON = dict(algorithm="newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
_batch_w = {}


def batch_overrides(kind):
    """Two members of tests/batch_family.py, then the six calibrations: the members with theta > 0 (positive,
    fractional, linear) sit between members with theta < 0."""
    from batch_family import member
    return [member(kind, 0), member(kind, 1)] + [C.overrides(kind, name) for name in C.NAMES]


def batch_models(S, kind):
    cls = S.SSY if kind == "ssy" else S.GCY
    models = [cls(**C.greek(over)) for over in batch_overrides(kind)]
    signs = [m.θ > 0 for m in models]
    assert signs == [False, False, False, False, True, True, True, False]
    return models


def batch_fixed_points(S, kind, shapes):
    """w* of the eight members by the batch Newton solve from 800, as the batch suites solve theirs (once per module)."""
    if kind not in _batch_w:
        res = S.solve_batch(batch_models(S, kind), shapes, **TIGHT_NEWTON)
        assert res.plan == "batch" and np.all(res.status == 0), (res.plan, res.status)
        _batch_w[kind] = res.w
    return _batch_w[kind]


@pytest.mark.parametrize("kind,shapes", BATCH_SHAPES, ids=BATCH_IDS)
def test_batch_sa_iterates(S, kind, shapes):
    """solve_batch, k = 1, 2, 3 applications from 800: every member against oracle_apply with its own overrides, rtol
    1e-11 (tests/test_hip_batch.py); the reversed batch gives the reversed result bit for bit."""
    from batch_family import oracle_apply
    models, overs = batch_models(S, kind), batch_overrides(kind)
    for k in (1, 2, 3):
        res = S.solve_batch(models, shapes, tol=0.0, max_iter=k)
        assert res.plan == "batch" and np.all(res.n_iter == k) and np.all(res.status == 1)
        for b, over in enumerate(overs):
            want = oracle_apply(kind, shapes, over, np.full(shapes, 800.0), k)
            assert np.all(np.isfinite(want))
            note(f"batch-{kind}", f"member{b}", f"SA k={k}", np.max(np.abs(res.w[b] - want) / np.abs(want)), 1e-11)
        rev = S.solve_batch(models[::-1], shapes, tol=0.0, max_iter=k)
        assert np.array_equal(rev.w, res.w[::-1]) and np.array_equal(rev.error, res.error[::-1])
        assert np.array_equal(rev.n_iter, res.n_iter[::-1]) and np.array_equal(rev.status, res.status[::-1])


@pytest.mark.parametrize("kind,shapes", BATCH_SHAPES, ids=BATCH_IDS)
def test_batch_newton(S, kind, shapes):
    """solve_batch(algorithm="newton") with the options of tests/test_hip_batch_newton.py: status 0 for every member,
    within 1e-8 of the oracle's polished fixed point, oracle residual <= 1e-9; reversed batch, reversed bits."""
    from batch_newton_family import INNER_RTOL, TOL, oracle_ops
    from oracle import solvers as osolvers
    models, overs = batch_models(S, kind), batch_overrides(kind)
    opts = dict(algorithm="newton", tol=TOL, inner_rtol=INNER_RTOL, inner_atol=0.0)
    res = S.solve_batch(models, shapes, **opts)
    assert res.plan == "batch" and np.all(res.status == 0), res.status
    for b, over in enumerate(overs):
        T, jvp = oracle_ops(kind, shapes, over)
        with np.errstate(all="ignore"):
            wo, _ = osolvers.newton_solver(T, np.full(shapes, 800.0), tol=TOL, verbose=False, jvp=jvp,
                                           bicgstab_tol=INNER_RTOL, bicgstab_atol=0.0)
            wstar = osolvers.newton_polish(T, jvp, wo)
        assert np.max(np.abs(T(wstar) - wstar)) <= 1e-11
        note(f"batch-{kind}", f"member{b}", "newton max|w - w*|", np.max(np.abs(res.w[b] - wstar)), 1e-8)
        note(f"batch-{kind}", f"member{b}", "newton residual", np.max(np.abs(T(res.w[b]) - res.w[b])), 1e-9)
        assert res.n_apply[b] > res.n_iter[b] > 0
    rev = S.solve_batch(models[::-1], shapes, **opts)
    for f in ("w", "n_iter", "error", "status", "n_apply"):
        assert np.array_equal(getattr(rev, f), getattr(res, f)[::-1]), f


@limit(300)
@pytest.mark.parametrize("kind,shapes", BATCH_SHAPES, ids=BATCH_IDS)
def test_batch_gradient(S, kind, shapes):
    """gradient_batch at the members' fixed points: all 13 / 18 entries of every member against <lambda_dense,
    complex-step dT/dp> (tests/batch_adjoint_oracle.py), within 1e-8 |want| (test_gradient_against_dense_truth);
    status 0; reversed batch, reversed bits."""
    import batch_adjoint_oracle as bao
    models, overs = batch_models(S, kind), batch_overrides(kind)
    w = batch_fixed_points(S, kind, shapes)
    g = 0.5 + np.random.default_rng(9).random((len(models),) + shapes)
    res = S.gradient_batch(models, shapes, w, g, rtol=1e-12)
    assert res.plan == "batch" and np.all(res.status == 0), (res.plan, res.status)
    assert res.grad.shape == (len(models), 13 if kind == "ssy" else 18)
    for b, over in enumerate(overs):
        params, arrays = bao.oracle_inputs(kind, shapes, over)
        lam = bao.dense_lambda(kind, shapes, params, arrays, w[b], g[b])
        truth = bao.truth_gradient(S, kind, shapes, models[b], params, arrays, w[b], lam)
        for k, nm in enumerate(res.names):
            want = truth[nm]
            note(f"batch-{kind}", f"member{b}", f"gradient {nm}", abs(res.grad[b, k] - want) / abs(want), 1e-8)
    rev = S.gradient_batch(models[::-1], shapes, w[::-1].copy(), g[::-1].copy(), rtol=1e-12)
    assert np.array_equal(rev.grad, res.grad[::-1]) and np.array_equal(rev.status, res.status[::-1])


@limit(300)
@pytest.mark.parametrize("kind,shapes", BATCH_SHAPES, ids=BATCH_IDS)
def test_batch_prices(S, kind, shapes):
    """price_batch (kappa = 2, 50 horizons, rtol 1e-12) with the checks and bounds of tests/test_hip_batch_pricing.py:
    E_M and E_M2 to 1e-12 of tests/batch_pricing_oracle.py's member, the claim's true residual <= 1e-10, resid_T <=
    1e-9, the twelve words within 1e-11 sum|terms| of the restatement; status 0; reversed batch, reversed bits."""
    import batch_pricing_oracle as bpo
    from test_hip_batch_pricing import KAPPA, n_max_of, rel_err
    models = batch_models(S, kind)
    w = batch_fixed_points(S, kind, shapes)
    kw = dict(kappa=KAPPA, n_max=n_max_of(shapes), rtol=1e-12, return_grids=True)
    res = S.price_batch(models, shapes, w, **kw)
    assert res.plan == "batch" and np.all(res.status == 0), (res.plan, res.status)
    for b, m in enumerate(models):
        mem = bpo.Member(kind, shapes, m, bpo.discretize(S, kind, m, shapes), w[b])
        note(f"batch-{kind}", f"member{b}", "E_M", rel_err(res.grids["E_M"][b], mem.E_M()), 1e-12)
        note(f"batch-{kind}", f"member{b}", "E_M2", rel_err(res.grids["E_M2"][b], mem.E_M2()), 1e-12)
        v = res.grids["pd"][b]
        r, k1 = mem.claim_residual(v, KAPPA)
        note(f"batch-{kind}", f"member{b}", "claim true residual", np.linalg.norm(r) / np.linalg.norm(k1), 1e-10)
        note(f"batch-{kind}", f"member{b}", "resid_T", res.resid_T[b], 1e-9)
        assert np.all(v > 0) and res.moments[b, 11] == 0.0 and res.n_horizons[b] == n_max_of(shapes)
        gw = bpo.point_weights(S.stationary_weights(m, shapes))
        gr = res.grids
        want, scale = bpo.words(gw, gr["E_M"][b], gr["E_M2"][b], gr["pd"][b], gr["expected_return"][b])
        note(f"batch-{kind}", f"member{b}", "words", np.max(np.abs(res.moments[b][:9] - want[:9]) / scale[:9]), 1e-11)
        assert np.array_equal(res.moments[b][9:], want[9:])
    rev = S.price_batch(models[::-1], shapes, w[::-1].copy(), **kw)
    assert np.array_equal(rev.moments, res.moments[::-1]) and np.array_equal(rev.status, res.status[::-1])
    for name in res.grids:
        assert np.array_equal(rev.grids[name], res.grids[name][::-1]), name


@limit(300)
@pytest.mark.parametrize("kind,shapes", BATCH_SHAPES, ids=BATCH_IDS)
def test_batch_simulation(S, kind, shapes):
    """simulate_batch: every member against the twin of tests/sim_oracle.py with the bounds of
    tests/test_hip_batch_simulation.py (stationary start, burn-in 7, a claim with kappa = 2); status 0; reversed batch,
    reversed bits."""
    from test_hip_batch_simulation import P, SEED, T, assert_same_member, every_member_matches_the_twin
    models = batch_models(S, kind)
    w = batch_fixed_points(S, kind, shapes)
    _, worst = every_member_matches_the_twin(S, kind, shapes, "stationary", 7, 2.0, models, w)
    for (what, value), bound in zip(worst.items(), SIM_BOUNDS):         # (asserted by the body; printed here)
        note(f"batch-{kind}", "all", f"simulation {what}", value, bound)
    kw = dict(burn_in=7, seed=SEED, path_offset=123, kappa=2.0, return_per_path=True, return_paths=True)
    res = S.simulate_batch(models, shapes, w, P, T, **kw)
    rev = S.simulate_batch(models[::-1], shapes, w[::-1].copy(), P, T, **kw)
    assert res.plan == "batch" and np.all(res.status == 0) and np.all(rev.status == 0), (res.plan, res.status)
    for b in range(len(models)):
        assert_same_member(res, b, rev, len(models) - 1 - b)

"""
GPU tests of the reduced-precision operator forms, one product at a time, against the fp64 C oracle:

  (a) J.v in the storage of Newton's inner solve (opts.krylov_f32 = 1 fp32, 2 bf16-rounded, 3 fp32 LDS tiles + fp32
      MFMA), through the test hook sdfs_debug_jvp_storage_dev, on the pair plan (every row width, the persistent fp32
      middle pass and its one-tile-per-workgroup form), conditional tensors, and the generic fp32 passes the small-grid,
      padded and classic plans fall back to;
  (b) the handle's state after the hook;
  (c) one Newton step with the fused fp32 BiCGSTAB forms (jvpm32+p / +s, the dot3 last pass), its true residual;
  (d) one application of T with fp32 intermediates (opts.t_f32), every form of its passes.

Bounds: tests/f32_bound.py (derivation there, pinned on the CPU by tests/test_f32_bounds_cpu.py).  Every case runs on
the Rouwenhorst tensors (centrosymmetric) and on one random row-stochastic, non-centrosymmetric matrix per axis, names
its plan and fp32 form from describe_plan() and the counters, and checks that the error is non-zero somewhere (the
reduced path ran).

Largest measured err / (u (J|v| + m|v|)) on an MI355X over both w and m = 0 / 1 (every case prints its values under
pytest -s; the bound's C is 8 for modes 1 and 2, 8 + sum(n) for mode 3):
                                      Rouwenhorst             random
  pair plan                         mode 1   2     3        1     2     3
    GCY 16^6                          3.87  3.70  12.2     0.83  0.83  0.83
    GCY 20^6 (persistent mid pass)    3.96  3.85  13.6     0.83  0.83  0.83
    GCY 20^6, SDFS_NO_F32_STREAM=1    3.96   -    13.6     0.83   -    0.83
    GCY (20,20,16,16,16,16)           3.64  3.80  12.0     0.83  0.83  0.83
    GCY (24,24,20,20,16,16)           3.67  3.89  11.1     0.83  0.83  0.83
    GCY (32,32,16,16,16,16)           3.86  3.80  11.7     0.83  0.83  0.83
    SSY (16,16,24,24)                 2.70  2.74  8.77     0.75  0.72  0.75
    SSY (32,32,16,16)                 3.02  2.93  8.95     0.73  0.76  0.73
    SSY (24,24,32,32)                 2.85  2.92  8.76     0.81  0.81  0.81
So the fp32 J.v is within ~4 u J|v| of the exact product in fp32 storage and ~14 u J|v| with fp32 MFMA: ~2.4e-7 and
~8e-7 of J|v| (the f32_kernels.hpp header estimated ~1e-6).  The random matrices mix signs of v more evenly, and the
final float store dominates there.  The generic fp32 passes (small-grid, padded, classic, conditional tensors) measure
3.0 .. 4.0 on Rouwenhorst and 0.70 .. 0.83 on random tensors in every mode (mode 3 runs as mode 1 there); the sharded
stages 3.98 (Rouwenhorst) and 0.023 (random).  (c) uses at most 0.49 of its bound, (d) at most 0.236 of its bound
(Rouwenhorst) and 0.032 (random).
"""
import signal

import numpy as np
import pytest

import f32_bound as fb
from test_hip_pad_plan import SHAPES as PAD_SHAPES
from test_hip_pair_plan import wbench
from test_hip_vjp import QIDX, build, model_inputs, oracle

pytestmark = pytest.mark.gpu

INPUTS = ["rouwenhorst", "random"]
PAIR = "pair plan pass"
F32_NONE = "pair plan fp32: none"


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


def report(what, value):
    print(f"\nF32-MEASURED {what}: {value:.3f}")


def f32_lines(desc):
    return [ln for ln in desc.splitlines() if " fp32: " in ln and ln.startswith(PAIR)]


def hook(op, mode, wd, v32, m):
    """One product through sdfs_debug_jvp_storage_dev; returns (out as float64, counter names that ran)."""
    import torch
    vd = torch.from_numpy(v32 if mode else v32.astype(np.float64)).cuda()
    out = torch.empty_like(vd)
    op.set_profiling(True)
    op.reset_counters()
    op.debug_jvp_storage_dev(mode, wd.data_ptr(), vd.data_ptr(), out.data_ptr(), minus_identity=m)
    op.synchronize()
    names = [c["name"] for c in op.counters() if c["launches"]]
    op.set_profiling(False)
    host = out.cpu().numpy()
    if mode == 2:
        assert np.all((host.view(np.uint32) & 0xFFFF) == 0), "bf16 storage: an output float has low bits set"
    return host.astype(np.float64), names


def jvp_forms(S, model, shapes, inputs, expect, knobs, tensors=None, modes=(1, 2, 3), fixed_point=True):
    """expect: "mfma" (the pair plan's fp32-MFMA kernels run in mode 3), "pair32" (pair plan, fp32 storage kernels, no
    MFMA) or "generic" (the generic fp32 passes).  fixed_point=False: w from wbench only, no Newton solve first."""
    import torch
    params, arr = tensors or model_inputs(S, model, shapes, inputs)
    op = build(S, model, shapes, params, arr, **knobs)
    desc = op.describe_plan()
    lines = f32_lines(desc)
    if expect == "generic":
        assert not lines and (F32_NONE in desc or PAIR not in desc), desc
    else:
        assert PAIR in desc and lines, desc
    ref = oracle(model, shapes, params, arr)
    points = [("wbench", wbench(shapes))]
    if fixed_point:
        x, _, info = op.solve(np.full(shapes, 800.0), "newton", tol=1e-8)
        assert info["status"] == 0
        points.append(("fixed point", x))
    rng = np.random.default_rng(11)
    v32 = rng.standard_normal(shapes).astype(np.float32)
    v = v32.astype(np.float64)
    worst = {}
    for wname, w in points:
        wd = torch.from_numpy(np.ascontiguousarray(w)).cuda()
        jv = ref.jvp(w, v)
        jabs = ref.jvp(w, np.abs(v))
        for mode in modes:
            for m in (0, 1):
                got, names = hook(op, mode, wd, v32, m)
                mfma = any(n.startswith("jvpm32:") for n in names)
                if mode == 3 and expect == "mfma":
                    assert mfma and not any(n.startswith("jvp32:") for n in names), names
                else:
                    assert not mfma and any(n.startswith("jvp32:") for n in names), (mode, names)
                want = jv - v if m else jv
                what = f"{model} {shapes} {inputs} {knobs} w={wname} mode {mode} m={m}"
                C = fb.constant(mode, shapes, mfma)
                err = fb.measured(got, want, jabs, v, m, fb.U[mode])          # (= C x the fraction of the bound used)
                assert err <= C, f"{what}: error {err / C:.3g} x the bound C u (J|v| + m|v|), C = {C}"
                assert err > 0, f"{what}: bit-exact fp64 result, the reduced path did not run"
                worst[mode] = max(worst.get(mode, 0.0), err)
        del wd
    for mode, e in worst.items():
        report(f"{model} {shapes} {inputs} {knobs} mode {mode}", e)
    op.close()
    return desc


# -- (a) the pair plan -------------------------------------------------------------------------------------------------
GCY_PAIR = [(16,) * 6, (20,) * 6, (20, 20, 16, 16, 16, 16), (24, 24, 20, 20, 16, 16), (32, 32, 16, 16, 16, 16)]
SSY_PAIR = [(16, 16, 24, 24), (32, 32, 16, 16), (24, 24, 32, 32)]


@limit(420)
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("model,shapes", [("gcy", s) for s in GCY_PAIR] + [("ssy", s) for s in SSY_PAIR])
def test_jvp_storage_forms_pair_plan(S, model, shapes, inputs):
    desc = jvp_forms(S, model, shapes, inputs, "mfma", dict(SDFS_PLAN="pair"))
    lines = f32_lines(desc)
    assert all("mfma32 none" not in ln for ln in lines), lines
    if shapes == (20,) * 6:
        assert "row 32 floats" in desc and "persistent middle pass" in desc, lines
    if shapes == (16,) * 6:
        assert "row 32 floats" in desc, lines


@limit(420)
@pytest.mark.parametrize("inputs", INPUTS)
def test_jvp_storage_fp32_middle_pass_one_tile_per_workgroup(S, inputs):
    """GCY 20^6 with SDFS_NO_F32_STREAM=1: the fp32-MFMA middle pass keeps one tile per workgroup."""
    desc = jvp_forms(S, "gcy", (20,) * 6, inputs, "mfma", dict(SDFS_PLAN=None, SDFS_NO_F32_STREAM=1), modes=(1, 3))
    assert "persistent middle pass" not in desc and "one tile per workgroup" in desc, f32_lines(desc)


@limit(300)
def test_jvp_storage_conditional_tensors(S):
    """Per-slice distinct transition tensors on the conditioned axes (z, z_pi).  The pair plan needs unconditional
    tensors (pair_plan_legal), so every storage mode runs the generic fp32 passes with their per-slice indexing."""
    shapes = (16,) * 6
    params, arr = model_inputs(S, "gcy", shapes, "random")
    rng = np.random.default_rng(77)
    for i in (QIDX["gcy"][0], QIDX["gcy"][1]):
        q = rng.random(arr[i].shape) + 0.05
        arr[i] = q / q.sum(axis=-1, keepdims=True)
    desc = jvp_forms(S, "gcy", shapes, "conditional", "generic", dict(SDFS_PLAN=None), tensors=(params, arr), modes=(1, 3))
    assert PAIR not in desc and "stage 0 pass" in desc, desc


# -- (a) the generic fp32 passes ---------------------------------------------------------------------------------------
SMALL = "small-grid plan pass"
PADDED = "padded pair plan pass"
GENERIC = [("ssy", (15,) * 4, dict(SDFS_PLAN=None), SMALL), ("ssy", (16,) * 4, dict(SDFS_PLAN=None), SMALL),
           ("ssy", (7, 13, 11, 9), dict(SDFS_PLAN=None), SMALL), ("gcy", (3, 3, 12, 12, 13, 13), dict(SDFS_PLAN=None), SMALL),
           ("gcy", (15,) * 6, dict(SDFS_PLAN=None), PADDED), ("gcy", (18,) * 6, dict(SDFS_PLAN=None), PADDED),
           ("ssy", (25, 18, 32, 7), dict(SDFS_PAD_PLAN=2), PADDED), ("gcy", (16,) * 6, dict(SDFS_PLAN="classic"), None)]
GENERIC_IDS = ["small-ssy15", "small-ssy16", "small-ssy7-13-11-9", "small-gcy3-3-12-12-13-13", "pad-gcy15", "pad-gcy18",
               "pad-ssy25-18-32-7", "classic-gcy16"]


@limit(420)
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("model,shapes,knobs,marker", GENERIC, ids=GENERIC_IDS)
def test_jvp_storage_forms_generic_passes(S, model, shapes, knobs, marker, inputs):
    """The small-grid and padded plans and the classic tiles have no fp32 kernels of their own: every storage mode runs
    the generic passes at prec = 1 (mode 3 as mode 1, C = 8)."""
    if marker == PADDED:
        assert shapes in PAD_SHAPES
    desc = jvp_forms(S, model, shapes, inputs, "generic", knobs)
    if marker is None:
        assert SMALL not in desc and PAIR not in desc, desc
    else:
        assert marker in desc, desc


# -- (b) handle state after the hook -----------------------------------------------------------------------------------
@limit(300)
@pytest.mark.parametrize("model,shapes", [("gcy", (16,) * 6), ("ssy", (15,) * 4)], ids=["gcy16-pair", "ssy15-small"])
def test_state_after_the_hook(S, model, shapes):
    """After a reduced-precision product the cached linearisation is refused by the fp64 device forms until it is
    rebuilt; then fp64 J.v meets the 1e-11 bound again, and a fp64 Newton solve gives the bits of a fresh handle."""
    import torch
    from sdfs_via_autodiff_amd._lib import SdfsError
    params, arr = model_inputs(S, model, shapes, "random")
    op = build(S, model, shapes, params, arr, SDFS_PLAN=None)
    ref = oracle(model, shapes, params, arr)
    w = wbench(shapes)
    rng = np.random.default_rng(3)
    v32 = rng.standard_normal(shapes).astype(np.float32)
    v = v32.astype(np.float64)
    wd, vd = torch.from_numpy(w).cuda(), torch.from_numpy(v).cuda()
    out = torch.empty_like(wd)
    op.linearize_dev(wd.data_ptr())
    for mode in (3, 2, 1):
        hook(op, mode, wd, v32, 0)
        with pytest.raises(SdfsError):
            op.jvp_dev(vd.data_ptr(), out.data_ptr())
        with pytest.raises(SdfsError):
            op.vjp_dev(vd.data_ptr(), out.data_ptr())
        op.linearize_dev(wd.data_ptr())
        op.jvp_dev(vd.data_ptr(), out.data_ptr())
        op.synchronize()
        want = ref.jvp(w, v)
        err = float(np.max(np.abs(out.cpu().numpy() - want)))
        assert err <= 1e-11 * float(np.max(np.abs(want))), (mode, err)
    # the mode 0 hook is the fp64 product and leaves a valid linearisation behind
    got, names = hook(op, 0, wd, v32, 0)
    assert not any("32" in n for n in names), names
    assert np.max(np.abs(got - ref.jvp(w, v))) <= 1e-11 * np.max(np.abs(got))
    op.jvp_dev(vd.data_ptr(), out.data_ptr())
    op.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), got)
    hook(op, 3, wd, v32, 1)
    x1, n1, i1 = op.solve(np.full(shapes, 800.0), "newton", tol=1e-9)
    op.close()
    fresh = build(S, model, shapes, params, arr, SDFS_PLAN=None)
    x2, n2, i2 = fresh.solve(np.full(shapes, 800.0), "newton", tol=1e-9)
    fresh.close()
    assert i1["status"] == i2["status"] == 0 and n1 == n2
    np.testing.assert_array_equal(x1, x2)


def test_hook_refusals(S):
    from sdfs_via_autodiff_amd._lib import SdfsError
    import torch
    shapes = (15,) * 4
    params, arr = model_inputs(S, "ssy", shapes, "rouwenhorst")
    op = build(S, "ssy", shapes, params, arr)
    wd = torch.full(shapes, 800.0, dtype=torch.float64, device="cuda")
    v = torch.zeros(shapes, dtype=torch.float32, device="cuda")
    for bad in (-1, 4):
        with pytest.raises(SdfsError):
            op.debug_jvp_storage_dev(bad, wd.data_ptr(), v.data_ptr(), v.data_ptr())
    op.close()


# -- (c) one Newton step with the fused fp32 BiCGSTAB forms -----------------------------------------------------------
NEWTON = [("gcy", (16,) * 6, dict(SDFS_PLAN=None), "mfma"), ("gcy", (20,) * 6, dict(SDFS_PLAN=None), "mfma"),
          ("ssy", (15,) * 4, dict(SDFS_PLAN=None), "generic"), ("gcy", (15,) * 6, dict(SDFS_PLAN=None), "generic")]


@limit(600)
@pytest.mark.parametrize("beta", [None, 0.99])
@pytest.mark.parametrize("model,shapes,knobs,expect", NEWTON, ids=["gcy16", "gcy20", "small-ssy15", "pad-gcy15"])
def test_one_newton_step_true_residual(S, model, shapes, knobs, expect, beta):
    """x1 = one Newton step from x0 = w* (1 + 1e-2 smooth noise), inner_rtol rho, inner_atol 0.  delta = x1 - x0 solves
    (I - J(x0)) delta = b = T(x0) - x0 to rho in exact arithmetic; with reduced J.v storage the true residual
    r = b - delta + J(x0) delta, computed by the oracle, satisfies
        |r|_2 <= 2 rho |b|_2 + C u |J|delta||_2 + 2 u (|b|_2 + |delta|_2)        (C, u of the J.v bound; mode 0: C = 0).
    A smaller beta makes 1 - rho(J) larger: the system is better conditioned and the bound tighter."""
    m = S.SSY() if model == "ssy" else S.GCY()
    if beta is not None:
        m = type(m)(β=beta)
    arr = (S.discretize_ssy if model == "ssy" else S.discretize_gcy)(m, shapes)
    op = build(S, model, shapes, m.params, arr, **knobs)
    ref = oracle(model, shapes, m.params, arr)
    ws, _, info = op.solve(np.full(shapes, 800.0), "newton", tol=1e-9)
    assert info["status"] == 0
    grids = np.meshgrid(*[np.linspace(0, np.pi, n) for n in shapes], indexing="ij")
    x0 = ws * (1 + 1e-2 * np.sin(sum((k + 1) * g for k, g in enumerate(grids))))
    b = ref(x0) - x0
    nb = np.linalg.norm(b)
    for mode in (0, 1, 3):
        for rho in (1e-4, 1e-5):
            op.set_profiling(True)
            op.reset_counters()
            x1, n, info = op.solve(x0, "newton", tol=0.0, max_iter=1, inner_rtol=rho, inner_atol=0.0, krylov_f32=mode)
            names = [c["name"] for c in op.counters() if c["launches"]]
            op.set_profiling(False)
            assert n == 1, (mode, rho, info)
            if mode:
                assert any(nm.startswith("jvp32") or nm.startswith("jvpm32") for nm in names), names
                assert not any(nm.startswith("jvp:") or nm.startswith("jvp+") for nm in names), names   # no fp64 redo
            if mode == 3 and expect == "mfma":
                assert any(nm.startswith("jvpm32+p:") for nm in names) and any(nm.startswith("jvpm32+s:") for nm in names), names
            d = x1 - x0
            r = b - d + ref.jvp(x0, d)
            u = fb.U[mode] if mode else 2.0 ** -53
            C = fb.constant(mode, shapes, mode == 3 and expect == "mfma") if mode else 0
            lim = 2 * rho * nb + C * u * np.linalg.norm(ref.jvp(x0, np.abs(d))) + 2 * u * (nb + np.linalg.norm(d))
            nr = np.linalg.norm(r)
            report(f"newton {model} {shapes} beta={beta} mode {mode} rho={rho} |r| / bound", nr / lim)
            assert nr <= lim, f"{model} {shapes} beta={beta} mode {mode} rho {rho}: |r| {nr:.3e} > {lim:.3e}"
    op.close()


# -- (d) one application of T with fp32 intermediates --------------------------------------------------------------------
T32_SHAPES = [("gcy", (20,) * 6), ("gcy", (16,) * 6), ("gcy", (24, 24, 20, 20, 16, 16)),
              ("ssy", (16, 16, 24, 24)), ("ssy", (32, 32, 16, 16)), ("ssy", (20, 20, 20, 20))]
# (knobs, gathered): as built; the fp32 middle pass unstreamed; T's last pass gathering a3 (z states perturbed, see
# gathered_a3_inputs)
T32_CASES = [(dict(), False), (dict(SDFS_NO_F32_STREAM=1), False), (dict(), True)]


def gathered_a3_inputs(arr):
    """GCY arrays whose z states are no longer sigma_z[h_z] g[z] + m[h_zpi, z_pi]: a term in h_z times h_zpi makes the
    aggregator's scale a3 = exp((1 - gamma)(mu_c + z)) fail the two-table check of the pair plan's last pass, which then
    gathers a3 from its table."""
    z = np.asarray(arr[0])                        # z_states[z_pi, h_z, h_zpi, z]
    hz = np.arange(z.shape[1])[None, :, None, None]
    hzpi = np.arange(z.shape[2])[None, None, :, None]
    out = list(arr)
    out[0] = z + 1e-3 * float(np.std(z)) * hz * hzpi
    return out


@limit(420)
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("model,shapes", T32_SHAPES)
def test_t_f32_one_application(S, model, shapes, inputs):
    """solve(w, "successive_approx", tol=0, max_iter=1, t_f32=1) = T32(w): |T32 - T|_i <= 8 u (T_i - 1) / |theta|, and the
    fused residual max|T32(w) - w| within the largest of those of the oracle's max|T(w) - w|; as built, with the
    fp32 middle pass unstreamed (SDFS_NO_F32_STREAM=1) and, on GCY, with a3 gathered by the last pass (z states that
    break its two-table form, given to the handle and the oracle alike; SSY's a3 does not vary along the last pass's
    pair, so its two tables always hold)."""
    t32_one_application(S, model, shapes, inputs)


def t32_one_application(S, model, shapes, inputs, tensors=None, theta=None):
    """The body of test_t_f32_one_application; tensors = (params, arrays) and theta of another model than the default."""
    params, arr0 = tensors or model_inputs(S, model, shapes, inputs)
    if theta is None:
        theta = (S.SSY() if model == "ssy" else S.GCY()).θ
    w = wbench(shapes)
    want = {}
    worst = 0.0
    for knobs, gathered in T32_CASES:
        if gathered and model != "gcy":
            continue
        arr = gathered_a3_inputs(arr0) if gathered else arr0
        if gathered not in want:
            want[gathered] = oracle(model, shapes, params, arr)(w)
        T = want[gathered]
        lim = fb.t32_bound(T, theta)
        want_res = float(np.max(np.abs(T - w)))
        op = build(S, model, shapes, params, arr, SDFS_PLAN="pair", **knobs)
        assert PAIR in op.describe_plan()
        op.set_profiling(True)
        op.reset_counters()
        x, n, info = op.solve(w, "successive_approx", tol=0.0, max_iter=1, t_f32=1)
        names = [c["name"] for c in op.counters() if c["launches"]]
        op.close()
        assert n == 1 and any(nm.startswith("T32:") for nm in names), names
        err = np.abs(x - T)
        what = f"{model} {shapes} {inputs} {knobs}{' a3 gathered' if gathered else ''}"
        assert np.all(err <= lim), f"{what}: {float(np.max(err / lim)):.3g} x the bound"
        assert np.max(err) > 0, what
        assert abs(info["final_err"] - want_res) <= float(np.max(lim)), (what, info["final_err"], want_res)
        report(f"t_f32 {what} max err / bound", float(np.max(err / lim)))
        worst = max(worst, float(np.max(err / lim)))
    return worst


@limit(120)
@pytest.mark.parametrize("model,shapes", [("ssy", (15,) * 4), ("gcy", (6,) * 6)])
def test_t_f32_is_fp64_on_the_small_grid_plan(S, model, shapes):
    params, arr = model_inputs(S, model, shapes, "random")
    op = build(S, model, shapes, params, arr, SDFS_PLAN=None)
    assert "small-grid plan pass" in op.describe_plan()
    w = wbench(shapes)
    xa, _, ia = op.solve(w, "successive_approx", tol=0.0, max_iter=1, t_f32=1)
    xb, _, ib = op.solve(w, "successive_approx", tol=0.0, max_iter=1)
    op.close()
    np.testing.assert_array_equal(xa, xb)
    assert ia["final_err"] == ib["final_err"]


# -- (e) the sharded handle's stages in fp32, in process -----------------------------------------------------------------
@limit(600)
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("shapes,world", [((16,) * 6, 2), ((20,) * 6, 8)], ids=["gcy16-2way", "gcy20-8way"])
def test_sharded_stages_in_fp32(S, shapes, world, inputs):
    """Every rank's stage 0 on its z-block, the exchange as host slicing, every rank's stage 1 on its h_c-block (as
    tests/test_hip_fullsize.py drives them), with w_ref = sqrt(max w min w) as the distributed Newton / SA loops take it:
    sdfs_set_krylov_f32 -> MODE_T_LIN, then MODE_JVP on float32 blocks, held to the mode-1 bound; sdfs_set_t_f32 ->
    MODE_T (stage 0 writes floats, stage 1 reads them), held to the bound of (d), its residual too."""
    import torch
    from sdfs_via_autodiff_amd import distributed as D
    params, arr = model_inputs(S, "gcy", shapes, inputs)
    ref = oracle("gcy", shapes, params, arr)
    A, B = D.SHARD_AXES["gcy"]
    a_sz, b_sz = D.block_sizes(shapes[A], world), D.block_sizes(shapes[B], world)
    a_off, b_off = D.block_offsets(a_sz), D.block_offsets(b_sz)
    w = wbench(shapes)
    w_ref = float(np.sqrt(w.max() * w.min()))
    v32 = np.random.default_rng(12).standard_normal(shapes).astype(np.float32)
    v = v32.astype(np.float64)
    dev = torch.device("cuda", 0)

    def sl(axis, lo, n):
        s = [slice(None)] * 6
        s[axis] = slice(lo, lo + n)
        return tuple(s)

    def two_stage(bes, mode, x_full, old_full=None):
        dt0 = bes[0].dtypes(0, mode)
        mid = np.empty(shapes, dtype=np.float32 if dt0[1] == torch.float32 else np.float64)
        for r in range(world):
            xin = torch.from_numpy(np.ascontiguousarray(x_full[sl(A, a_off[r], a_sz[r])])).to(dev)
            mid[sl(A, a_off[r], a_sz[r])] = bes[r].run(0, mode, xin).cpu().numpy()
        out, res_max = None, 0.0
        for r in range(world):
            zin = torch.from_numpy(np.ascontiguousarray(mid[sl(B, b_off[r], b_sz[r])])).to(dev)
            old = res = None
            if old_full is not None:
                old = torch.from_numpy(np.ascontiguousarray(old_full[sl(B, b_off[r], b_sz[r])])).to(dev)
                res = torch.zeros(1, dtype=torch.float64, device=dev)
            y = bes[r].run(1, mode, zin, old=old, resid=res).cpu().numpy()
            if out is None:
                out = np.empty(shapes, dtype=y.dtype)
            out[sl(B, b_off[r], b_sz[r])] = y
            if res is not None:
                res_max = max(res_max, float(res.item()))
        return out.astype(np.float64), res_max

    bes = [D.HipStages("gcy", shapes, params, arr, A, a_off[r], a_sz[r], B, b_off[r], b_sz[r], 0) for r in range(world)]
    try:
        for be in bes:
            be.set_krylov_f32(True, w_ref)
        two_stage(bes, D.MODE_T_LIN, w)
        got, _ = two_stage(bes, D.MODE_JVP, v32)
        jabs = ref.jvp(w, np.abs(v))
        err = fb.measured(got, ref.jvp(w, v), jabs, v, 0, fb.U[1])
        assert 0 < err <= fb.constant(1, shapes, False), f"sharded fp32 J.v: {err:.3g} x u (J|v|)"
        report(f"sharded {shapes} x{world} {inputs} fp32 J.v", err)
        for be in bes:
            be.set_krylov_f32(False)
            assert be.set_t_f32(True, w_ref)
        got, res = two_stage(bes, D.MODE_T, w, old_full=w)
        T = ref(w)
        lim = fb.t32_bound(T, S.GCY().θ)
        e = np.abs(got - T)
        assert np.all(e <= lim) and np.max(e) > 0, float(np.max(e / lim))
        assert abs(res - float(np.max(np.abs(T - w)))) <= float(np.max(lim))
        report(f"sharded {shapes} x{world} {inputs} t_f32 max err / bound", float(np.max(e / lim)))
    finally:
        for be in bes:
            be.close()

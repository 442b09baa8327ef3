"""
Times of the parameter sensitivities (sdfs_via_autodiff_amd/sensitivity.py) at GCY 16^6 and 20^6 (-> profiles/).

Per grid: a Newton solve to the fixed point (the library's default options, for scale); one forward sensitivity
(tangent + BiCGSTAB at rtol 1e-10) for beta (elementwise tangent) and gamma (tangent with a J.v) with its J.v count;
the 12-parameter adjoint gradient (one transposed solve + 12 tangents); the two tangent kernels (HIP-event counters)
as a fraction of the streaming-copy rate measured in the same process.

``--persistence`` measures the persistence parameters instead (-> profiles/sensitivity_persistence_times.txt): per grid
k_sens_generator's time and its fraction of the copy rate, one forward d w*/d rho with its J.v count, the 18-parameter
gradient next to the 12-parameter one and, at 16^6, the device tangent along rho against a Richardson central
difference of the C oracle's T.

    python tools/sensitivity_times.py [--persistence] [16 20]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdfs_via_autodiff_amd as S                       # noqa: E402
from sdfs_via_autodiff_amd import sensitivity as sens  # noqa: E402
from sdfs_via_autodiff_amd import _requests  # noqa: E402


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def main(extents):
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)}; times are means over repeated calls after one warm-up call")
    for n in extents:
        shapes = (n,) * 6
        m = S.GCY()
        op, arr = _requests._operator(m, shapes)
        N = op.size
        w = torch.full(shapes, 800.0, dtype=torch.float64, device=dev)
        wn = w.clone()
        t_newton, (it, info) = timed(lambda: (wn.copy_(w), op.solve_dev(wn.data_ptr(), "newton"))[1], 3)
        op.solve_dev(w.data_ptr(), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
        # streaming copy: what a pass that reads and writes every point once can reach
        a, b = torch.empty_like(w), torch.empty_like(w)
        op.stream_copy_dev(w.data_ptr(), a.data_ptr(), N)
        t_copy, _ = timed(lambda: op.stream_copy_dev(w.data_ptr(), a.data_ptr(), N), 20)
        copy_gbs = 16.0 * N / t_copy / 1e9
        print(f"GCY {n}^6  N = {N}")
        print(f"  Newton solve (defaults: tol 1e-7, inner rtol 1e-5, atol 1e-4): {1e3 * t_newton:8.2f} ms, "
              f"{info['n_apply']} applications of T / J.v")
        print(f"  streaming copy: {1e3 * t_copy:.3f} ms = {copy_gbs:.0f} GB/s")
        dirs = {nm: d[:2] for nm, d in zip(sens.GCY_SUPPORTED, sens._directions(m, shapes, sens.GCY_SUPPORTED, arr))}
        rhs, x, tw = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)
        for name in ("β", "γ"):
            dp, da = dirs[name]
            need_jv = name == "γ"

            def one():
                op.param_tangent_dev(w.data_ptr(), dp, da, rhs.data_ptr(), tw.data_ptr())
                return op.solve_linear_dev(rhs.data_ptr(), x.data_ptr(), False, 1e-10, 0.0)
            one()
            t, (its, rel) = timed(one, 3)
            t_tan, _ = timed(lambda: op.param_tangent_dev(w.data_ptr(), dp, da, rhs.data_ptr(), tw.data_ptr()), 5)
            print(f"  forward sensitivity d w*/d {name} (rtol 1e-10): {1e3 * t:8.2f} ms  (tangent {1e3 * t_tan:.2f} ms), "
                  f"BiCGSTAB {its} iterations = {2 * its + need_jv} J.v, final rel. residual {rel:.1e}")
        g = torch.rand(shapes, dtype=torch.float64, device=dev)
        S.wc_ratio_gradient(m, shapes, w, g)
        t_adj, _ = timed(lambda: S.wc_ratio_gradient(m, shapes, w, g), 2)
        print(f"  adjoint gradient, all 12 parameters (rtol 1e-10): {1e3 * t_adj:8.2f} ms")
        # the tangent kernels alone
        op.set_profiling(True)
        op.reset_counters()
        for _ in range(10):
            for name in ("β", "γ"):
                dp, da = dirs[name]
                op.param_tangent_dev(w.data_ptr(), dp, da, rhs.data_ptr(), tw.data_ptr())
        for k in op.counters():
            if k["name"].startswith("sens:"):
                t = k["total_ms"] / k["launches"]
                gbs = k["alg_bytes"] / (t * 1e-3) / 1e9
                print(f"  {k['name']:<22s} {1e3 * t:8.1f} us  {gbs:6.0f} GB/s = {gbs / copy_gbs:.2f} of the copy rate")
        op.set_profiling(False)
        del a, b, rhs, x, tw, w, wn, g
        _requests._ops.clear()
        torch.cuda.empty_cache()


def richardson_tangent_c_oracle(shapes, name, w):
    """dT(w)/dp by Richardson-extrapolated central differences (step 1e-4 |p|) of the C oracle's T."""
    from oracle.c_oracle import COperator
    p0 = dict(zip(sens.GCY_PARAMS, S.GCY().params))

    def T_at(value):
        m = S.GCY(**{**p0, name: value})
        return COperator("gcy", shapes, m.params, S.discretize_gcy(m, shapes))(w)

    def cd(step):
        return (T_at(p0[name] + step) - T_at(p0[name] - step)) / (2.0 * step)
    h = 1e-4 * abs(p0[name])
    return (4.0 * cd(h / 2) - cd(h)) / 3.0


def main_persistence(extents):
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)}; times are means over repeated calls after one warm-up call")
    for n in extents:
        shapes = (n,) * 6
        m = S.GCY()
        op, arr = _requests._operator(m, shapes)
        N = op.size
        w = torch.full(shapes, 800.0, dtype=torch.float64, device=dev)
        op.solve_dev(w.data_ptr(), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
        a = torch.empty_like(w)
        op.stream_copy_dev(w.data_ptr(), a.data_ptr(), N)
        t_copy, _ = timed(lambda: op.stream_copy_dev(w.data_ptr(), a.data_ptr(), N), 20)
        copy_gbs = 16.0 * N / t_copy / 1e9
        print(f"GCY {n}^6  N = {N}")
        print(f"  streaming copy: {1e3 * t_copy:.3f} ms = {copy_gbs:.0f} GB/s")
        dirs = dict(zip(sens.GCY_PERSISTENCE, sens._directions(m, shapes, sens.GCY_PERSISTENCE, arr, True)))
        rhs, x, tw = torch.empty_like(w), torch.empty_like(w), torch.empty_like(w)
        dp, da, dg = dirs["ρ"]

        def one():
            op.param_tangent_dev(w.data_ptr(), dp, da, rhs.data_ptr(), tw.data_ptr(), dgen=dg)
            return op.solve_linear_dev(rhs.data_ptr(), x.data_ptr(), False, 1e-10, 0.0)
        one()
        t, (its, rel) = timed(one, 3)
        t_tan, _ = timed(lambda: op.param_tangent_dev(w.data_ptr(), dp, da, rhs.data_ptr(), tw.data_ptr(), dgen=dg), 5)
        print(f"  forward sensitivity d w*/d ρ (rtol 1e-10): {1e3 * t:8.2f} ms  (tangent {1e3 * t_tan:.2f} ms), "
              f"BiCGSTAB {its} iterations = {2 * its} J.v, final rel. residual {rel:.1e}")
        g = torch.rand(shapes, dtype=torch.float64, device=dev)
        S.wc_ratio_gradient(m, shapes, w, g)
        t12, _ = timed(lambda: S.wc_ratio_gradient(m, shapes, w, g), 2)
        S.wc_ratio_gradient(m, shapes, w, g, persistence=True)
        t18, _ = timed(lambda: S.wc_ratio_gradient(m, shapes, w, g, persistence=True), 2)
        print(f"  adjoint gradient (rtol 1e-10): 12 parameters {1e3 * t12:8.2f} ms, all 18 parameters {1e3 * t18:8.2f} ms")
        # the generator pass alone, by the axis it runs along (axis 5 is the fastest)
        for name in sens.GCY_PERSISTENCE:
            dp_, da_, dg_ = dirs[name]
            axis = [i for i, gen in enumerate(dg_) if gen is not None][0]
            op.set_profiling(True)
            op.reset_counters()
            for _ in range(10):
                op.param_tangent_dev(w.data_ptr(), dp_, da_, rhs.data_ptr(), tw.data_ptr(), dgen=dg_)
            for k in op.counters():
                if k["name"] == "sens:generator":
                    tk = k["total_ms"] / k["launches"]
                    gbs = k["alg_bytes"] / (tk * 1e-3) / 1e9
                    print(f"  sens:generator, {name:<5s} (axis {axis}) {1e3 * tk:8.1f} us  {gbs:6.0f} GB/s = "
                          f"{gbs / copy_gbs:.2f} of the copy rate")
            op.set_profiling(False)
        if n == 16:
            wh = 500.0 + 200.0 * np.random.default_rng(96).random(shapes)
            got = op.param_tangent(wh, dp, da, dgen=dg)
            want = richardson_tangent_c_oracle(shapes, "ρ", wh)
            print(f"  device dT/dρ at a non-constant w vs Richardson central difference of the C oracle's T: "
                  f"{np.max(np.abs(got - want)) / np.max(np.abs(want)):.3e} of max|dT/dρ| = {np.max(np.abs(want)):.3e}")
        del a, rhs, x, tw, w, g
        _requests._ops.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--persistence"]
    run = main_persistence if "--persistence" in sys.argv[1:] else main
    run([int(a) for a in args] or [16, 20])

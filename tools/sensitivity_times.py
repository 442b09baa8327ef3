"""
Times of the parameter sensitivities (sdfs_via_autodiff_amd/sensitivity.py) at GCY 16^6 and 20^6 (-> profiles/).

Per grid: a Newton solve to the fixed point (the library's default options, for scale); one forward sensitivity
(tangent + BiCGSTAB at rtol 1e-10) for beta (elementwise tangent) and gamma (tangent with a J.v) with its J.v count;
the 12-parameter adjoint gradient (one transposed solve + 12 tangents); the two tangent kernels (HIP-event counters)
as a fraction of the streaming-copy rate measured in the same process.

    python tools/sensitivity_times.py [16 20]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdfs_via_autodiff_amd as S                       # noqa: E402
from sdfs_via_autodiff_amd import sensitivity as sens  # noqa: E402


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
        op, arr = sens._operator(m, shapes)
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
        dirs = dict(zip(sens.GCY_SUPPORTED, sens._directions(m, shapes, sens.GCY_SUPPORTED, arr)))
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
        sens._ops.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [16, 20])

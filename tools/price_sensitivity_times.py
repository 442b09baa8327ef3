"""
Times of the price sensitivities (sdfs_tilt_tangent_dev, ``price_sensitivities``) at GCY 16^6 and 20^6
(-> profiles/price_sensitivity_times.txt).

Per grid, at the fixed point of a tight Newton solve: the three tangent kernels (HIP-event counters), with the logarithms
(γ: dθ ≠ 0) and without (s_c), and the generator pass along the slowest and the fastest axis, as fractions of the
streaming-copy rate measured in the same process; one whole tangent (K f given) against one tilted product; one parameter
of ``price_sensitivities(kappa=2)`` against one parameter of ``wc_ratio_sensitivities`` on the same handle.

    python tools/price_sensitivity_times.py [16 20]
"""
import os
import sys
import time

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
        op.solve_dev(w.data_ptr(), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
        a = torch.empty_like(w)
        op.stream_copy_dev(w.data_ptr(), a.data_ptr(), N)
        t_copy, _ = timed(lambda: op.stream_copy_dev(w.data_ptr(), a.data_ptr(), N), 20)
        copy_gbs = 16.0 * N / t_copy / 1e9
        print(f"GCY {n}^6  N = {N}")
        print(f"  streaming copy: {1e3 * t_copy:.3f} ms = {copy_gbs:.0f} GB/s")
        names = ("γ", "s_c", "ρ", "ρ_λ")                   # logarithms, none, generator on axis 0, on axis 5
        dirs = dict(zip(names, sens._directions(m, shapes, names, arr, True)))
        dw, f, kf, out = torch.randn_like(w), torch.rand_like(w) + 0.5, torch.empty_like(w), torch.empty_like(w)
        th, g = m.θ, m.γ
        for p, kl, kc in [(1, th, 2.0 - g), (2, 2 * th, -2 * g), (0, 0.0, 2.0)]:
            op.set_tilt_dev(w.data_ptr(), p, kl, kc)
            op.apply_tilted_dev(f.data_ptr(), kf.data_ptr())
            t_prod, _ = timed(lambda: op.apply_tilted_dev(f.data_ptr(), kf.data_ptr()), 5)
            print(f"  tilt K({p}, {kl:.3g}, {kc:.3g}): one tilted product {1e3 * t_prod:.2f} ms")
            for name in names:
                dp, da, dg = dirs[name]

                def one():
                    op.tilt_tangent_dev(w.data_ptr(), dw.data_ptr(), dw.data_ptr(), dp, da, dg, 0.5, -0.5, f.data_ptr(), None,
                                        kf.data_ptr(), out.data_ptr())
                one()
                t, _ = timed(one, 5)
                print(f"    tangent along {name:<4s} (K f given): {1e3 * t:7.2f} ms = {t / t_prod:.2f} tilted products")
                op.set_profiling(True)
                op.reset_counters()
                for _ in range(5):
                    one()
                for k in op.counters():
                    if k["name"].startswith("price:dtilt") and k["launches"]:
                        tk = k["total_ms"] / k["launches"]
                        gbs = k["alg_bytes"] / (tk * 1e-3) / 1e9
                        print(f"      {k['name']:<22s} {1e3 * tk:8.1f} us  {gbs:6.0f} GB/s = {gbs / copy_gbs:.2f} of the copy rate")
                op.set_profiling(False)
        del dw, f, kf, out, a
        for name in ("γ",):
            S.wc_ratio_sensitivities(m, shapes, w, wrt=name)
            t_w, _ = timed(lambda: S.wc_ratio_sensitivities(m, shapes, w, wrt=name), 2)
            S.price_sensitivities(m, shapes, w, kappa=2.0, wrt=name)
            t_p, r = timed(lambda: S.price_sensitivities(m, shapes, w, kappa=2.0, wrt=name), 2)
            t_m, _ = timed(lambda: S.price_sensitivities(m, shapes, w, wrt=name), 2)
            t_2, _ = timed(lambda: S.price_sensitivities(m, shapes, w, kappa=2.0, wrt=(name, "ψ")), 2)
            print(f"  one parameter ({name}, rtol 1e-10): wc_ratio_sensitivities {1e3 * t_w:8.2f} ms; price_sensitivities(kappa=2) "
                  f"{1e3 * t_p:8.2f} ms (BiCGSTAB iterations dw*, dv: {r['_info'][name]}); SDF moments only {1e3 * t_m:8.2f} ms")
            print(f"  a second parameter (ψ) adds {1e3 * (t_2 - t_p):8.2f} ms (the prices themselves are computed once)")
        del w
        _requests._ops.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [16, 20])

"""
Times of asset pricing with the SDF at w* (sdfs_via_autodiff_amd/pricing.py) at GCY 16^6 and 20^6 (-> profiles/).

Per grid, at a tight Newton fixed point: set_tilt (fp64 linearisation + the scaling pass), one tilted product, 120
horizons of the real term structure, one perpetual-claim solve (kappa = 1, rtol 1e-10) with its BiCGSTAB count, and
the two new kernels (HIP-event counters) as fractions of the streaming-copy rate measured in the same process.

    python tools/pricing_times.py [16 20]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdfs_via_autodiff_amd as S                       # noqa: E402
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
        op, _ = _requests._operator(m, shapes)
        N = op.size
        w = torch.full(shapes, 800.0, dtype=torch.float64, device=dev)
        op.solve_dev(w.data_ptr(), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
        a = torch.empty_like(w)
        op.stream_copy_dev(w.data_ptr(), a.data_ptr(), N)
        t_copy, _ = timed(lambda: op.stream_copy_dev(w.data_ptr(), a.data_ptr(), N), 20)
        copy_gbs = 16.0 * N / t_copy / 1e9
        print(f"GCY {n}^6  N = {N}")
        print(f"  streaming copy: {1e3 * t_copy:.3f} ms = {copy_gbs:.0f} GB/s")
        one, out, x = torch.ones_like(w), torch.empty_like(w), torch.empty_like(w)
        jv = torch.empty_like(w)
        for p, kl, kc, what in ((1, m.θ, -m.γ, "E[M]"), (2, 2 * m.θ, -2 * m.γ, "E[M^2]"), (0, 0.0, 1.0, "E[G_c]")):
            wp = w.data_ptr() if p else None
            op.set_tilt_dev(wp, p, kl, kc)
            t_set, _ = timed(lambda: op.set_tilt_dev(wp, p, kl, kc), 10)
            print(f"  set_tilt (p = {p}, {what}){' (no linearisation)' if wp is None else ''}: {1e3 * t_set:8.3f} ms")
        op.set_tilt_dev(w.data_ptr(), 1, m.θ, -m.γ)
        op.apply_tilted_dev(one.data_ptr(), out.data_ptr())
        t_apply, _ = timed(lambda: op.apply_tilted_dev(one.data_ptr(), out.data_ptr()), 20)
        op.linearize_dev(w.data_ptr())
        op.jvp_dev(one.data_ptr(), jv.data_ptr())
        t_jv, _ = timed(lambda: op.jvp_dev(one.data_ptr(), jv.data_ptr()), 20)
        print(f"  one tilted product: {1e3 * t_apply:8.3f} ms   (one fp64 J.v: {1e3 * t_jv:.3f} ms)")
        S.term_structure(m, shapes, w, 120, kappa=0.0)
        t_hz, _ = timed(lambda: S.term_structure(m, shapes, w, 120, kappa=0.0), 3)
        print(f"  term structure, 120 horizons (real bonds, stationary weights): {1e3 * t_hz:8.2f} ms "
              f"(set_tilt included)")
        op.set_tilt_dev(w.data_ptr(), 1, m.θ, 1.0 - m.γ)
        op.apply_tilted_dev(one.data_ptr(), out.data_ptr())

        def solve():
            return op.solve_tilted_dev(out.data_ptr(), x.data_ptr(), 1e-10)
        solve()
        t_solve, (its, rel) = timed(solve, 3)
        print(f"  perpetual consumption claim, (I - K) v = K 1 (rtol 1e-10): {1e3 * t_solve:8.2f} ms, BiCGSTAB {its} "
              f"iterations = {2 * its} products, final rel. residual {rel:.1e}")
        S.claim_prices(m, shapes, w, 1.0)
        t_claim, _ = timed(lambda: S.claim_prices(m, shapes, w, 1.0), 2)
        print(f"  claim_prices (kappa = 1: three set_tilt, three products, the solve, host copies): {1e3 * t_claim:8.2f} ms")
        # the new kernels alone
        op.set_profiling(True)
        op.reset_counters()
        for _ in range(10):
            op.set_tilt_dev(w.data_ptr(), 1, m.θ, -m.γ)
            op.set_tilt_dev(w.data_ptr(), 2, 2 * m.θ, -2 * m.γ)
            op.set_tilt_dev(None, 0, 0.0, 1.0)
        op.set_tilt_dev(w.data_ptr(), 1, m.θ, -m.γ)
        op.tilted_horizons_dev(20, None)
        for k in op.counters():
            if k["name"].startswith("price:"):
                t = k["total_ms"] / k["launches"]
                gbs = k["alg_bytes"] / (t * 1e-3) / 1e9
                print(f"  {k['name']:<22s} {1e3 * t:8.1f} us  {gbs:6.0f} GB/s = {gbs / copy_gbs:.2f} of the copy rate")
        op.set_profiling(False)
        del a, one, out, x, jv, w
        _requests._ops.clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [16, 20])

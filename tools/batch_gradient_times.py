"""
Throughput of the batch gradient (csrc/batch_adjoint.hpp) against the batched Newton-Krylov solve on the same handle and
against ``wc_ratio_gradient`` looped over members (-> profiles/batch_gradient_times.txt).

Per shape, B = 256, one process, the three routes alternating, a warm-up of each first, three repetitions (medians):
  (a) gradient  BatchOperator.adjoint_dev at the batch's w* (rtol 1e-10) -- w*, g and the outputs device-resident; the
                host half (adjoint_moments_to_gradient per member) is timed separately;
  (b) newton    BatchOperator.solve_dev(algorithm="newton", tol 1e-7, inner rtol 1e-5, atol 0) from 800, same handle;
  (c) loop      wc_ratio_gradient(..., rtol 1e-10, persistence=True) member after member (12 members; the operators
                are built and cached by a warm-up call outside the timed region).
Per row: seconds, gradients (problems) per second, microseconds per application per problem (B <= CUs: wall / most
applications of a member, i.e. what one workgroup takes), iterations per member, and the ratios (a)/(c) of gradients per
second and (a)/(b) of microseconds per application.
Members are the fixed family of tests/batch_family.py.

    python tools/batch_gradient_times.py [--quick] [ssy5 ssy10 ssy11 gcy5]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from batch_family import member, package_model         # noqa: E402

SHAPES = {"ssy5": ("ssy", (5,) * 4), "ssy10": ("ssy", (10,) * 4), "ssy11": ("ssy", (11,) * 4), "gcy5": ("gcy", (5,) * 6)}
NEWTON = dict(tol=1e-7, inner_rtol=1e-5, inner_atol=0.0)
POLISH = dict(tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
RTOL = 1e-10
NLOOP = 12


def med(ts):
    return float(np.median(ts))


def main(names, quick):
    import torch
    import sdfs_via_autodiff_amd as S
    from sdfs_via_autodiff_amd import sensitivity as sens
    from sdfs_via_autodiff_amd import _requests
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 64 if quick else 256
    reps = 1 if quick else 3
    nloop = 4 if quick else NLOOP
    print(f"# {torch.cuda.get_device_name(0)}, {cus} CUs; B = {B}; (a) batch gradient at w*, rtol {RTOL:g}; (b) batch Newton from "
          f"800, tol {NEWTON['tol']:g}, inner rtol {NEWTON['inner_rtol']:g}; (c) wc_ratio_gradient looped over {nloop} members, "
          f"rtol {RTOL:g}; {reps} repetitions, medians; the routes alternate in one process")
    for name in names:
        kind, shapes = SHAPES[name]
        N = int(np.prod(shapes))
        models = [package_model(S, kind, member(kind, b)) for b in range(B)]
        op = S.BatchOperator.from_models(models, shapes)
        w = torch.full((B,) + shapes, 800.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        n_iter, err, status, n_apply = op.solve_dev(w.data_ptr(), algorithm="newton", **POLISH)
        assert np.all(status == 0), status
        wstar = w.clone()
        g = torch.from_numpy(0.5 + np.random.default_rng(1).random(shapes)).to(dev)
        mom = torch.empty((B, op.adjoint_words()), dtype=torch.float64, device=dev)
        wh, gh = wstar.cpu().numpy(), g.cpu().numpy()
        torch.cuda.synchronize()
        _requests._OPS_MAX = max(_requests._OPS_MAX, nloop)          # the loop's operator cache holds every member: no handle is built in the timed region

        def gradient_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = op.adjoint_dev(wstar.data_ptr(), g.data_ptr(), 0, None, mom.data_ptr(), rtol=RTOL)
            dt = time.perf_counter() - t0
            assert np.all(out[4] == 0), out[4]
            return dt, out[0], out[1]

        def host_half():
            m = mom.cpu().numpy()
            t0 = time.perf_counter()
            for b in range(B):
                sens.adjoint_moments_to_gradient(models[b], shapes, m[b])
            return time.perf_counter() - t0

        def newton_route():
            w.fill_(800.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_iter, err, status, n_apply = op.solve_dev(w.data_ptr(), algorithm="newton", **NEWTON)
            dt = time.perf_counter() - t0
            assert np.all(status == 0), status
            return dt, n_apply

        def loop_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(nloop):
                S.wc_ratio_gradient(models[b], shapes, wh[b], gh, rtol=RTOL, persistence=True)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        print(f"\n{kind.upper()} {shapes}  N = {N}")
        print("  " + op.describe_plan().replace("\n", "\n  ").rstrip())
        gradient_route(); newton_route(); loop_route()        # warm-up of the three routes
        ta, tb, tc = [], [], []
        for _ in range(reps):
            t, it_a, ap_a = gradient_route(); ta.append(t)
            t, ap_b = newton_route(); tb.append(t)
            tc.append(loop_route())
        th = host_half()
        rounds = (B + cus - 1) // cus
        us_a = 1e6 * med(ta) / (int(ap_a.max()) * rounds)
        us_b = 1e6 * med(tb) / (int(ap_b.max()) * rounds)
        gps_a, gps_c = B / med(ta), nloop / med(tc)
        print(f"  (a) gradient {med(ta):8.4f} s  {gps_a:9.1f} gradients/s  {us_a:7.2f} us/application/problem  iterations "
              f"{it_a.mean():.1f}, applications {ap_a.mean():.1f} per member; host half {th:.4f} s for {B} members")
        print(f"  (b) newton   {med(tb):8.4f} s  {B / med(tb):9.1f} problems/s   {us_b:7.2f} us/application/problem  applications "
              f"{ap_b.mean():.1f} per member")
        print(f"  (c) loop     {med(tc):8.4f} s  {gps_c:9.1f} gradients/s  ({nloop} members)")
        print(f"  (a)/(c) gradients per second = {gps_a / gps_c:7.2f}   (a)/(b) us per application = {us_a / us_b:5.2f}")
        op.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args or list(SHAPES), "--quick" in sys.argv)

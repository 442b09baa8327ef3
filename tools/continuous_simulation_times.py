"""
Times of continuous-state paths at w* (sdfs_via_autodiff_amd/simulation.py ``simulate_continuous``) at the
reference's default grids, SSY 10x10x10x20 and GCY 10^4 x 20^2, Gauss-Hermite d = 5 (-> profiles/).

Per grid: the E_x[M] application (the C_EM form of cont_kernel), k_cont_sim_records, and k_cont_sim_paths in path-steps
per second for every look-ahead (1, 2, 4 states folded side by side) and group (4, 8, 16 corners loaded together) -- the
A/B that chose the defaults (HIP-event counters).  SSY runs at a Newton fixed point; the GCY grid (4 M points x 15625
nodes per application) would take minutes to solve, so it runs at a smooth synthetic grid function > 1.  For context:
k_sim_paths of the discretised chain at SSY 15^4, and the numpy twin (tests/cont_sim_oracle.py) on the host.

    python tools/continuous_simulation_times.py [--paths P] [--periods T] [--quick] [ssy gcy]

--quick: one launch of each kernel per grid with the defaults (the run rocprofv3 traces or counts).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdfs_via_autodiff_amd as S                                   # noqa: E402
from sdfs_via_autodiff_amd import _requests  # noqa: E402
from sdfs_via_autodiff_amd.simulation import cdf_tables           # noqa: E402

GRIDS = {"ssy": ("ssy", (10, 10, 10, 20)), "gcy": ("gcy", (10, 10, 10, 10, 20, 20))}
BURN = 16
FORMS = [(k, g) for g in (4, 8, 16) for k in (1, 2, 4)]


def counter_ms(op, name):
    for k in op.counters():
        if k["name"] == name:
            return k["total_ms"] / k["launches"]
    raise KeyError(name)


def smooth_w(grids):
    mesh = np.meshgrid(*[np.linspace(-1.0, 1.0, len(g)) for g in grids], indexing="ij")
    return 700.0 + 60.0 * sum(np.sin(1.0 + 0.7 * d + m) for d, m in enumerate(mesh))


def main(names, P, T, quick):
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)}; P = {P} paths, T = {T} recorded steps after a burn-in of {BURN}, zero "
          f"start; Gauss-Hermite d = 5; kernel times are HIP-event means")
    for nm in names:
        kind, sizes = GRIDS[nm]
        m = S.SSY() if kind == "ssy" else S.GCY()
        grids = S.build_grid(m, *sizes)
        nodes, weights = S.qnwnorm([5] * len(sizes))
        op = S.ContinuousOperator(np.array(m.params), grids, np.ascontiguousarray(nodes.T), weights)
        N, D = op.size, len(sizes)
        if kind == "ssy":
            xs, _, _ = op.solve(np.ones(sizes), "successive_approx", tol=1e-2, max_iter=50000)
            wh, _, info = op.solve(xs, "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
            what = f"Newton fixed point (status {info['status']})"
        else:
            wh, what = smooth_w(grids), "smooth synthetic w > 1 (a solve at this size takes minutes)"
        w = torch.from_numpy(np.ascontiguousarray(wh)).to(dev)
        em = torch.empty_like(w)
        rec = torch.empty((N, 2), dtype=torch.float64, device=dev)
        stats = torch.empty((19, P), dtype=torch.float64, device=dev)
        clamped = torch.empty((P,), dtype=torch.int32, device=dev)
        final = torch.empty((P, D), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        print(f"{nm}  {'x'.join(map(str, sizes))}  N = {N}, M = {weights.size} nodes, {what}")
        print("  " + op.describe_plan().strip())

        def paths(k=0, g=0):
            op.cont_sim_paths_dev(rec.data_ptr(), 1, 0, P, BURN, T, stats.data_ptr(), clamped.data_ptr(), final.data_ptr(),
                                  lookahead=k, group=g)
        op.set_profiling(True)
        op.cont_sdf_mean_dev(w.data_ptr(), em.data_ptr())
        op.cont_sim_records_dev(w.data_ptr(), em.data_ptr(), rec.data_ptr())
        if quick:
            paths()
            op.synchronize()
            op.set_profiling(False)
            continue
        op.synchronize()
        op.reset_counters()
        reps = 3 if kind == "ssy" else 1
        for _ in range(reps):
            op.cont_sdf_mean_dev(w.data_ptr(), em.data_ptr())
            op.cont_sim_records_dev(w.data_ptr(), em.data_ptr(), rec.data_ptr())
        op.synchronize()
        t = counter_ms(op, "cont:EM")
        print(f"  E_x[M] application (cont_kernel, C_EM): {t:10.3f} ms  {N * weights.size / (t * 1e-3) / 1e9:7.2f} G node "
              f"evaluations/s")
        t = counter_ms(op, "csim:records")
        print(f"  k_cont_sim_records: {1e3 * t:10.1f} us  {32.0 * N / (t * 1e-3) / 1e9:7.0f} GB/s (w, E_M in, 16-B records out)")
        steps = float(P) * (BURN + T)
        for k, g in FORMS:
            if g == 16 and (D == 4 or k == 4):
                continue
            paths(k, g)
            op.synchronize()
            op.reset_counters()
            for _ in range(2):
                paths(k, g)
            op.synchronize()
            t = counter_ms(op, "csim:paths")
            print(f"  k_cont_sim_paths  lookahead {k}  group {g:2d}: {t:9.2f} ms  {steps / (t * 1e-3) / 1e9:6.3f} G path-steps/s")
        share = clamped.cpu().numpy() / float(T)
        print(f"  clamped share of the recorded steps: mean {share.mean():.4f}, largest path {share.max():.4f}")
        op.set_profiling(False)
        del w, em, rec, stats, clamped, final, op
        torch.cuda.empty_cache()
    if quick:
        return
    # context: the discretised simulator, and the twin on the host
    shapes = (15,) * 4
    m = S.SSY()
    op, _ = _requests._operator(m, shapes)
    w = torch.full(shapes, 800.0, dtype=torch.float64, device=dev)
    op.solve_dev(w.data_ptr(), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
    rec = torch.empty((op.size, 8), dtype=torch.float64, device=dev)
    cdf, cdf0 = cdf_tables(m, shapes)
    cdf, cdf0 = np.concatenate([c.ravel() for c in cdf]), np.concatenate(cdf0)
    stats = torch.empty((19, P), dtype=torch.float64, device=dev)
    op.sim_records_dev(w.data_ptr(), None, rec.data_ptr())
    op.set_profiling(True)
    for _ in range(3):
        op.sim_paths_dev(rec.data_ptr(), cdf, cdf0, 1, 0, P, BURN, T, stats_ptr=stats.data_ptr())
    torch.cuda.synchronize()
    t = counter_ms(op, "sim:paths")
    op.set_profiling(False)
    print(f"context: k_sim_paths (discretised chain, SSY 15^4, defaults, no claim): {t:9.2f} ms  "
          f"{float(P) * (BURN + T) / (t * 1e-3) / 1e9:6.2f} G path-steps/s")
    import cont_sim_oracle as co
    import cont_sim_cases as CC
    kind, sizes = GRIDS["ssy"]
    par = CC.params_of(kind)
    grids = CC.grids_of(kind, sizes, 3.2)
    wh = smooth_w(grids)
    p, t = 1 << 12, 64
    t0 = time.perf_counter()
    co.simulate(kind, par, grids, wh, np.full(sizes, 0.998), seed=1, n_paths=p, burn_in=0, n_periods=t)
    dt = time.perf_counter() - t0
    print(f"context: numpy twin (tests/cont_sim_oracle.py, SSY 10x10x10x20, {p} paths x {t} steps, this process's CPU "
          f"threads): {p * t / dt / 1e6:.2f} M path-steps/s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("grids", nargs="*", default=["ssy", "gcy"])
    ap.add_argument("--paths", type=int, default=1 << 20)
    ap.add_argument("--periods", type=int, default=240)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    main(a.grids, a.paths, a.periods, a.quick)

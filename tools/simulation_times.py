"""
Times of simulated paths at w* (sdfs_via_autodiff_amd/simulation.py) on SSY 15^4, GCY 16^6 and GCY 20^6 (-> profiles/).

Per grid, at a tight Newton fixed point, with a claim (κ = 2, nine series) and P paths of T steps after a burn-in of 16:
k_sim_records against the streaming-copy rate measured in the same process, and k_sim_paths in path-steps per second
for every look-ahead depth (1, 2, 4 record loads in flight) and both inverse-CDF searches (binary, linear) -- the A/B
that chose the defaults (HIP-event counters).  Then the numpy twin (tests/sim_oracle.py) on the host for comparison.

    python tools/simulation_times.py [--paths P] [--periods T] [--quick] [ssy15 gcy16 gcy20]

--quick: one k_sim_paths launch per grid with the defaults (the run rocprofv3 traces or counts).
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

GRIDS = {"ssy15": ("ssy", (15,) * 4), "gcy16": ("gcy", (16,) * 6), "gcy20": ("gcy", (20,) * 6)}
KAPPA = 2.0
BURN = 16


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def counter_ms(op, name):
    for k in op.counters():
        if k["name"] == name:
            return k["total_ms"] / k["launches"]
    raise KeyError(name)


def main(names, P, T, quick):
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)}; P = {P} paths, T = {T} recorded steps after a burn-in of {BURN}, "
          f"kappa = {KAPPA}; kernel times are HIP-event means")
    for nm in names:
        kind, shapes = GRIDS[nm]
        m = S.SSY() if kind == "ssy" else S.GCY()
        op, _ = _requests._operator(m, shapes)
        N = op.size
        w = torch.full(shapes, 800.0, dtype=torch.float64, device=dev)
        op.solve_dev(w.data_ptr(), "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
        v = torch.from_numpy(S.claim_prices(m, shapes, w, KAPPA)["pd"]).to(dev)
        rec = torch.empty((N, 8), dtype=torch.float64, device=dev)
        cdf, cdf0 = cdf_tables(m, shapes)
        cdf, cdf0 = np.concatenate([c.ravel() for c in cdf]), np.concatenate(cdf0)
        stats = torch.empty((28, P), dtype=torch.float64, device=dev)
        print(f"{nm}  N = {N}")

        def paths(k=0, s=0):
            op.sim_paths_dev(rec.data_ptr(), cdf, cdf0, 1, 0, P, BURN, T, kappa=KAPPA, stats_ptr=stats.data_ptr(),
                             lookahead=k, search=s)
        op.set_profiling(True)
        op.sim_records_dev(w.data_ptr(), v.data_ptr(), rec.data_ptr())
        if quick:
            paths()
            torch.cuda.synchronize()
            op.set_profiling(False)
            del rec, stats, v, w
            _requests._ops.clear()
            torch.cuda.empty_cache()
            continue
        a = torch.empty_like(w)
        op.stream_copy_dev(w.data_ptr(), a.data_ptr(), N)
        t_copy = timed(lambda: op.stream_copy_dev(w.data_ptr(), a.data_ptr(), N), 20)
        copy_gbs = 16.0 * N / t_copy / 1e9
        print(f"  streaming copy: {1e3 * t_copy:.3f} ms = {copy_gbs:.0f} GB/s")
        op.reset_counters()
        for _ in range(5):
            op.sim_records_dev(w.data_ptr(), v.data_ptr(), rec.data_ptr())
        torch.cuda.synchronize()
        t = counter_ms(op, "sim:records")
        gbs = N * (24.0 + 64.0) / (t * 1e-3) / 1e9
        print(f"  k_sim_records: {1e3 * t:8.1f} us  {gbs:6.0f} GB/s = {gbs / copy_gbs:.2f} of the copy rate "
              f"(w, E_M, v in, 64-B records out)")
        steps = float(P) * (BURN + T)
        for s, sname in ((2, "binary"), (1, "linear")):
            for k in (1, 2, 4):
                paths(k, s)
                op.reset_counters()
                for _ in range(3):
                    paths(k, s)
                torch.cuda.synchronize()
                t = counter_ms(op, "sim:paths")
                print(f"  k_sim_paths  lookahead {k}  {sname:6s} search: {t:8.2f} ms  "
                      f"{steps / (t * 1e-3) / 1e9:6.2f} G path-steps/s")
        op.set_profiling(False)
        del a, rec, stats, v, w
        _requests._ops.clear()
        torch.cuda.empty_cache()
    if not quick:
        import sim_oracle as so
        kind, shapes = GRIDS["ssy15"]
        m = S.SSY()
        arr = S.discretize_ssy(m, shapes)
        cdf, cdf0 = cdf_tables(m, shapes, arr)
        rng = np.random.default_rng(0)
        w = 800.0 + rng.random(shapes)
        em = np.full(shapes, 0.998)
        v = w - 1.0
        p, t = 1 << 14, 64
        t0 = time.perf_counter()
        so.simulate(kind, m.params, arr, shapes, cdf, cdf0, w, em, v, KAPPA, seed=1, n_paths=p, burn_in=0, n_periods=t)
        dt = time.perf_counter() - t0
        print(f"numpy twin (tests/sim_oracle.py, SSY 15^4, {p} paths x {t} steps, this process's CPU threads): "
              f"{p * t / dt / 1e6:.2f} M path-steps/s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("grids", nargs="*", default=["ssy15", "gcy16", "gcy20"])
    ap.add_argument("--paths", type=int, default=1 << 20)
    ap.add_argument("--periods", type=int, default=1200)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    main(a.grids, a.paths, a.periods, a.quick)

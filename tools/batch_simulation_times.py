"""
Throughput of the batch simulation (csrc/batch_sim.hpp) against ``simulate`` looped over the same members
(-> profiles/batch_simulation_times.txt).

Per shape, one process, the routes alternating after a warm-up of each, three repetitions (median, and min / max):
  (a) BatchOperator.simulate_dev: records + paths + moments with stats_dev NULL, B = 256 members, P = 4096 paths of
      T = 1200 recorded steps after burn-in 16, kappa = 2; with the records in LDS (records=1, where the shape fits) and
      gathered from global memory (records=2) at lookahead 1, 2 and 4;
  (b) BatchOperator.price_dev alone (E_M and the claim's price-dividend grid), for its share of an estimation step;
  (c) simulate(...) member after member over 12 members at the same P and T, the single-problem handles warm.
Per row: milliseconds per batch (or per member for (c)), path-steps per second (burn-in included), and the ratio of
(a) to (c) per member.  Members are the fixed family of tests/batch_family.py at their Newton fixed points.

    python tools/batch_simulation_times.py [--quick] [ssy5 ssy10 ssy11 gcy5]
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
KAPPA, BURN, NLOOP, REPS = 2.0, 16, 12, 3


def med(ts):
    return float(np.median(ts))


def main(names, quick):
    import torch
    import sdfs_via_autodiff_amd as S
    from sdfs_via_autodiff_amd import _lib
    from sdfs_via_autodiff_amd.batch import batch_cdf_tables
    B, P, T = (32, 1024, 200) if quick else (256, 4096, 1200)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# {torch.cuda.get_device_name(0)}, {cus} CUs; B = {B} members, P = {P} paths, T = {T} after burn-in {BURN}, kappa = "
          f"{KAPPA:g}; medians of {REPS} (min / max), routes alternating after a warm-up of each")
    print("# for orientation, not a threshold: k_sim_paths alone ran 45.5 G path-steps/s at SSY 15^4 with 2^20 paths (DESIGN §4.8)")
    for name in names:
        kind, shapes = SHAPES[name]
        models = [package_model(S, kind, member(kind, b)) for b in range(B)]
        sol = S.solve_batch(models, shapes, algorithm="newton", tol=1e-10)
        assert np.all(sol.status == 0), sol.status
        op = S.BatchOperator.from_models(models, shapes)
        N, nstat = op.size, 28
        wd = op._to_dev(sol.w)
        dev = wd.device
        em, pd = torch.empty_like(wd), torch.empty_like(wd)
        pmom = torch.empty((B, _lib.SDFS_BATCH_PRICE_WORDS), dtype=torch.float64, device=dev)
        rec = torch.empty((B, N, 8), dtype=torch.float64, device=dev)
        mom = torch.empty((B, nstat, 3), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        kap = np.full(B, KAPPA)
        weights = op._stationary_weights()
        cdf, cdf0 = batch_cdf_tables(kind, shapes, op._arrays)

        def price():
            st = op.price_dev(wd.data_ptr(), kap, None, weights, 0, em.data_ptr(), None, pd.data_ptr(), None, pmom.data_ptr(), None)[-1]
            assert np.all(st == 0), st

        def sim(records, lookahead):
            op.simulate_dev(wd.data_ptr(), em.data_ptr(), pd.data_ptr(), rec.data_ptr(), cdf, cdf0, P, T, burn_in=BURN, seed=7,
                            kappa=kap, records=records, lookahead=lookahead, moments_ptr=mom.data_ptr())
            op.synchronize()

        def loop():
            for b in range(NLOOP):
                S.simulate(models[b], shapes, sol.w[b], P, T, burn_in=BURN, seed=7, kappa=KAPPA)
        price()
        routes = [("price_dev", price)]
        fits = S.batch_sim_lds_bytes(kind, shapes, 1) is not None
        if fits:
            routes.append(("sim lds", lambda: sim(1, 0)))
        for k in (1, 2, 4):
            routes.append((f"sim global K={k}", lambda k=k: sim(2, k)))
        routes.append((f"loop x{NLOOP}", loop))
        ref = None
        for label, fn in routes:                      # warm-up, and the forms agree bit for bit
            fn()
            if label.startswith("sim"):
                m = mom.cpu().numpy()
                assert ref is None or np.array_equal(ref, m, equal_nan=True), label
                ref = m
        times = {label: [] for label, _ in routes}
        for _ in range(REPS):
            for label, fn in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[label].append(time.perf_counter() - t0)
        steps = float(P) * (T + BURN)
        t_loop = med(times[f"loop x{NLOOP}"]) / NLOOP
        lds = f"fits: {S.batch_sim_lds_bytes(kind, shapes, 1)} B" if fits else "does not fit"
        print(f"\n{name}: {kind.upper()} {shapes}, {N} points; LDS form {lds}; global form {S.batch_sim_lds_bytes(kind, shapes, 2)} B")
        for label, _ in routes:
            ts = times[label]
            if label.startswith("sim"):
                per = med(ts) / B
                print(f"  (a) {label:16s} {1e3 * med(ts):9.3f} ms per batch ({1e3 * min(ts):.3f} / {1e3 * max(ts):.3f}), "
                      f"{B * steps / med(ts) / 1e9:7.2f} G path-steps/s, {1e6 * per:8.1f} us per member, (a)/(c) = {t_loop / per:6.1f}")
            elif label == "price_dev":
                print(f"  (b) {label:16s} {1e3 * med(ts):9.3f} ms per batch ({1e3 * min(ts):.3f} / {1e3 * max(ts):.3f})")
            else:
                print(f"  (c) {label:16s} {1e3 * t_loop:9.3f} ms per member ({1e3 * min(ts) / NLOOP:.3f} / {1e3 * max(ts) / NLOOP:.3f}), "
                      f"{steps / t_loop / 1e9:7.2f} G path-steps/s")
        op.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args or list(SHAPES), "--quick" in sys.argv)

"""
Times of continuous-state paths with the claim series rd, xd, pd (``simulate_continuous(..., kappa=)``)
against the plain form, at the reference's default grids, SSY 10x10x10x20 and GCY 10^4 x 20^2, Gauss-Hermite d = 5
(-> profiles/continuous_claim_simulation_times.txt).

Per grid: k_cont_sim_paths (defaults) and k_cont_sim_claim_paths with groups of 4 and of 8 corners, alternating in one
process, REPS times; per form the median and the range of the HIP-event times of its launches, path-steps per second and
claim form / plain form.  SSY runs at a Newton fixed point; the GCY grid (4 M points x 15625 nodes per application) would
take minutes to solve, so it runs at a smooth synthetic grid function > 1.  v is a smooth synthetic grid function > 0 on
both (a solved v changes no instruction the kernel runs).

    python tools/continuous_claim_simulation_times.py [--paths P] [--periods T] [--quick] [ssy gcy]

--quick: one launch of each form per grid with the defaults (the run rocprofv3 traces or counts).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sdfs_via_autodiff_amd as S                                   # noqa: E402

GRIDS = {"ssy": ("ssy", (10, 10, 10, 20)), "gcy": ("gcy", (10, 10, 10, 10, 20, 20))}
BURN = 16
REPS = 9
KAPPA = 2.0


def counter_ms(op, name):
    for k in op.counters():
        if k["name"] == name:
            return k["total_ms"] / k["launches"]
    raise KeyError(name)


def smooth_w(grids):
    mesh = np.meshgrid(*[np.linspace(-1.0, 1.0, len(g)) for g in grids], indexing="ij")
    return 700.0 + 60.0 * sum(np.sin(1.0 + 0.7 * d + m) for d, m in enumerate(mesh))


def smooth_v(grids):
    mesh = np.meshgrid(*[np.linspace(-1.0, 1.0, len(g)) for g in grids], indexing="ij")
    return 60.0 + 8.0 * sum(np.cos(0.5 + 0.9 * d + m) for d, m in enumerate(mesh))


def main(names, P, T, quick):
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_name(0)}; P = {P} paths, T = {T} recorded steps after a burn-in of {BURN}, zero "
          f"start; Gauss-Hermite d = 5; kappa = {KAPPA}; per form the median [min ... max] of {REPS} HIP-event times, the "
          f"forms alternating")
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
        v = torch.from_numpy(np.ascontiguousarray(smooth_v(grids))).to(dev)
        em = torch.empty_like(w)
        rec = torch.empty((N, 2), dtype=torch.float64, device=dev)
        crec = torch.empty((N, 4), dtype=torch.float64, device=dev)
        stats = torch.empty((28, P), dtype=torch.float64, device=dev)
        clamped = torch.empty((P,), dtype=torch.int32, device=dev)
        final = torch.empty((P, D), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        print(f"{nm}  {'x'.join(map(str, sizes))}  N = {N}, M = {weights.size} nodes, {what}, smooth synthetic v > 0")
        op.cont_sdf_mean_dev(w.data_ptr(), em.data_ptr())
        op.cont_sim_records_dev(w.data_ptr(), em.data_ptr(), rec.data_ptr())
        op.cont_sim_claim_records_dev(w.data_ptr(), em.data_ptr(), v.data_ptr(), crec.data_ptr())
        out = (stats.data_ptr(), clamped.data_ptr(), final.data_ptr())
        forms = {"plain (defaults)": ("csim:paths", lambda: op.cont_sim_paths_dev(rec.data_ptr(), 1, 0, P, BURN, T, *out))}
        for g in (4, 8):
            forms[f"claim, group {g}"] = ("csim:claim_paths", lambda g=g: op.cont_sim_claim_paths_dev(
                crec.data_ptr(), KAPPA, 1, 0, P, BURN, T, *out, group=g))
        default = "claim, group 8"
        op.set_profiling(True)
        if quick:
            forms["plain (defaults)"][1]()
            forms[default][1]()
            op.synchronize()
            op.set_profiling(False)
            continue
        for _, call in forms.values():          # one launch of each, not timed
            call()
        op.synchronize()
        times = {k: [] for k in forms}
        for _ in range(REPS):
            for k, (counter, call) in forms.items():
                op.reset_counters()
                call()
                op.synchronize()
                times[k].append(counter_ms(op, counter))
        steps = float(P) * (BURN + T)
        med = {k: float(np.median(t)) for k, t in times.items()}
        for k, t in times.items():
            tag = " (default)" if k == default else ""
            print(f"  {k + tag:26s}: {med[k]:8.2f} ms [{min(t):7.2f} ... {max(t):7.2f}]  {steps / (med[k] * 1e-3) / 1e9:6.3f} G path-steps/s"
                  f"  {med[k] / med['plain (defaults)']:5.2f} x plain")
        op.reset_counters()
        op.cont_sim_claim_records_dev(w.data_ptr(), em.data_ptr(), v.data_ptr(), crec.data_ptr())
        op.synchronize()
        t = counter_ms(op, "csim:claim_records")
        print(f"  k_cont_sim_claim_records: {1e3 * t:10.1f} us  {56.0 * N / (t * 1e-3) / 1e9:7.0f} GB/s (w, E_M, v in, 32-B records out)")
        share = clamped.cpu().numpy() / float(T)
        print(f"  clamped share of the recorded steps: mean {share.mean():.4f}, largest path {share.max():.4f}")
        op.set_profiling(False)
        del w, v, em, rec, crec, stats, clamped, final, op
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("grids", nargs="*", default=["ssy", "gcy"])
    ap.add_argument("--paths", type=int, default=1 << 20)
    ap.add_argument("--periods", type=int, default=240)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    main(a.grids, a.paths, a.periods, a.quick)

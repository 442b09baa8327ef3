"""
Times of continuous-state pricing (sdfs_via_autodiff_amd/pricing.py ``*_continuous``, csrc/cont_price.hpp)
on one MI355X (-> profiles/continuous_pricing_times.txt).

Per grid: ``cont_set_tilt_dev``; one application of K(p, ., .) for p = 0, 1, 2 beside the handle's T and J·v; 120 horizons of the term structure; one perpetual-claim solve at κ = 2 (κ = 1 where κ = 2 has no
finite price) with its iteration count.  Every window is warmed up; the variants alternate within one process, one
launch each per repetition, timed by HIP events (the library's counters).  The criterion of §4.15: the p = 1 product
takes at most (1 + s + 0.05) times the handle's J·v of the same run, s = the relative spread (max − min) / min of J·v
over the repetitions.

    python tools/continuous_pricing_times.py [--reps R] [--out FILE] [ssy gcy-small gcy]

ssy: 10x10x10x20, d = 5, at a Newton w*.  gcy-small: 6^4 x 10^2 at num_std_devs = 1.0, d = 3, at a Newton w* where the
solve converges (else at a smooth synthetic w > 1).  gcy: 10^4 x 20^2, d = 5, at the synthetic w, applications only.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sdfs_via_autodiff_amd as S                                   # noqa: E402
from sdfs_via_autodiff_amd import SdfsError                        # noqa: E402

GRIDS = {"ssy": ("ssy", (10, 10, 10, 20), 3.2, 5, True), "gcy-small": ("gcy", (6, 6, 6, 6, 10, 10), 1.0, 3, True),
         "gcy": ("gcy", (10, 10, 10, 10, 20, 20), 3.2, 5, False)}
HORIZONS = 120
NAMES = {"T": "cont:T", "Jv": "cont:jvp", "K0": "cont:K0", "K1": "cont:K1", "K2": "cont:K2"}


def counter_ms(op, name):
    for k in op.counters():
        if k["name"] == name:
            return k["total_ms"] / k["launches"]
    raise KeyError(name)


def smooth_w(grids):
    mesh = np.meshgrid(*[np.linspace(-1.0, 1.0, len(g)) for g in grids], indexing="ij")
    return 700.0 + 60.0 * sum(np.sin(1.0 + 0.7 * d + m) for d, m in enumerate(mesh))


def operator(m, grids, d):
    nodes, weights = S.qnwnorm([d] * len(grids))
    return S.ContinuousOperator(np.array(m.params), grids, np.ascontiguousarray(nodes.T), weights)


def main(names, reps, out):
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}; kernel times are HIP events around one launch, median [min, max] over the "
        f"repetitions of one process, variants alternating; wall times include the host")
    for nm in names:
        kind, sizes, sd, d, full = GRIDS[nm]
        m = S.SSY() if kind == "ssy" else S.GCY()
        grids = S.build_grid(m, *sizes, num_std_devs=sd)
        op = operator(m, grids, d)
        n_rep = reps if full else max(2, reps // 3)
        wh, what = smooth_w(grids), "smooth synthetic w > 1"
        if full:
            try:
                xs, _, i0 = op.solve(np.ones(sizes), "successive_approx", tol=1e-2, max_iter=20000)
                x, _, info = op.solve(xs, "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
                if info["status"] == 0 and np.all(x > 1.0):
                    wh, what = x, f"Newton fixed point, max|Tw - w| = {np.max(np.abs(op(x) - x)):.1e}"
                else:
                    what += f" (no fixed point found: SA status {i0['status']}, Newton status {info['status']})"
            except SdfsError as e:
                what += f" (no fixed point found: {e})"
        say(f"{nm}  {kind.upper()} {'x'.join(map(str, sizes))}, num_std_devs = {sd}, Gauss-Hermite d = {d}: N = {op.size}, "
            f"M = {d ** len(sizes)} nodes; {what}")
        say("  " + op.describe_plan().strip())
        θ, γ = m.θ, m.γ
        w = torch.from_numpy(np.ascontiguousarray(wh)).to(dev)
        f = 0.5 + torch.rand(sizes, dtype=torch.float64, device=dev)
        o = torch.empty_like(w)
        torch.cuda.synchronize()
        tilts = {"K0": (0, 0.0, 2.0), "K1": (1, θ, 2.0 - γ), "K2": (2, 2.0 * θ, -2.0 * γ)}

        def run(which):
            if which == "T":
                op.apply_dev(w.data_ptr(), o.data_ptr())
            elif which == "Jv":
                op.jvp_dev(f.data_ptr(), o.data_ptr())
            else:
                op.cont_set_tilt_dev(w.data_ptr(), *tilts[which])
                op.cont_apply_tilted_dev(f.data_ptr(), o.data_ptr())

        op.linearize_dev(w.data_ptr())
        variants = ["T", "Jv", "K0", "K1", "K2"]
        op.set_profiling(True)
        for which in variants:                          # warm-up
            run(which)
        times = {i: [] for i in range(len(variants))}
        d2 = []
        wall_tilt = []
        for _ in range(n_rep):
            for i, which in enumerate(variants):
                op.synchronize()
                op.reset_counters()
                t0 = time.perf_counter()
                if which in tilts:
                    op.cont_set_tilt_dev(w.data_ptr(), *tilts[which])
                    op.synchronize()
                    wall_tilt.append(1e3 * (time.perf_counter() - t0))
                    op.cont_apply_tilted_dev(f.data_ptr(), o.data_ptr())
                else:
                    run(which)
                op.synchronize()
                times[i].append(counter_ms(op, NAMES[which]))
                if which in tilts:
                    d2.append(counter_ms(op, "cprice:d2"))
        op.set_profiling(False)

        def fmt(v):
            return f"{np.median(v):11.4f} ms  [{min(v):.4f}, {max(v):.4f}]"
        labels = ["T (cont_kernel C_T)", "J.v (C_JVP)", "K(0, 0, 2) (C_K0)", "K(1, θ, 2-γ) (C_K1)",
                  "K(2, 2θ, -2γ) (C_K2)"]
        say(f"  one application, {n_rep} repetitions:")
        for i, lab in enumerate(labels):
            say(f"    {lab:42s} {fmt(times[i])}")
        say(f"    set_tilt: k_cont_tilt_d2 {fmt(d2)}; the call with its upload and synchronisation {np.median(wall_tilt):.3f} ms wall")
        jv, k1, k0 = times[1], times[3], times[2]
        s = (max(jv) - min(jv)) / min(jv)
        ratio = np.median(k1) / np.median(jv)
        say(f"  criterion: K1 / J.v = {ratio:.4f}, allowed 1 + s + 0.05 = {1.0 + s + 0.05:.4f} (s = {s:.4f}): "
            f"{'met' if ratio <= 1.0 + s + 0.05 else 'NOT met'}")
        say(f"  K0 / K1 = {np.median(k0) / np.median(k1):.4f} (no power, half the LDS)")
        if not full:
            del op, w, f, o
            torch.cuda.empty_cache()
            continue
        # the horizon loop
        op.cont_set_tilt_dev(w.data_ptr(), 1, θ, -γ)
        st = np.zeros((1, len(sizes)))
        hz = []
        note = ""
        for r in range(1 + min(n_rep, 3)):
            t0 = time.perf_counter()
            try:
                op.cont_tilted_horizons_dev(HORIZONS, st)
            except SdfsError as e:
                note = f" ({e})"
            if r:
                hz.append(1e3 * (time.perf_counter() - t0))
        say(f"  {HORIZONS} horizons of K(1, θ, -γ), one query state: {np.median(hz):.3f} ms wall, "
            f"{np.median(hz) / HORIZONS:.4f} ms per horizon{note}")
        # the perpetual claim
        one = torch.ones_like(w)
        k1v, v = torch.empty_like(w), torch.empty_like(w)
        torch.cuda.synchronize()
        for κ in (2.0, 1.0):
            op.cont_set_tilt_dev(w.data_ptr(), 1, θ, κ - γ)
            op.cont_apply_tilted_dev(one.data_ptr(), k1v.data_ptr())
            try:
                op.cont_solve_tilted_dev(k1v.data_ptr(), v.data_ptr(), 1e-10)      # warm-up
                t0 = time.perf_counter()
                it, rel = op.cont_solve_tilted_dev(k1v.data_ptr(), v.data_ptr(), 1e-10)
                dt = 1e3 * (time.perf_counter() - t0)
            except SdfsError as e:
                say(f"  perpetual claim, κ = {κ:g}: the solve stopped ({e})")
                continue
            if not bool(torch.all(v > 0)):
                say(f"  perpetual claim, κ = {κ:g}: {it} iterations, {dt:.3f} ms wall, but v is not positive: no finite price")
                continue
            say(f"  perpetual claim, κ = {κ:g}, rtol 1e-10: {it} BiCGSTAB iterations, relative residual {rel:.1e}, {dt:.3f} ms "
                f"wall ({dt / max(it, 1):.4f} ms per iteration, two products each); pd in [{float(v.min()):.2f}, {float(v.max()):.2f}]")
            break
        del op, w, f, o
        torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("grids", nargs="*", default=["ssy", "gcy-small", "gcy"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "continuous_pricing_times.txt"))
    a = ap.parse_args()
    main(a.grids, a.reps, a.out)

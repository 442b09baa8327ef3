"""
Times of the adjoint gradient of the continuous-state model (sdfs_via_autodiff_amd/sensitivity.py
``wc_ratio_gradient_continuous``, csrc/cont_adjoint.hpp, the C_VJP form of csrc/cont_kernel.hpp in csrc/cont_vjp.hip;
DESIGN §4.17) on one MI355X (-> profiles/continuous_gradient_times.txt).

Per grid: one Jᵀu (the zeroing of the output, the scatter form and nothing else: minus_identity off) beside the handle's
J·v at the same linearisation (warmed up, the two alternating within one process, timed by HIP events through the library's
counters), reported as Jᵀu / J·v with the relative spread (max − min) / min of J·v beside it, and the bound on the global
atomic traffic 8 N cap bytes over the time against the chip-wide rate of added bytes; the largest relative difference
between two runs of the same Jᵀu (the call is reproducible to rounding only); then, at a Newton fixed point, the adjoint
solve (iterations, wall time) and ``wc_ratio_gradient_continuous`` for every parameter against
``wc_ratio_sensitivities_continuous`` for every parameter on the same operator (wall times).

The one fixed condition: the whole gradient must take less time than the P forward solves it replaces.  The file says
whether it does.  The ratio Jᵀu / J·v is recorded, not judged.

    python tools/continuous_gradient_times.py [--reps R] [--out FILE] [ssy gcy-small ssy-mc ssy-global]

ssy and gcy-small are the grids of tools/continuous_sensitivity_times.py (both on the pre-contracted path).  ssy-mc (the
same SSY grid with 1000 Monte-Carlo draws: the staged path) and ssy-global (SSY 9x9x9x18 at num_std_devs = 0.4: the
global-gather path) are there for the other two paths, applications only.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sdfs_via_autodiff_amd as S                                   # noqa: E402
from sdfs_via_autodiff_amd import SdfsError                        # noqa: E402
from continuous_pricing_times import GRIDS as PRICING_GRIDS, counter_ms, smooth_w   # noqa: E402

# kind, sizes, num_std_devs, ("gh", d) or ("mc", draws), solve a fixed point and time the gradient, the gather path of
# every block (tests/cont_boxes.py classifies these grids: A-ssy-headline, B-ssy-mc, D-ssy)
GRIDS = {nm: (k, sz, sd, ("gh", d), True, "pre-contracted") for nm, (k, sz, sd, d, full) in PRICING_GRIDS.items() if full}
GRIDS["ssy-mc"] = ("ssy", (10, 10, 10, 20), 3.2, ("mc", 1000), False, "staged")
GRIDS["ssy-global"] = ("ssy", (9, 9, 9, 18), 0.4, ("gh", 5), False, "global gather")
NAMES = {"Jv": "cont:jvp", "JTu": "cont:vjp"}
ATOMIC_RATE = 1.3e12             # bytes added per second by global float atomics, chip-wide: the estimate of DESIGN §4.17


def operator(m, grids, rule):
    if rule[0] == "gh":
        nodes, weights = S.qnwnorm([rule[1]] * len(grids))
        return S.ContinuousOperator(np.array(m.params), grids, np.ascontiguousarray(nodes.T), weights)
    draws = np.random.default_rng(1234).standard_normal((len(grids), rule[1]))
    return S.ContinuousOperator(np.array(m.params), grids, draws, None)


def main(names, reps, out):
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}; kernel times are HIP events around one application, median [min, max] over the "
        f"repetitions of one process, variants alternating; wall times include the host")
    say("# J^T u accumulates with hardware fp64 atomic adds (ds_add_f64 on the LDS accumulators, global_atomic_add_f64 on the "
        "output; the compiled code has no compare-and-swap loop): reproducible to rounding only")
    for nm in names:
        kind, sizes, sd, rule, full, path = GRIDS[nm]
        m = S.SSY() if kind == "ssy" else S.GCY()
        grids = S.build_grid(m, *sizes, num_std_devs=sd)
        op = operator(m, grids, rule)
        wh, what, fixed = smooth_w(grids), "smooth synthetic w > 1", False
        if full:
            try:
                xs, _, i0 = op.solve(np.ones(sizes), "successive_approx", tol=1e-2, max_iter=20000)
                x, _, info = op.solve(xs, "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
                if info["status"] == 0 and np.all(x > 1.0):
                    wh, what, fixed = x, f"Newton fixed point, max|Tw - w| = {np.max(np.abs(op(x) - x)):.1e}", True
                else:
                    what += f" (no fixed point found: SA status {i0['status']}, Newton status {info['status']})"
            except SdfsError as e:
                what += f" (no fixed point found: {e})"
        npar = len(m.params)
        rule_s = f"Gauss-Hermite d = {rule[1]}" if rule[0] == "gh" else f"{rule[1]} Monte-Carlo draws"
        say(f"{nm}  {kind.upper()} {'x'.join(map(str, sizes))}, num_std_devs = {sd}, {rule_s}: N = {op.size}, "
            f"M = {op.nodes.shape[1]} nodes, {npar} parameters; path: {path}; {what}")
        plan = op.describe_plan().strip()
        say("  " + plan)
        w = torch.from_numpy(np.ascontiguousarray(wh)).to(dev)
        f = torch.randn(sizes, dtype=torch.float64, device=dev)
        o, o2 = torch.empty_like(w), torch.empty_like(w)
        torch.cuda.synchronize()

        def run(which, dst=o):
            if which == "Jv":
                op.jvp_dev(f.data_ptr(), dst.data_ptr())
            else:
                op.cont_vjp_dev(f.data_ptr(), dst.data_ptr())

        op.linearize_dev(w.data_ptr())
        variants = ["Jv", "JTu"]
        op.set_profiling(True)
        for which in variants:                          # warm-up
            run(which)
        times = {v: [] for v in variants}
        for _ in range(reps):
            for which in variants:
                op.synchronize()
                op.reset_counters()
                run(which)
                op.synchronize()
                times[which].append(counter_ms(op, NAMES[which]))
        op.set_profiling(False)

        def fmt(v):
            return f"{np.median(v):11.4f} ms  [{min(v):.4f}, {max(v):.4f}]"
        say(f"  one application, {reps} repetitions:")
        say(f"    {'J.v (C_JVP)':42s} {fmt(times['Jv'])}")
        say(f"    {'J^T u (zeroing + C_VJP)':42s} {fmt(times['JTu'])}")
        jv, jt = times["Jv"], times["JTu"]
        s = (max(jv) - min(jv)) / min(jv)
        say(f"  J^T u / J.v = {np.median(jt) / np.median(jv):.4f} (spread of J.v: s = {s:.4f})")
        if path == "global gather":
            ab, how = 8.0 * op.size * op.nodes.shape[1] * 2 ** len(sizes), "8 N M 2^D (every corner of every node"
        else:
            ab, how = 8.0 * op.size * int(plan.split("cap ")[1].split(",")[0]), "8 N cap (every box cell of every point"
        say(f"  global atomic adds: at most {how}; zero contributions are skipped) = {ab / 1e6:.1f} MB per application -> at "
            f"most {ab / (np.median(jt) * 1e-3) / 1e9:.1f} GB/s of added bytes, "
            f"{ab / (np.median(jt) * 1e-3) / ATOMIC_RATE:.3f} of the chip-wide {ATOMIC_RATE / 1e12:.1f} TB/s")
        run("JTu", o)
        run("JTu", o2)
        op.synchronize()
        scale = float(o.abs().max())
        say(f"  two runs of the same J^T u differ by at most {float((o - o2).abs().max()) / scale:.1e} of max|J^T u| "
            f"({int((o != o2).sum())} of {op.size} points differ)")
        if fixed:
            g = torch.full(sizes, 1.0 / op.size, dtype=torch.float64, device=dev)
            lam = torch.empty_like(w)
            torch.cuda.synchronize()
            op.cont_solve_adjoint_dev(g.data_ptr(), lam.data_ptr())      # warm-up
            t0 = time.perf_counter()
            its, rel = op.cont_solve_adjoint_dev(g.data_ptr(), lam.data_ptr())
            dt_solve = 1e3 * (time.perf_counter() - t0)
            say(f"  adjoint solve (I - J^T) lambda = g, g = 1/N, rtol 1e-10: {its} BiCGSTAB iterations, relative residual "
                f"{rel:.1e}, {dt_solve:.3f} ms wall")
            gh = g.cpu().numpy()
            S.wc_ratio_gradient_continuous(m, grids, wh, gh, operator=op)         # warm-up
            t0 = time.perf_counter()
            res = S.wc_ratio_gradient_continuous(m, grids, wh, gh, operator=op)
            dt_grad = 1e3 * (time.perf_counter() - t0)
            S.wc_ratio_sensitivities_continuous(m, grids, wh, operator=op)        # warm-up
            t0 = time.perf_counter()
            fwd = S.wc_ratio_sensitivities_continuous(m, grids, wh, operator=op)
            dt_fwd = 1e3 * (time.perf_counter() - t0)
            fits = [v[0] for v in fwd["_info"].values()]
            names_p = S.SSY_PARAMS if kind == "ssy" else S.GCY_PARAMS
            diff = max(abs(res[p] - float(np.sum(gh * fwd[p]))) / max(abs(res[p]), 1e-300) for p in names_p)
            say(f"  wc_ratio_gradient_continuous, all {npar} parameters, rtol 1e-10: {dt_grad:.3f} ms wall "
                f"({res['_info'][0]} iterations, residual {res['_info'][1]:.1e}); wc_ratio_sensitivities_continuous, all "
                f"{npar} parameters on the same operator: {dt_fwd:.3f} ms wall (BiCGSTAB iterations {min(fits)} ... {max(fits)})")
            say(f"  gradient / {npar} forward solves = {dt_grad / dt_fwd:.4f}: the gradient is "
                f"{'FASTER' if dt_grad < dt_fwd else 'NOT FASTER'} than the forward solves it replaces; the two agree to "
                f"{diff:.1e} relative, worst parameter")
            del g, lam
        del op, w, f, o, o2
        torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("grids", nargs="*", default=["ssy", "gcy-small", "ssy-mc", "ssy-global"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "continuous_gradient_times.txt"))
    a = ap.parse_args()
    main(a.grids, a.reps, a.out)

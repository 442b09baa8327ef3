"""
Times of the continuous-state parameter sensitivities (sdfs_via_autodiff_amd/sensitivity.py
``wc_ratio_sensitivities_continuous``, csrc/cont_sens.hpp, the C_PTAN form of csrc/cont_kernel.hpp) on one
MI355X (-> profiles/continuous_sensitivity_times.txt).

Per grid: one parameter tangent, with ln g from libm's log (C_PTAN) and from the power's own log₂ (C_PTANL, the
SDFS_PTAN_LOG_FROM_POW knob: the A/B behind the default), beside the handle's T and J·v (warmed up, the variants alternating within one process,
one launch each per repetition, timed by HIP events through the library's counters), reported as tangent / J·v with the
relative spread (max − min) / min of J·v beside it; then ``wc_ratio_sensitivities_continuous`` for every parameter
against one default Newton solve of the same operator (wall times).  Expectation from operation counts: the tangent
reads half of J·v's corners, folds three values per corner pair where J·v folds two and adds a logarithm, so it should
land between T's time and about 1.5 × J·v's.  Nothing here is a criterion.

    python tools/continuous_sensitivity_times.py [--reps R] [--out FILE] [ssy gcy-small gcy]

The grids are those of tools/continuous_pricing_times.py.  gcy (10^4 x 20^2, no fixed point found): applications only.
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
from continuous_pricing_times import GRIDS, counter_ms, smooth_w, operator   # noqa: E402

NAMES = {"T": "cont:T", "Jv": "cont:jvp", "tangent": "cont:ptan", "tangentL": "cont:ptan"}
LOG_KNOB = "SDFS_PTAN_LOG_FROM_POW"          # read by the library at every tangent call: 0 = libm's log, 1 = the power's own log2


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
        wh, what, fixed = smooth_w(grids), "smooth synthetic w > 1", False
        newton_ms = None
        if full:
            try:
                t0 = time.perf_counter()
                xs, n_sa, i0 = op.solve(np.ones(sizes), "successive_approx", tol=1e-2, max_iter=20000)
                sa_ms = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                x, n_it, info = op.solve(xs, "newton")
                newton_ms = 1e3 * (time.perf_counter() - t0)
                if info["status"] == 0 and np.all(x > 1.0):
                    x, _, info = op.solve(x, "newton", tol=1e-10, inner_rtol=1e-12, inner_atol=0.0)
                if info["status"] == 0 and np.all(x > 1.0):
                    wh, what, fixed = x, f"Newton fixed point, max|Tw - w| = {np.max(np.abs(op(x) - x)):.1e}", True
                else:
                    what += f" (no fixed point found: SA status {i0['status']}, Newton status {info['status']})"
            except SdfsError as e:
                what += f" (no fixed point found: {e})"
        npar = len(m.params)
        say(f"{nm}  {kind.upper()} {'x'.join(map(str, sizes))}, num_std_devs = {sd}, Gauss-Hermite d = {d}: N = {op.size}, "
            f"M = {d ** len(sizes)} nodes, {npar} parameters; {what}")
        say("  " + op.describe_plan().strip())
        w = torch.from_numpy(np.ascontiguousarray(wh)).to(dev)
        f = 0.5 + torch.rand(sizes, dtype=torch.float64, device=dev)
        o = torch.empty_like(w)
        dp = np.random.default_rng(1).standard_normal(npar)
        torch.cuda.synchronize()

        def run(which):
            if which == "T":
                op.apply_dev(w.data_ptr(), o.data_ptr())
            elif which == "Jv":
                op.jvp_dev(f.data_ptr(), o.data_ptr())
            else:
                os.environ[LOG_KNOB] = "1" if which == "tangentL" else "0"
                try:
                    op.cont_param_tangent_dev(w.data_ptr(), dp, o.data_ptr())
                finally:
                    del os.environ[LOG_KNOB]

        op.linearize_dev(w.data_ptr())
        variants = ["T", "Jv", "tangent", "tangentL"]
        op.set_profiling(True)
        for which in variants:                          # warm-up
            run(which)
        times = {v: [] for v in variants}
        for _ in range(n_rep):
            for which in variants:
                op.synchronize()
                op.reset_counters()
                run(which)
                op.synchronize()
                times[which].append(counter_ms(op, NAMES[which]))
        op.set_profiling(False)

        def fmt(v):
            return f"{np.median(v):11.4f} ms  [{min(v):.4f}, {max(v):.4f}]"
        say(f"  one application, {n_rep} repetitions:")
        for which, lab in zip(variants, ["T (cont_kernel C_T)", "J.v (C_JVP)", "parameter tangent, libm log (C_PTAN)",
                               "parameter tangent, log from the power (C_PTANL)"]):
            say(f"    {lab:42s} {fmt(times[which])}")
        jv = times["Jv"]
        s = (max(jv) - min(jv)) / min(jv)
        for which, lab in (("tangent", "libm log"), ("tangentL", "log from the power")):
            say(f"  {lab}: tangent / J.v = {np.median(times[which]) / np.median(jv):.4f} (spread of J.v: s = {s:.4f}); "
                f"tangent / T = {np.median(times[which]) / np.median(times['T']):.4f}")
        say(f"  A/B of the logarithm: from the power / libm = {np.median(times['tangentL']) / np.median(times['tangent']):.4f}")
        got = {}
        for which in ("tangent", "tangentL"):
            run(which)
            op.synchronize()
            got[which] = o.clone()
        scale = float(got["tangent"].abs().max())
        say(f"    the two tangents differ by at most {float((got['tangent'] - got['tangentL']).abs().max()) / scale:.1e} of max|tangent|")
        if fixed:
            S.wc_ratio_sensitivities_continuous(m, grids, w, operator=op)      # warm-up
            t0 = time.perf_counter()
            res = S.wc_ratio_sensitivities_continuous(m, grids, w, operator=op)
            dt = 1e3 * (time.perf_counter() - t0)
            its = [v[0] for v in res["_info"].values()]
            rel = max(v[1] for v in res["_info"].values())
            say(f"  wc_ratio_sensitivities_continuous, all {npar} parameters, rtol 1e-10: {dt:.3f} ms wall "
                f"({dt / npar:.3f} ms per parameter), BiCGSTAB iterations {min(its)} ... {max(its)}, worst relative residual "
                f"{rel:.1e}; one default Newton solve of the same operator: {newton_ms:.3f} ms wall, {n_it} iterations, "
                f"from the iterate of successive approximation to 1e-2 from w = 1 ({sa_ms:.1f} ms, {n_sa} iterations), as the "
                f"reference's drivers start it -> all sensitivities / (SA + Newton) = {dt / (sa_ms + newton_ms):.2f}, / Newton alone = "
                f"{dt / newton_ms:.1f}")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "continuous_sensitivity_times.txt"))
    a = ap.parse_args()
    main(a.grids, a.reps, a.out)

"""A/B of two builds of the package on one box: the GCY 20^6 headline step (T + fused residual, resident in HBM) with the
package found under argv[1] -- per-step time over 200 steps after spin-up, per-kernel HIP-event times of a second loop.
tools/ab_step.sh runs it alternately for the round-3 build (tools/probes/r3pkg, a worktree of the round-3 HEAD) and the
working tree, since boxes differ by more than the changes under test.

  python tools/ab_step.py --libs <a.so> <b.so> [...] [--rounds R] [--steps K] [--grid n]
is the same measurement in ONE process: every library (file names inside the package directory, loaded side by side
through SDFS_LIB_NAME) gets its own operator on the same device buffers, and the libraries take turns, R rounds of K
steps each (default 7 x 200), so clock, temperature and neighbours hit all of them alike.  Per library: every round's
ms per step, their median, and the per-kernel HIP-event means of a closing loop; the verdict line compares the first
library's (the baseline's) fastest round with every other library's slowest."""
import json, os, sys, time
import numpy as np


def ab_libs(argv):
    import importlib.util
    import statistics
    libs, rounds, steps, n = [], 7, 200, 20
    print("# tools/ab_step.py --libs " + " ".join(argv) + ": the headline step (T + fused residual, resident in HBM) with these builds of the library\n"
          "# side by side in one process, one operator each on the same device buffers, taking turns round by round (the turn\n"
          "# order alternates); ms per step of every round, their median, per-kernel HIP-event means of a closing loop, the\n"
          "# last pass's plan line, and whether the first application of the same w equals the first library's bit for bit.\n"
          "# Rule: a library's slowest round against the first library's (the baseline's) fastest.", flush=True)
    it = iter(argv)
    for a in it:
        if a == "--rounds": rounds = int(next(it))
        elif a == "--steps": steps = int(next(it))
        elif a == "--grid": n = int(next(it))
        else: libs.append(a)
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    pkgdir = os.path.join(root, "sdfs_via_autodiff_amd")
    import torch
    mods = []
    for i, name in enumerate(libs):            # one copy of the package per library (its modules import each other relatively)
        os.environ["SDFS_LIB_NAME"] = name
        spec = importlib.util.spec_from_file_location(f"sdfs_ab{i}", os.path.join(pkgdir, "__init__.py"), submodule_search_locations=[pkgdir])
        m = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = m
        spec.loader.exec_module(m)
        assert os.path.basename(m.LIB_PATH) == name, (m.LIB_PATH, name)
        mods.append(m)
    del os.environ["SDFS_LIB_NAME"]
    shp = (n,) * 6
    stream = torch.cuda.current_stream()
    w = 400 + 500 * np.random.default_rng(0).random(shp)
    w0 = torch.from_numpy(w).cuda()
    bufs = [w0.clone(), torch.empty(shp, dtype=torch.float64, device="cuda")]
    resid = torch.zeros(1, dtype=torch.float64, device="cuda")
    ops = []
    for m in mods:
        g = m.GCY()
        op = m.KoopmansOperator("gcy", shp, g.params, m.discretize_gcy(g, shp))
        op.set_stream(stream.cuda_stream)
        ops.append(op)
    def run(op, k):
        for i in range(k):
            op.apply_dev(bufs[i & 1].data_ptr(), bufs[(i + 1) & 1].data_ptr(), resid.data_ptr())
    # every library's first application of the same w must agree to the last bit
    outs = []
    for op in ops:
        bufs[0].copy_(w0); run(op, 1); torch.cuda.synchronize(); outs.append((bufs[1].clone(), float(resid.item())))
    same = [bool(torch.equal(outs[0][0], o[0])) and outs[0][1] == o[1] for o in outs]
    for op in ops:
        run(op, 150)
    torch.cuda.synchronize()
    ms = [[] for _ in ops]
    for r in range(rounds):
        for j in (range(len(ops)) if r % 2 == 0 else reversed(range(len(ops)))):      # (turn order alternates: nobody always follows the same neighbour)
            op = ops[j]
            t0 = time.perf_counter()
            run(op, steps)
            torch.cuda.synchronize()
            ms[j].append((time.perf_counter() - t0) / steps * 1e3)
    for j, op in enumerate(ops):
        op.set_profiling(True)
        run(op, 8); torch.cuda.synchronize()
        op.reset_counters()
        run(op, steps); torch.cuda.synchronize()
        ks = [(c["name"], round(c["total_ms"] / max(c["launches"], 1), 4)) for c in op.counters() if c["launches"]]
        op.set_profiling(False)
        print(json.dumps({"lib": libs[j], "grid": n, "rounds_ms_per_step": [round(x, 4) for x in ms[j]], "median_ms_per_step": round(statistics.median(ms[j]), 4),
                          "min": round(min(ms[j]), 4), "max": round(max(ms[j]), 4), "kernels_ms": ks, "first_application_equals_baseline": same[j],
                          "plan_last_pass": [ln for ln in op.describe_plan().splitlines() if ln.startswith("pair plan pass 2:")][-1]}), flush=True)
    for j in range(1, len(ops)):
        gain = 1.0 - statistics.median(ms[j]) / statistics.median(ms[0])
        print(f"# {libs[j]} against {libs[0]}: median {statistics.median(ms[j]):.4f} against {statistics.median(ms[0]):.4f} ms per step (gain {100 * gain:.2f} %); "
              f"slowest round {max(ms[j]):.4f} against the baseline's fastest {min(ms[0]):.4f}: {'FASTER in every round' if max(ms[j]) < min(ms[0]) else 'NOT separated from the baseline spread'}", flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "--libs":
    ab_libs(sys.argv[2:])
    sys.exit(0)
pkg = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
sys.path.insert(0, pkg)
import torch
import sdfs_via_autodiff_amd as S
assert os.path.abspath(S.__file__).startswith(os.path.abspath(pkg)), (S.__file__, pkg)
g = S.GCY(); shp = (n,) * 6
arr = S.discretize_gcy(g, shp)
op = S.KoopmansOperator("gcy", shp, g.params, arr)
stream = torch.cuda.current_stream()
op.set_stream(stream.cuda_stream)
w = 400 + 500 * np.random.default_rng(0).random(shp)
bufs = [torch.from_numpy(w).cuda(), torch.empty(shp, dtype=torch.float64, device="cuda")]
resid = torch.zeros(1, dtype=torch.float64, device="cuda")
def step(i):
    op.apply_dev(bufs[i & 1].data_ptr(), bufs[(i + 1) & 1].data_ptr(), resid.data_ptr())
for i in range(150):
    step(i)
torch.cuda.synchronize()
best = 1e9
for rep in range(3):
    t0 = time.perf_counter()
    for i in range(200):
        step(i)
    torch.cuda.synchronize()
    best = min(best, (time.perf_counter() - t0) / 200 * 1e3)
op.set_profiling(True)
for i in range(8):
    step(i)
torch.cuda.synchronize()
op.reset_counters()
for i in range(200):
    step(i)
torch.cuda.synchronize()
ks = [(c["name"], c["total_ms"] / max(c["launches"], 1)) for c in op.counters() if c["launches"]]
print(json.dumps({"pkg": pkg, "grid": n, "ms_per_step": round(best, 4), "kernels_ms": [(k, round(v, 4)) for k, v in ks], "resid": float(resid.item())}), flush=True)

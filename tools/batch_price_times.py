"""
Throughput of batch pricing (csrc/batch_price.hpp) against the batched Newton-Krylov solve on the same handle and against
``sdf_moments`` + ``claim_prices`` + ``term_structure`` looped over members (-> profiles/batch_price_times.txt).

Per shape, B = 256, kappa = 2, rtol 1e-10, one process, the routes alternating, a warm-up of each first, three
repetitions (medians):
  (a) price0    BatchOperator.price_dev at the batch's w* with n_max = 0 -- w*, the words and the horizons
                device-resident, no grids stored;
  (b) price120  the same with n_max = 120 (real bonds, kappa_ts = 0);
  (c) newton    BatchOperator.solve_dev(algorithm="newton", tol 1e-7, inner rtol 1e-5, atol 0) from 800, same handle;
  (d) loop      the three single-problem functions member after member (12 members, n_max = 120; the operators are
                built and cached by a warm-up call outside the timed region).
Per row: seconds, members (problems) per second, microseconds per application per problem (B <= CUs: wall / most
applications of a member, i.e. what one workgroup takes), iterations and applications per member, and the ratios of
members per second to the loop and of microseconds per application to the Newton figure.
Members are the fixed family of tests/batch_family.py.

    python tools/batch_price_times.py [--quick] [--out FILE] [ssy5 ssy10 ssy11 gcy5]
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
KAPPA = 2.0
N_MAX = 120
NLOOP = 12


def med(ts):
    return float(np.median(ts))


def main(names, quick, out_path):
    import torch
    import sdfs_via_autodiff_amd as S
    from sdfs_via_autodiff_amd import _requests
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 64 if quick else 256
    reps = 1 if quick else 3
    nloop = 4 if quick else NLOOP
    say(f"# {torch.cuda.get_device_name(0)}, {cus} CUs; B = {B}; kappa = {KAPPA:g}, rtol {RTOL:g}; (a) batch pricing at w*, n_max = 0; "
        f"(b) the same, n_max = {N_MAX}; (c) batch Newton from 800, tol {NEWTON['tol']:g}, inner rtol {NEWTON['inner_rtol']:g}; "
        f"(d) sdf_moments + claim_prices + term_structure({N_MAX}) looped over {nloop} members; {reps} repetitions, medians; "
        "the routes alternate in one process")
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
        wh = wstar.cpu().numpy()
        mom = torch.empty((B, 12), dtype=torch.float64, device=dev)
        hz = torch.empty((B, N_MAX, 4), dtype=torch.float64, device=dev)
        kap, kts = np.full(B, KAPPA), np.zeros(B)
        gax = op._stationary_weights()
        torch.cuda.synchronize()
        _requests._OPS_MAX = max(_requests._OPS_MAX, nloop)          # the loop's operator cache holds every member: no handle is built in the timed region

        def price_route(n_max):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = op.price_dev(wstar.data_ptr(), kap, kts, gax, n_max, None, None, None, None, mom.data_ptr(),
                               hz.data_ptr() if n_max else None, rtol=RTOL)
            dt = time.perf_counter() - t0
            assert np.all(out[5] == 0), out[5]
            return dt, out[0], out[1]

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
                S.sdf_moments(models[b], shapes, wh[b])
                S.claim_prices(models[b], shapes, wh[b], KAPPA, rtol=RTOL)
                S.term_structure(models[b], shapes, wh[b], N_MAX)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        say(f"\n{kind.upper()} {shapes}  N = {N}")
        say("  " + op.describe_plan().replace("\n", "\n  ").rstrip())
        price_route(0); price_route(N_MAX); newton_route(); loop_route()        # warm-up of the routes
        ta, tb, tc, td = [], [], [], []
        for _ in range(reps):
            t, it_a, ap_a = price_route(0); ta.append(t)
            t, it_b, ap_b = price_route(N_MAX); tb.append(t)
            t, ap_c = newton_route(); tc.append(t)
            td.append(loop_route())
        rounds = (B + cus - 1) // cus
        us_a = 1e6 * med(ta) / (int(ap_a.max()) * rounds)
        us_b = 1e6 * med(tb) / (int(ap_b.max()) * rounds)
        us_c = 1e6 * med(tc) / (int(ap_c.max()) * rounds)
        mps_a, mps_b, mps_d = B / med(ta), B / med(tb), nloop / med(td)
        say(f"  (a) price0   {med(ta):8.4f} s  {mps_a:9.1f} members/s   {us_a:7.2f} us/application/problem  iterations "
            f"{it_a.mean():.1f}, applications {ap_a.mean():.1f} per member")
        say(f"  (b) price120 {med(tb):8.4f} s  {mps_b:9.1f} members/s   {us_b:7.2f} us/application/problem  iterations "
            f"{it_b.mean():.1f}, applications {ap_b.mean():.1f} per member")
        say(f"  (c) newton   {med(tc):8.4f} s  {B / med(tc):9.1f} problems/s  {us_c:7.2f} us/application/problem  applications "
            f"{ap_c.mean():.1f} per member")
        say(f"  (d) loop     {med(td):8.4f} s  {mps_d:9.1f} members/s   ({nloop} members, n_max = {N_MAX})")
        say(f"  (b)/(d) members per second = {mps_b / mps_d:7.2f}   us per application: (a)/(c) = {us_a / us_c:5.2f}  "
            f"(b)/(c) = {us_b / us_c:5.2f}")
        op.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "batch_price_times.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    args = [a for a in argv if not a.startswith("--")]
    main(args or list(SHAPES), "--quick" in argv, out)

"""
Throughput of the batched solve (sdfs_via_autodiff_amd/batch.py) against the single-problem device solve looped over
the same members (-> profiles/batch_times.txt).

Per shape, one process, the two routes alternating, a warm-up of each first, three repetitions (min / median / max):
  loop   T.solve_dev(successive_approx, tol 1e-6) member after member, handles created outside the timed region and
         inside it (what a sweep pays today: sdfs_create + solve + sdfs_destroy per point);
  batch  BatchOperator.solve_dev at B = 1, 8, 64, 256, 1024 (creation outside and inside), seconds per batch,
         microseconds per iteration per problem (B <= CUs: wall / max iterations, i.e. what one workgroup takes),
         problems per second, and the break-even B against the loop.
Members are the fixed family of tests/batch_family.py, so the iteration counts are those of the tests.

    python tools/batch_times.py [--quick] [ssy5 ssy10 ssy11 gcy5]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdfs_via_autodiff_amd as S                       # noqa: E402
from batch_family import member, package_model         # noqa: E402

SHAPES = {"ssy5": ("ssy", (5,) * 4), "ssy10": ("ssy", (10,) * 4), "ssy11": ("ssy", (11,) * 4), "gcy5": ("gcy", (5,) * 6)}
TOL = 1e-6


def stats(ts):
    return f"{min(ts):9.4f} / {float(np.median(ts)):9.4f} / {max(ts):9.4f} s"


def loop_route(kind, shapes, models, w, create_inside, ops=None):
    """Seconds for the members one after the other, and the sum of their iterations."""
    disc = S.discretize_ssy if kind == "ssy" else S.discretize_gcy
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    its = 0
    for b, m in enumerate(models):
        T = S.KoopmansOperator(kind, shapes, m.params, disc(m, shapes)) if create_inside else ops[b]
        w[b].fill_(800.0)
        torch.cuda.synchronize()
        n, _ = T.solve_dev(w[b].data_ptr(), "successive_approx", tol=TOL)
        its += n
        if create_inside:
            T.close()
    return time.perf_counter() - t0, its


def batch_route(kind, shapes, models, w, create_inside, op=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if create_inside:
        op = S.BatchOperator.from_models(models, shapes)
    w.fill_(800.0)
    torch.cuda.synchronize()
    n_iter, err, status = op.solve_dev(w.data_ptr(), tol=TOL)
    dt = time.perf_counter() - t0
    if create_inside:
        op.close()
    assert np.all(status == 0), status
    return dt, n_iter


def main(names, quick):
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# {torch.cuda.get_device_name(0)}, {cus} CUs; successive approximation from 800 to tol {TOL:g}; "
          f"three repetitions, min / median / max; the routes alternate in one process")
    reps = 1 if quick else 3
    for name in names:
        kind, shapes = SHAPES[name]
        N = int(np.prod(shapes))
        disc = S.discretize_ssy if kind == "ssy" else S.discretize_gcy
        nloop = 4 if quick else 12                        # members of the looped route (>= 0.5 s of timed work)
        lmodels = [package_model(S, kind, member(kind, b)) for b in range(nloop)]
        ops = [S.KoopmansOperator(kind, shapes, m.params, disc(m, shapes)) for m in lmodels]
        wl = torch.empty((nloop,) + shapes, dtype=torch.float64, device=dev)
        sizes = [1, 8, 256] if quick else [1, 8, 64, 256, 1024]
        batches = {}
        for B in sizes:
            models = [package_model(S, kind, member(kind, b)) for b in range(B)]
            batches[B] = (models, S.BatchOperator.from_models(models, shapes), torch.empty((B,) + shapes, dtype=torch.float64, device=dev))
        print(f"\n{kind.upper()} {shapes}  N = {N}")
        print("  " + batches[sizes[-1]][1].describe_plan().replace("\n", "\n  ").rstrip())
        loop_route(kind, shapes, lmodels, wl, False, ops)                      # warm-up of both routes
        for B in sizes:
            batch_route(kind, shapes, batches[B][0], batches[B][2], False, batches[B][1])
        t_out, t_in, t_b, t_bi, its_b = [], [], {B: [] for B in sizes}, {B: [] for B in sizes}, {}
        its_loop = 0
        for _ in range(reps):
            t, its_loop = loop_route(kind, shapes, lmodels, wl, False, ops)
            t_out.append(t)
            for B in sizes:
                t, its_b[B] = batch_route(kind, shapes, batches[B][0], batches[B][2], False, batches[B][1])
                t_b[B].append(t)
            t, _ = loop_route(kind, shapes, lmodels, wl, True)
            t_in.append(t)
            for B in sizes:
                if B <= 256:
                    t, _ = batch_route(kind, shapes, batches[B][0], batches[B][2], True)
                    t_bi[B].append(t)
        pps_loop = nloop / float(np.median(t_out))
        pps_loop_in = nloop / float(np.median(t_in))
        print(f"  loop, {nloop} members, creation outside: {stats(t_out)}  {1e6 * np.median(t_out) / its_loop:7.2f} us/iteration  "
              f"{pps_loop:8.2f} problems/s")
        print(f"  loop, {nloop} members, creation inside : {stats(t_in)}  {pps_loop_in:8.2f} problems/s")
        for B in sizes:
            med = float(np.median(t_b[B]))
            rounds = (B + cus - 1) // cus
            us_it = 1e6 * med / (int(its_b[B].max()) * rounds)
            line = (f"  batch B = {B:4d}, creation outside: {stats(t_b[B])}  {us_it:7.2f} us/iteration/problem  "
                    f"{B / med:9.1f} problems/s  = {B / med / pps_loop:7.1f} x loop")
            if t_bi[B]:
                line += f"   | creation inside: {float(np.median(t_bi[B])):8.4f} s = {B / float(np.median(t_bi[B])) / pps_loop_in:7.1f} x loop"
            print(line)
        # break-even: the smallest B whose batch is faster than B looped solves
        t1 = float(np.median(t_b[sizes[0]]))
        per = float(np.median(t_out)) / nloop
        be = next((B for B in sizes if float(np.median(t_b[B])) < B * per), None)
        print(f"  break-even: one looped solve {per:.4f} s, a batch of 1 {t1:.4f} s -> the batch is ahead from B = "
              f"{be if be is not None else 'beyond ' + str(sizes[-1])} (of the sizes measured; estimate B > {t1 / per:.1f})")
        for T in ops:
            T.close()
        for B in sizes:
            batches[B][1].close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(args or list(SHAPES), "--quick" in sys.argv)

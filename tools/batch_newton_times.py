"""
Throughput of the batched Newton-Krylov solve (csrc/batch_newton.hpp) against the batched successive approximation and
against the single-problem device Newton looped over the same members (-> profiles/batch_newton_times.txt).

Per shape, one process, the three routes alternating, a warm-up of each first, three repetitions (min / median / max):
  (a) newton  BatchOperator.solve_dev(algorithm="newton", tol 1e-7, inner rtol 1e-5, atol 0) at B = 1, 8, 64, 256, 1024;
  (b) sa      BatchOperator.solve_dev(tol 1e-6), the call tools/batch_times.py times, on the same handle;
  (c) loop    KoopmansOperator.solve_dev("newton", same options) member after member, handles created outside the
              timed region (12 members).
Per row: seconds per batch, problems per second, microseconds per application (T or J.v) per problem (B <= CUs: wall /
most applications of a member, i.e. what one workgroup takes), Newton steps and applications per member, and the
ratios (a)/(b) and (a)/(c) of problems per second.
R is the ratio of application counts, sum of SA iterations / sum of (J.v + T applications of Newton): from the oracle
(oracle/solvers.py, on the CPU) for the first 12 members, cached in profiles/batch_newton_oracle_counts.json, and from
the device's own counts for all B members of a row.
Members are the fixed family of tests/batch_family.py.

    python tools/batch_newton_times.py [--quick] [ssy5 ssy10 ssy11 gcy5]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from batch_family import member, oracle_solve, package_model         # noqa: E402
from batch_newton_family import oracle_newton                        # noqa: E402

SHAPES = {"ssy5": ("ssy", (5,) * 4), "ssy10": ("ssy", (10,) * 4), "ssy11": ("ssy", (11,) * 4), "gcy5": ("gcy", (5,) * 6)}
SA_TOL = 1e-6
NEWTON = dict(tol=1e-7, inner_rtol=1e-5, inner_atol=0.0)
NLOOP = 12
CACHE = os.path.join(ROOT, "profiles", "batch_newton_oracle_counts.json")


def oracle_counts(name, members):
    """{"sa": [...], "newton_steps": [...], "newton_jv": [...]} of the first `members` members on the oracle; cached."""
    cache = {}
    if os.path.exists(CACHE):
        with open(CACHE) as f:
            cache = json.load(f)
    have = cache.get(name, {"sa": [], "newton_steps": [], "newton_jv": []})
    if len(have["sa"]) < members:
        kind, shapes = SHAPES[name]
        for b in range(len(have["sa"]), members):
            have["sa"].append(int(oracle_solve(kind, shapes, member(kind, b), SA_TOL)[1]))
            _, n, _, nmv, _ = oracle_newton(kind, shapes, b, NEWTON["tol"], NEWTON["inner_rtol"], NEWTON["inner_atol"], polish=False)
            have["newton_steps"].append(int(n))
            have["newton_jv"].append(int(nmv))
        cache[name] = have
        with open(CACHE, "w") as f:
            f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(cache[k], sort_keys=True)}' for k in sorted(cache)) + "\n}\n")
    return {k: v[:members] for k, v in have.items()}


def stats(ts):
    return f"{min(ts):8.4f} / {float(np.median(ts)):8.4f} / {max(ts):8.4f} s"


def main(names, quick):
    import torch
    import sdfs_via_autodiff_amd as S
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# {torch.cuda.get_device_name(0)}, {cus} CUs; from 800; (a) batch Newton tol {NEWTON['tol']:g}, inner rtol "
          f"{NEWTON['inner_rtol']:g}, atol {NEWTON['inner_atol']:g}; (b) batch SA tol {SA_TOL:g}; (c) single-problem device Newton, "
          f"looped; three repetitions, min / median / max; the routes alternate in one process")
    reps = 1 if quick else 3
    sizes = [1, 8, 256] if quick else [1, 8, 64, 256, 1024]

    def newton_route(op, w):
        w.fill_(800.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_iter, err, status, n_apply = op.solve_dev(w.data_ptr(), algorithm="newton", **NEWTON)
        dt = time.perf_counter() - t0
        assert np.all(status == 0), status
        return dt, n_iter, n_apply

    def sa_route(op, w):
        w.fill_(800.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_iter, err, status = op.solve_dev(w.data_ptr(), tol=SA_TOL)
        dt = time.perf_counter() - t0
        assert np.all(status == 0), status
        return dt, n_iter

    def loop_route(ops, w):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        apps = 0
        for b, T in enumerate(ops):
            w[b].fill_(800.0)
            torch.cuda.synchronize()
            n, info = T.solve_dev(w[b].data_ptr(), "newton", **NEWTON)
            apps += info["n_apply"]
        return time.perf_counter() - t0, apps

    for name in names:
        kind, shapes = SHAPES[name]
        N = int(np.prod(shapes))
        oc = oracle_counts(name, NLOOP)
        R12 = sum(oc["sa"]) / (sum(oc["newton_jv"]) + sum(oc["newton_steps"]))
        disc = S.discretize_ssy if kind == "ssy" else S.discretize_gcy
        lmodels = [package_model(S, kind, member(kind, b)) for b in range(NLOOP)]
        ops = [S.KoopmansOperator(kind, shapes, m.params, disc(m, shapes)) for m in lmodels]
        wl = torch.empty((NLOOP,) + shapes, dtype=torch.float64, device=dev)
        batches = {}
        for B in sizes:
            models = [package_model(S, kind, member(kind, b)) for b in range(B)]
            batches[B] = (S.BatchOperator.from_models(models, shapes), torch.empty((B,) + shapes, dtype=torch.float64, device=dev))
        print(f"\n{kind.upper()} {shapes}  N = {N}")
        print("  " + batches[sizes[-1]][0].describe_plan().replace("\n", "\n  ").rstrip())
        print(f"  oracle, members 0-{NLOOP - 1}: SA iterations {sum(oc['sa'])}, Newton steps {sum(oc['newton_steps'])} + J.v "
              f"{sum(oc['newton_jv'])}  ->  R = {R12:.2f}")
        loop_route(ops, wl)                                                       # warm-up of the three routes
        for B in sizes:
            newton_route(*batches[B])
            sa_route(*batches[B])
        t_c, t_a, t_b = [], {B: [] for B in sizes}, {B: [] for B in sizes}
        cnt = {}
        for _ in range(reps):
            t, apps_c = loop_route(ops, wl)
            t_c.append(t)
            for B in sizes:
                t, n_iter, n_apply = newton_route(*batches[B])
                t_a[B].append(t)
                t, n_sa = sa_route(*batches[B])
                t_b[B].append(t)
                cnt[B] = (n_iter, n_apply, n_sa)
        pps_c = NLOOP / float(np.median(t_c))
        print(f"  (c) loop, {NLOOP} members: {stats(t_c)}  {pps_c:9.1f} problems/s  {1e6 * np.median(t_c) / apps_c:7.2f} us/application")
        for B in sizes:
            n_iter, n_apply, n_sa = cnt[B]
            ma, mb = float(np.median(t_a[B])), float(np.median(t_b[B]))
            rounds = (B + cus - 1) // cus
            Rdev = float(n_sa.sum()) / float(n_apply.sum())
            print(f"  B = {B:4d}  (a) newton {stats(t_a[B])}  {B / ma:9.1f} problems/s  {1e6 * ma / (int(n_apply.max()) * rounds):7.2f} us/application/problem  "
                  f"steps {n_iter.mean():.2f}  J.v {(n_apply - n_iter).mean():.1f} per member")
            print(f"            (b) sa     {stats(t_b[B])}  {B / mb:9.1f} problems/s  {1e6 * mb / (int(n_sa.max()) * rounds):7.2f} us/iteration/problem  "
                  f"iterations {n_sa.mean():.0f} per member")
            print(f"            (a)/(b) = {mb / ma:7.2f}   (a)/(c) = {B / ma / pps_c:7.2f}   R (device counts, {B} members) = {Rdev:.2f}, R / 4 = {Rdev / 4:.2f}; "
                  f"R (oracle, 12 members) / 4 = {R12 / 4:.2f}")
        for T in ops:
            T.close()
        for B in sizes:
            batches[B][0].close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--oracle-only" in sys.argv:                       # fill the cache of the oracle's counts on the CPU
        for nm in args or list(SHAPES):
            c = oracle_counts(nm, NLOOP)
            print(nm, c)
    else:
        main(args or list(SHAPES), "--quick" in sys.argv)

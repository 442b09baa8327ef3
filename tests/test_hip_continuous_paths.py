"""
GPU tests of the continuous-state operator (csrc/cont_kernel.hpp) on each of its three gather paths, against the numpy
oracle (oracle/continuous.py):

  1  pre-contracted tensor path   box of next states in LDS, the two fastest dimensions interpolated once into U
  2  staged path                  box in LDS, full 2^D-corner fold with 32-bit offsets (Monte Carlo, or U does not fit)
  3  global-gather path           box larger than 4000 doubles: corners from global memory through long long strides

tests/cont_boxes.py restates the rule that selects the path and holds the case table (class A = every block on path 1,
B = every block on path 2, C = staged and unstaged blocks in one launch, D = no block staged);
tests/test_cont_boxes_cpu.py pins the table without a GPU.  Here every operator that is built first shows, through
describe_plan(), the cap / ucap / tq and dynamic LDS bytes the restatement predicts: that is what proves a case ran the
path its name claims.

Bounds.  One application of T: rtol 1e-12 elementwise (a-priori (M + O(D)) 2^-53 for M positive terms, 4.6e-13 at
M = 4096).  J.v: |got - want| <= 1e-11 J|v| elementwise, J|v| the oracle's product with |v| (every term of the sum is
positive, so this is the sum of the terms' magnitudes; worst-case summation bound (M + 2^D) 2^-53 <= 4.6e-13).  Path
against path on the same mathematics: 1e-13.  lin_interp: rtol 1e-14.

Every case prints its measured error / bound under pytest -s (lines "CONT-PATHS-MEASURED"); the figures measured on
an MI355X are in profiles/continuous_paths_errors.txt (largest: T 5.3e-15, J.v 5.6e-14 of J|v|, SA iterates 5.2e-15,
permuted nodes 9.4e-16, zero-weight node 0 exactly, lin_interp 1.1e-15; staged and unstaged blocks alike).

The oracle is a Python loop over grid points (seconds to tens of seconds per application at these sizes), so its
results are computed once per module, in worker processes that never touch the GPU.
"""
import concurrent.futures as cf
import multiprocessing as mp
import os
import re
import signal
import time

import numpy as np
import pytest

import cont_boxes as cb

pytestmark = pytest.mark.gpu

RTOL = 1e-12          # one application of T, as tests/test_hip_continuous.py
JTOL = 1e-11          # J.v against J|v|
PATH_TOL = 1e-13      # one path against another, same mathematics

# one case of each class for the device SA loop (three oracle applications each), the cheapest of its class
SA_CASES = ["A-ssy-headline", "B-ssy-refused", "C-gcy-mc", "D-ssy"]
NEWTON_CASES = ["C-gcy-mc", "D-ssy"]
T_START = time.time()


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


@pytest.fixture(autouse=True)
def time_limit():
    def expire(signum, frame):
        raise TimeoutError("test exceeded its 600 s limit")
    old = signal.signal(signal.SIGALRM, expire)
    signal.alarm(600)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


class OracleCache:
    """Oracle results per (case, quantity), each computed once: submitted to worker processes when the module starts
    (largest first) and collected by the test that needs them."""

    def __init__(self):
        workers = max(1, min(8, (os.cpu_count() or 2) - 1))
        self.pool = cf.ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn"))
        cost = {c[0]: int(np.prod(c[2])) * (c[4][1] ** len(c[2]) if c[4][0] == "gh" else c[4][1]) for c in cb.CASES}
        jobs = []
        for name in cb.CASE_IDS:
            k = 3 if name in SA_CASES else 1
            jobs += [(k * cost[name], name, "T", k), (2 * cost[name], name, "jv", 1), (2 * cost[name], name, "jabs", 1)]
        self.fut = {(name, what): self.pool.submit(cb.oracle_task, name, what, k)
                    for _, name, what, k in sorted(jobs, reverse=True)}

    def get(self, name, what):
        return self.fut[(name, what)].result()

    def close(self):
        self.pool.shutdown(wait=True, cancel_futures=True)


@pytest.fixture(scope="module")
def oracle():
    cache = OracleCache()
    yield cache
    cache.close()
    print(f"\nCONT-PATHS-MEASURED module wall time: {time.time() - T_START:.1f} s")


def report(what, value, bound):
    print(f"\nCONT-PATHS-MEASURED {what}: {value:.3e} = {value / bound:.4f} of the bound {bound:g}")


PLAN_RE = re.compile(r"cap (\d+), ucap (\d+), tq (\d+), dynamic LDS (\d+) B \(T\) / (\d+) B \(J\.v\)")


def plan_numbers(T):
    line = [ln for ln in T.describe_plan().splitlines() if ln.startswith("continuous operator:")]
    assert len(line) == 1, T.describe_plan()
    m = PLAN_RE.search(line[0])
    assert m, line[0]
    return dict(zip(("cap", "ucap", "tq", "lds_T", "lds_jvp"), map(int, m.groups())))


def build(S, model, params, grids, nodes, weights, expect_cls=None):
    """The operator and the restatement's verdict on it; describe_plan() must agree with the restatement."""
    r = cb.classify(model, params, grids, nodes)
    T = S.ContinuousOperator(np.array(params), grids, nodes, weights)
    got = plan_numbers(T)
    assert got == {k: r[k] for k in got}, (got, r)
    assert got["lds_jvp"] <= 65536
    if expect_cls is not None:
        assert r["cls"] == expect_cls
    return T, r


def build_case(S, name):
    case = cb.CASES[cb.CASE_IDS.index(name)]
    T, r = build(S, *cb.make_case(case), expect_cls=case[5])
    assert (r["n_staged"], r["n_unstaged"]) == case[6:8]
    return T, r, case


def masks(r):
    """(label, mask) over which errors are reported: staged and unstaged blocks apart in class C."""
    if r["cls"] != "C":
        return [("all blocks", np.ones_like(r["staged"]))]
    assert r["staged"].any() and (~r["staged"]).any()
    return [("staged blocks", r["staged"]), ("unstaged blocks", ~r["staged"])]


@pytest.mark.parametrize("name", cb.CASE_IDS)
def test_T_on_every_path_vs_oracle(S, oracle, name):
    T, r, case = build_case(S, name)
    w, _ = cb.case_inputs(name)
    got = T(w)
    resid = T.residual()
    want = oracle.get(name, "T")[0]
    rel = np.abs(got - want) / np.abs(want)
    for label, mask in masks(r):
        report(f"T {name} [{r['cls']}] {label} ({int(mask.sum())})", float(rel[mask].max()), RTOL)
    for label, mask in masks(r):
        assert rel[mask].max() <= RTOL, (name, label)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    assert resid == pytest.approx(np.max(np.abs(want - w)), rel=1e-12)
    T.close()


@pytest.mark.parametrize("name", cb.CASE_IDS)
def test_jvp_on_every_path_vs_oracle(S, oracle, name):
    T, r, case = build_case(S, name)
    w, v = cb.case_inputs(name)
    got = T.jvp(w, v)
    want, jabs = oracle.get(name, "jv"), oracle.get(name, "jabs")
    assert np.all(jabs > 0)
    ratio = np.abs(got - want) / jabs
    for label, mask in masks(r):
        report(f"J.v {name} [{r['cls']}] {label} ({int(mask.sum())})", float(ratio[mask].max()), JTOL)
    for label, mask in masks(r):
        assert ratio[mask].max() <= JTOL, (name, label)
    assert np.all(np.abs(got - want) <= JTOL * jabs)
    T.close()


@pytest.mark.parametrize("name", SA_CASES)
def test_device_sa_loop_on_every_path(S, oracle, name):
    """k device iterations against k oracle applications, and the error the loop reports for the last."""
    T, r, case = build_case(S, name)
    w, _ = cb.case_inputs(name)
    iterates = oracle.get(name, "T")
    assert len(iterates) == 3
    prev = w
    for k, x in zip((1, 2, 3), iterates):
        xk, n, info = T.solve(w, "successive_approx", tol=0.0, max_iter=k)
        assert n == k
        rel = float(np.max(np.abs(xk - x) / np.abs(x)))
        report(f"SA {name} [{r['cls']}] k = {k}", rel, 1e-11)
        assert rel <= 1e-11
        err = float(np.max(np.abs(x - prev)))
        assert abs(info["final_err"] - err) <= 1e-9 * err
        prev = x
    T.close()


@pytest.mark.parametrize("name", NEWTON_CASES)
def test_newton_krylov_fixed_point_is_the_oracles(S, name):
    """Newton-Krylov from a successive-approximation start (as test_gcy_continuous_solve_and_errors); the residual of
    the result is evaluated by the oracle's T, not the kernel's."""
    from oracle import continuous as OC
    T, r, case = build_case(S, name)
    model, params, grids, nodes, weights = cb.make_case(case)
    xs, ns, _ = T.solve(np.ones(T.shapes), "successive_approx", tol=1e-2, max_iter=50000)
    x, n, info = T.solve(xs, "newton", tol=1e-9, inner_rtol=1e-8, inner_atol=0.0)
    assert info["status"] == 0
    res = float(np.max(np.abs(OC.T_fun_factory(model, params, grids, nodes, weights)(x) - x)))
    report(f"Newton {name} [{r['cls']}] oracle residual after {ns} SA + {n} Newton steps", res, 1e-8)
    assert res < 1e-8 and np.all(x > 1)
    T.close()


# -- path against path ----------------------------------------------------------------------------------------------
def headline(S):
    case = cb.CASES[cb.CASE_IDS.index("A-ssy-headline")]
    model, params, grids, nodes, weights = cb.make_case(case)
    T, r = build(S, model, params, grids, nodes, weights, expect_cls="A")
    w, v = cb.case_inputs("A-ssy-headline")
    return model, params, grids, nodes, weights, T, w, v


def compare_paths(what, T_ref, T_alt, w, v):
    """T and J.v of two operators that state the same mathematics.  Relative tolerances need sums without
    cancellation: T's terms are positive, and J.v is compared for the positive direction |v| elementwise; for the
    signed direction the yardstick is J|v| (the sum of the term magnitudes), as against the oracle."""
    a, b = T_ref(w), T_alt(w)
    report(f"{what}: T", float(np.max(np.abs(a - b) / np.abs(a))), PATH_TOL)
    np.testing.assert_allclose(b, a, rtol=PATH_TOL, atol=0)
    ja, jb = T_ref.jvp(w, np.abs(v)), T_alt.jvp(w, np.abs(v))
    report(f"{what}: J|v|", float(np.max(np.abs(ja - jb) / np.abs(ja))), PATH_TOL)
    np.testing.assert_allclose(jb, ja, rtol=PATH_TOL, atol=0)
    sa, sb = T_ref.jvp(w, v), T_alt.jvp(w, v)
    report(f"{what}: J.v / J|v|", float(np.max(np.abs(sa - sb) / ja)), PATH_TOL)
    assert np.all(np.abs(sa - sb) <= PATH_TOL * ja)


def test_permuted_nodes_take_the_staged_path_and_agree(S):
    """Path 2 against path 1: the same rule with its node columns permuted is no tensor rule in gridmake order, so the
    host keeps tq = 0 and every node does the full fold."""
    model, params, grids, nodes, weights, T, w, v = headline(S)
    perm = np.random.default_rng(7).permutation(nodes.shape[1])
    assert np.any(perm != np.arange(perm.size))
    Tp, rp = build(S, model, params, grids, np.ascontiguousarray(nodes[:, perm]), weights[perm], expect_cls="B")
    assert plan_numbers(T)["tq"] == 5 and plan_numbers(Tp)["tq"] == 0
    assert plan_numbers(Tp)["cap"] == plan_numbers(T)["cap"]
    compare_paths("permuted nodes (path 2) vs tensor rule (path 1)", T, Tp, w, v)
    T.close(); Tp.close()


def test_zero_weight_far_node_takes_the_global_path_and_agrees(S):
    """Path 3 against path 1: one more node of weight 0 at eta = 1000 in every dimension makes every box the whole
    grid (20000 > 4000 doubles), so no block is staged; its term is 0 * pow(interpolant at the clipped corner), finite
    (the weight's factor exp(theta s_lambda eta_0) is exp(-6.4))."""
    model, params, grids, nodes, weights, T, w, v = headline(S)
    nodes0 = np.ascontiguousarray(np.concatenate([nodes, np.full((nodes.shape[0], 1), 1000.0)], axis=1))
    weights0 = np.concatenate([weights, [0.0]])
    T0, r0 = build(S, model, params, grids, nodes0, weights0, expect_cls="D")
    assert r0["vmax"] == 20000 and plan_numbers(T0) == dict(cap=4000, ucap=0, tq=0, lds_T=32000, lds_jvp=64000)
    compare_paths("zero-weight far node (path 3) vs tensor rule (path 1)", T, T0, w, v)
    T.close(); T0.close()


# -- edges of the node loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 37, 256, 257])
def test_monte_carlo_node_counts_at_the_wave_edges(S, M):
    """pow_fast_n runs on whole waves: one valid lane in all (M = 1), part of a wave, exactly one trip of 256, and one
    valid lane in the second trip."""
    from oracle import continuous as OC
    from oracle import models as OM
    params = OM.ssy_params()
    grids = OC.build_grid_ssy(params, (5, 4, 6, 7))
    rng = np.random.default_rng(1000 + M)
    draws = rng.standard_normal((4, M))
    T, r = build(S, "ssy", params, grids, draws, None, expect_cls="B")
    assert plan_numbers(T)["tq"] == 0
    w = 300 + 600 * rng.random((5, 4, 6, 7))
    v = rng.standard_normal((5, 4, 6, 7))
    got, want = T(w), OC.T_fun_factory("ssy", params, grids, draws)(w)
    report(f"T Monte Carlo M = {M}", float(np.max(np.abs(got - want) / want)), RTOL)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    J = OC.jvp_factory("ssy", params, grids, draws)
    ratio = float(np.max(np.abs(T.jvp(w, v) - J(w, v)) / J(w, np.abs(v))))
    report(f"J.v Monte Carlo M = {M}", ratio, JTOL)
    assert ratio <= JTOL
    T.close()


# -- lin_interp_kernel --------------------------------------------------------------------------------------------------
def uniform_grids(rng, shape):
    return tuple(np.linspace(lo, lo + width, n) for n, lo, width in
                 zip(shape, rng.uniform(-2, 1, len(shape)), rng.uniform(0.5, 3, len(shape))))


def check_lin_interp(S, what, grids, f, x):
    from oracle import continuous as OC
    got = np.atleast_1d(S.lin_interp(x, f, grids))
    want = OC.lin_interp(x, f, grids)
    assert got.shape == want.shape == (x.shape[1],)
    report(f"lin_interp {what}", float(np.max(np.abs(got - want) / np.abs(want))), 1e-14)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)


LI_SHAPES = {"4-D": (5, 4, 6, 7), "4-D, two extents of 2": (2, 5, 2, 7), "6-D": (3, 2, 4, 2, 3, 5)}


@pytest.mark.parametrize("nq", [1, 255, 256, 257, 10001])
@pytest.mark.parametrize("kind", list(LI_SHAPES))
def test_lin_interp_query_counts_and_grids(S, kind, nq):
    """Block edges of the 256-thread launch, a grid with extents of exactly 2, six dimensions; the queries reach a
    third of the range beyond both ends of every grid, so clipped and interior coordinates mix."""
    shape = LI_SHAPES[kind]
    rng = np.random.default_rng(nq + len(shape))
    grids = uniform_grids(rng, shape)
    f = 1.0 + rng.random(shape)
    x = np.stack([g[0] + (g[-1] - g[0]) * rng.uniform(-1 / 3, 4 / 3, nq) for g in grids])
    check_lin_interp(S, f"{kind}, nq = {nq}", grids, f, x)


@pytest.mark.parametrize("kind", list(LI_SHAPES))
def test_lin_interp_every_coordinate_clipped(S, kind):
    """Queries far outside on either side in every dimension (all 2^D corners of the sign pattern): the result is the
    value at the matching corner of the grid."""
    shape = LI_SHAPES[kind]
    D = len(shape)
    rng = np.random.default_rng(40 + D)
    grids = uniform_grids(rng, shape)
    f = 1.0 + rng.random(shape)
    signs = np.array([[(c >> d) & 1 for c in range(2 ** D)] for d in range(D)])          # (D, 2^D)
    for far in (1.0, 1e6):
        x = np.stack([np.where(signs[d] == 1, g[-1] + far * (g[-1] - g[0]), g[0] - far * (g[-1] - g[0]))
                      for d, g in enumerate(grids)])
        check_lin_interp(S, f"{kind}, all clipped, {far:g} ranges outside", grids, f, x)
        corners = f[tuple(np.where(signs[d] == 1, shape[d] - 1, 0) for d in range(D))]
        np.testing.assert_allclose(np.atleast_1d(S.lin_interp(x, f, grids)), corners, rtol=1e-14, atol=0)

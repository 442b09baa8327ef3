"""
The long-double twin of the device-resident Anderson loop (tests/anderson_twin.py), without a GPU:
  * pinned to the oracle's jaxopt semantics (oracle.solvers.anderson_solver) on a problem where no step is rejected;
  * the caps that keep the step test's tolerance (tests/test_hip_anderson_steps.py) from hiding a failure, for every case
    of its table: the tolerance comes from the twin's own sensitivity, so a schedule on which the twin itself is
    ill-conditioned would make the GPU test vacuous.  Such a case is re-drawn (another seed in CASE_SEEDS), not loosened.
"""
import numpy as np
import pytest

import anderson_twin as AT
from oracle import solvers as osol


@pytest.mark.parametrize("m,mf,tol", [(3, 2, 1e-4), (10, 4, 1e-9)])
def test_twin_follows_the_oracle_loop(m, mf, tol):
    """Diagonal affine contraction x -> a x + b, n = 40, from a start 1e-2 off the fixed point (Gram entries ~ 1e-3 against
    the ridge of 1e-6: the fp64 solve of the oracle and the long-double solve of the twin then agree far below 1e-10).
    Same pass count, every iterate within 1e-10 relative.  (m = 3 mixing every second pass with beta = 8 stalls near 1e-4
    once the ridge outweighs the Gram matrix -- the coefficients go to 1 / m --, hence its tol.)"""
    n = 40
    rng = np.random.default_rng(3)
    a = 0.3 + 0.6 * rng.random(n)
    b = 100.0 + 50.0 * rng.random(n)
    f = lambda x: a * x + b                                             # noqa: E731
    x0 = b / (1 - a) + 1e-2 * rng.random(n)
    seen = []

    def f_rec(x):
        seen.append(np.array(x, dtype=np.float64))
        return f(x)

    xo, n_o = osol.anderson_solver(f_rec, x0, tol=tol, max_iter=500, verbose=False, history_size=m, mixing_frequency=mf,
                                   beta=AT.BETA, ridge=1e-6)
    seen.append(np.asarray(xo))
    tw = AT.AndersonTwin(n, m, tol, 500, AT.BETA, 1e-6, mf)
    x = x0.copy()
    iterates = [x.copy()]
    i = 0
    mixed = 0
    while True:
        fx = f(x)
        if tw.push(i, x, fx) is None:
            break
        s = tw.step(i)
        assert s["mode"] in (0, 1)                                      # no rejection on this problem
        mixed += s["mode"]
        x = fx if s["x"] is None else np.asarray(s["x"], dtype=np.float64)
        iterates.append(x.copy())
        i += 1
    assert n_o < 500 and tw.it == n_o and tw.status == 0 and tw.rejected == 0, (tw.it, n_o)
    assert n_o >= m + 2 * mf and mixed >= 2, (n_o, mixed)               # the comparison covers mixing steps
    assert len(iterates) == len(seen)
    worst = max(float(np.max(np.abs(u - v) / np.abs(v))) for u, v in zip(iterates, seen))
    print(f"m={m} f={mf}: {n_o} passes, {mixed} mixing steps, worst relative difference {worst:.3e}")
    assert worst <= 1e-10, worst


def test_pair_layout_has_the_capacity_as_stride():
    idx = [AT.pair_index(i, j) for i in range(AT.LAZY_M) for j in range(i, AT.LAZY_M)]
    assert idx == list(range(AT.NPAIRS)) and AT.NPAIRS == 78
    assert AT.pair_index(1, 1) == 12 and AT.pair_index(2, 5) == 26       # (m-strided at m = 3 would say 3 and 8)


def test_gram_depth():
    assert AT.gram_depth(13, AT.SWEEP_BLOCKS) == 66 and AT.gram_depth(262144, AT.SWEEP_BLOCKS) == 66
    assert AT.gram_depth(262657, AT.SWEEP_BLOCKS) == 68 and AT.gram_depth(1049091, AT.SWEEP_BLOCKS) == 74
    assert AT.gram_depth(1048576, AT.PUSH_BLOCKS) == 66 and AT.gram_depth(1049091, AT.PUSH_BLOCKS) == 68


@pytest.mark.parametrize("case", AT.table_cases(), ids=AT.case_id)
def test_caps_on_the_mix_tolerance(case):
    """Where n >= m + 1 the tolerance of every mixing step must stay below 1e-12 max|x|, where n <= m (rank-deficient Gram
    matrix, held up by the ridge alone) below 1e-8 max|x|."""
    n, m, mf, ridge = case
    cap = AT.CAP_FULL if n >= m + 1 else AT.CAP_DEFICIENT
    assert ridge >= 0 or n >= m + 1                                      # the relative ridge only on full-rank cases
    tw, ratios = AT.run_on_twin(n, m, mf, ridge, AT.CASE_SEEDS.get(case, 0))
    assert tw.it == AT.n_passes(m, mf) and tw.rejected == 0 and tw.status == 0
    assert len(ratios) >= 2, ratios                                      # the schedule reaches the solve more than once
    print(f"{AT.case_id(case)}: {len(ratios)} mixing steps, worst tolerance {max(ratios):.3e} max|x| (cap {cap:g})")
    assert max(ratios) <= cap, (max(ratios), cap)


@pytest.mark.parametrize("name", sorted(AT.CONTROL_CASES))
def test_control_cases_end_where_they_should(name):
    """The control schedules on the twin alone: each ends on the pass and in the branch it is there for, inside the cap."""
    c = AT.CONTROL_CASES[name]
    tw, ratios = AT.run_on_twin(c["n"], c["m"], c["mf"], 1e-6, 0, passes=c["passes"], tol=c["tol"], max_iter=c["max_iter"],
                                nan_at=c.get("nan_at"))
    assert tw.it == c["ends_at"], (tw.it, c)
    assert tw.last_mixed == c["ends_mixed"], (tw.last_mixed, c)
    assert tw.rejected == c.get("rejected", 0) and tw.status == c.get("status", 0), (tw.state(), c)
    if c["ends_at"] > c["m"]:
        assert ratios and max(ratios) <= AT.CAP_FULL, ratios

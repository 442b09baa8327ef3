"""
The analysis table: what the analysis entry points at w* launch and compute on the smallest grids -- ``sdf_moments``,
``term_structure``, ``claim_prices``, ``wc_ratio_sensitivities``, ``wc_ratio_gradient`` and ``simulate`` on the discretised
operator, their ``*_continuous`` twins on the continuous-state one.  Per call: the operator's counter table (names,
launches, bytes and flops, profiling on) and the SHA-256 of every array or number in the result (profiling off).
Every call is recorded on an operator of its own: a handle keeps the counter names it has met (at most MAX_NAMES, any
further name is counted in the last slot), so a table read from a handle that served other calls would depend on them.
tools/analysis_table.py records it into tests/golden/analysis_table.json, tests/test_hip_analysis_table.py recomputes it
and requires equality.

No solve runs here: the discrete cases take w* from the committed successive-approximation fixtures, the continuous ones
from tests/golden/cont_sim_wstar.npz, so no hash inherits a solver's bits.  The (grid, κ) pairs of the continuous claims
are those of ``cont_pricing_oracle.claim_pairs()``, which tests/test_cont_pricing_cpu.py holds to r(K) < 1.
"""
import os

import numpy as np

import cont_pricing_oracle as cp
import cont_sim_cases as CC
from launch_table import GOLD, counter_table, sha

FIXTURE = os.path.join(GOLD, "analysis_table.json")

N_MAX, SAVE = 24, (7,)
PATHS, PERIODS, SEED = 64, 8, 20240229
WRT = ("β", "ρ_z")                            # (a preference parameter and a persistence)
KAPPAS = (0.0, 1.0, 2.0)
MAX_NAMES = 16                                # SDFS_MAX_KERNELS of include/sdfs_hip.h

# name -> (model, shapes, fixture, key of w*)
DISCRETE = {
    "ssy 2x3x4x5": ("ssy", (2, 3, 4, 5), "sa_ssy_2x3x4x5.npz", "w_1e8"),
    "gcy 3x3x3x3x3x3": ("gcy", (3, 3, 3, 3, 3, 3), "sa_gcy_3x3x3x3x3x3.npz", "w_1e7"),
}
# name -> grid of cont_sim_cases.GRIDS (Gauss–Hermite rule of order cont_sim_cases.QUAD_D)
CONTINUOUS = {
    "continuous ssy 2x3x4x5 sd1.0": ("ssy", (2, 3, 4, 5), 1.0),
    "continuous gcy 2x3x2x3x4x3 sd1.0": ("gcy", (2, 3, 2, 3, 4, 3), 1.0),
}
CASES = list(DISCRETE) + list(CONTINUOUS)
# the calls whose every output is reproducible bit for bit: tilted applications and the horizon loop have no atomics and
# reduce in a fixed order (csrc/price_kernels.hpp, csrc/cont_price.hpp)
EXACT = ("sdf_moments", "term_structure")


def continuous_kappas(name):
    return sorted(k for g, k in cp.claim_pairs() if g == CONTINUOUS[name])


def calls_of(name):
    """The names of the calls recorded for one case."""
    if name in DISCRETE:
        return (["sdf_moments"] + ["term_structure kappa=%g" % k for k in (0.0, 1.0)] +
                ["claim_prices kappa=%g" % k for k in KAPPAS] +
                ["wc_ratio_sensitivities", "wc_ratio_gradient", "simulate"])
    return (["sdf_moments_continuous"] + ["term_structure_continuous kappa=%g" % k for k in (0.0, 1.0)] +
            ["claim_prices_continuous kappa=%g" % k for k in continuous_kappas(name)] +
            ["wc_ratio_sensitivities_continuous", "simulate_continuous"])


ALL = [(name, call) for name in CASES for call in calls_of(name)]
_SETUP = {}


def setup(S, name):
    """(model, shapes or grids, w*) of a case, read once."""
    if name not in _SETUP:
        if name in DISCRETE:
            kind, shapes, fixture, key = DISCRETE[name]
            _SETUP[name] = (S.SSY() if kind == "ssy" else S.GCY(), shapes, np.load(os.path.join(GOLD, fixture))[key])
        else:
            kind, sizes, sd = CONTINUOUS[name]
            _SETUP[name] = (S.SSY() if kind == "ssy" else S.GCY(), CC.grids_of(kind, sizes, sd),
                            CC.golden_wstar(kind, sizes, sd))
    return _SETUP[name]


def fresh_operator(S, name):
    """A new operator for one call: the discretised one as the analysis functions find it in their cache (emptied
    first), the continuous one with the Gauss–Hermite rule of the cases."""
    m, grid, _ = setup(S, name)
    if name in DISCRETE:
        from sdfs_via_autodiff_amd import _requests
        _requests._ops.clear()
        return _requests._operator(m, grid)[0]
    nodes, weights = S.qnwnorm([CC.QUAD_D] * len(grid))
    return S.ContinuousOperator(np.array(m.params), grid, np.ascontiguousarray(nodes.T), weights)


def thunk(S, name, call, op):
    """The call as a function of no arguments (``op``: the operator a continuous call runs on)."""
    m, grid, w = setup(S, name)
    fn, _, arg = call.partition(" kappa=")
    kappa = float(arg) if arg else None
    if name in DISCRETE:
        if fn == "sdf_moments":
            return lambda: S.sdf_moments(m, grid, w)
        if fn == "term_structure":
            return lambda: S.term_structure(m, grid, w, N_MAX, kappa=kappa, save=SAVE)
        if fn == "claim_prices":
            return lambda: S.claim_prices(m, grid, w, kappa)
        if fn == "wc_ratio_sensitivities":
            return lambda: S.wc_ratio_sensitivities(m, grid, w, wrt=WRT, persistence=True)
        if fn == "wc_ratio_gradient":
            g = np.random.default_rng(7).random(grid)
            return lambda: S.wc_ratio_gradient(m, grid, w, g)
        if fn == "simulate":
            return lambda: S.simulate(m, grid, w, PATHS, PERIODS, seed=SEED, return_paths=True)
    else:
        if fn == "sdf_moments_continuous":
            return lambda: S.sdf_moments_continuous(m, grid, w, operator=op)
        if fn == "term_structure_continuous":
            states = np.stack([np.zeros(len(grid)), CC.start_of(grid, "vector")])
            return lambda: S.term_structure_continuous(m, grid, w, N_MAX, kappa, states=states, save=SAVE, operator=op)
        if fn == "claim_prices_continuous":
            return lambda: S.claim_prices_continuous(m, grid, w, kappa, operator=op)
        if fn == "wc_ratio_sensitivities_continuous":
            return lambda: S.wc_ratio_sensitivities_continuous(m, grid, w, wrt=WRT, operator=op)
        if fn == "simulate_continuous":
            return lambda: S.simulate_continuous(m, grid, w, PATHS, PERIODS, seed=SEED, operator=op, return_paths=True)
    raise KeyError((name, call))


def leaves(x, prefix=""):
    """(path, float64 array) of every array or number in a result; tuples of names are left out."""
    if isinstance(x, dict):
        for k, v in x.items():
            yield from leaves(v, f"{prefix}/{k}" if prefix else str(k))
    elif not (isinstance(x, (tuple, list)) and x and isinstance(x[0], str)):
        yield prefix, np.asarray(x, dtype=np.float64)


def record_call(S, name, call):
    """Counter table of the call with profiling on; the hashes of its result with it off."""
    op = fresh_operator(S, name)
    run = thunk(S, name, call, op)
    op.set_profiling(True)
    op.reset_counters()
    try:
        run()
        op.synchronize()
        table = counter_table(op)
    finally:
        op.set_profiling(False)
    return dict(counters=table, hashes={k: sha(a) for k, a in leaves(run())})


def record_all(S):
    return {name: {call: record_call(S, name, call) for call in calls_of(name)} for name in CASES}

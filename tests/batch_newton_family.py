"""
Helper of tests/test_batch_newton_cpu.py and tests/test_hip_batch_newton.py (not a test module): the members of
batch_family.py as oracle operators with their analytic J.v, and cached oracle Newton solves.
"""
import functools

import numpy as np

from batch_family import member
from oracle import gcy as ogcy
from oracle import models as omodels
from oracle import solvers as osolvers
from oracle import ssy as ossy

# the cases of the GPU tests: (kind, shapes, members)
CASES = [("ssy", (5,) * 4, 12), ("gcy", (3,) * 6, 12), ("ssy", (10,) * 4, 3), ("ssy", (7, 13, 11, 9), 2),
         ("ssy", (11,) * 4, 2), ("gcy", (5,) * 6, 2), ("gcy", (3, 4, 5, 2, 3, 4), 3)]
TOL, INNER_RTOL = 1e-7, 1e-5


def oracle_ops(kind, shapes, over):
    """(T, jvp) of one member on the oracle."""
    shapes = tuple(shapes)
    if kind == "ssy":
        p = omodels.ssy_params(**over)
        arr = ossy.discretize_ssy(p, shapes)
        return (lambda w: ossy.T_ssy_factorised(w, shapes, p, arr)), (lambda w, v: ossy.jvp_ssy(w, v, shapes, p, arr))
    p = omodels.gcy_params(**over)
    arr = ogcy.discretize_gcy(p, shapes)
    return (lambda w: ogcy.T_gcy_factorised(w, shapes, p, arr)), (lambda w, v: ogcy.jvp_gcy(w, v, shapes, p, arr))


@functools.lru_cache(maxsize=None)
def _newton(kind, shapes, b, tol, rtol, atol, max_iter, polish):
    T, jvp = oracle_ops(kind, shapes, member(kind, b))
    errors, stats = [], {}
    with np.errstate(all="ignore"):
        w, n = osolvers.newton_solver(T, np.full(shapes, 800.0), tol=tol, max_iter=max_iter, bicgstab_atol=atol,
                                      verbose=False, jvp=jvp, bicgstab_tol=rtol, errors=errors, stats=stats)
        wstar = osolvers.newton_polish(T, jvp, w) if polish else None
    return w, n, np.array(errors), stats.get("matvecs", 0), wstar


def oracle_newton(kind, shapes, b, tol=TOL, rtol=INNER_RTOL, atol=0.0, max_iter=10**6, polish=True):
    """(w, Newton steps, error trace, J.v count, polished w*) of the oracle's Newton solve of member b from 800; cached
    per process."""
    return _newton(kind, tuple(shapes), int(b), float(tol), float(rtol), float(atol), int(max_iter), bool(polish))


def first_step_residual(kind, shapes, b, step):
    """|(J - I) step - g|_2 / |g|_2 at w = 800 on the oracle."""
    T, jvp = oracle_ops(kind, shapes, member(kind, b))
    w = np.full(shapes, 800.0)
    g = T(w) - w
    r = jvp(w, step) - step - g
    return float(np.linalg.norm(r.ravel()) / np.linalg.norm(g.ravel()))

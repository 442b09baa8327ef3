"""
Helper of tests/test_batch_cpu.py and tests/test_hip_batch.py (not a test module): the fixed parameter family of the
batched solve, its members as oracle operators and as package models, and cached oracle solves.
"""
import functools

import numpy as np

from oracle import gcy as ogcy
from oracle import models as omodels
from oracle import solvers as osolvers
from oracle import ssy as ossy

GREEK = {"gamma": "γ", "psi": "ψ", "beta": "β", "mu_c": "μ_c", "s_lam": "s_λ"}


def member(kind, b):
    """Overrides of the default calibration for member b (ASCII names, as oracle.models takes them)."""
    if kind == "ssy":
        return dict(gamma=7.89 + 0.45 * (b % 7), psi=1.97 - 0.06 * (b % 5), beta=0.999 - 0.0003 * (b % 3),
                    mu_c=0.0016 * (1 + 0.05 * (b % 4)), s_lam=0.0004 * (1 + 0.25 * (b % 2)))
    return dict(gamma=13.01 - 0.6 * (b % 7), psi=1.5 + 0.05 * (b % 5), beta=0.9987 - 0.0002 * (b % 3),
                mu_c=0.0016 * (1 + 0.05 * (b % 4)))


def package_model(S, kind, over):
    cls = S.SSY if kind == "ssy" else S.GCY
    return cls(**{GREEK[k]: v for k, v in over.items()})


def oracle_T(kind, shapes, over):
    shapes = tuple(shapes)
    if kind == "ssy":
        p = omodels.ssy_params(**over)
        arr = ossy.discretize_ssy(p, shapes)
        return lambda w: ossy.T_ssy_factorised(w, shapes, p, arr)
    p = omodels.gcy_params(**over)
    arr = ogcy.discretize_gcy(p, shapes)
    return lambda w: ogcy.T_gcy_factorised(w, shapes, p, arr)


def _freeze(over):
    return tuple(sorted(over.items()))


@functools.lru_cache(maxsize=None)
def _oracle_solve(kind, shapes, frozen, tol, max_iter):
    T = oracle_T(kind, shapes, dict(frozen))
    errors = []
    with np.errstate(all="ignore"):
        w, n = osolvers.successive_approx(T, np.full(shapes, 800.0), tol=tol, max_iter=max_iter, verbose=False,
                                          errors=errors)
    return w, n, np.array(errors)


def oracle_solve(kind, shapes, over, tol=1e-6, max_iter=10**6):
    """(w, n_iter, error trace) of the oracle's successive approximation from 800; cached per process."""
    return _oracle_solve(kind, tuple(shapes), _freeze(over), float(tol), int(max_iter))


def oracle_apply(kind, shapes, over, w, k):
    T = oracle_T(kind, shapes, over)
    with np.errstate(all="ignore"):
        for _ in range(k):
            w = T(w)
    return w


# the solves of the count test: (kind, shapes, members)
COUNT_CASES = [("ssy", (5, 5, 5, 5), 12), ("gcy", (3,) * 6, 12), ("ssy", (10, 10, 10, 10), 3)]

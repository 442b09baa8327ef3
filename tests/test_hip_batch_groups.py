"""
GPU test of the group loop of the batch host layer (csrc/batch_api.hpp, batch_run_groups): a batch whose Newton workspace
would pass the handle's cap runs group after group, workgroup i of a group on problem b0 + i in slot i of the workspace.
SDFS_BATCH_WS_MAX (bytes, read at sdfs_batch_create) lowers the cap from its 2 GiB so that exactly two problems fit a
group; the Newton solve, the gradients and the prices of such a handle must then carry the bits of the ungrouped run.

  (a) SSY 5^4, B = 5: the vectors live in registers; 7 x 626 x 8 = 35 056 B per problem, cap 70 112: groups of 2, 2, 1
  (b) SSY 10^4, B = 3: the vectors live in the workspace, so the slot index addresses live data; 560 000 B per
      problem, cap 1 120 000: groups of 2, 1
"""
import os

import numpy as np
import pytest

from batch_family import member, package_model

pytestmark = pytest.mark.gpu

VAR = "SDFS_BATCH_WS_MAX"
OPTS = dict(algorithm="newton", tol=1e-7, inner_rtol=1e-5, inner_atol=0.0)
GROUPED = "2 problems per group (the batch runs group after group)"
# (shapes, members, the placement describe_plan reports, bytes of workspace per problem)
CASES = [((5,) * 4, 5, "in registers", 7 * 626 * 8), ((10,) * 4, 3, "in global memory", 7 * 10000 * 8)]


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(S, models, shapes, g):
    """The three calls of the comparison: {field: array}."""
    out = {}
    for check_every in (8, 0):
        res = S.solve_batch(models, shapes, check_every=check_every, **OPTS)
        assert res.plan == "batch"
        for f in ("w", "n_iter", "n_apply", "error", "status"):
            out[f"newton[{check_every}].{f}"] = getattr(res, f)
    w = res.w
    gr = S.gradient_batch(models, shapes, w, g)
    for f in ("grad", "n_iter", "n_apply", "rel_resid", "resid_T", "status"):
        out[f"gradient.{f}"] = getattr(gr, f)
    pr = S.price_batch(models, shapes, w, kappa=2.0, n_max=3)
    for f in ("moments", "price", "yield_", "n_horizons", "n_iter", "n_apply", "rel_resid", "resid_T", "status"):
        out[f"price.{f}"] = getattr(pr, f)
    assert gr.plan == pr.plan == "batch"
    return out


@pytest.mark.parametrize("shapes,members,placement,per_problem", CASES)
def test_groups_carry_the_bits_of_one_group(S, monkeypatch, shapes, members, placement, per_problem):
    models = [package_model(S, "ssy", member("ssy", b)) for b in range(members)]
    g = np.random.default_rng(11).standard_normal(shapes)
    monkeypatch.delenv(VAR, raising=False)
    op = S.BatchOperator.from_models(models, shapes)
    plan = op.describe_plan()
    op.close()
    assert placement in plan and f"{members} problems per group;" in plan and "group after group" not in plan, plan
    one = run(S, models, shapes, g)
    for f in one:
        if f.endswith(".status"):
            assert np.all(one[f] == 0), (f, one[f])

    # the cap holds around the creation of a handle only, and every handle created below is a grouped one
    create = S.BatchOperator.__init__
    made = []

    def capped_create(self, *args, **kwargs):
        os.environ[VAR] = str(2 * per_problem)
        try:
            create(self, *args, **kwargs)
        finally:
            del os.environ[VAR]
        made.append(self.describe_plan())

    monkeypatch.setattr(S.BatchOperator, "__init__", capped_create)
    grouped = run(S, models, shapes, g)
    assert VAR not in os.environ
    monkeypatch.undo()
    assert len(made) == 4 and all(GROUPED in p and placement in p for p in made), made
    assert sorted(grouped) == sorted(one)
    for f in one:
        assert same_bits(grouped[f], one[f]), (f, grouped[f], one[f])

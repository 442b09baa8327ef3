"""CPU pin of which gather path of csrc/cont_kernel.hpp each continuous-operator test case runs (tests/cont_boxes.py
restates the rule).  A change of calibration, grid builder or LDS limit that moves a case of
tests/test_hip_continuous_paths.py to another path fails here, without a GPU."""
import glob
import os

import numpy as np
import pytest

import cont_boxes as cb

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "cont_*_sd*.npz")))


@pytest.mark.parametrize("case", cb.CASES, ids=cb.CASE_IDS)
def test_case_table_runs_the_path_its_name_claims(case):
    name, _, sizes, _, (kind, k), cls, n_staged, n_unstaged, cap = case
    model, params, grids, nodes, weights = cb.make_case(case)
    r = cb.classify(model, params, grids, nodes)
    assert nodes.shape[1] <= 4096                      # the T tolerance of the GPU test is derived for M <= 4096
    assert (r["cls"], r["n_staged"], r["n_unstaged"]) == (cls, n_staged, n_unstaged)
    assert r["staged"].shape == tuple(sizes) and r["n_staged"] + r["n_unstaged"] == int(np.prod(sizes))
    if cap is not None:
        assert r["cap"] == cap
    if cls == "A":
        assert r["tq"] == k and r["ucap"] == r["uomax"] * k * k and r["ucap"] + r["cap"] <= 4000
    else:
        assert r["tq"] == 0 and r["ucap"] == 0
    if cls in "CD":
        # the J.v launch asks for its largest dynamic LDS: 2 * 4000 doubles
        assert r["vmax"] > cb.CAP_LIMIT and r["cap"] == 4000 and r["lds_jvp"] == 64000
    if cls == "B" and kind == "gh":
        # a tensor rule was supplied and recognised, and its pre-contracted array refused
        assert r["tq_rule"] == k and r["vmax"] <= cb.CAP_LIMIT and r["uomax"] * k * k + r["cap"] > 4000
    if kind == "mc":
        assert r["tq_rule"] == 0 and weights is None


def test_every_class_is_in_the_table():
    for cls in "ABCD":                                 # the 4-D and the 6-D kernel on every path
        assert {c[1] for c in cb.CASES if c[5] == cls} == {"ssy", "gcy"}
    assert {c[1] for c in cb.CASES if c[5] == "B" and c[4][0] == "gh"} == {"ssy", "gcy"}
    assert {c[5] for c in cb.CASES if c[4][0] == "mc"} == {"B", "C"}


@pytest.mark.parametrize("fn", FILES, ids=[os.path.basename(f) for f in FILES])
def test_golden_fixtures_are_all_fully_staged(fn):
    """What tests/test_hip_continuous.py covers: quadrature always pre-contracted (class A), Monte Carlo always the
    staged full fold (class B); no fixture reaches the global-gather path."""
    z = np.load(fn)
    model = "ssy" if "cont_ssy" in fn else "gcy"
    grids = tuple(z[f"grid{i}"] for i in range(len(z["sizes"])))
    q = cb.classify(model, z["params"], grids, z["nodes"])
    m = cb.classify(model, z["params"], grids, z["mc_draws"])
    assert q["cls"] == "A" and q["n_unstaged"] == 0 and q["tq"] > 0
    assert m["cls"] == "B" and m["n_unstaged"] == 0 and m["tq"] == 0
    assert max(q["vmax"], m["vmax"]) <= 324 and z["w"].size <= 840


def test_tensor_detection_needs_gridmake_order():
    from oracle import continuous as OC
    nodes, _ = OC.qnwnorm([3] * 4)
    nodes = np.ascontiguousarray(nodes.T)
    assert cb.tensor_order(nodes) == 3
    assert cb.tensor_order(nodes[:, ::-1]) == 3        # the mirrored rule is still a tensor rule in gridmake order
    assert cb.tensor_order(nodes[:, np.random.default_rng(7).permutation(81)]) == 0
    assert cb.tensor_order(np.random.default_rng(1).standard_normal((4, 256))) == 0
    assert cb.tensor_order(np.zeros((4, 1))) == 0


def test_staging_rule_is_cumulative_from_the_last_dimension():
    """cont_kernel.hpp:162-163 on a hand-made case: cap = 4000 and boxes of 5 x 9 x 9 x 18 fail at the last factor."""
    model, params, grids, nodes, _ = cb.make_case(cb.CASES[cb.CASE_IDS.index("D-ssy")])
    r = cb.classify(model, params, grids, nodes)
    assert r["mext"] == [9, 9, 9, 18] and r["vmax"] == 13122 and r["cap"] == 4000
    bext = [np.broadcast_to(b, r["staged"].shape) for b in cb.box_extents(model, params, grids, nodes)]
    total = bext[0] * bext[1] * bext[2] * bext[3]
    np.testing.assert_array_equal(r["staged"], total <= r["cap"])      # extents >= 2: the running product is monotone

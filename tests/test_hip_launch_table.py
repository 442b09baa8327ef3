"""
Characterisation of the host layer (csrc/sdfs_api.hip): on the smallest shape of every path -- generic tiles with
unconditional and with conditional tensors and in fp32 storage, small-grid, padded and pair plans with the streamed and the
plain line passes and with fp32 intermediates, the continuous and the dense operator -- one application launches the kernels
under the counter names with the byte and flop counts, prints the plan and computes the bits that
tests/golden/launch_table.json holds, and the three solver loops take the iterations and reach the final error recorded
there, with the captured graph and with plain launches.

The fixture is recorded by tools/launch_table.py on the commit BEFORE a change of the host layer, twice; an output that
is not reproducible bit for bit between the two recordings has no hash in it (null) and is skipped here.  Equality
throughout: counter names and plan text are strings, bytes and flops are computed from integers, and a kernel that is
launched with the same arguments on the same inputs sums in the same order.
"""
import json

import pytest

import launch_table as LT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


@pytest.fixture(scope="module")
def gold():
    with open(LT.FIXTURE) as f:
        return json.load(f)


def check(got, want, name):
    if "describe" in want:
        assert got["describe"] == want["describe"], name
    assert [c[0] for c in got["counters"]] == [c[0] for c in want["counters"]], name
    assert got["counters"] == want["counters"], name
    assert set(got["hashes"]) == set(want["hashes"]), name
    for k, hx in want["hashes"].items():
        if hx is not None:
            assert got["hashes"][k] == hx, f"{name}: output {k} differs from the recording"


@pytest.mark.parametrize("name", LT.CASES)
def test_applications(S, gold, name):
    check(LT.record_case(S, name), gold["applications"][name], name)


def test_generic_tiles_fp32_storage(S, gold):
    for k, got in LT.storage_forms(S).items():
        check(got, gold["applications"][LT.STORAGE_CASE + " " + k], k)


def test_pair_plan_t_f32(S, gold):
    check(LT.t32_form(S), gold["applications"][LT.T32_CASE + " t_f32"], "t_f32")


def test_fixture_is_complete(gold):
    names = set(LT.CASES) | {LT.STORAGE_CASE + " krylov_f32=1", LT.STORAGE_CASE + " krylov_f32=2", LT.T32_CASE + " t_f32"}
    assert set(gold["applications"]) == names
    assert set(gold["loops"]) == {LT.loop_key(n, a, g) for n in LT.LOOP_CASES for a in LT.ALGORITHMS for g in (1, 0)}
    hashes = [hx for c in gold["applications"].values() for hx in c["hashes"].values()]
    assert sum(hx is None for hx in hashes) <= 2, "more than two outputs were not reproducible when the fixture was recorded"


@pytest.mark.parametrize("use_graph", [1, 0], ids=["graph", "launches"])
@pytest.mark.parametrize("algorithm", LT.ALGORITHMS)
@pytest.mark.parametrize("name", list(LT.LOOP_CASES))
def test_loops(S, gold, name, algorithm, use_graph):
    assert LT.record_loop(S, name, algorithm, use_graph) == gold["loops"][LT.loop_key(name, algorithm, use_graph)]

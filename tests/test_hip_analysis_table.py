"""
Characterisation of the analysis layer (sdfs_via_autodiff_amd/pricing.py, sensitivity.py, simulation.py and the host
code under them: the pricing section of csrc/sdfs_api.hip, csrc/cont_price.hpp): on the smallest grids every analysis
function at w*, on the discretised and on the continuous-state operator, launches the kernels under the counter names
with the launch, byte and flop counts and computes the bits that tests/golden/analysis_table.json holds.

The fixture is recorded by tools/analysis_table.py on the commit BEFORE a change of that layer, twice; an output that is
not reproducible bit for bit between the two recordings has no hash in it (null) and is skipped here.  Every call is
recorded on an operator of its own, so each case stands alone, whatever ran before it in the process.  The tilted
applications and the horizon loop use no atomics and reduce in a fixed order, so none of their outputs may be null.
"""
import json

import pytest

import analysis_table as AT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


@pytest.fixture(scope="module")
def gold():
    with open(AT.FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name,call", AT.ALL, ids=[f"{n}: {c}" for n, c in AT.ALL])
def test_calls(S, gold, name, call):
    got, want = AT.record_call(S, name, call), gold[name][call]
    assert len(want["counters"]) < AT.MAX_NAMES, "the handle's counter names overflowed when the fixture was recorded"
    assert [c[0] for c in got["counters"]] == [c[0] for c in want["counters"]], (name, call)
    assert got["counters"] == want["counters"], (name, call)
    assert set(got["hashes"]) == set(want["hashes"]), (name, call)
    for k, hx in want["hashes"].items():
        if hx is not None:
            assert got["hashes"][k] == hx, f"{name}: {call}: output {k} differs from the recording"


def test_fixture_is_complete(gold):
    assert set(gold) == set(AT.CASES)
    for name in AT.CASES:
        assert set(gold[name]) == set(AT.calls_of(name)), name
    hashes = {(name, call, k): hx for name, case in gold.items() for call, c in case.items() for k, hx in c["hashes"].items()}
    missing = [key for key, hx in hashes.items() if hx is None]
    assert len(missing) <= 2, f"more than two outputs were not reproducible when the fixture was recorded: {missing}"
    assert not [key for key in missing if key[1].startswith(AT.EXACT)], "a tilted application or a horizon output has no hash"
    for name in AT.CASES:
        for call in AT.calls_of(name):
            assert gold[name][call]["hashes"] and gold[name][call]["counters"], (name, call)

"""
CPU tests of the continuous-state simulation (sdfs_via_autodiff_amd/simulation.py ``simulate_continuous``);
no device call is made here:

 (1) the exports; (2) every bad request raises before a device call; (3) the numpy twin (tests/cont_sim_oracle.py) is
 consistent with the oracle's ``next_state`` on its own normals; (4) the twin's E_x[M] at a constant w equals the closed
 form; (5) the input conditions of the GPU tests: on the ``num_std_devs = 1.0`` grids at least 5 % of the recorded steps
 are clamped on every axis, on the 3.2 grids fewer than 5 % overall; (6) the rounding amplification A of the GPU test
 cases: the largest ``close(fp64 twin, longdouble twin, 1.0)`` over all their series.
"""
import numpy as np
import pytest

import sdfs_via_autodiff_amd as S
from sdfs_via_autodiff_amd import simulate_continuous, _lib

import cont_sim_cases as CC
import cont_sim_oracle as co
from oracle import continuous as OC


# -- (1) ------------------------------------------------------------------------------------------------------------------
def test_exports():
    assert "simulate_continuous" in S.__all__ and S.simulate_continuous is simulate_continuous
    for name in ("sdfs_cont_sdf_mean_dev", "sdfs_cont_sim_records_dev", "sdfs_cont_sim_paths_dev"):
        assert name in _lib.SYMBOLS
    for name in ("cont_sdf_mean_dev", "cont_sim_records_dev", "cont_sim_paths_dev"):
        assert callable(getattr(S.ContinuousOperator, name))


# -- (2) ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def request_case():
    m = S.SSY()
    grids = S.build_grid(m, 2, 3, 4, 5)
    return m, grids, np.full((2, 3, 4, 5), 700.0)


def no_device(monkeypatch):
    """Any attempt to open the device fails the test."""
    import torch

    def boom(*a, **k):
        raise AssertionError("a bad request reached the device")
    monkeypatch.setattr(torch.cuda, "mem_get_info", boom)
    monkeypatch.setattr(S.ContinuousOperator, "__init__", boom)


BAD = [
    (dict(n_paths=0), ValueError, "n_paths"),
    (dict(n_paths=2.5), ValueError, "n_paths"),
    (dict(n_periods=1), ValueError, "n_periods"),
    (dict(burn_in=-1), ValueError, "burn_in"),
    (dict(seed=-1), ValueError, "seed"),
    (dict(path_offset=(1 << 32) - 1, n_paths=2), ValueError, "path_offset \\+ n_paths"),
    (dict(step_offset=-1), ValueError, "step_offset"),
    (dict(step_offset=(1 << 32) - 10, n_periods=10), ValueError, "step_offset \\+ burn_in \\+ n_periods"),
    (dict(step_offset=1 << 31, burn_in=1 << 31, n_periods=8), ValueError, "2\\^32"),
    (dict(start=np.zeros(3)), ValueError, "start has shape"),
    (dict(start=np.zeros((5, 4)), n_paths=6), ValueError, "start has shape"),
    (dict(start=np.array([0.0, np.nan, 0.0, 0.0])), ValueError, "finite"),
    (dict(start=np.array([0.0, np.inf, 0.0, 0.0])), ValueError, "finite"),
    (dict(n_paths=1 << 13, n_periods=(1 << 12) + 1, return_paths=True), ValueError, "2\\^25 path-steps"),
    (dict(d=0), ValueError, "d must be"),
    (dict(operator=object()), TypeError, "ContinuousOperator"),
]


@pytest.mark.parametrize("kw,exc,msg", BAD, ids=[f"{i}:{sorted(k)[0]}" for i, (k, _, _) in enumerate(BAD)])
def test_bad_requests_raise_before_any_device_call(monkeypatch, request_case, kw, exc, msg):
    no_device(monkeypatch)
    m, grids, w = request_case
    args = dict(n_paths=16, n_periods=8)
    args.update(kw)
    with pytest.raises(exc, match=msg):
        simulate_continuous(m, grids, w, args.pop("n_paths"), args.pop("n_periods"), **args)


def test_bad_grids_w_star_and_model_raise_before_any_device_call(monkeypatch, request_case):
    no_device(monkeypatch)
    m, grids, w = request_case
    with pytest.raises(ValueError, match="w_star has shape"):
        simulate_continuous(m, grids, w[:, :, :, :4], 16, 8)
    bad = w.copy()
    bad[1, 2, 0, 4] = 1.0
    with pytest.raises(ValueError, match="exceed 1"):
        simulate_continuous(m, grids, bad, 16, 8)
    bad[1, 2, 0, 4] = 0.5
    with pytest.raises(ValueError, match="exceed 1"):
        simulate_continuous(m, grids, bad, 16, 8)
    # the grid count against the model
    with pytest.raises(ValueError, match="4 state variables, got 3 grids"):
        simulate_continuous(m, grids[:3], w[..., 0], 16, 8)
    g6 = S.build_grid(S.GCY(), 2, 2, 2, 2, 2, 2)
    with pytest.raises(ValueError, match="4 state variables, got 6 grids"):
        simulate_continuous(m, g6, np.full((2,) * 6, 700.0), 16, 8)
    with pytest.raises(ValueError, match="6 state variables, got 4 grids"):
        simulate_continuous(S.GCY(), grids, w, 16, 8)
    with pytest.raises(ValueError, match="increasing"):
        simulate_continuous(m, (grids[0][::-1],) + tuple(grids[1:]), w, 16, 8)
    with pytest.raises(TypeError, match="SSY or a GCY"):
        simulate_continuous(object(), grids, w, 16, 8)


# -- (3) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes", [("ssy", (2, 3, 4, 5)), ("gcy", (2, 3, 2, 3, 4, 3))], ids=["ssy", "gcy"])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble], ids=["fp64", "longdouble"])
def test_twin_first_state_is_next_state_of_its_own_normals(kind, sizes, dtype):
    par = CC.params_of(kind)
    grids = CC.grids_of(kind, sizes, 3.2)
    D = len(grids)
    start = CC.start_of(grids, "vector")
    paths = np.arange(5, 12, dtype=np.uint64)
    X, xi = co.state_paths(kind, par, D, CC.SEED, 5, 7, 3, 4, step_offset=11, start=start, dtype=dtype)
    assert X.dtype == dtype and X.shape == (7, 5, D) and xi.shape == (7, 4)
    nxt = OC.next_state_ssy if kind == "ssy" else OC.next_state_gcy
    x = np.broadcast_to(np.asarray(start, dtype=dtype), (7, D)).T
    for k in range(1, 5):
        eta, z = co.normals(CC.SEED, 11 + k, paths, D, dtype)
        x = nxt(par, x, eta)
        if k >= 3:
            assert np.array_equal(X[:, k - 3, :], x.T)
        if k > 3:
            assert np.array_equal(xi[:, k - 4], z)
    # the normals: n_4b … n_4b+3 from block b, streams apart from the discretised simulator's (last counter word 1)
    import sim_oracle as so
    key = (CC.SEED & 0xFFFFFFFF, CC.SEED >> 32)
    r = so.philox4x32_10((12, paths, 1, 1), key)
    eta, z = co.normals(CC.SEED, 12, paths, D, np.float64)
    u = (r[0].astype(np.float64) + 0.5) * 2.0 ** -32
    want = np.sqrt(-2.0 * np.log(u)) * np.cos(2.0 * np.pi * (r[1].astype(np.float64) * 2.0 ** -32))
    assert np.array_equal(z if D == 4 else eta[4], want)
    assert not np.array_equal(so.philox4x32_10((12, paths, 1, 0), key)[0], r[0])
    assert np.all(np.abs(eta) < 7.0)


# -- (4) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sizes", [("ssy", (2, 3, 4, 5)), ("gcy", (2, 3, 2, 3, 2, 3))], ids=["ssy", "gcy"])
def test_twin_sdf_mean_of_a_constant_w_is_the_closed_form(kind, sizes):
    """w ≡ c: the interpolant is c everywhere and Gauss–Hermite (d = 5) integrates exp(θ s_λ η) exactly to rounding."""
    par = CC.params_of(kind)
    grids = CC.grids_of(kind, sizes, 3.2)
    nodes, weights = OC.qnwnorm([5] * len(grids))
    c = 650.0
    got = co.sdf_mean(kind, par, grids, np.full(sizes, c), nodes.T, weights)
    np.testing.assert_allclose(got, co.sdf_mean_constant_w(kind, par, grids, c), rtol=1e-12)


# -- (5), (6) -------------------------------------------------------------------------------------------------------------
_EM = {}


def twin_inputs(kind, sizes, sd):
    key = CC.tag(kind, sizes, sd)
    if key not in _EM:
        par = CC.params_of(kind)
        grids = CC.grids_of(kind, sizes, sd)
        w = CC.golden_wstar(kind, sizes, sd)
        nodes, weights = OC.qnwnorm([CC.QUAD_D] * len(grids))
        _EM[key] = (par, grids, w, co.sdf_mean(kind, par, grids, w, nodes.T, weights))
    return _EM[key]


@pytest.mark.parametrize("kind,sizes,sd", CC.GRIDS, ids=[CC.tag(*g) for g in CC.GRIDS])
def test_input_conditions_of_the_gpu_cases(kind, sizes, sd):
    """Share of the recorded steps outside the grid in the cases the GPU file runs on this grid (P = 1000, T = 64,
    burn-in 0 and 7, the zero and the one-vector start of cont_sim_cases.start_of).

    On a 1.0 grid each case with the vector start, and the four cases pooled, have at least 5 % of their recorded steps
    clamped on every axis; on a 3.2 grid each of the four cases has fewer than 5 % clamped overall.

    Measured, per axis, burn-in 7 (burn-in 0 is within 0.05 of it).  Zero start: SSY at 1.0 (both sizes) 0.293, 0.156,
    0.137, 0.712; GCY at 1.0 0.235, 0.141, 0.243, 0.266, 0.000, 0.065.  Vector start: SSY at 1.0 0.351, 0.257, 0.583,
    0.532; GCY at 1.0 0.426, 0.252, 0.429, 0.291, 0.279, 0.183.  Overall on the 3.2 grids: SSY 0.011 (zero) and 0.004
    (vector), GCY 0.001 and 0.005.

    From the zero state no step leaves the z axis of the GCY 1.0 grid (share 0.000): the reference's build_grid divides
    the z range by 1 − ρ_zπ where the persistence of z was meant (gcy_wc_ratio_continuous.py:47, :68-69, kept so that
    grids agree with the reference's), which makes it ±0.0097 against a sample standard deviation of z of 0.0015.  The
    vector start is what clamps that axis; it is chosen outside the 1.0 grids for that."""
    par, grids, w, em = twin_inputs(kind, sizes, sd)
    assert w.shape == tuple(sizes) and np.all(w > 1.0) and np.all(em > 0.0)
    vec = CC.start_of(grids, "vector")
    assert np.array_equal(vec, CC.start_of(CC.grids_of(kind, sizes, 3.2), "vector"))      # one state for both grids
    assert all(g[0] < v < g[-1] for v, g in zip(vec, CC.grids_of(kind, sizes, 3.2)))
    pooled = []
    for burn_in in CC.BURN_INS:
        for start in CC.STARTS:
            X, _ = co.state_paths(kind, par, len(grids), CC.SEED, CC.PATH_OFFSET, CC.P, burn_in, CC.T,
                                  start=CC.start_of(grids, start))
            rec = X[:, 1:, :]
            out = np.stack([(rec[..., d] < g[0]) | (rec[..., d] > g[-1]) for d, g in enumerate(grids)], axis=-1)
            assert np.array_equal(out.any(axis=-1), co.outside(grids, X)[0][:, 1:])
            per_axis = out.mean(axis=(0, 1))
            overall = float(out.any(axis=-1).mean())
            print(f"{CC.tag(kind, sizes, sd)} burn-in {burn_in} {start} start: clamped share per axis "
                  f"{np.round(per_axis, 4)}, overall {overall:.4f}")
            if sd == 1.0 and start == "vector":
                assert per_axis.min() >= 0.05, (burn_in, start, per_axis)
            if sd != 1.0:
                assert overall < 0.05, (burn_in, start, overall)
            pooled.append(out)
    if sd == 1.0:
        per_axis = np.concatenate(pooled).mean(axis=(0, 1))
        print(f"{CC.tag(kind, sizes, sd)} the four cases pooled: clamped share per axis {np.round(per_axis, 4)}")
        assert per_axis.min() >= 0.05, per_axis


def amplification_cases():
    for kind, sizes, sd in CC.GRIDS:
        for burn_in in CC.BURN_INS:
            for start in CC.STARTS:
                yield kind, sizes, sd, burn_in, start
        yield kind, sizes, sd, 0, "far"


def test_rounding_amplification_of_the_gpu_cases():
    """A = the largest close(fp64 twin, longdouble twin, 1.0) over the states and all series of the GPU test cases:
    every grid of cont_sim_cases.GRIDS with burn-in 0 and 7 and the zero and the vector start (the cases of the GPU
    file's (2)), and the far-outside start (its (4)).

    Measured: over the cases of (2) A = 7.7e-14 (m of gcy_2x3x2x3x4x3_sd1.0: ln ŵ(x_t) − ln(ŵ(x_{t−1}) − 1) is multiplied
    by θ − 1; states 2.0e-15).  With the far-outside start A = 1.7e-10 (z and with it dc, m, rc, xc of
    gcy_2x3x2x3x4x3_sd3.2; 2.5e-11 on the SSY 3.2 grids, 1.1e-12 and below on the 1.0 grids): ten grid widths out
    exp(h_z) is of the order 1e4, z is that large for the first steps and keeps the absolute rounding error of that
    phase while it decays to order one, which is what ``close`` then measures it against."""
    A = {"(2)": 0.0, "(4)": 0.0}
    worst = {}
    for kind, sizes, sd, burn_in, start in amplification_cases():
        par, grids, w, em = twin_inputs(kind, sizes, sd)
        kw = dict(seed=CC.SEED, path_offset=CC.PATH_OFFSET, n_paths=CC.P, burn_in=burn_in, n_periods=CC.T,
                  start=CC.start_of(grids, start))
        lo = co.simulate(kind, par, grids, w, em, dtype=np.float64, **kw)
        hi = co.simulate(kind, par, grids, w, em, dtype=np.longdouble, **kw)
        which = "(4)" if start == "far" else "(2)"
        for nm, e in [("state", co.close(lo["state"], hi["state"], 1.0))] + \
                     [(nm, co.close(lo["series"][nm], hi["series"][nm], 1.0)) for nm in co.SERIES]:
            if e > A[which]:
                A[which], worst[which] = e, (CC.tag(kind, sizes, sd), burn_in, start, nm)
    print(f"rounding amplification A: cases of (2) {A['(2)']:.3e} at {worst['(2)']}, far-outside start {A['(4)']:.3e} "
          f"at {worst['(4)']}")
    # rounding alone must stay below the largest bound the device comparison may use (1e-9)
    assert max(A.values()) <= 1e-9

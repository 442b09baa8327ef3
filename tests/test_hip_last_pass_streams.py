"""
GPU tests of the streamed last pass of T (csrc/stream_kernels.hpp, line_stream_kernel with OLDPF, one tile per
workgroup) at the smallest shapes that reach it: the pair plan forced on 4-D SSY grids whose line pass runs on whole
128-byte chunks.  On the 16- and 20-wide extents a launch that reads the side stream (the residual's w, Anderson's x)
issues its loads right behind the tile's own; a launch without one, and every linearising T, runs the old-order form;
the 24- and 32-wide kernels keep the side stream behind the park (registers).  20^4: 3200 units over 256 threads, the
partial last unit per thread; 16^4: whole units; 24^4: the old order, asserted through the plan line.
Checked against the numpy oracle with the tolerances of tests/test_hip_pair_plan.py (1e-12 relative per application:
sums in a different order, powers within a few ulp; J.v 1e-11).
"""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

APPLY_RTOL = 1e-12
NEW_LINE = "side stream in flight with the tile"
OLD_LINE = "side stream loaded early"
SHAPES = [(20, 20, 20, 20), (16, 16, 16, 16), (24, 24, 24, 24)]


@pytest.fixture(scope="module")
def S():
    import sdfs_via_autodiff_amd as S
    return S


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


_CACHE = {}


def case(S, shapes):
    """(operator on the streamed pair plan, w, v, oracle T w, oracle J v) -- the reference is computed once per shape."""
    if shapes not in _CACHE:
        from oracle import models, ssy
        p = models.ssy_params()
        arr = ssy.discretize_ssy(p, shapes)
        w = 400 + 500 * np.random.default_rng(5).random(shapes)
        v = np.random.default_rng(6).standard_normal(shapes)
        Tw = ssy.T_ssy_factorised(w, shapes, p, arr)
        Jv = ssy.jvp_ssy(w, v, shapes, p, arr)
        for a in (w, v, Tw, Jv):
            a.setflags(write=False)
        _CACHE[shapes] = (w, v, Tw, Jv)
    m = S.SSY()
    with env(SDFS_PLAN="pair", SDFS_LINE_STREAM=7):
        T = S.KoopmansOperator("ssy", shapes, m.params, S.discretize_ssy(m, shapes))
    plan = T.describe_plan()
    assert "pair plan pass" in plan and "streamed" in plan, plan
    # which order the last pass runs: the plan line says it
    assert (NEW_LINE if shapes[0] <= 20 else OLD_LINE) in plan, plan
    assert (OLD_LINE if shapes[0] <= 20 else NEW_LINE) not in plan, plan
    return (T,) + _CACHE[shapes]


@pytest.mark.parametrize("shapes", SHAPES)
def test_apply_with_residual(S, shapes):
    """(a) T w and max|T w - w| in one application: the side stream is read."""
    T, w, _, Tw, _ = case(S, shapes)
    for _ in range(2):
        got = T(w)
        np.testing.assert_allclose(got, Tw, rtol=APPLY_RTOL)
        r = np.max(np.abs(Tw - w))
        assert abs(T.residual() - r) <= 1e-12 * r + 1e-9
    T.close()


@pytest.mark.parametrize("shapes", SHAPES)
def test_apply_without_residual(S, shapes):
    """(b) no residual asked for: nothing of the side stream is issued or consumed (the launch runs the form without its
    loads) -- T w only."""
    import torch
    T, w, _, Tw, _ = case(S, shapes)
    dw = torch.from_numpy(np.array(w)).cuda()
    out = torch.zeros_like(dw)
    T.apply_dev(dw.data_ptr(), out.data_ptr(), None)
    T.synchronize()
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), Tw, rtol=APPLY_RTOL)
    # ... and with one, on the same handle, the same T w to the last bit (the order of the loads changes no arithmetic)
    out2 = torch.zeros_like(dw)
    resid = torch.zeros(1, dtype=torch.float64, device="cuda")
    T.apply_dev(dw.data_ptr(), out2.data_ptr(), resid.data_ptr())
    T.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    r = np.max(np.abs(Tw - w))
    assert abs(float(resid.item()) - r) <= 1e-12 * r + 1e-9
    T.close()


@pytest.mark.parametrize("shapes", SHAPES)
def test_linearise_and_jvp(S, shapes):
    """(c) the linearising T (L_TLAST_LIN) and one J v - v (L_JLAST with minus_identity) against the oracle's jvp.  Neither
    has an early form: no caller asks a linearising T for a residual and no L_JLAST form prefetches its side stream, so
    this case guards the old-order kernels that share the source with the new one."""
    import torch
    T, w, v, Tw, Jv = case(S, shapes)
    dw = torch.from_numpy(np.array(w)).cuda()
    dv = torch.from_numpy(np.array(v)).cuda()
    out = torch.zeros_like(dw)
    jout = torch.zeros_like(dw)
    T.linearize_dev(dw.data_ptr(), out.data_ptr())
    T.jvp_dev(dv.data_ptr(), jout.data_ptr(), minus_identity=True)
    T.synchronize()
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), Tw, rtol=APPLY_RTOL)
    want = Jv - v
    np.testing.assert_allclose(jout.cpu().numpy(), want, rtol=1e-11, atol=1e-12 * np.max(np.abs(Jv)) + 1e-15 * np.max(np.abs(v)))
    np.testing.assert_allclose(T.jvp(w, v), Jv, rtol=1e-11, atol=1e-12 * np.max(np.abs(Jv)))
    T.close()


@pytest.mark.parametrize("shapes", SHAPES)
def test_nonfinite_residual(S, shapes):
    """(e) one NaN in w: T w is NaN exactly where the oracle's is and the residual is +inf (the NaN flag of the
    residual travels through the side-stream registers)."""
    from oracle import models, ssy
    T, w, _, _, _ = case(S, shapes)
    wn = np.array(w)
    wn[shapes[0] - 1, 1, 2, shapes[3] - 1] = np.nan
    p = models.ssy_params()
    with np.errstate(all="ignore"):
        want = ssy.T_ssy_factorised(wn, shapes, p, ssy.discretize_ssy(p, shapes))
    got = T(wn)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=APPLY_RTOL)
    assert T.residual() == np.inf
    T.close()


@pytest.mark.parametrize("shapes", [(16, 16, 20, 20, 16, 16)])
def test_anderson_push_on_the_last_pass(S, shapes):
    """(d) Anderson's push riding on the last pass: r = T x - x and y = x + beta r are written by the last pass itself,
    <r, r> is summed there.  The library routes the push through T's last pass only on grids of 2^21 points and more, so
    this case runs on the smallest 6-D GCY grid whose last line pair is 20 wide (C oracle; and_r / and_y are the
    library's own history buffers, reachable only through the solver).  Two passes with a
    history of two and a mixing step on the second: x2 = sum_j alpha_j (x_j + beta r_j) with alpha from the Gram matrix
    of r_0, r_1 -- every output of the push is used.  The relative ridge (tr G / m) keeps the 2 x 2 solve at a condition
    number below 3.
    Bounds: one application is within 1e-12 relative, so x_1, r_0, r_1 carry at most 2e-12 |T x| each and
    x2 = alpha (x + beta r) at most (1 + 2 beta) 2e-12 max|x| = 1e-11 max|x| at beta = 2; ||r||_2 moves by at most
    ||delta r||_2 <= 2e-12 ||T x||_2."""
    from oracle.c_oracle import COperator
    from oracle import models, gcy, solvers
    g = S.GCY()
    arr = S.discretize_gcy(g, shapes)
    T = S.KoopmansOperator("gcy", shapes, g.params, arr)
    plan = T.describe_plan()
    last = [ln for ln in plan.splitlines() if ln.startswith("pair plan pass 2")]
    assert last and NEW_LINE in last[0], plan
    p = models.gcy_params()
    oc = COperator("gcy", shapes, p, gcy.discretize_gcy(p, shapes))
    beta = 2.0
    x0 = 400 + 500 * np.random.default_rng(7).random(shapes)
    x, n, info = T.solve(x0, "anderson", tol=0.0, max_iter=2, history=2, mixing_freq=2, beta=beta, ridge=-1.0,
                         record_errors=True)
    assert n == 2 and info["n_apply"] == 2
    Tx0 = oc(x0)
    r0 = Tx0 - x0
    Tx1 = oc(Tx0)
    r1 = Tx1 - Tx0
    want, it = solvers.anderson_solver(oc, x0, tol=0.0, max_iter=2, verbose=False, history_size=2, mixing_frequency=2,
                                       beta=beta, ridge=-1.0)
    assert it == 2
    assert np.max(np.abs(x - want)) <= (1 + 2 * beta) * 2e-12 * np.max(np.abs(want))
    for e, r, tx in zip(info["errors"][:2], (r0, r1), (Tx0, Tx1)):
        nr = np.linalg.norm(r.ravel())
        assert abs(e - nr) <= 2e-12 * np.linalg.norm(tx.ravel()) + 1e-15 * nr, (e, nr)
    T.close()

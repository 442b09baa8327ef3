"""
Host-side tests of the batch simulation (no GPU): the per-member cumulative tables against ``simulation.cdf_tables``, the
numpy restatement of the device's fixed-order Chan reduction against a two-pass numpy, which shapes take the LDS form,
and the refusals, which come before any device call.
"""
import numpy as np
import pytest

import sdfs_via_autodiff_amd as S
from sdfs_via_autodiff_amd import batch, simulation
from batch_family import member, package_model

import sim_oracle as so


def family(kind, n=3):
    return [package_model(S, kind, member(kind, b)) for b in range(n)]


def stacked(kind, models, shapes):
    disc = S.discretize_ssy if kind == "ssy" else S.discretize_gcy
    per = [disc(m, shapes) for m in models]
    return per, [np.stack([np.asarray(a[i], dtype=np.float64).ravel() for a in per]) for i in range(len(per[0]))]


@pytest.mark.parametrize("kind,shapes", [("ssy", (3, 4, 3, 5)), ("gcy", (3, 2, 3, 2, 2, 3))], ids=["ssy", "gcy"])
def test_member_tables_are_those_of_cdf_tables(kind, shapes):
    models = family(kind)
    per, arrays = stacked(kind, models, shapes)
    cdf, cdf0 = batch.batch_cdf_tables(kind, shapes, arrays)
    assert cdf.shape == (3, sum(n * n for n in shapes)) and cdf0.shape == (3, sum(shapes))
    for b, m in enumerate(models):
        c, c0 = simulation.cdf_tables(m, shapes, per[b])
        assert np.array_equal(cdf[b], np.concatenate([x.ravel() for x in c]))
        assert np.array_equal(cdf0[b], np.concatenate(c0))
        o = 0
        for n in shapes:                                  # rows that rise to the sentinel 2
            rows = cdf[b, o:o + n * n].reshape(n, n)
            assert np.all(np.diff(rows, axis=1) >= 0) and np.all(rows[:, -1] == 2.0)
            o += n * n


@pytest.mark.parametrize("kind,shapes", [("ssy", (3, 4, 3, 5)), ("gcy", (3, 2, 3, 2, 2, 3))], ids=["ssy", "gcy"])
@pytest.mark.parametrize("start", ["stationary", "fixed"])
def test_table_blocks_are_cdf_tables_and_model_pieces(kind, shapes, start):
    """The blocks the library stages for the path kernel (sdfs_batch_sim_tables: the host code of
    sdfs_batch_sim_paths_dev) against ``cdf_tables`` and the twin's ``model_pieces``, member by member."""
    models = family(kind)
    per, arrays = stacked(kind, models, shapes)
    params = np.array([m.params for m in models], dtype=np.float64)
    cdf, cdf0 = batch.batch_cdf_tables(kind, shapes, arrays)
    fixed = None if start == "stationary" else tuple(n // 2 for n in shapes)
    kap = np.array([2.0, 1.5, 3.0])
    tab, scal, zt = batch.batch_sim_tables(kind, shapes, params, arrays, cdf, None if fixed else cdf0, start=fixed, kappa=kap,
                                           skip=[0, 1, 0])
    ncdf, ncdf0 = sum(n * n for n in shapes), sum(shapes)
    for b, m in enumerate(models):
        th, beta, gamma, hl, ax_l, sc, ax_c, muz = so.model_pieces(kind, m.params, per[b], shapes)
        c, c0 = simulation.cdf_tables(m, shapes, per[b])
        assert tab.shape[1] == (ncdf + ncdf0 + hl.size + sc.size + 1) // 2 * 2
        assert np.array_equal(tab[b, :ncdf], np.concatenate([x.ravel() for x in c]))
        assert np.array_equal(tab[b, ncdf:ncdf + ncdf0], np.full(ncdf0, 2.0) if fixed else np.concatenate(c0))
        o = ncdf + ncdf0
        assert np.array_equal(tab[b, o:o + hl.size], hl) and np.array_equal(tab[b, o + hl.size:o + hl.size + sc.size], sc)
        assert np.all(tab[b, o + hl.size + sc.size:] == 0.0)
        # theta = (1 - gamma) / (1 - 1 / psi) and theta ln beta are formed by the library's own arithmetic: three roundings, the
        # one of 1 / psi amplified about threefold by 1 - 1 / psi at psi near 1.5 -> 8 eps; a logarithm and a product on top
        assert abs(scal[b, 0] - th) <= 2e-15 * abs(th) and abs(scal[b, 1] - th * np.log(beta)) <= 4e-15 * abs(th * np.log(beta))
        assert scal[b, 2] == gamma and scal[b, 3] == (0.0 if b == 1 else kap[b])
        if kind == "ssy":
            grid = np.broadcast_to(zt[b].reshape(shapes[2], shapes[3])[None, None], shapes)
        else:                                             # a3 layout [z_pi, h_z, h_zpi, z] -> grid order
            z = np.transpose(zt[b].reshape(shapes[1], shapes[2], shapes[4], shapes[0]), (3, 0, 1, 2))
            grid = np.broadcast_to(z[:, :, :, None, :, None], shapes)
        assert np.array_equal(grid, muz)
    assert not np.array_equal(scal[0], scal[2]) and not np.array_equal(zt[0], zt[1])


def test_conditional_tensors_are_refused():
    kind, shapes = "ssy", (3, 4, 3, 5)
    _, arrays = stacked(kind, family(kind, 1), shapes)
    q = np.tile(arrays[1].reshape(1, 3, 3), (2, 1, 1))
    q[1, 0, :2] = q[1, 0, 1::-1] + [1e-3, -1e-3]
    arrays[1] = q.reshape(1, -1)
    with pytest.raises(ValueError, match="does not factorise"):
        batch.batch_cdf_tables(kind, shapes, arrays)


def chan_merge(a, b):
    """Chan, Golub and LeVeque's merge of two (n, mean, M2) triples as the device forms it (bsim_merge of
    csrc/batch_sim.hpp, up to its fused multiply-adds); an empty side leaves the other unchanged."""
    n = a[0] + b[0]
    f = b[0] / n if n > 0 else 0.0
    d = b[1] - a[1]
    return (n, a[1] + d * f, (a[2] + b[2]) + d * d * (a[0] * f))


def chan_fixed_order(x, block=256):
    """(n, mean, se) of the finite entries of ``x`` in the device's order: one triple per path, a pairwise tree over the 64
    lanes of a wave (the lower lane on the left), the waves of a workgroup of ``block`` paths in order, then the
    workgroups in order.  Numpy restatement of the reduction of csrc/batch_sim.hpp."""
    x = np.asarray(x, dtype=np.float64).ravel()
    total = None
    for g0 in range(0, max(x.size, 1), block):
        wg = None
        for w0 in range(g0, g0 + block, 64):
            t = [(1.0, float(v), 0.0) if np.isfinite(v) else (0.0, 0.0, 0.0) for v in x[w0:w0 + 64]]
            t += [(0.0, 0.0, 0.0)] * (64 - len(t))
            while len(t) > 1:
                t = [chan_merge(t[i], t[i + 1]) for i in range(0, len(t), 2)]
            wg = t[0] if wg is None else chan_merge(wg, t[0])
        total = wg if total is None else chan_merge(total, wg)
    n, mean, m2 = total
    nan = float("nan")
    return n, mean if n > 0 else nan, float(np.sqrt(m2 / (n - 1.0) / n)) if n > 1 else nan


def two_pass(x):
    x = x[np.isfinite(x)]
    n = x.size
    if n == 0:
        return 0, np.nan, np.nan
    return n, x.mean(), (x.std(ddof=1) / np.sqrt(n) if n > 1 else np.nan)


@pytest.mark.parametrize("size", [1, 2, 5, 63, 64, 65, 255, 256, 257, 1000, 4096])
def test_fixed_order_chan_reduction_matches_two_pass(size):
    rng = np.random.default_rng(size)
    # a mean far from zero next to a small spread is where raw sums of squares lose their digits
    x = 1e3 + 1e-3 * rng.standard_normal(size)
    x[rng.random(size) < 0.2] = np.nan
    if size > 2:
        x[2] = np.inf
    n, mean, se = chan_fixed_order(x)
    rn, rmean, rse = two_pass(x)
    assert n == rn
    if rn > 0:
        assert abs(mean - rmean) <= 1e-14 * abs(rmean)
    else:
        assert np.isnan(mean)
    if rn > 1:
        assert abs(se - rse) <= 1e-10 * rse
    else:
        assert np.isnan(se)


def test_chan_merge_with_an_empty_side_is_exact():
    t = (7.0, 0.1 + 0.2, 1.0 / 3.0)
    assert chan_merge((0.0, 0.0, 0.0), t) == t and chan_merge(t, (0.0, 0.0, 0.0)) == t
    assert chan_merge((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) == (0.0, 0.0, 0.0)


def test_which_shapes_take_the_lds_form():
    rec = simulation.REC_BYTES
    for kind, shapes, fits in (("ssy", (5,) * 4, True), ("ssy", (3, 4, 3, 5), True), ("gcy", (3, 2, 3, 2, 2, 3), True),
                               ("ssy", (7,) * 4, True), ("ssy", (8,) * 4, False), ("ssy", (10,) * 4, False),
                               ("gcy", (5,) * 6, False)):
        n = int(np.prod(shapes))
        lds, glob = batch.batch_sim_lds_bytes(kind, shapes, 1), batch.batch_sim_lds_bytes(kind, shapes, 2)
        assert glob is not None and glob < 64 * 1024
        assert (lds is not None) == fits, (kind, shapes, lds)
        if fits:
            assert lds == glob + n * rec and lds <= 160 * 1024
    assert batch.batch_sim_lds_bytes("ssy", (12,) * 4, 2) is None          # beyond the batch plan
    with pytest.raises(S.SdfsError):
        batch.batch_sim_lds_bytes("ssy", (5,) * 4, 3)


def test_refusals_come_before_any_device_call():
    kind, shapes = "ssy", (3, 4, 3, 5)
    models = family(kind)
    w = np.full((3,) + shapes, 700.0)
    ok = dict(n_paths=16, n_periods=8)

    def call(models=models, shapes=shapes, w=w, **kw):
        a = dict(ok, **kw)
        return S.simulate_batch(models, shapes, w, a.pop("n_paths"), a.pop("n_periods"), **a)
    for kw, pat in ((dict(n_paths=0), "n_paths"), (dict(n_periods=1), "n_periods"), (dict(burn_in=-1), "burn_in"),
                    (dict(seed=-1), "seed"), (dict(seed=1.5), "seed"), (dict(path_offset=1 << 32), "path_offset"),
                    (dict(start="ergodic"), "start"), (dict(start=(0, 0, 0)), "one state index per axis"),
                    (dict(start=(0, 4, 0, 0)), r"start\[1\]"), (dict(rtol=0.0), "rtol"), (dict(records=3), "records"),
                    (dict(records=True), "records"), (dict(kappa=[1.0, 2.0]), "kappa"), (dict(kappa=float("nan")), "kappa"),
                    (dict(n_paths=1 << 12, n_periods=1 << 12, return_paths=True), "2\\^25"),
                    (dict(w=w[:2]), "w_star"), (dict(shapes=(3, 4, 3)), "4 axes"), (dict(models=[]), "empty"),
                    (dict(models=models[:2] + [S.GCY()]), "all SSY or all GCY")):
        with pytest.raises((ValueError, TypeError), match=pat):
            call(**kw)
    with pytest.raises(ValueError, match="2\\^32"):
        call(n_paths=(1 << 31) + 1, path_offset=1 << 31)
    with pytest.raises(ValueError, match="beyond the batch plan"):
        S.simulate_batch(models, (12,) * 4, np.full((3,) + (12,) * 4, 700.0), 16, 8, records=1)


def test_exports():
    for name in ("simulate_batch", "BatchSimulation", "batch_sim_lds_bytes", "batch_cdf_tables"):
        assert name in S.__all__ and hasattr(S, name)
    assert S.BatchSimulation._fields == ("series", "moments", "per_path", "paths", "status", "price", "plan")
    for name in ("sdfs_batch_sim_lds_bytes", "sdfs_batch_sim_tables", "sdfs_batch_sim_records_dev", "sdfs_batch_sim_paths_dev"):
        assert name in S._lib.SYMBOLS

"""
The kernels of the batched-Gram Anderson loop -- k_and_push_lite, k_and_gram_full, k_and_step_lazy (and_step_wave /
and_solve_fast) and k_and_mix_y -- held to a long-double twin STEP BY STEP through the sharded-loop ABI
(sdfs_anderson_begin / _step / _state), which takes x_out = T(x_in) from the caller: the test prescribes the residual of
every pass (x_out = x_in + r_i, r_i = s_i N(0, 1) with the tail elements x 8; tests/anderson_twin.py) instead of applying
an operator, so the Gram matrix is well-conditioned and every comparison is tight.  No model, grid or process group is
involved; the handle is a tiny sharded one and only lends its stream and its device state.

Per pass: after PUSH  R[pos] bit for bit, Y[pos] within 1 ulp, <r, r>;  after GRAM (where a solve is due) the 78 pair sums in
the kernels' layout -- pair (i, j) at 12 i - i (i - 1) / 2 + (j - i), zeros wherever j >= m;  after STEP and MIX all eight
state words, the error ring and x_out.

Tolerances (derived, not tuned):
  * Gram bound: a sum of products over any tree of depth D is off by at most (D + 1) 2^-53 sum |r_i||r_j|.  From the
    kernels: D = 2 ceil(n / (blocks 512)) + 64 -- a thread adds two products per trip of its grid-stride loop (256 threads
    x 2 elements per block and trip; blocks = 512 for the sweep, 2048 for the push), then at most 6 + 16 + 32 + 6 levels
    across wave, LDS and block partials (anderson_twin.gram_depth).  The error |r|_2 = sqrt(<r, r>) inherits half of the
    relative bound plus the rounding of the root: held to (D + 1) 2^-53 |r|_2.
  * mix tolerance, per element: 4 x the twin's own sensitivity to a Gram perturbation of (D + 17) 2^-53 sum |r_i||r_j|
    plus 4 m 2^-53 sum_j |alpha_j Y_j| (anderson_twin).  tests/test_anderson_twin_cpu.py caps it at 1e-12 max|x| where
    n >= m + 1 and 1e-8 max|x| where n <= m, so it cannot hide a failure.
  * rejected step x = Y_prev + (1 - beta) R_prev: 4 x 2^-53 (|Y_prev| + |(1 - beta) R_prev|).

Measured on an MI355X: profiles/anderson_step_errors.txt (worst device-to-twin error of each case and its ratio to the
tolerance).
"""
import ctypes as C

import numpy as np
import pytest

import anderson_twin as AT

pytestmark = pytest.mark.gpu

PUSH, GRAM, STEP, MIX = range(4)
SENTINEL = -12345.678
U53 = AT.U53
DEV = "cuda"


def sync():
    import torch
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def backends():
    import sdfs_via_autodiff_amd as S
    from sdfs_via_autodiff_amd.distributed import HipStages
    ssy = S.SSY()
    shapes = (2, 2, 2, 2)
    arr = S.discretize_ssy(ssy, shapes)
    bes = [HipStages("ssy", shapes, ssy.params, arr, 0, 0, 2, 1, 0, 2, 0) for _ in range(2)]
    yield bes
    for be in bes:
        be.close()


class Loop:
    """One handle's Anderson loop on n points: the caller-owned history and sums, and the four steps."""

    def __init__(self, be, n, m, tol, max_iter, ridge, mf):
        import torch
        from sdfs_via_autodiff_amd._lib import lib, check
        self.lib, self.chk, self.h, self.torch = lib, check, be._h, torch
        self.n, self.m, self.mf = n, m, mf
        self.Y = torch.full((m, n), SENTINEL, dtype=torch.float64, device=DEV)
        self.R = torch.full((m, n), SENTINEL, dtype=torch.float64, device=DEV)
        self.sums = torch.zeros(1 + AT.NPAIRS, dtype=torch.float64, device=DEV)
        sync()
        check(lib.sdfs_anderson_begin(self.h, n, m, self.Y.data_ptr(), self.R.data_ptr(), float(tol), int(max_iter),
                                      AT.BETA, float(ridge), int(mf)), self.h)

    def step(self, which, i, xi=None, xo=None):
        sync()
        self.chk(self.lib.sdfs_anderson_step(self.h, which, i, xi.data_ptr() if xi is not None else None,
                                             xo.data_ptr() if xo is not None else None, self.sums.data_ptr()), self.h)

    def state(self, first=0, count=0):
        """(the eight words, errors of passes first .. first + count) -- synchronises the handle's stream"""
        st = (C.c_double * 8)()
        errs = (C.c_double * max(count, 1))()
        self.chk(self.lib.sdfs_anderson_state(self.h, st, errs, first, count), self.h)
        return list(st), list(errs)[:count]

    def snapshot(self):
        self.state()
        return [t.clone() for t in (self.Y, self.R, self.sums)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def close_or_both_nan(dev, ref, bound):
    dev, ref = float(dev), float(ref)
    if np.isnan(ref) or np.isnan(dev):
        return bool(np.isnan(ref) and np.isnan(dev))
    if np.isinf(ref) or np.isinf(dev):
        return dev == ref
    return abs(dev - ref) <= float(bound)


def check_state(st, tw, d_push, where):
    want = tw.state()
    for k in (0, 2, 3, 4, 5, 6, 7):
        assert st[k] == want[k], (where, "state word", k, st, want)
    assert close_or_both_nan(st[1], want[1], (d_push + 1) * U53 * abs(want[1]) if np.isfinite(want[1]) else 0.0), (where, st, want)


class Worst:
    """worst device-to-twin error of a case, per quantity: (absolute, ratio to its tolerance)"""

    def __init__(self):
        self.w = {}

    def add(self, key, err, tol):
        err, tol = np.asarray(err, dtype=AT.LD), np.asarray(tol, dtype=AT.LD)
        if err.size == 0:
            return
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
        a, r = float(np.max(err)), float(np.max(ratio))
        pa, pr = self.w.get(key, (0.0, 0.0))
        self.w[key] = (max(pa, a), max(pr, r))

    def line(self, name):
        return f"ANDERSON_STEP {name}: " + "  ".join(f"{k} {a:.3e} ({r:.3f} of tol)" for k, (a, r) in sorted(self.w.items()))


def drive(loops, shards, n, m, mf, ridge, seed, passes, tol=0.0, max_iter=10 ** 6, nan_at=None, name="", extra_closed=3):
    """The schedule on one handle (or on several, each with a shard of the vector and the sums added between the steps),
    every step held to the twin.  Returns (twin, per-pass device errors, Worst)."""
    import torch
    nan_at = nan_at or {}
    tw = AT.AndersonTwin(n, m, tol, max_iter, AT.BETA, ridge, mf, seed=seed)
    d_push, d_sweep = AT.gram_depth(n, AT.PUSH_BLOCKS), AT.gram_depth(n, AT.SWEEP_BLOCKS)
    worst = Worst()
    bounds = np.cumsum([0] + list(shards))
    assert bounds[-1] == n
    x0 = AT.start_iterate(n, seed)
    X = [[torch.from_numpy(x0[a:b].copy()).to(DEV), torch.empty(b - a, dtype=torch.float64, device=DEV)]
         for a, b in zip(bounds[:-1], bounds[1:])]
    sent = [torch.empty(b - a, dtype=torch.float64, device=DEV) for a, b in zip(bounds[:-1], bounds[1:])]
    cat = lambda ts: np.concatenate([t.cpu().numpy() for t in ts])          # noqa: E731

    def all_reduce(lo, hi):
        if len(loops) > 1:
            sync()
            tot = sum(L.sums[lo:hi] for L in loops)
            for L in loops:
                L.sums[lo:hi] = tot
            sync()

    dev_err = {}
    closed_passes = 0
    cur = [x[0] for x in X]
    i = 0
    while i < passes + extra_closed and closed_passes < extra_closed:
        where = f"{name} pass {i}"
        if not tw.open:
            # the loop has ended: a full pass sequence must leave everything bit-unchanged (sentinel in x_out)
            closed_passes += 1
            for s_ in sent:
                s_.fill_(SENTINEL)
            before = [L.snapshot() for L in loops]
            st_before = [L.state(0, AT.RING) for L in loops]
            x_before = cat(cur)
            for L, xi, xo in zip(loops, cur, sent):
                L.step(PUSH, i, xi, xo)
            for L in loops:
                L.step(GRAM, i)
            for L, xo in zip(loops, sent):
                L.step(STEP, i)
                L.step(MIX, i, None, xo)
            for L, b4, s4 in zip(loops, before, st_before):
                st_now = L.state(0, AT.RING)
                assert same_bits(np.array(st_now[0]), np.array(s4[0])) and same_bits(np.array(st_now[1]), np.array(s4[1])), where
                for t_now, t_b4 in zip((L.Y, L.R, L.sums), b4):
                    assert same_bits(t_now.cpu().numpy(), t_b4.cpu().numpy()), (where, "history / sums changed after the end")
            assert same_bits(cat(cur), x_before), where
            assert all(bool((s_ == SENTINEL).all().item()) for s_ in sent), (where, "x_out written after the end")
            i += 1
            continue
        if i >= passes:
            break
        pos = i % m
        xin_t = cur
        xout_t = [x[(i + 1) & 1] for x in X]
        xi = cat(xin_t)
        fx = xi + AT.residual(n, i, seed)
        if i in nan_at:
            fx[nan_at[i]] = np.nan
        for t, (a, b) in zip(xout_t, zip(bounds[:-1], bounds[1:])):
            t.copy_(torch.from_numpy(fx[a:b].copy()))
        # ---- PUSH
        for L, a, b in zip(loops, xin_t, xout_t):
            L.step(PUSH, i, a, b)
        for L in loops:
            L.state()
        p = tw.push(i, xi, fx)
        r64 = fx - xi
        assert same_bits(np.concatenate([L.R[pos].cpu().numpy() for L in loops]), r64), (where, "R[pos] is not fp64 x_out - x_in")
        y_dev = np.concatenate([L.Y[pos].cpu().numpy() for L in loops])
        y_tw = p["Y"]
        fin = np.isfinite(y_tw.astype(np.float64))
        assert np.array_equal(np.isfinite(y_dev), fin), where
        ulp = np.spacing(np.abs(y_tw[fin].astype(np.float64)))
        dy = np.abs(y_dev[fin].astype(AT.LD) - y_tw[fin])
        worst.add("Y[ulp]", dy, ulp)
        assert bool(np.all(dy <= ulp)), (where, "Y[pos] more than 1 ulp off", float(np.max(dy / ulp)))
        rr_dev = sum(float(L.sums[0].item()) for L in loops)           # (what the all-reduce hands every rank)
        b_rr = (d_push + 1) * U53 * float(p["rr_abs"]) if np.isfinite(float(p["rr"])) else 0.0
        if np.isfinite(float(p["rr"])):
            worst.add("<r,r>", abs(AT.LD(rr_dev) - p["rr"]), b_rr)
        assert close_or_both_nan(rr_dev, p["rr"], b_rr), (where, "<r, r>", rr_dev, float(p["rr"]), b_rr)
        all_reduce(0, 1)
        # ---- GRAM
        if (i + 1) % mf == 0:
            for L in loops:
                L.step(GRAM, i)
            for L in loops:
                L.state()
            g = tw.gram()
            if g is not None and np.isfinite(float(p["rr"])):
                g_dev = sum(L.sums[1:].cpu().numpy().astype(AT.LD) for L in loops)
                sums, ab = g
                bound = (d_sweep + 1) * U53 * ab
                inside = np.zeros(AT.NPAIRS, dtype=bool)
                for a in range(m):
                    for b in range(a, m):
                        inside[AT.pair_index(a, b)] = True
                for L in loops:
                    assert bool(np.all(L.sums[1:].cpu().numpy()[~inside] == 0.0)), (where, "a pair sum with j >= m is not 0")
                err = np.abs(g_dev - sums)
                worst.add("Gram", err[inside], bound[inside])
                assert bool(np.all(err <= bound)), (where, "Gram sums", np.argmax(err - bound), float(np.max(err - bound)))
            all_reduce(1, 1 + AT.NPAIRS)
        # ---- STEP, MIX
        for L, b in zip(loops, xout_t):
            L.step(STEP, i)
            L.step(MIX, i, None, b)
        sts = [L.state(i, 1) for L in loops]
        s = tw.step(i)
        for st, _ in sts[1:]:
            assert same_bits(np.array(st), np.array(sts[0][0])), (where, "the ranks' states differ", st, sts[0][0])
        st, ring1 = sts[0]
        check_state(st, tw, d_push, where)
        x_dev = cat(xout_t)
        if s["mode"] == 0:
            assert same_bits(x_dev, fx), (where, "a plain step touched x_out")
        else:
            assert s["tol_x"] is not None and bool(np.all(np.isfinite(x_dev))), where
            err = np.abs(x_dev.astype(AT.LD) - s["x"])
            worst.add("x reject" if s["mode"] == 2 else "x mix", err, s["tol_x"])
            worst.add("tol/max|x|", np.max(s["tol_x"]) / np.max(np.abs(s["x"])), 1.0)
            assert bool(np.all(err <= s["tol_x"])), (where, "x_out", int(np.argmax(err / s["tol_x"])), float(np.max(err / s["tol_x"])))
        if s["mode"] == 2:
            # the poisoned slot: Y[pos] = the iterate the step went back to, R[pos] = 0; no ring entry for this pass
            assert same_bits(np.concatenate([L.Y[pos].cpu().numpy() for L in loops]), x_dev), where
            assert all(bool((L.R[pos] == 0.0).all().item()) for L in loops), where
        else:
            dev_err[i] = st[1]
            assert same_bits(np.array(ring1), np.array([st[1]])), (where, "error ring", ring1, st[1])
        cur = xout_t
        i += 1
    print(worst.line(name))
    return tw, dev_err, worst


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AT.table_cases(), ids=AT.case_id)
def test_steps_follow_the_twin(backends, case):
    n, m, mf, ridge = case
    passes = AT.n_passes(m, mf)
    L = Loop(backends[0], n, m, 0.0, 10 ** 6, ridge, mf)
    tw, _, worst = drive([L], [n], n, m, mf, ridge, AT.CASE_SEEDS.get(case, 0), passes, name=AT.case_id(case))
    assert tw.it == passes and tw.rejected == 0 and tw.status == 0
    assert "x mix" in worst.w and "Gram" in worst.w


# ---- control cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(k for k in AT.CONTROL_CASES if not k.startswith("i_")))
def test_control_cases(backends, name):
    """a / b / c: tol met on a mixing pass (x_out is then the mixed iterate), on a plain pass, max_iter;  e / f: a NaN on the
    pass after a mix (first element; last element of an odd n) is a rejected step, mixing resumes at no_mix_until and not
    before;  g / h: a NaN with no mix to undo ends the loop with status 1.  d: after every end three more pass sequences
    with a sentinel in x_out change nothing (inside drive)."""
    c = AT.CONTROL_CASES[name]
    n, m, mf = c["n"], c["m"], c["mf"]
    L = Loop(backends[0], n, m, c["tol"], c["max_iter"], 1e-6, mf)
    tw, _, worst = drive([L], [n], n, m, mf, 1e-6, 0, c["passes"], tol=c["tol"], max_iter=c["max_iter"], nan_at=c.get("nan_at"),
                         name=name)
    st, _ = L.state()
    assert st[0] == c["ends_at"] and st[6] == c["ends_mixed"], (st, c)
    assert st[4] == c.get("rejected", 0) and st[3] == c.get("status", 0), (st, c)
    if c.get("rejected") and not c.get("status"):
        assert "x reject" in worst.w and st[2] == 1.0
    if name[0] in "abcgh":
        assert st[2] == 0.0                                                # closed: the three no-op sequences ran
    if name.startswith("a_") or name.startswith("c_"):
        assert "x mix" in worst.w and st[6] == 1.0                          # the closing pass mixed, and x_out was held to it


def test_error_ring_wraps_at_256(backends):
    """300 passes with tol = 0: the windows (first, count) of sdfs_anderson_state return the right passes across the wrap."""
    c = AT.CONTROL_CASES["i_ring_wrap"]
    n, m, mf = c["n"], c["m"], c["mf"]
    L = Loop(backends[0], n, m, 0.0, c["max_iter"], 1e-6, mf)
    tw, dev_err, _ = drive([L], [n], n, m, mf, 1e-6, 0, c["passes"], name="i_ring_wrap")
    assert tw.it == 300 and len(dev_err) == 300
    assert len({dev_err[p] for p in range(300)}) == 300                    # no two passes share an error
    for first, count in ((0, 256), (250, 50), (44, 256)):
        _, errs = L.state(first, count)
        # a slot holds the latest pass that maps to it: slots 0 .. 43 those of the passes 256 .. 299
        want = [dev_err[max(p for p in range(300) if p % 256 == (first + k) % 256)] for k in range(count)]
        assert same_bits(np.array(errs), np.array(want)), (first, count)
        if first >= 44:
            assert same_bits(np.array(errs), np.array([dev_err[first + k] for k in range(count)])), (first, count)
        for k in range(count):
            ref = tw.ring[(first + k) % 256]
            assert abs(errs[k] - ref) <= (AT.gram_depth(n, AT.PUSH_BLOCKS) + 1) * U53 * ref, (first, k)


def test_two_ranks_share_one_state(backends):
    """Two handles emulate two ranks: shards of 257 and 300 points of one 557-vector, the sums added between the steps as
    an all-reduce would.  Both states bit-identical after every step, the concatenated iterate held to the twin on the
    whole vector."""
    n, m, mf = 557, 3, 1
    shards = [257, 300]
    loops = [Loop(be, k, m, 0.0, 10 ** 6, 1e-6, mf) for be, k in zip(backends, shards)]
    tw, _, worst = drive(loops, shards, n, m, mf, 1e-6, 0, AT.n_passes(m, mf), name="j_two_ranks")
    assert tw.it == AT.n_passes(m, mf) and "x mix" in worst.w and "Gram" in worst.w


def test_gated_unpack_follows_the_loop_word(backends):
    """sdfs_unpack_blocks_gated, the launch that lands T x in the iterate buffers of the sharded loop: the plain unpack
    while the loop's word is open, nothing at all once the loop has ended (16-byte and 8-byte units)."""
    import torch
    be = backends[0]
    gen = torch.Generator().manual_seed(1)
    for closed in (False, True):
        L = Loop(be, 13, 3, 0.0, 0 if closed else 10, 1e-6, 1)             # max_iter = 0: the loop never opens
        assert L.state()[0][2] == (0.0 if closed else 1.0)
        gate = be.gate_tensor("anderson")
        for shp, axis, offs in (((3, 5, 4), 1, [0, 2, 5]), ((2, 4, 3), 1, [0, 1, 4])):
            x = torch.rand(shp, generator=gen, dtype=torch.float64).to(DEV)
            packed = torch.empty(x.numel(), dtype=torch.float64, device=DEV)
            assert be.pack_blocks(x, packed, axis, offs)
            back = torch.full(shp, SENTINEL, dtype=torch.float64, device=DEV)
            assert be.pack_blocks(back, packed, axis, offs, unpack=True, gate=gate)
            sync()
            want = torch.full_like(x, SENTINEL) if closed else x
            assert torch.equal(back, want), (closed, shp)

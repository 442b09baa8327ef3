"""
Step-wise twin of the device-resident Anderson loop (sdfs_anderson_begin / _step / _state), in numpy long double.

Written from the contract in include/sdfs_hip.h ("Anderson acceleration ... on a SHARDED grid") and the decision rules of
and_step_wave (csrc/anderson_step.hpp) -- a restatement of WHAT a pass does, not of how the kernels add: sums are
numpy's, the (m+1) x (m+1) system is solved by Gaussian elimination with partial pivoting in long double.

The twin runs TEACHER-FORCED: every pass is handed the x_in and x_out = T(x_in) the device saw (fp64), so that an error
of one pass cannot grow over the passes behind it; the history (Y_j = x_j + beta r_j, R_j = r_j) and the control state
are the twin's own.

    tw = AndersonTwin(n, m, tol, max_iter, beta, ridge, mixing_freq)
    p = tw.push(i, x_in, x_out)      # None once the loop has ended;  else pos, R, Y, rr, rr_abs
    g = tw.gram()                    # None unless the step of this pass may mix;  else sums[78], abs[78] (device layout)
    s = tw.step(i)                   # None once the loop has ended;  else mode, x (None on a plain step), tol_x, ...
    tw.state()                       # the eight words of sdfs_anderson_state

Sensitivity.  The device's Gram sums carry the rounding of its summation tree, and the solve amplifies it by the
condition of the bordered system.  For every mixing step the twin therefore redoes its own solve three times with the Gram
block perturbed entrywise (random signs, symmetric) by (D + 17) 2^-53 sum_e |r_i||r_j| -- D the depth of the device's tree,
gram_depth() below; the 17 covers the <= 13 eliminations of the solve on each entry plus the Newton-refined reciprocal --
and reports the largest |dx| per element.  The mix tolerance is 4 x that, plus 4 m 2^-53 sum_j |alpha_j Y_j| for the m
fused multiply-adds of the update (each rounds once, and each Y_j carries the one rounding of its own fma).
"""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
LAZY_M = 12                    # AND_LAZY_M: capacity of the history, and the STRIDE of the pair layout
NPAIRS = LAZY_M * (LAZY_M + 1) // 2
RING = 256                     # slots of the error ring
SWEEP_BLOCKS, PUSH_BLOCKS = 512, 2048


def pair_index(i, j):
    """Where k_and_gram_full leaves <R_i, R_j>, i <= j: rows of the upper triangle of a 12 x 12 matrix, whatever m."""
    assert 0 <= i <= j < LAZY_M
    return LAZY_M * i - i * (i - 1) // 2 + (j - i)


def gram_depth(n, blocks):
    """Depth D of the device's summation tree over n products: a thread adds two products per trip of its grid-stride
    loop, ceil(n / (blocks * 512)) trips (256 threads x 2 elements per block and trip), then at most 6 + 16 + 32 + 6
    levels across the wave, the LDS rows, the block partials and the finishing wave.  A sum over any tree of depth D
    has an error of at most (D + 1) 2^-53 sum |r_i||r_j|.  blocks: 512 for the Gram sweep, 2048 for the push."""
    return 2 * -(-int(n) // (blocks * 512)) + 64


def solve_bordered(G, rho):
    """alpha of [0 1^T; 1 G + rho I] [. ; alpha] = [1; 0], Gaussian elimination with partial pivoting in long double.
    None if a pivot column is all zeros (the device then does not mix)."""
    m = G.shape[0]
    d = m + 1
    A = np.zeros((d, d), dtype=LD)
    A[0, 1:] = 1
    A[1:, 0] = 1
    A[1:, 1:] = G + LD(rho) * np.eye(m, dtype=LD)
    b = np.zeros(d, dtype=LD)
    b[0] = 1
    for c in range(d):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if not (np.abs(A[p, c]) > 0):
            return None
        if p != c:
            A[[c, p]] = A[[p, c]]
            b[[c, p]] = b[[p, c]]
        for r in range(c + 1, d):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            b[r] -= f * b[c]
    x = np.zeros(d, dtype=LD)
    for r in range(d - 1, -1, -1):
        x[r] = (b[r] - A[r, r + 1:] @ x[r + 1:]) / A[r, r]
    return x[1:]


class AndersonTwin:
    def __init__(self, n, m, tol, max_iter, beta, ridge, mixing_freq, seed=0):
        assert 1 <= m <= LAZY_M and mixing_freq >= 1
        self.n, self.m, self.tol, self.max_iter = int(n), int(m), float(tol), int(max_iter)
        self.beta, self.ridge, self.mf = LD(beta), float(ridge), int(mixing_freq)
        self.Y = np.zeros((m, n), dtype=LD)
        self.R = np.zeros((m, n), dtype=LD)
        self.it, self.err = 0, np.inf
        self.open = max_iter > 0 and self.err > tol
        self.status, self.rejected, self.no_mix_until, self.last_mixed, self.prev_pos = 0, 0, 0, 0, -1
        self.ring = [None] * RING           # error ring: None = never written
        self.depth = gram_depth(n, SWEEP_BLOCKS)
        self.rng = np.random.default_rng(seed)
        self._rr = None
        self._pos = None
        self._gram_cache = None

    # -- the loop's own test: may the step of the pass that is running mix?  (state BEFORE that step)
    def mix_due(self):
        it1 = self.it + 1
        return it1 >= self.m and it1 >= self.no_mix_until and it1 % self.mf == 0

    def state(self):
        return [float(self.it), float(self.err), 1.0 if self.open else 0.0, float(self.status), float(self.rejected),
                float(self.no_mix_until), float(self.last_mixed), float(self.prev_pos)]

    def push(self, i, x_in, x_out):
        if not self.open:
            return None
        pos = i % self.m
        x = np.asarray(x_in, dtype=np.float64).astype(LD)
        fx = np.asarray(x_out, dtype=np.float64).astype(LD)
        with np.errstate(invalid="ignore"):
            r = fx - x
            self.R[pos] = r
            self.Y[pos] = x + self.beta * r
            self._rr = r @ r
        self._pos = pos
        self._gram_cache = None
        return dict(pos=pos, R=self.R[pos], Y=self.Y[pos], rr=self._rr, rr_abs=self._rr)

    def _gram(self):
        if self._gram_cache is None:                         # (one per pass: the history only changes in push / a rejection)
            with np.errstate(invalid="ignore"):
                self._gram_cache = (self.R @ self.R.T, np.abs(self.R) @ np.abs(self.R).T)
        return self._gram_cache

    def gram(self):
        """The 78 sums in the device's layout (and sum |r_i||r_j| for the bound), where the step of this pass may mix."""
        if not self.open or not self.mix_due():
            return None
        G, A = self._gram()
        sums = np.zeros(NPAIRS, dtype=LD)
        ab = np.zeros(NPAIRS, dtype=LD)
        for i in range(self.m):
            for j in range(i, self.m):
                sums[pair_index(i, j)] = G[i, j]
                ab[pair_index(i, j)] = A[i, j]
        return sums, ab

    def _mix(self, G, rho):
        alpha = solve_bordered(G, rho)
        if alpha is None:
            return None, None
        return alpha, alpha @ self.Y

    def step(self, i):
        if not self.open:
            return None
        m, pos = self.m, i % self.m
        assert pos == self._pos, "push first"
        it = self.it
        with np.errstate(invalid="ignore"):
            err = float(np.sqrt(self._rr))
        finite = bool(np.isfinite(err))
        out = dict(pos=pos, x=None, tol_x=None, alpha=None, sens=None)
        if not finite and self.last_mixed and self.prev_pos >= 0 and self.rejected < 1000:
            # a mixing step left the domain: plain step from the last good iterate, the poisoned slot cleared
            pp = self.prev_pos
            x = self.Y[pp] + (1 - self.beta) * self.R[pp]
            # device: Y_prev carries one rounding, the fma another
            out.update(mode=2, x=x, tol_x=4 * U53 * (np.abs(self.Y[pp]) + np.abs((1 - self.beta) * self.R[pp])))
            self.Y[pos] = x
            self.R[pos] = 0
            self._gram_cache = None
            self.rejected += 1
            self.no_mix_until = it + 1 + m
            self.last_mixed = 0
            err = self.err                                   # the previous pass's; prev_pos stays; no ring entry
            self.open = err > self.tol and it + 1 < self.max_iter
        else:
            mixed = False
            if self.mix_due() and finite:
                G, A = self._gram()
                rho = self.ridge if self.ridge >= 0 else -self.ridge * float(np.trace(G)) / m
                alpha, x = self._mix(G, rho)
                if alpha is not None:
                    mixed = True
                    pert = LD((self.depth + 17) * U53) * A
                    sens = np.zeros(self.n, dtype=LD)
                    for _ in range(3):
                        s = np.triu(self.rng.choice([-1.0, 1.0], size=(m, m)))
                        s = s + np.triu(s, 1).T
                        rho_p = rho if self.ridge >= 0 else -self.ridge * float(np.trace(G + s * pert)) / m
                        a2, x2 = self._mix(G + s * pert, rho_p)
                        sens = np.maximum(sens, np.abs(x2 - x)) if a2 is not None else np.full(self.n, np.inf, dtype=LD)
                    acc = np.abs(alpha)[:, None] * np.abs(self.Y)
                    out.update(x=x, alpha=alpha, sens=sens, tol_x=4 * sens + 4 * m * U53 * acc.sum(axis=0))
            out["mode"] = 1 if mixed else 0
            self.last_mixed = 1 if mixed else 0
            self.prev_pos = pos
            self.ring[i % RING] = err
            if not finite:
                self.status = 1
                self.open = False
            else:
                self.open = err > self.tol and it + 1 < self.max_iter
        self.err = err
        self.it = it + 1
        return out


# ---- prescribed residual schedules (shared by the CPU and the GPU tests) -------------------------------------------------
def residual_scale(i):
    """|r_i|_2 / sqrt(n) of pass i: 15 % smaller per pass (errors in strict order: a tol between two of them closes the
    loop on a chosen pass), starting over every 24 passes, 1 % higher each time, so that a long run never falls below the
    iterate's last bits and no two passes of it have the same norm."""
    return 2.0 * 0.85 ** (i % 24) * (1.0 + 0.01 * (i // 24))


def start_iterate(n, seed):
    return 600.0 + 100.0 * np.random.default_rng([seed, n, 1]).random(n)


def residual(n, i, seed):
    """r_i = s_i N(0, 1), the last element and those at 511 and 512 (where they exist) x 8 -- a dropped or doubled tail
    element then moves every sum by far more than the bound --, scaled to |r_i|_2 = residual_scale(i) sqrt(n)."""
    g = np.random.default_rng([seed, n, 2, i]).standard_normal(n)
    for k in (n - 1, 511, 512):
        if 0 <= k < n:
            g[k] *= 8.0
    nrm = float(np.sqrt(g @ g))
    if nrm == 0.0:
        g[:] = 1.0
        nrm = float(np.sqrt(n))
    return g * (residual_scale(i) * np.sqrt(n) / nrm)


def n_passes(m, mixing_freq):
    return m + 2 * mixing_freq + 3


# the table of the step test: (n, m, mixing_freq, ridge)
def table_cases():
    cases = []
    for n in (1, 2, 3):
        for m in (1, 2, 3, 12):
            cases.append((n, m, 1, 1e-6))
    for m in (1, 2, 5, 10, 12):
        for ridge in (1e-6, -1e-10):
            cases.append((13, m, 1 if m == 1 else 4, ridge))     # (relative ridge: n = 13 >= m + 1 throughout)
    for n in (511, 512, 513):
        for m in (3, 12):
            cases.append((n, m, 1, 1e-6))
    cases.append((1025, 10, 4, 1e-6))
    cases.append((262657, 12, 4, 1e-6))
    cases.append((1049091, 5, 4, 1e-6))
    return cases


def case_id(c):
    n, m, mf, ridge = c
    return f"n{n}-m{m}-f{mf}-{'rel' if ridge < 0 else 'abs'}"


BETA = 8.0            # the reference's (jaxopt) mixing parameter
CAP_FULL, CAP_DEFICIENT = 1e-12, 1e-8      # x max|x|: caps on the mix tolerance where n >= m + 1 / n <= m


# table case -> seed of its schedule where seed 0 is not used.  (1, 3): seed 0 left the twin at 8.7e-9 max|x|, a hair inside
# its cap of 1e-8 (a rank-1 Gram matrix under three slots); seed 2 stays at 1.1e-10.
CASE_SEEDS = {(1, 3, 1, 1e-6): 2}


def tol_closing_at(n, p):
    """A tol the residual norm first meets on pass p: 5 % above |r_p|, 10 % below |r_(p-1)| (p < 24)."""
    return 1.05 * residual_scale(p) * float(np.sqrt(n))


# control cases of the step test (m = 3): name -> schedule and where it must end.  nan_at: {pass: index} of a NaN put
# into x_out.  Mixing is due on the passes i with i + 1 >= 3 and (i + 1) % mf == 0: 3, 5, 7, 9 for mf = 2.
_BIG = 10 ** 6
CONTROL_CASES = {
    "a_tol_on_mixing_pass": dict(n=513, m=3, mf=2, passes=10, tol=tol_closing_at(513, 5), max_iter=_BIG, ends_at=6, ends_mixed=1),
    "b_tol_on_plain_pass": dict(n=13, m=3, mf=2, passes=10, tol=tol_closing_at(13, 6), max_iter=_BIG, ends_at=7, ends_mixed=0),
    "c_max_iter": dict(n=13, m=3, mf=2, passes=10, tol=0.0, max_iter=6, ends_at=6, ends_mixed=1),
    "e_rejected_first_element": dict(n=13, m=3, mf=2, passes=10, tol=0.0, max_iter=_BIG, nan_at={4: 0}, ends_at=10,
                                     ends_mixed=1, rejected=1),
    "f_rejected_odd_tail": dict(n=513, m=3, mf=2, passes=10, tol=0.0, max_iter=_BIG, nan_at={4: 512}, ends_at=10,
                                ends_mixed=1, rejected=1),
    "g_nan_after_rejection": dict(n=13, m=3, mf=2, passes=8, tol=0.0, max_iter=_BIG, nan_at={4: 0, 5: 0}, ends_at=6,
                                  ends_mixed=0, rejected=1, status=1),
    "h_nan_on_pass_0": dict(n=13, m=3, mf=2, passes=3, tol=0.0, max_iter=_BIG, nan_at={0: 0}, ends_at=1, ends_mixed=0, status=1),
    "i_ring_wrap": dict(n=13, m=3, mf=1, passes=300, tol=0.0, max_iter=_BIG, ends_at=300, ends_mixed=1),
}


def run_on_twin(n, m, mixing_freq, ridge, seed, passes=None, tol=0.0, max_iter=_BIG, nan_at=None):
    """The schedule on the twin alone (its own iterate, rounded to fp64, fed back): per mixing step the largest
    tolerance relative to max|x|.  What the CPU test holds to the caps."""
    tw = AndersonTwin(n, m, tol, max_iter, BETA, ridge, mixing_freq, seed=seed)
    x = start_iterate(n, seed)
    ratios = []
    for i in range(n_passes(m, mixing_freq) if passes is None else passes):
        fx = x + residual(n, i, seed)
        if nan_at and i in nan_at:
            fx[nan_at[i]] = np.nan
        if tw.push(i, x, fx) is None:
            break
        s = tw.step(i)
        if s["mode"] == 1:
            ratios.append(float(np.max(s["tol_x"]) / np.max(np.abs(s["x"]))))
        x = fx if s["x"] is None else np.asarray(s["x"], dtype=np.float64)
    return tw, ratios

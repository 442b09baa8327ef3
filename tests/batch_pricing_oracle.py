"""
Helper of tests/test_batch_pricing_cpu.py and tests/test_hip_batch_pricing.py (not a test module): the stages of
csrc/batch_price.hpp and the 12 words of its moment block restated in numpy on top of ``folded_K`` and ``dense_chain`` of
tests/test_pricing_cpu.py, with T w from extended precision (``extended_Tw`` says why ``oracle_T``'s is not enough).

    E_M = K(1, θ, −γ)·1, E_M2 = K(2, 2θ, −2γ)·1, v = (I − K_κ)⁻¹ K_κ·1 with K_κ = K(1, θ, κ−γ),
    ER = K(0, 0, κ)(1 + v) / v, P_n = K(1, θ, κ_ts−γ) P_{n−1}

    words: 0 Σg | 1 ⟨g,log_rf⟩ 2 ⟨g,log_rf²⟩ | 3 ⟨g,hj⟩ | 4 ⟨g,ln v⟩ 5 ⟨g,(ln v)²⟩ | 6 ⟨g,ln ER⟩ | 7 ⟨g,lp⟩ 8 ⟨g,lp²⟩ |
           9 min v 10 max v | 11 number of points with v ≤ 0

``words`` also returns Σ|terms| of every sum: the scale of the tolerance of a fixed-order fp64 summation.
"""
import numpy as np

from oracle import gcy as ogcy, ssy as ossy
from test_pricing_cpu import dense_chain, folded_K, pieces

WORDS = 12
# (axis of h_lam, axis of h_c), and the grid axes of the a3 table in its layout's order (slowest first)
AXES = {"ssy": (0, 1), "gcy": (5, 3)}


def discretize(S, kind, model, shapes):
    return (S.discretize_ssy if kind == "ssy" else S.discretize_gcy)(model, shapes)


def point_weights(per_axis):
    """The weight of every grid point, ∏_a g_a[i_a], from the per-axis vectors."""
    gw = np.asarray(per_axis[0], dtype=np.float64)
    for v in per_axis[1:]:
        gw = np.multiply.outer(gw, np.asarray(v, dtype=np.float64))
    return gw


def extended_Tw(kind, shapes, model, arrays, w):
    """T w = 1 + β (a3 a2 H0(a1 w^θ))^(1/θ) evaluated in extended precision (np.longdouble) and rounded to fp64.

    ``folded_K`` raises T w − 1 to the power 1 − θ (17 for SSY, 37 for GCY), so a relative error e of T w − 1 is an error
    (1 − θ) e of every K it returns.  ``oracle_T`` in fp64 is accurate to a few ulp, but not without bias: its exponent
    1/θ is rounded once for all points, which shifts T w − 1 by (δ/θ) ln(a3 S) with |ln(a3 S)| ≈ 224 at GCY, the same
    sign everywhere.  Through the power that is 1.15e-14 on every application of K at GCY 3⁶, and ln P_n / n returns it
    undivided: above the 1e-14 the yields are held to.  With T w rounded from extended precision ``folded_K`` agreed with
    an extended-precision restatement of the horizons to 2e-16 there (tests/test_batch_pricing_cpu.py holds the offset
    between the two T w: its size and that it is the same at every horizon)."""
    L = np.longdouble
    beta, theta, gamma, mu_c, hl, sc, zz, _ = pieces(kind, model, arrays)
    if kind == "ssy":
        _, Ql, _, Qc, _, Qz, _, zQ, _, _ = arrays
        Q = tuple(np.asarray(q, dtype=L) for q in (Ql, Qc, Qz, zQ))
        H0 = lambda x: ossy.expect_ssy(x, Q)             # noqa: E731
    else:
        _, zQ, _, zpQ, _, Qhz, _, _, Qhc, _, _, Qhzp, _, _, Qhl = arrays
        Q = tuple(np.asarray(q, dtype=L) for q in (zQ, zpQ, Qhz, Qhc, Qhzp, Qhl))
        H0 = lambda x: ogcy.expect_gcy(x, Q)             # noqa: E731
    hl, sc, zz, w = (np.asarray(x, dtype=L) for x in (hl, sc, zz, w))
    beta, theta, gamma, mu_c = L(beta), L(theta), L(gamma), L(mu_c)
    a1 = np.exp(theta * hl)
    a2 = np.exp(L(0.5) * (1 - gamma) ** 2 * sc * sc)
    a3 = np.exp((1 - gamma) * (mu_c + zz))
    S = a2 * H0(a1 * w ** theta)
    Tw = 1 + beta * (a3 * S) ** (1 / theta)
    assert Tw.dtype == L and np.finfo(L).eps < 1e-18, "extended precision is not available"
    return np.broadcast_to(Tw, shapes).astype(np.float64)


class Member:
    """One member at w: K(p, κ_λ, κ_c) by ``folded_K`` with T w computed once (``extended_Tw``)."""

    def __init__(self, kind, shapes, model, arrays, w):
        self.kind, self.shapes, self.model, self.arrays, self.w = kind, tuple(shapes), model, arrays, w
        self.Tw = extended_Tw(kind, self.shapes, model, arrays, w)
        self.theta, self.gamma = model.θ, model.γ

    def K(self, f, p, kl, kc):
        return folded_K(self.kind, self.shapes, self.model, self.arrays, self.w, f, p, kl, kc, Tw=self.Tw)

    def K_claim(self, f, kappa):
        return self.K(f, 1, self.theta, kappa - self.gamma)

    def E_M(self):
        return self.K(np.ones(self.shapes), 1, self.theta, -self.gamma)

    def E_M2(self):
        return self.K(np.ones(self.shapes), 2, 2.0 * self.theta, -2.0 * self.gamma)

    def ER(self, v, kappa):
        return self.K(1.0 + v, 0, 0.0, kappa) / v

    def claim_residual(self, v, kappa):
        """K_κ·1 − (v − K_κ v) and K_κ·1."""
        k1 = self.K_claim(np.ones(self.shapes), kappa)
        return k1 - (v - self.K_claim(v, kappa)), k1

    def dense(self, p, kl, kc):
        """K(p, κ_λ, κ_c) as an N × N matrix: the folded form's two diagonal scalings around the dense chain."""
        beta, theta, gamma, mu_c, hl, sc, zz, _ = pieces(self.kind, self.model, self.arrays)
        c1 = self.w ** (theta - 1.0)
        c2 = beta ** theta * (self.Tw - 1.0) ** (1.0 - theta)
        right = np.broadcast_to(c1 ** p * np.exp(kl * hl), self.shapes).reshape(-1)
        left = np.broadcast_to(c2 ** p * np.exp(0.5 * kc * kc * sc * sc + kc * (mu_c + zz)), self.shapes).reshape(-1)
        return left[:, None] * dense_chain(self.kind, self.shapes, self.arrays) * right[None, :]

    def horizons(self, kappa_ts, n_max, gw):
        """Rows (⟨g,P_n⟩, ⟨g,−ln P_n⟩ / n, min and max of P_n / P_{n−1}) for n = 1 … n_max by repeated ``folded_K``."""
        P = np.ones(self.shapes)
        out = np.empty((n_max, 4))
        for n in range(1, n_max + 1):
            Pn = self.K(P, 1, self.theta, kappa_ts - self.gamma)
            ratio = Pn / P
            out[n - 1] = np.sum(gw * Pn), np.sum(gw * -np.log(Pn)) / n, ratio.min(), ratio.max()
            P = Pn
        return out


def stages(mem, kappa, v=None):
    """The grids of the stages: {"E_M", "E_M2", "pd", "expected_return"}.  ``v`` None: the dense solve of
    (I − K_κ) v = K_κ·1; ``kappa`` None: no claim (pd and expected_return are None)."""
    out = {"E_M": mem.E_M(), "E_M2": mem.E_M2(), "pd": None, "expected_return": None}
    if kappa is not None:
        if v is None:
            Kd = mem.dense(1, mem.theta, kappa - mem.gamma)
            v = np.linalg.solve(np.eye(Kd.shape[0]) - Kd, Kd.sum(axis=1)).reshape(mem.shapes)
        out["pd"] = v
        out["expected_return"] = mem.ER(v, kappa) if np.all(v > 0) else None
    return out


def words(gw, E_M, E_M2, v=None, ER=None):
    """(words, scale): the 12 words from the grids, and Σ|terms| of every sum (0 for words 9-11, which are exact).
    ``v`` None: no claim, words 4-11 NaN; ``ER`` None with a ``v``: no finite price, words 4-8 NaN."""
    out = np.full(WORDS, np.nan)
    scale = np.zeros(WORDS)

    def put(i, terms):
        out[i] = np.sum(terms)
        scale[i] = np.sum(np.abs(terms))
    lr = -np.log(E_M)
    put(0, gw)
    put(1, gw * lr)
    put(2, gw * lr * lr)
    put(3, gw * np.sqrt(np.maximum(E_M2 / E_M ** 2 - 1.0, 0.0)))
    if v is not None:
        out[9], out[10], out[11] = v.min(), v.max(), float(np.sum(~(v > 0)))
        if ER is not None:
            lv, le = np.log(v), np.log(ER)
            lp = le + np.log(E_M)
            put(4, gw * lv)
            put(5, gw * lv * lv)
            put(6, gw * le)
            put(7, gw * lp)
            put(8, gw * lp * lp)
    return out, scale


def batch_form_K(kind, shapes, model, arrays, w, f, p, kl, kc):
    """K(p, κ_λ, κ_c) f in the form of the batch kernels: d2 ⊙ H(d1 ⊙ f) with H = a2 ⊙ H0(a1 ⊙ ·) (a1 and a2 folded into
    the matrices, a3 left out), c_in = w^θ / w, c_out = β a3 (a3 S)^(1/θ) / (a3 S), S = H(w^θ), and the three tables
    t1 = exp((κ_λ − θ) h_λ), t2 = exp(½(κ_c² − (1−γ)²) σ_c²), t3 = exp((κ_c − p(1−γ))(μ_c + z))."""
    beta, theta, gamma, mu_c, hl, sc, zz, H0 = pieces(kind, model, arrays)
    a1 = np.exp(theta * hl)
    a2 = np.exp(0.5 * (1.0 - gamma) ** 2 * sc * sc)
    a3 = np.exp((1.0 - gamma) * (mu_c + zz))

    def H(x):
        return a2 * H0(a1 * x)
    S = H(w ** theta)
    c_in = w ** theta / w
    c_out = beta * a3 * (a3 * S) ** (1.0 / theta) / (a3 * S)
    t1 = np.exp((kl - theta) * hl)
    t2 = np.exp(0.5 * (kc * kc - (1.0 - gamma) ** 2) * sc * sc)
    t3 = np.exp((kc - p * (1.0 - gamma)) * (mu_c + zz))
    d1 = c_in ** p * t1
    d2 = c_out ** p * t2 * t3
    return d2 * H(d1 * f)

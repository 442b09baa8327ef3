"""
Elementwise error bound of one reduced-precision J.v product (the storage forms of Newton's inner solve, opts.krylov_f32),
shared by tests/test_f32_bounds_cpu.py, which pins it against a numpy emulation and four deliberate faults, and
tests/test_hip_f32_forms.py, which holds the library's kernels to it.

Derivation.  J(w) = diag(c2) H diag(c1) with c1 = a1 w^(theta-1) > 0, c2 = beta (K S)^(1/theta-1) K > 0 and
H = H0 >= 0 the product of the per-axis transition matrices (oracle/ssy.py, oracle/gcy.py: jvp_*).  Every factor is
non-negative, so a relative rounding error delta (|delta| <= u) made anywhere on the way from v to J v moves each output
by at most |delta| times the same chain applied to |v|: J|v| is an exact elementwise scale for rounding errors.

One product in the storage forms (v already a float, and the reference `want` uses the same rounded v):
  * c1 and c2 are computed in fp64 and stored once as floats, scaled by a power of two (exact): 2 roundings;
  * pass 1 forms c1 v and contracts its two axes, every later pass contracts two more; each pass but the last stores its
    result as floats: one rounding per intermediate (1 in 4-D, 2 in 6-D);
  * the last pass multiplies by c2, subtracts v when m = 1 (minus_identity) and stores a float: one rounding on
    |J v - m v| <= J|v| + m|v|.
That is at most 5 relative roundings of size u, and (1 + u)^5 - 1 < 8u: C = 8 leaves room for the fp64 arithmetic in
between (~1e-16 relative) and for the bf16 form's double rounding (float, then bfloat16: u (1 + 2^-16)).

  opts.krylov_f32 = 1: fp32 storage, fp64 arithmetic:           u = 2^-24, C = 8
  opts.krylov_f32 = 2: every stored float rounded to bfloat16:  u = 2^-8,  C = 8
  opts.krylov_f32 = 3: fp32 LDS tiles and fp32 MFMA (v_mfma_f32_16x16x4_f32, fp32 accumulation): each contraction of
      n_a terms adds at most gamma_{n_a} ~ n_a u relative to the same sum of absolute values (again a positive chain),
      so C = 8 + sum_a n_a.  Only where the fp32-MFMA kernels run: on a plan without them (generic, small-grid, padded
      plans) krylov_f32 = 3 runs exactly as 1 and keeps C = 8.

Bound:  |got - want|_i <= C u ((J|v|)_i + m |v_i|).
"""
import numpy as np

U = {1: 2.0 ** -24, 2: 2.0 ** -8, 3: 2.0 ** -24}


def constant(mode, shapes, mfma_ran):
    """C of the derivation above for storage mode 1, 2 or 3 on `shapes`; mfma_ran: the fp32-MFMA kernels ran."""
    return 8 + (sum(int(n) for n in shapes) if mode == 3 and mfma_ran else 0)


def bound(jabs_v, v, m, C, u):
    return C * u * (np.abs(jabs_v) + (np.abs(v) if m else 0.0))


def ratio(got, want, jabs_v, v, m, C, u):
    """max_i |got - want|_i / bound_i (<= 1: the bound holds)."""
    b = bound(jabs_v, v, m, C, u)
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    if np.any((b == 0) & (err != 0)):
        return np.inf
    return float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0)))


def measured(got, want, jabs_v, v, m, u):
    """max_i |got - want|_i / (u ((J|v|)_i + m |v_i|)): the measured value of C (reported by the GPU tests)."""
    return ratio(got, want, jabs_v, v, m, 1.0, u)


def check(got, want, jabs_v, v, m, C, u, what):
    r = ratio(got, want, jabs_v, v, m, C, u)
    assert r <= 1.0, f"{what}: error {r:.3g} x the bound C u (J|v| + m|v|), C = {C}, u = {u:.3g}"
    return r


# -- fp32 residual of one application of T in opts.t_f32 (tests/test_hip_f32_forms.py (d)) ----------------------------
def t32_bound(T, theta, u=2.0 ** -24):
    """|T32 - T|_i <= 8 u (T_i - 1) / |theta|: T = 1 + beta (K S)^(1/theta), the intermediates of S stored as floats
    (a relative error e on S becomes e / theta on T - 1), up to 5 roundings as for J.v."""
    return 8 * u * (np.asarray(T) - 1.0) / abs(theta)

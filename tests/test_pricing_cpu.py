"""
CPU tests of the asset-pricing layer (sdfs_via_autodiff_amd/pricing.py):

 (1) the folded tilted expectation K(p, κ_λ, κ_c) f = d2 ⊙ H'(d1 ⊙ f) -- the form the library evaluates on the J·v
     kernels -- against a literal dense SDF M' = β^θ exp(θ g_λ' − γ g_c') (w(X') / (Tw(x) − 1))^(θ−1) with
     Gauss–Hermite quadrature over the consumption shock, on SSY 3×3×3×5 and a ragged GCY grid;
 (2) K(1, θ, 1−γ) against the oracle's J·v, and the physical moments E_x[1] = 1, E_x[G_c] = exp(μ_c + z + σ_c²/2);
 (3) ``stationary_weights`` against the left Perron vector of the dense chain, and its refusal when a conditional
     tensor's slices differ;
 (4) the argument checks, which run before any device work (this machine has no GPU to reach).

``folded_K`` and ``dense_chain`` are the numpy oracle of tests/test_hip_pricing.py as well.
"""
import numpy as np
import pytest

import sdfs_via_autodiff_amd as S
from oracle import ssy as ossy, gcy as ogcy


def model_of(kind):
    return S.SSY() if kind == "ssy" else S.GCY()


def pieces(kind, model, arrays):
    """(beta, theta, gamma, mu_c, h_lam, sigma_c, z) broadcast to the grid's axes, and H0 (the pure expectation)."""
    if kind == "ssy":
        p = model.params
        beta, gamma, mu_c = p[0], p[1], p[3]
        h_l, Ql, _, Qc, _, Qz, z, zQ, sig_c, _ = arrays
        hl = np.asarray(h_l)[:, None, None, None]
        sc = np.asarray(sig_c)[None, :, None, None]
        zz = np.asarray(z)[None, None, :, :]
        H0 = lambda x: ossy.expect_ssy(x, (Ql, Qc, Qz, zQ))          # noqa: E731
    else:
        p = model.params
        beta, gamma, mu_c = p[0], p[2], p[5]
        z, zQ, _, zpQ, _, Qhz, _, _, Qhc, sig_c, _, Qhzp, _, h_l, Qhl = arrays
        hl = np.asarray(h_l)[None, None, None, None, None, :]
        sc = np.asarray(sig_c)[None, None, None, :, None, None]
        zz = np.transpose(np.asarray(z), (3, 0, 1, 2))[:, :, :, None, :, None]     # [b,c,e,a] -> [a,b,c,.,e,.]
        H0 = lambda x: ogcy.expect_gcy(x, (zQ, zpQ, Qhz, Qhc, Qhzp, Qhl))      # noqa: E731
    return beta, model.θ, gamma, mu_c, hl, sc, zz, H0


def oracle_T(kind, shapes, model, arrays, w):
    f = ossy.T_ssy_factorised if kind == "ssy" else ogcy.T_gcy_factorised
    return f(w, shapes, model.params, arrays)


def folded_K(kind, shapes, model, arrays, w, f, p, kl, kc, Tw=None):
    """K f = c2^p exp(½κ_c²σ_c² + κ_c(μ_c + z)) ⊙ H0(c1^p exp(κ_λ h_λ) ⊙ f), c1 = w^(θ−1), c2 = β^θ (Tw − 1)^(1−θ)."""
    beta, theta, gamma, mu_c, hl, sc, zz, H0 = pieces(kind, model, arrays)
    if Tw is None:
        Tw = oracle_T(kind, shapes, model, arrays, w)
    c1 = w ** (theta - 1.0)
    c2 = beta ** theta * (Tw - 1.0) ** (1.0 - theta)
    cur = np.exp(0.5 * kc * kc * sc * sc + kc * (mu_c + zz))
    return c2 ** p * cur * H0(c1 ** p * np.exp(kl * hl) * f)


def dense_chain(kind, shapes, arrays):
    """The N × N transition matrix of the discretised chain (C order on both sides)."""
    N = int(np.prod(shapes))
    if kind == "ssy":
        _, Ql, _, Qc, _, Qz, _, zQ, _, _ = arrays
        P = np.einsum("lL,kK,iI,ijJ->lkijLKIJ", Ql, Qc, Qz, zQ)
    else:
        _, zQ, _, zpQ, _, Qhz, _, _, Qhc, _, _, Qhzp, _, _, Qhl = arrays
        P = np.einsum("bceaA,ebB,cC,dD,eE,fF->abcdefABCDEF", zQ, zpQ, Qhz, Qhc, Qhzp, Qhl)
    return P.reshape(N, N)


def dense_K(kind, shapes, model, arrays, w, p, kl, kc, nodes=60):
    """K as an N × N matrix from the literal SDF, the consumption shock integrated by Gauss–Hermite quadrature:
    K[x, X'] = P(x, X') Σ_q ω_q M'(x, X', ξ_q)^p exp((κ_λ − pθ) h_λ' + (κ_c + pγ) g_c'(x, ξ_q)) w(X')^0."""
    beta, theta, gamma, mu_c, hl, sc, zz, _ = pieces(kind, model, arrays)
    N = int(np.prod(shapes))
    Tw = oracle_T(kind, shapes, model, arrays, w)
    xi, om = np.polynomial.hermite_e.hermegauss(nodes)
    om = om / np.sqrt(2.0 * np.pi)
    hl_n = np.broadcast_to(hl, shapes).reshape(N)                 # h_λ of the next state
    mu = np.broadcast_to(mu_c + zz, shapes).reshape(N)            # μ_c + z of the current state
    sg = np.broadcast_to(sc, shapes).reshape(N)                   # σ_c of the current state
    wn = w.reshape(N)
    Tc = Tw.reshape(N)
    gc = mu[:, None] + sg[:, None] * xi[None, :]                  # g_c'(x, ξ_q)
    out = np.zeros((N, N))
    for q in range(nodes):
        M = (beta ** theta * np.exp(theta * hl_n[None, :] - gamma * gc[:, q][:, None])
             * (wn[None, :] / (Tc[:, None] - 1.0)) ** (theta - 1.0))
        out += om[q] * M ** p * np.exp((kl - p * theta) * hl_n[None, :] + (kc + p * gamma) * gc[:, q][:, None])
    return dense_chain(kind, shapes, arrays) * out


def tilts(model):
    th, g = model.θ, model.γ
    return [(1, th, -g), (2, 2 * th, -2 * g), (1, th, 2 - g), (0, 0.0, 1.0)]


SHAPES = [("ssy", (3, 3, 3, 5)), ("gcy", (2, 3, 2, 3, 2, 3))]


def grid_w(shapes, seed=0):
    rng = np.random.default_rng(seed)
    return 500.0 + 400.0 * rng.random(shapes)


@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_folded_K_matches_literal_dense_sdf(kind, shapes):
    m = model_of(kind)
    arr = (S.discretize_ssy if kind == "ssy" else S.discretize_gcy)(m, shapes)
    w = grid_w(shapes)
    f = 0.5 + np.random.default_rng(1).random(shapes)
    for p, kl, kc in tilts(m):
        got = folded_K(kind, shapes, m, arr, w, f, p, kl, kc)
        want = (dense_K(kind, shapes, m, arr, w, p, kl, kc) @ f.reshape(-1)).reshape(shapes)
        rel = np.max(np.abs(got - want) / np.abs(want))
        assert rel < 1e-13, f"tilt {(p, kl, kc)}: relative difference {rel:.2e}"


@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_K_at_consumption_tilt_is_the_jacobian_and_physical_moments(kind, shapes):
    m = model_of(kind)
    arr = (S.discretize_ssy if kind == "ssy" else S.discretize_gcy)(m, shapes)
    w = grid_w(shapes, 2)
    v = np.random.default_rng(3).standard_normal(shapes)
    jvp = ossy.jvp_ssy if kind == "ssy" else ogcy.jvp_gcy
    want = jvp(w, v, shapes, m.params, arr)
    got = folded_K(kind, shapes, m, arr, w, v, 1, m.θ, 1 - m.γ)
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
    one = np.ones(shapes)
    assert np.max(np.abs(folded_K(kind, shapes, m, arr, w, one, 0, 0.0, 0.0) - 1.0)) < 1e-14
    _, _, _, mu_c, _, sc, zz, _ = pieces(kind, m, arr)
    eg = folded_K(kind, shapes, m, arr, w, one, 0, 0.0, 1.0)
    np.testing.assert_allclose(eg, np.broadcast_to(np.exp(mu_c + zz + 0.5 * sc * sc), shapes), rtol=1e-14)


@pytest.mark.parametrize("kind,shapes", SHAPES)
def test_stationary_weights_are_the_dense_left_perron_vector(kind, shapes):
    m = model_of(kind)
    arr = (S.discretize_ssy if kind == "ssy" else S.discretize_gcy)(m, shapes)
    g = S.stationary_weights(m, shapes)
    assert [len(x) for x in g] == list(shapes)
    pi = g[0]
    for x in g[1:]:
        pi = np.multiply.outer(pi, x)
    P = dense_chain(kind, shapes, arr)
    vals, vecs = np.linalg.eig(P.T)
    k = int(np.argmin(np.abs(vals - 1.0)))
    ref = np.real(vecs[:, k])
    ref = ref / ref.sum()
    np.testing.assert_allclose(pi.reshape(-1), ref, rtol=0, atol=1e-13)
    np.testing.assert_allclose(pi.reshape(-1) @ P, pi.reshape(-1), rtol=0, atol=1e-15)


def test_stationary_weights_refuse_a_non_factorising_chain():
    m = S.SSY()
    shapes = (3, 3, 3, 5)
    arr = list(S.discretize_ssy(m, shapes))
    zQ = np.array(arr[7])
    zQ[1, 0, :] = zQ[1, 0, ::-1]                     # one slice of the conditional z tensor differs (rows still sum to 1)
    arr[7] = zQ
    with pytest.raises(ValueError, match="does not factorise"):
        S.stationary_weights(m, shapes, arrays=arr)
    g = S.GCY()
    gs = (2, 3, 2, 3, 2, 3)
    arr = list(S.discretize_gcy(g, gs))
    zpQ = np.array(arr[3])
    zpQ[0] = np.eye(3)[::-1] * 0.5 + 0.5 * np.eye(3)
    arr[3] = zpQ
    with pytest.raises(ValueError, match="axis 1"):
        S.stationary_weights(g, gs, arrays=arr)


def test_argument_checks_before_device_work():
    m = S.SSY()
    shapes = (3, 3, 3, 5)
    w = np.full(shapes, 800.0)
    with pytest.raises(ValueError, match="4 axes"):
        S.sdf_moments(m, (3, 3, 3), w)
    with pytest.raises(ValueError, match="2 ... 32"):
        S.sdf_moments(m, (3, 3, 1, 5), np.full((3, 3, 1, 5), 800.0))
    with pytest.raises(ValueError, match="w_star has shape"):
        S.sdf_moments(m, shapes, np.full((3, 3, 3, 4), 800.0))
    with pytest.raises(TypeError):
        S.sdf_moments(object(), shapes, w)
    with pytest.raises(ValueError, match="n_max"):
        S.term_structure(m, shapes, w, 0)
    with pytest.raises(ValueError, match="n_max"):
        S.term_structure(m, shapes, w, 2.5)
    with pytest.raises(ValueError, match="save horizon"):
        S.term_structure(m, shapes, w, 10, save=(0, 3))
    with pytest.raises(ValueError, match="save horizon"):
        S.term_structure(m, shapes, w, 10, save=(11,))
    with pytest.raises(ValueError, match="kappa"):
        S.term_structure(m, shapes, w, 10, kappa=float("nan"))
    with pytest.raises(ValueError, match="one entry per axis"):
        S.term_structure(m, shapes, w, 10, weights=[np.ones(3)])
    with pytest.raises(ValueError, match="state index"):
        S.term_structure(m, shapes, w, 10, weights=[0, 0, 3, 0])
    with pytest.raises(ValueError, match="weights\\[3\\] has"):
        S.term_structure(m, shapes, w, 10, weights=[0, 0, 0, np.ones(4)])
    with pytest.raises(ValueError, match="kappa"):
        S.claim_prices(m, shapes, w, "one")
    with pytest.raises(ValueError, match="rtol"):
        S.claim_prices(m, shapes, w, 1.0, rtol=0.0)
    with pytest.raises(ValueError, match="w_star has shape"):
        S.claim_prices(m, shapes, w[:2], 1.0)

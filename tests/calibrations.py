"""
Helper of tests/test_oracle_calibrations.py, tests/test_hip_calibrations.py and tests/golden/make_golden.py (not a test
module): the non-default calibrations the oracle is pinned at and the kernels are held to.

  name         beta    gamma   psi    theta = (1 - gamma) / (1 - 1 / psi)
  steep        0.99    13.68   1.5    -38.04     (beyond GCY's default -36)
  shallow      0.97     4.71   2.5     -6.18
  positive     0.995    9.58   0.7    +20.02     (psi < 1: theta, 1/theta > 0, theta - 1 > 0)
  fractional   0.99     0.8    2.0     +0.4      (0 < theta < 1: theta - 1 < 0 < 1/theta - 1)
  linear       0.99     0.5    2.0     exactly 1 (T is affine in w)
  shifted      the default beta, gamma, psi (factor 1.0, so theta is the default one) and every other field of the
               default model times its own fixed factor in [0.9, 1.1] (SHIFT_SSY / SHIFT_GCY below); persistences stay
               below 1.  For the fields beta, gamma and psi do not reach.  The factors were chosen so that the
               oracle's Newton from 800 finds a fixed point at SSY 10^4 and GCY 5^6 (spectral radius of J(w*) 0.998
               and 0.997; tests/test_oracle_calibrations.py repeats the solve): factors that all lower the risk or
               all raise the persistences push w* out of reach of that start.

Names are ASCII, as oracle.models takes them; ``greek`` turns an override dict into the package's (and the reference's)
keyword names.
"""
import unicodedata

from oracle import models as omodels

NAMES = ("steep", "shallow", "positive", "fractional", "linear", "shifted")

_BGP = {"steep": (0.99, 13.68, 1.5), "shallow": (0.97, 4.71, 2.5), "positive": (0.995, 9.58, 0.7),
        "fractional": (0.99, 0.8, 2.0), "linear": (0.99, 0.5, 2.0)}

# factor per field of the default model (beta, gamma, psi: 1.0)
SHIFT_SSY = dict(mu_c=0.92, rho=1.004, phi_z=1.07, phi_c=1.05, rho_z=0.96, rho_c=1.003, rho_lam=0.95,
                 s_z=1.06, s_c=0.93, s_lam=1.09)
SHIFT_GCY = dict(rho_lam=1.01, s_lam=0.91, mu_c=0.94, phi_c=1.07, rho=0.98, rho_pi=1.1, phi_z=0.9, rho_c=1.004,
                 s_c=0.95, rho_z=0.93, s_z=1.08, rho_pipi=1.01, phi_zpi=1.05, rho_zpi=0.96, s_zpi=1.03)

_GREEK = {"beta": "β", "gamma": "γ", "psi": "ψ", "mu_c": "μ_c", "rho": "ρ", "phi_z": "φ_z", "phi_c": "φ_c",
          "rho_z": "ρ_z", "rho_c": "ρ_c", "rho_lam": "ρ_λ", "s_z": "s_z", "s_c": "s_c", "s_lam": "s_λ",
          "rho_pi": "ρ_π", "rho_pipi": "ρ_ππ", "phi_zpi": "φ_zπ", "rho_zpi": "ρ_zπ", "s_zpi": "s_zπ"}


def overrides(kind, name, defaults=None):
    """Overrides of the default calibration (ASCII names).  ``defaults``: field -> default value, for ``shifted``
    (the oracle's own defaults when omitted; make_golden.py passes the reference's)."""
    if name != "shifted":
        beta, gamma, psi = _BGP[name]
        return dict(beta=beta, gamma=gamma, psi=psi)
    if defaults is None:
        fields = omodels.SSY_FIELDS if kind == "ssy" else omodels.GCY_FIELDS
        defaults = dict(zip(fields, omodels.ssy_params() if kind == "ssy" else omodels.gcy_params()))
    shift = SHIFT_SSY if kind == "ssy" else SHIFT_GCY
    return {k: float(defaults[k]) * f for k, f in shift.items()}


def greek(over):
    """Keyword names as Python spells identifiers (NFKC), so they also serve for getattr on a model."""
    return {unicodedata.normalize("NFKC", _GREEK[k]): v for k, v in over.items()}


def oracle_params(kind, name):
    return (omodels.ssy_params if kind == "ssy" else omodels.gcy_params)(**overrides(kind, name))


def package_model(S, kind, name):
    return (S.SSY if kind == "ssy" else S.GCY)(**greek(overrides(kind, name)))


def theta(kind, name):
    p = oracle_params(kind, name)
    return omodels.theta_of(p[1], p[2]) if kind == "ssy" else omodels.theta_of(p[2], p[1])

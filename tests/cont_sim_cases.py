"""
The cases of the continuous-state simulation tests (tests/test_cont_simulation_cpu.py checks their input conditions and
their rounding amplification on the numpy twin, tests/test_hip_cont_simulation.py runs them on the device), and the
fixed points they share: tests/golden/cont_sim_wstar.npz holds, per grid, the w* a tight Newton solve of the device
operator (Gauss–Hermite d = 3) returned, so that the CPU file needs no solve.

GCY 2x3x2x3x4x3 at num_std_devs = 3.2 has no fixed point: successive approximation from w = 1 grows without bound (the
operator is monotone, so a fixed point above 1 would stop it), on the device and in the oracle, as
tests/test_hip_continuous.py records for GCY 3x3x3x3x4x4.  That case runs at ``smooth_w``, a smooth grid function of a
wealth-consumption ratio's size; nothing the simulation computes needs w to be a fixed point.  The GPU file asserts that
the solve does diverge there.
"""
import os

import numpy as np

from oracle import continuous as OC
from oracle import models as OM

GOLD = os.path.join(os.path.dirname(__file__), "golden", "cont_sim_wstar.npz")

SIZES = [("ssy", (2, 3, 4, 5)), ("ssy", (3, 4, 3, 5)), ("gcy", (2, 3, 2, 3, 4, 3))]
STD_DEVS = (1.0, 3.2)
GRIDS = [(kind, sizes, sd) for kind, sizes in SIZES for sd in STD_DEVS]
P, T, PATH_OFFSET, SEED = 1000, 64, 123, 0x9E3779B97F4A7C15
QUAD_D = 3                       # Gauss–Hermite order of the operator whose fixed point the cases run at
BURN_INS = (0, 7)
STARTS = ("zero", "vector")


NO_FIXED_POINT = [("gcy", (2, 3, 2, 3, 4, 3), 3.2)]


def smooth_w(grids):
    """A smooth grid function > 1 of the size of a wealth-consumption ratio."""
    mesh = np.meshgrid(*[np.linspace(-1.0, 1.0, len(g)) for g in grids], indexing="ij")
    return 700.0 + 60.0 * sum(np.sin(1.0 + 0.7 * d + m) for d, m in enumerate(mesh))


def tag(kind, sizes, sd):
    return f"{kind}_{'x'.join(map(str, sizes))}_sd{sd}"


def params_of(kind):
    return tuple(float(p) for p in (OM.ssy_params() if kind == "ssy" else OM.gcy_params()))


def grids_of(kind, sizes, sd):
    build = OC.build_grid_ssy if kind == "ssy" else OC.build_grid_gcy
    return build(params_of(kind), sizes, sd)


def start_of(grids, which):
    """None (the zero state), one state off the centre, or the far-outside start.

    The one state is the same on both grids of a size: −1.5 times the maximum of the ``num_std_devs = 1.0`` grid on the
    even axes, +0.75 times on the odd ones.  It lies outside the 1.0 grid on every even axis and inside the 3.2 grid on
    every axis.  From the zero state the z axis of the GCY 1.0 grid is never left (the reference's ``build_grid``
    divides the z range by 1 − ρ_zπ: ±0.0097 against a standard deviation of z of 0.0015); from this state z starts
    below that grid and takes some thirty steps to decay into it, so the cases with this start clamp on every axis
    (tests/test_cont_simulation_cpu.py holds them to that)."""
    if which == "zero":
        return None
    if which == "vector":
        kind = "ssy" if len(grids) == 4 else "gcy"
        unit = grids_of(kind, tuple(len(g) for g in grids), 1.0)
        return np.array([-1.5 * g[-1] if d % 2 == 0 else 0.75 * g[-1] for d, g in enumerate(unit)])
    if which == "far":
        return np.array([10.0 * g[-1] for g in grids])
    raise KeyError(which)


def golden_wstar(kind, sizes, sd):
    if (kind, sizes, sd) in NO_FIXED_POINT:
        return smooth_w(grids_of(kind, sizes, sd))
    z = np.load(GOLD)
    return z[tag(kind, sizes, sd)]

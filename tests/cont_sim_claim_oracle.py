"""
Numpy twin of the claim series of the continuous-state simulation (``simulate_continuous`` with ``kappa``):
on the states, the draws and the six base series of tests/cont_sim_oracle.py, with v̂ the ``lin_interp`` of the grid
function v (the price–dividend ratio of a claim on G_c^κ) along the states,

    rd_t = κ dc_t + ln(1 + v̂(x_t)) − ln v̂(x_{t−1}),  xd_t = rd_t − rf_t,  pd_t = ln v̂(x_t)

and the slope is the OLS slope of xd_t on pd_{t−1} = ln v̂(x_{t−1}).  ``dtype=np.longdouble`` runs the series in extended
precision as ``cont_sim_oracle.series`` does (the interpolation itself stays fp64).
"""
import numpy as np

import cont_sim_oracle as co
import sim_oracle as so

SERIES = co.SERIES + ("rd", "xd", "pd")


def smooth_v(grids):
    """A smooth grid function of a price–dividend ratio's size: at least 60 − 8 D > 0 for D ≤ 6."""
    mesh = np.meshgrid(*[np.linspace(-1.0, 1.0, len(g)) for g in grids], indexing="ij")
    return 60.0 + 8.0 * sum(np.cos(0.5 + 0.9 * d + m) for d, m in enumerate(mesh))


def series(kind, params, grids, X, xi, w, em, v, kappa, dtype=np.float64):
    """The nine series along states X (P, T+1, D) with draws xi (P, T): ({name: (P, T)}, slope regressor pd_{t−1})."""
    out, _ = co.series(kind, params, grids, X, xi, w, em, dtype)
    vh = co.interp_along(X, v, grids).astype(dtype)
    lv = np.log(vh)
    out["rd"] = dtype(kappa) * out["dc"] + np.log(dtype(1.0) + vh[:, 1:]) - lv[:, :-1]
    out["xd"] = out["rd"] - out["rf"]
    out["pd"] = lv[:, 1:]
    return out, lv[:, :-1]


def statistics(ser, xr):
    out = {}
    for nm, s in ser.items():
        m, sd, a = so.two_pass(np.asarray(s, dtype=np.float64))
        out[nm] = {"mean": m, "std": sd, "ac1": a}
    out["slope"] = so.ols_slope(np.asarray(xr, dtype=np.float64), np.asarray(ser["xd"], dtype=np.float64))
    return out


def simulate(kind, params, grids, w, em, v, kappa, seed=0, path_offset=0, n_paths=1, burn_in=0, n_periods=2, step_offset=0,
             start=None, dtype=np.float64):
    """``cont_sim_oracle.simulate`` with the nine series and the claim's slope."""
    X, xi = co.state_paths(kind, params, len(grids), seed, path_offset, n_paths, burn_in, n_periods, step_offset, start, dtype)
    ser, xr = series(kind, params, grids, X, xi, w, em, v, kappa, dtype)
    out, near = co.outside(grids, X)
    return {"state": X, "series": ser, "stats": statistics(ser, xr), "outside": out[:, 1:],
            "clamped": out[:, 1:].sum(axis=1), "near_edge": near[:, 1:], "final_state": X[:, -1, :]}

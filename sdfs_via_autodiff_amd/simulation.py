"""
Simulated paths of the discretised chain at the fixed point w*: the SDF, returns and their sample moments.

What a long-run-risk model is compared with are moments of simulated series of data length, across many samples.  Each
path starts at x_0 (drawn from the stationary distribution, or a given state), runs B burn-in steps, then records T
transitions x_{t−1} → x_t with a standard normal ξ_t (t = B+1 … B+T):

    dc_t = μ_c + z(x_{t−1}) + σ_c(x_{t−1}) ξ_t                                  log consumption growth
    m_t  = θ ln β + θ h_λ(x_t) − γ dc_t + (θ−1)(ln w(x_t) − ln(w(x_{t−1}) − 1))   log SDF
    rf_t = −ln E_{x_{t−1}}[M]                                                   log risk-free rate
    rc_t = dc_t + ln w(x_t) − ln(w(x_{t−1}) − 1),  xc_t = rc_t − rf_t,  wc_t = w(x_t)
    with κ (a claim on G_c^κ, v its price–dividend ratio):
    rd_t = κ dc_t + ln(1 + v(x_t)) − ln v(x_{t−1}),  xd_t = rd_t − rf_t,  pd_t = ln v(x_t)

Random numbers are Philox4x32-10 with counter (t, p, b, 0) for step t of path p, so every index can be reproduced
(tests/sim_oracle.py is the numpy twin).  The grid work (records) and the paths (one lane each) run in libsdfs_hip.so
(sdfs_sim_records_dev, sdfs_sim_paths_dev), fp64.  DESIGN §4.8.

``simulate_continuous`` walks the continuous-state model instead (x_t = next_state(x_{t−1}, η_t), w* and −ln E_x[M]
interpolated along the path): counter (t, p, b, 1), tests/cont_sim_oracle.py, sdfs_cont_sim_*_dev, DESIGN §4.14.  With
``kappa`` it interpolates the claim's v as well and adds rd, xd, pd (sdfs_cont_sim_claim_*_dev).
"""
import math

import numpy as np

from ._requests import MAX_RETURNED  # noqa: F401  (path-steps of returned series; a name of this module)
from ._requests import (LAYOUT, _kind, _shapes, _check_grid, _kappa, _count, _check_w_star, _path_request,
                        _cont_grids, _cont_operator_or_d, _operator, _cont_operator, _device_grid, _Fence,
                        _check_finite_grid, stationary_weights)
from .pricing import claim_prices, _claim_prices

SERIES = ("dc", "m", "rf", "rc", "xc", "wc")
SERIES_KAPPA = SERIES + ("rd", "xd", "pd")
STATS = ("mean", "std", "ac1")
REC_BYTES = 64                    # per state


def cdf_tables(model, shapes, arrays=None):
    """(cdf, cdf0): per axis the cumulative rows of its transition matrix and the cumulative stationary marginal, np.cumsum
    in fp64 with the last entry of every row set to 2.0.  ValueError (of ``stationary_weights``) when the chain does not
    factorise."""
    kind, shapes = _shapes(model, shapes)
    arr = LAYOUT[kind].discretize(model, shapes) if arrays is None else arrays
    pis = stationary_weights(model, shapes, arr)
    cdf, cdf0 = [], []
    for qi, n, pi in zip(LAYOUT[kind].transitions, shapes, pis):
        Q = np.asarray(arr[qi], dtype=np.float64).reshape(-1, n, n)[0]
        c = np.cumsum(Q, axis=1)
        c[:, -1] = 2.0
        c0 = np.cumsum(pi)
        c0[-1] = 2.0
        cdf.append(c)
        cdf0.append(c0)
    return cdf, cdf0


def _summary(a):
    a = np.asarray(a, dtype=np.float64)
    ok = a[np.isfinite(a)]
    if ok.size == 0:
        nan = float("nan")
        return {"mean": nan, "median": nan, "p05": nan, "p95": nan}
    return {"mean": float(ok.mean()), "median": float(np.median(ok)), "p05": float(np.percentile(ok, 5)),
            "p95": float(np.percentile(ok, 95))}


def _by_statistic(names, entry):
    """{name: {"mean" | "std" | "ac1": entry(row)}, "slope": entry(3 nser)}: the rows of a statistics array, named."""
    out = {nm: {s: entry(3 * i + j) for j, s in enumerate(STATS)} for i, nm in enumerate(names)}
    out["slope"] = entry(3 * len(names))
    return out


def _named_paths(first, names, series):
    """The "paths" of a result: its first entry (indices or states), then series[..., i, :, :] under names[i]."""
    return {**first, **{nm: series[..., i, :, :] for i, nm in enumerate(names)}}


def _result(names, st, P):
    """The dict ``simulate`` returns (without "paths") from the (3 nser + 1, P) statistics ``st``."""
    per_path = _by_statistic(names, lambda k: st[k])
    summary = _by_statistic(names, lambda k: _summary(st[k]))
    pooled = {}
    for nm in names:
        m = per_path[nm]["mean"]
        pooled[nm] = {"mean": float(m.mean()), "se": float(m.std(ddof=1) / math.sqrt(P)) if P > 1 else float("nan")}
    return {"series": names, "per_path": per_path, "summary": summary, "pooled": pooled}


def simulate(model, shapes, w_star, n_paths, n_periods, *, burn_in=0, seed=0, path_offset=0, start="stationary",
             kappa=None, rtol=1e-10, return_paths=False):
    """Simulate ``n_paths`` paths (numbered path_offset … path_offset + n_paths − 1) of ``n_periods`` recorded steps
    after ``burn_in`` steps of the discretised chain of (model, shapes) at the fixed point ``w_star``.

    start: "stationary" (x_0 from the product of the stationary marginals) or one state index per axis.  kappa: None,
    or the leverage of a claim on G_c^κ whose price–dividend ratio v = claim_prices(...)["pd"] (at ``rtol``) adds the
    series rd, xd, pd.  Returns {"series": names, "per_path": {name: {"mean", "std", "ac1"}, "slope"} (host arrays of
    shape (n_paths,)), "summary": the NaN-ignoring cross-path mean, median, 5 % and 95 % of each, "pooled": {name:
    {"mean", "se"}} over all path-steps (se from the per-path means)}, and with ``return_paths`` "paths" = {"index":
    (P, T+1, d) uint8 for t = B … B+T, name: (P, T) float64}.  ``slope``: OLS slope of xd_t on pd_{t−1} (xc_t on
    ln(w(x_{t−1}) − 1) without κ).  A path's result depends only on its number, the seed and the model."""
    import torch
    kind, shapes = _shapes(model, shapes)
    _check_grid(w_star, shapes, "w_star")
    P, T, B, off, sd, rtol, fixed = _path_request(shapes, n_paths, n_periods, burn_in, seed, path_offset, start, rtol,
                                                  return_paths, check_kappa=lambda: kappa is None or _kappa(kappa))
    k = None if kappa is None else _kappa(kappa)
    _check_w_star(w_star)
    arr = _kind(model).discretize(model, shapes)
    cdf, cdf0 = cdf_tables(model, shapes, arr)          # (ValueError when the chain does not factorise)
    names = SERIES_KAPPA if k is not None else SERIES
    ns = len(names)
    N = int(np.prod(shapes))
    need = N * REC_BYTES + (3 * ns + 1) * P * 8
    if return_paths:
        need += P * T * ns * 8 + P * (T + 1) * len(shapes)
    free = torch.cuda.mem_get_info(torch.cuda.current_device())[0]
    if need > free:
        raise ValueError(f"the per-state records and outputs need {need / 2**30:.2f} GiB, {free / 2**30:.2f} GiB of "
                         "device memory is free")

    op, _ = _operator(model, shapes)
    w = _device_grid(op, w_star, "w_star")
    v = None
    if k is not None:
        v = _device_grid(op, claim_prices(model, shapes, w_star, k, rtol=rtol)["pd"], "pd")
    dev = w.device
    rec = torch.empty((N, 8), dtype=torch.float64, device=dev)
    op.sim_records_dev(w.data_ptr(), v.data_ptr() if v is not None else None, rec.data_ptr())
    stats = torch.empty((3 * ns + 1, P), dtype=torch.float64, device=dev)
    idx = ser = None
    if return_paths:
        idx = torch.empty((P, T + 1, len(shapes)), dtype=torch.uint8, device=dev)
        ser = torch.empty((ns, P, T), dtype=torch.float64, device=dev)
    op.sim_paths_dev(rec.data_ptr(), np.concatenate([c.ravel() for c in cdf]),
                     None if fixed is not None else np.concatenate(cdf0), sd, off, P, B, T, kappa=k, start=fixed,
                     stats_ptr=stats.data_ptr(), idx_ptr=idx.data_ptr() if idx is not None else None,
                     series_ptr=ser.data_ptr() if ser is not None else None)
    out = _result(names, stats.cpu().numpy(), P)
    if return_paths:
        out["paths"] = _named_paths({"index": idx.cpu().numpy()}, names, ser.cpu().numpy())
    del rec
    return out


CONT_REC_BYTES = 16               # per grid point: {w, −ln E_x[M]}
CONT_CLAIM_REC_BYTES = 32         # ... with a claim: {w, −ln E_x[M], v, 0}


def _cont_start(start, nd, P):
    """The start of ``simulate_continuous``: None, or one state (nd,) or one per path (P, nd) as a float64 array."""
    if start is None:
        return None
    try:
        st = np.ascontiguousarray(np.asarray(start, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("start must be None, one state (D,) or one state per path (n_paths, D)") from None
    if st.shape not in ((nd,), (P, nd)):
        raise ValueError(f"start has shape {st.shape}: one state ({nd},) or one per path ({P}, {nd})")
    if not np.all(np.isfinite(st)):
        raise ValueError("start must be finite")
    return st


def _cont_pd(pd, kappa, shapes):
    """The checks of a caller's price–dividend ratio: it needs ``kappa``, the grid's shape, finite and positive entries."""
    if kappa is None:
        raise ValueError("pd is the price–dividend ratio of a claim on G_c^κ: it needs kappa")
    _check_finite_grid(pd, shapes, "pd")
    import torch
    ok = bool(torch.all(pd > 0)) if isinstance(pd, torch.Tensor) else bool(np.all(np.asarray(pd, dtype=np.float64) > 0.0))
    if not ok:
        raise ValueError("pd must be positive at every grid point (the series need ln v)")


def simulate_continuous(model, grids, w_star, n_paths, n_periods, *, burn_in=0, seed=0, path_offset=0, step_offset=0,
                        start=None, operator=None, d=5, return_paths=False, device=0, kappa=None, pd=None, rtol=1e-10):
    """Simulate ``n_paths`` paths (numbered path_offset … path_offset + n_paths − 1) of the continuous-state model:
    x_t = next_state(x_{t−1}, η_t) with standard normal η_t, the grid function ``w_star`` (on ``grids``, as
    ``wc_ratio_continuous`` returns them) and −ln E_x[M] interpolated multilinearly along the path, the coordinates
    clamped to the grid as ``lin_interp`` clamps them.  After ``burn_in`` steps, ``n_periods`` steps are recorded:

        dc_t = μ_c + z_{t−1} + φ_c exp(h_c,t−1) ξ_t
        m_t  = θ ln β + θ h_λ,t − γ dc_t + (θ−1)(ln ŵ(x_t) − ln(ŵ(x_{t−1}) − 1))
        rf_t = r̂f(x_{t−1}),  rc_t = dc_t + ln ŵ(x_t) − ln(ŵ(x_{t−1}) − 1),  xc_t = rc_t − rf_t,  wc_t = ŵ(x_t)

    start: None (the zero state), one state (D,) or one per path (P, D).  operator: a ``ContinuousOperator`` on these
    parameters and grids, whose nodes and weights define E_x[M]; otherwise one is built with ``qnwnorm([d] * D)``.
    step_offset: the run's steps are numbered step_offset + 1 …, so that a run continued from ``final_state`` with
    step_offset = the steps already taken draws the random numbers the longer run would have drawn.

    kappa: None, or the leverage of a claim on G_c^κ, which adds the series

        rd_t = κ dc_t + ln(1 + v̂(x_t)) − ln v̂(x_{t−1}),  xd_t = rd_t − rf_t,  pd_t = ln v̂(x_t)

    with v̂ the interpolant of the claim's price–dividend ratio v on the grid: ``claim_prices_continuous(...)["pd"]`` on the
    same operator at ``rtol`` (ValueError "no finite price" when r(K) ≥ 1), or the grid function ``pd`` (positive; no
    solve is run).  With a claim the slope is that of xd_t on pd_{t−1}, the result has the nine series of ``SERIES_KAPPA``
    and "pd" = v on the grid; the six base series keep the bits of the run without a claim.  DESIGN §4.18.

    Returns the dict of ``simulate`` ("series", "per_path", "summary", "pooled") for dc, m, rf, rc, xc, wc (slope: xc_t
    on ln(ŵ(x_{t−1}) − 1)) and "clamped" = {"per_path": share of the recorded steps whose x_t lay outside the grid on
    some axis, "summary"}, "final_state" (P, D), "E_M" on the grid, and with ``return_paths`` "paths" = {"state":
    (P, T+1, D) for t = B … B+T, name: (P, T)}.  Random numbers are Philox4x32-10 with counter (t, p, b, 1)
    (tests/cont_sim_oracle.py is the numpy twin).  A path's result depends only on its number, the seed, step_offset,
    its start and the model.  DESIGN §4.14."""
    import torch
    _, nd, grids, shapes = _cont_grids(model, grids, w_star)
    P, T, B, off, sd, rtol, _ = _path_request(shapes, n_paths, n_periods, burn_in, seed, path_offset, "stationary", rtol,
                                              return_paths, check_kappa=lambda: kappa is None or _kappa(kappa))
    k = None if kappa is None else _kappa(kappa)
    if pd is not None:
        _cont_pd(pd, k, shapes)
    s0 = _count(step_offset, "step_offset", 0, (1 << 32) - 1)
    if s0 + B + T >= 1 << 32:
        raise ValueError(f"step_offset + burn_in + n_periods = {s0 + B + T} >= 2^32: step numbers are 32-bit")
    start = _cont_start(start, nd, P)
    d = _cont_operator_or_d(model, grids, shapes, operator, d)
    _check_w_star(w_star)
    names = SERIES_KAPPA if k is not None else SERIES
    ns = len(names)
    N = int(np.prod(shapes))
    # the records, w and E_M (with a claim also v, and the six work grids of its solve), the statistics, clamped, the
    # final states and a start per path
    grid_bytes = CONT_REC_BYTES + 16 if k is None else CONT_CLAIM_REC_BYTES + 24 + (48 if pd is None else 0)
    need = N * grid_bytes + (3 * ns + 1) * P * 8 + P * 4 + 2 * P * nd * 8
    if return_paths:
        need += P * T * ns * 8 + P * (T + 1) * nd * 8
    devno = operator.device if operator is not None else int(device)
    dev = torch.device("cuda", devno)
    free = torch.cuda.mem_get_info(dev)[0]
    if need > free:
        raise ValueError(f"the per-point records and outputs need {need / 2**30:.2f} GiB, {free / 2**30:.2f} GiB of "
                         "device memory is free")
    op = _cont_operator(model, grids, operator, d, devno)
    w = _device_grid(op, w_star, "w_star")
    em = torch.empty_like(w)
    v = None
    if k is not None:
        v = _device_grid(op, pd, "pd") if pd is not None else \
            _device_grid(op, _claim_prices(op, w, model.θ, model.γ, k, rtol, _Fence(op))["pd"], "pd")
    rec = torch.empty((N, 2 if k is None else 4), dtype=torch.float64, device=dev)
    stats = torch.empty((3 * ns + 1, P), dtype=torch.float64, device=dev)
    clamped = torch.empty((P,), dtype=torch.int32, device=dev)
    final = torch.empty((P, nd), dtype=torch.float64, device=dev)
    start_dev = states = ser = None
    if start is not None and start.ndim == 2:
        start_dev = torch.from_numpy(start).to(dev)
    if return_paths:
        states = torch.empty((P, T + 1, nd), dtype=torch.float64, device=dev)
        ser = torch.empty((ns, P, T), dtype=torch.float64, device=dev)
    _Fence(op).before_library()
    op.cont_sdf_mean_dev(w.data_ptr(), em.data_ptr())
    kw = dict(step_offset=s0, start=start if start is not None and start.ndim == 1 else None,
              start_ptr=start_dev.data_ptr() if start_dev is not None else None,
              states_ptr=states.data_ptr() if states is not None else None,
              series_ptr=ser.data_ptr() if ser is not None else None)
    if k is None:
        op.cont_sim_records_dev(w.data_ptr(), em.data_ptr(), rec.data_ptr())
        op.cont_sim_paths_dev(rec.data_ptr(), sd, off, P, B, T, stats.data_ptr(), clamped.data_ptr(), final.data_ptr(), **kw)
    else:
        op.cont_sim_claim_records_dev(w.data_ptr(), em.data_ptr(), v.data_ptr(), rec.data_ptr())
        op.cont_sim_claim_paths_dev(rec.data_ptr(), k, sd, off, P, B, T, stats.data_ptr(), clamped.data_ptr(),
                                    final.data_ptr(), **kw)
    op.synchronize()
    share = clamped.cpu().numpy().astype(np.float64) / T
    out = _result(names, stats.cpu().numpy(), P)
    out.update({"clamped": {"per_path": share, "summary": _summary(share)}, "final_state": final.cpu().numpy(),
                "E_M": em.cpu().numpy()})
    if k is not None:
        out["pd"] = v.cpu().numpy()
    if return_paths:
        out["paths"] = _named_paths({"state": states.cpu().numpy()}, names, ser.cpu().numpy())
    del rec
    return out


__all__ = ["simulate", "simulate_continuous", "cdf_tables"]

"""
sdfs_via_autodiff_amd -- MI355X-native solver for the wealth-consumption-ratio
fixed point of the SSY / GCY long-run-risk models (the hot path of
jstac/sdfs_via_autodiff): hand-written HIP for gfx950 behind the reference's own
``T(w)`` / ``solver(f, x_init, algorithm)`` call shapes.

    from sdfs_via_autodiff_amd import SSY, discretize_ssy, ssy_operator, solver
    ssy = SSY(); shapes = (15, 15, 15, 15)
    T = ssy_operator(shapes, ssy.params, discretize_ssy(ssy, shapes))
    w_star = solver(T, 800.0 * np.ones(shapes), algorithm="newton")

Importing the package loads libsdfs_hip.so and fails loudly if it has not been
built; there is no CPU fallback for the operator.
"""
from .models import SSY, GCY
from .discretize import rouwenhorst, tauchen, discretize_ssy, discretize_gcy
from .operators import (KoopmansOperator, ssy_operator, gcy_operator, T_ssy, T_gcy)
from .solvers import (successive_approx, newton_solver, anderson_solver,
                      fixed_point_via_gradient_decent, solvers, solver,
                      default_tolerance, default_max_iter)
from .drivers import test_compute_wc_ratio_ssy, test_compute_wc_ratio_gcy
from .loglinear import wc_loglinear_factory, loglinear_guess
from .continuous import (ContinuousOperator, build_grid, T_fun_factory, wc_ratio_continuous, qnwnorm,
                         lin_interp, vals_to_coords, construct_wstar_callable, save_wstar, load_wstar)
from .single_index import (DenseOperator, compute_H_single_index, discretize_single_index, single_index_T,
                           single_to_multi, multi_to_single)
from .sensitivity import (discretize_ssy_tangent, discretize_gcy_tangent, wc_ratio_sensitivities,
                          wc_ratio_gradient, rouwenhorst_generator, discretize_ssy_persistence_tangent,
                          discretize_gcy_persistence_tangent, SSY_PERSISTENCE, GCY_PERSISTENCE,
                          adjoint_moments_to_gradient, wc_ratio_sensitivities_continuous, wc_ratio_gradient_continuous,
                          SSY_PARAMS, GCY_PARAMS)
from .pricing import (stationary_weights, sdf_moments, term_structure, claim_prices, price_sensitivities,
                      sdf_moments_continuous, term_structure_continuous, claim_prices_continuous)
from .simulation import simulate, simulate_continuous
from .batch import (BatchOperator, BatchResult, solve_batch, batch_lds_bytes, BatchGradient, gradient_batch, BatchPrices,
                    price_batch, price_words_to_stats, BatchSimulation, simulate_batch, batch_sim_lds_bytes,
                    batch_cdf_tables, batch_sim_tables)
from ._lib import SdfsError, LIB_PATH

__all__ = ["SSY", "GCY", "rouwenhorst", "tauchen", "discretize_ssy", "discretize_gcy",
           "KoopmansOperator", "ssy_operator", "gcy_operator", "T_ssy", "T_gcy",
           "successive_approx", "newton_solver", "anderson_solver",
           "fixed_point_via_gradient_decent", "solvers", "solver",
           "default_tolerance", "default_max_iter", "test_compute_wc_ratio_ssy", "test_compute_wc_ratio_gcy",
           "wc_loglinear_factory", "loglinear_guess",
           "ContinuousOperator", "build_grid", "T_fun_factory", "wc_ratio_continuous", "qnwnorm",
           "lin_interp", "vals_to_coords", "construct_wstar_callable", "save_wstar", "load_wstar",
           "DenseOperator", "compute_H_single_index", "discretize_single_index", "single_index_T",
           "single_to_multi", "multi_to_single",
           "discretize_ssy_tangent", "discretize_gcy_tangent", "wc_ratio_sensitivities", "wc_ratio_gradient",
           "rouwenhorst_generator", "discretize_ssy_persistence_tangent", "discretize_gcy_persistence_tangent",
           "SSY_PERSISTENCE", "GCY_PERSISTENCE", "adjoint_moments_to_gradient",
           "wc_ratio_sensitivities_continuous", "wc_ratio_gradient_continuous", "SSY_PARAMS", "GCY_PARAMS",
           "stationary_weights", "sdf_moments", "term_structure", "claim_prices", "simulate", "simulate_continuous",
           "sdf_moments_continuous", "term_structure_continuous", "claim_prices_continuous", "price_sensitivities",
           "BatchOperator", "BatchResult", "solve_batch", "batch_lds_bytes", "BatchGradient", "gradient_batch", "BatchPrices", "price_batch", "price_words_to_stats",
           "BatchSimulation", "simulate_batch", "batch_sim_lds_bytes", "batch_cdf_tables", "batch_sim_tables",
           "SdfsError", "LIB_PATH"]

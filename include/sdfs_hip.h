/*
 * sdfs_hip.h -- C ABI of libsdfs_hip.so: the MI355X (gfx950) implementation of the
 * wealth-consumption-ratio fixed-point path of jstac/sdfs_via_autodiff.
 *
 * The reference has no FFI layer; its boundary for this path is two Python call
 * shapes (paths relative to the reference repo):
 *
 *   operator  T(w) = T_ssy(w, shapes, params, arrays)   code/ssy/discrete/ssy_wc_ratio.py:82-151
 *             T(w) = T_gcy(w, shapes, params, arrays)   code/gcy/discrete/gcy_wc_ratio.py:134-238
 *   solver    solver(f, x_init, algorithm, verbose)     code/solvers.py:154-177
 *             successive_approx / newton_solver / anderson_solver   code/solvers.py:19-124
 *
 * Each entry point below names the reference call it replaces.  Conventions:
 * opaque handle; every call returns 0 on success and a negative code on error
 * (message via sdfs_last_error); no exceptions cross the boundary; the caller
 * owns host buffers; the library owns its device buffers and one HIP stream per
 * handle; a handle is not thread-safe, distinct handles are independent.
 * Grids are C-order fp64 exactly as the reference lays them out
 * (SSY: (h_lam, h_c, h_z, z), z fastest; GCY: (z, z_pi, h_z, h_c, h_zpi, h_lam),
 * h_lam fastest).  "_dev" variants take device pointers (hipMalloc'd or
 * torch.Tensor.data_ptr()) and never touch host memory.
 */
#ifndef SDFS_HIP_H
#define SDFS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdfs_handle sdfs_handle;

enum { SDFS_MODEL_SSY = 0, SDFS_MODEL_GCY = 1 };
enum { SDFS_ALGO_SA = 0, SDFS_ALGO_NEWTON = 1, SDFS_ALGO_ANDERSON = 2 };

enum {
  SDFS_OK = 0,
  SDFS_ERR_ARG = -1,      /* bad argument (shape, count, null pointer) */
  SDFS_ERR_HIP = -2,      /* a HIP runtime call failed */
  SDFS_ERR_UNSUPPORTED = -3,
  SDFS_ERR_NUMERIC = -4   /* NaN/Inf met in the iteration */
};

/* Options of sdfs_solve*.  Defaults (sdfs_default_opts) are the reference's:
 * code/solvers.py:16-17 (tol 1e-7, max_iter 1e6), :55 (bicgstab_atol 1e-4),
 * jax.scipy.sparse.linalg.bicgstab default tol 1e-5, :104-114 (Anderson
 * history 10, mixing 4, beta 8, ridge 1e-6, max_iter 1e4). */
typedef struct sdfs_opts {
  double tol;            /* sup-norm step tolerance (SA, Newton); l2 residual (Anderson) */
  int64_t max_iter;
  double inner_rtol;     /* BiCGSTAB relative tolerance on |r|_2            */
  double inner_atol;     /* BiCGSTAB absolute tolerance on |r|_2            */
  int64_t inner_max_iter;/* 0 -> 10 * N (JAX default)                       */
  int32_t history;       /* Anderson history size m                         */
  int32_t mixing_freq;   /* Anderson mixing frequency                       */
  double beta;           /* Anderson damping                                */
  double ridge;          /* Anderson ridge.  >= 0: jaxopt's absolute ridge on the Gram matrix (the reference's 1e-6,
                          * code/solvers.py:113).  < 0 (opt-in, NOT the reference's semantics): relative,
                          * |ridge| * trace(G) / history -- on grids of 1e7 .. 1e8 points the Gram entries N r^2 sink
                          * below an absolute 1e-6 while the residual is still 1e-6 and the acceleration stalls */
  int32_t check_every;   /* 0 (default): the library's choice -- 32, or 120 where the fused small-grid Anderson loop runs.
                            k >= 1: the host polls the device residual every k iterations: SA and Anderson enqueue (or replay from
                            a hipGraph) k gated iterations per synchronisation -- rounded up to an even number (SA) or to a
                            multiple of `history` (Anderson); the iterates, counts and error trace do not depend on k */
  int32_t use_graph;     /* 1: replay the iteration chunk from a hipGraph   */
  int32_t record_errors; /* 1: keep the per-iteration error trace (sdfs_error_trace) */
  int32_t krylov_f32;    /* Newton: 1 = inner BiCGSTAB in fp32 storage (Krylov vectors, J.v streams), fp64
                          * arithmetic and reductions, fp64 outer residual and iterate -- the mixed-precision
                          * configuration of BASELINE.json (config 5).  2 = the same with every store of those fp32
                          * containers rounded to bfloat16: the NUMERICS of bf16 storage at the bytes of fp32 (evaluation
                          * mode of the config-5 sweep).  3 = fp32 storage as under 1 AND the J.v passes of the pair
                          * plan on an fp32 LDS tile with v_mfma_f32_16x16x4_f32 (fp32 products and sums inside a
                          * pass; the BiCGSTAB reductions, the outer residual and the iterate stay fp64) -- config 5's
                          * "on MFMA" (csrc/f32_kernels.hpp); plans without such kernels run as under 1.
                          * Default 0 (everything fp64).    */
  int32_t t_f32;         /* Successive approximation on the pair plan (extents 16/20/24/32, whole 16-element chunks): 1 = the
                          * applications of T keep the intermediates between their passes as scaled floats while the step
                          * is above ~64 * 2^-24 * w / |theta| (what that storage can resolve), then the loop finishes in
                          * fp64 to `tol`: config 5 for the T passes.  The iteration count is then this configuration's
                          * own.  Ignored where the plan has no fp32 forms.  Default 0.                                 */
} sdfs_opts;

/* Per-kernel counters for the roofline line of bench.py. */
#define SDFS_MAX_KERNELS 16
typedef struct sdfs_kernel_counter {
  char name[48];
  int64_t launches;       /* launches bracketed by HIP events               */
  double total_ms;        /* sum of their durations (hipEventElapsedTime)   */
  double alg_bytes;       /* algorithmic bytes of ONE launch    */
  double alg_flops;       /* algorithmic flops of ONE launch                */
} sdfs_kernel_counter;

typedef struct sdfs_counters {
  int32_t nkernels;
  int32_t reserved;
  sdfs_kernel_counter k[SDFS_MAX_KERNELS];
} sdfs_counters;

/* Build an operator handle.  Replaces the closure
 *   T = lambda w: T_ssy(w, shapes, params, arrays)    (ssy_wc_ratio.py:230)
 *   T = lambda w: T_gcy(w, shapes, params, arrays)    (gcy_wc_ratio.py:333)
 * `params`: the 13 (SSY, ssy_model.py:81) or 18 (GCY, gcy_model.py:72-75) scalars.
 * `arrays`: the 10 (discretize_ssy, ssy_wc_ratio.py:73-77) or 15 (discretize_gcy,
 * gcy_wc_ratio.py:123-128) host arrays in the reference's order and layout;
 * `array_sizes[i]` = element count of arrays[i] (checked against `shapes`). */
int sdfs_create(int model, int ndim, const int64_t* shapes,
                const double* params, int nparams,
                const double* const* arrays, const int64_t* array_sizes, int narrays,
                int device_id, sdfs_handle** out);

/* Sharded variant for one rank of a multi-GPU run: this rank owns the
 * index block [lo, lo+len) of `shard_axis` of its INPUT grid; see
 * sdfs_apply_stage_dev.  shard_axis must be an axis no transition matrix is
 * conditioned on. */
int sdfs_create_sharded(int model, int ndim, const int64_t* shapes,
                        const double* params, int nparams,
                        const double* const* arrays, const int64_t* array_sizes, int narrays,
                        int device_id, int axis_a, int64_t a_lo, int64_t a_len,
                        int axis_b, int64_t b_lo, int64_t b_len, sdfs_handle** out);

/* Continuous-state operator: replaces the closure T_fun_factory(params, method, batch_size) returns
 * (code/ssy/continuous_junnan/ssy_wc_ratio_continuous.py:156-226,
 *  code/gcy/continuous/gcy_wc_ratio_continuous.py:190-260):
 *   Tw(x) = 1 + beta * (const(x) * E_x[ exp(theta h_lambda') * lin_interp(w)(x')^theta ])^(1/theta)
 * with the expectation a weighted sum over M shock nodes (Gauss-Hermite: `weights` from
 * quantecon.quad.qnwnorm; Monte Carlo: weights == NULL, plain mean).  `grids`: ndim uniform axis
 * grids in the reference's order (SSY h_lambda, h_c, h_z, z; GCY h_lambda, h_c, h_z, h_zpi, z, z_pi),
 * grids[d] has shapes[d] >= 2 points; `nodes`: [ndim][M] row-major, as the reference passes them.
 * The handle works with every entry point below (apply, JVP, solve, counters); batching is internal
 * (the reference's batch_size / ram_free only bound JAX's temporaries). */
int sdfs_create_continuous(int model, int ndim, const int64_t* shapes,
                           const double* params, int nparams, const double* const* grids,
                           const double* nodes, const double* weights, int64_t M,
                           int device_id, sdfs_handle** out);

/* Single-index dense form (code/ssy/discrete/temp_ssy.py:109-159: H = compute_H_single_index(ssy, shapes),
 * single_index_T(w, H, params) = 1 + beta * (H @ w**theta)**(1/theta); analytic Jacobian :204-216).  The
 * reference keeps it "for cross-checking solutions produced by the multi-index code"; same role here.
 * H: N x N row-major host array (copied to the device).  The handle works with every entry point below. */
int sdfs_create_dense(int64_t N, const double* H, double beta, double theta, int device_id, sdfs_handle** out);

/* lin_interp(x, fun_vals, grids) of code/utils.py:18-23 (multilinear, indices clipped to the grid):
 * x is [ndim][nq] row-major, out[nq]; all host pointers; ndim 4 or 6. */
int sdfs_lin_interp(int device_id, int ndim, const int64_t* shapes, const double* const* grids,
                    const double* fun_vals, const double* x, int64_t nq, double* out);

void sdfs_destroy(sdfs_handle* h);
const char* sdfs_last_error(const sdfs_handle* h);   /* h may be NULL: last create error */
int sdfs_default_opts(sdfs_opts* o);

int64_t sdfs_grid_size(const sdfs_handle* h);        /* N = prod(shapes) */
/* Launch on the caller's HIP stream (hip_stream == NULL is the device's default stream, which is
 * what torch.cuda.current_stream().cuda_stream returns for torch's default stream); use_own != 0
 * switches back to the handle's private non-blocking stream. */
int sdfs_set_stream(sdfs_handle* h, void* hip_stream, int use_own);
int sdfs_synchronize(sdfs_handle* h);

/* Tw = T(w).  Replaces one call of T_ssy / T_gcy.  Host buffers of N doubles. */
int sdfs_apply_T(sdfs_handle* h, const double* w_host, double* Tw_host);
/* Same on device pointers; if resid_dev != NULL also writes max|Tw - w| there
 * (the reduction of code/solvers.py:36 fused into the operator's last kernel). */
int sdfs_apply_T_dev(sdfs_handle* h, const double* w_dev, double* Tw_dev, double* resid_dev);

/* out = dT(w)[v], the map jax.jvp(f, (w,), (v,))[1] of code/solvers.py:87
 * (without the "- v" of g = f - id). */
int sdfs_apply_jvp(sdfs_handle* h, const double* w_host, const double* v_host, double* out_host);
/* Device form: linearise once at w (caches the two diagonal scalings), then
 * apply to any number of v.  If Tw_dev != NULL the linearisation also returns T(w). */
int sdfs_linearize_dev(sdfs_handle* h, const double* w_dev, double* Tw_dev);
int sdfs_apply_jvp_dev(sdfs_handle* h, const double* v_dev, double* out_dev, int minus_identity);

/* out = dT(w)^T [u], the vector-Jacobian product jax.grad needs for the reference's "gd" solver
 * (loss = |f(x) - x|^2, code/solvers.py:127-140): gradient = 2 (dT(x)^T r - r), r = f(x) - x.  Same
 * kernels as J.v with transposed matrices and the two diagonal scalings in each other's place; available
 * when every transition tensor is unconditional (Rouwenhorst / Tauchen chains), SDFS_ERR_UNSUPPORTED
 * otherwise.  The device form uses the linearisation cached by sdfs_linearize_dev. */
int sdfs_apply_vjp(sdfs_handle* h, const double* w_host, const double* u_host, double* out_host);
int sdfs_apply_vjp_dev(sdfs_handle* h, const double* u_dev, double* out_dev, int minus_identity);

/* Parameter sensitivities of the fixed point w* = T(w*; p) (the open item of the reference paper's conclusion: the fixed point
 * "can potentially [be differentiated] with respect to the parameters").  A direction of (params, arrays) -- the reference's
 * own terms, as in sdfs_create -- is (dparams, darrays): `dparams` has the handle's nparams entries, `darrays` its narrays
 * HOST pointers of the same sizes as the arrays (NULL, or darrays == NULL: a zero tangent); e.g. what jax.jvp of the
 * reference's discretize_ssy / discretize_gcy returns.
 *
 * out = dT(w)[dparams, darrays], the tangent of T at a fixed w (device pointers, N doubles each; out distinct from Tw):
 *   (T w - 1) (dbeta/beta - (dtheta/theta) ln((T w - 1)/beta) + (dln a2 + dln a3)/theta) + (1/theta) J(w) [w .* (dtheta ln w + dln a1)]
 * with theta = (1-gamma)/(1-1/psi) and the log-tangents of the scale tables a1 = exp(theta h_lambda), a2 = exp((1/2)((1-gamma)
 * sigma_c)^2), a3 = exp((1-gamma)(mu_c + z)).  Linearises at w (one linearising application of T, T w into Tw_dev when not
 * NULL) and leaves that linearisation cached for sdfs_apply_jvp_dev / sdfs_solve_linear_dev.  The J.v term is skipped for
 * directions with dtheta = 0 and dln a1 = 0.  SDFS_ERR_UNSUPPORTED: a non-zero tangent of a transition array (SSY arrays
 * 1, 3, 5, 7; GCY 1, 3, 5, 8, 11, 14 -- the persistence parameters move those; see sdfs_param_tangent_gen_dev), or a
 * continuous, dense or sharded handle. */
int sdfs_param_tangent_dev(sdfs_handle* h, const double* w_dev, const double* dparams, const double* const* darrays,
                           double* out_dev, double* Tw_dev);
/* The same with transition matrices that move: `dgen` is NULL (then the call is sdfs_param_tangent_dev) or has ndim entries,
 * each NULL or 3 n_a HOST doubles (sub-, main, super-diagonal by row; sub[0] and super[n_a - 1] are ignored) of a tridiagonal
 * left generator G_a by which the caller states dQ_a = G_a Q_a for every matrix of axis a.  A Rouwenhorst matrix has
 * dTheta_n/drho = G_n Theta_n with G_n[i, i-1] = -i/(2 rho), G_n[i, i] = (n-1)/(2 rho), G_n[i, i+1] = -(n-1-i)/(2 rho), so the
 * persistence parameters are such directions.  With E = ((T w - 1)/beta)^theta / (a2 a3) each generator adds
 *   (T w - 1)/theta . sum_j G_a[i_a, j] E(x with i_a -> j) / E(x)
 * to `out`, one streaming pass per axis after the passes of sdfs_param_tangent_dev.  The transition entries of `darrays` stay
 * NULL or zero (SDFS_ERR_UNSUPPORTED otherwise, as above).  A generator needs every transition tensor of the handle to be
 * unconditional (slice-identical, the condition of sdfs_apply_vjp_dev): SDFS_ERR_UNSUPPORTED otherwise, since the stencil
 * commutes with the other axes' contractions only then.  A non-finite generator entry is SDFS_ERR_ARG. */
int sdfs_param_tangent_gen_dev(sdfs_handle* h, const double* w_dev, const double* dparams, const double* const* darrays,
                               const double* const* dgen, double* out_dev, double* Tw_dev);
/* x = (I - J)^{-1} rhs, or (I - J^T)^{-1} rhs when `transpose` != 0, at the cached linearisation (sdfs_linearize_dev or
 * sdfs_param_tangent_dev): forward sensitivities dw* / dp = (I - J(w*))^{-1} dT/dp, adjoints lambda = (I - J(w*)^T)^{-1} g.
 * BiCGSTAB on the device (x0 = 0, stop when |r|_2 <= max(opts.inner_rtol |rhs|_2, opts.inner_atol), at most
 * opts.inner_max_iter iterations, 0 -> 10 N; opts NULL = defaults), fp64 only: opts.krylov_f32 != 0 is SDFS_ERR_ARG.
 * `transpose` is SDFS_ERR_UNSUPPORTED where sdfs_apply_vjp_dev is.  n_iter (iterations; two products each) and
 * final_rel_resid (|r|_2 / |rhs|_2 of the recursion) may be NULL.  A breakdown or a solve that stops above the tolerance
 * returns SDFS_ERR_NUMERIC, with x and the residual where it stopped. */
int sdfs_solve_linear_dev(sdfs_handle* h, int transpose, const sdfs_opts* opts, const double* rhs_dev, double* x_dev,
                          int64_t* n_iter, double* final_rel_resid);

/* Asset pricing with the SDF M' = beta^theta exp(theta g_lam' - gamma g_c') (w(X') / (w(X) - 1))^(theta-1) at w.  For a power
 * p in {0, 1, 2} of the SDF and exponents (kappa_lam, kappa_c) the tilted expectation is
 *   K f (x) = [beta^theta (Tw(x) - 1)^(1-theta)]^p E_x[exp(kappa_lam g_lam' + kappa_c g_c') w(X')^(p (theta-1)) f(X')]
 *           = d2 .* H'(d1 .* f),   d1 = c1^p e_lam,  d2 = c2^p e_c e_z
 * with (c1, c2) the linearisation at w: (1, theta, 1 - gamma) is J(w) bit for bit; (1, theta, -gamma) gives E_x[M] = K 1,
 * (2, 2 theta, -2 gamma) E_x[M^2], (1, theta, kappa - gamma) the price operator of a claim on G_c^kappa, (0, 0, kappa)
 * the physical E_x[G_c^kappa f].  Discretised unsharded handles only (SDFS_ERR_UNSUPPORTED otherwise); fp64 whatever
 * fp32 solve options the handle has run with.
 *
 * sdfs_set_tilt_dev linearises at w (fp64; replaces the cached linearisation, as sdfs_param_tangent_dev does; w may be
 * NULL when sdf_power = 0, and then nothing is linearised) and forms d1, d2.  The later calls use them and leave the
 * cached linearisation untouched; before a set_tilt they are SDFS_ERR_ARG, as is sdf_power outside {0, 1, 2}. */
int sdfs_set_tilt_dev(sdfs_handle* h, const double* w_dev, int sdf_power, double kappa_lam, double kappa_c);
/* out = K f (device pointers, N doubles each, distinct). */
int sdfs_apply_tilted_dev(sdfs_handle* h, const double* f_dev, double* out_dev);
/* x = (I - K)^{-1} rhs by the device BiCGSTAB (the stopping rule and opts of sdfs_solve_linear_dev; opts.krylov_f32 is
 * ignored: fp64).  SDFS_ERR_NUMERIC for a breakdown or a solve that stops above the tolerance. */
int sdfs_solve_tilted_dev(sdfs_handle* h, const sdfs_opts* opts, const double* rhs_dev, double* x_dev,
                          int64_t* n_iter, double* final_rel_resid);
/* out = d(K f): the tangent of the tilt set by sdfs_set_tilt_dev along a direction that moves the
 * parameters and state arrays (dparams, darrays: HOST, as sdfs_param_tangent_dev; dgen: per-axis left generators
 * dQ = G Q or NULL, as sdfs_param_tangent_gen_dev), the tilt's exponents (dkappa_lam, dkappa_c), the linearisation point
 * w by dw_dev and T w by dtw_dev (the total movement of T w; at a fixed point with dw = dw* / dp it is dw* too, and the
 * two may be one pointer), and f by df_dev:
 *   d(K f) = u2 .* K f + K (u1 .* f + df) + sum_k R .* (G_k along axis k on (K f / R)),
 *   u1 = p (dtheta ln w + (theta-1) dw / w) + dkappa_lam h_lam + kappa_lam dh_lam,
 *   u2 = p (theta dbeta / beta + dtheta ln beta - dtheta ln(Tw - 1) + (1-theta) dTw / (Tw - 1)) + kappa_c dkappa_c sigma_c^2
 *        + kappa_c^2 sigma_c dsigma_c + dkappa_c (mu_c + z) + kappa_c (dmu_c + dz).
 * w_dev is the w of the set_tilt; w_dev, dw_dev, dtw_dev are read for sdf_power >= 1 only (NULL then: SDFS_ERR_ARG) and
 * may be NULL for power 0.  f_dev NULL: f = 1; df_dev NULL: df = 0; kf_dev: K f where the caller has it, NULL: one more
 * product computes it.  out_dev is distinct from every input.  One tilted product per call (two with kf_dev NULL), two
 * streaming passes and one per axis with a generator; two runs give identical bits.  SDFS_ERR_ARG before a set_tilt or
 * for a non-finite exponent tangent; SDFS_ERR_UNSUPPORTED for a non-zero transition-array tangent in darrays (state it
 * as dgen) and for a generator on a handle with a conditional transition tensor. */
int sdfs_tilt_tangent_dev(sdfs_handle* h, const double* w_dev, const double* dw_dev, const double* dtw_dev,
                          const double* dparams, const double* const* darrays, const double* const* dgen,
                          double dkappa_lam, double dkappa_c, const double* f_dev, const double* df_dev,
                          const double* kf_dev, double* out_dev);
/* P_0 = 1, P_n = K P_{n-1} for n = 1 ... n_max on the device, no host synchronisation per horizon.  Row n-1 of out_host
 * (n_max x 4) = <g, P_n>, <g, -log P_n> / n, min and max of P_n / P_{n-1} over the grid (the Collatz-Wielandt bracket of
 * the spectral radius of K), with product-form weights g(x) = prod_a weight_axes[a][x_a] (HOST pointers, shapes[a]
 * doubles each; weight_axes NULL, or an entry NULL: uniform 1 / shapes[a]).  P_n is copied to save_dev[j] (device, N
 * doubles) at the horizons save_at[j] (strictly rising within 1 ... n_max).  The sums are finished in a fixed order: two
 * runs give identical bits.  SDFS_ERR_NUMERIC (results written) if some P_n is not strictly positive. */
int sdfs_tilted_horizons_dev(sdfs_handle* h, int64_t n_max, const double* const* weight_axes, int64_t n_save,
                             const int64_t* save_at, double* const* save_dev, double* out_host);

/* Simulated paths of the discretised chain at w* (unsharded multi-index handles only, else
 * SDFS_ERR_UNSUPPORTED; fp64 whatever the handle's fp32 settings).  The chain must factorise: axis a moves by one
 * n_a x n_a matrix, whose cumulative rows the caller passes (the last entry of each row set to 2).  Step t of path p
 * draws Philox4x32-10 words with counter (t, p, b, 0), b = 0, 1, and key (seed & 0xffffffff, seed >> 32). */
typedef struct sdfs_sim_desc {
  uint64_t seed;
  int64_t path_offset;      /* number of the first path; path_offset + n_paths <= 2^32 */
  int64_t n_paths;
  int64_t burn_in;          /* B >= 0 */
  int64_t n_periods;        /* T >= 2, B + T < 2^32 */
  int32_t has_kappa;        /* the records carry ln v and ln(1 + v) of a claim on G_c^kappa: the series rd, xd, pd */
  int32_t start_fixed;      /* 1: x_0 = start[]; 0: x_0 drawn from the stationary marginals (cdf0) */
  double kappa;
  int32_t start[6];
  int32_t lookahead;        /* record loads in flight per lane: 1, 2 or 4 (0: the default) */
  int32_t search;           /* inverse-CDF search: 1 linear, 2 binary (0: the default) */
  const double* cdf;        /* HOST: per axis in grid order, its n_a x n_a cumulative rows (row-major), concatenated */
  const double* cdf0;       /* HOST: per axis, its n_a cumulative stationary weights, concatenated (NULL with start_fixed) */
} sdfs_sim_desc;
/* One 64-byte record per state into records_dev (N x 8 doubles): {ln w, ln(w - 1), -ln E_x[M], mu_c + z(x), w, ln v,
 * ln(1 + v), 0}, with E_x[M] = K(1, theta, -gamma) 1 formed by sdfs_set_tilt_dev(w, 1, theta, -gamma) and
 * sdfs_apply_tilted_dev (so the cached linearisation and the tilt are those of that call afterwards).  v_dev (N doubles)
 * may be NULL: the two fields are then 0. */
int sdfs_sim_records_dev(sdfs_handle* h, const double* w_dev, const double* v_dev, double* records_dev);
/* desc->n_paths paths of desc->n_periods recorded steps after desc->burn_in, one lane per path, from the records of
 * sdfs_sim_records_dev.  stats_dev: (3 nser + 1) x n_paths doubles, structure of arrays: mean, std, ac1 of series
 * k at rows 3k ... 3k+2, the slope last; series dc, m, rf, rc, xc, wc (nser = 6), and rd, xd, pd with a claim (nser = 9).
 * idx_dev (n_paths x (T+1) x ndim bytes: x_B ... x_{B+T}) and series_dev (nser x n_paths x T doubles) are both NULL or
 * both set; set, they run with the default lookahead and search.  No host synchronisation; two runs give identical bits. */
int sdfs_sim_paths_dev(sdfs_handle* h, const double* records_dev, const sdfs_sim_desc* desc, double* stats_dev,
                       uint8_t* idx_dev, double* series_dev);

/* Simulated paths of the continuous-state model at w* (handles of sdfs_create_continuous only, else
 * SDFS_ERR_UNSUPPORTED; fp64).
 *
 * em = E_x[M] of the handle's nodes and weights on the grid (device pointers, N doubles each, distinct):
 *   beta^theta (w(x) - 1)^(1 - theta) exp(-gamma (mu_c + z) + gamma^2 sigma_c(x)^2 / 2)
 *     * sum_m W_m exp(theta h_lambda'(x, m)) lin_interp(w)(x'(x, m))^(theta - 1)
 * by T's kernel with the exponent theta - 1 on the interpolant, on the gather path T takes.  NaN where w <= 1. */
int sdfs_cont_sdf_mean_dev(sdfs_handle* h, const double* w_dev, double* em_dev);
/* One 16-byte record {w, -ln E_x[M]} per grid point into records_dev (N x 2 doubles, 16-byte aligned). */
int sdfs_cont_sim_records_dev(sdfs_handle* h, const double* w_dev, const double* em_dev, double* records_dev);
/* Step s0 + k of path p (s0 = step_offset) draws the Philox4x32-10 blocks b = 0, 1 with counter (s0 + k, p, b, 1) and key
 * (seed & 0xffffffff, seed >> 32); the words r0 ... r3 of a block give the normals n_4b ... n_4b+3 by Box-Muller
 * (u = (r0 + 0.5) 2^-32, phi = 2 pi r1 2^-32: sqrt(-2 ln u) cos phi, sqrt(-2 ln u) sin phi; r2, r3 likewise); eta_d = n_d for
 * d < ndim in the handle's state order, xi = n_ndim.  x_k = next_state(x_{k-1}, eta_k) (the reference's); steps 1 ... B
 * are burn-in, B+1 ... B+T recorded. */
typedef struct sdfs_cont_sim_desc {
  uint64_t seed;
  int64_t path_offset;      /* number of the first path; path_offset + n_paths <= 2^32 */
  int64_t n_paths;
  int64_t burn_in;          /* B >= 0 */
  int64_t n_periods;        /* T >= 2 */
  int64_t step_offset;      /* s0 >= 0, s0 + B + T < 2^32 */
  int32_t start_mode;       /* x_0: 0 the zero state, 1 start[] for every path, 2 start_dev */
  int32_t lookahead;        /* states interpolated side by side: 1, 2 or 4 (0: the default) */
  int32_t group;            /* corners loaded together: 4, 8 or, in 6-D with lookahead <= 2, 16 (0: the default) */
  int32_t reserved;
  double start[6];
  const double* start_dev;  /* DEVICE: n_paths x ndim, the start of every path of this call */
} sdfs_cont_sim_desc;
/* desc->n_paths paths, one lane each, from the records of sdfs_cont_sim_records_dev, whose two fields are interpolated
 * along the path (multilinear, coordinates clamped to the grid as lin_interp clamps them).  stats_dev: 19 x n_paths
 * doubles, structure of arrays: mean, std, ac1 of series k at rows 3k ... 3k+2 for dc, m, rf, rc, xc, wc, then the OLS
 * slope of xc_t on ln(w(x_{t-1}) - 1).  clamped_dev: n_paths counts of recorded steps whose x_t lay outside the grid on
 * some axis.  final_state_dev: n_paths x ndim, x_{B+T}.  states_dev (n_paths x (T+1) x ndim: x_B ... x_{B+T}) and
 * series_dev (6 x n_paths x T) are both NULL or both set; set, they run with the default lookahead and group.  No host
 * synchronisation and no atomics; a path's output depends only on its number, the seed, s0, its start and the model. */
int sdfs_cont_sim_paths_dev(sdfs_handle* h, const double* records_dev, const sdfs_cont_sim_desc* desc, double* stats_dev,
                            uint32_t* clamped_dev, double* final_state_dev, double* states_dev, double* series_dev);
/* The same paths with the return series of a claim on G_c^kappa.  v_dev: the claim's price-dividend ratio
 * on the grid (N doubles, positive; what sdfs_cont_solve_tilted_dev returns for K(1, theta, kappa - gamma), or any grid
 * function).  sdfs_cont_sim_claim_records_dev writes one 32-byte record {w, -ln E_x[M], v, 0} per grid point into
 * records_dev (N x 4 doubles, 32-byte aligned), and sdfs_cont_sim_claim_paths_dev interpolates its three fields with the
 * same clamped cell and offsets: with v^ the interpolant of v,
 *   rd_t = kappa dc_t + ln(1 + v^(x_t)) - ln v^(x_{t-1}),  xd_t = rd_t - rf_t,  pd_t = ln v^(x_t).
 * stats_dev: 28 x n_paths doubles: mean, std, ac1 of dc, m, rf, rc, xc, wc, rd, xd, pd at rows 3k ... 3k+2, then the OLS
 * slope of xd_t on pd_{t-1}.  series_dev: 9 x n_paths x T.  The six base series, the states, clamped_dev and
 * final_state_dev have the bits sdfs_cont_sim_paths_dev gives for the same desc.  desc->lookahead: 0 or 1; desc->group: 0
 * (the default), 4 or 8; kappa finite; anything else is SDFS_ERR_ARG before any launch. */
int sdfs_cont_sim_claim_records_dev(sdfs_handle* h, const double* w_dev, const double* em_dev, const double* v_dev,
                                    double* records_dev);
int sdfs_cont_sim_claim_paths_dev(sdfs_handle* h, const double* records_dev, const sdfs_cont_sim_desc* desc, double kappa,
                                  double* stats_dev, uint32_t* clamped_dev, double* final_state_dev, double* states_dev,
                                  double* series_dev);

/* Asset prices of the continuous-state model at w (handles of sdfs_create_continuous only, else
 * SDFS_ERR_UNSUPPORTED; fp64).  With the handle's nodes eta_m and weights W_m, x'_m = next_state(x, eta_m) and ^ the
 * multilinear interpolant of lin_interp (clamped coordinates), for a power p in {0, 1, 2} of the SDF:
 *   K f (x) = d2(x) sum_m W_m exp(kappa_lam s_lam eta_0m) w^(x'_m)^(p (theta-1)) f^(x'_m)
 *   d2(x)   = [beta^theta (w(x) - 1)^(1-theta)]^p exp(kappa_c (mu_c + z) + kappa_c^2 sigma_c(x)^2 / 2 + kappa_lam rho_lam h_lam)
 * -- the K of sdfs_set_tilt_dev with the quadrature in place of H' and w(x) - 1 where that one has Tw(x) - 1 (what
 * sdfs_cont_sdf_mean_dev does: (1, theta, -gamma) applied to 1 is its E_x[M]).  (1, theta, 1 - gamma) is J(w) up to
 * |theta - 1| |Tw - w| / (w - 1); (2, 2 theta, -2 gamma) applied to 1 is E_x[M^2]; (1, theta, kappa - gamma) is the price
 * operator of a claim on G_c^kappa; (0, 0, kappa) the physical E_x[G_c^kappa f].  K runs on the gather path T takes.
 *
 * sdfs_cont_set_tilt_dev copies w (the caller's buffer is free afterwards; NULL allowed when sdf_power = 0), writes d2
 * (NaN where sdf_power > 0 and w <= 1) and the tilted node weights.  It leaves the cached linearisation untouched: a J.v
 * before and after gives the same bits.  SDFS_ERR_ARG: sdf_power outside {0, 1, 2}, sdf_power > 0 without w, non-finite
 * exponents; for the later calls, any call before a set_tilt. */
int sdfs_cont_set_tilt_dev(sdfs_handle* h, const double* w_dev, int sdf_power, double kappa_lam, double kappa_c);
/* out = K f (device pointers, N doubles each, distinct: f == out is SDFS_ERR_ARG). */
int sdfs_cont_apply_tilted_dev(sdfs_handle* h, const double* f_dev, double* out_dev);
/* x = (I - K)^{-1} rhs by the device BiCGSTAB (the stopping rule and opts of sdfs_solve_linear_dev; fp64).
 * SDFS_ERR_NUMERIC for a breakdown or a solve that stops above the tolerance. */
int sdfs_cont_solve_tilted_dev(sdfs_handle* h, const sdfs_opts* opts, const double* rhs_dev, double* x_dev,
                               int64_t* n_iter, double* final_rel_resid);
/* P_0 = 1, P_n = K P_{n-1} for n = 1 ... n_max (1 ... 2^24) on the device, no host synchronisation per horizon.
 * price_host (n_max x nq) = P_n interpolated at the nq query states (`states`: HOST, laid out [ndim][nq], finite; nq may
 * be 0); bracket_host (n_max x 2) = min and max of P_n / P_{n-1} over the grid (the Collatz-Wielandt bracket of the
 * spectral radius of K).  P_n is copied to save_dev[j] (device, N doubles) at the horizons save_at[j] (strictly rising
 * within 1 ... n_max; anything else is SDFS_ERR_ARG).  The reductions are finished in a fixed order, no atomics: two
 * runs give identical bits.  SDFS_ERR_NUMERIC (results written) if some P_n leaves the positive finite numbers. */
int sdfs_cont_tilted_horizons_dev(sdfs_handle* h, int64_t n_max, const double* states, int64_t nq, int64_t n_save,
                                  const int64_t* save_at, double* const* save_dev, double* price_host, double* bracket_host);

/* The parameter tangent of the continuous-state operator (handles of sdfs_create_continuous only, else
 * SDFS_ERR_UNSUPPORTED; fp64): out = dT(w; p)[dparams], the derivative of T at the fixed grid function w along the
 * direction dparams (HOST, 13 / 18 doubles in sdfs_create_continuous's parameter order; every parameter, the persistences
 * included), with the handle's grids, nodes and weights held fixed -- jax.jvp of the reference's T with respect to the
 * parameters with `grids, nodes, weights` closed over.  build_grid depends on the parameters too: the movement of the
 * grid is NOT part of this derivative.  The tangent passes through the multilinear interpolant (the slope of w^ along the
 * direction each node moves; zero where map_coordinates clamps the coordinate, one-sided where a node sits on a grid
 * line) and through ln w^ (theta is an exponent).  One launch on the gather path T takes; fixed-order reduction, no
 * atomics: two runs give identical bits.  Tw_dev (may be NULL) receives T w.  Like sdfs_param_tangent_dev the call
 * linearises at w, so sdfs_apply_jvp_dev and sdfs_solve_linear_dev can follow: dw-star/dp = (I - J)^{-1} out.
 * SDFS_ERR_ARG: NULL w / dparams / out, a non-finite direction, or w, out, Tw not pairwise distinct. */
int sdfs_cont_param_tangent_dev(sdfs_handle* h, const double* w_dev, const double* dparams, double* out_dev, double* Tw_dev);

/* The transposed Jacobian of the continuous-state operator and the adjoint solve on it (handles of
 * sdfs_create_continuous only, else SDFS_ERR_UNSUPPORTED; fp64).
 *
 *   out[j] = sum_x c2(x) u(x) sum_m W_m g_m(x)^(theta-1) phi_j(x'(x, m))   (- u[j] with minus_identity),
 *
 * at the cached linearisation (sdfs_linearize_dev or sdfs_cont_param_tangent_dev; left untouched), phi_j the multilinear
 * hat weight of grid point j at the clamped next state: the cells and weights sdfs_apply_jvp_dev reads with, so out is the
 * exact transpose of what that call computes: <u, J v> = <J^T u, v> to rounding.  A gather through an interpolant
 * transposes into a scatter: one launch on the gather path T takes, out zeroed in-stream ahead of it, every
 * contribution added with a hardware fp64 atomic add (LDS accumulators per grid point, then global memory); u is
 * subtracted in one pass behind it, so out with minus_identity is one rounding away from out without.
 *
 * RESULTS ARE REPRODUCIBLE TO ROUNDING ONLY.  The last bits of out depend on the order in which the atomic adds arrive;
 * two runs on the same input differ by a few units of rounding of the sum of the magnitudes.  These are the library's
 * only entry points without bit-for-bit repeatability (every other reduction is finished in a fixed order), which is why
 * they carry names of their own: sdfs_apply_vjp / sdfs_apply_vjp_dev / sdfs_solve_linear_dev(transpose != 0) keep
 * returning SDFS_ERR_UNSUPPORTED on a continuous handle.
 *
 * out_dev must be ORDINARY device memory (hipMalloc; not fine-grained, host-pinned or managed memory: hardware
 * floating-point atomics are not defined there).  SDFS_ERR_ARG: NULL u / out, u == out, or no linearisation yet. */
int sdfs_cont_apply_vjp_dev(sdfs_handle* h, const double* u_dev, double* out_dev, int minus_identity);
/* x = (I - J^T)^{-1} rhs at the cached linearisation by the device BiCGSTAB on the product above: the adjoint
 * lambda = (I - J(w*)^T)^{-1} g of d<g, w*>/dp_k = <lambda, dT/dp_k> (sdfs_cont_param_tangent_dev), one solve for all
 * parameters.  Stopping rule, opts, n_iter, final_rel_resid and SDFS_ERR_NUMERIC as sdfs_solve_linear_dev (fp64 only:
 * opts.krylov_f32 != 0 is SDFS_ERR_ARG).  Reproducible to rounding only, as the product is; iteration counts may differ by
 * one between runs where a residual sits on the tolerance.  SDFS_ERR_ARG: NULL rhs / x, or no linearisation yet. */
int sdfs_cont_solve_adjoint_dev(sdfs_handle* h, const sdfs_opts* opts, const double* rhs_dev, double* x_dev, int64_t* n_iter,
                                double* final_rel_resid);

/* max|T(w) - w| of the most recent apply that computed it. */
int sdfs_residual(sdfs_handle* h, double* sup_norm);

/* Fixed-point solve, all iterations on the device.  Replaces
 * successive_approx / newton_solver / anderson_solver (code/solvers.py:19-124):
 * w_inout holds x_init on entry and x_star on return; n_iter is the value the
 * reference returns as its second tuple element; n_apply counts operator and
 * JVP applications; final_err is the last value of the solver's own error. */
int sdfs_solve(sdfs_handle* h, int algo, const sdfs_opts* opts, double* w_inout_host,
               int64_t* n_iter, int64_t* n_apply, double* final_err);
int sdfs_solve_dev(sdfs_handle* h, int algo, const sdfs_opts* opts, double* w_inout_dev,
                   int64_t* n_iter, int64_t* n_apply, double* final_err);
/* Error trace of the last solve (record_errors = 1): copies min(cap, n) values. */
int64_t sdfs_error_trace(sdfs_handle* h, double* out, int64_t cap);

/* Multi-GPU building block: run the local kernels of one operator application.
 * stage 0: contractions that need no other rank's data (input sharded on axis_a);
 * stage 1: after the grid re-shard (input sharded on axis_b): the contractions left over -- axis_a among them -- and the
 * aggregator.  Which complete axes are contracted in which stage is the library's choice (the expectation is a Kronecker
 * product, the order is free: 6-D grids of the compile-time pair plan leave axis_a's partner axis to stage 1, so that both
 * stages run that plan's kernels), so what stage 0 writes is an intermediate only the same handle's stage 1 understands.
 * `mode` 0 = T, 1 = JVP (uses the cached linearisation), 2 = T + linearise. */
int sdfs_apply_stage_dev(sdfs_handle* h, int stage, int mode, const double* in_dev,
                         double* out_dev, const double* w_old_dev, double* resid_dev);

/* The same launch behind a device-side gate (multi-GPU successive approximation without a host read per iteration:
 * sdfs_via_autodiff_amd/distributed.py; the loop it serves is code/solvers.py:34-36).  gate_dev points at a device
 * double -- the all-reduced error of the previous iteration; if *gate_dev <= gate_tol (both non-negative) every
 * kernel of the stage returns at once and `out_dev` keeps its contents, and resid_dev, if given, is left at 0, which
 * keeps every later gate on it closed.  gate_dev == NULL: ungated. */
int sdfs_apply_stage_gated_dev(sdfs_handle* h, int stage, int mode, const double* in_dev, double* out_dev,
                               const double* w_old_dev, double* resid_dev, const double* gate_dev, double gate_tol);

/* Exchange buffers of the re-shard between two stage calls (sdfs_via_autodiff_amd/distributed.py; the reference has no
 * multi-GPU path).  The grid is viewed as [outer][n_axis][inner] in C order; `packed` is the concatenation
 * over the nblocks blocks j (axis indices offs[j] .. offs[j+1], offs[0] = 0, offs[nblocks] = n_axis) of
 * [outer][size_j][inner], i.e. what every peer sends or receives is one contiguous piece.  unpack = 0: src is the
 * grid, dst the packed buffer; unpack = 1: the reverse.  elem_bytes 8 (fp64) or 4 (fp32 Krylov streams).  One launch on
 * the handle's stream. */
int sdfs_pack_blocks(sdfs_handle* h, int unpack, const void* src_dev, void* dst_dev, int64_t outer, int64_t n_axis,
                     int64_t inner, int nblocks, const int64_t* offs, int elem_bytes);

/* Multi-GPU Krylov building blocks: the fused BLAS-1 kernels of the single-GPU BiCGSTAB / Newton loops
 * (jax.scipy.sparse.linalg.bicgstab inside code/solvers.py:91-93) on caller-owned device vectors of `n` LOCAL
 * elements -- this rank's shard -- with the scalar recurrences in the handle's device block.  A step either
 * leaves the rank's partial sums in `sums_dev` (the caller all-reduces them, SUM; MAX for the Newton step) or
 * consumes the all-reduced values from it.  v = {b, r, rhat, p, q, t, x} (b fp64; the others fp64, or fp32 when
 * f32 != 0).  Sequence per solve:  INIT -> [all-reduce 1] -> INIT_FIN;  per iteration:  UPDATE_P, (q = J p - p by
 * the caller), DOT_RQ -> [1] -> ALPHA_S -> [1] -> S_FIN, (t = J s - s, s lives in r), DOT_TS -> [2] -> OMEGA_XR
 * -> [2] -> ITER_FIN; sdfs_krylov_scalars reads the block back (one synchronisation per iteration). */
enum { SDFS_KS_INIT = 0, SDFS_KS_INIT_FIN, SDFS_KS_UPDATE_P, SDFS_KS_DOT_RQ, SDFS_KS_ALPHA_S, SDFS_KS_S_FIN,
       SDFS_KS_DOT_TS, SDFS_KS_OMEGA_XR, SDFS_KS_ITER_FIN, SDFS_KS_SUB_DOT, SDFS_KS_NEWTON_UPDATE };
enum { SDFS_SC_RR = 9, SDFS_SC_BB = 10, SDFS_SC_ATOL2 = 11, SDFS_SC_BREAK = 13, SDFS_SC_ITERS = 15 };   /* indices into the scalar block */
int sdfs_krylov_step(sdfs_handle* h, int step, int64_t n, int f32, void* const* v, double* sums_dev,
                     double rtol, double atol);
int sdfs_krylov_scalars(sdfs_handle* h, double* out16_host);
/* step | SDFS_KS_GATED: the kernels of the step return at once while the handle's gate word is closed.  INIT_FIN opens it
 * when |b|^2 is above the stopping level, ITER_FIN closes it on convergence, breakdown or a non-finite |r|^2 -- the gate
 * of the single-GPU loop (csrc/vec_kernels.hpp) -- so a caller enqueues several iterations (stage launches gated on the
 * same word: sdfs_krylov_gate + sdfs_apply_stage_gated_dev with gate_tol 0, all-reduces on whatever the sums buffer
 * holds) per sdfs_krylov_scalars; the iterates and SDFS_SC_ITERS are those of the one-iteration-per-read loop. */
enum { SDFS_KS_GATED = 0x100 };
int sdfs_krylov_gate(sdfs_handle* h, const void** gate_dev);
/* sdfs_pack_blocks(unpack = 1) with the Krylov operator's "- v" folded in: grid_out = unpacked - sub_dev (sub_dev laid out
 * like grid_out; fp64 or fp32 by elem_bytes).  (J - I) v then costs the J v stages plus ONE extra stream in the pass that
 * scatters the exchanged result back, instead of a subtraction and a copy over the whole shard. */
int sdfs_unpack_blocks_sub(sdfs_handle* h, const void* packed_dev, void* grid_out_dev, const void* sub_dev, int64_t outer,
                           int64_t n_axis, int64_t inner, int nblocks, const int64_t* offs, int elem_bytes);
/* sdfs_pack_blocks(unpack = 1) behind a gate word of the handle (sdfs_anderson_gate, sdfs_krylov_gate): the launch returns at
 * once while the word is 0 and grid_out keeps its contents.  The sharded Anderson loop lands T x in its two iterate buffers
 * through this call, so that the passes a chunk enqueues behind the pass that ended the loop cannot overwrite the iterate
 * that pass left (the stage kernels in front of it are gated on the same word). */
int sdfs_unpack_blocks_gated(sdfs_handle* h, const void* packed_dev, void* grid_out_dev, int64_t outer, int64_t n_axis,
                             int64_t inner, int nblocks, const int64_t* offs, int elem_bytes, const void* gate_dev);

/* Anderson acceleration (jaxopt.AndersonAcceleration as called at code/solvers.py:104-114; semantics restated in
 * oracle/solvers.py, iterate parity unpinned) on a SHARDED grid: the single-GPU loop's large-grid kernels
 * (csrc/vec_kernels.hpp: history as Y_j = x_j + beta r_j and r_j, <r, r> per pass, the whole Gram matrix in one sweep
 * where a solve is due) on this rank's n local points, the loop's control -- Gram matrix, the (m+1)^2 solve, the
 * domain safeguard, the stopping test -- in the handle's device state, identical on every rank because it only ever sees
 * all-reduced sums.  Sequence per pass i (0, 1, ...):  x_out = T(x_in) by the caller (stage launches gated on
 * sdfs_anderson_gate, gate_tol 0);  PUSH -> [all-reduce SUM sums[0]];  if (i + 1) % mixing_freq == 0: GRAM -> [all-reduce SUM
 * sums[1 .. 1 + SDFS_AND_NPAIRS)];  STEP;  MIX (x_out becomes the next iterate: pass i + 1 reads it as x_in, so the caller
 * alternates two buffers).  Every kernel is a no-op once the loop has ended; sdfs_anderson_state reads the state back
 * (out8 = passes executed, error = |T x - x|_2 of the last pass, 1 while the loop runs, 1 if a non-finite residual ended it,
 * rejected mixing steps, ...) and the errors of passes first .. first + count (a ring of 256).  history <= 12; the history
 * buffers hold history * n doubles each and stay the caller's. */
enum { SDFS_AND_PUSH = 0, SDFS_AND_GRAM = 1, SDFS_AND_STEP = 2, SDFS_AND_MIX = 3 };
enum { SDFS_AND_NPAIRS = 78 };
int sdfs_anderson_begin(sdfs_handle* h, int64_t n, int history, double* y_hist_dev, double* r_hist_dev, double tol,
                        int64_t max_iter, double beta, double ridge, int mixing_freq);
int sdfs_anderson_gate(sdfs_handle* h, const void** gate_dev);
int sdfs_anderson_step(sdfs_handle* h, int step, int64_t pass, const double* x_in_dev, double* x_out_dev, double* sums_dev);
int sdfs_anderson_state(sdfs_handle* h, double* out8_host, double* errs_host, int64_t first_pass, int64_t count);
/* Sharded handles: fp32 storage of the J.v streams and of the linearisation (opts.krylov_f32 of the single-GPU
 * solve) for the stage calls that follow.  `w_ref`: one positive value shared by all ranks (e.g. the geometric
 * mean of the all-reduced min and max of the iterate) from which every rank and both stages derive the same
 * power-of-two scale of c1 / c2. */
int sdfs_set_krylov_f32(sdfs_handle* h, int on, double w_ref);

/* Sharded handles whose stages run the pair plan's kernels (6-D grids, sdfs_describe_plan says "pair-plan"): fp32
 * intermediates for the plain applications of T that follow (mode 0; opts.t_f32 of the single-GPU successive
 * approximation, code/solvers.py:19-48 is the loop).  Stage 0 then WRITES scaled floats -- the re-shard between the stages
 * moves half the bytes -- and stage 1 reads them; w, T w and the residual stay fp64.  One stored float carries 2^-24
 * relative, ~ w 2^-24 / |theta| on T w: the caller runs this form while the step is well above that and finishes in fp64
 * (sdfs_via_autodiff_amd/distributed.py, successive_approx_sharded(t_f32=True)).  `w_ref` as for sdfs_set_krylov_f32: every
 * rank and both stages derive the same power-of-two scale from it.  SDFS_ERR_UNSUPPORTED on handles with generic stage plans. */
int sdfs_set_t_f32(sdfs_handle* h, int on, double w_ref);

/* Profiling: when enabled every kernel launch is bracketed by HIP events on the
 * handle's stream; sdfs_get_counters synchronises and sums them. */
int sdfs_set_profiling(sdfs_handle* h, int on);
int sdfs_reset_counters(sdfs_handle* h);
int sdfs_get_counters(sdfs_handle* h, sdfs_counters* out);

/* Test hook: out[i] = x[i]^y through the kernels' own device power routine (the
 * replacement for jnp's `**` at ssy_wc_ratio.py:145,148 / gcy_wc_ratio.py:232,235),
 * so that its accuracy can be checked in isolation. */
int sdfs_debug_pow(const double* x_host, double y, double* out_host, int64_t n, int device_id);
/* The same for the routine the kernels use when the exponent is fixed for a launch (theta in the first pass of T,
 * 1/theta in the last; csrc/pass_kernel.hpp, powy): degree 6 = the form inside the operator kernels (|y| * 1.04e-17
 * polynomial error on x^y), degree 7 = accurate for any |y| <= 64, degree 0 = sdfs_debug_pow. */
int sdfs_debug_powy(const double* x_host, double y, double* out_host, int64_t n, int degree, int device_id);
/* Test hook: one J.v product in the reduced-precision storage of Newton's inner solve.  Sets the handle's storage flags
 * as sdfs_solve does for opts.krylov_f32 = `krylov_f32` (0: fp64, 1: fp32, 2: bf16-rounded fp32, 3: fp32 with the pair
 * plan's fp32-MFMA kernels), linearises at w_dev in that storage (c1 / c2 as scaled floats), runs one J.v application
 * (out = J v, or J v - v when `minus_identity`) and restores the flags.  v_dev and out_dev hold N floats when `krylov_f32`
 * != 0 and N doubles when it is 0.  A reduced-precision call leaves c1 / c2 as floats and marks the cached linearisation
 * invalid: sdfs_apply_jvp_dev, sdfs_apply_vjp_dev and sdfs_solve_linear_dev then return SDFS_ERR_ARG until the next
 * sdfs_linearize_dev or sdfs_param_tangent_dev.  SDFS_ERR_UNSUPPORTED for a non-zero `krylov_f32` on continuous, dense or
 * sharded handles (sdfs_solve ignores the option there). */
int sdfs_debug_jvp_storage_dev(sdfs_handle* h, int krylov_f32, const double* w_dev, const void* v_dev, void* out_dev,
                               int minus_identity);

/* Measurement aid (bench.py's `copy_ceiling_GBps`; no counterpart in the reference): dst[0..n) = src[0..n) by the library's
 * own streaming copy -- one launch on the handle's stream, 16 bytes per lane, eight loads in flight per lane, non-temporal
 * loads and stores: what a pass that reads and writes every grid point once can reach on this box.  Buffers 16-byte
 * aligned, not overlapping. */
int sdfs_stream_copy_dev(sdfs_handle* h, const double* src_dev, double* dst_dev, int64_t n);

/* Human-readable description of the kernel plan (passes, tiles, grid sizes). */
int sdfs_describe_plan(const sdfs_handle* h, char* buf, int64_t cap);

/* ---- Batched successive approximation: B parameter vectors of one model on one grid shape ---------------------------
 * The loop of code/solvers.py:19-48 (error = max|x_new - x|, while error > tol and it < max_iter) for B problems at once,
 * one workgroup per problem with the problem's grid in the LDS of its CU (csrc/batch_kernels.hpp); every problem stops on
 * its own.  What an estimation loop (SMM, MCMC, a grid search over gamma or psi) calls instead of B times sdfs_create +
 * sdfs_solve.  fp64; unconditional (slice-identical) transition tensors only, i.e. every Rouwenhorst or Tauchen
 * discretisation; grids that fit 160 KiB of LDS only (sdfs_batch_lds_bytes).  A problem's result depends on its own
 * inputs only: not on B, its position in the batch or check_every. */
typedef struct sdfs_batch sdfs_batch;

enum { SDFS_BATCH_CONVERGED = 0, SDFS_BATCH_MAX_ITER = 1, SDFS_BATCH_NONFINITE = 2 };

/* Dynamic LDS in bytes the batch plan needs for this shape (>= 8 N, <= 163840), SDFS_ERR_UNSUPPORTED if the grid with
 * its tables does not fit one CU or an extent exceeds 32, SDFS_ERR_ARG for a bad model / ndim / extent.  Makes no
 * device call. */
int64_t sdfs_batch_lds_bytes(int model, int ndim, const int64_t* shapes);

/* `params`: B x 13 (SSY) or B x 18 (GCY) scalars, problem-major.  `arrays[i]`: the B copies of array i of sdfs_create,
 * problem-major (array_sizes[i] elements each).  The folded matrices and the a3 table of every problem come from the
 * host code sdfs_create runs, so a problem of the batch is the operator sdfs_create builds from the same inputs. */
int sdfs_batch_create(int model, int ndim, const int64_t* shapes, int64_t B, const double* params,
                      const double* const* arrays, const int64_t* array_sizes, int narrays, int device_id,
                      sdfs_batch** out);
void sdfs_batch_destroy(sdfs_batch* h);
const char* sdfs_batch_last_error(const sdfs_batch* h);   /* h == NULL: the last failed sdfs_batch_create / _lds_bytes */
int sdfs_batch_set_stream(sdfs_batch* h, void* hip_stream, int use_own);   /* as sdfs_set_stream */
int sdfs_batch_synchronize(sdfs_batch* h);

/* One application per problem: Tw[b] = T_b(w[b]), resid[b] = max|Tw[b] - w[b]| (resid_dev may be NULL).  w_dev and
 * Tw_dev: B x N doubles, problem-major; w_dev is not written.  Asynchronous on the handle's stream. */
int sdfs_batch_apply_T_dev(sdfs_batch* h, const double* w_dev, double* Tw_dev, double* resid_dev);

/* Solve all B problems from the start values in w_inout_dev (B x N, results in place).  Read from opts: tol, max_iter,
 * check_every (most iterations of one launch; 0 = the library's choice, sized so that a launch stays near 0.05 s);
 * the other fields are ignored.  Host outputs, B entries each: n_iter, final_err (the last max|x_new - x|; +inf for
 * status 2) and status: 0 converged, 1 max_iter reached, 2 the iterate left the finite range.  Returns when every
 * problem has stopped; a numerical status of a problem is not an error of the call. */
int sdfs_batch_solve_dev(sdfs_batch* h, const sdfs_opts* opts, double* w_inout_dev, int64_t* n_iter, double* final_err,
                         int32_t* status);

/* Newton-Krylov for all B problems from the start values in w_inout_dev (B x N, results in place): the loop of
 * code/solvers.py:51-95 per problem (x <- x - step, step = BiCGSTAB on (J - I) step = T x - x with x0 = 0, stopped when
 * |r|^2 <= max(inner_rtol^2 |T x - x|^2, inner_atol^2), on |s|^2 below that threshold, after inner_max_iter iterations
 * (0 -> 10 N) or on a breakdown (rho, omega or alpha = 0: the step is the x reached so far); error = max|step|, while
 * error > tol and it < max_iter), one workgroup per problem, every problem stopping on its own
 * (csrc/batch_newton.hpp).  As in the reference, a step whose |T x - x|_2 <= inner_atol is exactly 0 and ends the problem
 * as converged.  Read from opts: tol, max_iter, inner_rtol, inner_atol, inner_max_iter and check_every (most
 * applications, T or J.v, of one launch per problem; 0 = the library's choice, sized so that a launch stays near
 * 0.05 s); krylov_f32 != 0 is SDFS_ERR_ARG (the vectors are fp64).  Host outputs, B entries each: n_iter (Newton steps),
 * n_apply (applications of T plus J.v), final_err (the last max|step|; +inf for status 2) and status: 0 converged,
 * 1 max_iter reached (max_iter < 1: before any application), 2 the iterate, a step or an inner product left the finite
 * range or an iterate has a point <= 0.  The eight vectors of a problem live in registers up to 2048 grid points and in
 * global memory beyond (sdfs_batch_describe says which): the handle allocates 7 N doubles per problem at its first
 * Newton solve, at most 2 GiB (or the bytes the environment variable SDFS_BATCH_WS_MAX named at sdfs_batch_create) -- a
 * larger batch runs group after group.  A problem's w, counts and error depend on its own inputs only: not on B, its
 * position in the batch or check_every.  Returns when every problem has stopped. */
int sdfs_batch_newton_dev(sdfs_batch* h, const sdfs_opts* opts, double* w_inout_dev, int64_t* n_iter, int64_t* n_apply,
                          double* final_err, int32_t* status);

/* Doubles per problem of the moment block of sdfs_batch_adjoint_dev.  Layout, with n_lam, n_c the extents of the h_lam
 * and h_c axes (SSY axes 0 and 1, GCY axes 5 and 3) and na3 the entries of the a3 table (SSY [h_z, z]; GCY [z_pi, h_z,
 * h_zpi, z], C order):   s0 s1 s2 | R[ndim] | M1[n_lam] | M2[n_c] | M3[na3]. */
int64_t sdfs_batch_adjoint_words(const sdfs_batch* h);

/* Adjoint moments for all B problems at w_dev (B x N, normally the batch's w*): lambda = (I - J(w)^T)^(-1) g by BiCGSTAB
 * from x0 = 0 with the stopping rule of the Newton kernel's inner solve (|r|^2 <= max(inner_rtol^2 |g|^2, inner_atol^2),
 * the early exit on |s|^2, the breakdown exits, inner_max_iter with 0 -> 10 N), one workgroup per problem
 * (csrc/batch_adjoint.hpp), then with m = lambda (T w - 1), mu = (J^T lambda) w and E = H0(a1 w^theta):
 *   s0 = sum m, s1 = sum m ln((T w - 1) / beta), s2 = sum mu ln w, M1[i_lam] = sum mu over the other axes, M2[i_c] the
 *   same of m, M3[ia3] = sum m over (h_c, h_lam), R[k] = sum m (i_k (E(i_k - 1) / E(i_k) - 1) + (n_k - 1 - i_k)
 *   (E(i_k + 1) / E(i_k) - 1)) per grid axis k,
 * from which  d<g, w*>/dp = dbeta/beta s0 - dtheta/theta s1 + (<M2, dln a2> + <M3, dln a3>)/theta + (dtheta s2 + <M1,
 * dln a1>)/theta - [p = rho_k] R[k] / (2 rho_k theta)  for every parameter (dtheta, dln a1, dln a2, dln a3 as
 * sdfs_param_tangent_dev forms them).  g_dev: B x N with g_stride = N, or one grid for all with g_stride = 0.  lam_dev
 * (B x N) may be NULL.  moments_dev: B x sdfs_batch_adjoint_words(h).  Read from opts: inner_rtol, inner_atol,
 * inner_max_iter and check_every (most applications of one launch per problem; 0 = the library's choice);
 * krylov_f32 != 0 is SDFS_ERR_ARG.  Host outputs, B entries each: n_iter (BiCGSTAB iterations), n_apply (applications:
 * the linearising T, two per full iteration, those of the moment phase), rel_resid (the true |g - lambda + J^T lambda|_2
 * / |g|_2 at the final lambda; where it is above the tolerance after the recurrence's residual has converged, the solve
 * restarts from it, lambda kept, at most twice),
 * resid_T (max|T w - w| at w_dev) and status: 0 converged; 1 stopped above the tolerance (inner_max_iter or a breakdown;
 * the moments are those of lambda where it stopped); 2 a non-finite inner product, w, T w or lambda (the problem's lambda
 * and moments are NaN; no other problem is touched).  g = 0 gives lambda = 0, zero moments, status 0 and n_iter 0.  The
 * vectors live as those of the Newton solve, in its workspace; a problem's lambda, moments and counts depend on its own
 * inputs only: not on B, its position in the batch or check_every. */
int sdfs_batch_adjoint_dev(sdfs_batch* h, const sdfs_opts* opts, const double* w_dev, const double* g_dev, int64_t g_stride,
                           double* lam_dev, double* moments_dev, int64_t* n_iter, int64_t* n_apply, double* rel_resid,
                           double* resid_T, int32_t* status);

/* Asset prices for all B problems at w_dev (B x N, normally the batch's w*), one workgroup per problem
 * (csrc/batch_price.hpp).  With K(p, kl, kc) the tilted operator of sdfs_set_tilt_dev, per problem b:
 *   E_M = K(1, theta, -gamma) 1, log_rf = -ln E_M;  E_M2 = K(2, 2 theta, -2 gamma) 1, hj = sqrt(max(E_M2 / E_M^2 - 1, 0));
 *   v = (I - K)^(-1) K 1 with K = K(1, theta, kappa[b] - gamma) by BiCGSTAB (the price-dividend ratio of the claim on
 *   G_c^kappa);  ER = K(0, 0, kappa[b])(1 + v) / v, lp = ln ER + ln E_M;
 *   P_n = K(1, theta, kappa_ts[b] - gamma) P_(n-1), P_0 = 1, n = 1 .. n_max.
 * kappa (host, B entries) may be NULL: no claim.  kappa_ts (host, B entries) is read when n_max > 0.  weights (host,
 * B x sum n_a): the per-axis weight vectors g_a of every problem, axis-major; the weight of a point is prod_a g_a[i_a].
 * EM_dev, EM2_dev, pd_dev, ER_dev (B x N each) may be NULL.  moments_dev: B x SDFS_BATCH_PRICE_WORDS,
 *   0 sum g | 1 <g,log_rf> 2 <g,log_rf^2> | 3 <g,hj> | 4 <g,ln v> 5 <g,(ln v)^2> | 6 <g,ln ER> | 7 <g,lp> 8 <g,lp^2> |
 *   9 min v 10 max v | 11 number of points with v <= 0;  words 4-11 are NaN without a claim.
 * horizons_dev: B x n_max x 4 (<g,P_n>, <g,-ln P_n> / n, min and max of P_n / P_(n-1)); may be NULL when n_max == 0.  A
 * horizon whose P_n has a non-positive or non-finite point ends that problem's loop: n_horizons[b] rows were written and
 * the later ones are NaN.  Read from opts: inner_rtol, inner_atol, inner_max_iter (0 -> 10 N), check_every (applications
 * per launch, 0 = the library's choice); krylov_f32 != 0 is SDFS_ERR_ARG, and so are non-finite kappa, kappa_ts or
 * weights and n_max < 0 or > 2^24, before any device work.  Host outputs of length B: n_iter (BiCGSTAB iterations),
 * n_apply (operator applications), n_horizons, rel_resid (the true |K1 - v + K v|_2 / |K1|_2; NaN without a claim),
 * resid_T (max|T w - w|) and status: SDFS_BATCH_CONVERGED done, SDFS_BATCH_MAX_ITER the claim solve stopped above its
 * tolerance (the words are those of v where it stopped), SDFS_BATCH_NONFINITE (the problem's outputs are NaN),
 * SDFS_BATCH_NO_PRICE the solve converged but v is not strictly positive: r(K) >= 1, words 4-8 are NaN, 9-11 kept, E_M
 * and the horizons delivered.  The call uses the Newton workspace (allocated on first use) and leaves the handle's solve,
 * Newton and adjoint state alone.  A problem's results depend on its own inputs only: not on B, its position in the batch
 * or check_every. */
enum { SDFS_BATCH_NO_PRICE = 3 };
#define SDFS_BATCH_PRICE_WORDS 12
int sdfs_batch_price_dev(sdfs_batch* h, const sdfs_opts* opts, const double* w_dev, const double* kappa, const double* kappa_ts,
                         const double* weights, int64_t n_max, double* EM_dev, double* EM2_dev, double* pd_dev, double* ER_dev,
                         double* moments_dev, double* horizons_dev, int64_t* n_iter, int64_t* n_apply, int64_t* n_horizons,
                         double* rel_resid, double* resid_T, int32_t* status);

/* Simulated paths for all B problems at the batch's w* (csrc/batch_sim.hpp): the chain, the random
 * numbers, the series and the per-path statistics of sdfs_sim_paths_dev, on a launch grid of (workgroups per member,
 * members), and the cross-path moments of every statistic reduced on the device.  One seed serves all members (common
 * random numbers); a path's indices, series and statistics depend only on its number, the seed and its member's inputs,
 * not on B or the member's place in the batch. */
typedef struct sdfs_batch_sim_desc {
  uint64_t seed;
  int64_t path_offset;      /* number of the first path; path_offset + n_paths <= 2^32 */
  int64_t n_paths;          /* per member */
  int64_t burn_in;          /* >= 0 */
  int64_t n_periods;        /* T >= 2, burn_in + T < 2^32 - 8 */
  int32_t has_kappa;        /* the records carry ln v and ln(1 + v): the series rd, xd, pd */
  int32_t start_fixed;      /* 1: x_0 = start[]; 0: x_0 drawn from every member's stationary marginals (cdf0) */
  int32_t start[6];
  int32_t records;          /* where a path-step reads its record: 1 LDS, 2 global memory, 0 the default of the shape */
  int32_t lookahead;        /* global form: record loads in flight per lane, 1, 2 or 4 (0: the default) */
  int32_t search;           /* inverse-CDF search: 0 or 2 (bisection); 1 (linear) is SDFS_ERR_UNSUPPORTED */
  int32_t reserved;
  const double* kappa;      /* HOST: B leverages (read with has_kappa) */
  const double* cdf;        /* HOST: per member, then per axis in grid order, the n_a x n_a cumulative rows (last entry 2) */
  const double* cdf0;       /* HOST: per member, then per axis, the n_a cumulative stationary weights (NULL with start_fixed) */
  const int32_t* skip;      /* HOST: B flags, nonzero = the member runs no path and its outputs are NaN; NULL: none */
} sdfs_batch_sim_desc;
/* Dynamic LDS in bytes of the path kernel for this shape with records == 1 (tables + N x 64 B of records + the reduction
 * slots) or records == 2 (tables + slots); SDFS_ERR_UNSUPPORTED where the shape is beyond the batch plan or, with
 * records == 1, the records do not fit one CU.  Makes no device call. */
int64_t sdfs_batch_sim_lds_bytes(int model, int ndim, const int64_t* shapes, int records);
/* The table blocks sdfs_batch_sim_paths_dev uploads for a request, formed on the host by the code that call and
 * sdfs_batch_create run (no device call): tab_out B x words, per member the cumulative rows per axis, the cumulative
 * stationary marginals (2 everywhere with start_fixed), h_lambda and sigma_c, padded to an even count; scal_out B x 4 =
 * theta, theta ln beta, gamma, kappa (0 without a claim or for a skipped member); zt_out (may be NULL) B x na3 = mu_c + z
 * in the a3 layout, the table of sdfs_batch_sim_records_dev.  The first eight arguments are those of sdfs_batch_create.
 * Returns words (also with the three outputs NULL, which only asks for it), or an error code. */
int64_t sdfs_batch_sim_tables(int model, int ndim, const int64_t* shapes, int64_t B, const double* params,
                              const double* const* arrays, const int64_t* array_sizes, int narrays,
                              const sdfs_batch_sim_desc* desc, double* tab_out, double* scal_out, double* zt_out);
/* One 64-byte record per state and member into records_dev (B x N x 8): the fields of sdfs_sim_records_dev from w_dev,
 * em_dev (E_x[M], e.g. EM_dev of sdfs_batch_price_dev) and v_dev (pd_dev of that call; NULL: no claim), B x N each.
 * Asynchronous on the handle's stream. */
int sdfs_batch_sim_records_dev(sdfs_batch* h, const double* w_dev, const double* em_dev, const double* v_dev,
                               double* records_dev);
/* stats_dev: B x (3 nser + 1) x n_paths, rows as sdfs_sim_paths_dev (may be NULL).  moments_dev: B x (3 nser + 1) x 3 =
 * (n, mean, se) over a member's paths of every statistic: n counts the finite values (a NaN statistic, i.e. a zero
 * denominator, is left out), se = sqrt(M2 / (n - 1) / n), NaN for n < 2 (may be NULL; not both).  Each workgroup reduces
 * its 256 paths to (n, mean, M2) in a fixed order and the triples are merged in workgroup order by Chan's pairwise
 * formula: no atomics, two runs give identical bits, and both record forms give the same bits.  idx_dev (B x n_paths x
 * (T+1) x ndim bytes) and series_dev (B x nser x n_paths x T) are both NULL or both set (then with the default
 * lookahead).  A skipped member gets NaN statistics, moments and series and zero indices.  records == 1 on a shape whose
 * records do not fit LDS is SDFS_ERR_ARG.  The host waits only for the table uploads of the handle's previous call (an
 * event behind them), never for kernels. */
int sdfs_batch_sim_paths_dev(sdfs_batch* h, const double* records_dev, const sdfs_batch_sim_desc* desc, double* stats_dev,
                             double* moments_dev, uint8_t* idx_dev, double* series_dev);

/* Human-readable description of the batch plan. */
int sdfs_batch_describe(const sdfs_batch* h, char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SDFS_HIP_H */

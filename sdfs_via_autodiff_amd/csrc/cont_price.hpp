// cont_price.hpp -- asset prices of the continuous-state model at w* (sdfs_cont_set_tilt_dev, sdfs_cont_apply_tilted_dev,
// sdfs_cont_solve_tilted_dev, sdfs_cont_tilted_horizons_dev).
//
// Not a header of its own: sdfs_api.hip includes it once, after cont_sim.hpp, and it uses sdfs_handle, launch_kernel,
// Counter, check, fail, apply, cont_handle_ok and the pricing helpers stream_grid, tilted_solve, save_list_ok and
// horizon_loop of those files.
//
// The tilted expectation K(p, kappa_lambda, kappa_c) is the C_K0 / C_K1 / C_K2 form of cont_kernel (cont_kernel.hpp):
// the node loop of J.v on the tilted node weights, with the exponent p (theta - 1) on the interpolant of w and the
// per-point factor d2 that k_cont_tilt_d2 writes once per tilt.  run_cont (sdfs_api.hip) takes the tilt from the request
// (Apply::lc1 = the tilt's copy of w, Apply::lc2 = d2), so the BiCGSTAB of linear_solve serves (I - K) x = rhs unchanged.
// The horizon loop P_n = K P_{n-1} keeps per horizon the minimum and maximum of P_n / P_{n-1} over the grid and the
// number of points where P_n is no positive finite number (k_cont_horizon_reduce: per-workgroup partials, finished in a
// fixed order by one wave) and interpolates P_n at the query states with lin_interp_kernel.  No atomics anywhere: two runs
// give identical bits.
#pragma once

#include <hip/hip_runtime.h>

#include "cont_kernel.hpp"

extern "C++" {
namespace sdfs {

constexpr int CPRICE_BLOCK = 256;
constexpr int CPRICE_MAX_BLOCKS = 1024;
constexpr int CPRICE_NRED = 3;               // min, max of P_n / P_{n-1}; points where P_n is not positive and finite

// d2(x) = [beta^theta (w(x) - 1)^(1 - theta)]^p exp(kappa_c (mu_c + z) + kappa_c^2 sigma_c(x)^2 / 2 + kappa_lambda rho_lambda h_lambda),
// NaN where p > 0 and w(x) <= 1 (as C_EM)
__global__ void __launch_bounds__(CPRICE_BLOCK)
k_cont_tilt_d2(const ContDesc P, int power, double kappa_lam, double kappa_c, const double* __restrict__ w, double* __restrict__ d2) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const double pw = (double)power;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P.N; p += stride) {
    long long r = p;
    double x0 = 0.0, zval = 0.0, hcval = 0.0;
#pragma unroll
    for (int d = CMAXD - 1; d >= 0; --d) {
      if (d < P.D) {
        const int i = (int)(r % P.n[d]);
        r /= P.n[d];
        const double xd = P.grid[d][i];
        if (d == 0) x0 = xd;
        if (P.zdim == d) zval = xd;
        if (P.hcdim == d) hcval = xd;
      }
    }
    const double sig_c = P.phi_c * exp(hcval);
    const double lc = pw * P.theta * log(P.beta) + kappa_c * (P.mu_c + zval) + 0.5 * kappa_c * kappa_c * sig_c * sig_c +
                      kappa_lam * P.rho[0] * x0;
    double val = exp(lc);
    if (power > 0) {
      const double wx = w[p];
      val = wx > 1.0 ? val * pow(wx - 1.0, pw * (1.0 - P.theta)) : __builtin_nan("");
    }
    d2[p] = val;
  }
}

__global__ void __launch_bounds__(CPRICE_BLOCK) k_cont_fill(double* __restrict__ x, long long n, double v) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = v;
}

struct ContRed { double lo, hi, bad; };

__device__ __forceinline__ ContRed cont_red_wave(ContRed a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.lo = fmin(a.lo, __shfl_xor(a.lo, o));
    a.hi = fmax(a.hi, __shfl_xor(a.hi, o));
    a.bad += __shfl_xor(a.bad, o);           // (a count: exact in any order)
  }
  return a;
}

// one horizon: partials [block][CPRICE_NRED]
__global__ void __launch_bounds__(CPRICE_BLOCK)
k_cont_horizon_reduce(long long n, const double* __restrict__ cur, const double* __restrict__ prev, double* __restrict__ part) {
  __shared__ double s[CPRICE_BLOCK / 64][CPRICE_NRED];
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  ContRed a = {inf, -inf, 0.0};
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double c = cur[i], r = c / prev[i];
    if (!(c > 0.0 && c < inf)) a.bad += 1.0;
    a.lo = fmin(a.lo, r);                    // (a NaN ratio is skipped here and counted above, now or at its first horizon)
    a.hi = fmax(a.hi, r);
  }
  a = cont_red_wave(a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s[wave][0] = a.lo; s[wave][1] = a.hi; s[wave][2] = a.bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double lo = s[0][0], hi = s[0][1], bad = s[0][2];
#pragma unroll
    for (int k = 1; k < CPRICE_BLOCK / 64; ++k) { lo = fmin(lo, s[k][0]); hi = fmax(hi, s[k][1]); bad += s[k][2]; }
    double* o = part + (size_t)blockIdx.x * CPRICE_NRED;
    o[0] = lo; o[1] = hi; o[2] = bad;
  }
}

// one wave, partials in the order of their workgroups
__global__ void __launch_bounds__(64) k_cont_horizon_finish(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  ContRed a = {inf, -inf, 0.0};
  for (int b = threadIdx.x; b < nblocks; b += 64) {
    const double* q = part + (size_t)b * CPRICE_NRED;
    a.lo = fmin(a.lo, q[0]); a.hi = fmax(a.hi, q[1]); a.bad += q[2];
  }
  a = cont_red_wave(a);
  if (threadIdx.x == 0) { out[0] = a.lo; out[1] = a.hi; out[2] = a.bad; }
}

}  // namespace sdfs

namespace {
int cont_tilt_ok(sdfs_handle* h, const char* fn, bool need_tilt) {
  int rc = cont_handle_ok(h, fn);
  if (rc) return rc;
  if (need_tilt && h->ctilt.power < 0) return fail(h, SDFS_ERR_ARG, "%s before sdfs_cont_set_tilt_dev", fn);
  return 0;
}

// device buffers of one call, released however it ends
struct ContScratch {
  std::vector<void*> p;
  int alloc(sdfs_handle* h, double** out, size_t count) {
    HIPCHK(h, hipMalloc((void**)out, std::max<size_t>(count, 1) * sizeof(double)));
    p.push_back(*out);
    return 0;
  }
  ~ContScratch() { for (void* q : p) hipFree(q); }
};
}  // namespace
}  // extern "C++"

extern "C" {

int sdfs_cont_set_tilt_dev(sdfs_handle* h, const double* w, int sdf_power, double kappa_lam, double kappa_c) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_tilt_ok(h, "sdfs_cont_set_tilt_dev", false))) return rc;
  if (sdf_power < 0 || sdf_power > 2) return fail(h, SDFS_ERR_ARG, "sdf_power = %d: 0, 1 or 2", sdf_power);
  if (sdf_power > 0 && !w) return fail(h, SDFS_ERR_ARG, "sdf_power = %d needs the grid function w", sdf_power);
  if (!std::isfinite(kappa_lam) || !std::isfinite(kappa_c)) return fail(h, SDFS_ERR_ARG, "non-finite tilt exponent");
  auto& Ct = h->ctilt;
  const ContDesc& cd = h->cd;
  Ct.power = -1;                           // (until the tilt below is in place)
  if ((rc = ensure_buf(h, &Ct.w)) || (rc = ensure_buf(h, &Ct.d2))) return rc;
  if (!Ct.wq && (rc = dev_alloc(h, &Ct.wq, (size_t)cd.M))) return rc;
  // (a launch of the previous tilt may still read the weights; their staging copy may still be in flight)
  HIPCHK(h, hipStreamSynchronize(h->stream));
  Ct.wq_host.resize((size_t)cd.M);
  for (int m = 0; m < cd.M; ++m) Ct.wq_host[(size_t)m] = Ct.weight[(size_t)m] * std::exp(kappa_lam * cd.sconst[0] * Ct.eta0[(size_t)m]);
  HIPCHK(h, hipMemcpyAsync(Ct.wq, Ct.wq_host.data(), sizeof(double) * (size_t)cd.M, hipMemcpyHostToDevice, h->stream));
  if (w) HIPCHK(h, hipMemcpyAsync(Ct.w, w, sizeof(double) * (size_t)cd.N, hipMemcpyDeviceToDevice, h->stream));
  const double n8 = 8.0 * (double)cd.N;
  if ((rc = launch_kernel(h, k_cont_tilt_d2, dim3(stream_grid(h, cd.N, CPRICE_BLOCK)), dim3(CPRICE_BLOCK), 0,
                          Counter("cprice:d2", (sdf_power ? 2 : 1) * n8, 0), cd, sdf_power, kappa_lam, kappa_c,
                          sdf_power ? (const double*)Ct.w : nullptr, Ct.d2)))
    return rc;
  Ct.power = sdf_power;
  return 0;
}

int sdfs_cont_apply_tilted_dev(sdfs_handle* h, const double* f, double* out) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_tilt_ok(h, "sdfs_cont_apply_tilted_dev", true))) return rc;
  if (!f || !out) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  if (f == out) return fail(h, SDFS_ERR_ARG, "f and out: two distinct grids");
  Apply a(MODE_JVP, f, out, f);
  a.lc1 = h->ctilt.w; a.lc2 = h->ctilt.d2;
  return apply(h, a);
}

int sdfs_cont_solve_tilted_dev(sdfs_handle* h, const sdfs_opts* opts, const double* rhs, double* x, int64_t* n_iter,
                               double* final_rel_resid) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_tilt_ok(h, "sdfs_cont_solve_tilted_dev", true))) return rc;
  return tilted_solve(h, opts, rhs, x, n_iter, final_rel_resid, h->ctilt.w, h->ctilt.d2, "tilted continuous");
}

int sdfs_cont_tilted_horizons_dev(sdfs_handle* h, int64_t n_max, const double* states, int64_t nq, int64_t n_save,
                                  const int64_t* save_at, double* const* save_dev, double* price_host, double* bracket_host) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_tilt_ok(h, "sdfs_cont_tilted_horizons_dev", true))) return rc;
  if (n_max < 1 || n_max > (1LL << 24)) return fail(h, SDFS_ERR_ARG, "n_max = %lld: 1 ... 2^24 horizons", (long long)n_max);
  if (nq < 0 || nq > (1LL << 24) || (nq > 0 && (!states || !price_host)))
    return fail(h, SDFS_ERR_ARG, "nq = %lld query states: 0 ... 2^24, with states and price_host", (long long)nq);
  if (!bracket_host) return fail(h, SDFS_ERR_ARG, "NULL bracket_host");
  if ((rc = save_list_ok(h, n_max, n_save, save_at, save_dev))) return rc;
  const ContDesc& cd = h->cd;
  for (int64_t i = 0; i < nq * cd.D; ++i)
    if (!std::isfinite(states[i])) return fail(h, SDFS_ERR_ARG, "states[%lld] is not finite", (long long)i);
  auto& Ct = h->ctilt;
  if ((rc = ensure_buf(h, &Ct.pa)) || (rc = ensure_buf(h, &Ct.pb))) return rc;
  if (!Ct.part && (rc = dev_alloc(h, &Ct.part, (size_t)CPRICE_MAX_BLOCKS * CPRICE_NRED))) return rc;
  ContScratch scratch;
  double *res = nullptr, *xq = nullptr, *pq = nullptr;
  if ((rc = scratch.alloc(h, &res, (size_t)CPRICE_NRED * (size_t)n_max))) return rc;
  if (nq > 0) {
    if ((rc = scratch.alloc(h, &xq, (size_t)nq * cd.D)) || (rc = scratch.alloc(h, &pq, (size_t)nq * (size_t)n_max))) return rc;
    HIPCHK(h, hipMemcpyAsync(xq, states, sizeof(double) * (size_t)nq * cd.D, hipMemcpyHostToDevice, h->stream));
  }
  const long long N = cd.N;
  const int rgrid = std::min(stream_grid(h, N, CPRICE_BLOCK), CPRICE_MAX_BLOCKS);
  const dim3 qgrid((unsigned)((nq + 255) / 256));
  const int cid = h->profiling ? counter_id(h, "cprice:horizon_reduce", 16.0 * (double)N, 0) : -1;
  rc = horizon_loop(h, N, n_max, k_cont_fill, CPRICE_BLOCK, Ct.pa, Ct.pb, Ct.w, Ct.d2, n_save, save_at, save_dev,
                    [&](int64_t n, const double* cur, const double* prev) {
    {
      ProfScope ps(h, cid);
      hipLaunchKernelGGL(k_cont_horizon_reduce, dim3(rgrid), dim3(CPRICE_BLOCK), 0, h->stream, N, cur, prev, Ct.part);
    }
    hipLaunchKernelGGL(k_cont_horizon_finish, dim3(1), dim3(64), 0, h->stream, (const double*)Ct.part, rgrid,
                       res + CPRICE_NRED * (n - 1));
    if (nq > 0) {
      if (cd.D == 4) hipLaunchKernelGGL((lin_interp_kernel<4>), qgrid, dim3(256), 0, h->stream, cd, cur, (const double*)xq,
                                        (long long)nq, pq + (size_t)(n - 1) * (size_t)nq);
      else hipLaunchKernelGGL((lin_interp_kernel<6>), qgrid, dim3(256), 0, h->stream, cd, cur, (const double*)xq,
                              (long long)nq, pq + (size_t)(n - 1) * (size_t)nq);
    }
  });
  if (rc) return rc;
  std::vector<double> hres((size_t)CPRICE_NRED * n_max);
  HIPCHK(h, hipMemcpyAsync(hres.data(), res, sizeof(double) * hres.size(), hipMemcpyDeviceToHost, h->stream));
  if (nq > 0) HIPCHK(h, hipMemcpyAsync(price_host, pq, sizeof(double) * (size_t)nq * (size_t)n_max, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  long long first_bad = 0;
  for (int64_t n = 1; n <= n_max; ++n) {
    const double* r = hres.data() + CPRICE_NRED * (n - 1);
    bracket_host[2 * (n - 1) + 0] = r[0];
    bracket_host[2 * (n - 1) + 1] = r[1];
    if (r[2] != 0.0 && first_bad == 0) first_bad = n;
  }
  if (first_bad)
    return fail(h, SDFS_ERR_NUMERIC, "P_n is not a positive finite number at %.0f grid points at horizon %lld",
                hres[CPRICE_NRED * (first_bad - 1) + 2], first_bad);
  return 0;
}

}  // extern "C"

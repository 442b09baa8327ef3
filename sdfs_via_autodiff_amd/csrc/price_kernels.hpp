// price_kernels.hpp -- streaming kernels of the tilted expectation K (sdfs_set_tilt_dev, sdfs_tilted_horizons_dev).
//
// For a power p of the SDF and exponents (kappa_lam, kappa_c),
//
//   K f = d2 .* H'(d1 .* f),   d1 = c1^p .* e_lam[h_lam'],   d2 = c2^p .* e_c[h_c] .* e_z[.]
//
// with H' the library's expectation (a1 folded into the next-state columns, a2 and a3 into the current-state rows) and
// c1 = w^(theta-1), c2 = beta^theta (Tw - 1)^(1-theta) the linearisation cached at w.  So K runs on the J.v kernels of
// every plan with (d1, d2) in place of (c1, c2).  (Where the aggregator applies a3 as a table, the cached c2 holds
// c2 a3 and H' lacks a3; the host then builds e_z with exponent kappa_c - p (1-gamma), see sdfs_set_tilt_dev.)
// k_tilt_scalings forms d1 and d2 in one pass; k_horizon_reduce reduces one horizon of the term structure P_n = K P_{n-1} to per-workgroup partials that k_horizon_finish sums in a fixed
// order (no atomics: two runs are bit-identical).
//
// The short tables (e_lam along h_lambda, e_c along h_c, the product-form weights) travel by value in the kernel
// arguments and are staged in LDS, where the per-lane lookups do not serialise; e_z is as large as the a3 table and is
// read from global memory with the a3 strides.  Grid coordinates come from multiply-high divisions (N <= 32^6 < 2^31).
// fp64 throughout.
#pragma once

#include <hip/hip_runtime.h>

#include "sens_kernels.hpp"
#include "wave_reduce.hpp"

constexpr int PRICE_BLOCK = 256;
constexpr int PRICE_MAX_BLOCKS = 2048;       // workgroups of k_horizon_reduce (partials per horizon)
constexpr int PRICE_NSUM = 5;                // <g, P>, <g, -log P>, min P/P_prev, max P/P_prev, count of bad points

// n / d for n < 2^31 (the multiply-high form: m = floor(2^32 (2^s - d) / d) + 1, s = ceil(log2 d))
struct PriceDiv { unsigned d, m, s; };
inline PriceDiv price_div(unsigned d) {
  unsigned s = 0;
  while ((1u << s) < d) ++s;
  return PriceDiv{d, (unsigned)(((1ULL << 32) * ((1ULL << s) - d)) / d + 1), s};
}
__device__ __forceinline__ unsigned price_q(const PriceDiv& f, unsigned n) { return (__umulhi(n, f.m) + n) >> f.s; }

struct PriceGeom {
  long long n;                               // grid points
  int ndim;
  PriceDiv ext[SENS_MAXD];                   // extents, C order (last axis fastest)
  int a3s[SENS_MAXD];                        // stride of each axis in the e_z table (0: it does not depend on the axis)
  int ax_lam, ax_c;                          // axes e_lam (next state) and e_c (current state) are indexed by
};

struct PriceWeights { double t[SENS_MAXD][SENS_MAXN]; };   // per-axis weights; g(x) = prod_a t[a][x_a]

// d1 = c1^P e_lam[h_lam], d2 = c2^P e_c[h_c] e_z[.]  (ez == nullptr: e_z = 1).  P is 0, 1 or 2: c^2 is one multiply and
// P = 0 reads neither c1 nor c2.  With every exponent zero the tables are exactly 1 and (d1, d2) = (c1, c2) bit for bit.
template <int P>
__global__ void __launch_bounds__(PRICE_BLOCK)
k_tilt_scalings(PriceGeom g, SensTab el, SensTab ec, const double* __restrict__ ez, const double* __restrict__ c1,
                const double* __restrict__ c2, double* __restrict__ d1, double* __restrict__ d2) {
  __shared__ double tl[SENS_MAXN], tc[SENS_MAXN];
  if (threadIdx.x < SENS_MAXN) { tl[threadIdx.x] = el.t[threadIdx.x]; tc[threadIdx.x] = ec.t[threadIdx.x]; }
  __syncthreads();
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
    unsigned r = (unsigned)i, off = 0, il = 0, ic = 0;
    for (int a = g.ndim - 1; a >= 0; --a) {
      const unsigned q = price_q(g.ext[a], r);
      const unsigned c = r - q * g.ext[a].d;
      off += c * (unsigned)g.a3s[a];
      if (a == g.ax_lam) il = c;
      if (a == g.ax_c) ic = c;
      r = q;
    }
    double s1 = tl[il], s2 = tc[ic];
    if (ez) s2 *= ez[off];
    if (P >= 1) {
      const double x1 = __builtin_nontemporal_load(c1 + i), x2 = __builtin_nontemporal_load(c2 + i);
      s1 *= (P == 2) ? x1 * x1 : x1;
      s2 *= (P == 2) ? x2 * x2 : x2;
    }
    __builtin_nontemporal_store(s1, d1 + i);
    __builtin_nontemporal_store(s2, d2 + i);
  }
}

// x = v everywhere (P_0 = 1)
__global__ void __launch_bounds__(PRICE_BLOCK)
k_price_fill(double* __restrict__ x, long long n, double v) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = v;
}

// One horizon: per-workgroup partials of <g, P_n>, <g, -log P_n>, min and max of P_n / P_{n-1} over the points where
// both are positive, and the number of points where P_n or P_{n-1} is not positive (or NaN).  part[blockIdx.x * 5 + k].
// Every lane reaches the wave reductions (wave_reduce.hpp needs all 64 active).
__global__ void __launch_bounds__(PRICE_BLOCK)
k_horizon_reduce(PriceGeom g, PriceWeights wt, const double* __restrict__ pn, const double* __restrict__ pp,
                 double* __restrict__ part) {
  __shared__ double tw[SENS_MAXD][SENS_MAXN];
  __shared__ double red[PRICE_BLOCK / 64][PRICE_NSUM];
  for (int k = threadIdx.x; k < SENS_MAXD * SENS_MAXN; k += blockDim.x) tw[k / SENS_MAXN][k % SENS_MAXN] = wt.t[k / SENS_MAXN][k % SENS_MAXN];
  __syncthreads();
  double sp = 0.0, sy = 0.0, rmin = INFINITY, rmax = -INFINITY, bad = 0.0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
    const double p = __builtin_nontemporal_load(pn + i), q = __builtin_nontemporal_load(pp + i);
    unsigned r = (unsigned)i;
    double gw = 1.0;
    for (int a = g.ndim - 1; a >= 0; --a) {
      const unsigned qq = price_q(g.ext[a], r);
      gw *= tw[a][r - qq * g.ext[a].d];
      r = qq;
    }
    if (p > 0.0 && q > 0.0) {
      sp = fma(gw, p, sp);
      sy = fma(gw, -log(p), sy);
      const double ratio = p / q;
      rmin = fmin(rmin, ratio);
      rmax = fmax(rmax, ratio);
    } else {
      bad += 1.0;
    }
  }
  sp = sdfs::wave_sum_f64(sp);
  sy = sdfs::wave_sum_f64(sy);
  rmin = -sdfs::wave_max_f64(-rmin);
  rmax = sdfs::wave_max_f64(rmax);
  bad = sdfs::wave_sum_f64(bad);
  const int wv = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) { red[wv][0] = sp; red[wv][1] = sy; red[wv][2] = rmin; red[wv][3] = rmax; red[wv][4] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double o[PRICE_NSUM] = {red[0][0], red[0][1], red[0][2], red[0][3], red[0][4]};
    for (int w = 1; w < PRICE_BLOCK / 64; ++w) {
      o[0] += red[w][0]; o[1] += red[w][1]; o[2] = fmin(o[2], red[w][2]); o[3] = fmax(o[3], red[w][3]); o[4] += red[w][4];
    }
    for (int k = 0; k < PRICE_NSUM; ++k) part[(long long)blockIdx.x * PRICE_NSUM + k] = o[k];
  }
}

// The partials of `nblocks` workgroups -> res[0..4], in a fixed order: lane l takes workgroups l, l + 64, ... in turn,
// then the wave reduction (one wave).
__global__ void __launch_bounds__(64)
k_horizon_finish(const double* __restrict__ part, int nblocks, double* __restrict__ res) {
  double sp = 0.0, sy = 0.0, rmin = INFINITY, rmax = -INFINITY, bad = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) {
    const double* q = part + (long long)b * PRICE_NSUM;
    sp += q[0]; sy += q[1]; rmin = fmin(rmin, q[2]); rmax = fmax(rmax, q[3]); bad += q[4];
  }
  sp = sdfs::wave_sum_f64(sp);
  sy = sdfs::wave_sum_f64(sy);
  rmin = -sdfs::wave_max_f64(-rmin);
  rmax = sdfs::wave_max_f64(rmax);
  bad = sdfs::wave_sum_f64(bad);
  if (threadIdx.x == 0) { res[0] = sp; res[1] = sy; res[2] = rmin; res[3] = rmax; res[4] = bad; }
}

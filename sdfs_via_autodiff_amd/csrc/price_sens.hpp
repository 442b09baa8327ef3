// price_sens.hpp -- streaming kernels of the tangent of the tilted expectation K (sdfs_tilt_tangent_dev).
//
// With K f = R .* H0(a1' .* w^(p(theta-1)) .* f),  a1' = exp(kappa_lam h_lam') on the next state and
// R = [beta^theta (Tw - 1)^(1-theta)]^p exp(kappa_c^2 sigma_c^2 / 2 + kappa_c (mu_c + z)) on the current one, a direction
// that moves the parameters, the exponents, w, Tw, f and the transition matrices (dQ_k = G_k Q_k) moves K f by
//
//   d(K f) = u2 .* K f + K (u1 .* f + df) + sum_k R .* (G_k along axis k on (K f / R))
//
//   u1 = p (dtheta ln w + (theta-1) dw / w) + [dkappa_lam h_lam + kappa_lam dh_lam]                       (next state)
//   u2 = p (theta dbeta / beta + dtheta ln beta - dtheta ln(Tw - 1) + (1-theta) dTw / (Tw - 1))
//        + [kappa_c dkappa_c sigma_c^2 + kappa_c^2 sigma_c dsigma_c] + [dkappa_c (mu_c + z) + kappa_c (dmu_c + dz)]
//
// The prologue forms v = u1 .* f + df, one tilted product gives K v, the epilogue adds u2 .* K f, and each axis with a
// generator adds one three-point stencil pass.  The bracketed terms are tables the host builds: the two short ones
// (along h_lambda and h_c) travel by value and are staged in LDS, the last is as large as the a3 table and is read from
// global memory with the a3 strides.  P is the power of the SDF (0, 1 or 2); P = 0 reads none of w, dw, Tw, dTw.  LOG is
// set when dtheta != 0: only then is a logarithm taken.  Streamed data moves with non-temporal loads and stores, one
// thread per point, grid-stride; no atomics, so two runs are bit-identical.  fp64 throughout.
#pragma once

#include <hip/hip_runtime.h>

#include "price_kernels.hpp"

// coordinates of point i: the a3 offset, and the coordinates on the three axes asked for (an axis of -1 is never met)
__device__ __forceinline__ void price_coords(const PriceGeom& g, unsigned i, int ax0, int ax1, unsigned& off, unsigned& c0,
                                             unsigned& c1) {
  unsigned r = i;
  off = 0; c0 = 0; c1 = 0;
  for (int a = g.ndim - 1; a >= 0; --a) {
    const unsigned q = price_q(g.ext[a], r);
    const unsigned c = r - q * g.ext[a].d;
    off += c * (unsigned)g.a3s[a];
    if (a == ax0) c0 = c;
    if (a == ax1) c1 = c;
    r = q;
  }
}

// v = u1 .* f + df,  u1 = ul[h_lam] + pthm1 dw / w + pdth ln w   (pthm1 = p (theta-1), pdth = p dtheta)
// f == nullptr: f = 1; df == nullptr: df = 0.
template <int P, bool LOG>
__global__ void __launch_bounds__(PRICE_BLOCK)
k_tilt_tangent_prologue(PriceGeom g, SensTab ul, double pthm1, double pdth, const double* __restrict__ w,
                        const double* __restrict__ dw, const double* __restrict__ f, const double* __restrict__ df,
                        double* __restrict__ v) {
  __shared__ double tl[SENS_MAXN];
  if (threadIdx.x < SENS_MAXN) tl[threadIdx.x] = ul.t[threadIdx.x];
  __syncthreads();
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
    unsigned off, il, unused;
    price_coords(g, (unsigned)i, g.ax_lam, -1, off, il, unused);
    double u = tl[il];
    if (P >= 1) {
      const double wi = __builtin_nontemporal_load(w + i);
      u = fma(pthm1, __builtin_nontemporal_load(dw + i) / wi, u);
      if (LOG) u = fma(pdth, log(wi), u);
    }
    double o = f ? u * __builtin_nontemporal_load(f + i) : u;
    if (df) o += __builtin_nontemporal_load(df + i);
    __builtin_nontemporal_store(o, v + i);
  }
}

// out = u2 .* kf + kv,  u2 = c0 + uc[h_c] + tz[.] + p1mth dTw / (Tw - 1) - pdth ln(Tw - 1)
// (c0 = p (theta dbeta / beta + dtheta ln beta), p1mth = p (1-theta); tz == nullptr: a zero table; kv may be out)
template <int P, bool LOG>
__global__ void __launch_bounds__(PRICE_BLOCK)
k_tilt_tangent_epilogue(PriceGeom g, SensTab uc, double c0, double p1mth, double pdth, const double* __restrict__ tz,
                        const double* __restrict__ Tw, const double* __restrict__ dTw, const double* __restrict__ kf,
                        const double* kv, double* out) {
  __shared__ double tc[SENS_MAXN];
  if (threadIdx.x < SENS_MAXN) tc[threadIdx.x] = uc.t[threadIdx.x];
  __syncthreads();
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
    unsigned off, ic, unused;
    price_coords(g, (unsigned)i, g.ax_c, -1, off, ic, unused);
    double u = c0 + tc[ic];
    if (tz) u += tz[off];
    if (P >= 1) {
      const double e = __builtin_nontemporal_load(Tw + i) - 1.0;
      u = fma(p1mth, __builtin_nontemporal_load(dTw + i) / e, u);
      if (LOG) u = fma(-pdth, log(e), u);
    }
    const double o = fma(u, __builtin_nontemporal_load(kf + i), __builtin_nontemporal_load(kv + i));
    __builtin_nontemporal_store(o, out + i);
  }
}

// Generator term of one axis: out += sum_j G[c, j] kf_j R_c / R_j over the three neighbours along `axis`.  The rows of a
// Rouwenhorst generator sum to zero and neighbouring values differ by per cent, so the differences are formed first:
//
//   out += (diag + sub + sup) kf_c + sub (kf_{c-1} rho- - kf_c) + sup (kf_{c+1} rho+ - kf_c),
//   kf_j rho - kf_c = (kf_j - kf_c) + kf_j expm1(l_c - l_j),
//   l_c - l_j = -p1mth log1p((Tw_j - Tw_c) / (Tw_c - 1)) + (qc[c] - qc[j], if the axis is h_c) + kc (zt_c - zt_j)
//
// with qc = kappa_c^2 sigma_c^2 / 2 by value and zt = mu_c + z a device table read with the a3 strides (nullptr when
// kappa_c = 0).  R is the mathematical row factor, not the d2 buffer; P = 0 takes no logarithm.  The caller zeroes sub[0]
// and sup[n - 1], so no neighbour outside the axis is read.  inner: the stride of `axis` in the grid.  out is distinct
// from kf and Tw.
template <int P>
__global__ void __launch_bounds__(PRICE_BLOCK)
k_tilt_tangent_generator(PriceGeom g, SensGen G, SensTab qc, int axis, unsigned inner, double p1mth, double kc,
                         const double* __restrict__ Tw, const double* __restrict__ zt, const double* __restrict__ kf,
                         double* __restrict__ out) {
  __shared__ double sb[SENS_MAXN], dg[SENS_MAXN], sp[SENS_MAXN], tq[SENS_MAXN];
  if (threadIdx.x < SENS_MAXN) {
    sb[threadIdx.x] = G.sub[threadIdx.x]; dg[threadIdx.x] = G.diag[threadIdx.x]; sp[threadIdx.x] = G.sup[threadIdx.x];
    tq[threadIdx.x] = qc.t[threadIdx.x];
  }
  __syncthreads();
  const unsigned n_ax = g.ext[axis].d;
  const unsigned s3 = (unsigned)g.a3s[axis];
  const bool on_c = axis == g.ax_c;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
    unsigned off, c, unused;
    price_coords(g, (unsigned)i, axis, -1, off, c, unused);
    const double lo = sb[c], up = sp[c];
    const double kc0 = __builtin_nontemporal_load(kf + i);
    double t0 = 0.0, inv_e = 0.0, z0 = 0.0;
    if (P >= 1) { t0 = Tw[i]; inv_e = 1.0 / (t0 - 1.0); }
    if (zt) z0 = zt[off];
    double acc = (dg[c] + lo + up) * kc0;
    if (c > 0 && lo != 0.0) {
      double d = 0.0;
      if (P >= 1) d = -p1mth * log1p((Tw[i - inner] - t0) * inv_e);
      if (zt) d = fma(kc, z0 - zt[off - s3], d);
      if (on_c) d += tq[c] - tq[c - 1];
      const double kj = kf[i - inner];
      acc = fma(lo, fma(kj, expm1(d), kj - kc0), acc);
    }
    if (c + 1 < n_ax && up != 0.0) {
      double d = 0.0;
      if (P >= 1) d = -p1mth * log1p((Tw[i + inner] - t0) * inv_e);
      if (zt) d = fma(kc, z0 - zt[off + s3], d);
      if (on_c) d += tq[c] - tq[c + 1];
      const double kj = kf[i + inner];
      acc = fma(up, fma(kj, expm1(d), kj - kc0), acc);
    }
    __builtin_nontemporal_store(__builtin_nontemporal_load(out + i) + acc, out + i);
  }
}

// sens_kernels.hpp -- elementwise kernels of the parameter tangent of T (sdfs_param_tangent_dev).
//
// With Y = K H0(a1 w^theta), K = a2 a3 and T w = 1 + beta Y^(1/theta), a direction (dbeta, dtheta, dln a1, dln a2,
// dln a3) that leaves every transition matrix fixed moves T(w), at a fixed w, by
//
//   dT = (Tw - 1) (dbeta / beta - (dtheta / theta) ln((Tw - 1) / beta) + (dln a2 + dln a3) / theta)
//        + (1 / theta) J(w) [w .* (dtheta ln w + dln a1)]
//
// (J(w) = the library's J.v at w).  The prologue forms the J.v direction, the epilogue the rest; each is one
// streaming pass over the grid.  The two short tables (dln a1 along h_lambda, dln a2 along h_c; extents <= MAXN)
// travel by value in the kernel arguments, i.e. in the constant segment every wave reads through the scalar cache;
// dln a3 is as large as the a3 table (up to N / (n_h_c n_h_lambda) points) and is read from global memory with the
// strides the pass kernels use for a3.  A direction that moves a transition matrix through a tridiagonal left
// generator (a persistence parameter) adds one more streaming pass per such axis, k_sens_generator.  fp64 throughout.
#pragma once

#include <hip/hip_runtime.h>

constexpr int SENS_BLOCK = 256;
constexpr int SENS_MAXD = 6;
constexpr int SENS_MAXN = 32;          // = MAXN (pass_kernel.hpp): the longest axis a handle has

struct SensGeom {
  long long n;                         // grid points
  int ndim;
  int ext[SENS_MAXD];                  // extents, C order (last axis fastest)
  int a3s[SENS_MAXD];                  // stride of each axis in the dln a3 table (0: the table does not depend on it)
  int ax_tab;                          // axis the short table is indexed by (prologue: h_lambda, epilogue: h_c)
};

struct SensTab { double t[SENS_MAXN]; };

// coordinate of flat index i on axis `a` (unsigned 32-bit arithmetic: N <= 32^6 = 2^30)
__device__ inline unsigned sens_coord(const SensGeom& g, unsigned i, int a) {
  unsigned inner = 1;
  for (int b = g.ndim - 1; b > a; --b) inner *= (unsigned)g.ext[b];
  return (i / inner) % (unsigned)g.ext[a];
}

// v = w .* (dtheta ln w + dln a1[h_lambda])
__global__ void __launch_bounds__(SENS_BLOCK)
k_sens_prologue(SensGeom g, SensTab dla1, double dtheta, const double* __restrict__ w, double* __restrict__ v) {
  unsigned inner = 1;
  for (int b = g.ndim - 1; b > g.ax_tab; --b) inner *= (unsigned)g.ext[b];
  const unsigned n_tab = (unsigned)g.ext[g.ax_tab];
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
    const double wi = w[i];
    const double u = dla1.t[((unsigned)i / inner) % n_tab];
    v[i] = wi * (dtheta != 0.0 ? fma(dtheta, log(wi), u) : u);
  }
}

// out = (Tw - 1) (c0 - dth_th ln((Tw - 1) / beta) + (dln a2[h_c] + dln a3[.]) / theta) + jv / theta
// (jv == nullptr: no J.v term; dla3 == nullptr: a zero dln a3; jv may alias out)
__global__ void __launch_bounds__(SENS_BLOCK)
k_sens_epilogue(SensGeom g, SensTab dla2, double c0, double dth_th, double inv_beta, double inv_theta,
                const double* __restrict__ Tw, const double* jv, const double* __restrict__ dla3, double* out) {
  unsigned inner = 1;
  for (int b = g.ndim - 1; b > g.ax_tab; --b) inner *= (unsigned)g.ext[b];
  const unsigned n_tab = (unsigned)g.ext[g.ax_tab];
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
    const double e = Tw[i] - 1.0;
    double s = dla2.t[((unsigned)i / inner) % n_tab];
    if (dla3) {
      unsigned r = (unsigned)i, off = 0;
      for (int a = g.ndim - 1; a >= 0; --a) {
        const unsigned ex = (unsigned)g.ext[a];
        const unsigned q = r / ex;
        off += (r - q * ex) * (unsigned)g.a3s[a];
        r = q;
      }
      s += dla3[off];
    }
    double f = fma(s, inv_theta, c0);
    if (dth_th != 0.0) f -= dth_th * log(e * inv_beta);
    double o = e * f;
    if (jv) o = fma(jv[i], inv_theta, o);
    out[i] = o;
  }
}

// Generator term of a persistence tangent.  With every transition matrix unconditional, E = H0(a1 w^theta) =
// ((Tw - 1) / beta)^theta / (a2 a3), and a direction that moves the matrix of one axis by dQ = G Q (G tridiagonal: the
// Rouwenhorst matrix has d Theta / d rho = G Theta) moves E by G applied along that axis, hence T by
//
//   (Tw - 1) / theta . r,   r = sum_j G[c, j] E(c -> j) / E = diag + sub + super + sub expm1(l(c-1) - l(c)) + super expm1(l(c+1) - l(c))
//
// with l = ln E.  The rows of a Rouwenhorst generator sum to zero and neighbouring E differ by per cent, so the
// differences are formed before any exponential:  l(j) - l(c) = theta log1p((Tw_j - Tw_c) / (Tw_c - 1)) - (ln a2_j -
// ln a2_c) - (ln a3_j - ln a3_c).  The caller zeroes sub[0] and super[n - 1], so no neighbour outside the axis is read.
// One pass per axis with a generator; ln a2 by value, ln a3 a device table read with the a3 strides.
struct SensGen { double sub[SENS_MAXN], diag[SENS_MAXN], sup[SENS_MAXN]; };

// out += (Tw - 1) / theta . r   (g.ax_tab: the axis ln a2 is indexed by; out distinct from Tw)
__global__ void __launch_bounds__(SENS_BLOCK)
k_sens_generator(SensGeom g, SensGen G, SensTab la2, int axis, double theta, double inv_theta,
                 const double* __restrict__ Tw, const double* __restrict__ la3, double* __restrict__ out) {
  unsigned inner = 1;
  for (int b = g.ndim - 1; b > axis; --b) inner *= (unsigned)g.ext[b];
  const unsigned n_ax = (unsigned)g.ext[axis];
  const int s3 = g.a3s[axis];
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
    unsigned r = (unsigned)i, off = 0, c = 0, k2 = 0;
    for (int a = g.ndim - 1; a >= 0; --a) {
      const unsigned ex = (unsigned)g.ext[a];
      const unsigned q = r / ex;
      const unsigned x = r - q * ex;
      off += x * (unsigned)g.a3s[a];
      if (a == axis) c = x;
      if (a == g.ax_tab) k2 = x;
      r = q;
    }
    const double sb = G.sub[c], sp = G.sup[c];
    const double e = Tw[i] - 1.0;
    const double inv_e = 1.0 / e;
    const double l2 = la2.t[k2], l3 = la3[off];
    double acc = G.diag[c] + sb + sp;
    if (c > 0 && sb != 0.0) {
      double d = theta * log1p((Tw[i - inner] - Tw[i]) * inv_e) - (la3[off - s3] - l3);
      if (axis == g.ax_tab) d -= la2.t[c - 1] - l2;
      acc = fma(sb, expm1(d), acc);
    }
    if (c + 1 < n_ax && sp != 0.0) {
      double d = theta * log1p((Tw[i + inner] - Tw[i]) * inv_e) - (la3[off + s3] - l3);
      if (axis == g.ax_tab) d -= la2.t[c + 1] - l2;
      acc = fma(sp, expm1(d), acc);
    }
    out[i] = fma(e * inv_theta, acc, out[i]);
  }
}

// x = -b (the right-hand side of the BiCGSTAB loop, which solves (J - I) x = b)
__global__ void __launch_bounds__(SENS_BLOCK)
k_sens_neg(const double* __restrict__ b, double* __restrict__ x, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = -b[i];
}

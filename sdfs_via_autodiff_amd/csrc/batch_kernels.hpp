// batch_kernels.hpp -- successive approximation for a batch of parameter vectors: one workgroup per problem.
//
// A grid of up to 16 384 points fits the LDS of one CU with its iterate in the registers of 512 threads, so one
// workgroup runs a whole solve of one problem -- every application of T, the residual and the stopping test -- with no launch, no global round trip and no other
// workgroup inside its loop; the grid of the launch is the batch.  Per problem and launch:
//   * the iterate w stays in registers, K points per thread (point p = tid + k NT), with the a3 index of each point
//     (16 bits each); 256 threads (one wave per SIMD, 512 VGPRs) up to 2048 points, 512 threads (two waves per SIMD,
//     256 VGPRs) and up to 32 points per thread beyond.  (kernel-resource-usage: 32 points per thread use all 256
//     VGPRs with no scratch, 36 and 40 spill; 1024 threads leave 128 VGPRs, which spill from 6 points per thread on);
//   * the work buffer of N doubles is dynamic LDS; behind it the problem's folded matrices (rows zero-padded to the
//     unroll class of the extent: 4 / 8 / 12 / 16 / 24 / 32), its a3 table and one double per wave for the maximum;
//   * one iteration: x = w^theta into LDS | barrier | per axis: every thread takes whole lines, reads a line into
//     registers, writes M x back in place | barrier | Tw = 1 + beta (a3 S)^(1/theta), |Tw - w| per point, wave maximum
//     (wave_reduce.hpp), one LDS step, the stopping test -- uniform over the workgroup;
//   * at most `chunk` iterations, then w, the count, the last error and the status word go to global memory with plain
//     stores.  A problem whose status is no longer BATCH_OPEN returns at once.
// The contractions are fp64 FMAs in a fixed order and the powers are the library's powy (pass_kernel.hpp), so a problem's
// bits depend on its own inputs only: not on the batch, the workgroup's place or the chunk length.
#pragma once
#include <hip/hip_runtime.h>

#include "pass_kernel.hpp"
#include "wave_reduce.hpp"

namespace sdfs {

constexpr int BATCH_MAXD = 6;
constexpr int BATCH_LDS_MAX = 160 * 1024;        // LDS of one CU (gfx950)
constexpr int BATCH_RED = 16;                    // doubles behind the tables: one maximum per wave
enum { BATCH_CONVERGED = 0, BATCH_MAX_ITER = 1, BATCH_NONFINITE = 2, BATCH_OPEN = 3 };

// row length of an n x n matrix in the kernel's tables: the unroll class of the line contraction
__host__ __device__ inline int batch_row_class(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 12 ? 12 : n <= 16 ? 16 : n <= 24 ? 24 : 32; }

struct BatchDesc {
  int ndim, N;
  int nwork;                   // N rounded up to even: the tables start 16-byte aligned
  int n[BATCH_MAXD];           // extents
  int stride[BATCH_MAXD];      // element strides (C order)
  int np[BATCH_MAXD];          // batch_row_class(n)
  int qoff[BATCH_MAXD];        // offset of the axis's n x np matrix in a problem's table block
  int a3s[BATCH_MAXD];         // stride of the axis in the a3 table (0: a3 does not depend on it)
  int a3off;                   // offset of the a3 table in the block
  int tabwords;                // doubles per table block (even)
};

struct BatchArgs {
  const double* tab;           // [B][tabwords]
  const double* scal;          // [B][4]: beta, theta, 1 / theta
  const double* w_in;          // [B][N]
  double* w_out;               // [B][N]
  double* resid;               // apply: [B] max|Tw - w|
  int* status;                 // solve: [B]
  long long* it;               // solve: [B] iterations so far
  double* err;                 // solve: [B] last max|Tw - w|
  double tol;
  long long max_iter;
  int chunk;                   // most iterations of this launch
  int apply;                   // 1: one application, w_in -> w_out, no state
};

// all lines of one axis, in place: a thread owns whole lines
template <int NP>
__device__ __forceinline__ void batch_lines(double* wk, const double* q, int n, int s, int nlines, int tid, int nt) {
  for (int L = tid; L < nlines; L += nt) {
    const int o = (int)((unsigned)L / (unsigned)s), i = L - o * s;
    double* const p = wk + o * n * s + i;
    double x[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) x[j] = j < n ? p[j * s] : 0.0;
#pragma unroll 2
    for (int r = 0; r < n; ++r) {
      const double* const qr = q + r * NP;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < NP; ++j) acc = fma(qr[j], x[j], acc);
      p[r * s] = acc;
    }
  }
}

// K points per thread, NT threads (the second launch bound: waves per SIMD, i.e. the whole register file for the workgroup)
template <int K, int NT>
__global__ __launch_bounds__(NT, NT / 256) void batch_sa_kernel(const BatchDesc* __restrict__ Dp, const BatchArgs A) {
  const BatchDesc& D = *Dp;     // in device memory: the axis loop indexes its tables at run time
  extern __shared__ __attribute__((aligned(16))) double batch_lds[];
  // points per call of the power routine (their chains overlap; two where the iterate fills the registers)
  constexpr int PG = K < 4 ? K : (K >= 32 ? 2 : 4);
  static_assert(K % PG == 0, "whole groups");
  constexpr int NW = NT / 64;
  static_assert(NW <= BATCH_RED, "one maximum per wave");
  const int b = blockIdx.x;
  if (!A.apply && A.status[b] != BATCH_OPEN) return;              // uniform: this problem has finished
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = D.N;
  double* const wk = batch_lds;
  double* const tb = batch_lds + D.nwork;
  double* const red = tb + D.tabwords;
  {
    const double* const src = A.tab + (size_t)b * D.tabwords;
    for (int i = tid; i < D.tabwords; i += NT) tb[i] = src[i];
  }
  const double beta = A.scal[4 * b], theta = A.scal[4 * b + 1], inv_theta = A.scal[4 * b + 2];
  PowK<true> P1;
  PowK<false> P2;
  P1.init(theta, lane);
  P2.init(inv_theta, lane);
  // this thread's points: the iterate and the a3 index
  double w[K];
  unsigned ia3[(K + 1) / 2];                     // two 16-bit indices per register (the table has fewer than N entries)
#pragma unroll
  for (int k = 0; k < (K + 1) / 2; ++k) ia3[k] = 0u;
  const double* const win = A.w_in + (size_t)b * N;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int p = tid + k * NT;
    const bool ok = p < N;
    w[k] = ok ? win[ok ? p : 0] : 1.0;
    int ia = 0;
#pragma unroll
    for (int a = 0; a < BATCH_MAXD; ++a)
      if (a < D.ndim && D.a3s[a] != 0) ia += (int)(((unsigned)p / (unsigned)D.stride[a]) % (unsigned)D.n[a]) * D.a3s[a];
    ia3[k >> 1] |= (ok ? (unsigned)ia : 0u) << (16 * (k & 1));
  }
  const double* const a3 = tb + D.a3off;
  long long it = A.apply ? 0 : A.it[b];
  double err = 0.0;
  int status = BATCH_OPEN;
  __syncthreads();
  for (int c = 0; c < A.chunk; ++c) {
    // ---- x = w^theta (points beyond the grid feed the power 1; a wave with no point in a group skips it) -------------
#pragma unroll
    for (int k0 = 0; k0 < K; k0 += PG) {
      if (k0 * NT + wave * 64 < N) {
        double xin[PG], xw[PG];
#pragma unroll
        for (int j = 0; j < PG; ++j) xin[j] = w[k0 + j];
        P1.run<PG>(xin, xw);
#pragma unroll
        for (int j = 0; j < PG; ++j) if (tid + (k0 + j) * NT < N) wk[tid + (k0 + j) * NT] = xw[j];
      }
    }
    __syncthreads();
    // ---- the contractions, axis by axis, in place -----------------------------------------------------------------------
    for (int a = 0; a < D.ndim; ++a) {
      const int n = D.n[a], s = D.stride[a], nl = N / n;
      const double* const q = tb + D.qoff[a];
      switch (D.np[a]) {
        case 4: batch_lines<4>(wk, q, n, s, nl, tid, NT); break;
        case 8: batch_lines<8>(wk, q, n, s, nl, tid, NT); break;
        case 12: batch_lines<12>(wk, q, n, s, nl, tid, NT); break;
        case 16: batch_lines<16>(wk, q, n, s, nl, tid, NT); break;
        case 24: batch_lines<24>(wk, q, n, s, nl, tid, NT); break;
        default: batch_lines<32>(wk, q, n, s, nl, tid, NT); break;
      }
      __syncthreads();
    }
    // ---- Tw = 1 + beta (a3 S)^(1/theta), the step --------------------------------------------------------------------------
    double rmax = 0.0;
#pragma unroll
    for (int k0 = 0; k0 < K; k0 += PG) {
      if (k0 * NT + wave * 64 < N) {
        double ks[PG], uu[PG];
#pragma unroll
        for (int j = 0; j < PG; ++j) {
          const int p = tid + (k0 + j) * NT;
          ks[j] = p < N ? a3[(ia3[(k0 + j) >> 1] >> (16 * ((k0 + j) & 1))) & 0xffffu] * wk[p] : 1.0;
        }
        P2.run<PG>(ks, uu);
#pragma unroll
        for (int j = 0; j < PG; ++j) {
          const double y = 1.0 + beta * uu[j];
          if (tid + (k0 + j) * NT < N) {
            double r0 = fabs(y - w[k0 + j]);
            r0 = r0 < __builtin_huge_val() ? r0 : __builtin_huge_val();     // NaN and Inf: the iterate left the finite range
            rmax = fmax(rmax, r0);
            w[k0 + j] = y;
          }
        }
      }
    }
    rmax = wave_max_f64(rmax);
    if (lane == 0) red[wave] = rmax;
    __syncthreads();
    double m = red[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) m = fmax(m, red[i]);
    err = readlane_f64(m, 0);
    ++it;
    // code/solvers.py:19-48: loop while error > tol and it < max_iter
    if (!(err < __builtin_huge_val())) status = BATCH_NONFINITE;
    else if (!(err > A.tol)) status = BATCH_CONVERGED;
    else if (it >= A.max_iter) status = BATCH_MAX_ITER;
    if (status != BATCH_OPEN) break;             // uniform
  }
  double* const wout = A.w_out + (size_t)b * N;
#pragma unroll
  for (int k = 0; k < K; ++k) if (tid + k * NT < N) wout[tid + k * NT] = w[k];
  if (tid == 0) {
    if (A.apply) {
      if (A.resid != nullptr) A.resid[b] = err;
    } else {
      A.it[b] = it; A.err[b] = err; A.status[b] = status;
    }
  }
}

// start of a solve: every problem open (or, with max_iter < 1, at its limit before the first application)
__global__ void batch_init_kernel(int B, int* status, long long* it, double* err, double tol, long long max_iter) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) { status[b] = max_iter > 0 ? BATCH_OPEN : BATCH_MAX_ITER; it[b] = 0; err[b] = tol + 1.0; }
}

using batch_fn = void (*)(const BatchDesc*, const BatchArgs);

// the instantiation for a grid of N points: threads per workgroup and points per thread (none beyond 512 x 32 points)
inline batch_fn batch_kernel_for(int N, int* nt, int* k) {
  struct V { int nt, k; batch_fn f; };
  static const V v[] = {
      {256, 1, batch_sa_kernel<1, 256>},   {256, 2, batch_sa_kernel<2, 256>},   {256, 4, batch_sa_kernel<4, 256>},
      {256, 8, batch_sa_kernel<8, 256>},   {512, 8, batch_sa_kernel<8, 512>},   {512, 12, batch_sa_kernel<12, 512>},
      {512, 16, batch_sa_kernel<16, 512>}, {512, 20, batch_sa_kernel<20, 512>}, {512, 24, batch_sa_kernel<24, 512>},
      {512, 28, batch_sa_kernel<28, 512>}, {512, 32, batch_sa_kernel<32, 512>}};
  for (const V& e : v)
    if ((long long)e.nt * e.k >= N) { *nt = e.nt; *k = e.k; return e.f; }
  return nullptr;
}

}  // namespace sdfs

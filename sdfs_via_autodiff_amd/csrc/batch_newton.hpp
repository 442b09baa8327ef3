// batch_newton.hpp -- Newton-Krylov for a batch of parameter vectors: one workgroup per problem (beside batch_kernels.hpp).
//
// The reference's Newton loop (code/solvers.py:51-95: x <- x - step, step = BiCGSTAB((J - I), T x - x), error = max|step|,
// while error > tol and it < max_iter) with the stopping rule of its inner solve (x0 = 0, |r|^2 <= max(rtol^2 |g|^2,
// atol^2), the early exit on |s|^2, the breakdown exits), every problem in its own workgroup and stopping on its own.
// The problem state is that of batch_sa_kernel: tables and the work buffer of N doubles in LDS, the a3 index of a point in
// 16 bits.  One launch is a state machine over operator applications; a problem is in one of three phases:
//   T  one application of T as in the SA kernel, keeping  c_in = w^theta / w  and  c_out = beta a3 (a3 S)^(1/theta) / (a3 S)
//      (no extra power);  g = T w - w;  r = rhat = p = q = g, x = 0, alpha = omega = rho = 1;
//   A  rho' = <rhat, r>, p = r + beta (p - omega q), q = (J - I) p = c_out . H(c_in . p) - p, alpha = rho' / <rhat, q>,
//      s = r - alpha q (over r), |s|^2 -- below the threshold: x += alpha p and the iteration ends;
//   B  t = (J - I) s, left in the LDS buffer at the thread's own points, omega = <t, s> / <t, t>,
//      x += alpha p + omega s, r = s - omega t, |r|^2.
// After A's early exit, after B and after T the loop head of the inner solve decides: another iteration (A) or the end of
// the Newton step (w -= x, error = max|x|, the outer stopping test, T).  H is the axis-by-axis contraction of the SA
// kernel (batch_lines); a J.v has no power function.
// Inner products are fp64 in a fixed order: per thread over its points (k ascending), wave_sum_f64, then one LDS step
// over the waves (wave 0 first).  No atomics; results leave through plain vector stores.
// Placement of the eight vectors w, r, rhat, p, q, x, c_in, c_out (REG):
//   REG = true   all eight in registers, K points per thread (16 K VGPRs): 256 threads, K <= 8, up to 2048 points;
//   REG = false  all eight in global memory: w in the caller's buffer, the other seven in the problem's slot of the
//                workspace (7 x nwork doubles).  A thread touches its own points only (p = tid + k NT), so no vector needs
//                a barrier or a fence; the streams are coalesced and stay in L2 / Infinity Cache.
// A launch runs at most `budget` applications (T or J.v) per problem.  When it runs out the scalars of the problem go to
// its BatchNewtonState and (REG) the seven vectors to its workspace slot, all fp64 copies, and the next launch resumes at
// the same phase: nothing a problem computes depends on the budget, on B or on its place in the batch.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_kernels.hpp"

namespace sdfs {

// a batch whose workspace would exceed this runs group after group
constexpr long long BATCH_NEWTON_WS_MAX = 2LL << 30;
constexpr int BATCH_NEWTON_VECS = 7;             // r, rhat, p, q, x, c_in, c_out
enum { BN_PH_T = 0, BN_PH_A = 1, BN_PH_B = 2 };

struct BatchNewtonState {                        // one per problem; written by batch_newton_init_kernel
  double alpha, omega, rho, rho_new, atol2, rr;
  long long k;                                   // inner iterations of this step (-10 / -11: breakdown)
  long long napply;                              // applications of T plus J.v so far
  int phase, pad;
};

struct BatchNewtonArgs {
  const double* tab;           // [B][tabwords]
  const double* scal;          // [B][4]
  double* w;                   // [B][N] in and out
  double* ws;                  // [slots][7][nwork]
  BatchNewtonState* st;        // [B]
  int* status;                 // [B]
  long long* it;               // [B] Newton steps so far
  double* err;                 // [B] last max|step|
  double tol, rtol2, atol2;    // outer tolerance; squares of the inner tolerances
  long long max_iter, inner_max;
  int budget;                  // most applications of this launch
  int b0;                      // first problem of the group: workgroup i runs problem b0 + i in slot i
};

template <int K, bool REG> struct BatchVec {
  double a[REG ? K : 1];
  double* g;
  __device__ __forceinline__ double get(int k, int p) const { if constexpr (REG) return a[k]; else return g[p]; }
  __device__ __forceinline__ void set(int k, int p, double v) { if constexpr (REG) a[k] = v; else g[p] = v; }
};

// workgroup-wide sum / maximum of one double per thread; uniform result.  Consecutive calls alternate between two sets of
// NW slots, so one barrier per call is enough.
template <int NW> __device__ __forceinline__ double bn_sum(double v, double* red, int wave, int lane, int& par) {
  v = wave_sum_f64(v);
  double* const r = red + par * (BATCH_RED / 2);
  par ^= 1;
  if (lane == 0) r[wave] = v;
  __syncthreads();
  double m = r[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) m += r[i];
  return readlane_f64(m, 0);
}
template <int NW> __device__ __forceinline__ double bn_max(double v, double* red, int wave, int lane, int& par) {
  v = wave_max_f64(v);
  double* const r = red + par * (BATCH_RED / 2);
  par ^= 1;
  if (lane == 0) r[wave] = v;
  __syncthreads();
  double m = r[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) m = fmax(m, r[i]);
  return readlane_f64(m, 0);
}
__device__ __forceinline__ long long bn_uni(long long v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffLL)), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
  return ((long long)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ bool bn_finite(double v) { return fabs(v) < __builtin_huge_val(); }

__device__ __forceinline__ int bn_a3_index(const BatchDesc& D, int pt) {
  int ia = 0;
#pragma unroll
  for (int a = 0; a < BATCH_MAXD; ++a)
    if (a < D.ndim && D.a3s[a] != 0) ia += (int)(((unsigned)pt / (unsigned)D.stride[a]) % (unsigned)D.n[a]) * D.a3s[a];
  return ia;
}

template <int K, int NT, bool REG>
__global__ __launch_bounds__(NT, NT / 256) void batch_newton_kernel(const BatchDesc* __restrict__ Dp, const BatchNewtonArgs A) {
  const BatchDesc& D = *Dp;
  extern __shared__ __attribute__((aligned(16))) double batch_lds[];
  constexpr int PG = K < 4 ? K : (K >= 32 ? 2 : 4);      // points per call of the power routine, as in batch_sa_kernel
  constexpr int CH = K < 4 ? K : 4;                      // points per group of the vector updates (their loads overlap)
  static_assert(K % PG == 0 && K % CH == 0, "whole groups");
  constexpr int NW = NT / 64;
  static_assert(2 * NW <= BATCH_RED, "two sets of one slot per wave");
  const int slot = blockIdx.x, b = A.b0 + slot;
  if (A.status[b] != BATCH_OPEN) return;                 // uniform: this problem has finished
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
  const double* const a3 = tb + D.a3off;
  const double INF_ = __builtin_huge_val();

  // ---- the problem's state ---------------------------------------------------------------------------------------------
  BatchNewtonState S = A.st[b];
  double alpha = readlane_f64(S.alpha, 0), omega = readlane_f64(S.omega, 0), rho = readlane_f64(S.rho, 0);
  double rho_new = readlane_f64(S.rho_new, 0), atol2 = readlane_f64(S.atol2, 0), rr = readlane_f64(S.rr, 0);
  long long kin = bn_uni(S.k), napply = bn_uni(S.napply), it = bn_uni(A.it[b]);
  int phase = __builtin_amdgcn_readfirstlane(S.phase);
  double err = readlane_f64(A.err[b], 0);
  int status = BATCH_OPEN;
  int par = 0;

  BatchVec<K, REG> w, r, rh, p, q, x, cin, cout;
  double* const wsb = A.ws + (size_t)slot * BATCH_NEWTON_VECS * D.nwork;
  w.g = A.w + (size_t)b * N;
  r.g = wsb; rh.g = wsb + D.nwork; p.g = wsb + 2 * (size_t)D.nwork; q.g = wsb + 3 * (size_t)D.nwork;
  x.g = wsb + 4 * (size_t)D.nwork; cin.g = wsb + 5 * (size_t)D.nwork; cout.g = wsb + 6 * (size_t)D.nwork;
  // the a3 index of a point: packed as in batch_sa_kernel where the vectors live in registers; computed where it is used
  // (once per Newton step) where they do not, so that the loops over the points need not be unrolled
  unsigned ia3[REG ? (K + 1) / 2 : 1];
  if constexpr (REG) {
#pragma unroll
    for (int k = 0; k < (K + 1) / 2; ++k) ia3[k] = 0u;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int pt = tid + k * NT;
      ia3[k >> 1] |= (pt < N ? (unsigned)bn_a3_index(D, pt) : 0u) << (16 * (k & 1));
    }
  }
  if constexpr (REG) {
    const bool resume = phase != BN_PH_T;                // the vectors of an inner solve in progress were parked
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int pt = tid + k * NT;
      const bool ok = pt < N;
      w.a[k] = ok ? w.g[ok ? pt : 0] : 1.0;
      const bool ld = ok && resume;
      r.a[k] = ld ? r.g[ld ? pt : 0] : 0.0;
      rh.a[k] = ld ? rh.g[ld ? pt : 0] : 0.0;
      p.a[k] = ld ? p.g[ld ? pt : 0] : 0.0;
      q.a[k] = ld ? q.g[ld ? pt : 0] : 0.0;
      x.a[k] = ld ? x.g[ld ? pt : 0] : 0.0;
      cin.a[k] = ld ? cin.g[ld ? pt : 0] : 0.0;
      cout.a[k] = ld ? cout.g[ld ? pt : 0] : 0.0;
    }
  }
  __syncthreads();

  for (int used = 0; used < A.budget; ++used) {
    // ---- before the contraction: the vector H acts on goes to the work buffer -------------------------------------------
    if (phase == BN_PH_T) {
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += PG) {
        if (k0 * NT + wave * 64 < N) {
          double xin[PG], xw[PG];
#pragma unroll
          for (int j = 0; j < PG; ++j) { const int pt = tid + (k0 + j) * NT; xin[j] = pt < N ? w.get(k0 + j, pt) : 1.0; }
          P1.run<PG>(xin, xw);
#pragma unroll
          for (int j = 0; j < PG; ++j) {
            const int pt = tid + (k0 + j) * NT;
            if (pt < N) { wk[pt] = xw[j]; cin.set(k0 + j, pt, xw[j] / xin[j]); }
          }
        }
      }
    } else if (phase == BN_PH_A) {
      double part = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double u[CH], v[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; const bool ok = pt < N; u[j] = ok ? rh.get(k0 + j, pt) : 0.0; v[j] = ok ? r.get(k0 + j, pt) : 0.0; }
#pragma unroll
        for (int j = 0; j < CH; ++j) part = fma(u[j], v[j], part);
      }
      rho_new = bn_sum<NW>(part, red, wave, lane, par);
      const double bk = rho_new / rho * alpha / omega;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double rv[CH], pv[CH], qv[CH], cv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT; const bool ok = pt < N;
          rv[j] = ok ? r.get(k0 + j, pt) : 0.0; pv[j] = ok ? p.get(k0 + j, pt) : 0.0;
          qv[j] = ok ? q.get(k0 + j, pt) : 0.0; cv[j] = ok ? cin.get(k0 + j, pt) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT;
          if (pt < N) {
            const double pn = rv[j] + bk * (pv[j] - omega * qv[j]);
            p.set(k0 + j, pt, pn);
            wk[pt] = cv[j] * pn;
          }
        }
      }
    } else {
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double sv[CH], cv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; const bool ok = pt < N; sv[j] = ok ? r.get(k0 + j, pt) : 0.0; cv[j] = ok ? cin.get(k0 + j, pt) : 0.0; }
#pragma unroll
        for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; if (pt < N) wk[pt] = cv[j] * sv[j]; }
      }
    }
    __syncthreads();
    // ---- the contractions, axis by axis, in place ---------------------------------------------------------------------------
    for (int a = 0; a < D.ndim; ++a) {
      const int n = D.n[a], s = D.stride[a], nl = N / n;
      const double* const qm = tb + D.qoff[a];
      switch (D.np[a]) {
        case 4: batch_lines<4>(wk, qm, n, s, nl, tid, NT); break;
        case 8: batch_lines<8>(wk, qm, n, s, nl, tid, NT); break;
        case 12: batch_lines<12>(wk, qm, n, s, nl, tid, NT); break;
        case 16: batch_lines<16>(wk, qm, n, s, nl, tid, NT); break;
        case 24: batch_lines<24>(wk, qm, n, s, nl, tid, NT); break;
        default: batch_lines<32>(wk, qm, n, s, nl, tid, NT); break;
      }
      __syncthreads();
    }
    ++napply;
    // ---- after the contraction ----------------------------------------------------------------------------------------------
    bool head = false;                                   // the loop head of the inner solve decides what comes next
    double omega_new = omega;
    if (phase == BN_PH_T) {
      double part = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += PG) {
        if (k0 * NT + wave * 64 < N) {
          double ks[PG], uu[PG], av[PG];
#pragma unroll
          for (int j = 0; j < PG; ++j) {
            const int pt = tid + (k0 + j) * NT;
            if constexpr (REG) av[j] = a3[(ia3[(k0 + j) >> 1] >> (16 * ((k0 + j) & 1))) & 0xffffu];
            else av[j] = a3[pt < N ? bn_a3_index(D, pt) : 0];
            ks[j] = pt < N ? av[j] * wk[pt] : 1.0;
          }
          P2.run<PG>(ks, uu);
#pragma unroll
          for (int j = 0; j < PG; ++j) {
            const int pt = tid + (k0 + j) * NT;
            if (pt < N) {
              const double y = 1.0 + beta * uu[j];
              const double g = y - w.get(k0 + j, pt);
              cout.set(k0 + j, pt, beta * av[j] * uu[j] / ks[j]);
              r.set(k0 + j, pt, g); rh.set(k0 + j, pt, g); p.set(k0 + j, pt, g); q.set(k0 + j, pt, g);
              x.set(k0 + j, pt, 0.0);
              part = fma(g, g, part);
            }
          }
        }
      }
      const double gg = bn_sum<NW>(part, red, wave, lane, par);
      if (!bn_finite(gg)) { status = BATCH_NONFINITE; err = INF_; ++it; break; }      // T w or g left the finite range
      atol2 = fmax(A.rtol2 * gg, A.atol2);
      rr = gg;
      alpha = omega = rho = 1.0;
      omega_new = 1.0;
      kin = 0;
      head = true;
    } else if (phase == BN_PH_A) {
      double part = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double cv[CH], pv[CH], hv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT; const bool ok = pt < N;
          cv[j] = ok ? cout.get(k0 + j, pt) : 0.0; pv[j] = ok ? p.get(k0 + j, pt) : 0.0; hv[j] = ok ? rh.get(k0 + j, pt) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT;
          if (pt < N) {
            const double qn = cv[j] * wk[pt] - pv[j];
            q.set(k0 + j, pt, qn);
            part = fma(hv[j], qn, part);
          }
        }
      }
      const double rhq = bn_sum<NW>(part, red, wave, lane, par);
      alpha = rho_new / rhq;
      part = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double rv[CH], qv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; const bool ok = pt < N; rv[j] = ok ? r.get(k0 + j, pt) : 0.0; qv[j] = ok ? q.get(k0 + j, pt) : 0.0; }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT;
          if (pt < N) {
            const double sn = rv[j] - alpha * qv[j];
            r.set(k0 + j, pt, sn);                       // s overwrites r
            part = fma(sn, sn, part);
          }
        }
      }
      const double ss = bn_sum<NW>(part, red, wave, lane, par);
      if (!bn_finite(alpha) || !bn_finite(ss)) { status = BATCH_NONFINITE; err = INF_; ++it; break; }
      if (ss < atol2) {
#pragma unroll(REG ? K : 1)
        for (int k0 = 0; k0 < K; k0 += CH) {
          double xv[CH], pv[CH];
#pragma unroll
          for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; const bool ok = pt < N; xv[j] = ok ? x.get(k0 + j, pt) : 0.0; pv[j] = ok ? p.get(k0 + j, pt) : 0.0; }
#pragma unroll
          for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; if (pt < N) x.set(k0 + j, pt, xv[j] + alpha * pv[j]); }
        }
        rr = ss;
        head = true;
      } else {
        phase = BN_PH_B;
      }
    } else {
      double pts = 0.0, ptt = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double cv[CH], sv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; const bool ok = pt < N; cv[j] = ok ? cout.get(k0 + j, pt) : 0.0; sv[j] = ok ? r.get(k0 + j, pt) : 0.0; }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT;
          if (pt < N) {
            const double t = cv[j] * wk[pt] - sv[j];
            wk[pt] = t;                                  // the thread's own point: t waits here for omega
            pts = fma(t, sv[j], pts);
            ptt = fma(t, t, ptt);
          }
        }
      }
      const double ts = bn_sum<NW>(pts, red, wave, lane, par);
      const double tt = bn_sum<NW>(ptt, red, wave, lane, par);
      omega_new = ts / tt;
      double part = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double xv[CH], pv[CH], sv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT; const bool ok = pt < N;
          xv[j] = ok ? x.get(k0 + j, pt) : 0.0; pv[j] = ok ? p.get(k0 + j, pt) : 0.0; sv[j] = ok ? r.get(k0 + j, pt) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT;
          if (pt < N) {
            x.set(k0 + j, pt, (xv[j] + alpha * pv[j]) + omega_new * sv[j]);
            const double rn = sv[j] - omega_new * wk[pt];
            r.set(k0 + j, pt, rn);
            part = fma(rn, rn, part);
          }
        }
      }
      rr = bn_sum<NW>(part, red, wave, lane, par);
      if (!bn_finite(omega_new) || !bn_finite(rr)) { status = BATCH_NONFINITE; err = INF_; ++it; break; }
      head = true;
    }
    if (!head) continue;
    if (phase != BN_PH_T) {                              // the end of a BiCGSTAB iteration (oracle/solvers.py:89-95)
      if (rho_new == 0.0) kin = -10;
      else if (omega_new == 0.0 || alpha == 0.0) kin = -11;
      else ++kin;
      omega = omega_new; rho = rho_new;
    }
    if (rr > atol2 && kin >= 0 && kin < A.inner_max) { phase = BN_PH_A; continue; }
    // ---- the end of a Newton step: w <- w - x, error = max|x| -------------------------------------------------------------
    double emax = 0.0, bad = 0.0;
#pragma unroll(REG ? K : 1)
    for (int k0 = 0; k0 < K; k0 += CH) {
      double xv[CH], wv[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; const bool ok = pt < N; xv[j] = ok ? x.get(k0 + j, pt) : 0.0; wv[j] = ok ? w.get(k0 + j, pt) : 1.0; }
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int pt = tid + (k0 + j) * NT;
        if (pt < N) {
          double e = fabs(xv[j]);
          e = e < INF_ ? e : INF_;                       // NaN and Inf
          emax = fmax(emax, e);
          const double wn = wv[j] - xv[j];
          w.set(k0 + j, pt, wn);
          bad = wn > 0.0 ? bad : 1.0;                    // T is defined on positive iterates only
        }
      }
    }
    err = bn_max<NW>(emax, red, wave, lane, par);
    bad = bn_max<NW>(bad, red, wave, lane, par);
    ++it;
    phase = BN_PH_T;
    if (!(err < INF_) || bad > 0.0) { status = BATCH_NONFINITE; err = INF_; }
    else if (!(err > A.tol)) status = BATCH_CONVERGED;
    else if (it >= A.max_iter) status = BATCH_MAX_ITER;
    if (status != BATCH_OPEN) break;                     // uniform
  }

  if constexpr (REG) {
    const bool park = status == BATCH_OPEN && phase != BN_PH_T;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int pt = tid + k * NT;
      if (pt < N) {
        w.g[pt] = w.a[k];
        if (park) {
          r.g[pt] = r.a[k]; rh.g[pt] = rh.a[k]; p.g[pt] = p.a[k]; q.g[pt] = q.a[k];
          x.g[pt] = x.a[k]; cin.g[pt] = cin.a[k]; cout.g[pt] = cout.a[k];
        }
      }
    }
  }
  if (tid == 0) {
    BatchNewtonState O;
    O.alpha = alpha; O.omega = omega; O.rho = rho; O.rho_new = rho_new; O.atol2 = atol2; O.rr = rr;
    O.k = kin; O.napply = napply; O.phase = phase; O.pad = 0;
    A.st[b] = O;
    A.it[b] = it; A.err[b] = err; A.status[b] = status;
  }
}

// start of a Newton solve: every problem open at phase T (or, with max_iter < 1, at its limit before the first application)
__global__ void batch_newton_init_kernel(int B, int* status, long long* it, double* err, BatchNewtonState* st, double tol, long long max_iter) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    status[b] = max_iter > 0 ? BATCH_OPEN : BATCH_MAX_ITER; it[b] = 0; err[b] = tol + 1.0;
    BatchNewtonState O;
    O.alpha = O.omega = O.rho = O.rho_new = 1.0; O.atol2 = 0.0; O.rr = 0.0; O.k = 0; O.napply = 0; O.phase = BN_PH_T; O.pad = 0;
    st[b] = O;
  }
}

using batch_newton_fn = void (*)(const BatchDesc*, const BatchNewtonArgs);

// the instantiation for a grid of N points: the threads and points per thread of batch_kernel_for; *reg = the vectors
// live in registers
inline batch_newton_fn batch_newton_kernel_for(int N, int* nt, int* k, int* reg) {
  struct V { int nt, k, reg; batch_newton_fn f; };
  static const V v[] = {
      {256, 1, 1, batch_newton_kernel<1, 256, true>},    {256, 2, 1, batch_newton_kernel<2, 256, true>},
      {256, 4, 1, batch_newton_kernel<4, 256, true>},    {256, 8, 1, batch_newton_kernel<8, 256, true>},
      {512, 8, 0, batch_newton_kernel<8, 512, false>},   {512, 12, 0, batch_newton_kernel<12, 512, false>},
      {512, 16, 0, batch_newton_kernel<16, 512, false>}, {512, 20, 0, batch_newton_kernel<20, 512, false>},
      {512, 24, 0, batch_newton_kernel<24, 512, false>}, {512, 28, 0, batch_newton_kernel<28, 512, false>},
      {512, 32, 0, batch_newton_kernel<32, 512, false>}};
  for (const V& e : v)
    if ((long long)e.nt * e.k >= N) { *nt = e.nt; *k = e.k; *reg = e.reg; return e.f; }
  return nullptr;
}

}  // namespace sdfs

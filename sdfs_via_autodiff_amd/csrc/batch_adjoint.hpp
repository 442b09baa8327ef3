// batch_adjoint.hpp -- gradients of <g, w*> for a batch of parameter vectors: one workgroup per problem (beside
// batch_newton.hpp, whose geometry, table block, PowK, BatchVec and bn_sum / bn_max it uses).
//
// For phi = <g, w*> the implicit function theorem gives  dphi/dp = <lambda, dT/dp>,  lambda = (I - J(w*)^T)^(-1) g.  With
// the tangent formula of T and <lambda, J v> = <J^T lambda, v>, every parameter's derivative is a dot product
// of small host tables with a few adjoint moments of the problem, which do not depend on the parameter.  With
//   m = lambda . (T w - 1),   mu = (J^T lambda) . w,   S = H(w^theta) = a2 . E   (the contraction the linearising
//   application leaves in the work buffer; H carries a1 on the next h_lam state and a2 on the current h_c state)
// the moment block of a problem is  s0 s1 s2 | R[ndim] | M1[n_lam] | M2[n_c] | M3[na3]:
//   s0 = sum m,   s1 = sum m ln((T w - 1) / beta),   s2 = sum mu ln w,
//   M1[i_lam] = sum over the other axes of mu,   M2[i_c] = the same of m,   M3[ia3] = sum over (h_c, h_lam) of m,
//   R[k] = sum_x m(x) ( i_k (E(i_k - 1) / E(i_k) - 1) + (n_k - 1 - i_k) (E(i_k + 1) / E(i_k) - 1) )   per grid axis k,
// the Ehrenfest generator as a stencil; E_j / E_i - 1 = (S_j - S_i) / S_i on every axis but h_c, where it is
// (S_j a2_i - S_i a2_j) / (S_i a2_j) with a2 from a small per-problem table in global memory.
//
// One launch is a state machine over operator applications; a problem is in one of five phases:
//   L   phase T of the Newton kernel without the Newton update: c_in = w^theta / w, c_out = beta a3 (a3 S)^(1/theta) /
//       (a3 S), resid_T = max|T w - w|;  r = rhat = p = q = g, x = 0, alpha = omega = rho = 1;
//   A   rho' = <rhat, r>, p = r + beta (p - omega q), q = (I - J^T) p = p - c_in . H^T(c_out . p), alpha = rho' / <rhat, q>,
//       s = r - alpha q (over r), |s|^2 -- below the threshold: x += alpha p and the iteration ends;
//   B   t = (I - J^T) s in the LDS buffer at the thread's own points, omega = <t, s> / <t, t>, x += alpha p + omega s,
//       r = s - omega t, |r|^2;
//   M1  after the solve has stopped for any reason: J^T x computed explicitly (not as x - g), mu = (J^T x) . w over q, and
//       the true residual g - x + J^T x.  The recurrence's r drifts from it by rounding (in proportion to the peaks of the
//       iteration); where the true residual is still above the threshold and neither inner_max nor a breakdown stopped
//       the solve, BiCGSTAB restarts from it with x kept (phase A; at most BA_RESTARTS times);
//   M2  S = H(c_in . w) back into LDS, T w - 1 = c_out . S, the sums and the marginals; the problem ends.
// The stopping rule is the Newton kernel's inner solve: |r|^2 <= max(rtol^2 |g|^2, atol^2), the early exit on |s|^2, the
// breakdown exits (rho' = 0; omega = 0 or alpha = 0) and inner_max.  H^T is the axis-by-axis contraction with each folded
// matrix transposed in place (batch_lines_t); all tensors of a batch handle are unconditional, so the axes commute.
// Inner products and moments are fp64 in a fixed order: per thread over its points (k ascending), wave_sum_f64, then one
// LDS step over the waves (wave 0 first); a marginal entry is summed by one wave (M1, M2) or one thread (M3) from the
// per-point values in the work buffer, in index order.  No atomics; results leave through plain vector stores.
// Placement as in the Newton kernel: REG = true keeps w, r, rhat, p, q, x, c_in, c_out in registers (K <= 8, up to 2048
// points), REG = false keeps them in global memory (w in the caller's buffer, seven in the workspace slot).  A launch runs
// at most `budget` applications per problem; the scalars go to its BatchAdjointState and (REG) the seven vectors to its
// workspace slot, all fp64 copies, and the next launch resumes at the same phase: nothing a problem computes depends on
// the budget, on B or on its place in the batch.  No LDS beyond that of the SA kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_newton.hpp"

namespace sdfs {

enum { BA_PH_L = 0, BA_PH_A = 1, BA_PH_B = 2, BA_PH_M1 = 3, BA_PH_M2 = 4 };
constexpr int BA_RESTARTS = 2;                   // most restarts of a solve from its true residual

struct BatchAdjointState {                       // one per problem; written by batch_adjoint_init_kernel
  double alpha, omega, rho, rho_new, atol2, rr, gg, resid_T;
  double tr;                                     // |g - x + J^T x|^2 of the last M1: the true residual
  long long k;                                   // BiCGSTAB iterations so far
  long long napply;                              // applications so far (L, H^T, those of the moment phase)
  int phase, brk;                                // brk: the solve met a breakdown exit
  int restarts, pad;                             // restarts from the true residual so far
};

struct BatchAdjointArgs {
  const double* tab;           // [B][tabwords]
  const double* scal;          // [B][4]
  const double* w;             // [B][N]
  const double* g;             // [B][N] (g_stride = N) or [N] (g_stride = 0)
  const double* a2;            // [B][n_c]
  double* lam;                 // [B][N] or NULL
  double* mom;                 // [B][words]
  double* ws;                  // [slots][7][nwork]
  BatchAdjointState* st;       // [B]
  int* status;                 // [B]
  double rtol2, atol2;         // squares of the tolerances
  long long inner_max;
  long long g_stride;
  int budget;                  // most applications of this launch
  int b0;                      // first problem of the group: workgroup i runs problem b0 + i in slot i
  int ax_lam, ax_c;            // the h_lam and h_c axes
  int na3, words;              // entries of the a3 table; doubles per moment block
};

// all lines of one axis with the transposed matrix, in place: out[c] = sum_r q[r][c] x[r], r ascending.  Row r of the
// table is read whole at a wave-uniform address while x[r] comes from the line; the padding columns of q are zero.
template <int NP>
__device__ __forceinline__ void batch_lines_t(double* wk, const double* q, int n, int s, int nlines, int tid, int nt) {
  for (int L = tid; L < nlines; L += nt) {
    const int o = (int)((unsigned)L / (unsigned)s), i = L - o * s;
    double* const p = wk + o * n * s + i;
    double acc[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) acc[j] = 0.0;
#pragma unroll 2
    for (int r = 0; r < n; ++r) {
      const double* const qr = q + r * NP;
      const double xr = p[r * s];
#pragma unroll
      for (int j = 0; j < NP; ++j) acc[j] = fma(qr[j], xr, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) if (j < n) p[j * s] = acc[j];
  }
}

template <int K, int NT, bool REG>
__global__ __launch_bounds__(NT, NT / 256) void batch_adjoint_kernel(const BatchDesc* __restrict__ Dp, const BatchAdjointArgs A) {
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
  const double NAN_ = __builtin_nan("");

  // ---- the problem's state ---------------------------------------------------------------------------------------------
  BatchAdjointState S = A.st[b];
  double alpha = readlane_f64(S.alpha, 0), omega = readlane_f64(S.omega, 0), rho = readlane_f64(S.rho, 0);
  double rho_new = readlane_f64(S.rho_new, 0), atol2 = readlane_f64(S.atol2, 0), rr = readlane_f64(S.rr, 0);
  double gg = readlane_f64(S.gg, 0), resid_T = readlane_f64(S.resid_T, 0), tr = readlane_f64(S.tr, 0);
  long long kin = bn_uni(S.k), napply = bn_uni(S.napply);
  int phase = __builtin_amdgcn_readfirstlane(S.phase), brk = __builtin_amdgcn_readfirstlane(S.brk);
  int restarts = __builtin_amdgcn_readfirstlane(S.restarts);
  int status = BATCH_OPEN;
  int par = 0;

  BatchVec<K, REG> w, r, rh, p, q, x, cin, cout;
  double* const wsb = A.ws + (size_t)slot * BATCH_NEWTON_VECS * D.nwork;
  w.g = const_cast<double*>(A.w) + (size_t)b * N;        // read only
  r.g = wsb; rh.g = wsb + D.nwork; p.g = wsb + 2 * (size_t)D.nwork; q.g = wsb + 3 * (size_t)D.nwork;
  x.g = wsb + 4 * (size_t)D.nwork; cin.g = wsb + 5 * (size_t)D.nwork; cout.g = wsb + 6 * (size_t)D.nwork;
  const double* const gsrc = A.g + (size_t)b * (size_t)A.g_stride;
  double* const mom = A.mom + (size_t)b * A.words;
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
    const bool resume = phase != BA_PH_L;                // the vectors of a solve in progress were parked
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
    // ---- before the contraction: the vector H or H^T acts on goes to the work buffer ------------------------------------
    if (phase == BA_PH_L) {
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
    } else if (phase == BA_PH_A) {
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
          qv[j] = ok ? q.get(k0 + j, pt) : 0.0; cv[j] = ok ? cout.get(k0 + j, pt) : 0.0;
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
    } else if (phase == BA_PH_M2) {
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double wv[CH], cv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; const bool ok = pt < N; wv[j] = ok ? w.get(k0 + j, pt) : 0.0; cv[j] = ok ? cin.get(k0 + j, pt) : 0.0; }
#pragma unroll
        for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; if (pt < N) wk[pt] = cv[j] * wv[j]; }
      }
    } else {                                             // B: s (in r); M1: the final x
      const bool fin = phase == BA_PH_M1;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double sv[CH], cv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT; const bool ok = pt < N;
          sv[j] = ok ? (fin ? x.get(k0 + j, pt) : r.get(k0 + j, pt)) : 0.0; cv[j] = ok ? cout.get(k0 + j, pt) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; if (pt < N) wk[pt] = cv[j] * sv[j]; }
      }
    }
    __syncthreads();
    // ---- the contractions, axis by axis, in place: H for L and M2, H^T for the others -----------------------------------
    const bool fwd = phase == BA_PH_L || phase == BA_PH_M2;
    for (int a = 0; a < D.ndim; ++a) {
      const int n = D.n[a], s = D.stride[a], nl = N / n;
      const double* const qm = tb + D.qoff[a];
      if (fwd) {
        switch (D.np[a]) {
          case 4: batch_lines<4>(wk, qm, n, s, nl, tid, NT); break;
          case 8: batch_lines<8>(wk, qm, n, s, nl, tid, NT); break;
          case 12: batch_lines<12>(wk, qm, n, s, nl, tid, NT); break;
          case 16: batch_lines<16>(wk, qm, n, s, nl, tid, NT); break;
          case 24: batch_lines<24>(wk, qm, n, s, nl, tid, NT); break;
          default: batch_lines<32>(wk, qm, n, s, nl, tid, NT); break;
        }
      } else {
        switch (D.np[a]) {
          case 4: batch_lines_t<4>(wk, qm, n, s, nl, tid, NT); break;
          case 8: batch_lines_t<8>(wk, qm, n, s, nl, tid, NT); break;
          case 12: batch_lines_t<12>(wk, qm, n, s, nl, tid, NT); break;
          case 16: batch_lines_t<16>(wk, qm, n, s, nl, tid, NT); break;
          case 24: batch_lines_t<24>(wk, qm, n, s, nl, tid, NT); break;
          default: batch_lines_t<32>(wk, qm, n, s, nl, tid, NT); break;
        }
      }
      __syncthreads();
    }
    ++napply;
    // ---- after the contraction ----------------------------------------------------------------------------------------------
    bool head = false;                                   // the loop head of the solve decides what comes next
    double omega_new = omega;
    if (phase == BA_PH_L) {
      double part = 0.0, rmax = 0.0;
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
              double r0 = fabs(y - w.get(k0 + j, pt));
              r0 = r0 < INF_ ? r0 : INF_;                // NaN and Inf
              rmax = fmax(rmax, r0);
              const double g = gsrc[pt];
              cout.set(k0 + j, pt, beta * av[j] * uu[j] / ks[j]);
              r.set(k0 + j, pt, g); rh.set(k0 + j, pt, g); p.set(k0 + j, pt, g); q.set(k0 + j, pt, g);
              x.set(k0 + j, pt, 0.0);
              part = fma(g, g, part);
            }
          }
        }
      }
      gg = bn_sum<NW>(part, red, wave, lane, par);
      resid_T = bn_max<NW>(rmax, red, wave, lane, par);
      if (!bn_finite(gg) || !(resid_T < INF_)) { status = BATCH_NONFINITE; break; }     // w, T w or g left the finite range
      atol2 = fmax(A.rtol2 * gg, A.atol2);
      rr = gg;
      alpha = omega = rho = 1.0;
      omega_new = 1.0;
      kin = 0; brk = 0; restarts = 0;
      head = true;
    } else if (phase == BA_PH_A) {
      double part = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double cv[CH], pv[CH], hv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT; const bool ok = pt < N;
          cv[j] = ok ? cin.get(k0 + j, pt) : 0.0; pv[j] = ok ? p.get(k0 + j, pt) : 0.0; hv[j] = ok ? rh.get(k0 + j, pt) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT;
          if (pt < N) {
            const double qn = pv[j] - cv[j] * wk[pt];
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
      if (!bn_finite(alpha) || !bn_finite(ss)) { status = BATCH_NONFINITE; break; }
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
        phase = BA_PH_B;
      }
    } else if (phase == BA_PH_B) {
      double pts = 0.0, ptt = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double cv[CH], sv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) { const int pt = tid + (k0 + j) * NT; const bool ok = pt < N; cv[j] = ok ? cin.get(k0 + j, pt) : 0.0; sv[j] = ok ? r.get(k0 + j, pt) : 0.0; }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT;
          if (pt < N) {
            const double t = sv[j] - cv[j] * wk[pt];
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
      if (!bn_finite(omega_new) || !bn_finite(rr)) { status = BATCH_NONFINITE; break; }
      head = true;
    } else if (phase == BA_PH_M1) {
      // J^T x = c_in . H^T(c_out . x), explicitly: mu = (J^T x) . w over q, and the true residual g - x + J^T x
      double part = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double cv[CH], wv[CH], xv[CH], gv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT; const bool ok = pt < N;
          cv[j] = ok ? cin.get(k0 + j, pt) : 0.0; wv[j] = ok ? w.get(k0 + j, pt) : 0.0;
          xv[j] = ok ? x.get(k0 + j, pt) : 0.0; gv[j] = ok ? gsrc[ok ? pt : 0] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT;
          if (pt < N) {
            const double jt = cv[j] * wk[pt];
            const double rt = (gv[j] - xv[j]) + jt;
            q.set(k0 + j, pt, jt * wv[j]);
            wk[pt] = rt;                                 // the thread's own point: kept for a restart
            part = fma(rt, rt, part);
          }
        }
      }
      tr = bn_sum<NW>(part, red, wave, lane, par);
      // The recurrence's residual drifts from the true one by rounding in proportion to the peaks of the iteration; where
      // the true residual is still above the threshold the solve restarts from it (x kept), at most BA_RESTARTS times.
      if (tr > atol2 && restarts < BA_RESTARTS && brk == 0 && kin < A.inner_max) {
#pragma unroll(REG ? K : 1)
        for (int k = 0; k < K; ++k) {
          const int pt = tid + k * NT;
          if (pt < N) { const double rt = wk[pt]; r.set(k, pt, rt); rh.set(k, pt, rt); p.set(k, pt, rt); q.set(k, pt, rt); }
        }
        alpha = omega = rho = 1.0;
        rr = tr;
        ++restarts;
        phase = BA_PH_A;
      } else {
        phase = BA_PH_M2;
      }
      continue;
    } else {
      // ---- M2: S is in the work buffer; m = x (T w - 1) over p, the sums, then the marginals ----------------------------
      double p0 = 0.0, p1 = 0.0, p2 = 0.0, pr[BATCH_MAXD];
#pragma unroll
      for (int a = 0; a < BATCH_MAXD; ++a) pr[a] = 0.0;
      const double* const a2 = A.a2 + (size_t)b * D.n[A.ax_c];
      const double inv_beta = 1.0 / beta;
#pragma unroll(REG ? K : 1)
      for (int k = 0; k < K; ++k) {
        const int pt = tid + k * NT;
        if (pt < N) {
          const double s = wk[pt];
          const double tm1 = cout.get(k, pt) * s;        // T w - 1 = beta (a3 S)^(1/theta) = c_out S
          const double m = x.get(k, pt) * tm1;
          const double mu = q.get(k, pt);
          p.set(k, pt, m);
          p0 += m;
          p1 = fma(m, log(tm1 * inv_beta), p1);
          p2 = fma(mu, log(w.get(k, pt)), p2);
          const double inv_s = 1.0 / s;
#pragma unroll
          for (int a = 0; a < BATCH_MAXD; ++a) {
            if (a < D.ndim) {
              const int n = D.n[a], st = D.stride[a];
              const int i = (int)(((unsigned)pt / (unsigned)st) % (unsigned)n);
              double dm = 0.0, dp = 0.0;
              if (a == A.ax_c) {
                const double ai = a2[i];
                if (i > 0) { const double aj = a2[i - 1]; dm = (wk[pt - st] * ai - s * aj) / (s * aj); }
                if (i < n - 1) { const double aj = a2[i + 1]; dp = (wk[pt + st] * ai - s * aj) / (s * aj); }
              } else {
                if (i > 0) dm = (wk[pt - st] - s) * inv_s;
                if (i < n - 1) dp = (wk[pt + st] - s) * inv_s;
              }
              pr[a] = fma(m, (double)i * dm + (double)(n - 1 - i) * dp, pr[a]);
            }
          }
        }
      }
      const double s0 = bn_sum<NW>(p0, red, wave, lane, par);
      const double s1 = bn_sum<NW>(p1, red, wave, lane, par);
      const double s2 = bn_sum<NW>(p2, red, wave, lane, par);
      double rs[BATCH_MAXD];
#pragma unroll
      for (int a = 0; a < BATCH_MAXD; ++a) rs[a] = a < D.ndim ? bn_sum<NW>(pr[a], red, wave, lane, par) : 0.0;
      if (!bn_finite(s0) || !bn_finite(s1) || !bn_finite(s2)) { status = BATCH_NONFINITE; break; }
      if (tid == 0) {
        mom[0] = s0; mom[1] = s1; mom[2] = s2;
#pragma unroll
        for (int a = 0; a < BATCH_MAXD; ++a) if (a < D.ndim) mom[3 + a] = rs[a];
      }
      double* const m1 = mom + 3 + D.ndim;
      double* const m2 = m1 + D.n[A.ax_lam];
      double* const m3 = m2 + D.n[A.ax_c];
      __syncthreads();                                   // every thread has read its neighbours of S
      // m into the work buffer; M2 (one entry per wave) and M3 (one entry per thread)
#pragma unroll(REG ? K : 1)
      for (int k = 0; k < K; ++k) { const int pt = tid + k * NT; if (pt < N) wk[pt] = p.get(k, pt); }
      __syncthreads();
      {
        const int n = D.n[A.ax_c], st = D.stride[A.ax_c], cnt = N / n;
        for (int e = wave; e < n; e += NW) {
          double acc = 0.0;
          for (int j = lane; j < cnt; j += 64) {
            const int o = (int)((unsigned)j / (unsigned)st);
            acc += wk[o * n * st + (j - o * st) + e * st];
          }
          acc = wave_sum_f64(acc);
          if (lane == 0) m2[e] = acc;
        }
        // the two axes a3 does not depend on: h_c and h_lam
        int c0 = -1, c1 = -1;
        for (int a = 0; a < D.ndim; ++a)
          if (D.a3s[a] == 0) { if (c0 < 0) c0 = a; else c1 = a; }
        const int n0 = D.n[c0], s0_ = D.stride[c0], n1 = D.n[c1], s1_ = D.stride[c1];
        for (int e = tid; e < A.na3; e += NT) {
          int base = 0;
          for (int a = 0; a < D.ndim; ++a)
            if (D.a3s[a] != 0) base += (int)(((unsigned)e / (unsigned)D.a3s[a]) % (unsigned)D.n[a]) * D.stride[a];
          double acc = 0.0;
          for (int i = 0; i < n0; ++i)
            for (int j = 0; j < n1; ++j) acc += wk[base + i * s0_ + j * s1_];
          m3[e] = acc;
        }
      }
      __syncthreads();
      // mu into the work buffer; M1 (one entry per wave)
#pragma unroll(REG ? K : 1)
      for (int k = 0; k < K; ++k) { const int pt = tid + k * NT; if (pt < N) wk[pt] = q.get(k, pt); }
      __syncthreads();
      {
        const int n = D.n[A.ax_lam], st = D.stride[A.ax_lam], cnt = N / n;
        for (int e = wave; e < n; e += NW) {
          double acc = 0.0;
          for (int j = lane; j < cnt; j += 64) {
            const int o = (int)((unsigned)j / (unsigned)st);
            acc += wk[o * n * st + (j - o * st) + e * st];
          }
          acc = wave_sum_f64(acc);
          if (lane == 0) m1[e] = acc;
        }
      }
      status = (rr <= atol2) ? BATCH_CONVERGED : BATCH_MAX_ITER;
      break;
    }
    if (!head) continue;
    if (phase != BA_PH_L) {                              // the end of a BiCGSTAB iteration (oracle/solvers.py:89-95)
      if (rho_new == 0.0 || omega_new == 0.0 || alpha == 0.0) brk = 1;
      else ++kin;
      omega = omega_new; rho = rho_new;
    }
    phase = (rr > atol2 && brk == 0 && kin < A.inner_max) ? BA_PH_A : BA_PH_M1;
  }

  // ---- the end of the launch: lambda and NaNs of a finished problem, the parked vectors of an open one ------------------
  if (status == BATCH_NONFINITE) {
    for (int i = tid; i < A.words; i += NT) mom[i] = NAN_;
    if (A.lam != nullptr) { double* const lo = A.lam + (size_t)b * N; for (int i = tid; i < N; i += NT) lo[i] = NAN_; }
  } else if (status != BATCH_OPEN) {
    if (A.lam != nullptr) {
      double* const lo = A.lam + (size_t)b * N;
#pragma unroll(REG ? K : 1)
      for (int k = 0; k < K; ++k) { const int pt = tid + k * NT; if (pt < N) lo[pt] = x.get(k, pt); }
    }
  } else if constexpr (REG) {
    if (phase != BA_PH_L) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int pt = tid + k * NT;
        if (pt < N) {
          r.g[pt] = r.a[k]; rh.g[pt] = rh.a[k]; p.g[pt] = p.a[k]; q.g[pt] = q.a[k];
          x.g[pt] = x.a[k]; cin.g[pt] = cin.a[k]; cout.g[pt] = cout.a[k];
        }
      }
    }
  }
  if (tid == 0) {
    BatchAdjointState O;
    O.alpha = alpha; O.omega = omega; O.rho = rho; O.rho_new = rho_new; O.atol2 = atol2; O.rr = rr; O.gg = gg;
    O.resid_T = resid_T; O.tr = tr; O.k = kin; O.napply = napply; O.phase = phase; O.brk = brk;
    O.restarts = restarts; O.pad = 0;
    A.st[b] = O;
    A.status[b] = status;
  }
}

// start of an adjoint solve: every problem open at phase L
__global__ void batch_adjoint_init_kernel(int B, int* status, BatchAdjointState* st) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    status[b] = BATCH_OPEN;
    BatchAdjointState O;
    O.alpha = O.omega = O.rho = O.rho_new = 1.0; O.atol2 = 0.0; O.rr = 0.0; O.gg = 0.0; O.resid_T = 0.0;
    O.tr = 0.0; O.k = 0; O.napply = 0; O.phase = BA_PH_L; O.brk = 0; O.restarts = 0; O.pad = 0;
    st[b] = O;
  }
}

using batch_adjoint_fn = void (*)(const BatchDesc*, const BatchAdjointArgs);

// the instantiation for a grid of N points: the table of batch_newton_kernel_for
inline batch_adjoint_fn batch_adjoint_kernel_for(int N, int* nt, int* k, int* reg) {
  struct V { int nt, k, reg; batch_adjoint_fn f; };
  static const V v[] = {
      {256, 1, 1, batch_adjoint_kernel<1, 256, true>},    {256, 2, 1, batch_adjoint_kernel<2, 256, true>},
      {256, 4, 1, batch_adjoint_kernel<4, 256, true>},    {256, 8, 1, batch_adjoint_kernel<8, 256, true>},
      {512, 8, 0, batch_adjoint_kernel<8, 512, false>},   {512, 12, 0, batch_adjoint_kernel<12, 512, false>},
      {512, 16, 0, batch_adjoint_kernel<16, 512, false>}, {512, 20, 0, batch_adjoint_kernel<20, 512, false>},
      {512, 24, 0, batch_adjoint_kernel<24, 512, false>}, {512, 28, 0, batch_adjoint_kernel<28, 512, false>},
      {512, 32, 0, batch_adjoint_kernel<32, 512, false>}};
  for (const V& e : v)
    if ((long long)e.nt * e.k >= N) { *nt = e.nt; *k = e.k; *reg = e.reg; return e.f; }
  return nullptr;
}

}  // namespace sdfs

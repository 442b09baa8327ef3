// batch_price.hpp -- asset prices at w* for a batch of parameter vectors: one workgroup per problem (beside
// batch_adjoint.hpp; the geometry, table block, PowK, BatchVec and bn_sum / bn_max of batch_newton.hpp).
//
// In the batch kernels J v = c_out . H(c_in . v) with H the axis-by-axis contraction (a1 and a2 folded into the matrices),
// c_in = w^theta / w and c_out = beta a3 (a3 S)^(1/theta) / (a3 S).  The tilted operator of DESIGN 4.7 is then
//   K(p, kl, kc) f = d2 . H(d1 . f),   d1 = c_in^p t1[i_lam],   d2 = c_out^p t2[i_c] t3[i_a3],
//   t1 = exp((kl - theta) h_lam),  t2 = exp((kc^2 - (1-gamma)^2) sigma_c^2 / 2),  t3 = exp((kc - p (1-gamma)) (mu_c + z)),
// three small per-problem tables the host builds in fp64 (one set per stage).  K(1, theta, 1-gamma) is J: the tables are 1.
//
// A problem runs five stages.  Each starts with the linearising application L (phase T of the Newton kernel without the
// update: c_in, c_out, resid_T = max|T w - w|), after which c_in and c_out are rescaled in place to the stage's d1 and d2;
// that is the only place that decodes i_lam, i_c and i_a3 for the operator.  Every other application of the stage is the
// Newton kernel's c_out . H(c_in . f) loop.
//   0  claim (skipped without one): k1 = K 1 with K = K(1, theta, kappa - gamma); BiCGSTAB on (I - K) v = k1 with the
//      Newton kernel's phases A / B and stopping rule (|r|^2 <= max(rtol^2 |k1|^2, atol^2), the early exit on |s|^2, the
//      breakdown exits, inner_max); then k1 again (over q) and the true residual k1 - v + K v; where that is above the
//      threshold and neither inner_max nor a breakdown stopped the solve it restarts from it with v kept, at most
//      BP_RESTARTS times.  v stays in x; min v, max v and the number of points with v <= 0 are words 9-11.
//   1  E_M = K(1, theta, -gamma) 1 over r; the weight of every point, prod_a g_a[i_a], over rhat (the per-axis vectors
//      come from global memory; this is the only decode of the reduction side); words 0-2.
//   2  E_M2 = K(2, 2 theta, -2 gamma) 1; word 3 against the E_M in r.
//   3  ER = K(0, 0, kappa)(1 + v) / v; words 4-8 with v and E_M at hand.  Skipped without a claim or where v is not
//      strictly positive (words 4-8 stay NaN).
//   4  horizons: P_n = K(1, theta, kappa_ts - gamma) P_(n-1), P_0 = 1 in p; per horizon <g, P_n>, <g, -ln P_n> / n and
//      the min and max of P_n / P_(n-1).  A horizon with a non-positive or non-finite point ends the loop; its row and
//      the later ones keep the NaN the init kernel wrote.
// Status: 0 done; 1 the claim solve stopped above its tolerance; 2 non-finite (every output of the problem NaN);
// 3 the solve converged but v is not strictly positive, so r(K) >= 1 and the claim has no finite price.
// Sums are fp64 in a fixed order: per thread over its points (k ascending), wave_sum_f64, then one LDS step over the
// waves (wave 0 first).  No atomics; results leave through plain vector stores.  Placement as in the Newton kernel:
// REG = true keeps w and the seven vectors in registers, REG = false in global memory (w in the caller's buffer, seven
// in the workspace slot).  No LDS beyond that of the SA kernel.
//
// A launch runs at most `budget` >= 1 applications per problem; the scalars go to its BatchPriceState and (REG) the seven
// vectors to its workspace slot, and the next launch resumes at the same phase: nothing a problem computes depends on the
// budget, on B or on its place in the batch.  Every pass of the budget loop performs one application and then either
// moves on within a finite count (the stage number, inner_max iterations, BP_RESTARTS restarts, n_max horizons) or closes
// the problem, so the host's relaunch loop ends.  Applications of one problem, at most:
//   stage 0: 1 (L) + 1 (k1) + 2 inner_max + 2 (BP_RESTARTS + 1);  stages 1-3: 2 each;  stage 4: 1 + n_max;
//   in all 2 inner_max + n_max + 2 BP_RESTARTS + 11.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_newton.hpp"

namespace sdfs {

enum { BP_PH_L = 0, BP_PH_ONE = 1, BP_PH_A = 2, BP_PH_B = 3, BP_PH_R = 4, BP_PH_ER = 5, BP_PH_H = 6 };
enum { BATCH_NO_PRICE_DEV = 4 };   // "no finite price" in the status word: BATCH_OPEN is 3 there; the host reports 3
constexpr int BP_RESTARTS = 2;                   // most restarts of the claim solve from its true residual (= BA_RESTARTS of the adjoint kernel)
constexpr int BP_STAGES = 5;
constexpr int BP_WORDS = 12;

struct BatchPriceState {                         // one per problem; written by batch_price_init_kernel
  double alpha, omega, rho, rho_new, atol2, rr, gg, resid_T;
  double tr;                                     // |k1 - v + K v|^2 of the last residual check
  double vbad;                                   // points with v <= 0
  long long k;                                   // BiCGSTAB iterations so far
  long long napply;                              // applications so far
  long long nh;                                  // horizons written so far
  int phase, stage;
  int brk, restarts;                             // the solve met a breakdown exit; restarts from the true residual
  int chk, conv;                                 // the application to 1 is the residual check's; the solve converged
};

struct BatchPriceArgs {
  const double* tab;           // [B][tabwords]
  const double* scal;          // [B][4]
  const double* w;             // [B][N]
  const double* tilt;          // [B][BP_STAGES][tiltwords]: t1[n_lam] t2[n_c] t3[na3] of every stage
  const double* gax;           // [B][sum n_a]: the per-axis weight vectors, axis-major
  double* EM;                  // [B][N] or NULL
  double* EM2;                 // [B][N] or NULL
  double* pd;                  // [B][N] or NULL
  double* ER;                  // [B][N] or NULL
  double* mom;                 // [B][BP_WORDS]
  double* hz;                  // [B][n_max][4] or NULL
  double* ws;                  // [slots][7][nwork]
  BatchPriceState* st;         // [B]
  int* status;                 // [B]
  double rtol2, atol2;         // squares of the tolerances
  long long inner_max, n_max;
  int budget;                  // most applications of this launch
  int b0;                      // first problem of the group: workgroup i runs problem b0 + i in slot i
  int ax_lam, ax_c;            // the h_lam and h_c axes
  int na3, tiltwords, gwords;  // entries of the a3 table; doubles per stage of tilt; sum n_a
  int claim;                   // stage 0 and stage 3 run
};

__device__ __forceinline__ double bp_pow(double c, int p) { return p == 0 ? 1.0 : (p == 1 ? c : c * c); }

template <int K, int NT, bool REG>
__global__ __launch_bounds__(NT, NT / 256) void batch_price_kernel(const BatchDesc* __restrict__ Dp, const BatchPriceArgs A) {
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
  BatchPriceState S = A.st[b];
  double alpha = readlane_f64(S.alpha, 0), omega = readlane_f64(S.omega, 0), rho = readlane_f64(S.rho, 0);
  double rho_new = readlane_f64(S.rho_new, 0), atol2 = readlane_f64(S.atol2, 0), rr = readlane_f64(S.rr, 0);
  double gg = readlane_f64(S.gg, 0), resid_T = readlane_f64(S.resid_T, 0), tr = readlane_f64(S.tr, 0);
  double vbad = readlane_f64(S.vbad, 0);
  long long kin = bn_uni(S.k), napply = bn_uni(S.napply), nh = bn_uni(S.nh);
  int phase = __builtin_amdgcn_readfirstlane(S.phase), stage = __builtin_amdgcn_readfirstlane(S.stage);
  int brk = __builtin_amdgcn_readfirstlane(S.brk), restarts = __builtin_amdgcn_readfirstlane(S.restarts);
  int chk = __builtin_amdgcn_readfirstlane(S.chk), conv = __builtin_amdgcn_readfirstlane(S.conv);
  int status = BATCH_OPEN;
  int par = 0;

  BatchVec<K, REG> w, r, rh, p, q, x, cin, cout;
  double* const wsb = A.ws + (size_t)slot * BATCH_NEWTON_VECS * D.nwork;
  w.g = const_cast<double*>(A.w) + (size_t)b * N;        // read only
  r.g = wsb; rh.g = wsb + D.nwork; p.g = wsb + 2 * (size_t)D.nwork; q.g = wsb + 3 * (size_t)D.nwork;
  x.g = wsb + 4 * (size_t)D.nwork; cin.g = wsb + 5 * (size_t)D.nwork; cout.g = wsb + 6 * (size_t)D.nwork;
  double* const mom = A.mom + (size_t)b * BP_WORDS;
  const double* const gax = A.gax + (size_t)b * A.gwords;
  const bool first = phase == BP_PH_L && napply == 0;    // nothing of this problem is in the workspace yet
  if constexpr (REG) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int pt = tid + k * NT;
      const bool ok = pt < N;
      w.a[k] = ok ? w.g[ok ? pt : 0] : 1.0;
      const bool ld = ok && !first;
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
    if (phase == BP_PH_L) {
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
    } else if (phase == BP_PH_ONE) {
#pragma unroll(REG ? K : 1)
      for (int k = 0; k < K; ++k) { const int pt = tid + k * NT; if (pt < N) wk[pt] = cin.get(k, pt); }
    } else if (phase == BP_PH_A) {
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
    } else {                                             // B: s (in r); R: v; ER: 1 + v; H: P_(n-1) (in p)
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double sv[CH], cv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT; const bool ok = pt < N;
          double f;
          if (phase == BP_PH_B) f = ok ? r.get(k0 + j, pt) : 0.0;
          else if (phase == BP_PH_H) f = ok ? p.get(k0 + j, pt) : 0.0;
          else f = ok ? x.get(k0 + j, pt) : 0.0;
          sv[j] = phase == BP_PH_ER ? 1.0 + f : f;
          cv[j] = ok ? cin.get(k0 + j, pt) : 0.0;
        }
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
    bool head = false;                                   // the loop head of the solve decides what comes next
    bool next_stage = false;                             // this stage has ended
    double omega_new = omega;
    if (phase == BP_PH_L) {
      // c_in and c_out of the linearisation, rescaled to this stage's d1 and d2
      const int pw = stage == 2 ? 2 : (stage == 3 ? 0 : 1);
      const double* const t1 = A.tilt + ((size_t)b * BP_STAGES + stage) * A.tiltwords;
      const double* const t2 = t1 + D.n[A.ax_lam];
      const double* const t3 = t2 + D.n[A.ax_c];
      const unsigned sl = (unsigned)D.stride[A.ax_lam], nl = (unsigned)D.n[A.ax_lam];
      const unsigned sc = (unsigned)D.stride[A.ax_c], nc = (unsigned)D.n[A.ax_c];
      double rmax = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += PG) {
        if (k0 * NT + wave * 64 < N) {
          double ks[PG], uu[PG], av[PG];
          int ia[PG];
#pragma unroll
          for (int j = 0; j < PG; ++j) {
            const int pt = tid + (k0 + j) * NT;
            ia[j] = pt < N ? bn_a3_index(D, pt) : 0;
            av[j] = a3[ia[j]];
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
              const double co = beta * av[j] * uu[j] / ks[j];
              const int il = (int)(((unsigned)pt / sl) % nl), ic = (int)(((unsigned)pt / sc) % nc);
              cout.set(k0 + j, pt, bp_pow(co, pw) * t2[ic] * t3[ia[j]]);
              cin.set(k0 + j, pt, bp_pow(cin.get(k0 + j, pt), pw) * t1[il]);
              if (stage == 4) p.set(k0 + j, pt, 1.0);    // P_0
            }
          }
        }
      }
      resid_T = bn_max<NW>(rmax, red, wave, lane, par);
      if (!(resid_T < INF_)) { status = BATCH_NONFINITE; break; }     // w or T w left the finite range
      if (stage == 0) chk = 0;
      phase = stage == 3 ? BP_PH_ER : (stage == 4 ? BP_PH_H : BP_PH_ONE);
      continue;
    } else if (phase == BP_PH_ONE) {
      if (stage == 0 && chk == 0) {
        // k1 = K 1: the right-hand side; x = 0, r = rhat = p = q = k1
        double part = 0.0;
#pragma unroll(REG ? K : 1)
        for (int k = 0; k < K; ++k) {
          const int pt = tid + k * NT;
          if (pt < N) {
            const double g = cout.get(k, pt) * wk[pt];
            r.set(k, pt, g); rh.set(k, pt, g); p.set(k, pt, g); q.set(k, pt, g);
            x.set(k, pt, 0.0);
            part = fma(g, g, part);
          }
        }
        gg = bn_sum<NW>(part, red, wave, lane, par);
        if (!bn_finite(gg)) { status = BATCH_NONFINITE; break; }
        atol2 = fmax(A.rtol2 * gg, A.atol2);
        rr = gg;
        alpha = omega = rho = 1.0;
        omega_new = 1.0;
        kin = 0; brk = 0; restarts = 0;
        head = true;
      } else if (stage == 0) {
        // k1 again, over q: the residual check follows
#pragma unroll(REG ? K : 1)
        for (int k = 0; k < K; ++k) { const int pt = tid + k * NT; if (pt < N) q.set(k, pt, cout.get(k, pt) * wk[pt]); }
        phase = BP_PH_R;
        continue;
      } else if (stage == 1) {
        // E_M over r, the weights over rhat; words 0-2
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, bad = 0.0;
        double* const eo = A.EM ? A.EM + (size_t)b * N : nullptr;
#pragma unroll(REG ? K : 1)
        for (int k = 0; k < K; ++k) {
          const int pt = tid + k * NT;
          if (pt < N) {
            const double em = cout.get(k, pt) * wk[pt];
            double gw = 1.0;
            int off = 0;
#pragma unroll
            for (int a = 0; a < BATCH_MAXD; ++a) {
              if (a < D.ndim) {
                const int i = (int)(((unsigned)pt / (unsigned)D.stride[a]) % (unsigned)D.n[a]);
                gw = a == 0 ? gax[i] : gw * gax[off + i];
                off += D.n[a];
              }
            }
            r.set(k, pt, em); rh.set(k, pt, gw);
            if (eo) eo[pt] = em;
            bad = (em > 0.0 && em < INF_) ? bad : 1.0;
            const double lr = -log(em);
            p0 += gw;
            p1 = fma(gw, lr, p1);
            p2 = fma(gw, lr * lr, p2);
          }
        }
        const double s0 = bn_sum<NW>(p0, red, wave, lane, par);
        const double s1 = bn_sum<NW>(p1, red, wave, lane, par);
        const double s2 = bn_sum<NW>(p2, red, wave, lane, par);
        bad = bn_max<NW>(bad, red, wave, lane, par);
        if (bad > 0.0) { status = BATCH_NONFINITE; break; }          // E_M left the positive finite numbers
        if (tid == 0) { mom[0] = s0; mom[1] = s1; mom[2] = s2; }
        next_stage = true;
      } else {
        // E_M2; word 3 against E_M
        double p3 = 0.0;
        double* const eo = A.EM2 ? A.EM2 + (size_t)b * N : nullptr;
#pragma unroll(REG ? K : 1)
        for (int k = 0; k < K; ++k) {
          const int pt = tid + k * NT;
          if (pt < N) {
            const double e2 = cout.get(k, pt) * wk[pt];
            const double em = r.get(k, pt);
            if (eo) eo[pt] = e2;
            p3 = fma(rh.get(k, pt), sqrt(fmax(e2 / (em * em) - 1.0, 0.0)), p3);
          }
        }
        const double s3 = bn_sum<NW>(p3, red, wave, lane, par);
        if (tid == 0) mom[3] = s3;
        next_stage = true;
      }
    } else if (phase == BP_PH_A) {
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
            const double qn = pv[j] - cv[j] * wk[pt];    // (I - K) p
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
        phase = BP_PH_B;
      }
    } else if (phase == BP_PH_B) {
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
            const double t = sv[j] - cv[j] * wk[pt];     // (I - K) s
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
    } else if (phase == BP_PH_R) {
      // the true residual k1 - v + K v, with k1 in q
      double part = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k0 = 0; k0 < K; k0 += CH) {
        double cv[CH], xv[CH], gv[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT; const bool ok = pt < N;
          cv[j] = ok ? cout.get(k0 + j, pt) : 0.0; xv[j] = ok ? x.get(k0 + j, pt) : 0.0; gv[j] = ok ? q.get(k0 + j, pt) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const int pt = tid + (k0 + j) * NT;
          if (pt < N) {
            const double rt = (gv[j] - xv[j]) + cv[j] * wk[pt];
            wk[pt] = rt;                                 // the thread's own point: kept for a restart
            part = fma(rt, rt, part);
          }
        }
      }
      tr = bn_sum<NW>(part, red, wave, lane, par);
      if (!bn_finite(tr)) { status = BATCH_NONFINITE; break; }
      // The recurrence's residual drifts from the true one by rounding in proportion to the peaks of the iteration; where
      // the true residual is still above the threshold the solve restarts from it (v kept), at most BP_RESTARTS times.
      if (tr > atol2 && restarts < BP_RESTARTS && brk == 0 && kin < A.inner_max) {
#pragma unroll(REG ? K : 1)
        for (int k = 0; k < K; ++k) {
          const int pt = tid + k * NT;
          if (pt < N) { const double rt = wk[pt]; r.set(k, pt, rt); rh.set(k, pt, rt); p.set(k, pt, rt); q.set(k, pt, rt); }
        }
        alpha = omega = rho = 1.0;
        rr = tr;
        ++restarts;
        phase = BP_PH_A;
        continue;
      }
      // the solve has ended: min v, max v, the points with v <= 0, and pd
      conv = rr <= atol2 ? 1 : 0;
      double vlo = INF_, vhi = -INF_, cnt = 0.0;
      double* const po = A.pd ? A.pd + (size_t)b * N : nullptr;
#pragma unroll(REG ? K : 1)
      for (int k = 0; k < K; ++k) {
        const int pt = tid + k * NT;
        if (pt < N) {
          const double v = x.get(k, pt);
          vlo = fmin(vlo, v); vhi = fmax(vhi, v);
          cnt += v > 0.0 ? 0.0 : 1.0;
          if (po) po[pt] = v;
        }
      }
      vlo = -bn_max<NW>(-vlo, red, wave, lane, par);
      vhi = bn_max<NW>(vhi, red, wave, lane, par);
      vbad = bn_sum<NW>(cnt, red, wave, lane, par);
      if (tid == 0) { mom[9] = vlo; mom[10] = vhi; mom[11] = vbad; }
      next_stage = true;
    } else if (phase == BP_PH_ER) {
      // ER = K(0, 0, kappa)(1 + v) / v; words 4-8
      double p4 = 0.0, p5 = 0.0, p6 = 0.0, p7 = 0.0, p8 = 0.0;
      double* const eo = A.ER ? A.ER + (size_t)b * N : nullptr;
#pragma unroll(REG ? K : 1)
      for (int k = 0; k < K; ++k) {
        const int pt = tid + k * NT;
        if (pt < N) {
          const double v = x.get(k, pt);
          const double er = cout.get(k, pt) * wk[pt] / v;
          const double gw = rh.get(k, pt);
          if (eo) eo[pt] = er;
          const double lv = log(v), le = log(er);
          const double lp = le + log(r.get(k, pt));
          p4 = fma(gw, lv, p4);
          p5 = fma(gw, lv * lv, p5);
          p6 = fma(gw, le, p6);
          p7 = fma(gw, lp, p7);
          p8 = fma(gw, lp * lp, p8);
        }
      }
      const double s4 = bn_sum<NW>(p4, red, wave, lane, par);
      const double s5 = bn_sum<NW>(p5, red, wave, lane, par);
      const double s6 = bn_sum<NW>(p6, red, wave, lane, par);
      const double s7 = bn_sum<NW>(p7, red, wave, lane, par);
      const double s8 = bn_sum<NW>(p8, red, wave, lane, par);
      if (tid == 0) { mom[4] = s4; mom[5] = s5; mom[6] = s6; mom[7] = s7; mom[8] = s8; }
      next_stage = true;
    } else {
      // a horizon: P_n over q, then over p
      double pp = 0.0, py = 0.0, lo = INF_, hi = -INF_, bad = 0.0;
#pragma unroll(REG ? K : 1)
      for (int k = 0; k < K; ++k) {
        const int pt = tid + k * NT;
        if (pt < N) {
          const double pn = cout.get(k, pt) * wk[pt];
          const double ratio = pn / p.get(k, pt);
          const double gw = rh.get(k, pt);
          q.set(k, pt, pn);
          bad = (pn > 0.0 && pn < INF_) ? bad : 1.0;
          pp = fma(gw, pn, pp);
          py = fma(gw, -log(pn), py);
          lo = fmin(lo, ratio); hi = fmax(hi, ratio);
        }
      }
      const double sp = bn_sum<NW>(pp, red, wave, lane, par);
      const double sy = bn_sum<NW>(py, red, wave, lane, par);
      lo = -bn_max<NW>(-lo, red, wave, lane, par);
      hi = bn_max<NW>(hi, red, wave, lane, par);
      bad = bn_max<NW>(bad, red, wave, lane, par);
      if (bad > 0.0) {
        next_stage = true;                               // the prices left the positive numbers: the loop ends here
      } else {
        if (tid == 0) {
          double* const row = A.hz + ((size_t)b * (size_t)A.n_max + (size_t)nh) * 4;
          row[0] = sp; row[1] = sy / (double)(nh + 1); row[2] = lo; row[3] = hi;
        }
#pragma unroll(REG ? K : 1)
        for (int k = 0; k < K; ++k) { const int pt = tid + k * NT; if (pt < N) p.set(k, pt, q.get(k, pt)); }
        ++nh;
        if (nh >= A.n_max) next_stage = true;
      }
    }
    if (head) {
      if (!(stage == 0 && phase == BP_PH_ONE)) {         // the end of a BiCGSTAB iteration (oracle/solvers.py:89-95)
        if (rho_new == 0.0 || omega_new == 0.0 || alpha == 0.0) brk = 1;
        else ++kin;
        omega = omega_new; rho = rho_new;
      }
      if (rr > atol2 && brk == 0 && kin < A.inner_max) phase = BP_PH_A;
      else { phase = BP_PH_ONE; chk = 1; }               // k1 again, then the true residual
      continue;
    }
    if (!next_stage) continue;
    // ---- the next stage that has something to do, or the end of the problem ------------------------------------------------
    ++stage;
    if (stage == 3 && (A.claim == 0 || vbad > 0.0)) ++stage;
    if (stage == 4 && A.n_max == 0) ++stage;
    phase = BP_PH_L;
    if (stage >= BP_STAGES) {
      status = A.claim == 0 ? BATCH_CONVERGED : (conv == 0 ? BATCH_MAX_ITER : (vbad > 0.0 ? BATCH_NO_PRICE_DEV : BATCH_CONVERGED));
      break;
    }
  }

  // ---- the end of the launch: NaNs of a non-finite problem, the parked vectors of an open one ---------------------------
  if (status == BATCH_NONFINITE) {
    for (int i = tid; i < BP_WORDS; i += NT) mom[i] = NAN_;
    if (A.EM != nullptr) { double* const g = A.EM + (size_t)b * N; for (int i = tid; i < N; i += NT) g[i] = NAN_; }
    if (A.EM2 != nullptr) { double* const g = A.EM2 + (size_t)b * N; for (int i = tid; i < N; i += NT) g[i] = NAN_; }
    if (A.pd != nullptr) { double* const g = A.pd + (size_t)b * N; for (int i = tid; i < N; i += NT) g[i] = NAN_; }
    if (A.ER != nullptr) { double* const g = A.ER + (size_t)b * N; for (int i = tid; i < N; i += NT) g[i] = NAN_; }
    if (A.hz != nullptr) { double* const g = A.hz + (size_t)b * (size_t)A.n_max * 4; for (long long i = tid; i < nh * 4; i += NT) g[i] = NAN_; }
    nh = 0;
  } else if (status == BATCH_OPEN) {
    if constexpr (REG) {
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
    BatchPriceState O;
    O.alpha = alpha; O.omega = omega; O.rho = rho; O.rho_new = rho_new; O.atol2 = atol2; O.rr = rr; O.gg = gg;
    O.resid_T = resid_T; O.tr = tr; O.vbad = vbad; O.k = kin; O.napply = napply; O.nh = nh; O.phase = phase; O.stage = stage;
    O.brk = brk; O.restarts = restarts; O.chk = chk; O.conv = conv;
    A.st[b] = O;
    A.status[b] = status;
  }
}

// start of a pricing call: every problem open at the L of its first stage; the moment blocks, the grids of a problem
// without a finite price (ER) and the horizon rows start as NaN and are overwritten by what a problem delivers
__global__ void batch_price_init_kernel(int B, int N, int* status, BatchPriceState* st, double* mom, double* hz, double* ER,
                                        double* pd, long long n_max, int first_stage) {
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
  const double NAN_ = __builtin_nan("");
  for (long long i = i0; i < (long long)B * BP_WORDS; i += step) mom[i] = NAN_;
  if (hz != nullptr) for (long long i = i0; i < (long long)B * n_max * 4; i += step) hz[i] = NAN_;
  if (ER != nullptr) for (long long i = i0; i < (long long)B * N; i += step) ER[i] = NAN_;
  if (pd != nullptr) for (long long i = i0; i < (long long)B * N; i += step) pd[i] = NAN_;     // (a call without a claim)
  for (long long b = i0; b < B; b += step) {
    status[b] = BATCH_OPEN;
    BatchPriceState O;
    O.alpha = O.omega = O.rho = O.rho_new = 1.0; O.atol2 = 0.0; O.rr = 0.0; O.gg = 0.0; O.resid_T = 0.0;
    O.tr = 0.0; O.vbad = 0.0; O.k = 0; O.napply = 0; O.nh = 0; O.phase = BP_PH_L; O.stage = first_stage;
    O.brk = 0; O.restarts = 0; O.chk = 0; O.conv = 0;
    st[b] = O;
  }
}

using batch_price_fn = void (*)(const BatchDesc*, const BatchPriceArgs);

// the instantiation for a grid of N points: the table of batch_newton_kernel_for
inline batch_price_fn batch_price_kernel_for(int N, int* nt, int* k, int* reg) {
  struct V { int nt, k, reg; batch_price_fn f; };
  static const V v[] = {
      {256, 1, 1, batch_price_kernel<1, 256, true>},    {256, 2, 1, batch_price_kernel<2, 256, true>},
      {256, 4, 1, batch_price_kernel<4, 256, true>},    {256, 8, 1, batch_price_kernel<8, 256, true>},
      {512, 8, 0, batch_price_kernel<8, 512, false>},   {512, 12, 0, batch_price_kernel<12, 512, false>},
      {512, 16, 0, batch_price_kernel<16, 512, false>}, {512, 20, 0, batch_price_kernel<20, 512, false>},
      {512, 24, 0, batch_price_kernel<24, 512, false>}, {512, 28, 0, batch_price_kernel<28, 512, false>},
      {512, 32, 0, batch_price_kernel<32, 512, false>}};
  for (const V& e : v)
    if ((long long)e.nt * e.k >= N) { *nt = e.nt; *k = e.k; *reg = e.reg; return e.f; }
  return nullptr;
}

}  // namespace sdfs

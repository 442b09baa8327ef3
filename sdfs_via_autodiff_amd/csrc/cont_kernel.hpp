// Continuous-state Koopmans operator on gfx950: expectation by quadrature / Monte Carlo over
// multilinear interpolation of the current iterate.
//
// Reference (what is computed, not how):
//   code/ssy/continuous_junnan/ssy_wc_ratio_continuous.py  next_state :66-87, Kg_vmap_quad :125-150,
//                                                          Kg_vmap_mc :94-119, T_fun_factory :156-226
//   code/gcy/continuous/gcy_wc_ratio_continuous.py         next_state :78-116, Kg_vmap_quad :159-184
//   code/utils.py:6-23                                      vals_to_coords, lin_interp (order 1, 'nearest')
//
//   Tw(x) = 1 + beta * ( const(x) * sum_m W_m * exp(theta * h_lambda'(x, m)) * interp(w)(x'(x, m))^theta )^(1/theta)
//
// One 256-thread workgroup per grid point x; lanes run over the M shock nodes.  Per node the next
// state is affine in the node (a_d(x) + k_d(x) * eta_d[m], already in grid coordinates), the 2^D
// corners are gathered from the iterate (L2 / MALL resident: 160 KB for the 10x10x10x20 SSY grid,
// 32 MB for the 10^4 x 20^2 GCY grid) and folded depth-first, the power is pow_fast_n.  The factor
// exp(theta * s_lambda * eta_0[m]) of the reference's `pf` is folded into the node weight on the host,
// exp(theta * rho_lambda * h_lambda) into the per-point constant.  No MFMA shape: the power sits
// between the interpolation sum and the quadrature sum.
//
// Gathers.  All next states of one grid point fall in a small box of the grid (one-step shocks are
// short against the stationary range the grids span), so the block first copies that box of the
// iterate into LDS (up to `cap` doubles, else it gathers from global memory) and the 2^D-corner
// reads of every node hit LDS; neighbouring corners along the fastest axis are one ds_read2_b64.
// First version (gathers from L2): 7.4 ms per application at GCY 4x4x4x4x6x6, d = 5; LDS box: 1.7 ms.
//
// Tensor-product rules.  With Gauss-Hermite nodes m = (j_0 .. j_{D-1}) the next state of dimension d
// depends on j_d only, so the interpolation over the two fastest dimensions is done once per
// (outer box cell, j_{D-2}, j_{D-1}) into a second LDS array U and every node then interpolates over
// the D-2 outer dimensions only: 2^(D-2) instead of 2^D corner reads per node (16 instead of 64 in
// 6-D, 4 instead of 16 in 4-D).  Monte-Carlo draws, or boxes that do not fit, take the path above.
#pragma once
#include <hip/hip_runtime.h>
#include "pass_kernel.hpp"

namespace sdfs {

constexpr int CMAXD = 6;

struct ContDesc {
  int D, M;
  long long N;
  int n[CMAXD];
  long long stride[CMAXD];
  const double* grid[CMAXD];                     // device copies of the axis grids
  double lo[CMAXD], inv_step[CMAXD];             // utils.py:11-15: first point, 1 / first spacing
  // next state of dimension d (the reference's next_state):
  //   rho[d] * x[d] + xcoef[d] * x[xdim[d]] + vol_d(x) * eta[d],
  //   vol_d(x) = sconst[d] (voldim[d] < 0)  or  phi[d] * exp(x[voldim[d]])
  double rho[CMAXD], xcoef[CMAXD], sconst[CMAXD], phi[CMAXD];
  int xdim[CMAXD], voldim[CMAXD];
  int zdim, hcdim;                               // the dimensions inside const(x)
  double one_m_gamma, mu_c, phi_c, theta, inv_theta, beta, theta_rho0;
  const double* eta;                             // [D][M] shocks
  const double* wq;                              // [M]  W_m * exp(theta * sconst[0] * eta[0][m])
  double etamax[CMAXD];                          // max_m |eta[d][m]|: bounds the box of next states
  int cap;                                       // LDS doubles available per staged array
  // tensor-product quadrature (M = tq^D, node m = (j_0 .. j_{D-1}), j_0 fastest): tq > 0 enables the
  // pre-contraction of the two fastest dimensions; tstride[d] = tq^d locates the 1-D node j of
  // dimension d at eta[d][j * tstride[d]]; ucap = LDS doubles per pre-contracted array
  int tq, ucap;
  int tstride[CMAXD];
  unsigned tmagic, tmagic2;                      // floor(2^32 / tq) + 1: exact m / tq for m <= 2^24, tq <= 64;
                                                 // floor(2^32 / tq^2) + 1: exact e / tq^2 for e <= ucap <= 4000
};

struct ContIO {
  const double* w;        // iterate (T modes) or linearisation point (JVP)
  const double* v;        // JVP direction
  double* out;
  double* c2_out;         // T_LIN: beta * C * u / Kg
  const double* c2_in;    // JVP
  const double* old;      // T modes: residual against this grid (or null)
  unsigned long long* resid;
  const unsigned long long* gate;
  double gate_tol;
  int minus_identity;
};

// C_EM: the conditional mean of the SDF at the grid function w,
//   E_x[M] = beta^theta (w(x) - 1)^(1 - theta) exp(-gamma (mu_c + z) + gamma^2 sigma_c(x)^2 / 2)
//            * sum_m W_m exp(theta h_lambda'(x, m)) interp(w)(x'(x, m))^(theta - 1)
// -- T's node sum with the exponent theta - 1 on the interpolant, -gamma where T's constant has 1 - gamma, and its own
// epilogue; the box, the pre-contraction and the node loop are T's, so the host's box logic decides its path as it does T's.
//
// C_K0 / C_K1 / C_K2: the tilted expectation K(p, kappa_lambda, kappa_c) f of DESIGN 4.15 for the SDF power p = 0, 1, 2,
//   K f (x) = d2(x) * sum_m Wt_m * interp(w)(x'(x, m))^(p (theta - 1)) * interp(f)(x'(x, m))
// with the tilted node weights Wt_m = W_m exp(kappa_lambda s_lambda eta_0m) in P.wq and the per-point factor d2 (k_cont_tilt_d2)
// in io.c2_in.  p = 1, 2 stage and interpolate w (io.w) and f (io.v) as C_JVP stages w and v, one pow_fast_n per node;
// p = 0 stages f alone (io.w = io.v = f), with T's LDS and no power.  The epilogue is J.v's: out = d2 * e (- f).
// C_K2 takes one power with the exponent 2 (theta - 1): squaring the theta - 1 power measured the same.
//
// C_PTAN: the tangent of T at a fixed w along a direction of the parameters, grids / nodes / weights held fixed:
//   dT(x) = dbeta u + beta u [ (dC/C + de/e) / theta - dtheta ln Kg / theta^2 ],   Kg = C e,  u = Kg^(1/theta),
//   de/e  = sum_m omega_m [ dtheta (s_lambda eta_0m + ln g_m) + theta ds_lambda eta_0m + theta dg_m / g_m ] / e,
//   omega_m = W_m exp(theta s_lambda eta_0m) g_m^theta,  g_m = interp(w)(c(m)),  dg_m = sum_d (d interp(w) / d c_d) dc_d(m),
//   dc_d(m) = da_d + dk_d eta_dm where 0 <= c_d(m) < n_d - 1 and 0 where the coordinate is clamped.
// dg is forward mode on the fold T has (DualRec); T's box, one field staged.  The pre-contracted path keeps the tangent
// of the inner-pair contraction in the second U array (where J.v keeps its direction): cap + 2 ucap doubles of LDS.
// The node sum carries omega and omega * [...], reduced in T's fixed order.  The epilogue also writes T_LIN's c2 (the
// same expressions on the same e: the same bits) and, if asked, T w.
// C_PTANL: C_PTAN with ln g_m taken from the power (pow_log_n below: ln 2 times the log2 g that g^theta forms anyway)
// instead of libm's log: 0.85 - 0.92 of C_PTAN's time (profiles/continuous_sensitivity_times.txt), the host's default.
//
// C_VJP: the transpose of C_JVP at the same linearisation.  io.v = u, io.c2_in = c2, io.w = the linearisation
// point; io.out already holds 0, written in-stream ahead of the launch (cont_vjp.hip, which also subtracts u behind it
// for minus_identity), and the block of x adds
//   out[j] += c2(x) u(x) sum_m W_m g_m(x)^(theta-1) phi_j(x'(x, m)),
// phi_j the multilinear hat weight of corner j: the cell and the t of the forward fold, the staged path's correction of
// t included, so this is the transpose of what C_JVP computes and not of an idealised operator.  Same prologue, box,
// node loop and power as C_JVP; the second array of each LDS pair (box, U) is a zeroed accumulator where C_JVP stages
// its direction.  Pre-contracted path: the node's coefficient is spread over the 2^(D-2) outer corners of the adjoint of
// U; after a barrier the transposed inner-pair contraction carries it into the accumulator box (four cells per entry,
// the forward tt weights); after another the box cells that received something are added to out.  Staged path: the 2^D
// corner weights go to the accumulator box, flushed the same way.  Global path: they go to out directly.
// Every accumulation is a hardware fp64 atomic add (ds_add_f64 / global_atomic_add_f64): THE LAST BITS OF THE RESULT
// DEPEND ON THE ORDER IN WHICH THE ADDS ARRIVE -- the one form of this kernel, and the first call of the library, that
// is reproducible to rounding only.  io.out must be ordinary (coarse-grained) device memory.
enum ContMode { C_T = 0, C_TLIN = 1, C_JVP = 2, C_EM = 3, C_K0 = 4, C_K1 = 5, C_K2 = 6, C_PTAN = 7, C_PTANL = 8, C_VJP = 9 };

// modes that stage and interpolate a second field (io.v) beside io.w
constexpr bool cont_two_fields(int mode) { return mode == C_JVP || mode == C_K1 || mode == C_K2; }

// C_PTAN's request: the direction in the descriptor's own terms (d rho_d, d xcoef_d, d sconst_d, d phi_d per dimension;
// d s_lambda = sconst[0], d rho_lambda = rho[0]) and the optional T w
struct ContTan {
  double rho[CMAXD], xcoef[CMAXD], sconst[CMAXD], phi[CMAXD];
  double gamma, mu_c, phi_c, theta, beta;
  double* Tw;
};
struct ContNoTan {};                             // what the other forms take in its place: nothing
template <int MODE> struct ContTanSel { using type = ContNoTan; };
template <> struct ContTanSel<C_PTAN> { using type = ContTan; };
template <> struct ContTanSel<C_PTANL> { using type = ContTan; };
constexpr bool cont_ptan(int mode) { return mode == C_PTAN || mode == C_PTANL; }
template <int MODE> using ContTanOf = typename ContTanSel<MODE>::type;

// The transpose of InterpRec: coef times the hat weight of every corner, added to f with hardware fp64 atomics.  The
// weights are those of InterpRec's fold, fma(t, v1 - v0, v0) = (1 - t) v0 + t v1; corners of weight zero (a clamped
// coordinate: t = 0 or 1) are skipped.
template <int D, int d, typename Idx>
struct ScatterRec {
  static __device__ __forceinline__ void run(double* __restrict__ f, Idx off, const Idx (&step)[D], const double (&t)[D], double coef) {
    ScatterRec<D, d + 1, Idx>::run(f, off, step, t, coef * (1.0 - t[d]));
    ScatterRec<D, d + 1, Idx>::run(f, off + step[d], step, t, coef * t[d]);
  }
};
template <int D, typename Idx>
struct ScatterRec<D, D, Idx> {
  static __device__ __forceinline__ void run(double* __restrict__ f, Idx off, const Idx (&)[D], const double (&)[D], double coef) {
    if (coef != 0.0) unsafeAtomicAdd(f + off, coef);
  }
};

template <int D, int d, typename Idx>
struct InterpRec {
  static __device__ __forceinline__ double run(const double* __restrict__ f, Idx off,
                                               const Idx (&step)[D], const double (&t)[D]) {
    const double v0 = InterpRec<D, d + 1, Idx>::run(f, off, step, t);
    const double v1 = InterpRec<D, d + 1, Idx>::run(f, off + step[d], step, t);
    return fma(t[d], v1 - v0, v0);
  }
};
template <int D, typename Idx>
struct InterpRec<D, D, Idx> {
  static __device__ __forceinline__ double run(const double* __restrict__ f, Idx off,
                                               const Idx (&)[D], const double (&)[D]) {
    return f[off];
  }
};

// InterpRec in forward mode: (v, dv) with dv = sum_d (dv / dt_d) td[d], plus the leaves' own tangents fd[] when FD.
// v is InterpRec's, operation for operation.
template <int D, int d, typename Idx, bool FD>
struct DualRec {
  static __device__ __forceinline__ void run(const double* __restrict__ f, const double* __restrict__ fd, Idx off,
                                             const Idx (&step)[D], const double (&t)[D], const double (&td)[D],
                                             double& v, double& dv) {
    double v0, v1, d0, d1;
    DualRec<D, d + 1, Idx, FD>::run(f, fd, off, step, t, td, v0, d0);
    DualRec<D, d + 1, Idx, FD>::run(f, fd, off + step[d], step, t, td, v1, d1);
    const double diff = v1 - v0;
    v = fma(t[d], diff, v0);
    if (!FD && d == D - 1) dv = td[d] * diff;                       // (the leaves' tangents are zero)
    else dv = fma(td[d], diff, fma(t[d], d1 - d0, d0));
  }
};
template <int D, typename Idx, bool FD>
struct DualRec<D, D, Idx, FD> {
  static __device__ __forceinline__ void run(const double* __restrict__ f, const double* __restrict__ fd, Idx off,
                                             const Idx (&)[D], const double (&)[D], const double (&)[D], double& v, double& dv) {
    v = f[off];
    dv = FD ? fd[off] : 0.0;
  }
};

// x^y (|y| large: pow_fast_n<true>) together with ln x = ln 2 * log2 x, from the log2 x = hi + lo the power forms: the
// straight-line path of pow_fast_try<true, N> (pass_kernel.hpp), operation for operation, with hi and lo kept.  Anything
// outside that path (a wave with a lane that is no positive normal number, |y log2 x| >= 1020) takes pow_fast_n and log.
#define CONT_FORJ _Pragma("unroll") for (int j = 0; j < N; ++j)
template <int N>
__device__ __forceinline__ void pow_log_n(const double (&x)[N], double y, const PowLane& T, double (&res)[N], double (&lnx)[N]) {
#pragma clang fp contract(off)
  constexpr int OFFH = (int)(POW_OFF >> 32);
  constexpr double SHIFT = 0x1.8p46;
  constexpr double LN2 = 0x1.62e42fefa39efp-1;
  int i4[N], ji[N];
  double kd[N], z[N], invc[N], lchi[N], lclo[N], r[N], t1[N], q[N], hi[N], d[N], e[N], lo[N], ehi[N], elo[N], f[N], t[N], p[N];
  bool rare = false;
  CONT_FORJ {
    const int hx = __double2hiint(x[j]);
    const int tmph = hx - OFFH;
    rare |= !__builtin_amdgcn_class(x[j], 0x100);
    i4[j] = tmph >> 12;
    kd[j] = (double)(tmph >> 20);
    z[j] = __hiloint2double(hx - (tmph & (int)0xfff00000), __double2loint(x[j]));
  }
  CONT_FORJ invc[j] = gather_hib(T.invc, i4[j]);
  CONT_FORJ lchi[j] = gather64b(T.lchi, i4[j]);
  CONT_FORJ lclo[j] = gather_hib(T.lclo, i4[j]);
  CONT_FORJ r[j] = fma(z[j], invc[j], -1.0);
  CONT_FORJ t1[j] = kd[j] + lchi[j];
  CONT_FORJ q[j] = fma_sc(r[j], POW_L8, POW_L7);
  CONT_FORJ q[j] = fma_sc(q[j], r[j], POW_L6);
  CONT_FORJ q[j] = fma_sc(q[j], r[j], POW_L5);
  CONT_FORJ q[j] = fma_sc(q[j], r[j], POW_L4);
  CONT_FORJ q[j] = fma_sc(q[j], r[j], POW_L3);
  CONT_FORJ q[j] = fma_sc(q[j], r[j], POW_L2);
  CONT_FORJ hi[j] = fma(r[j], POW_INVLN2_HI, t1[j]);
  CONT_FORJ d[j] = t1[j] - hi[j];
  CONT_FORJ e[j] = fma(r[j], POW_INVLN2_HI, d[j]);
  CONT_FORJ lo[j] = fma(r[j] * r[j], q[j], e[j] + fma(r[j], POW_INVLN2_LO, lclo[j]));
  CONT_FORJ lnx[j] = fma(hi[j], LN2, lo[j] * LN2);
  CONT_FORJ ehi[j] = y * hi[j];
  CONT_FORJ elo[j] = fma(y, lo[j], fma(y, hi[j], -ehi[j]));
  CONT_FORJ rare |= !(fabs(ehi[j]) < 1020.0);
  CONT_FORJ {
    double kk = ehi[j] + SHIFT;
    ji[j] = __double2loint(kk);
    kk -= SHIFT;
    f[j] = (ehi[j] - kk) + elo[j];
  }
  CONT_FORJ t[j] = gather64b(T.e2t, ji[j] << 2);
  CONT_FORJ p[j] = fma_sc(f[j], POW_E6, POW_E5);
  CONT_FORJ p[j] = fma_sc(p[j], f[j], POW_E4);
  CONT_FORJ p[j] = fma_sc(p[j], f[j], POW_E3);
  CONT_FORJ p[j] = fma_sc(p[j], f[j], POW_E2);
  CONT_FORJ p[j] = fma_sc(p[j], f[j], POW_E1);
  CONT_FORJ {
    const double v = fma(t[j], p[j] * f[j], t[j]);
    res[j] = __hiloint2double(__double2hiint(v) + ((ji[j] >> 6) << 20), __double2loint(v));
  }
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(rare) != 0ULL, 0)) {
    pow_fast_n<true, N>(x, y, T, res);
    CONT_FORJ lnx[j] = log(x[j]);
  }
}
#undef CONT_FORJ

// map_coordinates(order=1, mode='nearest') clips both corner indices into the grid, which equals
// interpolating at the coordinate clipped to [0, n-1]; with the lower corner capped at n-2 the upper
// corner is always the next point (at the top edge t = 1), so corner steps are plain strides and the
// two corners along the fastest axis are adjacent in memory.
template <int D>
__device__ __forceinline__ void interp_cell(const ContDesc& P, const double (&c)[D], int (&i0)[D], double (&t)[D]) {
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double cc = fmin(fmax(c[d], 0.0), (double)(P.n[d] - 1));
    i0[d] = min((int)cc, P.n[d] - 2);
    t[d] = cc - (double)i0[d];
  }
}

template <int D, int MODE>
__global__ void __launch_bounds__(256) cont_kernel(const ContDesc P, const ContIO io, const ContTanOf<MODE> tan) {
  constexpr bool TWO = cont_two_fields(MODE);
  constexpr bool PTAN = cont_ptan(MODE);
  constexpr bool VJP = MODE == C_VJP;
  constexpr int NBOX = (TWO || VJP) ? 2 : 1;     // arrays of each LDS pair: C_VJP's second one is the accumulator
  __shared__ double red[PTAN ? 8 : 4];
  if (io.gate != nullptr) {
    const unsigned long long g = *io.gate;
    if (g <= (unsigned long long)__double_as_longlong(io.gate_tol)) return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p = blockIdx.x;

  // this block's grid point and the affine map node -> next-state coordinates
  double x[D], a[D], k[D];
  [[maybe_unused]] double ad[PTAN ? D : 1], kd[PTAN ? D : 1];    // C_PTAN: the tangents of a and k
  {
    long long r = p;
#pragma unroll
    for (int d = D - 1; d >= 0; --d) {
      const int i = (int)(r % P.n[d]);
      r /= P.n[d];
      x[d] = P.grid[d][i];
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      double mean = P.rho[d] * x[d];
      double vol = P.sconst[d];
#pragma unroll
      for (int e = 0; e < D; ++e) {
        if (P.xdim[d] == e) mean += P.xcoef[d] * x[e];
        if (P.voldim[d] == e) vol = P.phi[d] * exp(x[e]);
      }
      a[d] = (mean - P.lo[d]) * P.inv_step[d];
      k[d] = vol * P.inv_step[d];
      if constexpr (PTAN) {
        double dmean = tan.rho[d] * x[d];
        double dvol = tan.sconst[d];
#pragma unroll
        for (int e = 0; e < D; ++e) {
          if (P.xdim[d] == e) dmean += tan.xcoef[d] * x[e];
          if (P.voldim[d] == e) dvol = tan.phi[d] * exp(x[e]);
        }
        ad[d] = dmean * P.inv_step[d];
        kd[d] = dvol * P.inv_step[d];
      }
    }
  }
  // C_PTAN: the tangent of the coordinate c = a + k eta, zero where map_coordinates clamps it
  [[maybe_unused]] auto ctan = [&](int d, double c, double eta) -> double {
    if constexpr (PTAN) return (c >= 0.0 && c < (double)(P.n[d] - 1)) ? fma(kd[d], eta, ad[d]) : 0.0;
    else return 0.0;
  };

  // box of the grid that holds every next state of this point: [blo, blo + bext) per dimension
  extern __shared__ double box[];
  int blo[D], bext[D], ls[D];
  long long gs[D];
  int V = 1;
  bool staged = true;
#pragma unroll
  for (int d = D - 1; d >= 0; --d) {
    const double span = fabs(k[d]) * P.etamax[d];
    const double hi = (double)(P.n[d] - 1);
    const double cmin = fmin(fmax(a[d] - span, 0.0), hi), cmax = fmin(fmax(a[d] + span, 0.0), hi);
    blo[d] = min((int)cmin, P.n[d] - 2);
    const int bhi = max(blo[d] + 1, min((int)cmax + 1, P.n[d] - 1));
    bext[d] = bhi - blo[d] + 1;
    ls[d] = V;
    gs[d] = P.stride[d];
    if ((long long)V * bext[d] > (long long)P.cap) staged = false;
    V = staged ? V * bext[d] : V;
  }
  if (staged) {
    for (int e = tid; e < V; e += 256) {
      int r = e;
      long long go = 0;
#pragma unroll
      for (int d = D - 1; d >= 0; --d) {
        const int q = r % bext[d];
        r /= bext[d];
        go += (long long)(blo[d] + q) * P.stride[d];
      }
      box[e] = io.w[go];
      if (TWO) box[P.cap + e] = io.v[go];
      if constexpr (VJP) box[P.cap + e] = 0.0;
    }
    __syncthreads();
  }

  // pre-contraction of the two fastest dimensions (tensor rules only)
  constexpr int DO = D - 2;                                      // outer dimensions
  const int tq = P.tq, tq2 = tq * tq;
  const int inner_v = bext[D - 1] * bext[D - 2];
  const int Vo = staged ? V / inner_v : 0;
  const bool tensor = staged && tq > 0 && (long long)Vo * tq2 <= (long long)P.ucap;
  double* const Uw = box + NBOX * P.cap;
  double* const Uv = Uw + P.ucap;
  int lsU[DO > 0 ? DO : 1];
  if (tensor) {
#pragma unroll
    for (int d = 0; d < DO; ++d) lsU[d] = ls[d] / inner_v * tq2;
    for (int e = tid; e < Vo * tq2; e += 256) {
      const int o = (int)__umulhi((unsigned)e, P.tmagic2), jj = e - o * tq2;
      const int ja = (int)__umulhi((unsigned)jj, P.tmagic), jb = jj - ja * tq;
      int il[2];
      double tt[2];
      [[maybe_unused]] double ttd[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int d = D - 2 + q;
        const double eta = P.eta[(long long)d * P.M + (long long)(q ? jb : ja) * P.tstride[d]];
        const double c = fma(k[d], eta, a[d]);
        const double cc = fmin(fmax(c, 0.0), (double)(P.n[d] - 1));
        const int i0 = min((int)cc, P.n[d] - 2);
        il[q] = min(max(i0 - blo[d], 0), bext[d] - 2);
        tt[q] = cc - (double)(blo[d] + il[q]);
        if constexpr (PTAN) ttd[q] = ctan(d, c, eta);
      }
      const int base = o * inner_v + il[0] * ls[D - 2] + il[1];
      {
        const double v0 = fma(tt[1], box[base + 1] - box[base], box[base]);
        const double v1 = fma(tt[1], box[base + ls[D - 2] + 1] - box[base + ls[D - 2]], box[base + ls[D - 2]]);
        Uw[e] = fma(tt[0], v1 - v0, v0);
      }
      if constexpr (VJP) Uv[e] = 0.0;
      if (TWO) {
        const double* bv = box + P.cap;
        const double v0 = fma(tt[1], bv[base + 1] - bv[base], bv[base]);
        const double v1 = fma(tt[1], bv[base + ls[D - 2] + 1] - bv[base + ls[D - 2]], bv[base + ls[D - 2]]);
        Uv[e] = fma(tt[0], v1 - v0, v0);
      }
      if constexpr (PTAN) {                                          // the tangent of Uw[e]: its t's move, the box does not
        const double d0 = box[base + 1] - box[base], d1 = box[base + ls[D - 2] + 1] - box[base + ls[D - 2]];
        const double v0 = fma(tt[1], d0, box[base]), v1 = fma(tt[1], d1, box[base + ls[D - 2]]);
        const double v0d = ttd[1] * d0, v1d = ttd[1] * d1;
        Uv[e] = fma(ttd[0], v1 - v0, fma(tt[0], v1d - v0d, v0d));
      }
    }
    __syncthreads();
  }

  const PowLane PT = pow_lane_init(lane);
  [[maybe_unused]] double cu = 0.0;              // C_VJP: c2(x) u(x)
  if constexpr (VJP) cu = io.c2_in[p] * io.v[p];
  double acc = 0.0;
  [[maybe_unused]] double accl = 0.0;            // (accl: C_PTAN's sum of omega * [...])
  const int trips = (P.M + 255) >> 8;            // uniform: pow_fast_n needs whole waves
  for (int it = 0; it < trips; ++it) {
    const int m = it * 256 + tid;
    const bool valid = m < P.M;
    double g[1] = {1.0}, iv = 0.0, wq = 0.0;
    [[maybe_unused]] double gd = 0.0, eta0 = 0.0;   // C_PTAN: the tangent of g, the node of dimension 0
    [[maybe_unused]] double vt[VJP ? D : 1];        // C_VJP: the t's and the cell of the fold, kept for the scatter
    [[maybe_unused]] long long voff = 0;
    if (valid && tensor) {
      // digits of m in base tq: j_0 fastest; the inner pair selects the column of U
      int r = m, off = 0;
      double to[DO > 0 ? DO : 1];
      [[maybe_unused]] double tod[DO > 0 ? DO : 1];
#pragma unroll
      for (int d = 0; d < DO; ++d) {
        const int rq = (int)__umulhi((unsigned)r, P.tmagic);
        const int j = r - rq * tq;
        r = rq;
        const double eta = P.eta[(long long)d * P.M + (long long)j * P.tstride[d]];
        const double c = fma(k[d], eta, a[d]);
        const double cc = fmin(fmax(c, 0.0), (double)(P.n[d] - 1));
        const int i0 = min((int)cc, P.n[d] - 2);
        const int il = min(max(i0 - blo[d], 0), bext[d] - 2);
        to[d] = cc - (double)(blo[d] + il);
        off += il * lsU[d];
        if constexpr (PTAN) { tod[d] = ctan(d, c, eta); if (d == 0) eta0 = eta; }
      }
      const int jb = (int)__umulhi((unsigned)r, P.tmagic), ja = r - jb * tq;   // j_{D-1}, j_{D-2}
      off += ja * tq + jb;
      if constexpr (PTAN) DualRec<DO, 0, int, true>::run(Uw, Uv, off, lsU, to, tod, g[0], gd);
      else g[0] = InterpRec<DO, 0, int>::run(Uw, off, lsU, to);
      if (TWO) iv = InterpRec<DO, 0, int>::run(Uv, off, lsU, to);
      if constexpr (VJP) {
        voff = off;
#pragma unroll
        for (int d = 0; d < DO; ++d) vt[d] = to[d];
      }
      wq = P.wq[m];
    } else if (valid) {
      double c[D], t[D];
      [[maybe_unused]] double td[D];
      int i0[D];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double eta = P.eta[(long long)d * P.M + m];
        c[d] = fma(k[d], eta, a[d]);
        if constexpr (PTAN) { td[d] = ctan(d, c[d], eta); if (d == 0) eta0 = eta; }
      }
      interp_cell<D>(P, c, i0, t);
      if (staged) {
        int off = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          // rounding in the bound above can leave a coordinate a hair outside the box: keep the
          // cell inside (the interpolant is then evaluated a rounding error outside its cell)
          const int il = min(max(i0[d] - blo[d], 0), bext[d] - 2);
          t[d] += (double)(i0[d] - blo[d] - il);
          off += il * ls[d];
        }
        if constexpr (PTAN) DualRec<D, 0, int, false>::run(box, nullptr, off, ls, t, td, g[0], gd);
        else g[0] = InterpRec<D, 0, int>::run(box, off, ls, t);
        if (TWO) iv = InterpRec<D, 0, int>::run(box + P.cap, off, ls, t);
        if constexpr (VJP) voff = off;
      } else {
        long long off = 0;
#pragma unroll
        for (int d = 0; d < D; ++d) off += (long long)i0[d] * P.stride[d];
        if constexpr (PTAN) DualRec<D, 0, long long, false>::run(io.w, nullptr, off, gs, t, td, g[0], gd);
        else g[0] = InterpRec<D, 0, long long>::run(io.w, off, gs, t);
        if (TWO) iv = InterpRec<D, 0, long long>::run(io.v, off, gs, t);
        if constexpr (VJP) voff = off;
      }
      if constexpr (VJP) {
#pragma unroll
        for (int d = 0; d < D; ++d) vt[d] = t[d];
      }
      wq = P.wq[m];
    }
    if (MODE == C_K0) {
      acc = fma(wq, g[0], acc);                                      // Wt interp(f): no power
      continue;
    }
    double pw[1];
    [[maybe_unused]] double lg[1];
    if constexpr (MODE == C_PTANL) pow_log_n<1>(g, P.theta, PT, pw, lg);
    else pow_fast_n<true, 1>(g, MODE == C_K2 ? 2.0 * (P.theta - 1.0) : (MODE == C_EM || MODE == C_K1 ? P.theta - 1.0 : P.theta), PT, pw);
    if constexpr (MODE == C_PTAN) lg[0] = log(g[0]);
    if constexpr (VJP) {
      // c2 u W g^(theta-1) onto the corners the forward fold read, with its weights
      if (valid) {
        const double coef = cu * (wq * (pw[0] / g[0]));
        if (tensor) {
          double to[DO > 0 ? DO : 1];
#pragma unroll
          for (int d = 0; d < DO; ++d) to[d] = vt[d];
          ScatterRec<DO, 0, int>::run(Uv, (int)voff, lsU, to, coef);
        } else if (staged) {
          ScatterRec<D, 0, int>::run(box + P.cap, (int)voff, ls, vt, coef);
        } else {
          ScatterRec<D, 0, long long>::run(io.out, voff, gs, vt, coef);
        }
      }
      continue;
    }
    if (MODE == C_JVP) acc = fma(wq * (pw[0] / g[0]), iv, acc);      // W g^(theta-1) interp(v)
    else if (MODE == C_K1 || MODE == C_K2) acc = fma(wq * pw[0], iv, acc);   // Wt g^(p (theta-1)) interp(f)
    else acc = fma(wq, pw[0], acc);
    if constexpr (PTAN) {
      // dtheta (s_lambda eta_0 + ln g) + theta ds_lambda eta_0 + theta dg / g
      const double L = fma(tan.theta, fma(P.sconst[0], eta0, lg[0]), P.theta * fma(tan.sconst[0], eta0, gd / g[0]));
      accl = fma(wq * pw[0], L, accl);
    }
  }
  if constexpr (VJP) {
    if (!staged) return;                         // (block-uniform: the global path has added to out already)
    __syncthreads();
    double* const ab = box + P.cap;              // the accumulator box
    if (tensor) {
      // the transposed inner-pair contraction: every adjoint entry of U feeds the four box cells its forward entry read
      for (int e = tid; e < Vo * tq2; e += 256) {
        const double ua = Uv[e];
        if (ua == 0.0) continue;
        const int o = (int)__umulhi((unsigned)e, P.tmagic2), jj = e - o * tq2;
        const int ja = (int)__umulhi((unsigned)jj, P.tmagic), jb = jj - ja * tq;
        int il[2];
        double tt[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int d = D - 2 + q;
          const double eta = P.eta[(long long)d * P.M + (long long)(q ? jb : ja) * P.tstride[d]];
          const double c = fma(k[d], eta, a[d]);
          const double cc = fmin(fmax(c, 0.0), (double)(P.n[d] - 1));
          const int i0 = min((int)cc, P.n[d] - 2);
          il[q] = min(max(i0 - blo[d], 0), bext[d] - 2);
          tt[q] = cc - (double)(blo[d] + il[q]);
        }
        const int base = o * inner_v + il[0] * ls[D - 2] + il[1];
        const double u0 = ua * (1.0 - tt[0]), u1 = ua * tt[0];
        const double c00 = u0 * (1.0 - tt[1]), c01 = u0 * tt[1], c10 = u1 * (1.0 - tt[1]), c11 = u1 * tt[1];
        if (c00 != 0.0) unsafeAtomicAdd(ab + base, c00);
        if (c01 != 0.0) unsafeAtomicAdd(ab + base + 1, c01);
        if (c10 != 0.0) unsafeAtomicAdd(ab + base + ls[D - 2], c10);
        if (c11 != 0.0) unsafeAtomicAdd(ab + base + ls[D - 2] + 1, c11);
      }
      __syncthreads();
    }
    // the box cells that received something, added to out at the box's global offsets
    for (int e = tid; e < V; e += 256) {
      const double val = ab[e];
      if (val == 0.0) continue;
      int r = e;
      long long go = 0;
#pragma unroll
      for (int d = D - 1; d >= 0; --d) {
        const int q = r % bext[d];
        r /= bext[d];
        go += (long long)(blo[d] + q) * P.stride[d];
      }
      unsafeAtomicAdd(io.out + go, val);
    }
    return;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if constexpr (PTAN) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) accl += __shfl_xor(accl, o);
  }
  if (lane == 0) {
    red[wave] = acc;
    if constexpr (PTAN) red[4 + wave] = accl;
  }
  __syncthreads();
  if (wave != 0) return;
  const double e = (red[0] + red[1]) + (red[2] + red[3]);

  if (TWO || MODE == C_K0) {
    if (lane == 0) {
      double r = io.c2_in[p] * e;
      if (io.minus_identity) r -= io.v[p];
      io.out[p] = r;
    }
    return;
  }
  double zval = 0.0, hcval = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (P.zdim == d) zval = x[d];
    if (P.hcdim == d) hcval = x[d];
  }
  const double sig_c = P.phi_c * exp(hcval);
  if (MODE == C_EM) {
    if (lane == 0) {
      const double gam = 1.0 - P.one_m_gamma, wx = io.w[p];          // (the descriptor carries 1 - gamma)
      const double lc = P.theta * log(P.beta) - gam * (P.mu_c + zval) + 0.5 * gam * gam * sig_c * sig_c + P.theta_rho0 * x[0];
      io.out[p] = wx > 1.0 ? exp(lc) * pow(wx - 1.0, 1.0 - P.theta) * e : __builtin_nan("");
    }
    return;
  }
  const double C = exp(P.one_m_gamma * (P.mu_c + zval) + 0.5 * P.one_m_gamma * P.one_m_gamma * sig_c * sig_c)
                   * exp(P.theta_rho0 * x[0]);
  const double Kg[1] = {C * e};
  double u[1];
  pow_fast_n<false, 1>(Kg, P.inv_theta, PT, u);                       // every lane of wave 0, same value
  if constexpr (PTAN) {
    if (lane == 0) {
      const double el = (red[4] + red[5]) + (red[6] + red[7]);
      const double omg = P.one_m_gamma, rho0 = P.rho[0];
      const double ln_c = omg * (P.mu_c + zval) + 0.5 * omg * omg * sig_c * sig_c + P.theta_rho0 * x[0];
      const double dsig_c = tan.phi_c * exp(hcval);
      const double dln_c = omg * tan.mu_c - tan.gamma * (P.mu_c + zval) + omg * sig_c * (omg * dsig_c - tan.gamma * sig_c) +
                           (tan.theta * rho0 + P.theta * tan.rho[0]) * x[0];
      const double ln_kg = ln_c + log(e);
      const double bu = P.beta * u[0];
      io.out[p] = tan.beta * u[0] + bu * ((dln_c + el / e) * P.inv_theta - tan.theta * ln_kg * P.inv_theta * P.inv_theta);
      io.c2_out[p] = P.beta * C * u[0] / Kg[0];                       // (T_LIN's expression on T_LIN's e)
      if (tan.Tw != nullptr) tan.Tw[p] = 1.0 + P.beta * u[0];
    }
    return;
  }
  if (lane == 0) {
    const double tw = 1.0 + P.beta * u[0];
    io.out[p] = tw;
    if (MODE == C_TLIN) io.c2_out[p] = P.beta * C * u[0] / Kg[0];
    if (io.resid != nullptr) {
      double r = fabs(tw - io.old[p]);
      if (!(r == r)) r = __longlong_as_double(0x7ff0000000000000LL);
      const unsigned long long rb = (unsigned long long)__double_as_longlong(r);
      if (rb > *(volatile unsigned long long*)io.resid) atomicMax(io.resid, rb);   // stale read only skips no-ops
    }
  }
}

// lin_interp(x, fun_vals, grids) of code/utils.py:18-23 at n query points, x laid out [D][n]
template <int D>
__global__ void __launch_bounds__(256) lin_interp_kernel(const ContDesc P, const double* __restrict__ f,
                                                         const double* __restrict__ xq, long long nq,
                                                         double* __restrict__ out) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  double c[D], t[D];
  int i0[D];
  long long gs[D], off = 0;
#pragma unroll
  for (int d = 0; d < D; ++d) c[d] = (xq[(long long)d * nq + q] - P.lo[d]) * P.inv_step[d];
  interp_cell<D>(P, c, i0, t);
#pragma unroll
  for (int d = 0; d < D; ++d) { gs[d] = P.stride[d]; off += (long long)i0[d] * P.stride[d]; }
  out[q] = InterpRec<D, 0, long long>::run(f, off, gs, t);
}

}  // namespace sdfs

// cont_sim.hpp -- simulated paths of the continuous-state model at w* (sdfs_cont_sim_records_dev,
// sdfs_cont_sim_paths_dev) and, further down, their claim form (sdfs_cont_sim_claim_*_dev).
//
// Not a header of its own: sdfs_api.hip includes it once, after the single-problem API, and it uses sdfs_handle,
// launch_kernel, Counter, check and fail of that file.
//
// k_cont_sim_records writes one 16-byte record {w, -ln E_x[M]} per grid point, so that a corner of the multilinear
// interpolation is one 16-byte load and the two corners along the fastest axis are 32 contiguous bytes.
// k_cont_sim_paths runs one path per lane, fp64: per step two Philox4x32-10 blocks (counter (t, p, b, 1): the last
// word keeps these streams apart from the discretised simulator's), Box-Muller normals, the reference's next_state
// (the coefficients of ContDesc), interp_cell's clamped cell, the 2^D-corner fold of both record fields, the series of
// DESIGN 4.14 and the shifted one-pass sums of sim_kernels.hpp (SimAcc / sim_acc).
//
// The fold.  The corner set of a state is never live as a whole: the GD fastest dimensions (2^GD corners, loaded
// together, folded in registers in InterpRec's order) form a group, and the D - GD outer dimensions are loops that the
// compiler is told not to unroll, each keeping the result of its lower half while the upper half is formed.  The nesting
// of the fused multiply-adds is InterpRec's, so an interpolated value has the bits lin_interp_kernel gives.
// The look-ahead.  The state recursion reads no record, so K states are advanced first and their folds run side by side:
// K * 2^GD loads of 16 bytes are in flight per lane.  Every state is interpolated once; it serves as x_t and then as
// x_{t-1}.  No atomics, no LDS, no barrier, no host synchronisation: a path's output depends only on its number, the
// seed, the step offset, its start and the model, and two runs give identical bits.  The arithmetic of a step is
// written with explicit fma() under `fp contract(off)`, so that the copies of it the compiler makes (first step, chunk
// loop, every K) round alike: a run of 100 steps equals a run of 40 continued by one of 60.
#pragma once

#include <hip/hip_runtime.h>

#include "cont_kernel.hpp"
#include "sim_kernels.hpp"

extern "C++" {
namespace sdfs {

constexpr int CSIM_BLOCK = 256;
constexpr int CSIM_NSER = 6;                 // dc m rf rc xc wc

struct ContSimArgs {
  unsigned key0, key1;
  unsigned step0;                            // s0: step s0 + k is the k-th step of the run
  unsigned burn_in, n_periods;               // B, T
  int start_mode;                            // 0: the zero state, 1: start[] for every path, 2: start_dev[path][D]
  unsigned long long path0;
  long long n_paths;
  double start[CMAXD];
  const double* start_dev;
  double theta, theta_ln_beta, gamma;
};

struct ContSimNormals { double eta[CMAXD]; double xi; };

// (r_a, r_b) -> sqrt(-2 ln u) (cos phi, sin phi), u = (r_a + 0.5) 2^-32, phi = 2 pi r_b 2^-32
template <bool BOTH>
__device__ __forceinline__ void csim_pair(unsigned ra, unsigned rb, double& c, double& s) {
  const double rad = sqrt(-2.0 * log(sim_u(ra)));
  const double phi = 2.0 * M_PI * ((double)rb * 0x1p-32);
  if (BOTH) {
    double sn, cs;
    sincos(phi, &sn, &cs);
    c = rad * cs; s = rad * sn;
  } else {
    c = rad * cos(phi); s = 0.0;
  }
}

// the normals of step t of path p: eta_d = n_d (d < D), xi = n_D; no normal is formed that is not used
template <int D, bool XI>
__device__ __forceinline__ void csim_normals(const ContSimArgs& a, unsigned t, unsigned p, ContSimNormals& n) {
  static_assert(D == 4 || D == 6, "SSY (4-D) or GCY (6-D)");
  const SimWords b0 = sim_philox(t, p, 0u, 1u, a.key0, a.key1);
  csim_pair<true>(b0.r[0], b0.r[1], n.eta[0], n.eta[1]);
  csim_pair<true>(b0.r[2], b0.r[3], n.eta[2], n.eta[3]);
  n.xi = 0.0;
  if (D == 6 || XI) {
    const SimWords b1 = sim_philox(t, p, 1u, 1u, a.key0, a.key1);
    double unused;
    if (D == 6) {
      csim_pair<true>(b1.r[0], b1.r[1], n.eta[4], n.eta[5]);
      if (XI) csim_pair<false>(b1.r[2], b1.r[3], n.xi, unused);
    } else {
      n.eta[4] = 0.0; n.eta[5] = 0.0;
      if (XI) csim_pair<false>(b1.r[0], b1.r[1], n.xi, unused);
    }
  } else {
    n.eta[4] = 0.0; n.eta[5] = 0.0;
  }
}

// x <- next_state(x, eta): rho_d x_d + xcoef_d x_{xdim(d)} + vol_d(x) eta_d, vol_d = sconst_d or phi_d exp(x_{voldim(d)})
template <int D>
__device__ __forceinline__ void csim_next(const ContDesc& P, double (&x)[D], const ContSimNormals& n) {
#pragma clang fp contract(off)
  double y[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    double mean = P.rho[d] * x[d];
    double vol = P.sconst[d];
#pragma unroll
    for (int e = 0; e < D; ++e) {
      if (P.xdim[d] == e) mean = mean + P.xcoef[d] * x[e];
      if (P.voldim[d] == e) vol = P.phi[d] * exp(x[e]);
    }
    y[d] = mean + vol * n.eta[d];
  }
#pragma unroll
  for (int d = 0; d < D; ++d) x[d] = y[d];
}

// what the series need of one state besides its two interpolated fields
template <int D>
struct ContSimState {
  double hl, muz, sc;                        // h_lambda, mu_c + z, phi_c exp(h_c)
  double t[D];                               // interp_cell: offsets inside the cell
  unsigned off;                              // ... and the flat index of its lowest corner
  bool out;                                  // some coordinate lies outside the grid
};

template <int D>
__device__ __forceinline__ void csim_locate(const ContDesc& P, const double (&x)[D], ContSimState<D>& s) {
  double c[D];
  int i0[D];
  double zval = 0.0, hcval = 0.0;
  bool out = false;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    c[d] = (x[d] - P.lo[d]) * P.inv_step[d];
    out = out || c[d] < 0.0 || c[d] > (double)(P.n[d] - 1);
    if (P.zdim == d) zval = x[d];
    if (P.hcdim == d) hcval = x[d];
  }
  interp_cell<D>(P, c, i0, s.t);             // 0 <= i0[d] <= n[d] - 2 whatever c is (NaN included): every corner is in the grid
  unsigned off = 0;
#pragma unroll
  for (int d = 0; d < D; ++d) off += (unsigned)i0[d] * (unsigned)P.stride[d];
  s.off = off; s.out = out;
  s.hl = x[0]; s.muz = P.mu_c + zval; s.sc = P.phi_c * exp(hcval);
}

__device__ __forceinline__ double2 csim_lerp(double t, const double2 v0, const double2 v1) {
  return make_double2(fma(t, v1.x - v0.x, v0.x), fma(t, v1.y - v0.y, v0.y));
}
// (the fourth word of a claim record is padding)
__device__ __forceinline__ double4 csim_lerp(double t, const double4 v0, const double4 v1) {
  return make_double4(fma(t, v1.x - v0.x, v0.x), fma(t, v1.y - v0.y, v0.y), fma(t, v1.z - v0.z, v0.z), 0.0);
}

// {w, rf}(x) for KK states side by side: dimensions below D - GD are loops, the GD fastest one group of loads
// (V: double2 for the records; the claim form folds its own record type)
template <int D, int GD, int KK, int d, class V>
__device__ __forceinline__ void csim_fold(const V* __restrict__ rec, const unsigned (&step)[D],
                                          const ContSimState<D> (&s)[KK], const unsigned (&off)[KK], V (&r)[KK]) {
  if constexpr (d == D) {
#pragma unroll
    for (int j = 0; j < KK; ++j) r[j] = rec[off[j]];
  } else {
    V v0[KK], v1[KK];
    if constexpr (d >= D - GD) {
      unsigned o1[KK];
#pragma unroll
      for (int j = 0; j < KK; ++j) o1[j] = off[j] + step[d];
      csim_fold<D, GD, KK, d + 1>(rec, step, s, off, v0);
      csim_fold<D, GD, KK, d + 1>(rec, step, s, o1, v1);
    } else {
#pragma unroll 1
      for (int b = 0; b < 2; ++b) {
        unsigned o[KK];
        V q[KK];
#pragma unroll
        for (int j = 0; j < KK; ++j) o[j] = off[j] + (b ? step[d] : 0u);
        csim_fold<D, GD, KK, d + 1>(rec, step, s, o, q);
#pragma unroll
        for (int j = 0; j < KK; ++j) {
          if (b == 0) v0[j] = q[j];
          v1[j] = q[j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < KK; ++j) r[j] = csim_lerp(s[j].t[d], v0[j], v1[j]);
  }
}

// fields of x_{t-1} a step needs
struct ContSimPrev { double lw1, rf, muz, sc; };

template <int D, int GD, int K, bool STORE>
__global__ void __launch_bounds__(CSIM_BLOCK)
k_cont_sim_paths(const ContDesc P, const ContSimArgs a, const double2* __restrict__ rec, double* __restrict__ stats,
                 unsigned* __restrict__ clamped, double* __restrict__ final_state, double* __restrict__ st_out,
                 double* __restrict__ ser_out) {
  static_assert(GD >= 1 && GD < D, "a group is a proper part of the corner set");
  const long long pl = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pl >= a.n_paths) return;               // (no barrier below)
  const unsigned p = (unsigned)(a.path0 + (unsigned long long)pl);
  const unsigned T = a.n_periods, B = a.burn_in, s0 = a.step0;
  unsigned step[D];
#pragma unroll
  for (int d = 0; d < D; ++d) step[d] = (unsigned)P.stride[d];

  // x_0, then the burn-in
  double x[D];
#pragma unroll
  for (int d = 0; d < D; ++d)
    x[d] = a.start_mode == 0 ? 0.0 : (a.start_mode == 1 ? a.start[d] : a.start_dev[(size_t)pl * D + d]);
  ContSimNormals nm;
  for (unsigned k = 1; k <= B; ++k) {
    csim_normals<D, false>(a, s0 + k, p, nm);
    csim_next<D>(P, x, nm);
  }

  auto store_state = [&](unsigned t) {       // x_{B + t}
    if (STORE) {
#pragma unroll
      for (int d = 0; d < D; ++d) st_out[((size_t)pl * (T + 1) + t) * D + d] = x[d];
    }
  };

  // x_B: the previous state of the first recorded step
  ContSimPrev pr;
  {
    ContSimState<D> s1[1];
    unsigned o1[1];
    double2 r1[1];
    csim_locate<D>(P, x, s1[0]);
    o1[0] = s1[0].off;
    csim_fold<D, GD, 1, 0>(rec, step, s1, o1, r1);
    pr.lw1 = log(r1[0].x - 1.0); pr.rf = r1[0].y; pr.muz = s1[0].muz; pr.sc = s1[0].sc;
    store_state(0u);
  }

  SimAcc acc[CSIM_NSER];
  double sx = 0.0, sxx = 0.0, sxy = 0.0, x0 = 0.0;
  unsigned nout = 0;

  // the series of recorded step number t (1 ... T) from x_{t-1} (pr) and x_t (s, its fields r), xi = the step's draw
  auto consume = [&](auto first_tag, const ContSimState<D>& s, const double2 r, double xi, unsigned t) {
#pragma clang fp contract(off)
    constexpr bool FIRST = decltype(first_tag)::value;
    const double lw = log(r.x);
    const double dc = fma(pr.sc, xi, pr.muz);
    const double rl = lw - pr.lw1;
    const double m = fma(a.theta - 1.0, rl, fma(-a.gamma, dc, fma(a.theta, s.hl, a.theta_ln_beta)));
    const double rc = dc + rl;
    const double v[CSIM_NSER] = {dc, m, pr.rf, rc, rc - pr.rf, r.x};
#pragma unroll
    for (int k = 0; k < CSIM_NSER; ++k) sim_acc<FIRST>(acc[k], v[k]);
    // slope: xc_t on ln(w(x_{t-1}) - 1)
    if (FIRST) {
      x0 = pr.lw1;
    } else {
      const double dx = pr.lw1 - x0, dy = acc[4].pv;
      sx += dx;
      sxx = fma(dx, dx, sxx);
      sxy = fma(dx, dy, sxy);
    }
    nout += s.out ? 1u : 0u;
    if (STORE) {
#pragma unroll
      for (int k = 0; k < CSIM_NSER; ++k) ser_out[((size_t)k * a.n_paths + pl) * T + (t - 1)] = v[k];
    }
    pr.lw1 = log(r.x - 1.0); pr.rf = r.y; pr.muz = s.muz; pr.sc = s.sc;
  };

  // recorded steps t ... t + KK - 1: advance, fold side by side, consume
  auto chunk = [&](auto first_tag, auto kk_tag, unsigned t) {
    constexpr int KK = decltype(kk_tag)::value;
    ContSimState<D> s[KK];
    unsigned o[KK];
    double2 r[KK];
    double xi[KK];
#pragma unroll
    for (int j = 0; j < KK; ++j) {
      if (t + j <= T) {                      // (uniform) past the end the slot repeats x_T and is not consumed
        csim_normals<D, true>(a, s0 + B + t + j, p, nm);
        csim_next<D>(P, x, nm);
        store_state(t + j);
      }
      xi[j] = nm.xi;
      csim_locate<D>(P, x, s[j]);
      o[j] = s[j].off;
    }
    csim_fold<D, GD, KK, 0>(rec, step, s, o, r);
#pragma unroll
    for (int j = 0; j < KK; ++j) {
      if (j == 0) consume(first_tag, s[0], r[0], xi[0], t);
      else if (t + j <= T) consume(std::false_type{}, s[j], r[j], xi[j], t + j);
    }
  };

  chunk(std::true_type{}, std::integral_constant<int, 1>{}, 1u);
  for (unsigned t = 2; t <= T; t += K) chunk(std::false_type{}, std::integral_constant<int, K>{}, t);

  // statistics: mean, std, ac1 per series (d = s - s_first, so d_1 = 0), then the slope
  const double Tn = (double)T;
#pragma unroll
  for (int k = 0; k < CSIM_NSER; ++k) {
    const SimAcc& c = acc[k];
    const double mt = c.s1 / Tn;
    const double den = c.s2 - c.s1 * mt;
    const double num = c.sl - mt * (2.0 * c.s1 - c.pv) + (Tn - 1.0) * mt * mt;
    stats[(size_t)(3 * k + 0) * a.n_paths + pl] = c.s0 + mt;
    stats[(size_t)(3 * k + 1) * a.n_paths + pl] = sqrt(fmax(den, 0.0) / Tn);
    stats[(size_t)(3 * k + 2) * a.n_paths + pl] = den > 0.0 ? num / den : __builtin_nan("");
  }
  const double sy = acc[4].s1;
  const double dxx = sxx - sx * (sx / Tn), dxy = sxy - sx * (sy / Tn);
  stats[(size_t)(3 * CSIM_NSER) * a.n_paths + pl] = dxx > 0.0 ? dxy / dxx : __builtin_nan("");
  clamped[pl] = nout;
#pragma unroll
  for (int d = 0; d < D; ++d) final_state[(size_t)pl * D + d] = x[d];
}

__global__ void __launch_bounds__(CSIM_BLOCK)
k_cont_sim_records(long long n, const double* __restrict__ w, const double* __restrict__ em, double2* __restrict__ rec) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    rec[i] = make_double2(w[i], -log(em[i]));
}

// -- the claim form (sdfs_cont_sim_claim_*_dev) ------------------------------------------------------------
// k_cont_sim_paths with a third interpolated field v, the price-dividend ratio of a claim on G_c^kappa, and its series
//   rd_t = kappa dc_t + ln(1 + v(x_t)) - ln v(x_{t-1}),  xd_t = rd_t - rf_t,  pd_t = ln v(x_t);
// the slope is that of xd_t on pd_{t-1}.  A kernel of its own, so that k_cont_sim_paths stays the code it was; what the
// two share is csim_normals, csim_next, csim_locate, csim_fold and sim_acc, and a base series has the plain form's bits.
// Nine series of five sums do not fit beside the normals' sincos in the 256 registers of two waves per SIMD, so the
// claim form carries less from step to step than the plain form would:
//   dc is formed from x_{t-1} as soon as xi is drawn, before the state advances (mu_c + z and phi_c exp(h_c) are not carried);
//   xc and xd are shifted by the difference of their terms' shifts, which is their first value bit for bit;
//   pd_{t-1} - pd_1 is both the previous shifted pd and the slope's regressor, so the regressor's sums are pd's own,
//   corrected at the ends (csim_claim_finish);
//   the storing form keeps no sums at all: it writes the series and then reads its own back in step order.
constexpr int CSIM_NSER_CLAIM = 9;           // dc m rf rc xc wc rd xd pd
constexpr int csim_claim_gd_default(int) { return 3; }   // groups of 8 corners in 4-D and in 6-D (the A/B of DESIGN 4.18)

// the sums of the nine series and of the slope; s0 of xc and xd and pv of pd are formed where they are used
struct ContSimClaimSums {
  SimAcc acc[CSIM_NSER_CLAIM];
  double sxy, dp0;                           // sum of (pd_{t-1} - pd_1)(xd_t - xd_1); pd_0 - pd_1
};

// step t's nine values v, pd_{t-1} = lvp
template <bool FIRST>
__device__ __forceinline__ void csim_claim_acc(ContSimClaimSums& c, const double (&v)[CSIM_NSER_CLAIM], double lvp) {
#pragma clang fp contract(off)
  if (!FIRST) {
    c.acc[4].s0 = c.acc[3].s0 - c.acc[2].s0;
    c.acc[7].s0 = c.acc[6].s0 - c.acc[2].s0;
    c.acc[8].pv = lvp - c.acc[8].s0;
  }
  const double dx = FIRST ? 0.0 : c.acc[8].pv;
#pragma unroll
  for (int k = 0; k < CSIM_NSER_CLAIM; ++k) sim_acc<FIRST>(c.acc[k], v[k]);
  if (FIRST) { c.sxy = 0.0; c.dp0 = lvp - v[8]; }
  else c.sxy = fma(dx, c.acc[7].pv, c.sxy);
}

__device__ __forceinline__ void csim_claim_finish(const ContSimClaimSums& c, unsigned T, long long n_paths, long long pl,
                                                  double* __restrict__ stats) {
  const double Tn = (double)T;
#pragma unroll
  for (int k = 0; k < CSIM_NSER_CLAIM; ++k) {
    const SimAcc& a = c.acc[k];
    const double s0 = k == 4 ? c.acc[3].s0 - c.acc[2].s0 : (k == 7 ? c.acc[6].s0 - c.acc[2].s0 : a.s0);
    const double mt = a.s1 / Tn;
    const double den = a.s2 - a.s1 * mt;
    const double num = a.sl - mt * (2.0 * a.s1 - a.pv) + (Tn - 1.0) * mt * mt;
    stats[(size_t)(3 * k + 0) * n_paths + pl] = s0 + mt;
    stats[(size_t)(3 * k + 1) * n_paths + pl] = sqrt(fmax(den, 0.0) / Tn);
    stats[(size_t)(3 * k + 2) * n_paths + pl] = den > 0.0 ? num / den : __builtin_nan("");
  }
  // the regressor pd_{t-1} - pd_1, t = 1 ... T: dp0, then pd's shifted values but the last
  const SimAcc& q = c.acc[8];
  const double sx = c.dp0 + (q.s1 - q.pv), sxx = fma(c.dp0, c.dp0, q.s2 - q.pv * q.pv);
  const double sy = c.acc[7].s1;
  const double dxx = sxx - sx * (sx / Tn), dxy = c.sxy - sx * (sy / Tn);
  stats[(size_t)(3 * CSIM_NSER_CLAIM) * n_paths + pl] = dxx > 0.0 ? dxy / dxx : __builtin_nan("");
}

// waves per SIMD the register allocation is held to: the plain form's two, but one where the 6-D form keeps its sums
// in registers, which at two waves spills
constexpr int csim_claim_waves(int D, bool store) { return D == 4 || store ? 2 : 1; }

// rec: one 32-byte record {w, -ln E_x[M], v, 0} per grid point (k_cont_sim_claim_records), a corner one 32-byte load
template <int D, int GD, bool STORE>
__global__ void __launch_bounds__(CSIM_BLOCK) __attribute__((amdgpu_waves_per_eu(csim_claim_waves(D, STORE), 2)))
k_cont_sim_claim_paths(const ContDesc P, const ContSimArgs a, const double4* __restrict__ rec, const double kappa,
                       double* __restrict__ stats, unsigned* __restrict__ clamped, double* __restrict__ final_state,
                       double* __restrict__ st_out, double* ser_out) {
  static_assert(GD >= 1 && GD < D, "a group is a proper part of the corner set");
  const long long pl = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pl >= a.n_paths) return;               // (no barrier below)
  const unsigned p = (unsigned)(a.path0 + (unsigned long long)pl);
  const unsigned T = a.n_periods, B = a.burn_in, s0 = a.step0;
  unsigned step[D];
#pragma unroll
  for (int d = 0; d < D; ++d) step[d] = (unsigned)P.stride[d];

  double x[D];
#pragma unroll
  for (int d = 0; d < D; ++d)
    x[d] = a.start_mode == 0 ? 0.0 : (a.start_mode == 1 ? a.start[d] : a.start_dev[(size_t)pl * D + d]);
  ContSimNormals nm;
  for (unsigned k = 1; k <= B; ++k) {
    csim_normals<D, false>(a, s0 + k, p, nm);
    csim_next<D>(P, x, nm);
  }

  auto store_state = [&](unsigned t) {       // x_{B + t}
    if (STORE) {
#pragma unroll
      for (int d = 0; d < D; ++d) st_out[((size_t)pl * (T + 1) + t) * D + d] = x[d];
    }
  };
  auto fields = [&](ContSimState<D> (&s)[1]) {       // {w, rf, v, .}(x)
    unsigned o[1];
    double4 r[1];
    csim_locate<D>(P, x, s[0]);
    o[0] = s[0].off;
    csim_fold<D, GD, 1, 0>(rec, step, s, o, r);
    return r[0];
  };

  // x_B: the previous state of the first recorded step
  double lw1, rf, lv;
  {
    ContSimState<D> s[1];
    const double4 r = fields(s);
    lw1 = log(r.x - 1.0); rf = r.y; lv = log(r.z);
    store_state(0u);
  }
  const double pd0 = lv;

  ContSimClaimSums sums;
  unsigned nout = 0;

  // recorded step t (1 ... T): draw, dc from x_{t-1}, advance, interpolate at x_t, the nine values
  auto record = [&](auto first_tag, unsigned t) {
#pragma clang fp contract(off)
    constexpr bool FIRST = decltype(first_tag)::value;
    csim_normals<D, true>(a, s0 + B + t, p, nm);
    double zval = 0.0, hcval = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (P.zdim == d) zval = x[d];
      if (P.hcdim == d) hcval = x[d];
    }
    const double muz = P.mu_c + zval, sc = P.phi_c * exp(hcval);       // (csim_locate's, at x_{t-1})
    const double dc = fma(sc, nm.xi, muz);
    csim_next<D>(P, x, nm);
    store_state(t);
    ContSimState<D> s[1];
    const double4 r = fields(s);
    const double lw = log(r.x), lvt = log(r.z), l1v = log(1.0 + r.z);
    const double rl = lw - lw1;
    const double m = fma(a.theta - 1.0, rl, fma(-a.gamma, dc, fma(a.theta, s[0].hl, a.theta_ln_beta)));
    const double rc = dc + rl;
    const double rd = fma(kappa, dc, l1v - lv);
    const double v[CSIM_NSER_CLAIM] = {dc, m, rf, rc, rc - rf, r.x, rd, rd - rf, lvt};
    nout += s[0].out ? 1u : 0u;
    if (STORE) {
#pragma unroll
      for (int k = 0; k < CSIM_NSER_CLAIM; ++k) ser_out[((size_t)k * a.n_paths + pl) * T + (t - 1)] = v[k];
    } else {
      csim_claim_acc<FIRST>(sums, v, lv);
    }
    lw1 = log(r.x - 1.0); rf = r.y; lv = lvt;
  };

  record(std::true_type{}, 1u);
  for (unsigned t = 2; t <= T; ++t) record(std::false_type{}, t);

  if (STORE) {                               // the sums from this lane's own stored series, in step order
    double lvp = pd0;
    auto replay = [&](auto first_tag, unsigned t) {
      double v[CSIM_NSER_CLAIM];
#pragma unroll
      for (int k = 0; k < CSIM_NSER_CLAIM; ++k) v[k] = ser_out[((size_t)k * a.n_paths + pl) * T + (t - 1)];
      csim_claim_acc<decltype(first_tag)::value>(sums, v, lvp);
      lvp = v[8];
    };
    replay(std::true_type{}, 1u);
    for (unsigned t = 2; t <= T; ++t) replay(std::false_type{}, t);
  }
  csim_claim_finish(sums, T, a.n_paths, pl, stats);
  clamped[pl] = nout;
#pragma unroll
  for (int d = 0; d < D; ++d) final_state[(size_t)pl * D + d] = x[d];
}

__global__ void __launch_bounds__(CSIM_BLOCK)
k_cont_sim_claim_records(long long n, const double* __restrict__ w, const double* __restrict__ em, const double* __restrict__ v,
                         double4* __restrict__ rec) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    rec[i] = make_double4(w[i], -log(em[i]), v[i], 0.0);
}

}  // namespace sdfs

namespace {
// the defaults, by the A/B of tools/continuous_simulation_times.py: one state at a time (a second state
// costs the second wave per SIMD in 6-D), groups of 8 corners in 4-D and of 4 in 6-D
constexpr int CSIM_K_DEFAULT = 1;            // states folded side by side
constexpr int csim_gd_default(int D) { return D == 4 ? 3 : 2; }   // log2 of the corners of a group

typedef void (*csim_fn)(const ContDesc, const ContSimArgs, const double2*, double*, unsigned*, double*, double*, double*);

// k_cont_sim_paths for a group and a look-ahead and, on the defaults of both, with the paths stored
template <int D, int GD, int K>
csim_fn csim_form(bool store) {
  if constexpr (GD == csim_gd_default(D) && K == CSIM_K_DEFAULT) {
    if (store) return k_cont_sim_paths<D, GD, K, true>;
  }
  return k_cont_sim_paths<D, GD, K, false>;
}

template <int D>
csim_fn csim_variant(int gd, int k, bool store) {
  if (gd == 2) return k == 1 ? csim_form<D, 2, 1>(store) : (k == 2 ? csim_form<D, 2, 2>(store) : csim_form<D, 2, 4>(store));
  if (gd == 3) return k == 1 ? csim_form<D, 3, 1>(store) : (k == 2 ? csim_form<D, 3, 2>(store) : csim_form<D, 3, 4>(store));
  if constexpr (D == 6) {
    if (gd == 4) return k == 1 ? csim_form<6, 4, 1>(store) : (k == 2 ? csim_form<6, 4, 2>(store) : nullptr);
  }
  return nullptr;
}

// the claim form: look-ahead 1, groups of 4 or 8 corners and, on the default group, with the paths stored
typedef void (*csim_claim_fn)(const ContDesc, const ContSimArgs, const double4*, const double, double*, unsigned*, double*, double*,
                              double*);

template <int D>
csim_claim_fn csim_claim_variant(int gd, bool store) {
  constexpr int GD0 = csim_claim_gd_default(D);
  if (store) return gd == GD0 ? k_cont_sim_claim_paths<D, GD0, true> : nullptr;
  return gd == 2 ? k_cont_sim_claim_paths<D, 2, false> : (gd == 3 ? k_cont_sim_claim_paths<D, 3, false> : nullptr);
}

int cont_handle_ok(sdfs_handle* h, const char* fn) {
  if (!h->cont) return fail(h, SDFS_ERR_UNSUPPORTED, "%s: exists for continuous-state handles only", fn);
  return 0;
}
}  // namespace
}  // extern "C++"

extern "C" {

int sdfs_cont_sdf_mean_dev(sdfs_handle* h, const double* w, double* em) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_handle_ok(h, "sdfs_cont_sdf_mean_dev"))) return rc;
  if (!w || !em || w == em) return fail(h, SDFS_ERR_ARG, "w and E_M: two distinct grids");
  ContIO io;
  memset(&io, 0, sizeof io);
  io.w = w; io.out = em;
  const ContDesc& cd = h->cd;
  const size_t lds = (size_t)(cd.cap + cd.ucap) * sizeof(double);       // T's: the staged box and its pre-contracted form
  const Counter c("cont:EM", 16.0 * (double)cd.N, (double)cd.N * cd.M * (2.0 * (double)(1 << cd.D) + 2.0 * cd.D + 2.0));
  const dim3 grid((unsigned)cd.N), block(256);
  return cd.D == 4 ? launch_kernel(h, cont_kernel<4, C_EM>, grid, block, lds, c, cd, io, ContNoTan{})
                   : launch_kernel(h, cont_kernel<6, C_EM>, grid, block, lds, c, cd, io, ContNoTan{});
}

int sdfs_cont_sim_records_dev(sdfs_handle* h, const double* w, const double* em, double* rec) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_handle_ok(h, "sdfs_cont_sim_records_dev"))) return rc;
  if (!w || !em || !rec) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  const long long N = h->cd.N;
  const int grid = stream_grid(h, N, CSIM_BLOCK);
  return launch_kernel(h, k_cont_sim_records, dim3(grid), dim3(CSIM_BLOCK), 0, Counter("csim:records", 32.0 * (double)N, 0), N, w, em,
                       reinterpret_cast<double2*>(rec));
}

}  // extern "C"

namespace {
// the two path entry points: claim = false (sdfs_cont_sim_paths_dev), or the claim form with its kappa
int csim_paths(sdfs_handle* h, const char* fn_name, bool claim, const double* rec, double kappa, const sdfs_cont_sim_desc* d, double* stats, uint32_t* clamped, double* final_state, double* states, double* series) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_handle_ok(h, fn_name))) return rc;
  if (!rec || !d || !stats || !clamped || !final_state) return fail(h, SDFS_ERR_ARG, "NULL records, desc, stats, clamped or final_state");
  if (claim && !std::isfinite(kappa)) return fail(h, SDFS_ERR_ARG, "kappa is not finite");
  if (!states != !series) return fail(h, SDFS_ERR_ARG, "states and series are stored together: both NULL or neither");
  char msg[160];
  if (!sim_ranges_ok(msg, d->path_offset, d->n_paths, &d->step_offset, d->burn_in, d->n_periods, 0)) return fail(h, SDFS_ERR_ARG, "%s", msg);
  if (d->start_mode < 0 || d->start_mode > 2 || (d->start_mode == 2 && !d->start_dev))
    return fail(h, SDFS_ERR_ARG, "start_mode = %d: 0 (zero state), 1 (start[]) or 2 (start_dev, not NULL)", d->start_mode);
  const ContDesc& cd = h->cd;
  for (int ax = 0; ax < cd.D && d->start_mode == 1; ++ax)
    if (!std::isfinite(d->start[ax])) return fail(h, SDFS_ERR_ARG, "start[%d] is not finite", ax);
  const int k = d->lookahead ? d->lookahead : CSIM_K_DEFAULT;
  const int g = d->group ? d->group : 1 << (claim ? csim_claim_gd_default(cd.D) : csim_gd_default(cd.D));
  const int gd = g == 4 ? 2 : (g == 8 ? 3 : (g == 16 ? 4 : 0));
  const bool store = states != nullptr;
  if (store && (k != CSIM_K_DEFAULT || gd != (claim ? csim_claim_gd_default(cd.D) : csim_gd_default(cd.D))))
    return fail(h, SDFS_ERR_ARG, "stored paths run with the default lookahead and group");
  csim_claim_fn cfn = nullptr;
  if (claim) {
    if (k == 1) cfn = cd.D == 4 ? csim_claim_variant<4>(gd, store) : csim_claim_variant<6>(gd, store);
    if (!cfn) return fail(h, SDFS_ERR_ARG, "lookahead = %d, group = %d: the claim form runs with lookahead 1 and groups of 4 or 8 corners",
                          d->lookahead, d->group);
  }
  const csim_fn fn = !claim && (k == 1 || k == 2 || k == 4) && gd ? (cd.D == 4 ? csim_variant<4>(gd, k, store) : csim_variant<6>(gd, k, store)) : nullptr;
  if (!fn && !cfn) return fail(h, SDFS_ERR_ARG, "lookahead = %d, group = %d: lookahead 1, 2 or 4 with groups of 4 or 8 corners, and in 6-D "
                       "lookahead 1 or 2 with groups of 16", d->lookahead, d->group);
  ContSimArgs a{};
  a.key0 = (unsigned)(d->seed & 0xffffffffu); a.key1 = (unsigned)(d->seed >> 32);
  a.step0 = (unsigned)d->step_offset; a.burn_in = (unsigned)d->burn_in; a.n_periods = (unsigned)d->n_periods;
  a.start_mode = d->start_mode;
  a.path0 = (unsigned long long)d->path_offset; a.n_paths = d->n_paths;
  for (int ax = 0; ax < cd.D; ++ax) a.start[ax] = d->start[ax];
  a.start_dev = d->start_dev;
  a.theta = h->theta; a.theta_ln_beta = h->theta * std::log(h->beta); a.gamma = h->cont_gamma;
  const dim3 grid((unsigned)((d->n_paths + CSIM_BLOCK - 1) / CSIM_BLOCK));
  const double steps = (double)d->n_paths * (double)(d->burn_in + d->n_periods);
  const double corners = (double)(1 << cd.D) * (double)d->n_paths * (double)(d->n_periods + 1);
  if (cfn)
    return launch_kernel(h, cfn, grid, dim3(CSIM_BLOCK), 0, Counter("csim:claim_paths", 32.0 * corners, steps), cd, a,
                         reinterpret_cast<const double4*>(rec), kappa, stats, clamped, final_state, states, series);
  return launch_kernel(h, fn, grid, dim3(CSIM_BLOCK), 0, Counter("csim:paths", 16.0 * corners, steps), cd, a,
                       reinterpret_cast<const double2*>(rec), stats, clamped, final_state, states, series);
}
}  // namespace

extern "C" {

int sdfs_cont_sim_paths_dev(sdfs_handle* h, const double* rec, const sdfs_cont_sim_desc* d, double* stats, uint32_t* clamped,
                            double* final_state, double* states, double* series) {
  return csim_paths(h, "sdfs_cont_sim_paths_dev", false, rec, 0.0, d, stats, clamped, final_state, states, series);
}

int sdfs_cont_sim_claim_records_dev(sdfs_handle* h, const double* w, const double* em, const double* v, double* rec) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_handle_ok(h, "sdfs_cont_sim_claim_records_dev"))) return rc;
  if (!w || !em || !v || !rec) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  const long long N = h->cd.N;
  const int grid = stream_grid(h, N, CSIM_BLOCK);
  return launch_kernel(h, k_cont_sim_claim_records, dim3(grid), dim3(CSIM_BLOCK), 0, Counter("csim:claim_records", 56.0 * (double)N, 0),
                       N, w, em, v, reinterpret_cast<double4*>(rec));
}

int sdfs_cont_sim_claim_paths_dev(sdfs_handle* h, const double* rec, const sdfs_cont_sim_desc* d, double kappa, double* stats,
                                  uint32_t* clamped, double* final_state, double* states, double* series) {
  return csim_paths(h, "sdfs_cont_sim_claim_paths_dev", true, rec, kappa, d, stats, clamped, final_state, states, series);
}

}  // extern "C"

// sim_kernels.hpp -- simulated paths of the discretised chain at w* (sdfs_sim_records_dev, sdfs_sim_paths_dev).
//
// k_sim_records streams the grid once and writes one 64-byte record per state,
//
//   {ln w, ln(w - 1), -ln E_x[M], mu_c + z(x), w, ln v, ln(1 + v), 0},
//
// so that a path-step costs one gathered cache line and no logarithm of w is recomputed along a path.  k_sim_paths runs
// one path per lane: Philox4x32-10 words (Salmon et al. 2011; counter (t, p, b, 0), key = the seed's two halves), one
// inverse-CDF search per axis over the host's cumulative transition rows (in LDS), one record load, the series of
// DESIGN §4.8 and their one-pass sums.  The index recursion never reads a record, so the chain runs K steps ahead of
// the series and K record loads stay in flight (a ring of K register slots, unrolled so every slot index is a
// compile-time constant).  The sums are shifted by each series' first value; the statistics go out structure-of-arrays,
// one coalesced store per statistic.  No atomics, no host synchronisation: two runs give identical bits, and a path's
// result depends only on its number, the seed and the model.  fp64 throughout.
#pragma once

#include <hip/hip_runtime.h>

#include "price_kernels.hpp"

constexpr int SIM_BLOCK = 256;
constexpr int SIM_MAXD = 6;
constexpr int SIM_MAXN = 32;
constexpr int SIM_REC = 8;                   // doubles per state record (64 B)
constexpr int SIM_NSER_MAX = 9;
// LDS table: the n_a x n_a cumulative rows of every axis, the stationary cumulative marginals, h_lambda and sigma_c
constexpr int SIM_TAB_MAX = SIM_MAXD * SIM_MAXN * SIM_MAXN + SIM_MAXD * SIM_MAXN + 2 * SIM_MAXN;

struct SimArgs {
  int n[SIM_MAXD];                           // extents (grid order)
  int stride[SIM_MAXD];                      // flat strides (C order)
  int cdf_off[SIM_MAXD];                     // offset of axis a's cumulative rows in the LDS table
  int cdf0_off[SIM_MAXD];                    // ... of its stationary cumulative marginal
  int start[SIM_MAXD];                       // fixed start x_0 (start_fixed)
  int ax_lam, ax_c;                          // axes h_lambda (next state) and sigma_c (current state) are indexed by
  int hl_off, sc_off;                        // offsets of the h_lambda / sigma_c tables
  int lds_n;                                 // doubles of the LDS table
  int start_fixed;
  unsigned key0, key1;
  unsigned long long path0;                  // number of the launch's first path
  long long n_paths;
  unsigned burn_in, n_periods;               // B, T
  double theta, theta_ln_beta, gamma, kappa;
};

// -- Philox4x32-10 ---------------------------------------------------------------------------------------------------
struct SimWords { unsigned r[4]; };

__device__ __forceinline__ SimWords sim_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
    const unsigned lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return SimWords{{c0, c1, c2, c3}};
}

__device__ __forceinline__ double sim_u(unsigned r) { return ((double)r + 0.5) * 0x1p-32; }   // exact, in (0, 1)

// least j with u < row[j] = the number of k < n - 1 with row[k] <= u (the rows rise; the host sets row[n-1] = 2)
template <bool LIN>
__device__ __forceinline__ unsigned sim_search(const double* row, int n, double u) {
  if (LIN) {
    unsigned j = 0;
    for (int k = 0; k < n - 1; ++k) j += row[k] <= u ? 1u : 0u;
    return j;
  }
  int top = 1;
  while (top < n) top <<= 1;                 // (uniform: n is a kernel argument)
  unsigned j = 0;
  for (int s = top >> 1; s >= 1; s >>= 1) {
    const unsigned c = j + (unsigned)s;      // the answer is >= c iff row[c - 1] <= u (c <= n - 1)
    if ((int)c <= n - 1 && row[c - 1] <= u) j = c;
  }
  return j;
}

// one step of the chain: x_t from x_{t-1} with step t's words (r0 ... r_{ND-1}); xi = the step's normal draw
template <int ND, bool LIN>
__device__ __forceinline__ void sim_advance(const SimArgs& a, const double* tab, unsigned t, unsigned p, unsigned (&ix)[ND],
                                            double* xi) {
  const SimWords b0 = sim_philox(t, p, 0u, 0u, a.key0, a.key1);
  unsigned r[8] = {b0.r[0], b0.r[1], b0.r[2], b0.r[3], 0u, 0u, 0u, 0u};
  if (ND > 4 || xi) {
    const SimWords b1 = sim_philox(t, p, 1u, 0u, a.key0, a.key1);
    r[4] = b1.r[0]; r[5] = b1.r[1]; r[6] = b1.r[2]; r[7] = b1.r[3];
  }
#pragma unroll
  for (int d = 0; d < ND; ++d) ix[d] = sim_search<LIN>(tab + a.cdf_off[d] + ix[d] * a.n[d], a.n[d], sim_u(r[d]));
  if (xi) *xi = sqrt(-2.0 * log(sim_u(r[6]))) * cos(2.0 * M_PI * ((double)r[7] * 0x1p-32));
}

template <int ND>
__device__ __forceinline__ unsigned sim_code(const unsigned (&ix)[ND], unsigned& off, const SimArgs& a) {
  unsigned c = 0;
  off = 0;
#pragma unroll
  for (int d = 0; d < ND; ++d) { c |= ix[d] << (5 * d); off += ix[d] * (unsigned)a.stride[d]; }
  return c;
}

// record fields a path-step reads (ln v and ln(1 + v) only with a claim)
template <bool KAP>
struct SimSlot {
  double lw, lw1, nlem, muz, w, lv, l1v;
  double xi;
  unsigned code;
};

template <bool KAP>
__device__ __forceinline__ void sim_load(SimSlot<KAP>& s, const double* __restrict__ rec, unsigned off) {
  const double2* q = reinterpret_cast<const double2*>(rec + (size_t)off * SIM_REC);
  const double2 a = q[0], b = q[1];
  s.lw = a.x; s.lw1 = a.y; s.nlem = b.x; s.muz = b.y;
  if (KAP) {
    const double2 c = q[2], d = q[3];
    s.w = c.x; s.lv = c.y; s.l1v = d.x;
  } else {
    s.w = rec[(size_t)off * SIM_REC + 4]; s.lv = 0.0; s.l1v = 0.0;
  }
}

// one-pass sums of one series, shifted by its first value
struct SimAcc { double s0, pv, s1, s2, sl; };

template <bool FIRST>
__device__ __forceinline__ void sim_acc(SimAcc& c, double v) {
  if (FIRST) { c.s0 = v; c.pv = 0.0; c.s1 = 0.0; c.s2 = 0.0; c.sl = 0.0; return; }
  const double d = v - c.s0;
  c.s1 += d;
  c.s2 = fma(d, d, c.s2);
  c.sl = fma(d, c.pv, c.sl);
  c.pv = d;
}

template <bool KAP>
struct SimPrev { double lw1, nlem, muz, lv, sc; };   // fields of x_{t-1} the step needs

template <int ND, bool KAP, bool LIN, int K, bool STORE>
__global__ void __launch_bounds__(SIM_BLOCK)
k_sim_paths(SimArgs a, const double* __restrict__ tabg, const double* __restrict__ rec, double* __restrict__ stats,
            unsigned char* __restrict__ idx_out, double* __restrict__ ser_out) {
  constexpr int NS = KAP ? 9 : 6;            // dc m rf rc xc wc [rd xd pd]
  extern __shared__ double tab[];
  for (int k = threadIdx.x; k < a.lds_n; k += blockDim.x) tab[k] = tabg[k];
  __syncthreads();
  const long long pl = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pl >= a.n_paths) return;               // (no barrier below)
  const unsigned p = (unsigned)(a.path0 + (unsigned long long)pl);
  const unsigned T = a.n_periods, B = a.burn_in;

  // x_0, then the burn-in
  unsigned ix[ND];
  if (a.start_fixed) {
#pragma unroll
    for (int d = 0; d < ND; ++d) ix[d] = (unsigned)a.start[d];
  } else {
    const SimWords b0 = sim_philox(0u, p, 0u, 0u, a.key0, a.key1);
    unsigned r[8] = {b0.r[0], b0.r[1], b0.r[2], b0.r[3], 0u, 0u, 0u, 0u};
    if (ND > 4) { const SimWords b1 = sim_philox(0u, p, 1u, 0u, a.key0, a.key1); r[4] = b1.r[0]; r[5] = b1.r[1]; }
#pragma unroll
    for (int d = 0; d < ND; ++d) ix[d] = sim_search<LIN>(tab + a.cdf0_off[d], a.n[d], sim_u(r[d]));
  }
  for (unsigned t = 1; t <= B; ++t) sim_advance<ND, LIN>(a, tab, t, p, ix, nullptr);

  // x_B: the previous state of the first recorded step
  SimPrev<KAP> pr;
  {
    unsigned off;
    const unsigned code = sim_code<ND>(ix, off, a);
    SimSlot<KAP> s0;
    sim_load<KAP>(s0, rec, off);
    pr.lw1 = s0.lw1; pr.nlem = s0.nlem; pr.muz = s0.muz; pr.lv = s0.lv;
    pr.sc = tab[a.sc_off + ((code >> (5 * a.ax_c)) & 31u)];
    if (STORE) {
#pragma unroll
      for (int d = 0; d < ND; ++d) idx_out[((size_t)pl * (T + 1)) * ND + d] = (unsigned char)ix[d];
    }
  }

  // the ring: slot j holds step B + 1 + j (loads in flight)
  SimSlot<KAP> ring[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if ((unsigned)j < T) {
      sim_advance<ND, LIN>(a, tab, B + 1 + j, p, ix, &ring[j].xi);
      unsigned off;
      ring[j].code = sim_code<ND>(ix, off, a);
      sim_load<KAP>(ring[j], rec, off);
    }
  }

  SimAcc acc[NS];
  double sx = 0.0, sxx = 0.0, sxy = 0.0, x0 = 0.0;

  // consume step s from a slot, then refill it with step s + K
  auto step = [&](auto first_tag, SimSlot<KAP>& sl, unsigned s) {
    constexpr bool FIRST = decltype(first_tag)::value;
    const double hl = tab[a.hl_off + ((sl.code >> (5 * a.ax_lam)) & 31u)];
    const double dc = pr.muz + pr.sc * sl.xi;
    const double rl = sl.lw - pr.lw1;
    const double v[9] = {dc,
                         a.theta_ln_beta + a.theta * hl - a.gamma * dc + (a.theta - 1.0) * rl,
                         pr.nlem,
                         dc + rl,
                         dc + rl - pr.nlem,
                         sl.w,
                         KAP ? a.kappa * dc + sl.l1v - pr.lv : 0.0,
                         KAP ? a.kappa * dc + sl.l1v - pr.lv - pr.nlem : 0.0,
                         sl.lv};
    // slope: y_t = xd_t (xc_t without a claim) on x_{t-1} = ln v(x_{t-1}) (ln(w(x_{t-1}) - 1))
    const double xr = KAP ? pr.lv : pr.lw1;
#pragma unroll
    for (int k = 0; k < NS; ++k) sim_acc<FIRST>(acc[k], v[k]);
    if (FIRST) {
      x0 = xr;
    } else {
      const double dx = xr - x0, dy = acc[KAP ? 7 : 4].pv;
      sx += dx;
      sxx = fma(dx, dx, sxx);
      sxy = fma(dx, dy, sxy);
    }
    if (STORE) {
      const unsigned t = s - B - 1;
#pragma unroll
      for (int k = 0; k < NS; ++k) ser_out[((size_t)k * a.n_paths + pl) * T + t] = v[k];
#pragma unroll
      for (int d = 0; d < ND; ++d) idx_out[((size_t)pl * (T + 1) + t + 1) * ND + d] = (unsigned char)((sl.code >> (5 * d)) & 31u);
    }
    pr.lw1 = sl.lw1; pr.nlem = sl.nlem; pr.muz = sl.muz; pr.lv = sl.lv;
    pr.sc = tab[a.sc_off + ((sl.code >> (5 * a.ax_c)) & 31u)];
    if (s + K <= B + T) {                    // (uniform)
      sim_advance<ND, LIN>(a, tab, s + K, p, ix, &sl.xi);
      unsigned off;
      sl.code = sim_code<ND>(ix, off, a);
      sim_load<KAP>(sl, rec, off);
    }
  };

  step(std::true_type{}, ring[0], B + 1);
  for (unsigned s = B + 2; s <= B + T; s += K) {
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (s + j <= B + T) step(std::false_type{}, ring[(j + 1) % K], s + j);
  }

  // statistics: mean, std, ac1 per series (d = s - s_first, so d_1 = 0), then the slope
  const double Tn = (double)T;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const SimAcc& c = acc[k];
    const double mt = c.s1 / Tn;
    const double den = c.s2 - c.s1 * mt;                       // sum (d - mean)^2
    const double num = c.sl - mt * (2.0 * c.s1 - c.pv) + (Tn - 1.0) * mt * mt;
    stats[(size_t)(3 * k + 0) * a.n_paths + pl] = c.s0 + mt;
    stats[(size_t)(3 * k + 1) * a.n_paths + pl] = sqrt(fmax(den, 0.0) / Tn);
    stats[(size_t)(3 * k + 2) * a.n_paths + pl] = den > 0.0 ? num / den : __builtin_nan("");
  }
  const double sy = acc[KAP ? 7 : 4].s1;
  const double dxx = sxx - sx * (sx / Tn), dxy = sxy - sx * (sy / Tn);
  stats[(size_t)(3 * NS) * a.n_paths + pl] = dxx > 0.0 ? dxy / dxx : __builtin_nan("");
}

// one record per state; zt = mu_c + z in the a3 layout (PriceGeom::a3s strides); v == nullptr: no claim
__global__ void __launch_bounds__(PRICE_BLOCK)
k_sim_records(PriceGeom g, const double* __restrict__ zt, const double* __restrict__ w, const double* __restrict__ em,
              const double* __restrict__ v, double* __restrict__ rec) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += stride) {
    unsigned r = (unsigned)i, off = 0;
    for (int a = g.ndim - 1; a >= 0; --a) {
      const unsigned q = price_q(g.ext[a], r);
      off += (r - q * g.ext[a].d) * (unsigned)g.a3s[a];
      r = q;
    }
    const double wi = w[i];
    double lv = 0.0, l1v = 0.0;
    if (v) { const double vi = v[i]; lv = log(vi); l1v = log(1.0 + vi); }
    double2* o = reinterpret_cast<double2*>(rec + (size_t)i * SIM_REC);
    o[0] = make_double2(log(wi), log(wi - 1.0));
    o[1] = make_double2(-log(em[i]), zt[off]);
    o[2] = make_double2(wi, lv);
    o[3] = make_double2(l1v, 0.0);
  }
}

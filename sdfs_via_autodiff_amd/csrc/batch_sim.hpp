// batch_sim.hpp -- simulated paths for a whole batch at w*, the cross-path moments reduced on chip
// (sdfs_batch_sim_records_dev, sdfs_batch_sim_paths_dev).
//
// k_batch_sim_records writes the 64-byte state records of sim_kernels.hpp for every member, [B][N][8], from the batch's
// w, E_x[M] and price-dividend grids.  k_batch_sim_paths runs one path per lane on a grid of (workgroups per member,
// members): a workgroup copies its member's table block (cumulative rows per axis, cumulative stationary marginals,
// h_lambda, sigma_c) and, in the LDS form, the member's N records into LDS, then walks its 256 paths with the device
// functions of sim_kernels.hpp (Philox counters (t, p, b, 0), the u-mapping, the inverse-CDF search, the shifted one-pass
// sums), so a path's indices equal those of k_sim_paths on the same tables bit for bit and depend only on the path's
// number, the seed and the member's inputs.
//   LDSREC = true : every path-step reads its record from LDS; no look-ahead ring (the gather never leaves the CU).
//   LDSREC = false: the records are gathered from global memory through the ring of K slots of k_sim_paths.
// Each of the 3 nser + 1 per-path statistics is then reduced over the workgroup's paths to (n finite, mean, M2) in a
// fixed order: one triple per lane, four DPP steps inside the rows of 16 and the four rows by v_readlane (the moves of
// wave_reduce.hpp, the lower lane's triple always the left operand), then one LDS step over the waves, wave 0 first; the
// triples are merged by Chan's pairwise formula.  k_batch_sim_moments merges a member's workgroup triples in workgroup
// order into (n, mean, se).  No atomics: two runs give identical bits.  A skipped member runs no path and gets NaN.
// fp64 throughout.
#pragma once

#include <hip/hip_runtime.h>

#include "batch_kernels.hpp"
#include "sim_kernels.hpp"
#include "wave_reduce.hpp"

namespace sdfs {

constexpr int BSIM_NW = SIM_BLOCK / 64;                      // waves of a workgroup
constexpr int BSIM_NSTAT_MAX = 3 * SIM_NSER_MAX + 1;
constexpr int BSIM_RED = BSIM_NW * BSIM_NSTAT_MAX * 3;       // doubles behind the tables (and records): one triple per wave and statistic
constexpr int BSIM_YMAX = 32768;                             // members per launch (gridDim.y)

struct BatchSimArgs {
  SimArgs s;                   // what the members share; theta, theta ln beta, gamma, kappa are read per member from scal
  const double* tab;           // [B][simwords]
  const double* scal;          // [B][4]: theta, theta ln beta, gamma, kappa
  const int* skip;             // [B]
  const double* rec;           // [B][N][8]
  double* stats;               // [B][3 nser + 1][P], or nullptr
  double* part;                // [B][3 nser + 1][G][3]
  unsigned char* idx;          // STORE: [B][P][T + 1][ND]
  double* ser;                 // STORE: [B][nser][P][T]
  int simwords;                // doubles per table block (even)
  int N;
  int b0;                      // member of blockIdx.y == 0
};

struct BsimTriple { double n, mean, m2; };

// Chan, Golub and LeVeque's merge of two (count, mean, sum of squared deviations); an empty side (n = 0, mean = 0, M2 = 0)
// leaves the other unchanged bit for bit
__device__ __forceinline__ BsimTriple bsim_merge(const BsimTriple& a, const BsimTriple& b) {
  const double n = a.n + b.n;
  const double f = n > 0.0 ? b.n / n : 0.0;
  const double d = b.mean - a.mean;
  return BsimTriple{n, fma(d, f, a.mean), fma(d * d, a.n * f, a.m2 + b.m2)};
}

// one butterfly step: the partner's triple by a DPP move; the lane whose BIT is clear holds the left operand
template <int CTRL, int BIT>
__device__ __forceinline__ BsimTriple bsim_step(const BsimTriple& t, int lane) {
  const BsimTriple o{dpp_mov_f64<CTRL>(t.n), dpp_mov_f64<CTRL>(t.mean), dpp_mov_f64<CTRL>(t.m2)};
  const bool upper = (lane & BIT) != 0;
  return bsim_merge(upper ? o : t, upper ? t : o);
}

__device__ __forceinline__ BsimTriple bsim_row(const BsimTriple& t, int l) {
  return BsimTriple{readlane_f64(t.n, l), readlane_f64(t.mean, l), readlane_f64(t.m2, l)};
}

// the wave's triple of one value per lane (NaN and infinities are left out); every lane must be active; wave-uniform result
__device__ __forceinline__ BsimTriple bsim_wave(double x, int lane) {
  const bool ok = fabs(x) < __builtin_huge_val();
  BsimTriple t{ok ? 1.0 : 0.0, ok ? x : 0.0, 0.0};
  t = bsim_step<0xB1, 1>(t, lane);             // quad_perm [1,0,3,2]
  t = bsim_step<0x4E, 2>(t, lane);             // quad_perm [2,3,0,1]
  t = bsim_step<0x141, 4>(t, lane);            // row_half_mirror
  t = bsim_step<0x140, 8>(t, lane);            // row_mirror
  return bsim_merge(bsim_merge(bsim_row(t, 0), bsim_row(t, 16)), bsim_merge(bsim_row(t, 32), bsim_row(t, 48)));
}

template <int ND, bool KAP, bool LDSREC, bool STORE, int K>
__global__ void __launch_bounds__(SIM_BLOCK)
k_batch_sim_paths(const BatchSimArgs A) {
  constexpr int NS = KAP ? 9 : 6;              // dc m rf rc xc wc [rd xd pd]
  constexpr int NSTAT = 3 * NS + 1;
  extern __shared__ __attribute__((aligned(16))) double bsim_lds[];
  const int b = A.b0 + (int)blockIdx.y, G = (int)gridDim.x;
  const int tid = (int)threadIdx.x;
  const long long P = A.s.n_paths;
  const long long pl = (long long)blockIdx.x * SIM_BLOCK + tid;
  const bool live = pl < P;
  const unsigned T = A.s.n_periods;
  const double nan = __builtin_nan("");
  double* const part = A.part + ((size_t)b * NSTAT * G + blockIdx.x) * 3;      // statistic k at part + 3 G k
  unsigned char* const idx_out = STORE ? A.idx + (size_t)b * P * (T + 1) * ND : nullptr;
  double* const ser_out = STORE ? A.ser + (size_t)b * NS * P * T : nullptr;

  if (A.skip[b]) {                             // (uniform) no path: NaN statistics and series, empty triples
    if (live) {
      if (A.stats)
        for (int k = 0; k < NSTAT; ++k) A.stats[((size_t)b * NSTAT + k) * P + pl] = nan;
      if (STORE) {
        for (int k = 0; k < NS; ++k)
          for (unsigned t = 0; t < T; ++t) ser_out[((size_t)k * P + pl) * T + t] = nan;
        for (size_t i = 0; i < (size_t)(T + 1) * ND; ++i) idx_out[(size_t)pl * (T + 1) * ND + i] = 0;
      }
    }
    if (tid < NSTAT) { part[(size_t)3 * G * tid] = 0.0; part[(size_t)3 * G * tid + 1] = 0.0; part[(size_t)3 * G * tid + 2] = 0.0; }
    return;
  }

  // the member's table block, and in the LDS form its records behind it
  double* const tab = bsim_lds;
  {
    const double2* src = reinterpret_cast<const double2*>(A.tab + (size_t)b * A.simwords);
    double2* dst = reinterpret_cast<double2*>(tab);
    for (int k = tid; k < A.simwords / 2; k += SIM_BLOCK) dst[k] = src[k];
  }
  const double* rec;
  double* red;
  if constexpr (LDSREC) {
    double* const lrec = bsim_lds + A.simwords;
    const double2* src = reinterpret_cast<const double2*>(A.rec + (size_t)b * A.N * SIM_REC);
    double2* dst = reinterpret_cast<double2*>(lrec);
    for (int k = tid; k < A.N * (SIM_REC / 2); k += SIM_BLOCK) dst[k] = src[k];
    rec = lrec;
    red = lrec + (size_t)A.N * SIM_REC;
  } else {
    rec = A.rec + (size_t)b * A.N * SIM_REC;
    red = bsim_lds + A.simwords;
  }
  __syncthreads();

  SimArgs a = A.s;
  {
    const double* sc = A.scal + (size_t)b * 4;
    a.theta = sc[0]; a.theta_ln_beta = sc[1]; a.gamma = sc[2]; a.kappa = sc[3];
  }

  double st[NSTAT];
#pragma unroll
  for (int k = 0; k < NSTAT; ++k) st[k] = nan;

  if (live) {
    const unsigned p = (unsigned)(a.path0 + (unsigned long long)pl);
    const unsigned B = a.burn_in;

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
      for (int d = 0; d < ND; ++d) ix[d] = sim_search<false>(tab + a.cdf0_off[d], a.n[d], sim_u(r[d]));
    }
    for (unsigned t = 1; t <= B; ++t) sim_advance<ND, false>(a, tab, t, p, ix, nullptr);

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

    SimAcc acc[NS];
    double sx = 0.0, sxx = 0.0, sxy = 0.0, x0 = 0.0;

    // recorded step t (0-based) is step B + 1 + t of the chain
    auto fill = [&](SimSlot<KAP>& sl, unsigned t) {
      sim_advance<ND, false>(a, tab, B + 1 + t, p, ix, &sl.xi);
      unsigned off;
      sl.code = sim_code<ND>(ix, off, a);
      sim_load<KAP>(sl, rec, off);
    };
    auto consume = [&](auto first_tag, const SimSlot<KAP>& sl, unsigned t) {
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
#pragma unroll
        for (int k = 0; k < NS; ++k) ser_out[((size_t)k * P + pl) * T + t] = v[k];
#pragma unroll
        for (int d = 0; d < ND; ++d) idx_out[((size_t)pl * (T + 1) + t + 1) * ND + d] = (unsigned char)((sl.code >> (5 * d)) & 31u);
      }
      pr.lw1 = sl.lw1; pr.nlem = sl.nlem; pr.muz = sl.muz; pr.lv = sl.lv;
      pr.sc = tab[a.sc_off + ((sl.code >> (5 * a.ax_c)) & 31u)];
    };

    if constexpr (LDSREC) {
      SimSlot<KAP> sl;
      fill(sl, 0u);
      consume(std::true_type{}, sl, 0u);
      for (unsigned t = 1; t < T; ++t) {
        fill(sl, t);
        consume(std::false_type{}, sl, t);
      }
    } else {
      // the ring: slot j holds recorded step j (loads in flight); a consumed slot is refilled with step t + K
      SimSlot<KAP> ring[K];
#pragma unroll
      for (int j = 0; j < K; ++j)
        if ((unsigned)j < T) fill(ring[j], (unsigned)j);
      consume(std::true_type{}, ring[0], 0u);
      if (T > (unsigned)K) fill(ring[0], (unsigned)K);
      for (unsigned t = 1; t < T; t += K) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if ((unsigned)j < T - t) {             // (uniform) step t + j exists
            const unsigned tt = t + j;
            SimSlot<KAP>& sl = ring[(j + 1) % K];
            consume(std::false_type{}, sl, tt);
            if (T - tt > (unsigned)K) fill(sl, tt + K);
          }
        }
      }
    }

    // statistics: mean, std, ac1 per series (d = s - s_first, so d_1 = 0), then the slope
    const double Tn = (double)T;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const SimAcc& c = acc[k];
      const double mt = c.s1 / Tn;
      const double den = c.s2 - c.s1 * mt;                       // sum (d - mean)^2
      const double num = c.sl - mt * (2.0 * c.s1 - c.pv) + (Tn - 1.0) * mt * mt;
      st[3 * k + 0] = c.s0 + mt;
      st[3 * k + 1] = sqrt(fmax(den, 0.0) / Tn);
      st[3 * k + 2] = den > 0.0 ? num / den : nan;
    }
    const double sy = acc[KAP ? 7 : 4].s1;
    const double dxx = sxx - sx * (sx / Tn), dxy = sxy - sx * (sy / Tn);
    st[3 * NS] = dxx > 0.0 ? dxy / dxx : nan;
    if (A.stats) {
#pragma unroll
      for (int k = 0; k < NSTAT; ++k) A.stats[((size_t)b * NSTAT + k) * P + pl] = st[k];
    }
  }

  // the workgroup's triple of every statistic: lanes, then waves (wave 0 first)
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < NSTAT; ++k) {
    const BsimTriple t = bsim_wave(st[k], lane);
    if (lane == 0) {
      double* const o = red + (wave * NSTAT + k) * 3;
      o[0] = t.n; o[1] = t.mean; o[2] = t.m2;
    }
  }
  __syncthreads();
  if (tid < NSTAT) {
    BsimTriple t{red[tid * 3], red[tid * 3 + 1], red[tid * 3 + 2]};
    for (int w = 1; w < BSIM_NW; ++w) {
      const double* const o = red + (w * NSTAT + tid) * 3;
      t = bsim_merge(t, BsimTriple{o[0], o[1], o[2]});
    }
    double* const o = part + (size_t)3 * G * tid;
    o[0] = t.n; o[1] = t.mean; o[2] = t.m2;
  }
}

// (n, mean, se) of every member and statistic from its workgroup triples, merged in workgroup order
__global__ void __launch_bounds__(256)
k_batch_sim_moments(int B, int nstat, int G, const int* __restrict__ skip, const double* __restrict__ part, double* __restrict__ mom) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= B * nstat) return;
  const double nan = __builtin_nan("");
  double* const o = mom + (size_t)i * 3;
  if (skip[i / nstat]) { o[0] = nan; o[1] = nan; o[2] = nan; return; }
  const double* const p = part + (size_t)i * G * 3;
  BsimTriple t{p[0], p[1], p[2]};
  for (int g = 1; g < G; ++g) t = bsim_merge(t, BsimTriple{p[3 * g], p[3 * g + 1], p[3 * g + 2]});
  o[0] = t.n;
  o[1] = t.n > 0.0 ? t.mean : nan;
  o[2] = t.n > 1.0 ? sqrt(t.m2 / (t.n - 1.0) / t.n) : nan;
}

// one record per state and member; zt = mu_c + z of every member in the a3 layout (BatchDesc::a3s strides); v == nullptr: no claim
__global__ void __launch_bounds__(256)
k_batch_sim_records(const BatchDesc D, int na3, int b0, const double* __restrict__ zt, const double* __restrict__ w,
                    const double* __restrict__ em, const double* __restrict__ v, double* __restrict__ rec) {
  const int b = b0 + (int)blockIdx.y;
  const size_t base = (size_t)b * D.N;
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < D.N; i += (int)(gridDim.x * blockDim.x)) {
    unsigned r = (unsigned)i, off = 0;
    for (int a = D.ndim - 1; a >= 0; --a) {
      const unsigned q = r / (unsigned)D.n[a];
      off += (r - q * (unsigned)D.n[a]) * (unsigned)D.a3s[a];
      r = q;
    }
    const double wi = w[base + i];
    double lv = 0.0, l1v = 0.0;
    if (v) { const double vi = v[base + i]; lv = log(vi); l1v = log(1.0 + vi); }
    double2* o = reinterpret_cast<double2*>(rec + (base + i) * SIM_REC);
    o[0] = make_double2(log(wi), log(wi - 1.0));
    o[1] = make_double2(-log(em[base + i]), zt[(size_t)b * na3 + off]);
    o[2] = make_double2(wi, lv);
    o[3] = make_double2(l1v, 0.0);
  }
}

using batch_sim_fn = void (*)(const BatchSimArgs);

}  // namespace sdfs

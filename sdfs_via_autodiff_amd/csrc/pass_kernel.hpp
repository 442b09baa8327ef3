// pass_kernel.hpp -- the expectation ("H-apply") kernel for gfx950.
//
// One launch = one PASS over the state grid.  A pass contracts up to three grid
// axes with their transition matrices inside an LDS tile:
//
//   y[.., i, ..] = sum_I Q_g[cond.., i, I] * x[.., I, ..]           (per axis g)
//
// which is how the reference's  sum_{next states} H * w^theta
// (code/ssy/discrete/ssy_wc_ratio.py:143-145, code/gcy/discrete/gcy_wc_ratio.py:230-232)
// factorises (every H is a product of per-axis transition matrices).
// The scale factors a1 (next-state), a2, a3 (current-state) of the reference are folded into the
// transition tensors on the host (sdfs_create), so the first pass applies just  x = w^theta  while
// loading and the last pass the Epstein-Zin aggregator  Tw = 1 + beta S^(1/theta)
// (ssy_wc_ratio.py:148, gcy_wc_ratio.py:235) and the sup-norm residual of
// code/solvers.py:36 while storing.
//
// Work decomposition: one workgroup per tile.  A tile has up to three "tile axes"
// (full extent in LDS, slot 2 = fastest in memory -> coalesced runs); every other
// grid axis is fixed for the block.  Each contraction is a batched
// (n x n) . (n x columns) product done with v_mfma_f64_16x16x4_f64: a wave owns
// 16 columns at a time, keeps the Q fragments in registers, reads the B operand
// from LDS and writes the result back in place (a wave reads all rows of its 16
// columns before it writes any of them).
//
// Memory phase: every thread owns EPT units of VEC consecutive doubles; all of a
// thread's global loads are issued back to back before the first is consumed, so a
// block keeps EPT*VEC*8 B per lane in flight instead of one dependent load at a time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_tables.hpp"

namespace sdfs {

constexpr int MAXF = 5;   // block-fixed axis slots
constexpr int MAXN = 32;  // max extent of a contracted axis (2 MFMA row tiles, 8 k-steps)

struct PassDesc {
  // block-fixed axes (slowest first)
  int nfixed;
  int fext[MAXF];
  int foff[MAXF];              // global index of local index 0 (sharded runs)
  long long fstride[MAXF];     // element stride in the (local) grid
  int fq[3][MAXF];             // matrix-index stride of step s's Q tensor
  int fa3[MAXF];               // index stride into the a3 table (only when a3 != nullptr)
  // tile axes, slot 0 slowest .. slot 2 fastest; unused slots have extent 1
  int m[3];
  int toff[3];
  int gstride[3];              // element strides inside the tile (tile span < 2^31)
  int L[3];                    // LDS strides (L[2] == 1)
  int ta3[3];                  // a3 index strides of the tile slots
  // contraction steps
  int nsteps;
  int sslot[3];
  int sn[3];
  int qlds[3];                 // LDS offset (doubles) of step s's staged Q matrix
  const double* Q[3];
  // elementwise stages
  int pro, epi;                // unused (always 0; kept so that the kernels' argument layout stays put): the kernel's MODE says it
  int minus_identity;          // M_JLAST: subtract old[idx]
  double theta, inv_theta, beta;
  // current-state scale a3 applied by the aggregator instead of being folded into the z tensor: set
  // when every slice of a conditional tensor is the same matrix (Rouwenhorst / Tauchen chains), which
  // lets the planner treat that axis as unconditional (longer contiguous runs in the last pass)
  const double* a3;
  long long ntiles;
  int ablate;                  // unused (always 0; kept so that the kernels' argument layout stays put)
  long long ref_off;           // grid offset of the mid-grid point (reference of the fp32 c1 / c2 scaling)
  double lin_ref;              // > 0: use this value as the reference instead (sharded handles: every rank and
                               // both stages must derive the same power of two, sdfs_set_krylov_f32)
};

struct PassIO {
  const double* in;        // grid read by the prologue
  double* out;             // grid written by the epilogue
  const double* aux_in;    // M_JFIRST: c1;  M_JLAST: c2
  double* aux_out;         // M_TFIRST_LIN: c1;  M_TLAST_LIN: c2
  const double* old;       // M_TONLY / M_TLAST / M_TLAST_LIN: w (for the residual);  M_JLAST: v
  unsigned long long* resid;        // M_TONLY / M_TLAST / M_TLAST_LIN: atomicMax target (bits of a non-negative double) or null
  const unsigned long long* gate;   // if non-null and *gate <= tol bits: the iteration has converged, do nothing
  double gate_tol;
  unsigned long long* dbg;          // diagnostic builds (-DSDFS_STAMP): per-phase s_memtime stamps
  double* dotp;                     // M_JLAST with minus_identity: per-block partial sums of <out, v> and <out, out>
                                    // (BiCGSTAB's <t, s>, <t, t>: s is in registers anyway), [2][ntiles], or null
};

typedef double v4d __attribute__((ext_vector_type(4)));
// tile registers as native vectors: a struct double2 moved between address spaces becomes an llvm.memcpy, and a tile
// array that lives across a loop then stays in scratch
typedef double v2d __attribute__((ext_vector_type(2)));

// Grid streams of the pair-plan kernels: every point of a pass is read once and written once, so the 16-byte accesses can
// carry the non-temporal hint (global_load/store_dwordx4 ... nt).  A plain streaming copy of one 512 MB grid gains 6 %
// from it, all of it from the STORES (tools/probes/kernel_bench.hip, profiles/round4_kernel_bench.txt: 5.43-5.54 TB/s
// default policy, 5.51 nt loads only, 5.68 nt stores only, 5.77-5.86 both) -- but inside the operator a pass's output
// is the next pass's input, and what an nt store saves its own kernel the consumer can lose: same-box A/B of whole
// library builds (tools/ab_step.sh, profiles/round4_ab_step.txt): with every store nt the first pass of GCY 20^6 keeps its
// time, the last one gains 3 %, the middle one -- 400 rows of 128 bytes from all over the grid per tile -- LOSES 10 %,
// and 16^6 (134 MB: the intermediates fit the Infinity Cache) loses 4 % overall.  SDFS_NT is a bit mask: 1 loads,
// 2 stores of the slice kernels, 4 stores of the middle line pass, 8 stores of the last line pass.
// SDFS_NT_LD_OFF: the loads' policy per kernel, in the stores' bits -- a kernel named there (the streamed line passes
// pass NT_MID / NT_LAST) keeps the default policy on its loads although bit 0 of SDFS_NT is set.
#ifndef SDFS_NT
#define SDFS_NT 9
#endif
#ifndef SDFS_NT_LD_OFF
#define SDFS_NT_LD_OFF 0
#endif
enum { NT_SLICE = 2, NT_MID = 4, NT_LAST = 8 };
template <int WHO = 0>
__device__ __forceinline__ v2d ldg_stream(const void* p) {
  if ((SDFS_NT & 1) && !(SDFS_NT_LD_OFF & WHO)) return __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p));
  return *reinterpret_cast<const v2d*>(p);
}
template <int WHO>
__device__ __forceinline__ void stg_stream(void* p, const v2d v) {
  if (SDFS_NT & WHO) __builtin_nontemporal_store(v, reinterpret_cast<v2d*>(p));
  else *reinterpret_cast<v2d*>(p) = v;
}
__device__ __forceinline__ double2 ldg_stream2(const void* p) { const v2d t = ldg_stream(p); return make_double2(t.x, t.y); }
template <int WHO>
__device__ __forceinline__ void stg_stream2(void* p, const double2 v) { stg_stream<WHO>(p, (v2d){v.x, v.y}); }

// ---------------------------------------------------------------------------
// pow_fast(x, y) for the two powers of the operator (w^theta and (K S)^(1/theta)).
// x^y = 2^(y log2 x) with log2 x in double-double:
//   x = 2^k z, z in [0.7055, 1.411); 64-entry table of 1/c and log2 c (tools/gen_pow_tables.py);
//   r = fma(z, 1/c, -1), |r| <= 2^-7;  log2 x = k + log2 c + r/ln2 + r^2 P(r)  (Taylor, degree 10)
//   e = y * log2 x (hi + lo);  2^e = 2^(j>>6) * 2^((j&63)/64) * 2^f, |f| <= 2^-7 (Taylor, degree 7)
// Absolute error of y*log2 x stays below ~2^-58 |y|, i.e. ~1 ulp of the result for
// |y| <= 64 (theta = -16, -36 here); tests/test_hip_parity.py checks it against long double.
// The tables live one entry per lane in registers and are gathered with ds_bpermute
// (no LDS memory, no bank conflicts): EVERY lane of the wave must be active at a call.  Six gathers per power since
// round 3 (1/c and the low log part have a zero low word; eight before): the LDS pipe was busy 68 % of the first pass.
// Inputs outside the fast range (x <= 0, NaN, Inf, subnormal, overflow/underflow) take libm pow().
struct PowLane { double invc, lchi, lclo, e2t; };

__device__ __forceinline__ PowLane pow_lane_init(int lane) {
  PowLane T;
  T.invc = POW_INVC[lane]; T.lchi = POW_LOGC_HI[lane]; T.lclo = POW_LOGC_LO[lane]; T.e2t = POW_EXP2T[lane];
  return T;
}

__device__ __forceinline__ double gather64(double v, int idx) {
  const int lo = __builtin_amdgcn_ds_bpermute(idx << 2, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(idx << 2, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
// table entries whose low word is zero by construction (POW_INVC, POW_LOGC_LO: tools/gen_pow_tables.py): one gather
__device__ __forceinline__ double gather_hi(double v, int idx) {
  return __hiloint2double(__builtin_amdgcn_ds_bpermute(idx << 2, __double2hiint(v)), 0);
}

// d = a * b + c with the constant c held in an SGPR pair.  gfx950 VOP3 takes no literal, so a plain
// fma(q, r, CONST) costs two v_mov_b32 per Horner step to build the constant in VGPRs (a third of
// pow's VALU instructions); the scalar move that feeds the SGPR pair issues on the SALU instead.
__device__ __forceinline__ double fma_sc(double a, double b, double c) {
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
  return d;
}

// HIPREC = true : log2 x carried as hi + lo (needed when |y| is large: w^theta, theta = -16 .. -36)
// HIPREC = false: plain double log2 x (enough for |y| < 1: the (K S)^(1/theta) of the aggregator)
template <bool HIPREC>
__device__ __forceinline__ double pow_core(double x, double y, const PowLane& T) {
#pragma clang fp contract(off)
  // subnormal inputs: rescale by 2^64 (exact) and fix the exponent below
  const bool tiny = x < 0x1p-1022;
  const double xs = tiny ? x * 0x1p64 : x;
  const unsigned long long ix = (unsigned long long)__double_as_longlong(xs);
  const unsigned long long tmp = ix - POW_OFF;
  const int i = (int)((tmp >> 46) & 63);
  const double kd = (double)((int)((long long)tmp >> 52) - (tiny ? 64 : 0));
  const double z = __longlong_as_double((long long)(ix - (tmp & 0xfff0000000000000ULL)));
  const double invc = gather_hi(T.invc, i);
  const double lchi = gather64(T.lchi, i);
  const double r = fma(z, invc, -1.0);
  const double t1 = kd + lchi;                         // exact: lchi is a multiple of 2^-40, |kd| < 2^12
  double q = fma_sc(r, POW_L10, POW_L9);
  q = fma_sc(q, r, POW_L8); q = fma_sc(q, r, POW_L7); q = fma_sc(q, r, POW_L6);
  q = fma_sc(q, r, POW_L5); q = fma_sc(q, r, POW_L4); q = fma_sc(q, r, POW_L3); q = fma_sc(q, r, POW_L2);
  const double lclo = gather_hi(T.lclo, i);
  double ehi, elo;
  if (HIPREC) {
    const double p1 = r * POW_INVLN2_HI;
    const double p1e = fma(r, POW_INVLN2_HI, -p1);
    const double hi = t1 + p1;                         // two-sum
    const double bb = hi - t1;
    const double e2 = (t1 - (hi - bb)) + (p1 - bb);
    const double lo = fma(r * r, q, (e2 + p1e) + fma(r, POW_INVLN2_LO, lclo));
    ehi = y * hi;
    elo = fma(y, hi, -ehi) + y * lo;
  } else {
    // |y| < 1: the product and table errors of the hi + lo form are below 2^-60 |y| and dropped;
    // what is kept is the rounding of the final sum (|log2 x| can be ~300 here) and of y * hi
    const double sm = fma(r * r, q, fma(r, POW_INVLN2_HI, lclo));
    const double hi = t1 + sm;
    const double e2 = sm - (hi - t1);                  // fast two-sum (|t1| >= |sm| whenever it matters)
    ehi = y * hi;
    elo = fma(y, hi, -ehi) + y * e2;
  }
  // clamp so that the integer part stays small (over/underflow then saturate in ldexp)
  ehi = fmin(fmax(ehi, -1200.0), 1200.0);
  const double jd = rint(ehi * 64.0);
  const double f = fma(jd, -0.015625, ehi) + elo;
  const int j = (int)jd;
  const double t = gather64(T.e2t, j & 63);
  double p = fma_sc(f, POW_E7, POW_E6);
  p = fma_sc(p, f, POW_E5); p = fma_sc(p, f, POW_E4);
  p = fma_sc(p, f, POW_E3); p = fma_sc(p, f, POW_E2); p = fma_sc(p, f, POW_E1);
  return ldexp(fma(t, p * f, t), j >> 6);
}

// IEEE corner cases of pow for the inputs this path can meet (y finite, y != 0): rare, kept out
// of the straight-line code so that the chains of neighbouring elements interleave
__device__ __forceinline__ bool pow_special(double x) {
  return !(x > 0.0 && x < __longlong_as_double(0x7ff0000000000000LL));
}
__device__ __forceinline__ double pow_fix(double x, double y, double res) {
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  if (pow_special(x)) {
    if (x == 0.0) res = y < 0.0 ? inf : 0.0;
    else if (x == inf) res = y < 0.0 ? 0.0 : inf;
    else res = __longlong_as_double(0x7ff8000000000000LL);   // negative base or NaN
  }
  return res;
}

// N independent powers -- the form the kernels use.  Written step by step across the N elements
// (structure-of-arrays) so that the dependent chains and table gathers of neighbouring elements
// interleave in one basic block.  The straight-line code assumes a positive normal x and a result
// well inside the normal range; anything else (x <= 0, subnormal, Inf, NaN, |y log2 x| >= 1020)
// sends the whole wave through pow_core / pow_fix once more (wave-uniform branch: the gathers need
// every lane active).  Compared with pow_core the fast path
//   * takes index, exponent and mantissa from the high word only (POW_OFF has a zero low word),
//   * gets the rounding error of hi = fma(r, 1/ln2, t1) from d = t1 - hi (exact: t1 is a multiple
//     of 2^-40, |r/ln2| <= 0.0113 < |t1|/2 whenever t1 != 0) and e = fma(r, 1/ln2, d),
//   * stops the log2 Taylor series at r^8 (r^7 when |y| < 1) and the exp2 series at f^6
//     (|r|, |f| <= 2^-7: the first dropped terms are below 2^-65 resp. 2^-58.5 and 2^-65),
//   * rounds y log2 x to a multiple of 1/64 with the 1.5 * 2^46 shift and scales by 2^(j >> 6)
//     with an integer add on the exponent field.
#define SDFS_FORJ _Pragma("unroll") for (int j = 0; j < N; ++j)
__device__ __forceinline__ double gather64b(double v, int byte_idx) {
  const int lo = __builtin_amdgcn_ds_bpermute(byte_idx, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(byte_idx, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double gather_hib(double v, int byte_idx) {      // low word zero by construction
  return __hiloint2double(__builtin_amdgcn_ds_bpermute(byte_idx, __double2hiint(v)), 0);
}
// pow_fast_try: the straight-line path alone.  Returns (per lane) whether any of its N inputs needs the
// full routine; `ehi` is y log2 x as the fast path saw it (the caller's fix-up test).
template <bool HIPREC, int N>
__device__ __forceinline__ bool pow_fast_try(const double (&x)[N], double y, const PowLane& T, double (&res)[N],
                                             double (&ehi)[N]) {
  // every product below that must round on its own is written as a separate statement: the compiler
  // may not fuse it into a neighbouring add (y * hi fused into ehi - kk counts its rounding twice)
#pragma clang fp contract(off)
  constexpr int OFFH = (int)(POW_OFF >> 32);
  constexpr double SHIFT = 0x1.8p46;
  int i4[N], ji[N];
  double kd[N], z[N], invc[N], lchi[N], lclo[N], r[N], t1[N], q[N], elo[N], f[N], t[N], p[N];
  bool rare = false;
  SDFS_FORJ {
    const int hx = __double2hiint(x[j]);
    const int tmph = hx - OFFH;
    rare |= !__builtin_amdgcn_class(x[j], 0x100);      // anything but a positive normal number (one v_cmp_class_f64)
    i4[j] = tmph >> 12;                                // table index * 4; ds_bpermute uses address bits [7:2] only
    kd[j] = (double)(tmph >> 20);
    z[j] = __hiloint2double(hx - (tmph & (int)0xfff00000), __double2loint(x[j]));
  }
  SDFS_FORJ invc[j] = gather_hib(T.invc, i4[j]);
  SDFS_FORJ lchi[j] = gather64b(T.lchi, i4[j]);
  SDFS_FORJ lclo[j] = gather_hib(T.lclo, i4[j]);
  SDFS_FORJ r[j] = fma(z[j], invc[j], -1.0);
  SDFS_FORJ t1[j] = kd[j] + lchi[j];                 // exact: lchi is a multiple of 2^-40, |kd| < 2^11
  if (HIPREC) {
    SDFS_FORJ q[j] = fma_sc(r[j], POW_L8, POW_L7);
    SDFS_FORJ q[j] = fma_sc(q[j], r[j], POW_L6);
  } else {
    SDFS_FORJ q[j] = fma_sc(r[j], POW_L7, POW_L6);
  }
  SDFS_FORJ q[j] = fma_sc(q[j], r[j], POW_L5);
  SDFS_FORJ q[j] = fma_sc(q[j], r[j], POW_L4);
  SDFS_FORJ q[j] = fma_sc(q[j], r[j], POW_L3);
  SDFS_FORJ q[j] = fma_sc(q[j], r[j], POW_L2);
  if (HIPREC) {
    double hi[N], d[N], e[N], lo[N];
    SDFS_FORJ hi[j] = fma(r[j], POW_INVLN2_HI, t1[j]);
    SDFS_FORJ d[j] = t1[j] - hi[j];
    SDFS_FORJ e[j] = fma(r[j], POW_INVLN2_HI, d[j]);
    SDFS_FORJ lo[j] = fma(r[j] * r[j], q[j], e[j] + fma(r[j], POW_INVLN2_LO, lclo[j]));
    SDFS_FORJ ehi[j] = y * hi[j];
    SDFS_FORJ elo[j] = fma(y, lo[j], fma(y, hi[j], -ehi[j]));
  } else {
    double sm[N], hi[N], e2[N];
    SDFS_FORJ sm[j] = fma(r[j] * r[j], q[j], fma(r[j], POW_INVLN2_HI, lclo[j]));
    SDFS_FORJ hi[j] = t1[j] + sm[j];
    SDFS_FORJ e2[j] = sm[j] - (hi[j] - t1[j]);       // fast two-sum (|t1| >= |sm| whenever it matters)
    SDFS_FORJ ehi[j] = y * hi[j];
    SDFS_FORJ elo[j] = fma(y, e2[j], fma(y, hi[j], -ehi[j]));
  }
  SDFS_FORJ rare |= !(fabs(ehi[j]) < 1020.0);
  SDFS_FORJ {
    double kk = ehi[j] + SHIFT;                      // low mantissa bits: round(64 ehi)
    ji[j] = __double2loint(kk);
    kk -= SHIFT;
    f[j] = (ehi[j] - kk) + elo[j];
  }
  SDFS_FORJ t[j] = gather64b(T.e2t, ji[j] << 2);          // lane = (address / 4) mod 64: no mask needed
  SDFS_FORJ p[j] = fma_sc(f[j], POW_E6, POW_E5);
  SDFS_FORJ p[j] = fma_sc(p[j], f[j], POW_E4);
  SDFS_FORJ p[j] = fma_sc(p[j], f[j], POW_E3);
  SDFS_FORJ p[j] = fma_sc(p[j], f[j], POW_E2);
  SDFS_FORJ p[j] = fma_sc(p[j], f[j], POW_E1);
  SDFS_FORJ {
    const double v = fma(t[j], p[j] * f[j], t[j]);
    res[j] = __hiloint2double(__double2hiint(v) + ((ji[j] >> 6) << 20), __double2loint(v));
  }
  return rare;
}

// the full-range answer for one element (IEEE corner cases included): what a wave re-runs when
// pow_fast_try flags a lane
template <bool HIPREC>
__device__ __forceinline__ double pow_full(double x, double y, const PowLane& T) {
  return pow_fix(x, y, pow_core<HIPREC>(x, y, T));
}

template <bool HIPREC, int N>
__device__ __forceinline__ void pow_fast_n(const double (&x)[N], double y, const PowLane& T, double (&res)[N]) {
  double ehi[N];
  const bool rare = pow_fast_try<HIPREC, N>(x, y, T, res, ehi);
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(rare) != 0ULL, 0)) {
    SDFS_FORJ {
      const double c = pow_fix(x[j], y, pow_core<HIPREC>(x[j], y, T));
      const int hx = __double2hiint(x[j]);
      const bool rj = (unsigned)(hx - 0x00100000) >= 0x7fe00000u || !(fabs(ehi[j]) < 1020.0);
      res[j] = rj ? c : res[j];
    }
  }
}
// ---------------------------------------------------------------------------
// powy: x^y with the exponent y FIXED FOR THE LAUNCH (theta in the first pass of T, 1/theta in its last) -- round 4.
// Every term of y log2 x = y k + y log2 c + y log2(1 + r) is scaled by y before the per-element work starts:
//   * lane i keeps  B = high word of y log2 c_i  (21 significant bits, one gather) and  Llo = the rest (a plain double);
//   * y = yhi + ylo with yhi = y's high word, so  t1 = fma(yhi, k, B)  is EXACT (<= 41 significant bits) and everything
//     else -- tlo = fma(ylo, k, Llo), the polynomial y log2(1 + r) = r (c1 + c2 r + ...) with c_j = y a_j held in SGPRs
//     -- stays below ~|y| / 100 in magnitude, where plain double arithmetic is 2^-54 absolute: no double-double
//     anywhere, no product y * hi with its error term, no two-sum;
//   * near-minimax polynomials (tools/gen_pow_tables.py): log2(1 + r) to r^6 (DEG = 6: 1.04e-17 absolute, i.e. |y| times
//     that on x^y -- operator grade: for y = theta the closing 1/theta power divides it out again, 1.2e-17 on T w; for
//     |y| < 1 it is below every rounding) or to r^7 (DEG = 7: 3.8e-20, any |y| <= 64); 2^f to f^5 (2.4e-18);
//   * the exponent arrives as k 2^20 = tmph & 0xfff00000, which the mantissa reduction needs anyway (yhi, ylo carry 2^-20).
// 31 VALU instructions per element against 44 for pow_fast_try (host emulation of both, same operations in the same
// order, against x87 long double: tools/probes/powy_host_check.cpp -- DEG 7 max 2.6e-16 like pow_fast_try's 2.2e-16,
// DEG 6 2.0e-16 for |y| < 1 and 4.4e-16 at y = -36).  Inputs outside the straight-line path (x <= 0, NaN, Inf,
// subnormal, |y log2 x| >= 1020) go through pow_core / pow_fix as before; that branch reloads the general tables.
template <int DEG> struct PowY {
  static_assert(DEG == 6 || DEG == 7, "polynomial degrees of tools/gen_pow_tables.py");
  double invc, B, Llo, e2t;      // per lane (lane = table index)
  double y, yhi, ylo, c[DEG];    // wave-uniform (SGPRs); c[DEG - 2] stays in a VGPR pair (the first Horner step reads two
                                 // coefficients and a VOP3 instruction of gfx950 takes one scalar operand)
};
// d = a * s + c with the multiplier held in an SGPR pair
__device__ __forceinline__ double fma_sm(double a, double s, double c) {
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(s), "v"(c));
  return d;
}
// a wave-uniform double into an SGPR pair.  (Opaque to the optimiser on purpose: with the readfirstlane builtin the
// compiler proves the value uniform, drops the move and then keeps all nine constants of the routine in VGPR pairs --
// fourteen registers the walking slice kernel does not have.)
__device__ __forceinline__ double uniform_f64(double v) {
  // (the hazard recogniser does not look inside inline assembly: without the s_nop in front, a readfirstlane issued
  // right behind the fp64 instruction that produces its operand read the register's previous contents -- constants off
  // in their low word, 1e-13 .. 3e-6 relative on the power, caught by kernel_bench's comparison with the general routine)
  int lo, hi;
  asm volatile("s_nop 7\n\tv_readfirstlane_b32 %0, %2\n\tv_readfirstlane_b32 %1, %3\n\ts_nop 3"
               : "=&s"(lo), "=&s"(hi) : "v"(__double2loint(v)), "v"(__double2hiint(v)));
  return __hiloint2double(hi, lo);
}
template <int DEG>
__device__ __forceinline__ PowY<DEG> powy_init(double y, int lane) {
#pragma clang fp contract(off)
  PowY<DEG> T;
  T.invc = POW_INVC[lane]; T.e2t = POW_EXP2T[lane];
  const double lchi = POW_LOGC_HI[lane], lclo = POW_LOGC_LO[lane];
  const double p = y * lchi;
  const double e = fma(y, lclo, fma(y, lchi, -p));     // y (lchi + lclo) = p + e
  T.B = __hiloint2double(__double2hiint(p), 0);
  T.Llo = (p - T.B) + e;                               // p - B is exact
  T.y = y;
  const double yh = __hiloint2double(__double2hiint(y), 0);
  T.yhi = uniform_f64(yh * 0x1p-20);
  T.ylo = uniform_f64((y - yh) * 0x1p-20);
  if (DEG == 6) {
    const double a[6] = {0.0, POW_A6_2, POW_A6_3, POW_A6_4, POW_A6_5, POW_A6_6};
    T.c[0] = uniform_f64(fma(y, POW_A6_1_LO, y * POW_A6_1_HI));
#pragma unroll
    for (int j = 1; j < 6; ++j) T.c[j] = j == DEG - 2 ? y * a[j] : uniform_f64(y * a[j]);
  } else {
    const double a[7] = {0.0, POW_A7_2, POW_A7_3, POW_A7_4, POW_A7_5, POW_A7_6, POW_A7_7};
    T.c[0] = uniform_f64(fma(y, POW_A7_1_LO, y * POW_A7_1_HI));
#pragma unroll
    for (int j = 1; j < DEG; ++j) T.c[j] = j == DEG - 2 ? y * a[j] : uniform_f64(y * a[j]);
  }
  return T;
}
#define SDFS_FORJ _Pragma("unroll") for (int j = 0; j < N; ++j)
// the straight-line path for N elements (structure of arrays: the chains and gathers of neighbours interleave);
// returns (per lane) whether any input needs the full routine, ts = y log2 x as this path saw it
template <int DEG, int N>
__device__ __forceinline__ bool powy_try(const double (&x)[N], const PowY<DEG>& T, double (&res)[N], double (&ts)[N]) {
#pragma clang fp contract(off)
  constexpr int OFFH = (int)(POW_OFF >> 32);
  constexpr double SHIFT = 0x1.8p46;
  int i4[N], ji[N];
  double kd[N], z[N], invc[N], B[N], Llo[N], r[N], t1[N], u[N], q[N], f[N], t[N], p[N];
  bool rare = false;
  SDFS_FORJ {
    const int hx = __double2hiint(x[j]);
    const int tmph = hx - OFFH;
    rare |= !__builtin_amdgcn_class(x[j], 0x100);      // anything but a positive normal number
    i4[j] = tmph >> 12;                                // table index * 4 (ds_bpermute reads address bits [7:2])
    const int m = tmph & (int)0xfff00000;
    kd[j] = (double)m;                                 // k 2^20
    z[j] = __hiloint2double(hx - m, __double2loint(x[j]));
  }
  SDFS_FORJ invc[j] = gather_hib(T.invc, i4[j]);
  SDFS_FORJ B[j] = gather_hib(T.B, i4[j]);
  SDFS_FORJ Llo[j] = gather64b(T.Llo, i4[j]);
  SDFS_FORJ r[j] = fma(z[j], invc[j], -1.0);
  SDFS_FORJ t1[j] = fma_sm(kd[j], T.yhi, B[j]);        // exact
  SDFS_FORJ u[j] = fma_sm(kd[j], T.ylo, Llo[j]);
  SDFS_FORJ q[j] = fma_sm(r[j], T.c[DEG - 1], T.c[DEG - 2]);
#pragma unroll
  for (int d = DEG - 3; d >= 0; --d) { SDFS_FORJ q[j] = fma_sc(q[j], r[j], T.c[d]); }
  SDFS_FORJ u[j] = fma(q[j], r[j], u[j]);
  SDFS_FORJ ts[j] = t1[j] + u[j];
  SDFS_FORJ rare |= !(fabs(ts[j]) < 1020.0);
  SDFS_FORJ {
    double kk = ts[j] + SHIFT;                         // low mantissa bits: round(64 ts)
    ji[j] = __double2loint(kk);
    kk -= SHIFT;
    f[j] = (t1[j] - kk) + u[j];                        // t1 - kk is exact
  }
  SDFS_FORJ t[j] = gather64b(T.e2t, ji[j] << 2);
  SDFS_FORJ p[j] = fma_sc(f[j], POW_X5_5, POW_X5_4);
  SDFS_FORJ p[j] = fma_sc(p[j], f[j], POW_X5_3);
  SDFS_FORJ p[j] = fma_sc(p[j], f[j], POW_X5_2);
  SDFS_FORJ p[j] = fma_sc(p[j], f[j], POW_X5_1);
  SDFS_FORJ {
    const double v = fma(t[j], p[j] * f[j], t[j]);
    res[j] = __hiloint2double(__double2hiint(v) + ((ji[j] & ~63) << 14), __double2loint(v));
  }
  return rare;
}
template <int DEG, int N>
__device__ __forceinline__ void powy_n(const double (&x)[N], const PowY<DEG>& T, double (&res)[N]) {
  double ts[N];
  const bool rare = powy_try<DEG, N>(x, T, res, ts);
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(rare) != 0ULL, 0)) {
    const PowLane PT = pow_lane_init((int)(threadIdx.x & 63));
    SDFS_FORJ {
      const double c = pow_fix(x[j], T.y, pow_core<true>(x[j], T.y, PT));
      const int hx = __double2hiint(x[j]);
      const bool rj = (unsigned)(hx - 0x00100000) >= 0x7fe00000u || !(fabs(ts[j]) < 1020.0);
      res[j] = rj ? c : res[j];
    }
  }
}
#undef SDFS_FORJ

// The power of a kernel whose exponent is fixed for the launch: powy (default) or, with -DSDFS_POWY=0 (A/B builds of
// tools/probes/kernel_bench.hip), the general routine.  HIPREC only matters to the latter.
#ifndef SDFS_POWY
#define SDFS_POWY 1
#endif
template <bool HIPREC> struct PowK {
#if SDFS_POWY
  PowY<6> T;
  __device__ __forceinline__ void init(double y, int lane) { T = powy_init<6>(y, lane); }
  template <int N> __device__ __forceinline__ void run(const double (&x)[N], double (&res)[N]) const { powy_n<6, N>(x, T, res); }
#else
  PowLane T;
  double y;
  __device__ __forceinline__ void init(double y_, int lane) { T = pow_lane_init(lane); y = y_; }
  template <int N> __device__ __forceinline__ void run(const double (&x)[N], double (&res)[N]) const { pow_fast_n<HIPREC, N>(x, y, T, res); }
#endif
};

// XCD-aware block -> tile map: blocks b, b+8, b+16.. share an XCD (round-robin
// dispatch), so give each XCD one contiguous chunk of tiles: neighbouring tiles
// share 128-B lines and Q matrices in that XCD's L2.  Bijective for any count.
__device__ __forceinline__ long long xcd_remap(long long b, long long n) {
  const long long q = n >> 3, r = n & 7;
  const long long x = b & 7, k = b >> 3;
  const long long start = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return start + k;
}

// walks the units (VEC consecutive doubles along slot 2) a thread owns: tid, tid+B, ...
struct Walker {
  int t0, t1, t2u;
  int d0, d1, d2u, m1, m2u;
  __device__ __forceinline__ void init(int tid, int B, int m1_, int m2u_) {
    // opaque copy: every phase recomputes its (cheap) coordinates instead of keeping the
    // previous phase's address registers alive across the MFMA/pow stages (that spilled)
    asm volatile("" : "+v"(tid));
    m1 = m1_; m2u = m2u_;
    t2u = tid % m2u; int r = tid / m2u; t1 = r % m1; t0 = r / m1;
    d2u = B % m2u; r = B / m2u; d1 = r % m1; d0 = r / m1;
  }
  __device__ __forceinline__ void next() {
    t2u += d2u; int c = t2u >= m2u; t2u -= c ? m2u : 0;
    t1 += d1 + c; c = t1 >= m1; t1 -= c ? m1 : 0;
    t0 += d0 + c;
  }
};

template <int VEC> struct VecT;
template <> struct VecT<1> {
  double v[1];
  __device__ __forceinline__ void load(const double* p) { v[0] = *p; }
  __device__ __forceinline__ void store(double* p) const { *p = v[0]; }
  __device__ __forceinline__ void load(const float* p) { v[0] = (double)*p; }
  __device__ __forceinline__ void store(float* p) const { *p = (float)v[0]; }
};
template <> struct VecT<2> {
  double v[2];
  __device__ __forceinline__ void load(const double* p) {
    const double2 t = *reinterpret_cast<const double2*>(p); v[0] = t.x; v[1] = t.y; }
  __device__ __forceinline__ void store(double* p) const {
    double2 t; t.x = v[0]; t.y = v[1]; *reinterpret_cast<double2*>(p) = t; }
  __device__ __forceinline__ void load(const float* p) {
    const float2 t = *reinterpret_cast<const float2*>(p); v[0] = (double)t.x; v[1] = (double)t.y; }
  __device__ __forceinline__ void store(float* p) const {
    float2 t; t.x = (float)v[0]; t.y = (float)v[1]; *reinterpret_cast<float2*>(p) = t; }
};

// four points per unit: the 16-byte access of the fp32 streams (LDS side: two double2)
template <> struct VecT<4> {
  double v[4];
  __device__ __forceinline__ void load(const double* p) {
    const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; }
  __device__ __forceinline__ void store(double* p) const {
    double2 a, b; a.x = v[0]; a.y = v[1]; b.x = v[2]; b.y = v[3];
    *reinterpret_cast<double2*>(p) = a; *reinterpret_cast<double2*>(p + 2) = b; }
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = (double)t.x; v[1] = (double)t.y; v[2] = (double)t.z; v[3] = (double)t.w; }
  __device__ __forceinline__ void store(float* p) const {
    float4 t; t.x = (float)v[0]; t.y = (float)v[1]; t.z = (float)v[2]; t.w = (float)v[3];
    *reinterpret_cast<float4*>(p) = t; }
};

// A grid stream is fp64 by default; under PREC = 1 (fp32 Krylov storage) the streams of
// the J.v path hold floats behind the same pointer fields.  Arithmetic stays fp64 either way.
template <bool F32, int VEC>
__device__ __forceinline__ void gload(VecT<VEC>& v, const double* base, long long off) {
  if (F32) v.load(reinterpret_cast<const float*>(base) + off); else v.load(base + off);
}
template <bool F32, int VEC>
__device__ __forceinline__ void gstore(const VecT<VEC>& v, double* base, long long off) {
  if (F32) v.store(reinterpret_cast<float*>(base) + off); else v.store(base + off);
}

// One contraction y[i, col] = sum_I Q[i, I] x[I, col] over the columns of the LDS tile.
// Output rows are covered by N16 row tiles of v_mfma_f64_16x16x4_f64 (64 cycles, 16 rows)
// plus N4 row tiles of v_mfma_f64_4x4x4_4b_f64 (20 cycles, 4 rows x 4 blocks of 4 columns):
// for n = 20 that is 84 cycles per k-step instead of 128 for two 16-row tiles.  Both shapes
// take the same B operand (lane l holds x[4kk + (l>>4)][col0 + (l&15)]).
//   n <= 12: (0, ceil(n/4));  13..16: (1, 0);  17..24: (1, ceil((n-16)/4));  25..32: (2, 0)
// Everything that does not depend on the column tile is hoisted: the masked Q fragments sit
// in registers, the row offsets of the B reads are precomputed (clamped in range), and the
// column -> LDS offset map advances incrementally (no division in the loop).  The loop body
// is then one address add + one ds_read_b64 per k-step next to the MFMAs.
template <int N16, int N4>
__device__ __forceinline__ void contract_cols(double* __restrict__ lds, const double* __restrict__ Qm,
                                              const int n, const int Ls, const int Lu,
                                              const int Lv, const int mv, const int ncols,
                                              const int lane, const int wave, const int nwaves) {
  constexpr int A16 = N16 > 0 ? N16 : 1, A4 = N4 > 0 ? N4 : 1;
  const int li = lane & 15, lk = lane >> 4, l4 = lane & 3;
  constexpr int rb = 16 * N16;
  // k-steps are a compile-time count per shape (the Q fragments of steps past n are zero), so the
  // trip below is one basic block: every B read is issued before the first MFMA waits on one
  constexpr int KT = N16 == 2 ? 8 : 4 * N16 + N4;
  double a16[A16][KT], a4[A4][KT];
  int roff[KT];
#pragma unroll
  for (int kk = 0; kk < KT; ++kk) {
    const int I0 = 4 * kk + lk;
    const bool iok = I0 < n;
    const int I = iok ? I0 : n - 1;          // rows >= n meet zero Q columns; keep the read in bounds
    roff[kk] = I * Ls;
#pragma unroll
    for (int t = 0; t < N16; ++t) {
      const int row = 16 * t + li;
      a16[t][kk] = (iok && row < n) ? Qm[row * n + I] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < N4; ++t) {
      const int row = rb + 4 * t + l4;
      a4[t][kk] = (iok && row < n) ? Qm[row * n + I] : 0.0;
    }
  }
  // column walk: col = ct*16 + li, advancing by 16*nwaves per trip
  int col = wave * 16 + li;
  int cu = col / mv, cv = col - cu * mv;
  const int adv = 16 * nwaves;
  const int du = adv / mv, dv = adv - du * mv;

  for (int ct = wave; ct * 16 < ncols; ct += nwaves) {
    const bool colok = col < ncols;
    const int cbase = colok ? cu * Lu + cv * Lv : (ncols - 1) / mv * Lu + ((ncols - 1) % mv) * Lv;
    v4d acc[A16];
    double d[A4];
#pragma unroll
    for (int t = 0; t < A16; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < A4; ++t) d[t] = 0.0;
    double b[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) b[kk] = lds[cbase + roff[kk]];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) {
#pragma unroll
      for (int t = 0; t < N16; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a16[t][kk], b[kk], acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < N4; ++t) d[t] = __builtin_amdgcn_mfma_f64_4x4x4f64(a4[t][kk], b[kk], d[t], 0, 0, 0);
    }
    if (colok) {
      // 16x16x4 D map: col = lane&15, row = (lane>>4) + 4*reg
#pragma unroll
      for (int t = 0; t < N16; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * t + lk + 4 * r;
          if (i < n) lds[cbase + i * Ls] = acc[t][r];
        }
      }
      // 4x4x4_4b D map: lane = i*16 + blk*4 + j -> row = lane>>4, col = lane&15 (one value per lane)
#pragma unroll
      for (int t = 0; t < N4; ++t) {
        const int i = rb + 4 * t + lk;
        if (i < n) lds[cbase + i * Ls] = d[t];
      }
    }
    col += adv;
    cv += dv; const int c = cv >= mv; cv -= c ? mv : 0; cu += du + c;
  }
}

__device__ __forceinline__ void contract_step(double* __restrict__ lds, const PassDesc& P, const int s,
                                              const int lane, const int wave, const int nwaves) {
  const int slot = P.sslot[s];
  const int n = P.sn[s];
  const double* __restrict__ Qm = lds + P.qlds[s];
  int Ls, Lu, Lv, mu, mv;
  if (slot == 0) { Ls = P.L[0]; Lu = P.L[1]; mu = P.m[1]; Lv = 1; mv = P.m[2]; }
  else if (slot == 1) { Ls = P.L[1]; Lu = P.L[0]; mu = P.m[0]; Lv = 1; mv = P.m[2]; }
  else { Ls = 1; Lu = P.L[0]; mu = P.m[0]; Lv = P.L[1]; mv = P.m[1]; }
  const int ncols = mu * mv;
#define SDFS_CC(A, B4) contract_cols<A, B4>(lds, Qm, n, Ls, Lu, Lv, mv, ncols, lane, wave, nwaves)
  if (n <= 4) SDFS_CC(0, 1);
  else if (n <= 8) SDFS_CC(0, 2);
  else if (n <= 12) SDFS_CC(0, 3);
  else if (n <= 16) SDFS_CC(1, 0);
  else if (n <= 20) SDFS_CC(1, 1);
  else if (n <= 24) SDFS_CC(1, 2);
  else SDFS_CC(2, 0);
#undef SDFS_CC
}

#ifdef SDFS_STAMP
#define STAMP(slot)                                                                        \
  do {                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    unsigned long long t_;                                                                 \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");             \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    if (io.dbg != nullptr && threadIdx.x == 0 && blockIdx.x < 64 && trip < 2)              \
      io.dbg[(blockIdx.x * 2 + trip) * 16 + (slot)] = t_;                                   \
  } while (0)
#else
#define STAMP(slot) do {} while (0)
#endif

// Compile-time role of a launch inside one operator application.
enum PassMode { M_MID = 0, M_TFIRST = 1, M_TLAST = 2, M_TONLY = 3, M_JFIRST = 4, M_JLAST = 5,
                M_TFIRST_LIN = 6, M_TLAST_LIN = 7, M_NMODES = 8 };

struct TileCtx {
  long long gbase;
  int q0, q1, q2;
  int ia3b;
};

__device__ __forceinline__ TileCtx decode_tile(const PassDesc& P, long long tile) {
  TileCtx c;
  c.gbase = 0; c.q0 = 0; c.q1 = 0; c.q2 = 0; c.ia3b = 0;
#pragma unroll
  for (int k = MAXF - 1; k >= 0; --k) {
    if (k < P.nfixed) {
      const int e = P.fext[k];
      const int cc = (int)(tile % e);
      tile /= e;
      const int gc = cc + P.foff[k];
      c.gbase += (long long)cc * P.fstride[k];
      c.q0 += gc * P.fq[0][k]; c.q1 += gc * P.fq[1][k]; c.q2 += gc * P.fq[2][k];
      c.ia3b += gc * P.fa3[k];
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) c.ia3b += P.toff[j] * P.ta3[j];
  return c;
}

// One workgroup per tile.  Phases (each thread revisits the same EPT units of VEC doubles):
//   load   : all global loads of the thread issued back to back (tile, c1 for the JVP, and the
//            transition matrices of the block's steps), then parked in LDS
//   pow    : x = w^theta in place in LDS (first pass of T)
//   MFMA   : up to three contractions in place in LDS
//   pow    : Tw = 1 + beta S^(1/theta) in place in LDS (last pass of T)
//   store  : residual / JVP scaling and the global store
// Two 512-thread workgroups share a CU (LDS-limited), so one block's memory phases overlap the
// other's MFMA / pow phases.  MODE is the compile-time role of the launch.
template <int EPT, int VEC, int MODE, int PREC = 0>
__global__ void __launch_bounds__(512, 4)
pass_kernel(const PassDesc P, const PassIO io) {
  // PREC = 1: the J.v streams (v, the intermediate grid, c1, c2, the result) are fp32; a linearising
  // application of T keeps its own streams fp64 and only writes c1 / c2 as fp32
  constexpr bool JV = PREC == 1 && (MODE == M_JFIRST || MODE == M_MID || MODE == M_JLAST);
  constexpr bool F_IN = JV, F_OUT = JV, F_OLD = JV, F_AUXIN = JV;
  constexpr bool F_AUXOUT = PREC == 1 && (MODE == M_TFIRST_LIN || MODE == M_TLAST_LIN);
  constexpr bool POWP = (MODE == M_TFIRST || MODE == M_TONLY || MODE == M_TFIRST_LIN);   // x = a1 w^theta
  constexpr bool CES = (MODE == M_TLAST || MODE == M_TONLY || MODE == M_TLAST_LIN);      // Tw = 1 + beta (K S)^(1/theta)
  constexpr bool LINP = (MODE == M_TFIRST_LIN);                  // also write c1 = a1 w^(theta-1)
  constexpr bool LINE = (MODE == M_TLAST_LIN);                   // also write c2 = beta u / S
  constexpr bool MULP = (MODE == M_JFIRST);                      // x = c1 * v
  constexpr bool MULE = (MODE == M_JLAST);                       // out = c2 * y (- v)
  constexpr int NAUX = MULP ? EPT : 1;
  constexpr int NC2 = MULE ? EPT : 1;
  extern __shared__ double lds[];
  __shared__ double red[16];

  if (io.gate != nullptr) {
    const unsigned long long g = *io.gate;
    if (g <= (unsigned long long)__double_as_longlong(io.gate_tol)) return;
  }

  const int tid = threadIdx.x;
  const int B = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nwaves = B >> 6;
  const int trip = 0;
  (void)trip;

  const TileCtx cur = decode_tile(P, xcd_remap((long long)blockIdx.x, P.ntiles));

  const int m1 = P.m[1];
  const int m2u = P.m[2] / VEC;
  const int tot = P.m[0] * m1 * m2u;          // units of VEC doubles
  const int iters = (tot + B - 1) / B;
  const int L0 = P.L[0], L1 = P.L[1];
  const int g0 = P.gstride[0], g1 = P.gstride[1], g2 = P.gstride[2];

  STAMP(0);
  // ---- load phase ------------------------------------------------------------------
  {
    // transition matrices first (they come from L2; vmcnt retires in order)
    const int nq0 = P.nsteps > 0 ? P.sn[0] * P.sn[0] : 0;
    const int nq1 = P.nsteps > 1 ? P.sn[1] * P.sn[1] : 0;
    const int nq2 = P.nsteps > 2 ? P.sn[2] * P.sn[2] : 0;
    const double* Q0 = P.Q[0] + (long long)cur.q0 * nq0;
    const double* Q1 = P.Q[1] + (long long)cur.q1 * nq1;
    const double* Q2 = P.Q[2] + (long long)cur.q2 * nq2;
    double qv0[2], qv1[2], qv2[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = tid + r * B;
      qv0[r] = i < nq0 ? Q0[i] : 0.0;
      qv1[r] = i < nq1 ? Q1[i] : 0.0;
      qv2[r] = i < nq2 ? Q2[i] : 0.0;
    }
    VecT<VEC> val[EPT];
    VecT<VEC> aux[NAUX];
    Walker wk;
    wk.init(tid, B, m1, m2u);
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      if (tid + k * B < tot) {
        const int go = wk.t0 * g0 + wk.t1 * g1 + wk.t2u * VEC * g2;
        gload<F_IN>(val[k], io.in, cur.gbase + go);
        if (MULP) gload<F_AUXIN>(aux[MULP ? k : 0], io.aux_in, cur.gbase + go);
      }
      wk.next();
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = tid + r * B;
      if (i < nq0) lds[P.qlds[0] + i] = qv0[r];
      if (i < nq1) lds[P.qlds[1] + i] = qv1[r];
      if (i < nq2) lds[P.qlds[2] + i] = qv2[r];
    }
    // matrices larger than 2*B entries (n = 32 with small blocks): plain loop for the rest
    for (int i = tid + 2 * B; i < nq0; i += B) lds[P.qlds[0] + i] = Q0[i];
    for (int i = tid + 2 * B; i < nq1; i += B) lds[P.qlds[1] + i] = Q1[i];
    for (int i = tid + 2 * B; i < nq2; i += B) lds[P.qlds[2] + i] = Q2[i];
    STAMP(1);
    wk.init(tid, B, m1, m2u);
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      if (tid + k * B < tot) {
        if (MULP) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) val[k].v[j] *= aux[MULP ? k : 0].v[j];
        }
        val[k].store(lds + wk.t0 * L0 + wk.t1 * L1 + wk.t2u * VEC);
      }
      wk.next();
    }
  }
  STAMP(2);

  PowLane PT;
  if (POWP || CES) PT = pow_lane_init(lane);

  // fp32 c1 / c2: c1 = w^(theta-1) is ~1e-50 and c2 ~1e+50 at theta = -16 .. -36 -- outside fp32 -- while
  // only their product matters.  Both are stored scaled by an exact power of two taken from the point in
  // the middle of the grid (c1 * 2^k, c2 * 2^-k, k = -ilogb(w_mid^(theta-1)); the middle, so that the
  // spread (w / w_mid)^(theta-1) splits evenly over fp32's range): the first pass reads w_mid from its
  // input, the last pass from the grid it forms the residual against, so both arrive at the same k.
  double lin_scale = 1.0;
  if (F_AUXOUT) {
    const double wref[1] = {P.lin_ref > 0.0 ? P.lin_ref : (LINP ? io.in[P.ref_off] : io.old[P.ref_off])};
    double xr[1];
    pow_fast_n<true, 1>(wref, P.theta, PT, xr);
    const int k = -ilogb(xr[0] / wref[0]);
    lin_scale = ldexp(1.0, LINP ? k : -k);
  }

  // ---- prologue x = a1 w^theta, in place in LDS (each thread revisits its own units).
  //      Uniform trip count: pow_fast needs every lane of the wave active.
  if (POWP) {
    Walker wk;
    wk.init(tid, B, m1, m2u);
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
      const bool valid = tid + it * B < tot;
      const int t2 = wk.t2u * VEC;
      const int lo = valid ? wk.t0 * L0 + wk.t1 * L1 + t2 : 0;
      VecT<VEC> x, c1;
      x.load(lds + lo);
      double xin[VEC], xw[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) xin[j] = valid ? x.v[j] : 1.0;
      pow_fast_n<true, VEC>(xin, P.theta, PT, xw);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if (LINP) c1.v[j] = xw[j] / xin[j] * lin_scale;         // c1 = w^(theta-1)
        x.v[j] = xw[j];
      }
      if (valid) {
        x.store(lds + lo);
        if (LINP) gstore<F_AUXOUT>(c1, io.aux_out, cur.gbase + wk.t0 * g0 + wk.t1 * g1 + t2 * g2);
      }
      wk.next();
    }
  }
  STAMP(3);
  __syncthreads();
  STAMP(4);

  // ---- contractions ------------------------------------------------------------------
  if (P.nsteps > 0) { contract_step(lds, P, 0, lane, wave, nwaves); STAMP(5); __syncthreads(); }
  STAMP(6);
  if (P.nsteps > 1) { contract_step(lds, P, 1, lane, wave, nwaves); STAMP(7); __syncthreads(); }
  STAMP(8);
  if (P.nsteps > 2) { contract_step(lds, P, 2, lane, wave, nwaves); STAMP(9); __syncthreads(); }
  STAMP(10);

  // ---- aggregator Tw = 1 + beta (K S)^(1/theta), in place in LDS (rolled, uniform) ------
  if (CES) {
    Walker wk;
    wk.init(tid, B, m1, m2u);
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
      const bool valid = tid + it * B < tot;
      const int t2 = wk.t2u * VEC;
      const int lo = valid ? wk.t0 * L0 + wk.t1 * L1 + t2 : 0;
      VecT<VEC> y, c2;
      y.load(lds + lo);
      double sv[VEC], ks[VEC], uu[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) { sv[j] = valid ? y.v[j] : 1.0; ks[j] = sv[j]; }
      if (P.a3 != nullptr && valid) {
        const int i3 = cur.ia3b + wk.t0 * P.ta3[0] + wk.t1 * P.ta3[1] + t2 * P.ta3[2];
#pragma unroll
        for (int j = 0; j < VEC; ++j) ks[j] = P.a3[i3 + j * P.ta3[2]] * sv[j];
      }
      pow_fast_n<false, VEC>(ks, P.inv_theta, PT, uu);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        if (LINE) c2.v[j] = P.beta * uu[j] / sv[j] * lin_scale; // c2 = beta a3 (a3 S)^(1/theta-1) = beta u / S (S unscaled)
        y.v[j] = 1.0 + P.beta * uu[j];
      }
      if (valid) {
        y.store(lds + lo);
        if (LINE) gstore<F_AUXOUT>(c2, io.aux_out, cur.gbase + wk.t0 * g0 + wk.t1 * g1 + t2 * g2);
      }
      wk.next();
    }
  }
  STAMP(11);

  // ---- residual / scaling and the global store -------------------------------------------
  const bool need_old = CES ? (io.resid != nullptr) : (MULE && P.minus_identity);
  double rmax = 0.0;
  double dot_yv = 0.0, dot_yy = 0.0;
  {
    VecT<VEC> oldv[EPT];
    VecT<VEC> c2v[NC2];
    Walker wk;
    if (CES || MULE) {
      wk.init(tid, B, m1, m2u);
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
        if (tid + k * B < tot) {
          const int go = wk.t0 * g0 + wk.t1 * g1 + wk.t2u * VEC * g2;
          if (need_old) gload<F_OLD>(oldv[k], io.old, cur.gbase + go);
          if (MULE) gload<F_AUXIN>(c2v[MULE ? k : 0], io.aux_in, cur.gbase + go);
        }
        wk.next();
      }
    }
    wk.init(tid, B, m1, m2u);
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      if (tid + k * B < tot) {
        const int t2 = wk.t2u * VEC;
        const int go = wk.t0 * g0 + wk.t1 * g1 + t2 * g2;
        VecT<VEC> y;
        y.load(lds + wk.t0 * L0 + wk.t1 * L1 + t2);
        if (MULE) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            y.v[j] *= c2v[MULE ? k : 0].v[j];
            if (P.minus_identity) {
              y.v[j] -= oldv[k].v[j];
              // what gets stored is what the dots refer to (fp32 storage rounds first)
              const double yr = F_OUT ? (double)(float)y.v[j] : y.v[j];
              dot_yv = fma(yr, oldv[k].v[j], dot_yv);
              dot_yy = fma(yr, yr, dot_yy);
            }
          }
        } else if (CES && need_old) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            double r = fabs(y.v[j] - oldv[k].v[j]);
            if (!(r == r)) r = __longlong_as_double(0x7ff0000000000000LL);   // NaN -> +inf
            rmax = fmax(rmax, r);
          }
        }
        gstore<F_OUT>(y, io.out, cur.gbase + go);
      }
      wk.next();
    }
  }
  STAMP(12);

  if (MULE && io.dotp != nullptr) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { dot_yv += __shfl_xor(dot_yv, o); dot_yy += __shfl_xor(dot_yy, o); }
    if (lane == 0) { red[wave] = dot_yv; red[8 + wave] = dot_yy; }
    __syncthreads();
    if (tid == 0) {
      double a = 0.0, b = 0.0;
      for (int w = 0; w < nwaves; ++w) { a += red[w]; b += red[8 + w]; }
      io.dotp[blockIdx.x] = a;
      io.dotp[P.ntiles + blockIdx.x] = b;
    }
  }
  if (CES && io.resid != nullptr) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, o));
    if (lane == 0) red[wave] = rmax;
    __syncthreads();
    if (tid == 0) {
      double r = red[0];
      for (int w = 1; w < nwaves; ++w) r = fmax(r, red[w]);
      atomicMax(io.resid, (unsigned long long)__double_as_longlong(r));
    }
  }
}

// (not a template: defined once, in sdfs_api.hip's translation unit; cont_ptan.hip leaves it out)
#ifndef SDFS_NO_DEBUG_POW_KERNEL
// test hook: out[i] = pow_fast(x[i], y) (n padded so that whole waves run); deg = 6 / 7: the pre-scaled routine powy
__global__ void __launch_bounds__(256) debug_pow_kernel(const double* __restrict__ x, double y,
                                                        double* __restrict__ out, long long n, int deg) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const double xv = i < n ? x[i] : 1.0;
  const double xin[1] = {xv};
  double r[1];
  if (deg == 6) {
    const PowY<6> T = powy_init<6>(y, threadIdx.x & 63);
    powy_n<6, 1>(xin, T, r);
  } else if (deg == 7) {
    const PowY<7> T = powy_init<7>(y, threadIdx.x & 63);
    powy_n<7, 1>(xin, T, r);
  } else {
    const PowLane PT = pow_lane_init(threadIdx.x & 63);
    if (fabs(y) < 1.0) pow_fast_n<false, 1>(xin, y, PT, r); else pow_fast_n<true, 1>(xin, y, PT, r);
  }
  if (i < n) out[i] = r[0];
}
#endif

typedef void (*pass_fn)(const PassDesc, const PassIO);

#ifndef SDFS_NO_VARIANT_TABLES   // (tools/probes/kernel_bench.hip names its kernels itself: referencing a variant instantiates it)

// EPT in {1,2,4,8,16}, VEC in {1,2}, MODE in PassMode, PREC in {0, 1}
template <int MODE, int PREC>
inline pass_fn pass_kernel_variant_m(int ept, int vec) {
  // VEC = 4 exists only where every global stream of the launch is fp32 (the J.v passes under PREC = 1)
  if constexpr (PREC == 1 && (MODE == M_JFIRST || MODE == M_MID || MODE == M_JLAST)) {
    if (vec == 4) {
      switch (ept) {
        case 1: return (pass_fn)pass_kernel<1, 4, MODE, PREC>;
        case 2: return (pass_fn)pass_kernel<2, 4, MODE, PREC>;
        case 4: return (pass_fn)pass_kernel<4, 4, MODE, PREC>;
        default: return nullptr;          // eight float4 units + their scaling stream spill: the planner stops at four
      }
    }
  }
  if (vec == 4) return nullptr;
#define SDFS_V(E) (vec == 2 ? (pass_fn)pass_kernel<E, 2, MODE, PREC> : (pass_fn)pass_kernel<E, 1, MODE, PREC>)
  switch (ept) {
    case 1: return SDFS_V(1);
    case 2: return SDFS_V(2);
    case 4: return SDFS_V(4);
    case 8: return SDFS_V(8);
    case 16:
      // sixteen double2 units spill in the J.v roles (tile + scaling stream in flight); the planner widens the
      // block instead, so only the 8-byte form exists there
      if constexpr (MODE == M_JFIRST || MODE == M_JLAST) return vec == 2 ? nullptr : (pass_fn)pass_kernel<16, 1, MODE, PREC>;
      else return SDFS_V(16);
    default: return nullptr;
  }
#undef SDFS_V
}
inline pass_fn pass_kernel_variant(int ept, int vec, int mode, int prec = 0) {
  if (prec == 1) {
    switch (mode) {                        // only the modes of the J.v path and of the linearisation
      case M_MID: return pass_kernel_variant_m<M_MID, 1>(ept, vec);
      case M_JFIRST: return pass_kernel_variant_m<M_JFIRST, 1>(ept, vec);
      case M_JLAST: return pass_kernel_variant_m<M_JLAST, 1>(ept, vec);
      case M_TFIRST_LIN: return pass_kernel_variant_m<M_TFIRST_LIN, 1>(ept, vec);
      case M_TLAST_LIN: return pass_kernel_variant_m<M_TLAST_LIN, 1>(ept, vec);
      default: return nullptr;
    }
  }
  switch (mode) {
    case M_MID: return pass_kernel_variant_m<M_MID, 0>(ept, vec);
    case M_TFIRST: return pass_kernel_variant_m<M_TFIRST, 0>(ept, vec);
    case M_TLAST: return pass_kernel_variant_m<M_TLAST, 0>(ept, vec);
    case M_TONLY: return pass_kernel_variant_m<M_TONLY, 0>(ept, vec);
    case M_JFIRST: return pass_kernel_variant_m<M_JFIRST, 0>(ept, vec);
    case M_JLAST: return pass_kernel_variant_m<M_JLAST, 0>(ept, vec);
    case M_TFIRST_LIN: return pass_kernel_variant_m<M_TFIRST_LIN, 0>(ept, vec);
    case M_TLAST_LIN: return pass_kernel_variant_m<M_TLAST_LIN, 0>(ept, vec);
    default: return nullptr;
  }
}

#endif

}  // namespace sdfs

// sdfs_api.hip -- host side of libsdfs_hip.so: model set-up, pass planner, launch
// plumbing, the device-resident solver loops and the C ABI of include/sdfs_hip.h.
//
// Reference behaviour mirrored here (paths relative to the reference repo):
//   operator      code/ssy/discrete/ssy_wc_ratio.py:82-151, code/gcy/discrete/gcy_wc_ratio.py:134-238
//   SA loop       code/solvers.py:19-48
//   Newton-Krylov code/solvers.py:51-95  (+ jax.scipy.sparse.linalg.bicgstab semantics)
//   Anderson      code/solvers.py:98-124 (+ jaxopt.AndersonAcceleration semantics, unpinned)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/sdfs_hip.h"
#include "pass_kernel.hpp"
#include "fast_kernels.hpp"
#include "stream_kernels.hpp"
#include "f32_kernels.hpp"
#include "pad_kernels.hpp"
#include "cont_kernel.hpp"
#include "dense_kernel.hpp"
#include "vec_kernels.hpp"
#include "krylov_kernels.hpp"
#include "sens_kernels.hpp"
#include "price_kernels.hpp"
#include "price_sens.hpp"
#include "sim_kernels.hpp"
#include "sim_host.hpp"
#include "batch_kernels.hpp"
#include "batch_newton.hpp"
#include "batch_adjoint.hpp"
#include "batch_price.hpp"
#include "batch_sim.hpp"

using namespace sdfs;

// the transpose of the continuous operator's J.v at the cached linearisation (cont_vjp.hip: the C_VJP form of cont_kernel
// behind the initialisation of io.out; run_cont's MODE_VJP branch, cont_adjoint.hpp)
namespace sdfs { hipError_t cont_vjp_launch(hipStream_t stream, const ContDesc& cd, const ContIO& io); }

namespace {

constexpr int MAXD = 6;
constexpr int SCHED_WORDS = TK_WORDS;   // scheduler words of one persistent line pass (stream_kernels.hpp; the older persistent form uses two)

thread_local std::string g_create_error;

struct AxisInfo {
  int n = 1;            // global extent
  int nloc = 1;         // local extent (== n unless this axis is sharded in this stage)
  int off = 0;          // global index of local index 0
  const double* Q = nullptr;   // device transition tensor [.., n, n]
  const double* Qt = nullptr;  // its transpose, for unconditional tensors only (the vector-Jacobian product)
  const double* Qp = nullptr;  // unconditional, n <= 16: the matrix and its transpose zero-padded to 16 x 16
  const double* Qtp = nullptr; // (small-grid pair plan)
  const double* Qpad[4] = {nullptr, nullptr, nullptr, nullptr};   // unconditional: zero-padded to 16 / 20 / 24 / 32 squared where n fits (padded pair plan)
  const double* Qtpad[4] = {nullptr, nullptr, nullptr, nullptr};
  int qs[MAXD] = {0, 0, 0, 0, 0, 0};  // matrix-index stride per conditioning axis
  long long qcount = 0;        // number of n x n matrices in Q
  int a3s = 0;                 // index stride of this axis in the a3 table (when it is kept as a table)
  char name[8] = "";
};

struct Pass {
  PassDesc d;
  int block = 256;
  bool vec2 = false;        // tile runs are even and 16-B aligned: double2 accesses
  bool vec4 = false;        // ... multiples of four: float4 accesses of the fp32 J.v streams
  int ept1 = 1, ept2 = 1, ept4 = 1;   // units per thread for VEC = 1 / 2 / 4
  size_t lds_bytes = 0;
  int tile_axes[3] = {-1, -1, -1};
  int step_axes[3] = {-1, -1, -1};
  double q_bytes = 0;
  double flops = 0;
  int counter = -1;
  std::string label;
};

struct Plan {
  std::vector<Pass> passes;
  long long nloc = 0;     // local grid points
  int shape[MAXD];
};

struct EventPair { hipEvent_t a, b; int counter; };

// "pair plan" (fast_kernels.hpp): one slice pass over the two fastest axes, then one line pass per slower pair
struct FastPass {
  bool line = false;
  int stream = 0;              // line pass: stream_kernels.hpp's forms -- bit 0: as a middle pass (T and J.v, fp64), bit 1: as T's last pass
  int n = 0;
  int ax0 = -1, ax1 = -1;      // the contracted pair (ax0 slower)
  SliceDesc sd;
  LineDesc ld;
  bool small = false;          // small-grid form: run-time extents <= 16, one wave per tile (SmallDesc)
  int r = 1;                   // its run length
  int wpt = 1;                 // ... and waves per tile
  SmallDesc sm;
  bool pad = false;            // padded form: run-time extents <= nt on nt x nt tiles (16 / 24 / 32), real strides (pad_kernels.hpp)
  int nt = 16;
  PadDesc pd;
  double q_bytes = 0, flops = 0;
  std::string label;
};
struct FastPlan {
  bool ok = false;
  bool small = false;          // built from small_tile_kernel passes
  bool pad = false;            // built from pad_kernels.hpp passes
  bool f32_ok = false;         // every line pass walks whole 16-element chunks: fp32 J.v forms exist
  std::vector<FastPass> passes;
};

// Run-time knobs (tools/README.md): read ONCE, when a handle is created -- never on a launch path
struct Knobs {
  int no_slice_merge = 0;      // SDFS_NO_SLICE_MERGE: 1 = slice-identical conditional tensors stay conditional
  int no_and_push_fusion = 0;  // SDFS_NO_AND_PUSH_FUSION: 1 = Anderson on large grids keeps the push as a kernel of its own
  int no_f32_stream = 0;       // SDFS_NO_F32_STREAM: 1 = the fp32-MFMA middle pass keeps one tile per workgroup
  int line_stream = 3;         // SDFS_LINE_STREAM: stream_kernels.hpp forms of the fp64 line passes; bit 0: middle pass, bit 1: T's
                               // last pass (both: on the extents they were measured on, n = 20), bit 2: on every extent
  int plan = 0;                // SDFS_PLAN: 0 = automatic, 1 = "classic" (generic tiles only), 2 = "pair" (pair plan whenever legal)
  int small_plan = 1;          // SDFS_SMALL_PLAN: 0 = never use the small-grid pair plan
  int small_r = 0;             // SDFS_SMALL_R: force the run length of its line passes (1 or 4)
  int small_wpt = 0;           // SDFS_SMALL_WPT: force its waves per tile (1 or 4)
  int pad_plan = 1;            // SDFS_PAD_PLAN: 0 = the grids between the plans keep the generic tiles; 2 = the padded plan also for
                               // shapes that mix extents above and below 16 (measured: no gain)
  int and_host = 0;            // SDFS_AND_HOST: 1 = Anderson with the Gram solve on the host (one synchronisation per iteration)
  int and_fused = 1;           // SDFS_AND_FUSED: 0 = Anderson on the small-grid plan keeps push / step / update as launches of their own
  int sa_fused = -1;           // SDFS_SA_FUSED: 0 = successive approximation keeps one launch per pass; 1 = fused end + start kernels;
                               // default (-1): fused on the small-grid plan, one launch per pass on the 6-D pair plan
};

// What the launches of the batched-Gram Anderson form are told about a run (anderson_host.hpp)
struct AndRun { long long n = 0; int m = 0, mixing_freq = 1; double tol = 0, max_iter = 0, beta = 0, ridge = 0; AndPtrs hp; };

}  // namespace

struct sdfs_handle {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  int model = 0, ndim = 0;
  int num_cus = 256;
  int shape[MAXD] = {1, 1, 1, 1, 1, 1};
  long long N = 0;
  double theta = 0, beta = 0;
  std::string err;

  // device copies of the model tensors
  std::vector<double*> dev_allocs;
  AxisInfo ax[MAXD];

  Knobs knobs;

  // plans: [0] full grid (or stage 0 of a sharded run), [1] stage 1 of a sharded run
  Plan plan[2];
  FastPlan fast;                      // pair plan of the full grid, when the model admits it
  FastPlan sfast[2];                  // sharded handle: the two stages on the pair plan's kernels (build_stage_fast_plans)
  unsigned* sched = nullptr;          // tile tickets of the persistent line passes (SCHED_WORDS per pass, zero between launches)
  double* sa_ring = nullptr;          // small-grid SA: per-workgroup residual maxima of the last two iterations [2][SA_RING]
  std::vector<void*> misc_allocs;     // device index tables of the pair plan
  bool sharded = false;
  int axis_a = -1, axis_b = -1;

  double* a3 = nullptr;              // current-state scale table, kept only when the z tensor is slice-identical

  // parameter tangent (sdfs_param_tangent_dev): what setup_model built the scale tables a1 / a2 / a3 from
  struct {
    int ip_beta = 0, ip_gamma = 0, ip_psi = 0, ip_mu_c = 0;   // indices into params
    int ia_hlam = 0, ia_sigc = 0, ia_z = 0;                   // indices into arrays
    std::vector<int> trans;                                   // indices of the transition arrays
    std::vector<long long> sizes;                             // element count of every array
    double gamma = 0, psi = 0, mu_c = 0;
    std::vector<double> hlam, sigc, z;                        // h_lambda, sigma_c, z states (z in the a3 layout)
    int ax_a1 = 0, ax_a2 = 0;                                 // axes a1 (next state) and a2 (current state) are indexed by
    int a3s[MAXD] = {0, 0, 0, 0, 0, 0};                       // strides of the a3 table along each axis
    std::vector<double> dla3_host;                            // staging of the dln a3 table (kept alive across the async copy)
    double* dla3 = nullptr;                                   // device copy
    double* v = nullptr;                                      // J.v direction of the tangent
    double* la3 = nullptr;                                    // ln a3 table (k_sens_generator), built on first use
  } sens;

  // tilted expectation K (sdfs_set_tilt_dev): its scalings d1 / d2 stand in for c1 / c2 in the J.v kernels; they never
  // replace the cached linearisation, and Newton's fused forms and the captured graphs never see them
  struct {
    int power = -1;                                           // -1: no tilt set
    double* d1 = nullptr; double* d2 = nullptr;               // next-state / current-state scalings
    std::vector<double> ez_host;                              // staging of the e_z table (kept alive across the async copy)
    double* ez = nullptr;                                     // device copy
    double* pa = nullptr; double* pb = nullptr;               // P_n ping-pong of the horizon loop
    double* part = nullptr;                                   // per-workgroup partials of one horizon
    double* res = nullptr; long long res_cap = 0;             // PRICE_NSUM doubles per horizon
    // the tilt's tangent (sdfs_tilt_tangent_dev)
    double kappa_lam = 0, kappa_c = 0;                        // the exponents the scalings were built with
    double* tw = nullptr;                                     // T w of the tilt's linearisation (power >= 1)
    double* tv = nullptr; double* kf = nullptr;               // the product's direction u1 f + df; K f when the caller has none
    std::vector<double> tz_host;                              // staging of the a3-shaped table of u2 (kept alive across the async copy)
    double* tz = nullptr;                                     // device copy
    double* zt = nullptr;                                     // mu_c + z in the a3 layout (k_tilt_tangent_generator), built on first use
  } price;

  // simulated paths (sdfs_sim_records_dev / sdfs_sim_paths_dev)
  struct {
    double* one = nullptr; double* em = nullptr;              // E_x[M] = K(1, theta, -gamma) 1
    double* zt = nullptr;                                     // mu_c + z in the a3 layout
    double* tab = nullptr;                                    // k_sim_paths' LDS table (SIM_TAB_MAX doubles)
    std::vector<double> tab_host;                             // its staging (kept alive across the async copy)
  } sim;

  // Anderson acceleration (anderson_host.hpp; `and` itself is an operator name in C++)
  struct {
    AndState* state = nullptr;                                // device-resident loops: control state (two buffers: the fused small-grid form alternates)
    AndState* state_host = nullptr;                           // pinned mirror of the one a chunk ends on
    double* gram_partial = nullptr;                           // large grids: partial sums of the whole Gram matrix (k_and_gram_full)
    double* err = nullptr; int* kind = nullptr;               // per pass of a chunk: its error and its step kind (1: the error belongs in the trace)
    unsigned* flag = nullptr;                                 // fused form, per pass of a chunk: set by a push that met a non-finite residual
    int slots = 0;                                            // passes that err / kind / flag and the two mirrors hold
    double* err_host = nullptr; int* kind_host = nullptr;     // pinned mirrors
    hipGraphExec_t graph = nullptr;                           // one captured chunk, and what it was captured for:
    int graph_chunk = 0, graph_m = 0, graph_freq = 0;
    double graph_key[4] = {0, 0, 0, 0};                       // tol, max_iter, beta, ridge: baked into the captured kernel arguments
    std::vector<double*> X, R;                                // history of the solve loops (and_history), grown on demand
    double* gram_row = nullptr;                               // host-controlled loop: the Gram row of the pass
    double* gram_row_host = nullptr;                          // pinned mirror
    // sharded step API (sdfs_anderson_begin / _step): history in caller-owned buffers, control state in `state`
    struct : AndRun { bool on = false; } dand;
  } anderson;

  std::vector<double> a3_host;       // host copy of the a3 table (the pair plan looks for its two-table form)
  // sharded handles: the stage settings of sdfs_set_krylov_f32 / sdfs_set_t_f32 (sdfs_apply_stage_gated_dev's requests)
  bool stage_f32 = false;            // J.v and linearising stages with fp32 Krylov storage
  double lin_ref = 0.0;              // ... the reference value of the fp32 linearisation scale
  bool stage_t32 = false;            // T stages with their intermediates as scaled floats
  double t32_ref = 0.0;              // ... the reference value of that scale, the same on every rank
  bool check_every_default = false;  // the running solve was given check_every <= 0 (sdfs_solve_dev)
  bool lin_stale = false;            // c1 / c2 hold the scaled floats of sdfs_debug_jvp_storage_dev: no fp64 J.v until the next
                                     // sdfs_linearize_dev / sdfs_param_tangent_dev

  // continuous-state operator (sdfs_create_continuous): no plan, one kernel per application
  bool cont = false;
  ContDesc cd;
  double cont_gamma = 0.0;           // gamma as given (the descriptor carries 1 - gamma): the series of cont_sim.hpp
  double cont_psi = 0.0;             // psi as given: d theta of cont_sens.hpp
  // its tilted expectation K (sdfs_cont_set_tilt_dev, cont_price.hpp): a copy of w, the per-point factor d2 and the tilted
  // node weights stand beside the cached linearisation c1 / c2 and never replace it
  struct {
    int power = -1;                                           // -1: no tilt set
    std::vector<double> weight, eta0;                         // W_m and eta_0m as the handle was created with
    double* w = nullptr; double* d2 = nullptr;                // the tilt's w, d2
    double* wq = nullptr;                                     // W_m exp(kappa_lambda s_lambda eta_0m)
    std::vector<double> wq_host;                              // its staging (kept alive across the async copy)
    double* pa = nullptr; double* pb = nullptr;               // P_n ping-pong of the horizon loop
    double* part = nullptr;                                   // per-workgroup partials of one horizon
  } ctilt;

  // single-index dense form (sdfs_create_dense): H materialised, one GEMV per application
  bool dense = false;
  double* denseH = nullptr;

  // work buffers (lazy)
  double* tmp = nullptr;
  double *c1 = nullptr, *c2 = nullptr;
  double *buf0 = nullptr, *buf1 = nullptr;
  double *hostio = nullptr;          // device staging for the host-pointer entry points
  double *hostio2 = nullptr, *hostio3 = nullptr;
  std::vector<double*> kry;          // r, rhat, p, q, t, step, g
  double* partial = nullptr;         // reduction partials
  double* sc = nullptr;              // device scalars
  double* sc_host = nullptr;         // pinned
  unsigned long long* slots = nullptr;      // residual slots (device)
  unsigned long long* slots_host = nullptr; // pinned mirror
  int nslots = 0;

  double last_resid = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> trace;

  // profiling
  bool profiling = false;
  sdfs_counters counters;
  std::vector<EventPair> pending;
  std::vector<hipEvent_t> event_pool;

  double* jf_ss = nullptr; long long jf_ss_n = 0;     // per-wave-tile partial sums of <s, s>
  int bicg_graph_chunk[2] = {0, 0};                    // iterations in the captured graph
  hipGraphExec_t bicg_graph[2] = {nullptr, nullptr};   // one BiCGSTAB iteration (fp64 / fp32 Krylov storage)
  unsigned long long* bicg_gate = nullptr;             // device flag the iteration's kernels are gated on
  unsigned long long* bicg_gate_host = nullptr;        // pinned mirror
  // graph cache for the SA chunk
  hipGraphExec_t sa_graph = nullptr;
  int sa_graph_chunk = 0;
  double sa_graph_tol = 0;   // the gate tolerance is baked into the captured kernel arguments
};

namespace {

int fail(sdfs_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_create_error = buf;
  return code;
}

#define HIPCHK(h, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail((h), SDFS_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                    \
  } while (0)

int dev_alloc(sdfs_handle* h, double** p, size_t count) {
  HIPCHK(h, hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(double)));
  h->dev_allocs.push_back(*p);
  return 0;
}

int upload(sdfs_handle* h, double** dst, const double* src, size_t count) {
  int rc = dev_alloc(h, dst, count);
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(*dst, src, count * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

int env_int(const char* name, int dflt) {
  const char* s = getenv(name);
  return (s && *s) ? atoi(s) : dflt;
}

Knobs read_knobs() {
  Knobs k;
  k.no_slice_merge = env_int("SDFS_NO_SLICE_MERGE", 0);
  k.no_f32_stream = env_int("SDFS_NO_F32_STREAM", 0);
  k.no_and_push_fusion = env_int("SDFS_NO_AND_PUSH_FUSION", 0);
  k.line_stream = env_int("SDFS_LINE_STREAM", 3);
  k.small_plan = env_int("SDFS_SMALL_PLAN", 1);
  k.small_r = env_int("SDFS_SMALL_R", 0);
  k.sa_fused = env_int("SDFS_SA_FUSED", -1);
  k.small_wpt = env_int("SDFS_SMALL_WPT", 0);
  k.pad_plan = env_int("SDFS_PAD_PLAN", 1);
  k.and_host = env_int("SDFS_AND_HOST", 0);
  k.and_fused = env_int("SDFS_AND_FUSED", 1);
  const char* pl = getenv("SDFS_PLAN");
  if (pl && !strcmp(pl, "classic")) k.plan = 1;
  else if (pl && !strcmp(pl, "pair")) k.plan = 2;
  return k;
}

// ---------------------------------------------------------------------------
// Planner: group the axes into passes (legal order, LDS budget, coalesced runs).
// `todo` = axes to contract in this plan (all, or a stage's subset); `done` = axes
// already in current-state form when the plan starts.
int build_plan(sdfs_handle* h, Plan& plan, const std::vector<int>& todo_in, std::vector<bool> done) {
  const int D = h->ndim;
  long long nloc = 1;
  for (int a = 0; a < D; ++a) { plan.shape[a] = h->ax[a].nloc; nloc *= h->ax[a].nloc; }
  plan.nloc = nloc;
  long long stride[MAXD];
  {
    long long s = 1;
    for (int a = D - 1; a >= 0; --a) { stride[a] = s; s *= h->ax[a].nloc; }
  }
  const long long budget = std::max<long long>(256, std::min<long long>(8192, nloc / 128));

  std::vector<int> todo = todo_in;
  auto cond_ok = [&](int g, const std::vector<bool>& dn) {
    for (int c = 0; c < D; ++c) if (h->ax[g].qs[c] != 0 && !dn[c]) return false;
    return true;
  };
  auto in = [](const std::vector<int>& v, int x) { return std::find(v.begin(), v.end(), x) != v.end(); };

  while (!todo.empty()) {
    std::vector<int> cand;
    for (int g : todo) if (cond_ok(g, done)) cand.push_back(g);
    if (cand.empty()) return fail(h, SDFS_ERR_ARG, "planner: cyclic conditioning between axes");
    std::sort(cand.begin(), cand.end(), [](int x, int y) { return x > y; });   // fastest first

    std::vector<int> G, tile;
    auto tile_elems = [&](const std::vector<int>& t) {
      long long e = 1; for (int a : t) e *= h->ax[a].nloc; return e; };
      auto conflicts = [&](const std::vector<int>& grp, const std::vector<int>& t) {
      for (int g : grp) for (int a : t) if (h->ax[g].qs[a] != 0) return true;
      return false;
    };
    const int F = D - 1;
    for (int g : cand) {
      if (h->ax[g].nloc != h->ax[g].n) continue;          // a sharded axis cannot be contracted locally
      std::vector<int> ng = G; ng.push_back(g);
      std::vector<int> nt = tile; if (!in(nt, g)) nt.push_back(g);
      std::vector<int> ntF = nt; if (!in(ntF, F)) ntF.push_back(F);
      if ((int)ntF.size() <= 3 && tile_elems(ntF) <= budget && !conflicts(ng, ntF)) { G = ng; tile = ntF; continue; }
      if (G.empty() && (int)nt.size() <= 3 && !conflicts(ng, nt)) {    // no room for the run axis
        if (h->ax[g].nloc > MAXN) return fail(h, SDFS_ERR_UNSUPPORTED, "axis extent %d > %d", h->ax[g].nloc, MAXN);
        G = ng; tile = nt;
      }
    }
    if (G.empty()) return fail(h, SDFS_ERR_ARG, "planner: no contractible axis (sharded axis still pending?)");
    // filler axes: amortise a conditional Q over more columns / keep >= 16 columns per step.
    // A filler is a pure batch axis, so it may enter the tile in CHUNKS (chunk = a divisor of its
    // extent): smaller tiles -> more resident blocks per CU where only the batch axis is shrunk.
    int chunk_axis = -1, chunk = 0;
    while ((int)tile.size() < 3) {
      int pick = -1;
      for (int a = D - 1; a >= 0; --a) {
        if (in(tile, a)) continue;
        bool bad = false;
        for (int g : G) if (h->ax[g].qs[a] != 0) bad = true;
        if (bad) continue;
        pick = a; break;
      }
      if (pick < 0) break;
      std::vector<int> nt = tile; nt.push_back(pick);
      const long long e = tile_elems(nt);
      long long mincols = 1LL << 60;
      for (int g : G) mincols = std::min(mincols, tile_elems(tile) / h->ax[g].nloc);
      const bool want = (mincols < 16) || (nloc / e >= 512);
      if (e > budget || !want) break;
      tile = nt;
      // a filler that makes the tile too big for more than two blocks per CU is taken in two halves
      // (GCY 20^6 last pass: 20x10x20 tiles, four 256-thread blocks per CU, 0.384 -> 0.363 ms)
      int fc = 0;
      if (pick != F && tile_elems(tile) * 8 > 53 * 1024 && h->ax[pick].nloc % 2 == 0) fc = h->ax[pick].nloc / 2;
      if (fc > 0 && chunk_axis < 0 && h->ax[pick].nloc % fc == 0 && fc < h->ax[pick].nloc &&
          tile_elems(tile) / h->ax[pick].nloc * fc / h->ax[G.back()].nloc >= 64) {
        chunk_axis = pick; chunk = fc;
      }
    }
    std::sort(tile.begin(), tile.end());                    // slow -> fast
    // steps: fastest axis first
    std::sort(G.begin(), G.end(), [](int x, int y) { return x > y; });

    Pass P;
    memset(&P.d, 0, sizeof P.d);
    PassDesc& d = P.d;
    const int nt = (int)tile.size();
    for (int j = 0; j < 3; ++j) { d.m[j] = 1; d.toff[j] = 0; d.gstride[j] = 0; d.ta3[j] = 0; }
    for (int j = 0; j < nt; ++j) {
      const int slot = 3 - nt + j, a = tile[j];
      d.m[slot] = (a == chunk_axis) ? chunk : h->ax[a].nloc; d.toff[slot] = h->ax[a].off; d.gstride[slot] = (int)stride[a];
      P.tile_axes[slot] = a;
      d.ta3[slot] = h->ax[a].a3s;
    }
    d.nfixed = 0;
    long long ntiles = 1;
    for (int a = 0; a < D; ++a) {
      if (a == chunk_axis) {               // the chunk number is one more block-fixed coordinate
        if (d.nfixed >= MAXF) return fail(h, SDFS_ERR_UNSUPPORTED, "too many fixed axes");
        const int k = d.nfixed++;
        d.fext[k] = h->ax[a].nloc / chunk; d.foff[k] = 0; d.fstride[k] = stride[a] * chunk;
        for (int s = 0; s < (int)G.size(); ++s) d.fq[s][k] = 0;
        d.fa3[k] = h->ax[a].a3s * chunk;
        ntiles *= d.fext[k];
        continue;
      }
      if (in(tile, a)) continue;
      if (d.nfixed >= MAXF) return fail(h, SDFS_ERR_UNSUPPORTED, "too many fixed axes");
      const int k = d.nfixed++;
      d.fext[k] = h->ax[a].nloc; d.foff[k] = h->ax[a].off; d.fstride[k] = stride[a];
      for (int s = 0; s < (int)G.size(); ++s) d.fq[s][k] = h->ax[G[s]].qs[a];
      d.fa3[k] = h->ax[a].a3s;
      ntiles *= h->ax[a].nloc;
    }
    d.ntiles = ntiles;
    d.nsteps = (int)G.size();
    bool contracts_fast_slot = false;
    long long maxct = 1;
    for (int s = 0; s < d.nsteps; ++s) {
      const int g = G[s];
      if (h->ax[g].n > MAXN) return fail(h, SDFS_ERR_UNSUPPORTED, "axis extent %d > %d", h->ax[g].n, MAXN);
      int slot = -1;
      for (int j = 0; j < 3; ++j) if (P.tile_axes[j] == g) slot = j;
      d.sslot[s] = slot; d.sn[s] = h->ax[g].n; d.Q[s] = h->ax[g].Q;
      P.step_axes[s] = g;
      if (slot == 2) contracts_fast_slot = true;
      const long long cols = (long long)d.m[0] * d.m[1] * d.m[2] / h->ax[g].nloc;
      maxct = std::max(maxct, (cols + 15) / 16);
      P.q_bytes += 8.0 * (double)h->ax[g].qcount * h->ax[g].n * h->ax[g].n;
      P.flops += 2.0 * (double)nloc * h->ax[g].n;
    }
    // LDS strides: pad the fastest stride to == 2 (mod 4) doubles when it is the
    // K dimension of an MFMA step (16 columns x 2 rows then hit 32 distinct b64 banks)
    int L1 = d.m[2];
    if (contracts_fast_slot && d.m[1] * d.m[0] > 1) { while ((L1 & 3) != 2) ++L1; }
    d.L[2] = 1; d.L[1] = L1; d.L[0] = L1 * d.m[1];
    long long lds_elems = (long long)d.L[0] * d.m[0];
    lds_elems += lds_elems & 1;
    for (int s = 0; s < 3; ++s) {                     // staged transition matrices behind the tile
      d.qlds[s] = (int)lds_elems;
      if (s < d.nsteps) lds_elems += d.sn[s] * d.sn[s];
    }
    P.lds_bytes = (size_t)lds_elems * 8;
    if (P.lds_bytes > 150 * 1024) return fail(h, SDFS_ERR_UNSUPPORTED, "tile of %lld doubles exceeds LDS", lds_elems);
    // block size: balance column tiles over waves, keep enough lanes for the elementwise stages
    const long long tot = (long long)d.m[0] * d.m[1] * d.m[2];
    int w_elem = (int)std::min<long long>(8, std::max<long long>(1, (tot + 127) / 128));
    int w_mfma = (int)std::min<long long>(maxct, 8);
    if (maxct > 4) {
      long long best = 1LL << 60;
      for (int w = 8; w >= 4; --w) {
        long long cost = 0;
        for (int s = 0; s < d.nsteps; ++s) {
          const long long ct = (tot / d.sn[s] + 15) / 16;
          cost += (ct + w - 1) / w;
        }
        if (cost < best) { best = cost; w_mfma = w; }
      }
    }
    int waves = std::max(w_elem, w_mfma);
    // Resident waves per CU are capped at 16 by the ~128 VGPRs of the kernel.  Where LDS would allow more
    // than two blocks per CU (tiles well under 80 KB), smaller blocks keep those 16 waves but put more
    // independent blocks -- in different phases -- on the CU (GCY 16^6: 3031 -> 3519 iterations/s).
    const int blocks_lds = (int)std::min<size_t>(8, (160 * 1024) / std::max<size_t>(P.lds_bytes, 1));
    if (blocks_lds > 2) {
      int w = 2;                                    // power of two: 16-column tiles split evenly over the waves
      while (2 * w <= 16 / blocks_lds) w *= 2;
      waves = std::min(waves, w);
    }
    P.block = 64 * waves;
    auto round_ept = [](long long e) { int r = 1; while (r < e) r <<= 1; return r; };
    auto units_per_thread = [&](long long units) { return round_ept((units + P.block - 1) / P.block); };
    while (units_per_thread(tot) > 16 && P.block < 512) P.block += 64;
    // 16 double2 units per thread spill in the J.v roles (the tile and its scaling stream are both in flight:
    // 128 of the 128 VGPRs): widen the block instead
    while (units_per_thread(tot / 2) > 8 && P.block < 512) P.block += 64;
    P.ept1 = units_per_thread(tot);
    if (P.ept1 > 16) return fail(h, SDFS_ERR_UNSUPPORTED, "tile too large for one block");
    // 16-byte accesses: runs along slot 2 must be even, contiguous and every base even
    bool v2 = (d.m[2] % 2 == 0) && d.gstride[2] == 1 && (d.L[1] % 2 == 0) && (d.L[0] % 2 == 0) &&
              (d.gstride[0] % 2 == 0 || d.m[0] == 1) && (d.gstride[1] % 2 == 0 || d.m[1] == 1);
    for (int k = 0; k < d.nfixed; ++k) if (d.fstride[k] % 2 != 0 && d.fext[k] > 1) v2 = false;
    P.vec2 = v2;
    P.ept2 = v2 ? units_per_thread(tot / 2) : P.ept1;
    bool v4 = v2 && (d.m[2] % 4 == 0) && (d.gstride[0] % 4 == 0 || d.m[0] == 1) && (d.gstride[1] % 4 == 0 || d.m[1] == 1);
    for (int k = 0; k < d.nfixed; ++k) if (d.fstride[k] % 4 != 0 && d.fext[k] > 1) v4 = false;
    P.vec4 = v4 && units_per_thread(tot / 4) <= 4;        // eight float4 units + their scaling stream spill
    P.ept4 = P.vec4 ? units_per_thread(tot / 4) : P.ept2;
    char lab[96];
    int o = snprintf(lab, sizeof lab, "expect[");
    for (int s = 0; s < d.nsteps; ++s) o += snprintf(lab + o, sizeof lab - o, "%s%s", s ? "," : "", h->ax[G[s]].name);
    o += snprintf(lab + o, sizeof lab - o, "|tile");
    for (int j = 0; j < 3; ++j) if (P.tile_axes[j] >= 0) o += snprintf(lab + o, sizeof lab - o, " %s", h->ax[P.tile_axes[j]].name);
    snprintf(lab + o, sizeof lab - o, "]");
    P.label = lab;
    plan.passes.push_back(P);

    for (int g : G) { done[g] = true; todo.erase(std::find(todo.begin(), todo.end(), g)); }
  }
  return 0;
}

// ---------------------------------------------------------------------------
int get_event(sdfs_handle* h, hipEvent_t* e) {
  if (!h->event_pool.empty()) { *e = h->event_pool.back(); h->event_pool.pop_back(); return 0; }
  HIPCHK(h, hipEventCreate(e));
  return 0;
}

int drain_events(sdfs_handle* h) {
  if (h->pending.empty()) return 0;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (auto& p : h->pending) {
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, p.a, p.b));
    h->counters.k[p.counter].launches += 1;
    h->counters.k[p.counter].total_ms += ms;
    h->event_pool.push_back(p.a);
    h->event_pool.push_back(p.b);
  }
  h->pending.clear();
  return 0;
}

int counter_id(sdfs_handle* h, const char* name, double bytes, double flops) {
  for (int i = 0; i < h->counters.nkernels; ++i)
    if (strncmp(h->counters.k[i].name, name, sizeof h->counters.k[i].name - 1) == 0) return i;
  if (h->counters.nkernels >= SDFS_MAX_KERNELS) return SDFS_MAX_KERNELS - 1;
  const int i = h->counters.nkernels++;
  memset(&h->counters.k[i], 0, sizeof h->counters.k[i]);
  strncpy(h->counters.k[i].name, name, sizeof h->counters.k[i].name - 1);
  h->counters.k[i].alg_bytes = bytes;
  h->counters.k[i].alg_flops = flops;
  return i;
}

struct ProfScope {
  sdfs_handle* h; hipEvent_t a = nullptr, b = nullptr; int counter; bool on;
  ProfScope(sdfs_handle* h_, int counter_) : h(h_), counter(counter_), on(h_->profiling && counter_ >= 0) {
    if (on) {
      if (get_event(h, &a) || get_event(h, &b)) { on = false; return; }
      hipEventRecord(a, h->stream);
    }
  }
  ~ProfScope() {
    if (on) {
      hipEventRecord(b, h->stream);
      h->pending.push_back({a, b, counter});
      if (h->pending.size() > 4096) drain_events(h);
    }
  }
};

int vec_grid(long long n) {
  // one 16-byte packet per thread up to the cap: small grids are latency-bound, a second trip through a thread's
  // grid-stride loop costs a memory round trip (15^4: k_and_push 8.2 us with 50 workgroups of two trips)
  long long g = (n + VEC_BLOCK * 2 - 1) / (VEC_BLOCK * 2);
  return (int)std::max<long long>(1, std::min<long long>(g, MAX_PARTIAL_BLOCKS));
}

// modes of one operator application
// MODE_VJP: u -> c1 .* H'^T (c2 .* u) (- u): the J.v kernels with transposed matrices and the two diagonal
// scalings in each other's place.  Unconditional tensors only (a conditional tensor's transpose conditions on
// indices that are summed over).
enum { MODE_T = 0, MODE_JVP = 1, MODE_T_LIN = 2, MODE_VJP = 3 };

// storage precision of one application: fp64; the fp32 Krylov storage of opts.krylov_f32 = 1 / 2 / 3 (J.v streams, and c1 / c2
// of a linearising T, as scaled floats; 2: every such store rounded to bfloat16; 3: the J.v passes of the pair plan on an fp32
// LDS tile and fp32 MFMA); or opts.t_f32's intermediates of a plain T application as scaled floats
enum { PREC_F64 = 0, PREC_F32 = 1, PREC_BF16 = 2, PREC_MFMA32 = 3, PREC_T32 = 4 };

// One operator application: everything that selects and feeds its kernels besides the handle's cached state (the
// linearisation c1 / c2, the plans, the buffers)
struct Apply {
  int mode;
  const double* in; double* out; const double* old;
  unsigned long long* resid = nullptr;          // T: max |T w - old| (the first pass clears the word)
  const unsigned long long* gate = nullptr;     // every kernel returns at once while *gate <= gate_tol
  double gate_tol = 0.0;
  int minus_identity = 0;                       // J.v: out = J v - v
  double* dotp = nullptr;                       // ... and its last pass writes per-workgroup partial sums of <out, in>, <out, out>
  const double* lc1 = nullptr;                  // J.v scalings in place of the cached c1 / c2 (the tilted expectation's d1 / d2;
  const double* lc2 = nullptr;                  // on a continuous handle the tilt's copy of w and its d2, cont_price.hpp)
  int prec = PREC_F64;
  const double* dot_with = nullptr;             // small-grid plan: the last pass also sums <out, dot_with> (needs dotp)
  // large-grid Anderson: the streamed last pass of T also does the push (LineIO::and_*); *tiles = the partial sums it
  // wrote, 0 where the pass was not a streamed one
  struct { double* y = nullptr; double* r = nullptr; double beta = 0.0; double* dot = nullptr; long long* tiles = nullptr; } push;
  // fused BiCGSTAB iteration on the compile-time pair plan (krylov_kernels.hpp): the first pass forms p or s on its registers
  // (kind JF_P / JF_S; -1: plain first pass), the last pass is the streamed form with one workgroup per tile and, where
  // dot_with is set, a third sum
  struct { int kind = -1; double* upd = nullptr; const double* a = nullptr; const double* q = nullptr; double* dot = nullptr;
           const double* dot_with = nullptr; } bicg;
  Apply(int mode_, const double* in_, double* out_, const double* old_) : mode(mode_), in(in_), out(out_), old(old_) {}
  bool f32() const { return prec == PREC_F32 || prec == PREC_BF16 || prec == PREC_MFMA32; }   // fp32 Krylov storage
};

// What one launch is counted as: a plain name, or "<tag>:<sub><label>" for a pass of a plan.  Only pointers are kept:
// the name is put together when profiling is on, never on the plain launch path.
struct Counter {
  const char* tag; const char* sub; const std::string* label; double bytes, flops;
  Counter(const char* name, double bytes_, double flops_) : tag(name), sub(""), label(nullptr), bytes(bytes_), flops(flops_) {}
  Counter(const char* tag_, const std::string& label_, double bytes_, double flops_, const char* sub_ = "")
      : tag(tag_), sub(sub_), label(&label_), bytes(bytes_), flops(flops_) {}
};

// counter, timing scope, launch on the handle's stream and error check of one kernel
template <typename... P, typename... A>
int launch_kernel(sdfs_handle* h, void (*fn)(P...), dim3 grid, dim3 block, size_t lds, const Counter& c, A&&... args) {
  int cid = -1;
  if (h->profiling) {
    char nm[48];
    if (c.label) snprintf(nm, sizeof nm, "%s:%s%s", c.tag, c.sub, c.label->c_str());
    cid = counter_id(h, c.label ? nm : c.tag, c.bytes, c.flops);
  }
  ProfScope ps(h, cid);
  hipLaunchKernelGGL(fn, grid, block, lds, h->stream, static_cast<P>(args)...);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// What pass i of a plan launches for a request: kernel, geometry, counter.  select_pass (below) is the one place that picks
// the form of a pass -- run_passes launches it, sdfs_describe_plan prints it, the fused dot products of BiCGSTAB size their
// partial sums by its grid.
struct PassLaunch {
  const void* fn = nullptr;          // (generic tiles: null -- VEC and EPT follow the pointers' alignment, launch_pass)
  unsigned grid = 0;
  int block = 256;
  size_t lds = 0;
  double bytes = 0;                  // algorithmic bytes of the counter
  const char* tag = "";              // counter name "<tag>:<pass label>"
  int kmode = 0;                     // the kernel's mode: M_* (generic tiles), S_* (slice passes), SM_* (small grid), L_* (line passes)
  bool f32 = false;                  // generic tiles: the pass runs in fp32 storage
  bool jfused = false;               // first pass with BiCGSTAB's p / s update (JFusedIO, JFused32IO with m32)
  bool m32 = false;                  // fp32-MFMA form (f32_kernels.hpp, krylov_kernels.hpp)
  bool persistent = false;           // ... its persistent middle pass, next tile in flight
  bool push = false;                 // T's streamed last pass with the Anderson push
  const double* dot_with = nullptr;  // J.v's last pass also sums <out, dot_with>
  const char* err = nullptr;         // no kernel for this pass
  int err_code = SDFS_ERR_UNSUPPORTED;
};

// ... and its launch: pass P (a Pass or a FastPass) with the kernel's descriptor and streams
template <typename AnyPass, typename Desc, typename IO>
int launch_selected(sdfs_handle* h, const PassLaunch& L, const AnyPass& P, const Desc& d, const IO& io) {
  return launch_kernel(h, (void (*)(const Desc, const IO))L.fn, dim3(L.grid), dim3(L.block), L.lds,
                       Counter(L.tag, P.label, L.bytes, P.flops), d, io);
}

// VEC and EPT of a generic pass: 16-byte accesses where the tile allows them and every grid pointer is aligned, float4
// accesses for the fp32 streams of a J.v pass
struct TileForm { int vec, ept; };
TileForm tile_form(const Pass& P, bool aligned, bool f32_jv) {
  const bool v2 = P.vec2 && aligned, v4 = v2 && P.vec4 && f32_jv;
  return {v4 ? 4 : (v2 ? 2 : 1), v4 ? P.ept4 : (v2 ? P.ept2 : P.ept1)};
}

// one pass on the generic tiles (pass_kernel.hpp) in the kernel mode L.kmode
int launch_pass(sdfs_handle* h, const Pass& P, PassLaunch L, const PassIO& io, int minus_identity, bool transposed) {
  PassDesc d = P.d;
  if (transposed)
    for (int s = 0; s < d.nsteps; ++s) d.Q[s] = h->ax[P.step_axes[s]].Qt;
  const int mode = L.kmode;
  d.pro = d.epi = 0; d.minus_identity = minus_identity;
  d.theta = h->theta; d.inv_theta = 1.0 / h->theta; d.beta = h->beta;
  d.ablate = 0;
  d.a3 = (mode == M_TONLY || mode == M_TLAST || mode == M_TLAST_LIN) ? h->a3 : nullptr;   // (the aggregator's passes)
  d.ref_off = 0;
  d.lin_ref = h->sharded ? h->lin_ref : 0.0;
  if (!h->sharded) {                       // C-order offset of the mid-grid point
    long long stride = 1;
    for (int a = h->ndim - 1; a >= 0; --a) { d.ref_off += (long long)(h->shape[a] / 2) * stride; stride *= h->shape[a]; }
  }
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const TileForm tf = tile_form(P, al16(io.in) && al16(io.out) && al16(io.aux_in) && al16(io.aux_out) && al16(io.old),
                               L.f32 && (mode == M_JFIRST || mode == M_MID || mode == M_JLAST));
  if (tf.vec == 1 && (long long)P.ept1 * P.block < (long long)d.m[0] * d.m[1] * d.m[2])
    return fail(h, SDFS_ERR_ARG, "grid pointers must be 16-byte aligned for this tile shape");
  pass_fn fn = pass_kernel_variant(tf.ept, tf.vec, mode, L.f32 ? 1 : 0);
  if (!fn) return fail(h, SDFS_ERR_UNSUPPORTED, "no kernel variant for EPT %d VEC %d", tf.ept, tf.vec);
  L.fn = (const void*)fn;
#ifdef SDFS_STAMP
  const long long grid = L.grid;
  const int block = L.block;
  PassIO io2 = io;
  static unsigned long long* dbg_dev = nullptr;
  if (!dbg_dev) hipMalloc((void**)&dbg_dev, 64 * 2 * 16 * 8);
  hipMemsetAsync(dbg_dev, 0, 64 * 2 * 16 * 8, h->stream);
  io2.dbg = dbg_dev;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(block), P.lds_bytes, h->stream, d, io2);
  {
    static int dumps = 0;
    if (dumps < 12) {
      std::vector<unsigned long long> hb(64 * 2 * 16);
      hipStreamSynchronize(h->stream);
      hipMemcpy(hb.data(), dbg_dev, hb.size() * 8, hipMemcpyDeviceToHost);
      if (dumps >= 6) {
        fprintf(stderr, "STAMP %s mode %d\n", P.label.c_str(), mode);
        for (int b = 0; b < 64; b += 9) for (int t = 0; t < 2; ++t) {
          fprintf(stderr, "  blk %2d trip %d:", b, t);
          for (int k = 1; k < 14; ++k) {
            unsigned long long a = hb[(b * 2 + t) * 16 + k - 1], c = hb[(b * 2 + t) * 16 + k];
            fprintf(stderr, " %6lld", (a && c) ? (long long)(c - a) : -1LL);
          }
          fprintf(stderr, "\n");
        }
      }
      ++dumps;
    }
  }
  return 0;
#endif
  return launch_selected(h, L, P, d, io);
}

int ensure_tmp(sdfs_handle* h) {
  if (!h->tmp) return dev_alloc(h, &h->tmp, (size_t)std::max(h->plan[0].nloc, h->plan[1].nloc));
  return 0;
}
int ensure_lin(sdfs_handle* h) {
  const size_t n = (size_t)std::max(h->plan[0].nloc, h->plan[1].nloc);
  if (!h->c1) { int rc = dev_alloc(h, &h->c1, n); if (rc) return rc; }
  if (!h->c2) { int rc = dev_alloc(h, &h->c2, n); if (rc) return rc; }
  return 0;
}

// One application of the continuous-state operator (cont_kernel.hpp) in the role run_passes has for the
// discretised one, so that every solver loop below serves both.
template <int D>
int launch_cont(sdfs_handle* h, int mode, const ContIO& io, const Counter& c) {
  const dim3 grid((unsigned)h->cd.N), block(256);
  // the staged box of the iterate + its pre-contracted form (x2 in the J.v kernel: the direction too)
  const size_t lds = (size_t)(h->cd.cap + h->cd.ucap) * sizeof(double);
  if (mode == MODE_T) return launch_kernel(h, cont_kernel<D, C_T>, grid, block, lds, c, h->cd, io, ContNoTan{});
  if (mode == MODE_T_LIN) return launch_kernel(h, cont_kernel<D, C_TLIN>, grid, block, lds, c, h->cd, io, ContNoTan{});
  return launch_kernel(h, cont_kernel<D, C_JVP>, grid, block, 2 * lds, c, h->cd, io, ContNoTan{});
}

// ... and of its tilted expectation (cont_price.hpp) for the SDF power p: p = 0 stages f alone, p = 1, 2 stage w and f
template <int D>
int launch_cont_tilted(sdfs_handle* h, int power, const ContDesc& cd, const ContIO& io, const Counter& c) {
  const dim3 grid((unsigned)cd.N), block(256);
  const size_t lds = (size_t)(cd.cap + cd.ucap) * sizeof(double);
  if (power == 0) return launch_kernel(h, cont_kernel<D, C_K0>, grid, block, lds, c, cd, io, ContNoTan{});
  if (power == 1) return launch_kernel(h, cont_kernel<D, C_K1>, grid, block, 2 * lds, c, cd, io, ContNoTan{});
  return launch_kernel(h, cont_kernel<D, C_K2>, grid, block, 2 * lds, c, cd, io, ContNoTan{});
}

int run_cont(sdfs_handle* h, const Apply& a) {
  int rc = 0;
  if (a.in == a.out) return fail(h, SDFS_ERR_ARG, "the continuous operator cannot run in place");
  ContIO io;
  memset(&io, 0, sizeof io);
  io.out = a.out; io.gate = a.gate; io.gate_tol = a.gate_tol; io.minus_identity = a.minus_identity;
  const double n8 = 8.0 * (double)h->cd.N;
  const double corners = (double)(1 << h->cd.D);
  double bytes = 2 * n8, flops = (double)h->cd.N * h->cd.M * (2.0 * corners + 2.0 * h->cd.D + 2.0);
  if (a.lc2) {
    // the tilted expectation: lc1 = the tilt's w, lc2 = d2; the node weights of the tilt replace the descriptor's, and the
    // cached linearisation is neither read nor written
    const int power = h->ctilt.power;
    if (a.mode != MODE_JVP || power < 0 || !a.lc1) return fail(h, SDFS_ERR_ARG, "a tilted application is a J.v request after sdfs_cont_set_tilt_dev");
    ContDesc cd = h->cd;
    cd.wq = h->ctilt.wq;
    io.w = power ? a.lc1 : a.in; io.v = a.in; io.c2_in = a.lc2;
    bytes += (power ? 2 : 1) * n8;
    if (power) flops *= 1.5;
    const Counter c(power == 0 ? "cont:K0" : (power == 1 ? "cont:K1" : "cont:K2"), bytes, flops);
    return cd.D == 4 ? launch_cont_tilted<4>(h, power, cd, io, c) : launch_cont_tilted<6>(h, power, cd, io, c);
  }
  if (a.mode != MODE_T && (rc = ensure_lin(h))) return rc;
  if (a.mode == MODE_VJP) {
    // J^T u at the cached linearisation: the scatter form (cont_vjp.hip) behind the in-stream zeroing of out, and
    // "- u" behind that.  Atomic adds: reproducible to rounding only.  Bytes: u, c2, w read, out zeroed
    // and read-modify-written (and u, out again for minus_identity); the atomic traffic depends on the boxes and is
    // not counted.
    io.w = h->c1; io.v = a.in; io.c2_in = h->c2;
    const int cid = h->profiling ? counter_id(h, "cont:vjp", (a.minus_identity ? 9 : 6) * n8, 1.5 * flops) : -1;
    ProfScope ps(h, cid);
    HIPCHK(h, sdfs::cont_vjp_launch(h->stream, h->cd, io));
    return 0;
  }
  const char* tag = "cont:T";
  if (a.mode == MODE_T) { io.w = a.in; io.old = a.old; io.resid = a.resid; if (a.resid) bytes += n8; }
  else if (a.mode == MODE_T_LIN) {
    // keep the linearisation point: the JVP re-evaluates interp(w)^(theta-1) at every node
    HIPCHK(h, hipMemcpyAsync(h->c1, a.in, (size_t)h->cd.N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    io.w = a.in; io.old = a.old; io.resid = a.resid; io.c2_out = h->c2; bytes += 3 * n8; tag = "cont:Tlin";
  } else { io.w = h->c1; io.v = a.in; io.c2_in = h->c2; bytes += 2 * n8; flops *= 1.5; tag = "cont:jvp"; }
  const Counter c(tag, bytes, flops);
  return h->cd.D == 4 ? launch_cont<4>(h, a.mode, io, c) : launch_cont<6>(h, a.mode, io, c);
}

// One application of the dense single-index operator (dense_kernel.hpp), same role as run_passes.
int run_dense(sdfs_handle* h, const Apply& a) {
  int rc = ensure_tmp(h);
  if (rc) return rc;
  if (a.mode != MODE_T && (rc = ensure_lin(h))) return rc;
  const long long N = h->N;
  DenseIO io;
  memset(&io, 0, sizeof io);
  io.H = h->denseH; io.N = N; io.out = a.out; io.gate = a.gate; io.gate_tol = a.gate_tol;
  io.beta = h->beta; io.inv_theta = 1.0 / h->theta; io.minus_identity = a.minus_identity;
  const double hbytes = 8.0 * (double)N * (double)N, flops = 2.0 * (double)N * (double)N;
  const dim3 rows((unsigned)N), block(256);
  if (a.mode == MODE_JVP) {
    io.x = a.in; io.c1 = h->c1; io.c2_in = h->c2; io.old = a.in;
    return launch_kernel(h, dense_gemv_kernel<D_JVP>, rows, block, 0, Counter("dense:jvp", hbytes + 40.0 * N, flops), io);
  }
  // (the power runs ahead of the counted launch: the counter times the GEMV alone)
  const unsigned pblocks = (unsigned)std::min<long long>((N + 255) / 256, 4096);
  if (a.mode == MODE_T_LIN)
    hipLaunchKernelGGL((dense_pow_kernel<true>), dim3(pblocks), block, 0, h->stream, a.in, h->tmp, h->c1, N, h->theta, a.gate, a.gate_tol);
  else
    hipLaunchKernelGGL((dense_pow_kernel<false>), dim3(pblocks), block, 0, h->stream, a.in, h->tmp, (double*)nullptr, N, h->theta, a.gate, a.gate_tol);
  io.x = h->tmp; io.old = a.old; io.resid = a.resid; io.c2_out = h->c2;
  const Counter c(a.mode == MODE_T ? "dense:T" : "dense:Tlin", hbytes + 32.0 * N, flops);
  return a.mode == MODE_T ? launch_kernel(h, dense_gemv_kernel<D_T>, rows, block, 0, c, io)
                          : launch_kernel(h, dense_gemv_kernel<D_TLIN>, rows, block, 0, c, io);
}

// ---------------------------------------------------------------------------
// Pair plan (fast_kernels.hpp).  Legal when every axis is unconditional (one n x n matrix per axis; the
// current-state scale a3 then lives in a table), the axes pair up (D-2, D-1), (D-4, D-3), ... with equal
// extents n in {16, 20, 24, 32}, and everything behind a line pass's pair is an even number of doubles.
// Automatic use needs enough line tiles to fill the chip (6-D grids from 16^6 up); SDFS_PLAN=pair forces it
// wherever it is legal (tests), SDFS_PLAN=classic switches it off.
int upload_ints(sdfs_handle* h, const std::vector<int>& v, int** out) {
  HIPCHK(h, hipMalloc((void**)out, std::max<size_t>(v.size(), 1) * sizeof(int)));
  h->misc_allocs.push_back(*out);
  HIPCHK(h, hipMemcpy(*out, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

// Index tables of the aggregator's a3 gather in a pass over the pair (a, a + 1) of a block of the grid (shp = local extents,
// off = global index of local index 0): a3 index = out_idx[outer] + x a3s[X] + y a3s[Y] + rest_idx[position behind Y].
// The host copies stay in outv / restv, the device copies in od / rd.
int a3_index_tables(sdfs_handle* h, const int* shp, const int* off, int a, std::vector<int>& outv, std::vector<int>& restv,
                    int** od, int** rd) {
  const int D = h->ndim;
  long long nouter = 1, lrest = 1;
  for (int c = 0; c < a; ++c) nouter *= shp[c];
  for (int c = a + 2; c < D; ++c) lrest *= shp[c];
  outv.assign((size_t)nouter, 0);
  restv.assign((size_t)lrest, 0);
  for (long long o = 0; o < nouter; ++o) {
    long long r = o; int idx = 0;
    for (int c = a - 1; c >= 0; --c) { idx += (off[c] + (int)(r % shp[c])) * h->ax[c].a3s; r /= shp[c]; }
    outv[(size_t)o] = idx;
  }
  for (long long q = 0; q < lrest; ++q) {
    long long r = q; int idx = 0;
    for (int c = D - 1; c > a + 1; --c) { idx += (off[c] + (int)(r % shp[c])) * h->ax[c].a3s; r /= shp[c]; }
    restv[(size_t)q] = idx;
  }
  int rc;
  if ((rc = upload_ints(h, outv, od)) || (rc = upload_ints(h, restv, rd))) return rc;
  return 0;
}

// Pair order of the pair, small-grid and padded plans: the two fastest axes (the first pass), then the slower pairs slowest
// first, so that the last pass walks the pair whose rows lie closest together.  Entries: the slower axis of each pair.
std::vector<int> pair_order(int D) {
  std::vector<int> pairs = {D - 2};
  for (int a = 0; a <= D - 4; a += 2) pairs.push_back(a);
  return pairs;
}

// One pass of the pair plan over a block of the grid: shp = local extents (a sharded stage holds a block of one axis,
// the whole-grid plan all of every axis), off = global index of local index 0 on every axis.
void make_slice_pass(sdfs_handle* h, const int* shp, FastPass& P) {
  const int D = h->ndim;
  long long stride[MAXD], nloc = 1;
  for (int a = D - 1; a >= 0; --a) { stride[a] = nloc; nloc *= shp[a]; }
  const int n = shp[D - 1];
  P.line = false; P.n = n; P.ax0 = D - 2; P.ax1 = D - 1;
  memset(&P.sd, 0, sizeof P.sd);
  P.sd.nslices = nloc / ((long long)n * n);
  P.sd.Qf = h->ax[D - 1].Q; P.sd.Qe = h->ax[D - 2].Q; P.sd.theta = h->theta;
  for (int c = D - 1; c >= 0; --c) P.sd.ref_off += (long long)(shp[c] / 2) * stride[c];
  P.q_bytes = 2 * 8.0 * n * n; P.flops = 2.0 * (double)nloc * 2 * n;
  P.label = std::string("slices[") + h->ax[D - 2].name + "," + h->ax[D - 1].name + "|wave-private " +
            std::to_string(slice_tile_slices(n, S_TFIRST)) + "x" + std::to_string(n) + "x" + std::to_string(n) + "]";
}

// line pass over the pair (a, a + 1), with the index tables of the aggregator's a3 gather when `tables`; returns 1
// when the block does not fit the kernels' index ranges (the caller then keeps the generic tiles)
int make_line_pass(sdfs_handle* h, const int* shp, const int* off, int a, bool tables, FastPass& P) {
  const int D = h->ndim;
  long long stride[MAXD], nloc = 1;
  for (int c = D - 1; c >= 0; --c) { stride[c] = nloc; nloc *= shp[c]; }
  const int n = shp[a];
  P.line = true; P.n = n; P.ax0 = a; P.ax1 = a + 1;
  memset(&P.ld, 0, sizeof P.ld);
  LineDesc& L = P.ld;
  L.lrest = stride[a + 1];
  if (L.lrest % 2 != 0) return 1;
  L.nchunks = (int)((L.lrest + LINE_R - 1) / LINE_R);
  L.nouter = nloc / ((long long)n * n * L.lrest);
  L.ntiles = L.nouter * L.nchunks;
  if (L.ntiles >= (1LL << 31) || (long long)n * n * L.lrest * 8 >= (1LL << 32)) return 1;
  L.Qx = h->ax[a].Q; L.Qy = h->ax[a + 1].Q;
  L.inv_theta = 1.0 / h->theta; L.beta = h->beta; L.theta = h->theta;
  L.cbt = (double)powl((long double)h->beta, (long double)h->theta);
  L.a3x = h->ax[a].a3s; L.a3y = h->ax[a + 1].a3s;
  for (int c = D - 1; c >= 0; --c) L.ref_off += (long long)(shp[c] / 2) * stride[c];
  L.cached_out = 8.0 * (double)nloc <= 192.0 * 1024 * 1024 ? 1 : 0;       // (the Infinity Cache holds 256 MB)
  P.q_bytes = 2 * 8.0 * n * n; P.flops = 2.0 * (double)nloc * 2 * n;
  P.label = std::string("lines[") + h->ax[a].name + "," + h->ax[a + 1].name + "|" + std::to_string(n) + "x" +
            std::to_string(n) + "x16 tile]";
  if (!tables) return 0;
  std::vector<int> outv, restv;
  int *od = nullptr, *rd = nullptr;
  int rc;
  if ((rc = a3_index_tables(h, shp, off, a, outv, restv, &od, &rd))) return rc;
  L.a3 = h->a3; L.out_idx = od; L.rest_idx = rd;
  // The aggregator's scale as two small tables (lever iii): for Rouwenhorst / Tauchen grids of the
  // GCY model z_states = sigma_z[h_z] g[z] + m[h_zpi, z_pi], so a3 = exp((1 - gamma)(mu_c + z_states)) is, for every
  // outer index o of this pass, a product F1[o][x] * F2[o][position behind Y] (and does not depend on Y).  Checked
  // entry by entry; where it holds the last pass reads 20 doubles and one 16-byte piece per tile instead of two
  // gathers and their index arithmetic per unit (stream_kernels.hpp, A3F).  The product differs from the table by
  // its own rounding (tolerance 64 ulp here; |theta| times less on T w).
  if (!h->a3_host.empty() && h->ax[a + 1].a3s == 0 && L.lrest % LINE_R == 0) {
    const long long no_ = L.nouter, lr = L.lrest;
    const int a3x = h->ax[a].a3s;
    std::vector<double> f1((size_t)(no_ * n)), f2((size_t)(no_ * lr));
    bool ok = true;
    const double tol = 64.0 * 2.220446049250313e-16;
    for (long long o = 0; o < no_ && ok; ++o) {
      const double* M = h->a3_host.data() + outv[(size_t)o];
      const double piv = M[restv[0]];
      if (!(piv > 0.0) || !std::isfinite(piv)) { ok = false; break; }
      for (int x = 0; x < n; ++x) f1[(size_t)(o * n + x)] = M[(long long)x * a3x + restv[0]];
      for (long long q = 0; q < lr; ++q) f2[(size_t)(o * lr + q)] = M[restv[(size_t)q]] / piv;
      for (int x = 0; x < n && ok; ++x)
        for (long long q = 0; q < lr; ++q) {
          const double want = M[(long long)x * a3x + restv[(size_t)q]];
          const double got = f1[(size_t)(o * n + x)] * f2[(size_t)(o * lr + q)];
          if (!(std::fabs(got - want) <= tol * std::fabs(want))) { ok = false; break; }
        }
    }
    if (ok) {
      double *d1 = nullptr, *d2 = nullptr;
      if ((rc = upload(h, &d1, f1.data(), f1.size())) || (rc = upload(h, &d2, f2.data(), f2.size()))) return rc;
      L.f1 = d1; L.f2 = d2;
    }
  }
  return 0;
}

// dynamic LDS above 64 KB has to be allowed per kernel variant; which line passes run stream_kernels.hpp's forms
int prepare_fast_passes(sdfs_handle* h, std::vector<FastPass>& passes) {
  for (const FastPass& P : passes) {
    if (!P.line) for (int m = 0; m < S_NMODES; ++m) {
      slice_fn f = slice_variant(P.n, m);
      if (!f) return 1;
      hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)slice_lds_bytes(P.n, m));
      slice_fn f32 = slice_variant(P.n, m, true);
      if (f32) hipFuncSetAttribute((const void*)f32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)slice_lds_bytes(P.n, m));
      if (slice_fn m32 = slice32_variant(P.n)) hipFuncSetAttribute((const void*)m32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)slice32_lds_bytes(P.n));
    } else for (int m = 0; m < L_NMODES; ++m) {
      line_fn f = line_variant(P.n, m, P.ld.lrest % LINE_R == 0);
      if (!f) return 1;
      hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)line_lds_bytes(P.n));
      line_fn f32 = line_variant(P.n, m, true, true);
      if (f32) hipFuncSetAttribute((const void*)f32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)line_lds_bytes(P.n));
      for (int r32 = 16; r32 <= 32; r32 += 16) for (int d3 = 0; d3 < 2; ++d3)
        if (line_fn m32 = line32_variant(P.n, m, r32, d3 != 0)) hipFuncSetAttribute((const void*)m32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)line32_lds_bytes(P.n, r32));
      for (int r32 = 16; r32 <= 32; r32 += 16)
        if (line_fn s32 = line32_stream_mid_variant(P.n, r32)) hipFuncSetAttribute((const void*)s32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)line32_lds_bytes(P.n, r32));
    }
  }
  if (!h->sched) {
    HIPCHK(h, hipMalloc((void**)&h->sched, sizeof(unsigned) * SCHED_WORDS * 4));
    h->misc_allocs.push_back(h->sched);
    HIPCHK(h, hipMemset(h->sched, 0, sizeof(unsigned) * SCHED_WORDS * 4));
  }
  for (FastPass& P : passes) {
    if (P.line && P.ld.lrest % LINE_R == 0) {
      line_fn f = line_tlast32_variant(P.n);
      if (f) hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)line_lds_bytes(P.n));
    }
    // which forms pay was measured per extent (tools/ab_plan.py, profiles/round4_ab_stream_forms.txt: 24^6 -13.7 % with
    // both; 16^6 -2.7 % with the last pass only, its middle pass loses 11 %; 32-wide pairs -1.8 % with the middle pass
    // only, their last pass loses 5 %); SDFS_LINE_STREAM bit 2 = both forms on every extent
    const int pays = (h->knobs.line_stream & 4) ? 3 : (P.n == 16 ? 2 : (P.n == 32 ? 1 : 3));
    P.stream = (P.line && P.ld.lrest % LINE_R == 0) ? (h->knobs.line_stream & 3 & pays) : 0;
    if (!P.stream) continue;
    for (int m : {(int)L_MID, (int)L_TLAST, (int)L_TLAST_LIN}) for (int a3f = 0; a3f < 2; ++a3f) for (int early = 0; early < 2; ++early) {
      line_fn f = line_stream_variant(P.n, m, a3f != 0, early != 0);
      if (!f) return 1;
      hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)line_lds_bytes(P.n));
      if (line_fn f32 = line_stream_t32_variant(P.n, m, a3f != 0, early != 0))
        hipFuncSetAttribute((const void*)f32, hipFuncAttributeMaxDynamicSharedMemorySize, (int)line_lds_bytes(P.n));
    }
  }
  return 0;
}

// every axis with one unconditional transition matrix, extents in pairs the compile-time kernels exist for
bool pair_plan_legal(const sdfs_handle* h) {
  const int D = h->ndim;
  if (h->cont || h->dense || (D != 4 && D != 6) || h->a3 == nullptr) return false;
  if (h->N >= (1LL << 29)) return false;                   // 32-bit byte offsets inside a tile
  for (int a = 0; a < D; ++a) {
    if (h->ax[a].qcount != 1) return false;
    for (int c = 0; c < D; ++c) if (h->ax[a].qs[c] != 0) return false;
    if (h->ax[a].a3s < 0 || h->ax[a].a3s >= (1 << 24)) return false;
  }
  for (int a = 0; a < D; a += 2) {
    const int n = h->shape[a];
    if (n != h->shape[a + 1] || !(n == 16 || n == 20 || n == 24 || n == 32)) return false;
  }
  return true;
}

int build_fast_plan(sdfs_handle* h) {
  h->fast.ok = false;
  h->fast.small = false;
  h->fast.pad = false;
  h->fast.passes.clear();
  const int D = h->ndim;
  if (h->knobs.plan == 1 || h->sharded || !pair_plan_legal(h)) return 0;
  const int zero[MAXD] = {0, 0, 0, 0, 0, 0};
  std::vector<FastPass> passes(1);
  make_slice_pass(h, h->shape, passes[0]);
  long long min_tiles = 1LL << 60;
  const std::vector<int> pairs = pair_order(D);
  // (successive approximation ends its applications on either line pair in turn: a3 tables for every line pass)
  for (size_t i = 1; i < pairs.size(); ++i) {
    const int a = pairs[i];
    FastPass P;
    const int rc = make_line_pass(h, h->shape, zero, a, true, P);
    if (rc == 1) return 0;
    if (rc) return rc;
    min_tiles = std::min(min_tiles, P.ld.ntiles);
    passes.push_back(P);
  }
  if (h->knobs.plan != 2 && min_tiles < 2LL * h->num_cus) return 0;      // too few tiles to fill the chip
  {
    const int rc = prepare_fast_passes(h, passes);
    if (rc == 1) return 0;
    if (rc) return rc;
  }
  bool f32_ok = true;
  for (const FastPass& P : passes) if (P.line && P.ld.lrest % LINE_R != 0) f32_ok = false;
  h->fast.f32_ok = f32_ok;
  h->fast.passes = passes;
  h->fast.ok = true;
  return 0;
}

// Sharded stages on the pair plan's kernels (6-D grids whose shard axes lie in the two line pairs, one in each): with
// Kronecker-factorised expectations the order of the contractions is free, so
//   stage 0 (axis A blocked)  = the slice pass over the two fastest axes + the middle line pass over B's pair,
//   stage 1 (axis B blocked)  = the last line pass, with the aggregator, over A's pair --
// the same three kernels as on one GPU, on a block of the grid each, instead of the generic 80 KB tiles (1200 tiles
// over 512 slots at GCY 20^6 over eight ranks: tools/stage_kernel_times.py).  fp64 streams; fp32 Krylov storage keeps
// the generic stage plans.
int build_stage_fast_plans(sdfs_handle* h, int a_lo, int a_len, int b_lo, int b_len) {
  h->sfast[0].ok = h->sfast[1].ok = false;
  const int D = h->ndim;
  if (h->knobs.plan == 1 || !h->sharded || D != 6 || !pair_plan_legal(h)) return 0;
  const int pa = h->axis_a & ~1, pb = h->axis_b & ~1;
  if (pa == pb || pa == D - 2 || pb == D - 2) return 0;
  int shp[MAXD], off[MAXD] = {0, 0, 0, 0, 0, 0};
  for (int a = 0; a < D; ++a) shp[a] = h->shape[a];
  std::vector<FastPass> s0(2), s1(1);
  shp[h->axis_a] = a_len; off[h->axis_a] = a_lo;
  make_slice_pass(h, shp, s0[0]);
  int rc = make_line_pass(h, shp, off, pb, false, s0[1]);
  shp[h->axis_a] = h->shape[h->axis_a]; off[h->axis_a] = 0;
  if (rc == 1) return 0;
  if (rc) return rc;
  shp[h->axis_b] = b_len; off[h->axis_b] = b_lo;
  rc = make_line_pass(h, shp, off, pa, true, s1[0]);
  if (rc == 1) return 0;
  if (rc) return rc;
  if ((rc = prepare_fast_passes(h, s0)) || (rc = prepare_fast_passes(h, s1))) return rc == 1 ? 0 : rc;
  h->sfast[0].passes = s0; h->sfast[1].passes = s1;
  h->sfast[0].ok = h->sfast[1].ok = true;
  h->sfast[0].f32_ok = s0[1].ld.lrest % LINE_R == 0;
  h->sfast[1].f32_ok = s1[0].ld.lrest % LINE_R == 0;
  return 0;
}

// Small grids: every extent <= 16 (fast_kernels.hpp, small_tile_kernel).  Same pass structure as the pair plan:
// the two fastest axes first, then the slower pairs, the aggregator in the last pass.
int build_small_plan(sdfs_handle* h) {
  const int D = h->ndim;
  if (h->fast.ok || h->knobs.plan == 1 || h->knobs.small_plan == 0 || h->sharded || h->cont || h->dense ||
      (D != 4 && D != 6) || h->a3 == nullptr) return 0;
  // one wave per tile pays while the grid is latency-bound; from about half a million points on the generic tiles
  // are faster (tools/ab_small.py: 8^6 25 us against 28 us per step, 10^6 58 us against 50 us)
  if (h->N > 400000 && h->knobs.plan != 2) return 0;
  if (h->N >= (1LL << 24)) return 0;                       // 24-bit index products, 32-bit element offsets
  for (int a = 0; a < D; ++a) {
    if (h->ax[a].qcount != 1 || h->shape[a] > 16 || !h->ax[a].Qp || !h->ax[a].Qtp) return 0;
    for (int c = 0; c < D; ++c) if (h->ax[a].qs[c] != 0) return 0;
    if (h->ax[a].a3s < 0 || h->ax[a].a3s >= (1 << 24)) return 0;
  }
  long long stride[MAXD];
  { long long st = 1; for (int a = D - 1; a >= 0; --a) { stride[a] = st; st *= h->shape[a]; } }
  const std::vector<int> pairs = pair_order(D);
  const int zero[MAXD] = {0, 0, 0, 0, 0, 0};
  std::vector<FastPass> passes;
  for (size_t i = 0; i < pairs.size(); ++i) {
    const int a = pairs[i];
    FastPass P;
    P.small = true; P.line = i > 0; P.n = 16; P.ax0 = a; P.ax1 = a + 1;
    memset(&P.sd, 0, sizeof P.sd); memset(&P.ld, 0, sizeof P.ld); memset(&P.sm, 0, sizeof P.sm);
    SmallDesc& S = P.sm;
    S.nx = h->shape[a]; S.ny = h->shape[a + 1];
    S.my = (unsigned)((65536 + S.ny - 1) / S.ny);
    const long long lrest = stride[a + 1];
    const long long nouter = h->N / ((long long)S.nx * S.ny * lrest);
    S.sx = (unsigned)(S.ny * lrest); S.sy = (unsigned)lrest; S.lrest = (unsigned)lrest;
    S.ostride = (long long)S.nx * S.ny * lrest;
    // 32-byte runs once there is a tile for every CU (tools/ab_small.py: 8^6 25 us against 41 us per step with
    // single positions; 15^4, 57 tiles of four: 17.6 us against 11.7 us)
    int r = 1;
    if (lrest >= 4 && nouter * ((lrest + 3) / 4) >= (long long)h->num_cus) r = 4;
    if (lrest > 1 && (h->knobs.small_r == 1 || h->knobs.small_r == 4)) r = h->knobs.small_r;
    P.r = r;
    S.nchunks = (unsigned)((lrest + r - 1) / r);
    S.ntiles = nouter * S.nchunks;
    // a whole workgroup per tile while there are CUs to spare: the power then runs on all four SIMDs of a CU
    P.wpt = S.ntiles <= 2LL * h->num_cus ? 4 : 1;
    if (h->knobs.small_wpt == 1 || h->knobs.small_wpt == 4) P.wpt = h->knobs.small_wpt;
    if (S.ntiles >= (1LL << 31)) return 0;
    // strided pass with as many workgroups as fit the GPU at once: neighbouring tiles (they share their 128-byte
    // lines) to the same XCD (tools/probes/anderson_fused_probe.hip: 15^4 pair of passes 7.8 -> 7.0 us)
    S.cpx = 0;
    if (lrest > 1 && small_grid(S.ntiles, P.wpt) <= 2u * (unsigned)h->num_cus) S.cpx = small_cpx(S.ntiles, P.wpt);
    S.Qxp = h->ax[a].Qp; S.Qyp = h->ax[a + 1].Qp;
    S.theta = h->theta; S.inv_theta = 1.0 / h->theta; S.beta = h->beta;
    S.cbt = (double)powl((long double)h->beta, (long double)h->theta);
    S.a3x = h->ax[a].a3s; S.a3y = h->ax[a + 1].a3s;
    P.q_bytes = 2 * 8.0 * 256; P.flops = 2.0 * (double)h->N * (S.nx + S.ny);
    P.label = std::string(i == 0 ? "slices[" : "lines[") + h->ax[a].name + "," + h->ax[a + 1].name + "|wave " +
              std::to_string(S.nx) + "x" + std::to_string(S.ny) + "x" + std::to_string(r) + "]";
    if (P.wpt == 4) P.label.replace(P.label.find("|wave "), 6, "|workgroup ");
    // a3 index tables: the last pass of T needs them, and successive approximation ends on either end pair
    if (i + 1 == pairs.size() || i == 0) {
      std::vector<int> outv, restv;
      int *od = nullptr, *rd = nullptr;
      const int rc = a3_index_tables(h, h->shape, zero, a, outv, restv, &od, &rd);
      if (rc) return rc;
      S.a3 = h->a3; S.out_idx = od; S.rest_idx = rd;
    }
    passes.push_back(P);
  }
  h->fast.passes = passes;
  h->fast.f32_ok = false;
  h->fast.small = true;
  h->fast.ok = true;
  return 0;
}

// Grids between the plans (pad_kernels.hpp): unconditional tensors, every extent <= 32, neither the compile-time pair
// kernels' shapes nor the latency-tuned small-grid kernels' sizes (10^6 ... 15^6, 17^6 ... 19^6, ragged shapes): the
// pair plan on padded 16 / 24 / 32-wide tiles, chosen per pass.
int build_pad_plan(sdfs_handle* h) {
  const int D = h->ndim;
  if (h->fast.ok || h->knobs.plan == 1 || h->knobs.pad_plan == 0 || h->sharded || h->cont || h->dense || (D != 4 && D != 6) || h->a3 == nullptr) return 0;
  if (h->N >= (1LL << 31)) return 0;
  // Default: 6-D grids with every extent <= 16 (16-wide tiles, rows of 16 doubles), and grids -- 4-D or 6-D -- with every
  // extent in 17 ... 32 (20- / 24- / 32-wide tiles, rows of 8 doubles): 17^6 614 against 744 us per SA iteration on the
  // generic tiles, 21^6 2202 against 5272, 20^4 / 25^4 / 32^4 23 / 25 / 39 against 26 / 30 / 56.  Shapes that mix wide pairs
  // with small ones measured no gain (24x24x12x12x8x8: 169 against 156 us, 30x30x9x9x5x5: 115 against 102) and keep the
  // generic tiles unless SDFS_PAD_PLAN=2 (profiles/round3_ab_small_mid_grids.txt).
  int lo = 1 << 30, hi = 0;
  for (int a = 0; a < D; ++a) { lo = std::min(lo, h->shape[a]); hi = std::max(hi, h->shape[a]); }
  const bool all_small = hi <= 16, all_wide = lo >= 17 && hi <= 32;
  if (!(h->knobs.pad_plan >= 2 || (D == 6 && all_small) || all_wide)) return 0;
  const int max_ext = 32;
  for (int a = 0; a < D; ++a) {
    if (h->ax[a].qcount != 1 || h->shape[a] > max_ext || !h->ax[a].Qpad[3] || !h->ax[a].Qtpad[3]) return 0;
    for (int c = 0; c < D; ++c) if (h->ax[a].qs[c] != 0) return 0;
    if (h->ax[a].a3s < 0 || h->ax[a].a3s >= (1 << 24)) return 0;
  }
  long long stride[MAXD];
  { long long st = 1; for (int a = D - 1; a >= 0; --a) { stride[a] = st; st *= h->shape[a]; } }
  const std::vector<int> pairs = pair_order(D);
  const int zero[MAXD] = {0, 0, 0, 0, 0, 0};
  std::vector<FastPass> passes;
  for (size_t i = 0; i < pairs.size(); ++i) {
    const int a = pairs[i];
    FastPass P;
    P.pad = true; P.line = i > 0; P.ax0 = a; P.ax1 = a + 1;
    memset(&P.sd, 0, sizeof P.sd); memset(&P.ld, 0, sizeof P.ld); memset(&P.sm, 0, sizeof P.sm); memset(&P.pd, 0, sizeof P.pd);
    PadDesc& S = P.pd;
    S.nx = h->shape[a]; S.ny = h->shape[a + 1];
    const int nmax = std::max(S.nx, S.ny);
    const int cls = nmax <= 16 ? 0 : (nmax <= 20 ? 1 : (nmax <= 24 ? 2 : 3));
    P.nt = cls == 0 ? 16 : (cls == 1 ? 20 : (cls == 2 ? 24 : 32)); P.n = P.nt;
    S.mxy = (unsigned)(((1u << 20) + S.nx * S.ny - 1) / (S.nx * S.ny));
    S.my = (unsigned)(((1u << 20) + S.ny - 1) / S.ny);
    const long long lrest = stride[a + 1];
    const long long nouter = h->N / ((long long)S.nx * S.ny * lrest);
    S.lrest = lrest; S.nouter = nouter;
    S.nchunks = (int)((lrest + pad_line_r(P.nt) - 1) / pad_line_r(P.nt));
    S.ntiles = nouter * S.nchunks;
    S.nslices = nouter;                      // (slice form: lrest = 1)
    if (S.ntiles >= (1LL << 31)) return 0;
    S.Qx = h->ax[a].Qpad[cls]; S.Qy = h->ax[a + 1].Qpad[cls];
    S.theta = h->theta; S.inv_theta = 1.0 / h->theta; S.beta = h->beta;
    S.a3x = h->ax[a].a3s; S.a3y = h->ax[a + 1].a3s;
    P.q_bytes = 2 * 8.0 * P.nt * P.nt; P.flops = 2.0 * (double)h->N * (S.nx + S.ny);
    P.label = std::string(i == 0 ? "slices[" : "lines[") + h->ax[a].name + "," + h->ax[a + 1].name + "|" +
              std::to_string(S.nx) + "x" + std::to_string(S.ny) + " on " + std::to_string(P.nt) + "x" + std::to_string(P.nt) + "]";
    if (P.line && pad_line_lds(P.nt) > 64 * 1024)
      for (int lm : {L_MID, L_TLAST, L_TLAST_LIN, L_JLAST})
        hipFuncSetAttribute((const void*)pad_line_variant(P.nt, lm, lrest % 2 == 0), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad_line_lds(P.nt));
    if (i + 1 == pairs.size()) {
      // a3 index tables of the last pass
      std::vector<int> outv, restv;
      int *od = nullptr, *rd = nullptr;
      const int rc = a3_index_tables(h, h->shape, zero, a, outv, restv, &od, &rd);
      if (rc) return rc;
      S.a3 = h->a3; S.out_idx = od; S.rest_idx = rd;
    }
    passes.push_back(P);
  }
  // enough tiles to fill the chip, else the generic kernel's finer tiles do better (4-D grids never have them: both
  // ways are latency-bound there, and this one has fewer launches)
  if (D == 6 && passes[0].pd.nslices < 8LL * h->num_cus) return 0;
  h->fast.passes = passes;
  h->fast.f32_ok = false;
  h->fast.small = false;
  h->fast.pad = true;
  h->fast.ok = true;
  return 0;
}

// persistent middle pass of stream_kernels.hpp: a multiple of 8 workgroups (one ticket range per XCD)
unsigned stream_mid_grid(const sdfs_handle* h, const FastPass& P) {
  long long g = std::min<long long>(P.ld.ntiles, (long long)line_stream_wpc_mid(P.n) * h->num_cus);
  g -= g % 8;
  return (unsigned)std::max<long long>(g, 8);
}

// bf16r emulation (opts.krylov_f32 = 2): round an fp32 stream a J.v / linearising pass has just written
int round_stream_bf16_n(sdfs_handle* h, void* p, long long n, const unsigned long long* gate) {
  hipLaunchKernelGGL(k_round_bf16, dim3(std::min<long long>((n / 4 + 255) / 256 + 1, 8192)), dim3(256), 0, h->stream, (float*)p, n, gate);
  HIPCHK(h, hipGetLastError());
  return 0;
}

// What pass i launches for request `a` (PassLaunch, above): of the pair / small-grid / padded plan or sharded stage `fp`,
// or, with fp == nullptr, of the generic tiles of `plan`; nloc = grid points of the block
PassLaunch select_pass(const sdfs_handle* h, const FastPlan* fp, const Plan& plan, int i, long long nloc, bool has_first,
                       bool has_last, const Apply& a) {
  PassLaunch L;
  const bool vjp = a.mode == MODE_VJP;       // the J.v kernels with transposed matrices and c1 / c2 swapped (fp64)
  const int mode = vjp ? MODE_JVP : a.mode;
  // fp32 Krylov storage: every stream of a J.v application holds floats; a linearising T keeps fp64 streams and writes
  // only c1 (first pass) and c2 (last pass) as scaled floats
  const bool f32 = !vjp && a.f32() && mode != MODE_T;
  // opts.t_f32: the intermediates between the passes of a plain T application as scaled floats (whole chunks everywhere)
  // (a sharded handle's stages, sdfs_set_t_f32: stage 0 then WRITES floats -- the exchange moves half the bytes -- and
  // stage 1 reads them)
  const bool t32 = fp && mode == MODE_T && a.prec == PREC_T32 && fp->f32_ok && !fp->small &&
                   ((has_first && has_last) || (h->sharded && h->t32_ref > 0.0));
  const bool last = has_last && i == (int)(fp ? fp->passes.size() : plan.passes.size()) - 1;
  const double n8 = 8.0 * (double)nloc;
  L.tag = t32 ? "T32" : vjp ? "vjp" : (mode == MODE_JVP) ? (f32 ? "jvp32" : "jvp") : (mode == MODE_T_LIN ? "Tlin" : "T");
  L.bytes = 2 * n8 + (fp ? fp->passes[i].q_bytes : plan.passes[i].q_bytes);
  // first pass: c1 written (linearising T) or read (J.v); last pass: the epilogue's extra streams
  const int first_bytes = mode == MODE_T ? 0 : 1;
  auto last_mode = [&](int t, int tlin, int j) {
    if (mode == MODE_T) { if (a.resid) L.bytes += n8; return t; }
    L.bytes += n8;
    if (mode == MODE_T_LIN) { if (a.resid) L.bytes += n8; return tlin; }
    if (a.minus_identity) L.bytes += n8;
    return j;
  };
  if (!fp) {
    // generic tiles (pass_kernel.hpp): one kernel, the first and the last pass of the operator in modes of their own
    const Pass& G = plan.passes[i];
    const bool first = has_first && i == 0;
    L.kmode = M_MID;
    if (first) {
      L.kmode = mode == MODE_T ? M_TFIRST : (mode == MODE_T_LIN ? M_TFIRST_LIN : M_JFIRST);
      L.bytes += first_bytes * n8;
    }
    if (last) {
      L.kmode = last_mode(M_TLAST, M_TLAST_LIN, M_JLAST);
      // (a linearising pass writes c1 or c2 to the one aux_out, a J.v pass reads c1 or c2 from the one aux_in)
      if (first && mode == MODE_T) L.kmode = M_TONLY;
      else if (first) L.err = mode == MODE_T_LIN ? "single-pass linearise not supported" : "single-pass JVP not supported";
    }
    // (a linearising T stores floats only where it writes c1 and c2)
    L.f32 = f32 && (mode == MODE_JVP || first || last);
    if (L.f32 && mode == MODE_JVP) L.bytes *= 0.5;
    L.grid = (unsigned)G.d.ntiles; L.block = G.block; L.lds = G.lds_bytes;
    return L;
  }
  const FastPass& P = fp->passes[i];
  if (P.pad) {
    if (!P.line) {
      L.kmode = mode == MODE_T_LIN ? S_TFIRST_LIN : (mode == MODE_JVP ? S_JFIRST : S_TFIRST);
      L.bytes += first_bytes * n8;
      L.fn = (const void*)pad_slice_variant(P.nt, L.kmode, P.pd.nx * P.pd.ny);
      L.grid = (unsigned)(((P.pd.nslices + pad_slice_g(P.nt) - 1) / pad_slice_g(P.nt) + 3) / 4);
    } else {
      L.kmode = last ? last_mode(L_TLAST, L_TLAST_LIN, L_JLAST) : L_MID;
      L.fn = (const void*)pad_line_variant(P.nt, L.kmode, P.pd.lrest % 2 == 0);
      L.grid = (unsigned)P.pd.ntiles; L.block = pad_line_block(P.nt); L.lds = pad_line_lds(P.nt);
    }
    if (!L.fn) L.err = "no padded-plan kernel variant";
    return L;
  }
  if (P.small) {
    if (i == 0) {
      L.kmode = mode == MODE_T ? SM_FIRST_T : (mode == MODE_T_LIN ? SM_FIRST_TLIN : SM_FIRST_J);
      L.bytes += first_bytes * n8;
    } else if (last) {
      L.kmode = last_mode(SM_LAST_T, SM_LAST_TLIN, SM_LAST_J);
      if (mode == MODE_JVP && a.dotp && a.dot_with) { L.dot_with = a.dot_with; L.bytes += n8; }
    } else L.kmode = SM_MID;
    L.fn = (const void*)small_variant(L.kmode, P.r, P.wpt);
    L.grid = small_grid(P.sm, P.wpt);
    if (!L.fn) L.err = "no small-grid kernel variant";
    return L;
  }
  // opts.krylov_f32 = 3: fp32 LDS tile + fp32 MFMA for the J.v passes (f32_kernels.hpp)
  const bool m32 = f32 && a.prec == PREC_MFMA32 && mode == MODE_JVP && !t32;
  const bool bicg = mode == MODE_JVP && !vjp && a.bicg.kind >= 0;
  L.m32 = m32;
  if (!P.line) {
    int sm = S_TFIRST;
    if (t32) { sm = S_TFIRST32; L.bytes -= 0.5 * n8; }
    if (mode == MODE_T_LIN) sm = S_TFIRST_LIN;
    else if (mode == MODE_JVP) sm = S_JFIRST;
    L.bytes += first_bytes * n8;
    L.kmode = sm;
    const int gsl = m32 ? slice32_tile_slices(P.n) : slice_tile_slices(P.n, sm);
    L.lds = m32 ? slice32_lds_bytes(P.n) : slice_lds_bytes(P.n, sm);
    if (bicg && (!f32 || m32)) {
      // BiCGSTAB's p / s update on the registers of this pass (krylov_kernels.hpp; fp32-MFMA: vectors, c1 and the output
      // are floats)
      const int kind = a.bicg.kind;
      if (!m32 && a.lc1) { L.err = "the fused BiCGSTAB first pass reads the cached linearisation only"; L.err_code = SDFS_ERR_ARG; return L; }
      L.jfused = true;
      L.fn = m32 ? (const void*)slice32_jfused_variant(P.n, kind) : (const void*)slice_jfused_variant(P.n, kind);
      if (!L.fn) L.err = m32 ? "no fused fp32 first pass for this extent" : "no fused first pass for this extent";
      L.bytes = (m32 ? 0.5 : 1.0) * (kind == JF_P ? 6.0 : 5.0) * n8 + P.q_bytes;
      L.tag = m32 ? (kind == JF_P ? "jvpm32+p" : "jvpm32+s") : (kind == JF_P ? "jvp+p" : "jvp+s");
    } else {
      L.fn = m32 ? (const void*)slice32_variant(P.n) : (const void*)slice_variant(P.n, sm, f32);
      if (!L.fn) L.err = "no slice kernel variant";
      if (f32 && mode == MODE_JVP) L.bytes *= 0.5;
      if (m32) L.tag = "jvpm32";
    }
    L.grid = (unsigned)(((P.sd.nslices + gsl - 1) / gsl + 3) / 4);
    return L;
  }
  const int lm = last ? last_mode(L_TLAST, L_TLAST_LIN, L_JLAST) : L_MID;
  const bool lf32 = f32 && (mode == MODE_JVP || lm == L_TLAST_LIN);
  const bool a3f = P.ld.f1 != nullptr;
  L.kmode = lm;
  line_fn fn = lf32 ? line_variant(P.n, lm, true, true) : line_variant(P.n, lm, P.ld.lrest % LINE_R == 0);
  unsigned grid = (unsigned)P.ld.ntiles;
  if (t32) {
    // fp32 intermediate: the fp32 middle form, or the last pass on a float tile (stream_kernels.hpp) ...
    fn = last ? line_tlast32_variant(P.n) : line_variant(P.n, L_MID, true, true);
    L.bytes -= last ? 0.5 * n8 : n8;
    // ... on the streamed forms where the fp64 passes run them (stream_kernels.hpp, IN32 / OUT32)
    if ((P.stream & (last ? 2 : 1)) && h->knobs.no_f32_stream == 0) {
      if (line_fn sf = line_stream_t32_variant(P.n, last ? L_TLAST : L_MID, a3f, last && a.resid != nullptr && a.old != nullptr)) {
        fn = sf;
        if (!last) {
          long long g = std::min<long long>(P.ld.ntiles, (long long)line_stream_wpc_mid32(P.n) * h->num_cus);
          g -= g % 8;
          grid = (unsigned)std::max<long long>(g, 8);
        }
      }
    }
  } else if (!lf32 && ((lm == L_MID && (P.stream & 1)) || ((lm == L_TLAST || lm == L_TLAST_LIN) && (P.stream & 2)))) {
    // stream_kernels.hpp: persistent middle pass with the next tile in flight; last pass with its side stream loaded early
    if (lm == L_MID) grid = stream_mid_grid(h, P);
    if (lm == L_TLAST && a.push.r != nullptr && a.old != nullptr && P.ld.ntiles <= (long long)MAX_PARTIAL_BLOCKS * AND_MAX_M) {
      L.push = true;
      L.bytes += 3 * n8;                                   // x read, y and r written
    }
    // (the side stream travels with the tile only in a launch that reads it: the residual's w, the push's x)
    fn = line_stream_variant(P.n, lm, a3f, lm == L_TLAST && a.old != nullptr && (a.resid != nullptr || L.push));
  }
  if (lm == L_JLAST && !lf32 && bicg) {
    // fused BiCGSTAB iteration: the streamed last pass, one workgroup per tile (the partial sums are counted per tile)
    fn = line_stream_variant(P.n, L_JLAST);
    L.dot_with = a.bicg.dot_with;
    L.bytes += 0.5 * n8;       // (rhat is read by the first of an iteration's two applications: one counter, their mean)
  }
  if (m32) {
    const int r32 = line32_row_floats(P.n, P.ld.lrest);
    fn = line32_variant(P.n, lm, r32);
    grid = (unsigned)(P.ld.ntiles * LINE_R / r32);
    if (lm == L_MID && (P.stream & 1) && grid >= 8u * TK_SUB && h->knobs.no_f32_stream == 0) {
      // persistent form, next tile in flight (krylov_kernels.hpp); a multiple of 8 workgroups, one ticket range per XCD
      if (line_fn sf = line32_stream_mid_variant(P.n, r32)) {
        long long g = std::min<long long>(grid, (long long)line32_stream_wpc(P.n, r32) * h->num_cus);
        g -= g % (8 * TK_SUB);
        fn = sf; grid = (unsigned)g;
        L.persistent = true;
      }
    }
    if (lm == L_JLAST && bicg) {
      L.dot_with = a.bicg.dot_with;
      L.bytes += n8;            // (halved below: the mean of the two applications)
      if (L.dot_with) fn = line32_variant(P.n, lm, r32, true);
    }
    L.tag = "jvpm32"; L.block = 256; L.lds = line32_lds_bytes(P.n, r32);
  } else {
    L.block = line_block(P.n); L.lds = line_lds_bytes(P.n);
  }
  if (f32 && mode == MODE_JVP) L.bytes *= 0.5;
  L.fn = (const void*)fn;
  L.grid = grid;
  if (!fn) L.err = "no line kernel variant";
  return L;
}

// the generic tile kernel has no word to clear ahead of the residual's atomicMax (its callers clear it)
void clear_word(PassIO&, unsigned long long*) {}
template <typename IO> void clear_word(IO& io, unsigned long long* word) { io.zero = word; }

// One application: the passes of fp -- the whole-grid pair / small-grid / padded plan (has_first and has_last), or one
// stage of a sharded handle (build_stage_fast_plans: stage 0 holds the first pass, stage 1 the last) -- or, with
// fp == nullptr, of the generic tiles of `plan` (conditional tensors, extents above 16, sharded stages, the fp32-storage
// fallback).  has_first / has_last tell whether the block holds the operator's first pass (prologue) and last pass
// (epilogue): a sharded stage holds only one.
int run_passes(sdfs_handle* h, const FastPlan* fp, const Plan& plan, bool has_first, bool has_last, const Apply& a) {
  const bool vjp = a.mode == MODE_VJP;
  const int mode = vjp ? MODE_JVP : a.mode;
  // J.v scalings: the cached linearisation, or the caller's (the tilted expectation's d1 / d2)
  const double* const C1 = a.lc1 ? a.lc1 : h->c1;
  const double* const C2 = a.lc2 ? a.lc2 : h->c2;
  int rc = ensure_tmp(h);
  if (rc) return rc;
  if (mode != MODE_T) { rc = ensure_lin(h); if (rc) return rc; }
  const long long nloc = fp == &h->fast ? h->N : plan.nloc;      // grid points of the block
  const int np = (int)(fp ? fp->passes.size() : plan.passes.size());
  const bool bf16 = !vjp && a.prec == PREC_BF16 && mode != MODE_T;
  // every pass reads the grid or the intermediate and writes the intermediate or the result, gated on the caller's word
  auto open_io = [&](auto& io, int i) {
    memset(&io, 0, sizeof io);
    io.in = (i == 0) ? a.in : h->tmp; io.out = (i == np - 1) ? a.out : h->tmp;
    io.gate = a.gate; io.gate_tol = a.gate_tol;
  };
  // the first pass clears the word the last pass maximises into, and reads / writes c1; the last one reads / writes c2
  auto first_io = [&](auto& io) {
    clear_word(io, (mode != MODE_JVP) ? a.resid : nullptr);
    if (mode == MODE_T_LIN) io.aux_out = h->c1;
    else if (mode == MODE_JVP) io.aux_in = vjp ? C2 : C1;
  };
  auto last_io = [&](auto& io) {
    io.old = a.old;
    if (mode == MODE_JVP) { io.aux_in = vjp ? C1 : C2; if (a.minus_identity) io.dotp = a.dotp; return; }
    io.resid = a.resid;
    if (mode == MODE_T_LIN) io.aux_out = h->c2;
  };
  for (int i = 0; i < np; ++i) {
    const bool first = has_first && i == 0, last = has_last && i == np - 1;
    const PassLaunch L = select_pass(h, fp, plan, i, nloc, has_first, has_last, a);
    if (L.err) return fail(h, L.err_code, "%s", L.err);
    double* const pout = (i == np - 1) ? a.out : h->tmp;
    if (!fp) {
      PassIO io;
      open_io(io, i);
      if (first) first_io(io);
      if (last) last_io(io);
      rc = launch_pass(h, plan.passes[i], L, io, a.minus_identity, vjp);
    } else if (const FastPass& P = fp->passes[i]; P.pad) {
      PadDesc d = P.pd;
      d.minus_identity = a.minus_identity;
      const int cls = P.nt == 16 ? 0 : (P.nt == 20 ? 1 : (P.nt == 24 ? 2 : 3));
      if (vjp) { d.Qx = h->ax[P.ax0].Qtpad[cls]; d.Qy = h->ax[P.ax1].Qtpad[cls]; }
      if (!P.line) {
        SliceIO io;
        open_io(io, i);
        first_io(io);
        rc = launch_selected(h, L, P, d, io);
      } else {
        LineIO io;
        open_io(io, i);
        if (last) last_io(io);
        rc = launch_selected(h, L, P, d, io);
      }
    } else if (P.small) {
      SmallIO io;
      open_io(io, i);
      SmallDesc d = P.sm;
      d.minus_identity = a.minus_identity;
      if (vjp) { d.Qxp = h->ax[P.ax0].Qtp; d.Qyp = h->ax[P.ax1].Qtp; }
      if (i == 0) first_io(io);
      else if (last) { last_io(io); io.dot_with = L.dot_with; }
      rc = launch_selected(h, L, P, d, io);
    } else if (!P.line) {
      SliceDesc sd = P.sd;
      if (vjp) { sd.Qf = h->ax[P.ax1].Qt; sd.Qe = h->ax[P.ax0].Qt; }
      if (h->sharded) sd.t32_ref = h->t32_ref;
      if (L.jfused && L.m32) {
        JFused32IO jio;
        memset(&jio, 0, sizeof jio);
        jio.upd = (float*)a.bicg.upd; jio.a = (const float*)a.bicg.a; jio.q = (const float*)a.bicg.q; jio.c1 = (const float*)h->c1;
        jio.out = (float*)pout; jio.sc = h->sc; jio.dot = a.bicg.dot; jio.gate = a.gate;
        rc = launch_selected(h, L, P, sd, jio);
      } else if (L.jfused) {
        JFusedIO jio;
        memset(&jio, 0, sizeof jio);
        jio.upd = a.bicg.upd; jio.a = a.bicg.a; jio.q = a.bicg.q; jio.c1 = h->c1; jio.out = pout; jio.sc = h->sc;
        jio.dot = a.bicg.dot; jio.gate = a.gate;
        rc = launch_selected(h, L, P, sd, jio);
      } else {
        SliceIO io;
        open_io(io, i);
        first_io(io);
        rc = launch_selected(h, L, P, sd, io);
      }
    } else {
      LineIO io;
      open_io(io, i);
      io.sched = h->sched + SCHED_WORDS * i;
      LineDesc d = P.ld;
      d.minus_identity = a.minus_identity;
      if (h->sharded) d.t32_ref = h->t32_ref;
      if (vjp) { d.Qx = h->ax[P.ax0].Qt; d.Qy = h->ax[P.ax1].Qt; }
      if (last) last_io(io);
      io.dot_with = L.dot_with;
      if (L.push) {
        io.and_y = a.push.y; io.and_r = a.push.r; io.and_beta = a.push.beta; io.and_dot = a.push.dot;
        if (a.push.tiles) *a.push.tiles = P.ld.ntiles;
      }
      rc = launch_selected(h, L, P, d, io);
    }
    if (rc) return rc;
    if (bf16) {
      // bf16r emulation: what this pass stored as floats is rounded to bfloat16 (the BiCGSTAB gate is a zero word when closed)
      if (mode == MODE_JVP && (rc = round_stream_bf16_n(h, pout, nloc, a.gate))) return rc;
      if (mode == MODE_T_LIN && first && (rc = round_stream_bf16_n(h, h->c1, nloc, nullptr))) return rc;
      if (mode == MODE_T_LIN && last && (rc = round_stream_bf16_n(h, h->c2, nloc, nullptr))) return rc;
    }
  }
  return 0;
}

// The pair / small-grid / padded plan, or a sharded stage on the pair plan's kernels, that serves request `a` on `plan`;
// nullptr: the generic tiles.  The pair plan's fp32-storage forms need whole 16-element chunks in every line pass, otherwise
// fp32 Krylov storage (and its linearisation) stays on the generic kernels; the sharded stages run fp64 streams only.
FastPlan* fast_plan_for(sdfs_handle* h, const Plan& plan, bool has_first, bool has_last, const Apply& a) {
  const bool f32 = a.f32() && a.mode != MODE_T;
  if (h->fast.ok && &plan == &h->plan[0] && has_first && has_last && !(f32 && !h->fast.f32_ok)) return &h->fast;
  const int st = &plan == &h->plan[0] ? 0 : (&plan == &h->plan[1] ? 1 : -1);
  if (h->sharded && st >= 0 && h->sfast[st].ok && a.mode != MODE_VJP && !f32 && has_first == (st == 0) && has_last == (st == 1))
    return &h->sfast[st];
  return nullptr;
}

// workgroups of the last pass of the whole-grid application `a` (one partial sum each of the fused dot products)
long long last_pass_grid(sdfs_handle* h, const Apply& a) {
  if (h->cont || h->dense) return 0;
  const FastPlan* fp = fast_plan_for(h, h->plan[0], true, true, a);
  const int np = (int)(fp ? fp->passes.size() : h->plan[0].passes.size());
  return np ? select_pass(h, fp, h->plan[0], np - 1, h->N, true, true, a).grid : 0;
}

// One application on `plan` (the whole grid, or a stage of a sharded handle): the continuous or the dense operator, or the
// passes of the plan that serves the request
int run_plan(sdfs_handle* h, Plan& plan, bool has_first, bool has_last, const Apply& a) {
  // (a continuous handle's transpose is the scatter form of its own kernel, reached through sdfs_cont_apply_vjp_dev /
  // sdfs_cont_solve_adjoint_dev alone: sdfs_apply_vjp_dev and sdfs_solve_linear_dev refuse it before they get here)
  if (a.mode == MODE_VJP && !h->cont) {
    if (h->dense) return fail(h, SDFS_ERR_UNSUPPORTED, "the vector-Jacobian product exists for the discretised operator only");
    for (int ax = 0; ax < h->ndim; ++ax)
      if (!h->ax[ax].Qt) return fail(h, SDFS_ERR_UNSUPPORTED, "the vector-Jacobian product needs unconditional transition tensors "
                                     "(axis %s is conditional)", h->ax[ax].name);
  }
  if (h->cont) return run_cont(h, a);
  if (h->dense) return run_dense(h, a);
  return run_passes(h, fast_plan_for(h, plan, has_first, has_last, a), plan, has_first, has_last, a);
}

// one application on the whole grid
int apply(sdfs_handle* h, const Apply& a) { return run_plan(h, h->plan[0], true, true, a); }

int apply_T_dev(sdfs_handle* h, const double* w, double* Tw, unsigned long long* resid,
                const unsigned long long* gate, double gate_tol, int prec = PREC_F64) {
  Apply a(MODE_T, w, Tw, w);
  a.resid = resid; a.gate = gate; a.gate_tol = gate_tol; a.prec = prec;
  return apply(h, a);
}

int ensure_slots(sdfs_handle* h, int n) {
  if (h->nslots >= n + 2) return 0;
  if (h->slots) { hipFree(h->slots); hipHostFree(h->slots_host); }
  h->nslots = n + 2;
  HIPCHK(h, hipMalloc((void**)&h->slots, sizeof(unsigned long long) * h->nslots));
  HIPCHK(h, hipHostMalloc((void**)&h->slots_host, sizeof(unsigned long long) * h->nslots));
  return 0;
}

int ensure_buf(sdfs_handle* h, double** p) {
  if (*p) return 0;
  return dev_alloc(h, p, (size_t)h->N);
}

int ensure_scalars(sdfs_handle* h) {
  if (!h->partial) { int rc = dev_alloc(h, &h->partial, (size_t)MAX_PARTIAL_BLOCKS * AND_MAX_M); if (rc) return rc; }
  if (!h->sc) {
    int rc = dev_alloc(h, &h->sc, SC_COUNT); if (rc) return rc;
    HIPCHK(h, hipHostMalloc((void**)&h->sc_host, sizeof(double) * SC_COUNT));
  }
  return 0;
}

// Successive approximation on the 6-D pair plan (fast_kernels.hpp, L_TFUSED): the contraction order of an
// application is free, so iteration `it` runs [slices, plain contraction] [lines L(it), fused], where the fused
// kernel closes application `it` on line pair L(it) = passes[1 + (it & 1)] (aggregator, residual, Tw) and opens
// application it+1 on the same pair.  Invariant before iteration `it`: h->tmp holds w_it^theta contracted over
// the OTHER line pair.  7 grid streams per iteration become 6, the strided middle pass becomes a contiguous one.
int big_sa_line(sdfs_handle* h, int pass, bool first_only, const double* in, double* w_new, const double* w_old,
                unsigned long long* resid, const unsigned long long* gate, double gate_tol) {
  const FastPass& P = h->fast.passes[pass];
  LineIO io;
  memset(&io, 0, sizeof io);
  io.in = in; io.out = w_new; io.old = w_old; io.resid = resid; io.aux_out = h->tmp; io.gate = gate; io.gate_tol = gate_tol;
  io.sched = h->sched + SCHED_WORDS * pass;
  LineDesc d = P.ld;
  d.first_only = first_only ? 1 : 0;
  line_fn fn = line_variant(P.n, L_TFUSED, P.ld.lrest % LINE_R == 0);
  if (!fn) return fail(h, SDFS_ERR_UNSUPPORTED, "no fused line kernel variant");
  const double n8 = 8.0 * (double)h->N;
  return launch_kernel(h, fn, dim3((unsigned)d.ntiles), dim3(line_block(P.n)), line_lds_bytes(P.n),
                       Counter("sa", P.label, (first_only ? 2 : 4) * n8 + P.q_bytes, (first_only ? 1 : 2) * P.flops, first_only ? "open " : "fused "), d, io);
}

int big_sa_iteration(sdfs_handle* h, long long it, const double* w_old, double* w_new, unsigned long long* resid,
                     const unsigned long long* gate, double gate_tol) {
  const FastPass& P = h->fast.passes[0];
  SliceIO io;
  memset(&io, 0, sizeof io);
  io.in = h->tmp; io.out = h->tmp; io.gate = gate; io.gate_tol = gate_tol;
  slice_fn fn = slice_variant(P.n, S_MID, false);
  if (!fn) return fail(h, SDFS_ERR_UNSUPPORTED, "no plain slice kernel variant");
  const long long ntile = (P.sd.nslices + slice_tile_slices(P.n, S_MID) - 1) / slice_tile_slices(P.n, S_MID);
  if (int rc = launch_kernel(h, fn, dim3((unsigned)((ntile + 3) / 4)), dim3(256), slice_lds_bytes(P.n, S_MID),
                             Counter("sa", P.label, 16.0 * (double)h->N + P.q_bytes, P.flops), P.sd, io))
    return rc;
  return big_sa_line(h, 1 + (int)(it & 1), false, h->tmp, w_new, w_old, resid, gate, gate_tol);
}

// Successive approximation on the small-grid plan (fast_kernels.hpp, SM_FUSED_T): the pair order is reversed
// every iteration, so the last pass of one application and the first pass of the next act on the same pair and
// run as one kernel.  Invariant before iteration `it`: h->tmp holds the first pair of this iteration's order
// already contracted over w_it^theta.  4-D: one launch per iteration; 6-D: two.
int small_sa_prologue(sdfs_handle* h, const double* w) {
  const FastPass& P = h->fast.passes[0];
  SmallIO io;
  memset(&io, 0, sizeof io);
  io.in = w; io.out = h->tmp;
  small_fn fn = small_variant(SM_FIRST_T, P.r, P.wpt);
  if (!fn) return fail(h, SDFS_ERR_UNSUPPORTED, "no small-grid kernel variant");
  return launch_kernel(h, fn, dim3(small_grid(P.sm, P.wpt)), dim3(256), 0, Counter("sa", P.label, 16.0 * (double)h->N, P.flops, "first "), P.sm, io);
}

constexpr int SA_RING = SMALL_RING;   // most workgroups of an end pass for which the atomic-free residual is used

// ring == true: the error of iteration it-1 is reduced by this iteration's kernels from sa_ring[(it-1) & 1] (and left
// in slot_prev for the host), this iteration's maxima go to sa_ring[it & 1]; otherwise resid / gate words as everywhere
int small_sa_iteration(sdfs_handle* h, long long it, const double* w_old, double* w_new, unsigned long long* resid,
                       const unsigned long long* gate, double gate_tol, bool ring, unsigned long long* slot_prev) {
  const int np = (int)h->fast.passes.size();
  const bool forward = (it & 1) == 0;
  const double n8 = 8.0 * (double)h->N;
  // writer of ring[p]: the end pass of the iterations of parity p (forward iterations end on the last pair)
  auto ring_n = [&](int parity) { const FastPass& E = h->fast.passes[parity == 0 ? np - 1 : 0]; return (int)small_grid(E.sm, E.wpt); };
  for (int j = 1; j < np; ++j) {
    const FastPass& P = h->fast.passes[forward ? j : np - 1 - j];
    const bool last = j == np - 1;
    SmallIO io;
    memset(&io, 0, sizeof io);
    io.in = h->tmp; io.gate_tol = gate_tol;
    if (ring) { io.gate_part = h->sa_ring + (size_t)((it + 1) & 1) * SA_RING; io.gate_n = ring_n((int)((it + 1) & 1)); }
    else io.gate = gate;
    if (last) {
      io.out = w_new; io.old = w_old; io.aux_out = h->tmp;
      if (ring) { io.part_out = h->sa_ring + (size_t)(it & 1) * SA_RING; io.slot_out = slot_prev; }
      else io.resid = resid;
    } else io.out = h->tmp;
    small_fn fn = small_variant(last ? SM_FUSED_T : SM_MID, P.r, P.wpt);
    if (!fn) return fail(h, SDFS_ERR_UNSUPPORTED, "no small-grid kernel variant");
    if (int rc = launch_kernel(h, fn, dim3(small_grid(P.sm, P.wpt)), dim3(256), 0,
                               Counter("sa", P.label, (last ? 4 : 2) * n8, (last ? 2 : 1) * P.flops, last ? "fused " : ""), P.sm, io))
      return rc;
  }
  return 0;
}

double bits_to_double(unsigned long long b) { double d; memcpy(&d, &b, 8); return d; }

long long lcm(long long a, long long b) { long long x = a, y = b; while (y) { const long long t = x % y; x = y; y = t; } return a / x * b; }

// What `enqueue` launches on the handle's stream, captured and instantiated into *exec (in place of the graph it held)
template <typename F>
int capture_graph(sdfs_handle* h, hipGraphExec_t* exec, F&& enqueue) {
  if (*exec) { hipGraphExecDestroy(*exec); *exec = nullptr; }
  hipGraph_t g = nullptr;
  HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue();
  hipError_t e = hipStreamEndCapture(h->stream, &g);
  if (rc || e != hipSuccess) {
    if (g) hipGraphDestroy(g);
    if (rc) return rc;
    HIPCHK(h, e);
  }
  e = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  HIPCHK(h, e);
  return 0;
}

// ---------------------------------------------------------------------------
// successive approximation (code/solvers.py:19-48), all iterations on the device.
// Iteration it computes x_{it+1} = T(x_it) and err_it = max|x_{it+1} - x_it| into
// slot it%chunk; every later kernel is gated on the previous slot, so once
// err <= tol the remaining launches of the chunk are no-ops and the iterate stays.
// prec: the storage of T's intermediates (PREC_T32: phase A of opts.t_f32, below)
int solve_sa(sdfs_handle* h, const sdfs_opts& o, double* w, int64_t* n_iter, int64_t* n_apply, double* final_err,
             int prec = PREC_F64) {
  int rc;
  if (o.t_f32 && prec != PREC_T32 && h->fast.ok && !h->fast.small && h->fast.f32_ok && !h->cont && !h->dense && !h->sharded) {
    // BASELINE config 5, T passes: phase A applies T with its intermediates stored as scaled floats (40 instead of 56
    // bytes per point and iteration) down to a step just above what that storage can resolve, phase B finishes in
    // fp64 from there.  One stored float carries 2^-24 relative, i.e. ~ w 2^-24 / |theta| on T w after the 1/theta
    // power; the step of two consecutive iterates stops shrinking geometrically at a few of those (at 16 of them phase
    // A lingered: 551 against 499 iterations at SSY 32x32x16x16), so the switch is at 64.  (The iterate path differs
    // from the all-fp64 one at that level, so the iteration COUNT is this configuration's own, not the reference's.)
    double wref = 0.0;
    // (on the handle's stream: sdfs_solve's upload, or the caller's writes under sdfs_set_stream, precede it there; the
    // handle's own stream does not synchronise with the null stream)
    HIPCHK(h, hipMemcpyAsync(&wref, w + h->fast.passes[0].sd.ref_off, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const double switch_tol = 64.0 * std::ldexp(1.0, -24) * std::fabs(wref) / std::max(std::fabs(h->theta), 1.0);
    if (std::isfinite(switch_tol) && switch_tol > o.tol) {
      sdfs_opts oa = o;
      oa.t_f32 = 0; oa.tol = switch_tol; oa.use_graph = 0;
      int64_t it_a = 0, ap_a = 0;
      double err_a = 0.0;
      rc = solve_sa(h, oa, w, &it_a, &ap_a, &err_a, PREC_T32);
      const std::vector<double> trace_a = h->trace;
      *n_iter = it_a; *n_apply = ap_a; *final_err = err_a;
      if (rc || it_a >= o.max_iter) return rc;
      sdfs_opts ob = o;
      ob.t_f32 = 0; ob.max_iter = o.max_iter - it_a;
      int64_t it_b = 0, ap_b = 0;
      rc = solve_sa(h, ob, w, &it_b, &ap_b, final_err);
      *n_iter = it_a + it_b; *n_apply = ap_a + ap_b;
      h->trace.insert(h->trace.begin(), trace_a.begin(), trace_a.end());
      return rc;
    }
  }
  if ((rc = ensure_buf(h, &h->buf0)) || (rc = ensure_buf(h, &h->buf1)) || (rc = ensure_tmp(h))) return rc;
  int chunk = std::max(1, o.check_every);
  if (o.use_graph && (chunk & 1)) ++chunk;                  // even: ping-pong parity repeats per replay
  if ((rc = ensure_slots(h, chunk))) return rc;
  unsigned long long* carry = h->slots + chunk;             // error of the last iteration of the previous chunk
  const size_t nb = sizeof(double) * (size_t)h->N;
  HIPCHK(h, hipMemcpyAsync(h->buf0, w, nb, hipMemcpyDeviceToDevice, h->stream));
  h->slots_host[chunk] = ~0ULL;                             // "not converged yet"
  HIPCHK(h, hipMemcpyAsync(carry, h->slots_host + chunk, 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->trace.clear();
  double* bufs[2] = {h->buf0, h->buf1};
  // small-grid plan: last pass of iteration k and first pass of iteration k+1 in one kernel (pair order alternates)
  const bool fused = h->fast.ok && h->fast.small && !h->cont && !h->dense && h->knobs.sa_fused != 0;
  if (fused && (rc = small_sa_prologue(h, h->buf0))) return rc;
  // 6-D pair plan: plain slice pass + fused line pass per iteration
  // (round 4, tools/sa_rate.py: with this round's first and last passes the three launches of T win on every extent --
  // 16^6 0.195 against 0.207 ms per iteration, 24^6 2.45 against 2.71, 32^4 x 16^2 4.21 against 4.45 -- so the fused form
  // runs on request only)
  const bool fusedbig = h->fast.ok && !h->fast.small && !h->fast.pad && h->fast.passes.size() == 3 && !h->cont && !h->dense && h->knobs.sa_fused > 0 &&
                        prec != PREC_T32;
  if (fusedbig && (rc = big_sa_line(h, 2, true, h->buf0, nullptr, nullptr, nullptr, nullptr, 0.0))) return rc;
  // ... and the residual without atomics: per-workgroup maxima, reduced by the next iteration's kernels
  bool ring = false;
  int ring_n[2] = {0, 0};
  if (fused && h->knobs.sa_fused != 2) {
    const FastPass& E0 = h->fast.passes.back();
    const FastPass& E1 = h->fast.passes.front();
    ring_n[0] = (int)small_grid(E0.sm, E0.wpt); ring_n[1] = (int)small_grid(E1.sm, E1.wpt);
    ring = ring_n[0] <= SA_RING && ring_n[1] <= SA_RING;
  }
  if (ring) {
    if (!h->sa_ring) {
      HIPCHK(h, hipMalloc((void**)&h->sa_ring, sizeof(double) * 2 * SA_RING));
      h->misc_allocs.push_back(h->sa_ring);
    }
    // iteration 0 reads "the error of iteration -1": open
    std::vector<double> open((size_t)SA_RING, 1e300);
    HIPCHK(h, hipMemcpyAsync(h->sa_ring + SA_RING, open.data(), sizeof(double) * SA_RING, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }

  // `count` iterations starting at global iteration it0 (it0 even whenever count == chunk)
  auto enqueue = [&](long long it0, int count) -> int {
    if (!ring) HIPCHK(h, hipMemsetAsync(h->slots, 0, 8 * (size_t)chunk, h->stream));
    for (int i = 0; i < count; ++i) {
      const long long it = it0 + i;
      int r2 = fused ? small_sa_iteration(h, it, bufs[it & 1], bufs[(it + 1) & 1], h->slots + i, i == 0 ? carry : h->slots + i - 1, o.tol,
                                          ring, i == 0 ? nullptr : h->slots + i - 1)
                     : fusedbig ? big_sa_iteration(h, it, bufs[it & 1], bufs[(it + 1) & 1], h->slots + i, i == 0 ? carry : h->slots + i - 1, o.tol)
                     : apply_T_dev(h, bufs[it & 1], bufs[(it + 1) & 1], h->slots + i, i == 0 ? carry : h->slots + i - 1, o.tol, prec);
      if (r2) return r2;
    }
    if (ring) {
      const int par = (int)((it0 + count - 1) & 1);
      hipLaunchKernelGGL(small_sa_finish, dim3(1), dim3(64), 0, h->stream, (const double*)(h->sa_ring + (size_t)par * SA_RING), ring_n[par], h->slots + count - 1);
      HIPCHK(h, hipGetLastError());
    } else HIPCHK(h, hipMemcpyAsync(carry, h->slots + count - 1, 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->slots_host, h->slots, 8 * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    return 0;
  };
  // hipStreamBeginCapture is illegal on the legacy NULL stream (sdfs_set_stream(h, NULL, 0)): plain launches there
  const bool graph = o.use_graph && !h->profiling && h->stream != nullptr;
  if (graph && (h->sa_graph == nullptr || h->sa_graph_chunk != chunk || h->sa_graph_tol != o.tol)) {
    if ((rc = capture_graph(h, &h->sa_graph, [&] { return enqueue(0, chunk); }))) return rc;
    h->sa_graph_chunk = chunk;
    h->sa_graph_tol = o.tol;
  }

  long long it = 0;            // completed iterations (the reference's current_iter)
  long long buf_it = 0;        // iterations whose result the buffers hold
  double err = o.tol + 1;
  bool stop = false;
  int status = 0;
  while (!stop && it < o.max_iter) {
    const int count = (int)std::min<long long>(chunk, o.max_iter - it);
    if (graph && count == chunk) { HIPCHK(h, hipGraphLaunch(h->sa_graph, h->stream)); }
    else if ((rc = enqueue(it, count))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const long long it0 = it;
    buf_it = it0 + count;                                   // unless the gate closed earlier
    for (int i = 0; i < count; ++i) {
      err = bits_to_double(h->slots_host[i]);
      if (o.record_errors) h->trace.push_back(err);
      it = it0 + i + 1;
      if (!std::isfinite(err)) { stop = true; status = SDFS_ERR_NUMERIC; break; }   // buffers ran on to it0+count
      if (!(err > o.tol)) { stop = true; buf_it = it; break; }                      // later launches were gated off
    }
  }
  HIPCHK(h, hipMemcpyAsync(w, bufs[buf_it & 1], nb, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->last_resid = err;
  *n_iter = it; *n_apply = buf_it; *final_err = err;
  if (status) return fail(h, status, "non-finite error at iteration %lld", it);
  return 0;
}

// ---------------------------------------------------------------------------
// BiCGSTAB on device vectors (jax.scipy.sparse.linalg.bicgstab semantics: x0 = 0,
// stop when |r|^2 <= max(rtol^2 |b|^2, atol^2), breakdown flags, maxiter 10 N).
// b in kry[6]; solution in kry[5].  One host sync per iteration (reads rr).
// T = storage type of the Krylov vectors: double, or float under opts.krylov_f32 (the vectors then
// occupy the first half of the same allocations and the J.v kernels read / write fp32, see run_plan)
// mode = the matvec: MODE_JVP solves (J - I) x = b, MODE_VJP (fp64 only) solves (J^T - I) x = b.  The fused forms below
// (dot products in the last J.v pass, the merged small-grid loop, the slice_jfused updates, the captured graph) are
// J.v-only: the transposed solve runs the plain iteration.  lc1 / lc2 (fp64 MODE_JVP only): the J.v scalings to use in
// place of the cached c1 / c2 (the tilted expectation, sdfs_solve_tilted_dev); they too run the plain iteration.
// prec: the storage of the J.v applications (PREC_F64, or the fp32 Krylov storage T = float / bf16r stands for).
template <typename T>
int bicgstab_dev_t(sdfs_handle* h, const sdfs_opts& o, int64_t* matvecs, int prec, int mode = MODE_JVP,
                   const double* lc1 = nullptr, const double* lc2 = nullptr) {
  const bool vjp = mode == MODE_VJP;
  const bool plain = vjp || lc1 != nullptr;     // only the plain iteration takes explicit scalings
  const bool f32 = prec != PREC_F64;
  T *r = (T*)h->kry[0], *rhat = (T*)h->kry[1], *p = (T*)h->kry[2], *q = (T*)h->kry[3], *t = (T*)h->kry[4],
    *x = (T*)h->kry[5];
  const double* b = h->kry[6];
  const long long n = h->N;
  const int g = vec_grid(n);
  hipStream_t st = h->stream;
  const int cvec = h->profiling ? counter_id(h, "bicgstab_blas1", 0, 0) : -1;
  int rc;
  // gate word: non-zero while the inner solve runs, 0 once converged / broken down (vec_kernels.hpp); an
  // allocation of its own, never moved: its address is baked into the captured iteration graph
  if (!h->bicg_gate) {
    HIPCHK(h, hipMalloc((void**)&h->bicg_gate, 64));
    h->misc_allocs.push_back(h->bicg_gate);
    HIPCHK(h, hipHostMalloc((void**)&h->bicg_gate_host, 64));
  }
  unsigned long long* gate = h->bicg_gate;
  // the J.v application in -> out of an iteration, (J - I) in with the partial sums of its fused dot products in dotp
  auto jv = [&](const T* in, T* out, double* dotp) {
    Apply a(mode, (const double*)in, (double*)out, (const double*)in);
    a.gate = gate; a.minus_identity = 1; a.dotp = dotp; a.prec = prec; a.lc1 = lc1; a.lc2 = lc2;
    return a;
  };
  {
    ProfScope ps(h, cvec);
    hipLaunchKernelGGL(k_bicg_init<T>, dim3(g), dim3(VEC_BLOCK), 0, st, b, r, rhat, p, q, x, n);
    hipLaunchKernelGGL(k_dot<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)r, (const T*)r, n, h->partial, (const unsigned long long*)nullptr);
    hipLaunchKernelGGL(k_bicg_init_finish, dim3(1), dim3(VEC_BLOCK), 0, st, h->partial, g, h->sc, o.inner_rtol, o.inner_atol, gate);
  }
  const long long maxit = o.inner_max_iter > 0 ? o.inner_max_iter : 10 * n;
  // <t, s> and <t, t> come out of the last J.v pass when its tiles fit the partial-sum buffer
  const long long last_tiles = last_pass_grid(h, jv(p, q, h->partial));
  const bool fused_dots = !plain && last_tiles > 0 && 2 * last_tiles <= (long long)MAX_PARTIAL_BLOCKS * AND_MAX_M &&
                          (h->plan[0].passes.size() > 1 || (h->fast.ok && (!f32 || h->fast.f32_ok))) &&
                          prec != PREC_BF16;      // (the fused sums would see the J.v output before its rounding)
  // small grids are launch-bound: the finishing kernels merge into the vector kernels behind them (vec_kernels.hpp),
  // each reduction with its own region of the partial-sum buffer
  constexpr int PR = 2 * MAX_PARTIAL_BLOCKS;
  double* const pdot = h->partial;              // <rhat, q>
  double* const pss = h->partial + PR;          // <s, s>
  double* const pt = h->partial + 2 * PR;       // <t, s>, <t, t>
  double* const prr = h->partial + 4 * PR;      // <r, r>, <rhat, r>
  const bool merged = !plain && n <= (1LL << 22) && (!fused_dots || last_tiles <= MAX_PARTIAL_BLOCKS);
  auto iteration_merged = [&]() -> int {
    int rc2;
    { ProfScope ps(h, cvec);
      hipLaunchKernelGGL(k_bicg_update_p<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)r, p, (const T*)q, n, h->sc, (const unsigned long long*)gate); }
    // small-grid plan, fp64 vectors: <rhat, q> comes out of the last J.v pass as well
    const bool fused_rhat = fused_dots && h->fast.ok && h->fast.small && std::is_same<T, double>::value;
    Apply a = jv(p, q, fused_rhat ? pdot : nullptr);
    if (fused_rhat) a.dot_with = (const double*)rhat;
    if ((rc2 = apply(h, a))) return rc2;
    { ProfScope ps(h, cvec);
      if (!fused_rhat) hipLaunchKernelGGL(k_dot<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)rhat, (const T*)q, n, pdot, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_s_m<T>, dim3(g), dim3(VEC_BLOCK), 0, st, r, (const T*)q, n, h->sc, (const double*)pdot, fused_rhat ? (int)last_tiles : g, pss, (const unsigned long long*)gate); }
    if ((rc2 = apply(h, jv(r, t, fused_dots ? pt : nullptr)))) return rc2;
    { ProfScope ps(h, cvec);
      if (!fused_dots) hipLaunchKernelGGL(k_dot2<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)t, (const T*)r, n, pt, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_update_xr_m<T>, dim3(g), dim3(VEC_BLOCK), 0, st, x, r, (const T*)p, (const T*)t, (const T*)rhat, n, h->sc,
                         (const double*)pss, g, (const double*)pt, fused_dots ? (int)last_tiles : g, prr, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_iter_finish, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)prr, g, h->sc, gate); }
    return 0;
  };
  // one BiCGSTAB iteration, every launch gated on the device flag
  auto iteration_plain = [&]() -> int {
    int rc2;
    { ProfScope ps(h, cvec);
      hipLaunchKernelGGL(k_bicg_update_p<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)r, p, (const T*)q, n, h->sc, (const unsigned long long*)gate); }
    if ((rc2 = apply(h, jv(p, q, nullptr)))) return rc2;
    { ProfScope ps(h, cvec);
      hipLaunchKernelGGL(k_dot<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)rhat, (const T*)q, n, h->partial, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_alpha_finish, dim3(1), dim3(VEC_BLOCK), 0, st, h->partial, g, h->sc, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_s<T>, dim3(g), dim3(VEC_BLOCK), 0, st, r, (const T*)q, n, h->sc, h->partial, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_s_finish, dim3(1), dim3(VEC_BLOCK), 0, st, h->partial, g, h->sc, (const unsigned long long*)gate); }
    if ((rc2 = apply(h, jv(r, t, fused_dots ? h->partial : nullptr)))) return rc2;
    { ProfScope ps(h, cvec);
      if (!fused_dots) hipLaunchKernelGGL(k_dot2<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)t, (const T*)r, n, h->partial, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_omega_finish, dim3(1), dim3(VEC_BLOCK), 0, st, h->partial, fused_dots ? (int)last_tiles : g, h->sc, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_update_xr<T>, dim3(g), dim3(VEC_BLOCK), 0, st, x, r, (const T*)p, (const T*)t, (const T*)rhat, n, h->sc, h->partial, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_iter_finish, dim3(1), dim3(VEC_BLOCK), 0, st, h->partial, g, h->sc, gate); }
    return 0;
  };
  // Large grids on the compile-time pair plan: the p and s updates on the registers of J.v's first pass, <rhat, q> in its
  // last (krylov_kernels.hpp) -- 31 grid streams per iteration instead of 34
  const FastPass* const P0 = (h->fast.ok && !h->fast.passes.empty()) ? &h->fast.passes.front() : nullptr;
  const FastPass* const PL = (h->fast.ok && !h->fast.passes.empty()) ? &h->fast.passes.back() : nullptr;
  // (fp64 storage on the fp64 kernels; fp32 storage on the fp32-MFMA kernels, opts.krylov_f32 = 3)
#ifdef SDFS_NO_JF32      // (build-time probe: the fp32-MFMA loop with the separate BLAS-1 kernels)
  const bool jf32 = false;
#else
  const bool jf32 = std::is_same<T, float>::value && prec == PREC_MFMA32 && h->fast.f32_ok;
#endif
  bool jfuse = !plain && ((std::is_same<T, double>::value && !f32) || jf32) && !merged && h->fast.ok && !h->fast.small && !h->fast.pad &&
               h->fast.passes.size() >= 2 && !P0->line && !P0->pad && PL->line && PL->ld.lrest % LINE_R == 0;
  // the two applications of a fused iteration: q = (J - I) p, p = r + beta (p - omega q) formed in the first pass, <rhat, q>
  // summed by the last; t = (J - I) s, s = r - alpha q (in r) and <s, s> formed in the first pass, <t, s> and <t, t> summed
  // by the last (partial sums dp: [0, nt) <out, in>, [nt, 2 nt) <out, out>, [2 nt, 3 nt) <out, rhat>)
  double* const dp = h->partial;
  Apply jfp = jv(p, q, dp), jfs = jv(r, t, dp);
  jfp.bicg.kind = JF_P; jfp.bicg.upd = (double*)p; jfp.bicg.a = (const double*)r; jfp.bicg.q = (const double*)q;
  jfp.bicg.dot_with = (const double*)rhat;
  jfs.bicg.kind = JF_S; jfs.bicg.upd = (double*)r; jfs.bicg.q = (const double*)q;
  // workgroups of the last pass (one partial sum each per inner product), wave tiles of the first
  const long long jf_last = jfuse ? last_pass_grid(h, jfp) : 0;
  if (3 * jf_last > (long long)MAX_PARTIAL_BLOCKS * AND_MAX_M) jfuse = false;
  long long jf_tiles0 = 0;
  if (jfuse) {
    const int gsl = jf32 ? slice32_tile_slices(P0->n) : slice_tile_slices(P0->n, S_JFIRST);
    jf_tiles0 = (P0->sd.nslices + gsl - 1) / gsl;
    if (h->jf_ss_n < jf_tiles0) {
      double* d = nullptr;
      if (hipMalloc((void**)&d, sizeof(double) * (size_t)jf_tiles0) != hipSuccess) jfuse = false;
      else { h->misc_allocs.push_back(d); h->jf_ss = d; h->jf_ss_n = jf_tiles0; }
    }
    if (jfuse && jf32) {
      if (!slice32_jfused_variant(P0->n, JF_P)) jfuse = false;
      else for (int kd : {(int)JF_P, (int)JF_S})
        hipFuncSetAttribute((const void*)slice32_jfused_variant(P0->n, kd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)slice32_lds_bytes(P0->n));
    } else if (jfuse) {
      hipFuncSetAttribute((const void*)slice_jfused_variant(P0->n, JF_P), hipFuncAttributeMaxDynamicSharedMemorySize, (int)slice_lds_bytes(P0->n, S_JFIRST));
      hipFuncSetAttribute((const void*)slice_jfused_variant(P0->n, JF_S), hipFuncAttributeMaxDynamicSharedMemorySize, (int)slice_lds_bytes(P0->n, S_JFIRST));
      hipFuncSetAttribute((const void*)line_stream_variant(PL->n, L_JLAST), hipFuncAttributeMaxDynamicSharedMemorySize, (int)line_lds_bytes(PL->n));
    }
  }
  jfs.bicg.dot = h->jf_ss;
  auto iteration_jfused = [&]() -> int {
    int rc2;
    const int nt = (int)jf_last;
    if ((rc2 = apply(h, jfp))) return rc2;
    { ProfScope ps(h, cvec);
      hipLaunchKernelGGL(k_bicg_alpha_finish, dim3(1), dim3(1024), 0, st, (const double*)(dp + 2 * (size_t)nt), nt, h->sc, (const unsigned long long*)gate); }
    if ((rc2 = apply(h, jfs))) return rc2;
    { ProfScope ps(h, cvec);
      hipLaunchKernelGGL(k_bicg_s_finish_wide, dim3(1), dim3(1024), 0, st, (const double*)h->jf_ss, (int)jf_tiles0, h->sc, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_omega_finish, dim3(1), dim3(1024), 0, st, (const double*)dp, nt, h->sc, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_update_xr<T>, dim3(g), dim3(VEC_BLOCK), 0, st, x, r, (const T*)p, (const T*)t, (const T*)rhat, n, h->sc, h->partial, (const unsigned long long*)gate);
      hipLaunchKernelGGL(k_bicg_iter_finish, dim3(1), dim3(VEC_BLOCK), 0, st, h->partial, g, h->sc, gate); }
    return 0;
  };
  auto iteration = [&]() -> int { return jfuse ? iteration_jfused() : (merged ? iteration_merged() : iteration_plain()); };
  // Small grids are launch- and sync-bound: the iteration is captured once into a hipGraph (pointers, scalars
  // and the gate are fixed device addresses) and replayed; `chunk` iterations go out per host synchronisation.
  // Large grids (an iteration is milliseconds) keep one iteration per sync so that nothing runs past the
  // breakdown / convergence test for long.
  const int chunk = (int)std::min<long long>(maxit, n <= (1LL << 22) ? 8 : 1);
  const int gslot = std::is_same<T, float>::value ? 1 : 0;
  const bool graph = !plain && o.use_graph && !h->profiling && st != nullptr && chunk > 1 && !std::is_same<T, bf16r>::value;
  if (graph && (h->bicg_graph[gslot] == nullptr || h->bicg_graph_chunk[gslot] != chunk)) {
    // the whole chunk is one graph: one launch per synchronisation
    rc = capture_graph(h, &h->bicg_graph[gslot], [&] {
      int rc2 = 0;
      for (int i = 0; i < chunk && !rc2; ++i) rc2 = iteration();
      return rc2;
    });
    if (rc) return rc;
    h->bicg_graph_chunk[gslot] = chunk;
  }
  long long k = 0;
  for (;;) {
    HIPCHK(h, hipMemcpyAsync(h->sc_host, h->sc, sizeof(double) * SC_COUNT, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(h->bicg_gate_host, gate, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    k = (long long)h->sc_host[SC_ITERS];
    if (h->bicg_gate_host[0] == 0ULL || k >= maxit) break;       // converged, broken down, NaN, or out of iterations
    const int todo = (int)std::min<long long>(chunk, maxit - k);
    if (graph && todo == h->bicg_graph_chunk[gslot]) { HIPCHK(h, hipGraphLaunch(h->bicg_graph[gslot], st)); }
    else for (int i = 0; i < todo; ++i) if ((rc = iteration())) return rc;
    HIPCHK(h, hipGetLastError());
  }
  *matvecs += 2 * k;
  return 0;
}

// Newton on g = T - id (code/solvers.py:51-95): x <- x - J(x)^{-1} g(x), outer loop is
// the successive_approx stopping rule on the Newton map.

int bicgstab_dev(sdfs_handle* h, const sdfs_opts& o, int64_t* matvecs, int prec) {
  if (prec == PREC_BF16) return bicgstab_dev_t<bf16r>(h, o, matvecs, prec);
  return prec != PREC_F64 ? bicgstab_dev_t<float>(h, o, matvecs, prec) : bicgstab_dev_t<double>(h, o, matvecs, prec);
}

int solve_newton(sdfs_handle* h, const sdfs_opts& o, double* w, int64_t* n_iter, int64_t* n_apply, double* final_err) {
  int rc;
  if ((rc = ensure_buf(h, &h->buf0)) || (rc = ensure_buf(h, &h->buf1)) || (rc = ensure_scalars(h)) ||
      (rc = ensure_slots(h, 2)))
    return rc;
  while (h->kry.size() < 7) { double* p = nullptr; if ((rc = dev_alloc(h, &p, (size_t)h->N))) return rc; h->kry.push_back(p); }
  const long long n = h->N;
  const int g = vec_grid(n);
  const size_t nb = sizeof(double) * (size_t)n;
  hipStream_t st = h->stream;
  double* x = h->buf0;
  double* Tx = h->buf1;
  HIPCHK(h, hipMemcpyAsync(x, w, nb, hipMemcpyDeviceToDevice, st));
  h->trace.clear();
  long long it = 0;
  double err = o.tol + 1;
  int64_t applies = 0;
  int status = 0;
  const int cvec = h->profiling ? counter_id(h, "newton_blas1", 0, 0) : -1;
  // opts.krylov_f32: inexact Newton with the inner solve in fp32 storage (Krylov vectors, c1 / c2, the
  // J.v intermediates) and fp64 arithmetic / reductions; the outer residual T(x) - x and the iterate
  // stay fp64, so the fixed point is reached to the same tolerance.  Discretised, unsharded handles only.
  const bool want_f32 = o.krylov_f32 != 0 && !h->cont && !h->dense && !h->sharded;
  const int prec_f32 = (o.krylov_f32 == PREC_BF16 || o.krylov_f32 == PREC_MFMA32) ? o.krylov_f32 : PREC_F32;
  int prec = want_f32 ? prec_f32 : PREC_F64;      // the storage of this step's inner solve
  int f32_failures = 0;
  while (err > o.tol && it < o.max_iter) {
    // g(x) = T(x) - x, linearisation cached for the J.v products
    Apply lin(MODE_T_LIN, x, Tx, x);
    lin.prec = prec;
    if ((rc = apply(h, lin))) return rc;
    ++applies;
    { ProfScope ps(h, cvec);
      hipLaunchKernelGGL(k_sub_dot, dim3(g), dim3(VEC_BLOCK), 0, st, Tx, x, h->kry[6], n, h->partial); }
    if ((rc = bicgstab_dev(h, o, &applies, prec))) return rc;
    const bool f32 = prec != PREC_F64;
    // fp32 storage can overflow while the iterate is still far from the fixed point ((w / w_0)^(theta-1)
    // spans more than fp32's range): keep the iterate so that such a step can be redone in fp64
    if (f32) HIPCHK(h, hipMemcpyAsync(Tx, x, nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemsetAsync(h->slots, 0, 8, st));
    { ProfScope ps(h, cvec);
      if (f32) hipLaunchKernelGGL(k_newton_update<float>, dim3(g), dim3(VEC_BLOCK), 0, st, x, (const float*)h->kry[5], x, n, h->slots);
      else hipLaunchKernelGGL(k_newton_update<double>, dim3(g), dim3(VEC_BLOCK), 0, st, x, (const double*)h->kry[5], x, n, h->slots); }
    HIPCHK(h, hipMemcpyAsync(h->slots_host, h->slots, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    err = bits_to_double(h->slots_host[0]);
    // A BiCGSTAB breakdown (rho, omega or alpha = 0) leaves a zero step, which the stopping rule below -- the
    // reference's, code/solvers.py:36 -- would read as convergence wherever the iterate happens to be (seen with fp32
    // storage at inner_rtol 1e-2: "converged" 352 away from the fixed point).  Such a step did nothing: in reduced
    // storage it is redone in fp64 like an overflowed one; in fp64 the solve ends with a numeric error.  (A zero step
    // because |g|_2 <= inner_atol is the reference's own rule and stays.)
    // (a NaN or infinite right-hand side -- an iterate that left the domain -- closes the solve's gate at once: also a zero step)
    const bool broke = err == 0.0 && (h->sc_host[SC_BREAK] != 0.0 || !std::isfinite(h->sc_host[SC_BB]));
    if (broke && !f32) { status = SDFS_ERR_NUMERIC; ++it; break; }
    if ((!std::isfinite(err) || broke) && f32) {
      HIPCHK(h, hipMemcpyAsync(x, Tx, nb, hipMemcpyDeviceToDevice, st));
      prec = PREC_F64;                       // redo this step in fp64
      ++f32_failures;
      err = o.tol + 1;
      continue;
    }
    // an fp64 step after an overflow went through: the iterate has usually calmed down, try fp32 again
    // (twice at most -- every failed attempt costs one inner solve)
    if (want_f32 && !f32 && f32_failures < 3) prec = prec_f32;
    if (o.record_errors) h->trace.push_back(err);
    ++it;
    if (!std::isfinite(err)) { status = SDFS_ERR_NUMERIC; break; }
  }
  HIPCHK(h, hipMemcpyAsync(w, x, nb, hipMemcpyDeviceToDevice, st));
  HIPCHK(h, hipStreamSynchronize(st));
  *n_iter = it; *n_apply = applies; *final_err = err;
  if (status) return fail(h, status, "non-finite Newton step or BiCGSTAB breakdown with no progress at iteration %lld", it);
  return 0;
}

// ---------------------------------------------------------------------------
// true when the `count` consecutive blocks of `len` doubles are bit for bit the same
bool slices_identical(const double* p, long long count, size_t len) {
  for (long long i = 1; i < count; ++i)
    if (memcmp(p, p + (size_t)i * len, len * sizeof(double)) != 0) return false;
  return true;
}

// What setup_model works out on the host: the transition matrices with the scale tables folded in, and the a3 table
// where it stays a table.  sdfs_create uploads them as they are; sdfs_batch_create packs one set per problem.
struct ModelTables {
  std::vector<double> q[MAXD];   // per axis: qcount matrices of n x n
  std::vector<double> a3;
  bool keep_a3 = false;          // the z tensor is slice-identical: a3 stays a table the aggregator applies
};

// The host half of setup_model: checks, the handle's host fields, and the tables into M.  Touches no device.
int fill_model(sdfs_handle* h, int model, int ndim, const int64_t* shapes, const double* params, int nparams,
               const double* const* arrays, const int64_t* sizes, int narrays, ModelTables& M) {
  h->model = model; h->ndim = ndim;
  long long N = 1;
  for (int a = 0; a < ndim; ++a) {
    if (shapes[a] < 2) return fail(h, SDFS_ERR_ARG, "shapes[%d] = %lld: every axis needs >= 2 states (Rouwenhorst)", a, (long long)shapes[a]);
    if (shapes[a] > MAXN) return fail(h, SDFS_ERR_UNSUPPORTED, "shapes[%d] = %lld > %d unsupported", a, (long long)shapes[a], MAXN);
    h->shape[a] = (int)shapes[a]; N *= shapes[a];
    h->ax[a].n = h->ax[a].nloc = (int)shapes[a]; h->ax[a].off = 0;
  }
  h->N = N;
  auto need = [&](int i, long long cnt, const char* nm) -> int {
    if (!arrays[i]) return fail(h, SDFS_ERR_ARG, "arrays[%d] (%s) is NULL", i, nm);
    if (sizes[i] != cnt) return fail(h, SDFS_ERR_ARG, "arrays[%d] (%s) has %lld elements, expected %lld", i, nm, (long long)sizes[i], cnt);
    return 0;
  };
  int rc;
  std::vector<double> a1, a2;
  std::vector<double>& a3 = M.a3;
  auto& qf = M.q;
  if (model == SDFS_MODEL_SSY) {
    if (ndim != 4 || nparams != 13 || narrays != 10) return fail(h, SDFS_ERR_ARG, "SSY needs ndim 4, 13 params, 10 arrays");
    // params: beta, gamma, psi, mu_c, ...  (ssy_model.py:81)
    const double beta = params[0], gamma = params[1], psi = params[2], mu_c = params[3];
    h->beta = beta; h->theta = (1 - gamma) / (1 - 1 / psi);
    const int nl = h->shape[0], nc = h->shape[1], nz = h->shape[2], nj = h->shape[3];
    if ((rc = need(0, nl, "h_lam_states")) || (rc = need(1, (long long)nl * nl, "h_lam_Q")) ||
        (rc = need(2, nc, "h_c_states")) || (rc = need(3, (long long)nc * nc, "h_c_Q")) ||
        (rc = need(4, nz, "h_z_states")) || (rc = need(5, (long long)nz * nz, "h_z_Q")) ||
        (rc = need(6, (long long)nz * nj, "z_states")) || (rc = need(7, (long long)nz * nj * nj, "z_Q")) ||
        (rc = need(8, nc, "sigma_c_states")) || (rc = need(9, nz, "sigma_z_states")))
      return rc;
    a1.resize(nl); a2.resize(nc); a3.resize((size_t)nz * nj);
    for (int l = 0; l < nl; ++l) a1[l] = std::exp(h->theta * arrays[0][l]);                       // ssy_wc_ratio.py:116
    for (int k = 0; k < nc; ++k) { const double s = (1 - gamma) * arrays[8][k]; a2[k] = std::exp(0.5 * s * s); }   // :120
    for (size_t i = 0; i < a3.size(); ++i) a3[i] = std::exp((1 - gamma) * (mu_c + arrays[6][i])); // :124
    const int qi[4] = {1, 3, 5, 7};
    const char* nm[4] = {"h_lam", "h_c", "h_z", "z"};
    // The scale tables are folded into the transition tensors once, here, so the kernels' pow loops
    // need no lookups:  Ql[l,L]*a1[L] (next state),  a2[k]*Qc[k,K]  and  a3[i,j]*zQ[i,j,J] (current state).
    for (int a = 0; a < 4; ++a) qf[a].assign(arrays[qi[a]], arrays[qi[a]] + sizes[qi[a]]);
    for (int l = 0; l < nl; ++l) for (int L = 0; L < nl; ++L) qf[0][(size_t)l * nl + L] *= a1[L];
    for (int k = 0; k < nc; ++k) for (int K = 0; K < nc; ++K) qf[1][(size_t)k * nc + K] *= a2[k];
    // z_Q[i, :, :] the same matrix for every i (Rouwenhorst / Tauchen: it depends on (n, rho) only)?  Then
    // z is an unconditional axis with one matrix, and a3 stays a table the aggregator applies.
    const bool z_same = slices_identical(qf[3].data(), nz, (size_t)nj * nj) && h->knobs.no_slice_merge == 0;
    if (z_same) qf[3].resize((size_t)nj * nj);
    else for (size_t r = 0; r < a3.size(); ++r) for (int J = 0; J < nj; ++J) qf[3][r * nj + J] *= a3[r];
    for (int a = 0; a < 4; ++a) {
      h->ax[a].qcount = (long long)qf[a].size() / ((long long)h->shape[a] * h->shape[a]);
      strncpy(h->ax[a].name, nm[a], sizeof h->ax[a].name - 1);
    }
    h->sens.ip_beta = 0; h->sens.ip_gamma = 1; h->sens.ip_psi = 2; h->sens.ip_mu_c = 3;
    h->sens.ia_hlam = 0; h->sens.ia_sigc = 8; h->sens.ia_z = 6; h->sens.trans = {1, 3, 5, 7};
    h->sens.ax_a1 = 0; h->sens.ax_a2 = 1; h->sens.a3s[2] = nj; h->sens.a3s[3] = 1;
    if (z_same) {
      M.keep_a3 = true;
      h->ax[2].a3s = nj; h->ax[3].a3s = 1;            // a3[i, j]
    } else {
      h->ax[3].qs[2] = 1;               // z_Q[i, j, J] conditioned on the current h_z index
    }
  } else if (model == SDFS_MODEL_GCY) {
    if (ndim != 6 || nparams != 18 || narrays != 15) return fail(h, SDFS_ERR_ARG, "GCY needs ndim 6, 18 params, 15 arrays");
    // params: beta, psi, gamma, rho_lam, s_lam, mu_c, ...  (gcy_model.py:72-75)
    const double beta = params[0], psi = params[1], gamma = params[2], mu_c = params[5];
    h->beta = beta; h->theta = (1 - gamma) / (1 - 1 / psi);
    const long long na = h->shape[0], nbp = h->shape[1], nc = h->shape[2], nd = h->shape[3], ne = h->shape[4], nf = h->shape[5];
    if ((rc = need(0, nbp * nc * ne * na, "z_states")) || (rc = need(1, nbp * nc * ne * na * na, "z_Q")) ||
        (rc = need(2, ne * nbp, "z_pi_states")) || (rc = need(3, ne * nbp * nbp, "z_pi_Q")) ||
        (rc = need(4, nc, "h_z_states")) || (rc = need(5, nc * nc, "h_z_Q")) || (rc = need(6, nc, "sigma_z_states")) ||
        (rc = need(7, nd, "h_c_states")) || (rc = need(8, nd * nd, "h_c_Q")) || (rc = need(9, nd, "sigma_c_states")) ||
        (rc = need(10, ne, "h_zpi_states")) || (rc = need(11, ne * ne, "h_zpi_Q")) || (rc = need(12, ne, "sigma_zpi_states")) ||
        (rc = need(13, nf, "h_lam_states")) || (rc = need(14, nf * nf, "h_lam_Q")))
      return rc;
    a1.resize(nf); a2.resize(nd); a3.resize((size_t)(nbp * nc * ne * na));
    for (int f = 0; f < nf; ++f) a1[f] = std::exp(h->theta * arrays[13][f]);                        // gcy_wc_ratio.py:178
    for (int d = 0; d < nd; ++d) { const double s = (1 - gamma) * arrays[9][d]; a2[d] = std::exp(0.5 * s * s); }   // :182
    for (size_t i = 0; i < a3.size(); ++i) a3[i] = std::exp((1 - gamma) * (mu_c + arrays[0][i]));   // :186, layout [b,c,e,a]
    const int qi[6] = {1, 3, 5, 8, 11, 14};
    const char* nm[6] = {"z", "z_pi", "h_z", "h_c", "h_zpi", "h_lam"};
    // scale tables folded into the transition tensors (see SSY above):
    // Qhl[f,F]*a1[F],  a2[d]*Qhc[d,D],  a3[b,c,e,a]*zQ[b,c,e,a,A]
    for (int a = 0; a < 6; ++a) qf[a].assign(arrays[qi[a]], arrays[qi[a]] + sizes[qi[a]]);
    for (int f = 0; f < nf; ++f) for (int F = 0; F < nf; ++F) qf[5][(size_t)f * nf + F] *= a1[F];
    for (int d = 0; d < nd; ++d) for (int D = 0; D < nd; ++D) qf[3][(size_t)d * nd + D] *= a2[d];
    // slice-identical conditional tensors become unconditional axes (see SSY above)
    const bool merge = h->knobs.no_slice_merge == 0;
    const bool z_same = merge && slices_identical(qf[0].data(), nbp * nc * ne, (size_t)(na * na));
    const bool zpi_same = merge && slices_identical(qf[1].data(), ne, (size_t)(nbp * nbp));
    if (z_same) qf[0].resize((size_t)(na * na));
    else for (size_t r = 0; r < a3.size(); ++r) for (int A = 0; A < na; ++A) qf[0][r * na + A] *= a3[r];
    if (zpi_same) qf[1].resize((size_t)(nbp * nbp));
    for (int a = 0; a < 6; ++a) {
      h->ax[a].qcount = (long long)qf[a].size() / ((long long)h->shape[a] * h->shape[a]);
      strncpy(h->ax[a].name, nm[a], sizeof h->ax[a].name - 1);
    }
    h->sens.ip_beta = 0; h->sens.ip_gamma = 2; h->sens.ip_psi = 1; h->sens.ip_mu_c = 5;
    h->sens.ia_hlam = 13; h->sens.ia_sigc = 9; h->sens.ia_z = 0; h->sens.trans = {1, 3, 5, 8, 11, 14};
    h->sens.ax_a1 = 5; h->sens.ax_a2 = 3;
    h->sens.a3s[0] = 1; h->sens.a3s[4] = (int)na; h->sens.a3s[2] = (int)(ne * na); h->sens.a3s[1] = (int)(nc * ne * na);
    if (z_same) {
      M.keep_a3 = true;
      h->ax[0].a3s = 1; h->ax[4].a3s = (int)na; h->ax[2].a3s = (int)(ne * na); h->ax[1].a3s = (int)(nc * ne * na);  // a3[b,c,e,a]
    } else {
      // z_Q[b, c, e, a, A]: conditioned on current (z_pi, h_z, h_zpi)
      h->ax[0].qs[1] = (int)(nc * ne); h->ax[0].qs[2] = (int)ne; h->ax[0].qs[4] = 1;
    }
    // z_pi_Q[e, b, B]: conditioned on current h_zpi
    if (!zpi_same) h->ax[1].qs[4] = 1;
  } else {
    return fail(h, SDFS_ERR_ARG, "unknown model %d", model);
  }
  if (!(h->theta == h->theta) || h->theta == 0.0 || !std::isfinite(h->theta))
    return fail(h, SDFS_ERR_ARG, "theta = (1-gamma)/(1-1/psi) is not finite / zero");
  {
    auto& S = h->sens;
    S.gamma = params[S.ip_gamma]; S.psi = params[S.ip_psi]; S.mu_c = params[S.ip_mu_c];
    S.sizes.assign(sizes, sizes + narrays);
    S.hlam.assign(arrays[S.ia_hlam], arrays[S.ia_hlam] + sizes[S.ia_hlam]);
    S.sigc.assign(arrays[S.ia_sigc], arrays[S.ia_sigc] + sizes[S.ia_sigc]);
    S.z.assign(arrays[S.ia_z], arrays[S.ia_z] + sizes[S.ia_z]);
  }
  return 0;
}

int setup_model(sdfs_handle* h, int model, int ndim, const int64_t* shapes, const double* params, int nparams,
                const double* const* arrays, const int64_t* sizes, int narrays) {
  ModelTables M;
  int rc = fill_model(h, model, ndim, shapes, params, nparams, arrays, sizes, narrays, M);
  if (rc) return rc;
  for (int a = 0; a < ndim; ++a) {
    double* q = nullptr;
    if ((rc = upload(h, &q, M.q[a].data(), M.q[a].size()))) return rc;
    h->ax[a].Q = q;
  }
  if (M.keep_a3) {
    if ((rc = upload(h, &h->a3, M.a3.data(), M.a3.size()))) return rc;
    h->a3_host = M.a3;
  }
  return 0;
}

// Log-tangents of the scale tables setup_model builds, along one direction (dparams, darrays) of (params, arrays):
//   theta = (1 - gamma) / (1 - 1/psi),  a1 = exp(theta h_lam),  a2 = exp((1/2) ((1 - gamma) sigma_c)^2),
//   a3 = exp((1 - gamma) (mu_c + z)),
// so  dln a1 = dtheta h_lam + theta dh_lam,  dln a2 = (1 - gamma) sigma_c ((1 - gamma) dsigma_c - dgamma sigma_c),
//     dln a3 = (1 - gamma) (dmu_c + dz) - dgamma (mu_c + z).
// dln a3 lands in h->sens.dla3_host.  A non-zero tangent of a transition array is SDFS_ERR_UNSUPPORTED: a moving matrix
// is stated as a left generator instead (sdfs_param_tangent_gen_dev).  *need_jv: the J.v term is present (dtheta or dln a1 non-zero).
int sens_tables(sdfs_handle* h, const double* dparams, const double* const* darrays, double* dtheta, double* dbeta,
                SensTab& dla1, SensTab& dla2, bool* need_jv, bool* any_a3) {
  auto& S = h->sens;
  auto darr = [&](int i) -> const double* { return darrays ? darrays[i] : nullptr; };
  for (int i : S.trans) {
    const double* d = darr(i);
    if (!d) continue;
    for (long long k = 0; k < S.sizes[i]; ++k)
      if (d[k] != 0.0) return fail(h, SDFS_ERR_UNSUPPORTED, "arrays[%d] is a transition array: its tangent must be zero "
                                   "(a persistence parameter states dQ = G Q through sdfs_param_tangent_gen_dev)", i);
  }
  const double g = S.gamma, psi = S.psi, th = h->theta;
  const double dg = dparams[S.ip_gamma], dpsi = dparams[S.ip_psi], dmu = dparams[S.ip_mu_c];
  // dtheta/dgamma = -1 / (1 - 1/psi),  dtheta/dpsi = -theta / (psi (psi - 1))
  *dtheta = -dg / (1.0 - 1.0 / psi) - dpsi * th / (psi * (psi - 1.0));
  *dbeta = dparams[S.ip_beta];
  const double* dhl = darr(S.ia_hlam);
  const double* dsc = darr(S.ia_sigc);
  const double* dz = darr(S.ia_z);
  bool a1nz = false;
  for (int i = 0; i < SENS_MAXN; ++i) { dla1.t[i] = 0.0; dla2.t[i] = 0.0; }
  for (size_t l = 0; l < S.hlam.size(); ++l) {
    dla1.t[l] = *dtheta * S.hlam[l] + (dhl ? th * dhl[l] : 0.0);
    a1nz |= dla1.t[l] != 0.0;
  }
  for (size_t k = 0; k < S.sigc.size(); ++k)
    dla2.t[k] = (1.0 - g) * S.sigc[k] * ((1.0 - g) * (dsc ? dsc[k] : 0.0) - dg * S.sigc[k]);
  *any_a3 = dg != 0.0 || dmu != 0.0;
  if (dz) for (size_t i = 0; i < S.z.size() && !*any_a3; ++i) *any_a3 = dz[i] != 0.0;
  if (*any_a3) {
    S.dla3_host.resize(S.z.size());
    for (size_t i = 0; i < S.z.size(); ++i)
      S.dla3_host[i] = (1.0 - g) * (dmu + (dz ? dz[i] : 0.0)) - dg * (S.mu_c + S.z[i]);
  }
  *need_jv = *dtheta != 0.0 || a1nz;
  return 0;
}

int create_common(int model, int ndim, const int64_t* shapes, const double* params, int nparams,
                  const double* const* arrays, const int64_t* sizes, int narrays, int device_id,
                  int axis_a, int64_t a_lo, int64_t a_len, int axis_b, int64_t b_lo, int64_t b_len,
                  sdfs_handle** out) {
  if (!out) return fail(nullptr, SDFS_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (!shapes || !params || !arrays || !sizes) return fail(nullptr, SDFS_ERR_ARG, "NULL argument");
  if (ndim < 1 || ndim > MAXD) return fail(nullptr, SDFS_ERR_ARG, "ndim %d out of range", ndim);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, SDFS_ERR_HIP, "no HIP device available (libsdfs_hip has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, SDFS_ERR_ARG, "device_id %d out of range (%d devices)", device_id, ndev);
  sdfs_handle* h = new sdfs_handle();
  h->knobs = read_knobs();
  memset(&h->counters, 0, sizeof h->counters);
  h->device = device_id;
  auto bail = [&](int rc) { g_create_error = h->err; sdfs_destroy(h); return rc; };
  if (hipSetDevice(device_id) != hipSuccess) return bail(fail(h, SDFS_ERR_HIP, "hipSetDevice(%d) failed", device_id));
  if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(h, SDFS_ERR_HIP, "hipStreamCreate failed"));
  h->stream = h->own_stream;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) h->num_cus = prop.multiProcessorCount;
  }
  int rc = setup_model(h, model, ndim, shapes, params, nparams, arrays, sizes, narrays);
  if (rc) return bail(rc);
  for (int a = 0; a < ndim; ++a) {                       // transposed copies of the unconditional matrices (VJP)
    if (h->ax[a].qcount != 1) continue;
    const int n = h->ax[a].n;
    std::vector<double> q((size_t)n * n), qt((size_t)n * n);
    if (hipMemcpy(q.data(), h->ax[a].Q, q.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
      return bail(fail(h, SDFS_ERR_HIP, "read-back of a transition matrix failed"));
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) qt[(size_t)j * n + i] = q[(size_t)i * n + j];
    double* d = nullptr;
    if ((rc = upload(h, &d, qt.data(), qt.size()))) return bail(rc);
    h->ax[a].Qt = d;
    if (n <= 16) {
      std::vector<double> qp(256, 0.0), qtp(256, 0.0);
      for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { qp[(size_t)i * 16 + j] = q[(size_t)i * n + j]; qtp[(size_t)j * 16 + i] = q[(size_t)i * n + j]; }
      double *dp = nullptr, *dtp = nullptr;
      if ((rc = upload(h, &dp, qp.data(), 256)) || (rc = upload(h, &dtp, qtp.data(), 256))) return bail(rc);
      h->ax[a].Qp = dp; h->ax[a].Qtp = dtp;
    }
    for (int c = 0; c < 4; ++c) {
      const int nt = c == 0 ? 16 : (c == 1 ? 20 : (c == 2 ? 24 : 32));
      if (n > nt) continue;
      if (c == 0) { h->ax[a].Qpad[0] = h->ax[a].Qp; h->ax[a].Qtpad[0] = h->ax[a].Qtp; continue; }
      std::vector<double> qp((size_t)nt * nt, 0.0), qtp((size_t)nt * nt, 0.0);
      for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { qp[(size_t)i * nt + j] = q[(size_t)i * n + j]; qtp[(size_t)j * nt + i] = q[(size_t)i * n + j]; }
      double *dp = nullptr, *dtp = nullptr;
      if ((rc = upload(h, &dp, qp.data(), qp.size())) || (rc = upload(h, &dtp, qtp.data(), qtp.size()))) return bail(rc);
      h->ax[a].Qpad[c] = dp; h->ax[a].Qtpad[c] = dtp;
    }
  }
  // dynamic LDS above 64 KB has to be allowed per kernel variant (and per device)
  static unsigned long long attr_done = 0;
  if (device_id < 64 && !(attr_done & (1ULL << device_id))) {
    for (int e = 1; e <= 16; e <<= 1)
      for (int v = 1; v <= 2; ++v)
        for (int j = 0; j < M_NMODES; ++j)
          for (int pr = 0; pr < 2; ++pr) {
            if (v == 2 && pr == 1) {
              pass_fn f4 = pass_kernel_variant(e, 4, j, 1);
              if (f4) hipFuncSetAttribute((const void*)f4, hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
            }
            pass_fn fn = pass_kernel_variant(e, v, j, pr);
            if (fn) hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
          }
    attr_done |= 1ULL << device_id;
  }
  std::vector<int> all;
  for (int a = 0; a < ndim; ++a) all.push_back(a);
  if (axis_a < 0) {
    rc = build_plan(h, h->plan[0], all, std::vector<bool>(ndim, false));
    if (rc) return bail(rc);
    rc = build_fast_plan(h);
    if (rc) return bail(rc);
    rc = build_small_plan(h);
    if (rc) return bail(rc);
    rc = build_pad_plan(h);
    if (rc) return bail(rc);
  } else {
    if (axis_a >= ndim || axis_b < 0 || axis_b >= ndim || axis_a == axis_b)
      return bail(fail(h, SDFS_ERR_ARG, "bad shard axes %d / %d", axis_a, axis_b));
    // no transition tensor may be conditioned on A or B, and A's own tensor (contracted in stage 1,
    // where only B is incomplete) must not be conditioned on B
    for (int g = 0; g < ndim; ++g)
      if (h->ax[g].qs[axis_a] != 0 || h->ax[g].qs[axis_b] != 0)
        return bail(fail(h, SDFS_ERR_ARG, "shard axes must not condition any transition matrix"));
    for (int c = 0; c < ndim; ++c)
      if (h->ax[axis_b].qs[c] != 0) return bail(fail(h, SDFS_ERR_ARG, "shard axis B must be unconditional"));
    if (a_lo < 0 || a_len < 1 || a_lo + a_len > h->shape[axis_a] || b_lo < 0 || b_len < 1 || b_lo + b_len > h->shape[axis_b])
      return bail(fail(h, SDFS_ERR_ARG, "shard block out of range"));
    h->sharded = true; h->axis_a = axis_a; h->axis_b = axis_b;
    // stage 0: input sharded on A; contract everything but A
    h->ax[axis_a].nloc = (int)a_len; h->ax[axis_a].off = (int)a_lo;
    std::vector<int> s0;
    for (int a = 0; a < ndim; ++a) if (a != axis_a) s0.push_back(a);
    rc = build_plan(h, h->plan[0], s0, std::vector<bool>(ndim, false));
    if (rc) return bail(rc);
    // stage 1: data re-sharded on B; contract A
    h->ax[axis_a].nloc = h->ax[axis_a].n; h->ax[axis_a].off = 0;
    h->ax[axis_b].nloc = (int)b_len; h->ax[axis_b].off = (int)b_lo;
    std::vector<bool> done(ndim, true); done[axis_a] = false;
    rc = build_plan(h, h->plan[1], std::vector<int>{axis_a}, done);
    h->ax[axis_b].nloc = h->ax[axis_b].n; h->ax[axis_b].off = 0;
    if (rc) return bail(rc);
    rc = build_stage_fast_plans(h, (int)a_lo, (int)a_len, (int)b_lo, (int)b_len);
    if (rc) return bail(rc);
  }
  *out = h;
  return 0;
}

int check(sdfs_handle* h) {
  if (!h) return SDFS_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return fail(h, SDFS_ERR_HIP, "hipSetDevice failed");
  return 0;
}

}  // namespace

namespace {
template <typename T>
int krylov_step_t(sdfs_handle* h, int step, long long n, void* const* v, double* sums, double rtol, double atol) {
  const double* b = (const double*)v[0];
  T *r = (T*)v[1], *rhat = (T*)v[2], *p = (T*)v[3], *q = (T*)v[4], *t = (T*)v[5], *x = (T*)v[6];
  const int g = vec_grid(n);
  hipStream_t st = h->stream;
  // SDFS_KS_GATED: every kernel of the step returns at once while the handle's gate word is closed (INIT_FIN opens it
  // when there is something to solve, ITER_FIN closes it on convergence, breakdown or a non-finite |r|^2), so the caller
  // can enqueue several iterations per read of the scalar block; INIT and INIT_FIN themselves always run
  const bool gated = (step & SDFS_KS_GATED) != 0;
  step &= ~SDFS_KS_GATED;
  const unsigned long long* nog = (gated && step != SDFS_KS_INIT) ? h->bicg_gate : nullptr;
  unsigned long long* const wgate = gated ? h->bicg_gate : nullptr;
  switch (step) {
    case SDFS_KS_INIT:
      hipLaunchKernelGGL(k_bicg_init<T>, dim3(g), dim3(VEC_BLOCK), 0, st, b, r, rhat, p, q, x, n);
      hipLaunchKernelGGL(k_dot<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)r, (const T*)r, n, h->partial, nog);
      hipLaunchKernelGGL(k_presum, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)h->partial, g, 1, sums, nog);
      break;
    case SDFS_KS_INIT_FIN:
      hipLaunchKernelGGL(k_bicg_init_finish, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)sums, 0, h->sc, rtol, atol, wgate);
      break;
    case SDFS_KS_UPDATE_P:
      hipLaunchKernelGGL(k_bicg_update_p<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)r, p, (const T*)q, n, h->sc, nog);
      break;
    case SDFS_KS_DOT_RQ:
      hipLaunchKernelGGL(k_dot<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)rhat, (const T*)q, n, h->partial, nog);
      hipLaunchKernelGGL(k_presum, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)h->partial, g, 1, sums, nog);
      break;
    case SDFS_KS_ALPHA_S:
      hipLaunchKernelGGL(k_bicg_alpha_finish, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)sums, 0, h->sc, nog);
      hipLaunchKernelGGL(k_bicg_s<T>, dim3(g), dim3(VEC_BLOCK), 0, st, r, (const T*)q, n, h->sc, h->partial, nog);
      hipLaunchKernelGGL(k_presum, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)h->partial, g, 1, sums, nog);
      break;
    case SDFS_KS_S_FIN:
      hipLaunchKernelGGL(k_bicg_s_finish, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)sums, 0, h->sc, nog);
      break;
    case SDFS_KS_DOT_TS:
      hipLaunchKernelGGL(k_dot2<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const T*)t, (const T*)r, n, h->partial, nog);
      hipLaunchKernelGGL(k_presum, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)h->partial, g, 2, sums, nog);
      break;
    case SDFS_KS_OMEGA_XR:
      hipLaunchKernelGGL(k_bicg_omega_finish, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)sums, 0, h->sc, nog);
      hipLaunchKernelGGL(k_bicg_update_xr<T>, dim3(g), dim3(VEC_BLOCK), 0, st, x, r, (const T*)p, (const T*)t, (const T*)rhat, n, h->sc, h->partial, nog);
      hipLaunchKernelGGL(k_presum, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)h->partial, g, 2, sums, nog);
      break;
    case SDFS_KS_ITER_FIN:
      hipLaunchKernelGGL(k_bicg_iter_finish, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)sums, 0, h->sc, wgate);
      break;
    case SDFS_KS_SUB_DOT:        // v[0] = out g (fp64), v[1] = a, v[2] = b (fp64): g = a - b, sums[0] = <g, g> (local)
      hipLaunchKernelGGL(k_sub_dot, dim3(g), dim3(VEC_BLOCK), 0, st, (const double*)v[1], (const double*)v[2], (double*)v[0], n, h->partial);
      hipLaunchKernelGGL(k_presum, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)h->partial, g, 1, sums, nog);
      break;
    case SDFS_KS_NEWTON_UPDATE:  // v[0] = x (fp64, in place), v[6] = step (T); sums[0] = max|step| of this rank (NaN -> inf)
      HIPCHK(h, hipMemsetAsync(sums, 0, 8, st));
      hipLaunchKernelGGL(k_newton_update<T>, dim3(g), dim3(VEC_BLOCK), 0, st, (const double*)v[0], (const T*)x, (double*)v[0], n, (unsigned long long*)sums);
      break;
    default:
      return fail(h, SDFS_ERR_ARG, "unknown Krylov step %d", step);
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

// workgroups of a grid-stride pass over n points: one per `block` points, at most 16 per CU
int stream_grid(const sdfs_handle* h, long long n, int block) {
  return (int)std::min<long long>((n + block - 1) / block, (long long)h->num_cus * 16);
}
}  // namespace

#include "anderson_host.hpp"   // Anderson acceleration: its loops (solve_anderson) and step API (sdfs_anderson_*), built on the definitions above

// ===========================================================================
extern "C" {

int sdfs_create(int model, int ndim, const int64_t* shapes, const double* params, int nparams,
                const double* const* arrays, const int64_t* array_sizes, int narrays, int device_id,
                sdfs_handle** out) {
  return create_common(model, ndim, shapes, params, nparams, arrays, array_sizes, narrays, device_id,
                       -1, 0, 0, -1, 0, 0, out);
}

int sdfs_create_sharded(int model, int ndim, const int64_t* shapes, const double* params, int nparams,
                        const double* const* arrays, const int64_t* array_sizes, int narrays, int device_id,
                        int axis_a, int64_t a_lo, int64_t a_len, int axis_b, int64_t b_lo, int64_t b_len,
                        sdfs_handle** out) {
  if (axis_a < 0) return fail(nullptr, SDFS_ERR_ARG, "axis_a must be >= 0");
  return create_common(model, ndim, shapes, params, nparams, arrays, array_sizes, narrays, device_id,
                       axis_a, a_lo, a_len, axis_b, b_lo, b_len, out);
}

// Fills the model-specific parts of a ContDesc (the reference's next_state / const term) and the
// grid geometry.  Shared by sdfs_create_continuous and sdfs_lin_interp.
static int cont_geometry(sdfs_handle* h, ContDesc& cd, int ndim, const int64_t* shapes, const double* const* grids) {
  memset(&cd, 0, sizeof cd);
  cd.D = ndim; cd.N = 1;
  for (int d = ndim - 1; d >= 0; --d) {
    if (shapes[d] < 2 || shapes[d] > (1 << 20)) return fail(h, SDFS_ERR_ARG, "grid %d needs 2 <= size, got %lld", d, (long long)shapes[d]);
    if (!grids[d]) return fail(h, SDFS_ERR_ARG, "grids[%d] is NULL", d);
    cd.n[d] = (int)shapes[d]; cd.stride[d] = cd.N; cd.N *= shapes[d];
    const double step = grids[d][1] - grids[d][0];                  // utils.py:11 (uniform grids)
    if (!(step > 0.0) || !std::isfinite(step)) return fail(h, SDFS_ERR_ARG, "grid %d is not increasing", d);
    cd.lo[d] = grids[d][0]; cd.inv_step[d] = 1.0 / step;
    cd.xdim[d] = -1; cd.voldim[d] = -1;
  }
  if (cd.N >= (1LL << 31)) return fail(h, SDFS_ERR_UNSUPPORTED, "more than 2^31 grid points");
  return 0;
}

int sdfs_create_continuous(int model, int ndim, const int64_t* shapes, const double* params, int nparams,
                           const double* const* grids, const double* nodes, const double* weights, int64_t M,
                           int device_id, sdfs_handle** out) {
  if (!out) return fail(nullptr, SDFS_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (!shapes || !params || !grids || !nodes) return fail(nullptr, SDFS_ERR_ARG, "NULL argument");
  if (M < 1 || M > (1 << 24)) return fail(nullptr, SDFS_ERR_ARG, "M = %lld nodes out of range", (long long)M);
  if (model == SDFS_MODEL_SSY ? (ndim != 4 || nparams != 13) : (model == SDFS_MODEL_GCY ? (ndim != 6 || nparams != 18) : true))
    return fail(nullptr, SDFS_ERR_ARG, "continuous SSY needs 4 grids / 13 params, GCY 6 grids / 18 params");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, SDFS_ERR_HIP, "no HIP device available (libsdfs_hip has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, SDFS_ERR_ARG, "device_id %d out of range (%d devices)", device_id, ndev);
  sdfs_handle* h = new sdfs_handle();
  h->knobs = read_knobs();
  memset(&h->counters, 0, sizeof h->counters);
  h->device = device_id;
  auto bail = [&](int rc) { g_create_error = h->err; sdfs_destroy(h); return rc; };
  if (hipSetDevice(device_id) != hipSuccess) return bail(fail(h, SDFS_ERR_HIP, "hipSetDevice(%d) failed", device_id));
  if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(h, SDFS_ERR_HIP, "hipStreamCreate failed"));
  h->stream = h->own_stream;
  ContDesc& cd = h->cd;
  int rc = cont_geometry(h, cd, ndim, shapes, grids);
  if (rc) return bail(rc);
  h->cont = true; h->model = model; h->ndim = ndim; h->N = cd.N;
  for (int d = 0; d < ndim; ++d) h->shape[d] = cd.n[d];
  h->plan[0].nloc = cd.N; h->plan[1].nloc = 0;
  cd.M = (int)M;
  double s0;
  if (model == SDFS_MODEL_SSY) {
    // params: beta, gamma, psi, mu_c, rho, phi_z, phi_c, rho_z, rho_c, rho_lam, s_z, s_c, s_lam (ssy_model.py:81)
    // dims  : h_lam, h_c, h_z, z  (ssy_wc_ratio_continuous.py:66-87)
    const double* q = params;
    h->beta = q[0]; h->theta = (1 - q[1]) / (1 - 1 / q[2]);
    cd.one_m_gamma = 1 - q[1]; cd.mu_c = q[3]; cd.phi_c = q[6]; h->cont_gamma = q[1]; h->cont_psi = q[2];
    cd.rho[0] = q[9]; cd.sconst[0] = q[12];
    cd.rho[1] = q[8]; cd.sconst[1] = q[11];
    cd.rho[2] = q[7]; cd.sconst[2] = q[10];
    cd.rho[3] = q[4]; cd.voldim[3] = 2; cd.phi[3] = q[5];
    cd.zdim = 3; cd.hcdim = 1;
    s0 = q[12];
  } else {
    // params: beta, psi, gamma, rho_lam, s_lam, mu_c, phi_c, rho, rho_pi, phi_z, rho_c, s_c, rho_z, s_z,
    //         rho_pipi, phi_zpi, rho_zpi, s_zpi (gcy_model.py:72-75)
    // dims  : h_lam, h_c, h_z, h_zpi, z, z_pi  (gcy_wc_ratio_continuous.py:78-116)
    const double* q = params;
    h->beta = q[0]; h->theta = (1 - q[2]) / (1 - 1 / q[1]);
    cd.one_m_gamma = 1 - q[2]; cd.mu_c = q[5]; cd.phi_c = q[6]; h->cont_gamma = q[2]; h->cont_psi = q[1];
    cd.rho[0] = q[3]; cd.sconst[0] = q[4];
    cd.rho[1] = q[10]; cd.sconst[1] = q[11];
    cd.rho[2] = q[12]; cd.sconst[2] = q[13];
    cd.rho[3] = q[16]; cd.sconst[3] = q[17];
    cd.rho[4] = q[7]; cd.xdim[4] = 5; cd.xcoef[4] = q[8]; cd.voldim[4] = 2; cd.phi[4] = q[9];
    cd.rho[5] = q[14]; cd.voldim[5] = 3; cd.phi[5] = q[15];
    cd.zdim = 4; cd.hcdim = 1;
    s0 = q[4];
  }
  if (!(h->theta == h->theta) || h->theta == 0.0 || !std::isfinite(h->theta))
    return bail(fail(h, SDFS_ERR_ARG, "theta = (1-gamma)/(1-1/psi) is not finite / zero"));
  cd.theta = h->theta; cd.inv_theta = 1.0 / h->theta; cd.beta = h->beta; cd.theta_rho0 = h->theta * cd.rho[0];
  for (int d = 0; d < ndim; ++d) {
    double* g = nullptr;
    if ((rc = upload(h, &g, grids[d], (size_t)shapes[d]))) return bail(rc);
    cd.grid[d] = g;
  }
  // pf = exp(theta * h_lam') = exp(theta rho_lam h_lam) * exp(theta s_lam eta_0): the node part joins the weight
  std::vector<double> wq((size_t)M);
  for (int64_t m = 0; m < M; ++m)
    wq[(size_t)m] = (weights ? weights[m] : 1.0 / (double)M) * std::exp(h->theta * s0 * nodes[m]);
  double *eta = nullptr, *wqd = nullptr;
  if ((rc = upload(h, &eta, nodes, (size_t)M * ndim)) || (rc = upload(h, &wqd, wq.data(), (size_t)M))) return bail(rc);
  cd.eta = eta; cd.wq = wqd;
  h->ctilt.weight.resize((size_t)M);         // the raw weights and eta_0: what a tilt forms its node weights from
  for (int64_t m = 0; m < M; ++m) h->ctilt.weight[(size_t)m] = weights ? weights[m] : 1.0 / (double)M;
  h->ctilt.eta0.assign(nodes, nodes + M);
  for (int d = 0; d < ndim; ++d) {
    double mx = 0.0;
    for (int64_t m = 0; m < M; ++m) mx = std::max(mx, std::fabs(nodes[(size_t)d * M + m]));
    cd.etamax[d] = mx;
  }
  // Gauss-Hermite tensor rule?  M = tq^D and node m = (j_0 .. j_{D-1}) (j_0 fastest) with
  // eta[d][m] = xi_d[j_d]: checked value by value, Monte-Carlo draws fail the test and keep tq = 0.
  int tq = 0;
  for (int c = 2; c <= 64 && tq == 0; ++c) {
    long long pw = 1;
    for (int d = 0; d < ndim; ++d) pw *= c;
    if (pw == M) tq = c;
  }
  if (tq) {
    long long st = 1;
    for (int d = 0; d < ndim && tq; ++d, st *= tq) {
      cd.tstride[d] = (int)st;
      for (int64_t m = 0; m < M; ++m)
        if (nodes[(size_t)d * M + m] != nodes[(size_t)d * M + ((m / st) % tq) * st]) { tq = 0; break; }
    }
  } else tq = 0;
  // LDS need: the largest box any grid point can ask for, dimension by dimension (same formulas as
  // the kernel; the kernel re-checks its own box against these caps and falls back if it is larger)
  long long vmax = 1, uomax = 1;
  for (int d = 0; d < ndim; ++d) {
    int mext = 2;
    const int nx = cd.xdim[d] >= 0 ? cd.n[cd.xdim[d]] : 1, nv = cd.voldim[d] >= 0 ? cd.n[cd.voldim[d]] : 1;
    for (int i = 0; i < cd.n[d]; ++i)
      for (int ix = 0; ix < nx; ++ix)
        for (int iv = 0; iv < nv; ++iv) {
          const double mean = cd.rho[d] * grids[d][i] + (cd.xdim[d] >= 0 ? cd.xcoef[d] * grids[cd.xdim[d]][ix] : 0.0);
          const double vol = cd.voldim[d] >= 0 ? cd.phi[d] * std::exp(grids[cd.voldim[d]][iv]) : cd.sconst[d];
          const double a = (mean - cd.lo[d]) * cd.inv_step[d], span = std::fabs(vol * cd.inv_step[d]) * cd.etamax[d];
          const double hi = (double)(cd.n[d] - 1);
          const double cmin = std::min(std::max(a - span, 0.0), hi), cmax = std::min(std::max(a + span, 0.0), hi);
          const int blo = std::min((int)cmin, cd.n[d] - 2);
          const int bhi = std::max(blo + 1, std::min((int)cmax + 1, cd.n[d] - 1));
          mext = std::max(mext, bhi - blo + 1);
        }
    vmax *= mext;
    if (d < ndim - 2) uomax *= mext;
  }
  const int cap_limit = 4000;   // doubles; 2 * cap * 8 < 64 KB
  cd.cap = (int)std::min<long long>(vmax, cap_limit);
  cd.cap += cd.cap & 1;
  cd.tq = 0; cd.ucap = 0;
  if (tq && vmax <= cap_limit && uomax * tq * tq + cd.cap <= 4000) {
    cd.tq = tq; cd.ucap = (int)(uomax * tq * tq);
    cd.tmagic = (unsigned)((1ULL << 32) / (unsigned)tq + 1);
    cd.tmagic2 = (unsigned)((1ULL << 32) / (unsigned)(tq * tq) + 1);
  }
  *out = h;
  return 0;
}

int sdfs_create_dense(int64_t N, const double* H, double beta, double theta, int device_id, sdfs_handle** out) {
  if (!out) return fail(nullptr, SDFS_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (!H) return fail(nullptr, SDFS_ERR_ARG, "H is NULL");
  if (N < 1 || N > 46340) return fail(nullptr, SDFS_ERR_ARG, "N = %lld out of range (1 .. 46340)", (long long)N);
  if (!(theta == theta) || theta == 0.0 || !std::isfinite(theta) || !std::isfinite(beta))
    return fail(nullptr, SDFS_ERR_ARG, "beta / theta must be finite, theta non-zero");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, SDFS_ERR_HIP, "no HIP device available (libsdfs_hip has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, SDFS_ERR_ARG, "device_id %d out of range (%d devices)", device_id, ndev);
  sdfs_handle* h = new sdfs_handle();
  h->knobs = read_knobs();
  memset(&h->counters, 0, sizeof h->counters);
  h->device = device_id;
  auto bail = [&](int rc) { g_create_error = h->err; sdfs_destroy(h); return rc; };
  if (hipSetDevice(device_id) != hipSuccess) return bail(fail(h, SDFS_ERR_HIP, "hipSetDevice(%d) failed", device_id));
  if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(h, SDFS_ERR_HIP, "hipStreamCreate failed"));
  h->stream = h->own_stream;
  h->dense = true; h->model = -1; h->ndim = 1; h->N = N; h->shape[0] = (int)N;
  h->plan[0].nloc = N; h->plan[1].nloc = 0;
  h->beta = beta; h->theta = theta;
  int rc = upload(h, &h->denseH, H, (size_t)N * (size_t)N);
  if (rc) return bail(rc);
  *out = h;
  return 0;
}

int sdfs_lin_interp(int device_id, int ndim, const int64_t* shapes, const double* const* grids,
                    const double* fun_vals, const double* x, int64_t nq, double* out) {
  if (!shapes || !grids || !fun_vals || !x || !out || nq < 0) return fail(nullptr, SDFS_ERR_ARG, "NULL argument");
  if (ndim != 4 && ndim != 6) return fail(nullptr, SDFS_ERR_UNSUPPORTED, "lin_interp supports 4 or 6 dimensions");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, SDFS_ERR_HIP, "no HIP device available (libsdfs_hip has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev || hipSetDevice(device_id) != hipSuccess)
    return fail(nullptr, SDFS_ERR_ARG, "bad device_id %d", device_id);
  if (nq == 0) return 0;
  sdfs_handle tmp;                       // only for error text and allocation tracking
  ContDesc cd;
  int rc = cont_geometry(&tmp, cd, ndim, shapes, grids);
  if (rc) { g_create_error = tmp.err; return rc; }
  double *f = nullptr, *xd = nullptr, *od = nullptr;
  auto done = [&](int code) { for (double* p : tmp.dev_allocs) hipFree(p); if (code) g_create_error = tmp.err; return code; };
  if ((rc = upload(&tmp, &f, fun_vals, (size_t)cd.N)) || (rc = upload(&tmp, &xd, x, (size_t)nq * ndim)) ||
      (rc = dev_alloc(&tmp, &od, (size_t)nq)))
    return done(rc);
  const dim3 grid((unsigned)((nq + 255) / 256)), block(256);
  if (ndim == 4) hipLaunchKernelGGL((lin_interp_kernel<4>), grid, block, 0, 0, cd, f, xd, (long long)nq, od);
  else hipLaunchKernelGGL((lin_interp_kernel<6>), grid, block, 0, 0, cd, f, xd, (long long)nq, od);
  if (hipGetLastError() != hipSuccess || hipMemcpy(out, od, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
    fail(&tmp, SDFS_ERR_HIP, "lin_interp launch / copy failed");
    return done(SDFS_ERR_HIP);
  }
  return done(0);
}

void sdfs_destroy(sdfs_handle* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->sa_graph) hipGraphExecDestroy(h->sa_graph);
  if (h->anderson.graph) hipGraphExecDestroy(h->anderson.graph);
  for (void* p : {(void*)h->anderson.state_host, (void*)h->anderson.err_host, (void*)h->anderson.kind_host, (void*)h->anderson.gram_row_host})
    if (p) hipHostFree(p);
  for (int i = 0; i < 2; ++i) if (h->bicg_graph[i]) hipGraphExecDestroy(h->bicg_graph[i]);
  for (double* p : h->dev_allocs) hipFree(p);
  if (h->price.res) hipFree(h->price.res);
  for (void* p : h->misc_allocs) hipFree(p);
  if (h->slots) hipFree(h->slots);
  if (h->slots_host) hipHostFree(h->slots_host);
  if (h->sc_host) hipHostFree(h->sc_host);
  if (h->bicg_gate_host) hipHostFree(h->bicg_gate_host);
  for (auto& p : h->pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  for (auto e : h->event_pool) hipEventDestroy(e);
  if (h->own_stream) hipStreamDestroy(h->own_stream);
  delete h;
}

const char* sdfs_last_error(const sdfs_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int sdfs_default_opts(sdfs_opts* o) {
  if (!o) return SDFS_ERR_ARG;
  memset(o, 0, sizeof *o);
  o->tol = 1e-7;               // code/solvers.py:16
  o->max_iter = 1000000;       // code/solvers.py:17
  o->inner_rtol = 1e-5;        // jax bicgstab default tol
  o->inner_atol = 1e-4;        // code/solvers.py:55
  o->inner_max_iter = 0;
  o->history = 10; o->mixing_freq = 4; o->beta = 8.0; o->ridge = 1e-6;   // code/solvers.py:104-114
  o->check_every = 0;            // the library's choice (sdfs_solve_dev)
  o->use_graph = 1;
  o->record_errors = 0;
  o->krylov_f32 = 0;
  o->t_f32 = 0;
  return 0;
}

int64_t sdfs_grid_size(const sdfs_handle* h) { return h ? h->N : -1; }

int sdfs_set_stream(sdfs_handle* h, void* s, int use_own) {
  int rc = check(h); if (rc) return rc;
  hipStream_t ns = use_own ? h->own_stream : (hipStream_t)s;     // s == NULL is the device's default stream
  if (ns != h->stream && h->sa_graph) { hipGraphExecDestroy(h->sa_graph); h->sa_graph = nullptr; }
  if (ns != h->stream && h->anderson.graph) { hipGraphExecDestroy(h->anderson.graph); h->anderson.graph = nullptr; }
  if (ns != h->stream) for (int i = 0; i < 2; ++i) if (h->bicg_graph[i]) { hipGraphExecDestroy(h->bicg_graph[i]); h->bicg_graph[i] = nullptr; }
  h->stream = ns;
  return 0;
}

int sdfs_synchronize(sdfs_handle* h) {
  int rc = check(h); if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int sdfs_apply_T_dev(sdfs_handle* h, const double* w, double* Tw, double* resid_dev) {
  int rc = check(h); if (rc) return rc;
  if (!w || !Tw) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  if (h->sharded) return fail(h, SDFS_ERR_ARG, "sharded handle: use sdfs_apply_stage_dev");
  // (the pair plan's first kernel clears the residual word itself: one launch less per step)
  if (resid_dev && !(h->fast.ok && !h->cont && !h->dense)) HIPCHK(h, hipMemsetAsync(resid_dev, 0, 8, h->stream));
  return apply_T_dev(h, w, Tw, (unsigned long long*)resid_dev, nullptr, 0.0);
}

int sdfs_apply_T(sdfs_handle* h, const double* w_host, double* Tw_host) {
  int rc = check(h); if (rc) return rc;
  if (!w_host || !Tw_host) return fail(h, SDFS_ERR_ARG, "NULL host pointer");
  if (h->sharded) return fail(h, SDFS_ERR_ARG, "sharded handle: use sdfs_apply_stage_dev");
  if ((rc = ensure_buf(h, &h->hostio)) || (rc = ensure_buf(h, &h->hostio2)) || (rc = ensure_slots(h, 2))) return rc;
  const size_t nb = sizeof(double) * (size_t)h->N;
  HIPCHK(h, hipMemcpyAsync(h->hostio, w_host, nb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(h->slots, 0, 8, h->stream));
  if ((rc = apply_T_dev(h, h->hostio, h->hostio2, h->slots, nullptr, 0.0))) return rc;
  HIPCHK(h, hipMemcpyAsync(Tw_host, h->hostio2, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->slots_host, h->slots, 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->last_resid = bits_to_double(h->slots_host[0]);
  return 0;
}

int sdfs_linearize_dev(sdfs_handle* h, const double* w, double* Tw) {
  int rc = check(h); if (rc) return rc;
  if (!w) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  if (h->sharded) return fail(h, SDFS_ERR_ARG, "sharded handle: use sdfs_apply_stage_dev");
  double* out = Tw;
  if (!out) { if ((rc = ensure_buf(h, &h->hostio3))) return rc; out = h->hostio3; }
  if ((rc = apply(h, Apply(MODE_T_LIN, w, out, w)))) return rc;
  h->lin_stale = false;
  return 0;
}

int sdfs_apply_jvp_dev(sdfs_handle* h, const double* v, double* out, int minus_identity) {
  int rc = check(h); if (rc) return rc;
  if (!v || !out) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  if (h->sharded) return fail(h, SDFS_ERR_ARG, "sharded handle: use sdfs_apply_stage_dev");
  if (!h->c1 || !h->c2 || h->lin_stale) return fail(h, SDFS_ERR_ARG, "sdfs_apply_jvp_dev before sdfs_linearize_dev");
  Apply a(MODE_JVP, v, out, v);
  a.minus_identity = minus_identity;
  return apply(h, a);
}

int sdfs_apply_jvp(sdfs_handle* h, const double* w_host, const double* v_host, double* out_host) {
  int rc = check(h); if (rc) return rc;
  if (!w_host || !v_host || !out_host) return fail(h, SDFS_ERR_ARG, "NULL host pointer");
  if ((rc = ensure_buf(h, &h->hostio)) || (rc = ensure_buf(h, &h->hostio2)) || (rc = ensure_buf(h, &h->hostio3))) return rc;
  const size_t nb = sizeof(double) * (size_t)h->N;
  HIPCHK(h, hipMemcpyAsync(h->hostio, w_host, nb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->hostio2, v_host, nb, hipMemcpyHostToDevice, h->stream));
  if ((rc = sdfs_linearize_dev(h, h->hostio, h->hostio3))) return rc;
  if ((rc = sdfs_apply_jvp_dev(h, h->hostio2, h->hostio3, 0))) return rc;
  HIPCHK(h, hipMemcpyAsync(out_host, h->hostio3, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int sdfs_apply_vjp_dev(sdfs_handle* h, const double* u, double* out, int minus_identity) {
  int rc = check(h); if (rc) return rc;
  if (!u || !out) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  if (h->sharded) return fail(h, SDFS_ERR_ARG, "sharded handle: no vector-Jacobian product");
  if (!h->c1 || !h->c2 || h->lin_stale) return fail(h, SDFS_ERR_ARG, "sdfs_apply_vjp_dev before sdfs_linearize_dev");
  // (a continuous handle has sdfs_cont_apply_vjp_dev, whose result is reproducible to rounding only: never behind this name)
  if (h->cont) return fail(h, SDFS_ERR_UNSUPPORTED, "the vector-Jacobian product exists for the discretised operator only");
  Apply a(MODE_VJP, u, out, u);
  a.minus_identity = minus_identity;
  return apply(h, a);
}

int sdfs_apply_vjp(sdfs_handle* h, const double* w_host, const double* u_host, double* out_host) {
  int rc = check(h); if (rc) return rc;
  if (!w_host || !u_host || !out_host) return fail(h, SDFS_ERR_ARG, "NULL host pointer");
  if ((rc = ensure_buf(h, &h->hostio)) || (rc = ensure_buf(h, &h->hostio2)) || (rc = ensure_buf(h, &h->hostio3))) return rc;
  const size_t nb = sizeof(double) * (size_t)h->N;
  HIPCHK(h, hipMemcpyAsync(h->hostio, w_host, nb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->hostio2, u_host, nb, hipMemcpyHostToDevice, h->stream));
  if ((rc = sdfs_linearize_dev(h, h->hostio, h->hostio3))) return rc;
  if ((rc = sdfs_apply_vjp_dev(h, h->hostio2, h->hostio3, 0))) return rc;
  HIPCHK(h, hipMemcpyAsync(out_host, h->hostio3, nb, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int sdfs_param_tangent_dev(sdfs_handle* h, const double* w, const double* dparams, const double* const* darrays,
                           double* out, double* Tw) {
  return sdfs_param_tangent_gen_dev(h, w, dparams, darrays, nullptr, out, Tw);
}

int sdfs_param_tangent_gen_dev(sdfs_handle* h, const double* w, const double* dparams, const double* const* darrays,
                               const double* const* dgen, double* out, double* Tw) {
  int rc = check(h); if (rc) return rc;
  if (!w || !out || !dparams) return fail(h, SDFS_ERR_ARG, "NULL argument");
  if (h->cont || h->dense || h->sharded)
    return fail(h, SDFS_ERR_UNSUPPORTED, "parameter tangents exist for unsharded discretised (multi-index) handles only");
  double dtheta = 0.0, dbeta = 0.0;
  SensTab dla1, dla2;
  bool need_jv = false, any_a3 = false;
  if ((rc = sens_tables(h, dparams, darrays, &dtheta, &dbeta, dla1, dla2, &need_jv, &any_a3))) return rc;
  bool any_gen = false;
  if (dgen) {
    for (int a = 0; a < h->ndim; ++a) {
      if (!dgen[a]) continue;
      any_gen = true;
      for (int k = 0; k < 3 * h->shape[a]; ++k) {
        if (k == 0 || k == 3 * h->shape[a] - 1) continue;        // sub[0], super[n - 1]: ignored
        if (!std::isfinite(dgen[a][k])) return fail(h, SDFS_ERR_ARG, "dgen[%d][%d] is not finite", a, k);
      }
    }
  }
  if (any_gen) {
    // dQ_a = G_a Q_a becomes a stencil on E along axis a only when no other axis' matrix depends on the state of a
    for (int a = 0; a < h->ndim; ++a)
      if (h->ax[a].qcount != 1)
        return fail(h, SDFS_ERR_UNSUPPORTED, "a generator tangent needs unconditional transition tensors "
                                             "(axis %s is conditional)", h->ax[a].name);
    if (!h->sens.la3) {
      const auto& S = h->sens;
      std::vector<double> la3(S.z.size());
      for (size_t i = 0; i < la3.size(); ++i) la3[i] = (1.0 - S.gamma) * (S.mu_c + S.z[i]);
      if ((rc = upload(h, &h->sens.la3, la3.data(), la3.size()))) return rc;
    }
  }
  if (!Tw) { if ((rc = ensure_buf(h, &h->hostio3))) return rc; Tw = h->hostio3; }
  if (need_jv && (rc = ensure_buf(h, &h->sens.v))) return rc;
  if (any_a3) {
    if (!h->sens.dla3 && (rc = dev_alloc(h, &h->sens.dla3, h->sens.z.size()))) return rc;
    // (the previous call's epilogue may still read the table; its staging copy may still be in flight)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpyAsync(h->sens.dla3, h->sens.dla3_host.data(), sizeof(double) * h->sens.z.size(),
                             hipMemcpyHostToDevice, h->stream));
  }
  // linearise at w (T w, and the cache of c1 / c2 the J.v below and a later sdfs_solve_linear_dev use)
  if ((rc = apply(h, Apply(MODE_T_LIN, w, Tw, w)))) return rc;
  h->lin_stale = false;
  SensGeom g;
  memset(&g, 0, sizeof g);
  g.n = h->N; g.ndim = h->ndim;
  for (int a = 0; a < h->ndim; ++a) { g.ext[a] = h->shape[a]; g.a3s[a] = h->sens.a3s[a]; }
  const int grid = stream_grid(h, h->N, SENS_BLOCK);
  const double n8 = 8.0 * (double)h->N;
  if (need_jv) {
    g.ax_tab = h->sens.ax_a1;
    if ((rc = launch_kernel(h, k_sens_prologue, dim3(grid), dim3(SENS_BLOCK), 0, Counter("sens:prologue", 2 * n8, 0), g, dla1, dtheta, w,
                            h->sens.v)))
      return rc;
    if ((rc = apply(h, Apply(MODE_JVP, h->sens.v, out, h->sens.v)))) return rc;
  }
  g.ax_tab = h->sens.ax_a2;
  if ((rc = launch_kernel(h, k_sens_epilogue, dim3(grid), dim3(SENS_BLOCK), 0,
                          Counter(need_jv ? "sens:epilogue" : "sens:epilogue_nojv", (need_jv ? 3 : 2) * n8, 0), g, dla2, dbeta / h->beta,
                          dtheta / h->theta, 1.0 / h->beta, 1.0 / h->theta, (const double*)Tw, need_jv ? (const double*)out : nullptr,
                          any_a3 ? (const double*)h->sens.dla3 : nullptr, out)))
    return rc;
  if (any_gen) {
    SensTab la2;
    for (int i = 0; i < SENS_MAXN; ++i) la2.t[i] = 0.0;
    for (size_t k = 0; k < h->sens.sigc.size(); ++k) {
      const double s = (1.0 - h->sens.gamma) * h->sens.sigc[k];
      la2.t[k] = 0.5 * s * s;
    }
    for (int a = 0; a < h->ndim; ++a) {
      if (!dgen[a]) continue;
      const int n = h->shape[a];
      SensGen G;
      memset(&G, 0, sizeof G);
      for (int i = 0; i < n; ++i) {
        G.sub[i] = i > 0 ? dgen[a][i] : 0.0;
        G.diag[i] = dgen[a][n + i];
        G.sup[i] = i < n - 1 ? dgen[a][2 * n + i] : 0.0;
      }
      // Tw, out read and out written; the two neighbours along the axis come from lines the sweep fetches anyway
      if ((rc = launch_kernel(h, k_sens_generator, dim3(grid), dim3(SENS_BLOCK), 0, Counter("sens:generator", 3 * n8, 0), g, G, la2, a,
                              h->theta, 1.0 / h->theta, (const double*)Tw, (const double*)h->sens.la3, out)))
        return rc;
    }
  }
  return 0;
}

namespace {
// x = (I - A)^{-1} rhs with the fp64 device BiCGSTAB, A = J (MODE_JVP), J^T (MODE_VJP) or, with (lc1, lc2), the J.v
// kernels on those scalings.  fp64 storage.
int linear_solve(sdfs_handle* h, const sdfs_opts& o, int mode, const double* rhs, double* x, int64_t* n_iter,
                 double* final_rel_resid, const double* lc1, const double* lc2, const char* what) {
  int rc;
  if ((rc = ensure_scalars(h))) return rc;
  while (h->kry.size() < 7) { double* p = nullptr; if ((rc = dev_alloc(h, &p, (size_t)h->N))) return rc; h->kry.push_back(p); }
  const long long n = h->N;
  const int grid = stream_grid(h, n, SENS_BLOCK);
  // the loop solves (A - I) y = b: b = -rhs gives y = (I - A)^{-1} rhs
  hipLaunchKernelGGL(k_sens_neg, dim3(grid), dim3(SENS_BLOCK), 0, h->stream, rhs, h->kry[6], n);
  HIPCHK(h, hipGetLastError());
  int64_t mv = 0;
  if ((rc = bicgstab_dev_t<double>(h, o, &mv, PREC_F64, mode, lc1, lc2))) return rc;
  HIPCHK(h, hipMemcpyAsync(x, h->kry[5], sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));          // (the loop's last read of the scalars preceded this copy)
  const double rr = h->sc_host[SC_RR], bb = h->sc_host[SC_BB], a2 = h->sc_host[SC_ATOL2];
  const long long its = (long long)h->sc_host[SC_ITERS];
  const double rel = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
  if (n_iter) *n_iter = its;
  if (final_rel_resid) *final_rel_resid = rel;
  if (!(rr <= a2))
    return fail(h, SDFS_ERR_NUMERIC, "%s BiCGSTAB stopped at relative residual %.3e after %lld iterations (%s)",
                what, rel, its,
                h->sc_host[SC_BREAK] != 0.0 ? "breakdown" : (std::isfinite(rr) ? "not converged" : "non-finite residual"));
  return 0;
}
}  // namespace

int sdfs_solve_linear_dev(sdfs_handle* h, int transpose, const sdfs_opts* opts, const double* rhs, double* x,
                          int64_t* n_iter, double* final_rel_resid) {
  int rc = check(h); if (rc) return rc;
  if (!rhs || !x) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  if (h->sharded) return fail(h, SDFS_ERR_UNSUPPORTED, "sharded handle: no single-handle linear solve");
  if (!h->c1 || !h->c2 || h->lin_stale) return fail(h, SDFS_ERR_ARG, "sdfs_solve_linear_dev before a linearisation (sdfs_linearize_dev, "
                                    "sdfs_param_tangent_dev)");
  if (transpose) {                         // where sdfs_apply_vjp_dev is unsupported (run_plan, MODE_VJP)
    if (h->cont || h->dense) return fail(h, SDFS_ERR_UNSUPPORTED, "the vector-Jacobian product exists for the discretised operator only");
    for (int a = 0; a < h->ndim; ++a)
      if (!h->ax[a].Qt) return fail(h, SDFS_ERR_UNSUPPORTED, "the transposed solve needs unconditional transition tensors "
                                    "(axis %s is conditional)", h->ax[a].name);
  }
  sdfs_opts o;
  if (opts) o = *opts; else sdfs_default_opts(&o);
  if (o.krylov_f32 != 0) return fail(h, SDFS_ERR_ARG, "sdfs_solve_linear_dev is fp64 only (opts.krylov_f32 = %d)", o.krylov_f32);
  return linear_solve(h, o, transpose ? MODE_VJP : MODE_JVP, rhs, x, n_iter, final_rel_resid, nullptr, nullptr,
                      transpose ? "transposed" : "plain");
}

namespace {
PriceGeom price_geom(const sdfs_handle* h) {
  PriceGeom g;
  memset(&g, 0, sizeof g);
  g.n = h->N; g.ndim = h->ndim;
  for (int a = 0; a < h->ndim; ++a) { g.ext[a] = price_div((unsigned)h->shape[a]); g.a3s[a] = h->sens.a3s[a]; }
  g.ax_lam = h->sens.ax_a1; g.ax_c = h->sens.ax_a2;
  return g;
}

int price_handle_ok(sdfs_handle* h, const char* fn, bool need_tilt) {
  if (h->cont || h->dense || h->sharded)
    return fail(h, SDFS_ERR_UNSUPPORTED, "%s: pricing exists for unsharded discretised (multi-index) handles only", fn);
  if (need_tilt && h->price.power < 0) return fail(h, SDFS_ERR_ARG, "%s before sdfs_set_tilt_dev", fn);
  return 0;
}

int price_grid(const sdfs_handle* h) {
  return (int)std::max<long long>(1, std::min<long long>((h->N + PRICE_BLOCK - 1) / PRICE_BLOCK,
                                                         std::min<long long>((long long)h->num_cus * 8, PRICE_MAX_BLOCKS)));
}

// -- shared with the continuous-state pricing entry points (cont_price.hpp) --
// x = (I - K)^{-1} rhs, K the J.v kernels on the tilt's scalings (lc1, lc2); fp64 whatever the options say
int tilted_solve(sdfs_handle* h, const sdfs_opts* opts, const double* rhs, double* x, int64_t* n_iter, double* final_rel_resid,
                 const double* lc1, const double* lc2, const char* what) {
  if (!rhs || !x) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  sdfs_opts o;
  if (opts) o = *opts; else sdfs_default_opts(&o);
  o.krylov_f32 = 0;
  return linear_solve(h, o, MODE_JVP, rhs, x, n_iter, final_rel_resid, lc1, lc2, what);
}

// the save list of a horizon loop: horizons rising strictly within 1 ... n_max, a device grid for each
int save_list_ok(sdfs_handle* h, int64_t n_max, int64_t n_save, const int64_t* save_at, double* const* save_dev) {
  if (n_save < 0 || (n_save > 0 && (!save_at || !save_dev))) return fail(h, SDFS_ERR_ARG, "bad save list");
  for (int64_t j = 0; j < n_save; ++j) {
    if (save_at[j] < 1 || save_at[j] > n_max || (j > 0 && save_at[j] <= save_at[j - 1]))
      return fail(h, SDFS_ERR_ARG, "save_at must rise strictly within 1 ... n_max (save_at[%lld] = %lld)", (long long)j,
                  (long long)save_at[j]);
    if (!save_dev[j]) return fail(h, SDFS_ERR_ARG, "save_dev[%lld] is NULL", (long long)j);
  }
  return 0;
}

// P_n = K P_{n-1}, P_0 = 1 (written by `fill`) for n = 1 ... n_max on the pair (prev, cur), K as in tilted_solve.  After
// the product of horizon n, per_horizon(n, P_n, P_{n-1}) enqueues what the caller keeps of it; then P_n goes to
// save_dev[j] where n = save_at[j].
int horizon_loop(sdfs_handle* h, long long N, int64_t n_max, void (*fill)(double*, long long, double), int block, double* prev,
                 double* cur, const double* lc1, const double* lc2, int64_t n_save, const int64_t* save_at, double* const* save_dev,
                 const std::function<void(int64_t, const double*, const double*)>& per_horizon) {
  hipLaunchKernelGGL(fill, dim3(stream_grid(h, N, block)), dim3(block), 0, h->stream, prev, N, 1.0);
  HIPCHK(h, hipGetLastError());
  int64_t js = 0;
  for (int64_t n = 1; n <= n_max; ++n) {
    Apply a(MODE_JVP, prev, cur, prev);
    a.lc1 = lc1; a.lc2 = lc2;
    if (int rc = apply(h, a)) return rc;
    per_horizon(n, (const double*)cur, (const double*)prev);
    HIPCHK(h, hipGetLastError());
    if (js < n_save && save_at[js] == n) {
      HIPCHK(h, hipMemcpyAsync(save_dev[js], cur, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, h->stream));
      ++js;
    }
    std::swap(prev, cur);
  }
  return 0;
}
}  // namespace

int sdfs_set_tilt_dev(sdfs_handle* h, const double* w, int sdf_power, double kappa_lam, double kappa_c) {
  int rc = check(h); if (rc) return rc;
  if ((rc = price_handle_ok(h, "sdfs_set_tilt_dev", false))) return rc;
  if (sdf_power < 0 || sdf_power > 2) return fail(h, SDFS_ERR_ARG, "sdf_power = %d: 0, 1 or 2", sdf_power);
  if (sdf_power > 0 && !w) return fail(h, SDFS_ERR_ARG, "sdf_power = %d needs the linearisation point w", sdf_power);
  if (!std::isfinite(kappa_lam) || !std::isfinite(kappa_c)) return fail(h, SDFS_ERR_ARG, "non-finite tilt exponent");
  auto& S = h->sens;
  auto& Pr = h->price;
  Pr.power = -1;                           // (until the scalings below are in place)
  // e_lam = exp((kappa_lam - theta) h_lam), e_c = exp((1/2)(kappa_c^2 - (1-gamma)^2) sigma_c^2),
  // e_z = exp((kappa_c - (1-gamma)) (mu_c + z)); every exponent is exactly 0 at (kappa_lam, kappa_c) = (theta, 1 - gamma).
  // Where a3 is a table the aggregator applies (h->a3), the J.v passes leave it out and the cached c2 carries it
  // (c2 = beta u / S with S unscaled): e_z then also replaces c2^p's a3^p by the a3 of H', exponent kappa_c - p (1-gamma).
  const double og = 1.0 - S.gamma;
  const double xl = kappa_lam - h->theta, xc = 0.5 * (kappa_c * kappa_c - og * og);
  const double xz = h->a3 ? kappa_c - sdf_power * og : kappa_c - og;
  SensTab el, ec;
  for (int i = 0; i < SENS_MAXN; ++i) { el.t[i] = 1.0; ec.t[i] = 1.0; }
  for (size_t l = 0; l < S.hlam.size(); ++l) el.t[l] = std::exp(xl * S.hlam[l]);
  for (size_t k = 0; k < S.sigc.size(); ++k) ec.t[k] = std::exp(xc * S.sigc[k] * S.sigc[k]);
  if ((rc = ensure_buf(h, &Pr.d1)) || (rc = ensure_buf(h, &Pr.d2))) return rc;
  if (xz != 0.0) {
    if (!Pr.ez && (rc = dev_alloc(h, &Pr.ez, S.z.size()))) return rc;
    // (the previous call's scaling pass may still read the table; its staging copy may still be in flight)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    Pr.ez_host.resize(S.z.size());
    for (size_t i = 0; i < S.z.size(); ++i) Pr.ez_host[i] = std::exp(xz * (S.mu_c + S.z[i]));
    HIPCHK(h, hipMemcpyAsync(Pr.ez, Pr.ez_host.data(), sizeof(double) * S.z.size(), hipMemcpyHostToDevice, h->stream));
  }
  if (w) {
    // linearise at w in fp64: c1 = w^(theta-1), c2 = beta^theta (Tw - 1)^(1-theta) (replaces the cached linearisation)
    // (T w stays in the tilt's own buffer: sdfs_tilt_tangent_dev reads it)
    if ((rc = ensure_buf(h, &Pr.tw))) return rc;
    if ((rc = apply(h, Apply(MODE_T_LIN, w, Pr.tw, w)))) return rc;
    h->lin_stale = false;
  }
  const PriceGeom g = price_geom(h);
  const int grid = stream_grid(h, h->N, PRICE_BLOCK);
  const double* ez = xz != 0.0 ? (const double*)Pr.ez : nullptr;
  const double n8 = 8.0 * (double)h->N;
  // (power 0 reads no linearisation)
  auto fn = k_tilt_scalings<0>;
  if (sdf_power == 1) fn = k_tilt_scalings<1>;
  else if (sdf_power == 2) fn = k_tilt_scalings<2>;
  if ((rc = launch_kernel(h, fn, dim3(grid), dim3(PRICE_BLOCK), 0,
                          Counter(sdf_power == 0 ? "price:tilt0" : (sdf_power == 1 ? "price:tilt1" : "price:tilt2"), (sdf_power == 0 ? 2 : 4) * n8, 0),
                          g, el, ec, ez, sdf_power ? (const double*)h->c1 : nullptr, sdf_power ? (const double*)h->c2 : nullptr, Pr.d1, Pr.d2)))
    return rc;
  Pr.power = sdf_power;
  Pr.kappa_lam = kappa_lam; Pr.kappa_c = kappa_c;
  return 0;
}

int sdfs_apply_tilted_dev(sdfs_handle* h, const double* f, double* out) {
  int rc = check(h); if (rc) return rc;
  if ((rc = price_handle_ok(h, "sdfs_apply_tilted_dev", true))) return rc;
  if (!f || !out) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  Apply a(MODE_JVP, f, out, f);
  a.lc1 = h->price.d1; a.lc2 = h->price.d2;
  return apply(h, a);
}

int sdfs_solve_tilted_dev(sdfs_handle* h, const sdfs_opts* opts, const double* rhs, double* x, int64_t* n_iter,
                          double* final_rel_resid) {
  int rc = check(h); if (rc) return rc;
  if ((rc = price_handle_ok(h, "sdfs_solve_tilted_dev", true))) return rc;
  return tilted_solve(h, opts, rhs, x, n_iter, final_rel_resid, h->price.d1, h->price.d2, "tilted");
}

int sdfs_tilt_tangent_dev(sdfs_handle* h, const double* w, const double* dw, const double* dtw, const double* dparams,
                          const double* const* darrays, const double* const* dgen, double dkappa_lam, double dkappa_c,
                          const double* f, const double* df, const double* kf, double* out) {
  int rc = check(h); if (rc) return rc;
  if ((rc = price_handle_ok(h, "sdfs_tilt_tangent_dev", true))) return rc;
  if (!dparams || !out) return fail(h, SDFS_ERR_ARG, "NULL argument");
  auto& S = h->sens;
  auto& Pr = h->price;
  const int P = Pr.power;
  if (P >= 1 && (!w || !dw || !dtw))
    return fail(h, SDFS_ERR_ARG, "sdf_power = %d needs w, its direction dw and the direction dtw of T w", P);
  if (!std::isfinite(dkappa_lam) || !std::isfinite(dkappa_c)) return fail(h, SDFS_ERR_ARG, "non-finite tilt exponent tangent");
  if (out == kf || out == f || out == df || (P >= 1 && (out == w || out == dw || out == dtw)))
    return fail(h, SDFS_ERR_ARG, "out must be distinct from every input grid");
  auto darr = [&](int i) -> const double* { return darrays ? darrays[i] : nullptr; };
  for (int i : S.trans) {
    const double* d = darr(i);
    if (!d) continue;
    for (long long k = 0; k < S.sizes[i]; ++k)
      if (d[k] != 0.0) return fail(h, SDFS_ERR_UNSUPPORTED, "arrays[%d] is a transition array: its tangent must be zero "
                                   "(a persistence parameter states dQ = G Q through dgen)", i);
  }
  bool any_gen = false;
  if (dgen) {
    for (int a = 0; a < h->ndim; ++a) {
      if (!dgen[a]) continue;
      any_gen = true;
      for (int k = 1; k < 3 * h->shape[a] - 1; ++k)                // sub[0], super[n - 1]: ignored
        if (!std::isfinite(dgen[a][k])) return fail(h, SDFS_ERR_ARG, "dgen[%d][%d] is not finite", a, k);
    }
  }
  if (any_gen)
    for (int a = 0; a < h->ndim; ++a)
      if (h->ax[a].qcount != 1)
        return fail(h, SDFS_ERR_UNSUPPORTED, "a generator tangent needs unconditional transition tensors "
                                             "(axis %s is conditional)", h->ax[a].name);
  // the direction's scalars and tables (sens_tables reads the same places of dparams / darrays)
  const double th = h->theta, psi = S.psi, kl = Pr.kappa_lam, kc = Pr.kappa_c;
  const double dg = dparams[S.ip_gamma], dpsi = dparams[S.ip_psi], dmu = dparams[S.ip_mu_c], dbeta = dparams[S.ip_beta];
  const double dtheta = -dg / (1.0 - 1.0 / psi) - dpsi * th / (psi * (psi - 1.0));
  const double* dhl = darr(S.ia_hlam);
  const double* dsc = darr(S.ia_sigc);
  const double* dz = darr(S.ia_z);
  SensTab ul, uc;
  for (int i = 0; i < SENS_MAXN; ++i) { ul.t[i] = 0.0; uc.t[i] = 0.0; }
  for (size_t l = 0; l < S.hlam.size(); ++l) ul.t[l] = dkappa_lam * S.hlam[l] + kl * (dhl ? dhl[l] : 0.0);
  for (size_t k = 0; k < S.sigc.size(); ++k)
    uc.t[k] = kc * S.sigc[k] * (dkappa_c * S.sigc[k] + kc * (dsc ? dsc[k] : 0.0));
  const double c0 = P * (th * dbeta / h->beta + dtheta * std::log(h->beta));
  bool any_tz = dkappa_c != 0.0 || kc * dmu != 0.0;
  if (dz && kc != 0.0) for (size_t i = 0; i < S.z.size() && !any_tz; ++i) any_tz = dz[i] != 0.0;
  if ((rc = ensure_buf(h, &Pr.tv))) return rc;
  if (any_tz) {
    if (!Pr.tz && (rc = dev_alloc(h, &Pr.tz, S.z.size()))) return rc;
    // (the previous call's epilogue may still read the table; its staging copy may still be in flight)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    Pr.tz_host.resize(S.z.size());
    for (size_t i = 0; i < S.z.size(); ++i) Pr.tz_host[i] = dkappa_c * (S.mu_c + S.z[i]) + kc * (dmu + (dz ? dz[i] : 0.0));
    HIPCHK(h, hipMemcpyAsync(Pr.tz, Pr.tz_host.data(), sizeof(double) * S.z.size(), hipMemcpyHostToDevice, h->stream));
  }
  if (any_gen && kc != 0.0 && !Pr.zt) {
    std::vector<double> zt(S.z.size());
    for (size_t i = 0; i < zt.size(); ++i) zt[i] = S.mu_c + S.z[i];
    if ((rc = upload(h, &Pr.zt, zt.data(), zt.size()))) return rc;
  }
  const PriceGeom g = price_geom(h);
  const int grid = price_grid(h);
  const double n8 = 8.0 * (double)h->N;
  if (!kf) {                                             // K f by one more product (f = 1: a grid of ones first)
    if ((rc = ensure_buf(h, &Pr.kf))) return rc;
    if (out == Pr.kf) return fail(h, SDFS_ERR_ARG, "out must be distinct from every input grid");
    const double* src = f;
    if (!src) {
      hipLaunchKernelGGL(k_price_fill, dim3(stream_grid(h, h->N, PRICE_BLOCK)), dim3(PRICE_BLOCK), 0, h->stream, Pr.tv, h->N, 1.0);
      HIPCHK(h, hipGetLastError());
      src = Pr.tv;
    }
    Apply a(MODE_JVP, src, Pr.kf, src);
    a.lc1 = Pr.d1; a.lc2 = Pr.d2;
    if ((rc = apply(h, a))) return rc;
    kf = Pr.kf;
  }
  const double* tz = any_tz ? (const double*)Pr.tz : nullptr;
  // the logarithms only where dtheta moves an exponent of w or of T w - 1
  const bool lg = P >= 1 && dtheta != 0.0;
  auto pro = k_tilt_tangent_prologue<0, false>;
  auto epi = k_tilt_tangent_epilogue<0, false>;
  if (P == 1) { pro = lg ? k_tilt_tangent_prologue<1, true> : k_tilt_tangent_prologue<1, false>;
                epi = lg ? k_tilt_tangent_epilogue<1, true> : k_tilt_tangent_epilogue<1, false>; }
  if (P == 2) { pro = lg ? k_tilt_tangent_prologue<2, true> : k_tilt_tangent_prologue<2, false>;
                epi = lg ? k_tilt_tangent_epilogue<2, true> : k_tilt_tangent_epilogue<2, false>; }
  const double pthm1 = P * (th - 1.0), p1mth = P * (1.0 - th), pdth = P * dtheta;
  // counter names carry the number of grids a pass streams (the bytes of a name are set once, at its first launch)
  const int n_pro = 1 + (f ? 1 : 0) + (df ? 1 : 0) + (P ? 2 : 0), n_epi = 3 + (P ? 2 : 0), n_gen = 3 + (P ? 1 : 0);
  char nm_pro[32], nm_epi[32], nm_gen[32];
  snprintf(nm_pro, sizeof nm_pro, "price:dtilt_pro%d%s", n_pro, lg ? "_log" : "");
  snprintf(nm_epi, sizeof nm_epi, "price:dtilt_epi%d%s", n_epi, lg ? "_log" : "");
  snprintf(nm_gen, sizeof nm_gen, "price:dtilt_gen%d", n_gen);
  if ((rc = launch_kernel(h, pro, dim3(grid), dim3(PRICE_BLOCK), 0, Counter(nm_pro, n_pro * n8, 0),
                          g, ul, pthm1, pdth, w, dw, f, df, Pr.tv)))
    return rc;
  {
    Apply a(MODE_JVP, Pr.tv, out, Pr.tv);
    a.lc1 = Pr.d1; a.lc2 = Pr.d2;
    if ((rc = apply(h, a))) return rc;
  }
  if ((rc = launch_kernel(h, epi, dim3(grid), dim3(PRICE_BLOCK), 0,
                          Counter(nm_epi, n_epi * n8, 0), g, uc, c0, p1mth, pdth, tz,
                          (const double*)Pr.tw, dtw, kf, (const double*)out, out)))
    return rc;
  if (any_gen) {
    SensTab qc;
    for (int i = 0; i < SENS_MAXN; ++i) qc.t[i] = 0.0;
    for (size_t k = 0; k < S.sigc.size(); ++k) qc.t[k] = 0.5 * kc * kc * S.sigc[k] * S.sigc[k];
    auto fn = k_tilt_tangent_generator<0>;
    if (P == 1) fn = k_tilt_tangent_generator<1>;
    else if (P == 2) fn = k_tilt_tangent_generator<2>;
    for (int a = 0; a < h->ndim; ++a) {
      if (!dgen[a]) continue;
      const int n = h->shape[a];
      SensGen G;
      memset(&G, 0, sizeof G);
      for (int i = 0; i < n; ++i) {
        G.sub[i] = i > 0 ? dgen[a][i] : 0.0;
        G.diag[i] = dgen[a][n + i];
        G.sup[i] = i < n - 1 ? dgen[a][2 * n + i] : 0.0;
      }
      unsigned inner = 1;
      for (int b = h->ndim - 1; b > a; --b) inner *= (unsigned)h->shape[b];
      // K f, out (and T w) read, out written; the two neighbours along the axis come from lines the sweep fetches anyway
      if ((rc = launch_kernel(h, fn, dim3(grid), dim3(PRICE_BLOCK), 0, Counter(nm_gen, n_gen * n8, 0), g, G, qc, a,
                              inner, p1mth, kc, (const double*)Pr.tw, kc != 0.0 ? (const double*)Pr.zt : nullptr, kf, out)))
        return rc;
    }
  }
  return 0;
}

int sdfs_tilted_horizons_dev(sdfs_handle* h, int64_t n_max, const double* const* weight_axes, int64_t n_save,
                             const int64_t* save_at, double* const* save_dev, double* out_host) {
  int rc = check(h); if (rc) return rc;
  if ((rc = price_handle_ok(h, "sdfs_tilted_horizons_dev", true))) return rc;
  if (n_max < 1 || n_max > (1LL << 24)) return fail(h, SDFS_ERR_ARG, "n_max = %lld: 1 ... 2^24 horizons", (long long)n_max);
  if (!out_host) return fail(h, SDFS_ERR_ARG, "NULL out_host");
  if ((rc = save_list_ok(h, n_max, n_save, save_at, save_dev))) return rc;
  PriceWeights wt;
  for (int a = 0; a < SENS_MAXD; ++a) for (int k = 0; k < SENS_MAXN; ++k) wt.t[a][k] = 0.0;
  for (int a = 0; a < h->ndim; ++a)
    for (int k = 0; k < h->shape[a]; ++k) {
      const double v = weight_axes && weight_axes[a] ? weight_axes[a][k] : 1.0 / h->shape[a];
      if (!std::isfinite(v)) return fail(h, SDFS_ERR_ARG, "weight_axes[%d][%d] is not finite", a, k);
      wt.t[a][k] = v;
    }
  auto& Pr = h->price;
  if ((rc = ensure_buf(h, &Pr.pa)) || (rc = ensure_buf(h, &Pr.pb))) return rc;
  if (!Pr.part && (rc = dev_alloc(h, &Pr.part, (size_t)PRICE_MAX_BLOCKS * PRICE_NSUM))) return rc;
  if (Pr.res_cap < n_max) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (Pr.res) { hipFree(Pr.res); Pr.res = nullptr; Pr.res_cap = 0; }
    HIPCHK(h, hipMalloc((void**)&Pr.res, sizeof(double) * PRICE_NSUM * (size_t)n_max));
    Pr.res_cap = n_max;
  }
  const PriceGeom g = price_geom(h);
  const int rgrid = price_grid(h);
  const int cid = h->profiling ? counter_id(h, "price:horizon_reduce", 16.0 * (double)h->N, 0) : -1;
  rc = horizon_loop(h, h->N, n_max, k_price_fill, PRICE_BLOCK, Pr.pa, Pr.pb, Pr.d1, Pr.d2, n_save, save_at, save_dev,
                    [&](int64_t n, const double* cur, const double* prev) {
    {
      ProfScope ps(h, cid);
      hipLaunchKernelGGL(k_horizon_reduce, dim3(rgrid), dim3(PRICE_BLOCK), 0, h->stream, g, wt, cur, prev, Pr.part);
    }
    hipLaunchKernelGGL(k_horizon_finish, dim3(1), dim3(64), 0, h->stream, (const double*)Pr.part, rgrid, Pr.res + PRICE_NSUM * (n - 1));
  });
  if (rc) return rc;
  std::vector<double> res((size_t)PRICE_NSUM * n_max);
  HIPCHK(h, hipMemcpyAsync(res.data(), Pr.res, sizeof(double) * res.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  long long first_bad = 0;
  for (int64_t n = 1; n <= n_max; ++n) {
    const double* r = res.data() + PRICE_NSUM * (n - 1);
    out_host[4 * (n - 1) + 0] = r[0];
    out_host[4 * (n - 1) + 1] = r[1] / (double)n;
    out_host[4 * (n - 1) + 2] = r[2];
    out_host[4 * (n - 1) + 3] = r[3];
    if (r[4] != 0.0 && first_bad == 0) first_bad = n;
  }
  if (first_bad)
    return fail(h, SDFS_ERR_NUMERIC, "P_n is not strictly positive (or NaN) at %.0f grid points at horizon %lld",
                res[PRICE_NSUM * (first_bad - 1) + 4], first_bad);
  return 0;
}

// -- simulated paths (sim_kernels.hpp) -------------------------------------------------------------------------------
extern "C++" {
namespace {
constexpr int SIM_K_DEFAULT = 2;             // record loads in flight per lane (tools/simulation_times.py A/B)
constexpr bool SIM_LIN_DEFAULT = false;      // inverse-CDF search: binary (false) or linear (true)

int sim_handle_ok(sdfs_handle* h, const char* fn) {
  if (h->cont || h->dense || h->sharded)
    return fail(h, SDFS_ERR_UNSUPPORTED, "%s: simulation exists for unsharded discretised (multi-index) handles only", fn);
  return 0;
}

// k_sim_paths for a look-ahead k, a search and, on the defaults of both, with the paths stored
typedef void (*sim_fn)(SimArgs, const double*, const double*, double*, unsigned char*, double*);

template <int ND, bool KAP, bool LIN, int K>
sim_fn sim_form(bool store) {
  if constexpr (LIN == SIM_LIN_DEFAULT && K == SIM_K_DEFAULT) {
    if (store) return k_sim_paths<ND, KAP, LIN, K, true>;
  }
  return k_sim_paths<ND, KAP, LIN, K, false>;
}

template <int ND, bool KAP>
sim_fn sim_variant(int k, bool lin, bool store) {
  if (lin) return k == 1 ? sim_form<ND, KAP, true, 1>(store) : (k == 2 ? sim_form<ND, KAP, true, 2>(store) : sim_form<ND, KAP, true, 4>(store));
  return k == 1 ? sim_form<ND, KAP, false, 1>(store) : (k == 2 ? sim_form<ND, KAP, false, 2>(store) : sim_form<ND, KAP, false, 4>(store));
}
}  // namespace
}  // extern "C++"

int sdfs_sim_records_dev(sdfs_handle* h, const double* w, const double* v, double* rec) {
  int rc = check(h); if (rc) return rc;
  if ((rc = sim_handle_ok(h, "sdfs_sim_records_dev"))) return rc;
  if (!w || !rec) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  auto& Sm = h->sim;
  const auto& S = h->sens;
  if ((rc = ensure_buf(h, &Sm.one)) || (rc = ensure_buf(h, &Sm.em))) return rc;
  if (!Sm.zt) {
    std::vector<double> zt(S.z.size());
    for (size_t i = 0; i < zt.size(); ++i) zt[i] = S.mu_c + S.z[i];
    if ((rc = upload(h, &Sm.zt, zt.data(), zt.size()))) return rc;
  }
  const int fgrid = stream_grid(h, h->N, PRICE_BLOCK);
  hipLaunchKernelGGL(k_price_fill, dim3(fgrid), dim3(PRICE_BLOCK), 0, h->stream, Sm.one, (long long)h->N, 1.0);
  HIPCHK(h, hipGetLastError());
  // E_x[M] = K(1, theta, -gamma) 1: the product sdf_moments forms, bit for bit
  if ((rc = sdfs_set_tilt_dev(h, w, 1, h->theta, -S.gamma))) return rc;
  if ((rc = sdfs_apply_tilted_dev(h, Sm.one, Sm.em))) return rc;
  return launch_kernel(h, k_sim_records, dim3(fgrid), dim3(PRICE_BLOCK), 0,
                       Counter("sim:records", (double)h->N * (16.0 + (v ? 8.0 : 0.0) + 8.0 * SIM_REC), 0), price_geom(h), (const double*)Sm.zt, w,
                       (const double*)Sm.em, v, rec);
}

int sdfs_sim_paths_dev(sdfs_handle* h, const double* rec, const sdfs_sim_desc* d, double* stats, uint8_t* idx, double* ser) {
  int rc = check(h); if (rc) return rc;
  if ((rc = sim_handle_ok(h, "sdfs_sim_paths_dev"))) return rc;
  if (!rec || !d || !stats) return fail(h, SDFS_ERR_ARG, "NULL records, desc or stats");
  if (!idx != !ser) return fail(h, SDFS_ERR_ARG, "idx and series are stored together: both NULL or neither");
  char msg[160];
  if (!sim_ranges_ok(msg, d->path_offset, d->n_paths, nullptr, d->burn_in, d->n_periods, 0)) return fail(h, SDFS_ERR_ARG, "%s", msg);
  if (d->has_kappa && !std::isfinite(d->kappa)) return fail(h, SDFS_ERR_ARG, "kappa is not finite");
  if (!d->cdf || (!d->start_fixed && !d->cdf0)) return fail(h, SDFS_ERR_ARG, "NULL cumulative transition table");
  const int k = d->lookahead ? d->lookahead : SIM_K_DEFAULT;
  if (k != 1 && k != 2 && k != 4) return fail(h, SDFS_ERR_ARG, "lookahead = %d: 1, 2 or 4", d->lookahead);
  if (d->search < 0 || d->search > 2) return fail(h, SDFS_ERR_ARG, "search = %d: 0, 1 (linear) or 2 (binary)", d->search);
  const bool lin = d->search ? d->search == 1 : SIM_LIN_DEFAULT;
  if (idx && (k != SIM_K_DEFAULT || lin != SIM_LIN_DEFAULT))
    return fail(h, SDFS_ERR_ARG, "stored paths run with the default lookahead and search");
  const auto& S = h->sens;
  SimArgs a{};
  int stride[SIM_MAXD], ncdf = 0, ncdf0 = 0;
  long long st = 1;
  for (int ax = h->ndim - 1; ax >= 0; --ax) { stride[ax] = (int)st; st *= h->shape[ax]; }
  const int bad = sim_layout(h->ndim, h->shape, stride, S.ax_a1, S.ax_a2, d, a, &ncdf, &ncdf0);
  if (bad >= 0)
    return fail(h, SDFS_ERR_ARG, "start[%d] = %d: a state index of axis %d lies in 0 ... %d", bad, d->start[bad], bad, h->shape[bad] - 1);
  if (a.lds_n > SIM_TAB_MAX) return fail(h, SDFS_ERR_ARG, "LDS table of %d doubles", a.lds_n);
  auto& tb = h->sim.tab_host;
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (the previous call's staging copy may still be in flight)
  tb.resize((size_t)a.lds_n);
  sim_fill_table(a, ncdf, ncdf0, d->cdf, d->start_fixed ? nullptr : d->cdf0, S.hlam.data(), S.sigc.data(), tb.data());
  a.theta = h->theta; a.theta_ln_beta = h->theta * std::log(h->beta); a.gamma = S.gamma; a.kappa = d->has_kappa ? d->kappa : 0.0;
  if (!h->sim.tab && (rc = dev_alloc(h, &h->sim.tab, SIM_TAB_MAX))) return rc;
  HIPCHK(h, hipMemcpyAsync(h->sim.tab, tb.data(), sizeof(double) * tb.size(), hipMemcpyHostToDevice, h->stream));
  const dim3 grid((unsigned)((d->n_paths + SIM_BLOCK - 1) / SIM_BLOCK));
  const size_t lds = sizeof(double) * (size_t)a.lds_n;
  const double steps = (double)d->n_paths * (double)(d->burn_in + d->n_periods);
  const bool store = idx != nullptr;
  const sim_fn fn = h->ndim == 4 ? (d->has_kappa ? sim_variant<4, true>(k, lin, store) : sim_variant<4, false>(k, lin, store))
                                 : (d->has_kappa ? sim_variant<6, true>(k, lin, store) : sim_variant<6, false>(k, lin, store));
  return launch_kernel(h, fn, grid, dim3(SIM_BLOCK), lds,
                       Counter("sim:paths", 8.0 * SIM_REC * (double)d->n_paths * (double)(d->n_periods + 1), steps), a,
                       (const double*)h->sim.tab, rec, stats, idx, ser);
}

int sdfs_residual(sdfs_handle* h, double* sup_norm) {
  if (!h || !sup_norm) return SDFS_ERR_ARG;
  *sup_norm = h->last_resid;
  return 0;
}

int sdfs_solve_dev(sdfs_handle* h, int algo, const sdfs_opts* opts, double* w, int64_t* n_iter,
                   int64_t* n_apply, double* final_err) {
  int rc = check(h); if (rc) return rc;
  if (!w || !n_iter || !n_apply || !final_err) return fail(h, SDFS_ERR_ARG, "NULL argument");
  if (h->sharded) return fail(h, SDFS_ERR_ARG, "sharded handle: the multi-GPU loop lives in the host layer");
  sdfs_opts o;
  if (opts) o = *opts; else sdfs_default_opts(&o);
  // check_every <= 0: the library's choice (32; the fused small-grid Anderson loop stretches it to 120) -- an explicit
  // value, 32 included, is honoured
  h->check_every_default = o.check_every < 1;
  if (o.check_every < 1) o.check_every = 32;
  if (o.max_iter < 0) return fail(h, SDFS_ERR_ARG, "max_iter < 0");
  switch (algo) {
    case SDFS_ALGO_SA: return solve_sa(h, o, w, n_iter, n_apply, final_err);
    case SDFS_ALGO_NEWTON: return solve_newton(h, o, w, n_iter, n_apply, final_err);
    case SDFS_ALGO_ANDERSON: return solve_anderson(h, o, w, n_iter, n_apply, final_err);
    default: return fail(h, SDFS_ERR_ARG, "unknown algorithm %d", algo);
  }
}

int sdfs_solve(sdfs_handle* h, int algo, const sdfs_opts* opts, double* w_host, int64_t* n_iter,
               int64_t* n_apply, double* final_err) {
  int rc = check(h); if (rc) return rc;
  if (!w_host) return fail(h, SDFS_ERR_ARG, "NULL host pointer");
  if ((rc = ensure_buf(h, &h->hostio))) return rc;
  const size_t nb = sizeof(double) * (size_t)h->N;
  HIPCHK(h, hipMemcpyAsync(h->hostio, w_host, nb, hipMemcpyHostToDevice, h->stream));
  rc = sdfs_solve_dev(h, algo, opts, h->hostio, n_iter, n_apply, final_err);
  if (rc && rc != SDFS_ERR_NUMERIC) return rc;
  hipError_t e = hipMemcpyAsync(w_host, h->hostio, nb, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(h, SDFS_ERR_HIP, "copy back failed: %s", hipGetErrorString(e));
  return rc;
}

int64_t sdfs_error_trace(sdfs_handle* h, double* out, int64_t cap) {
  if (!h) return -1;
  const int64_t n = (int64_t)h->trace.size();
  if (out) for (int64_t i = 0; i < std::min(n, cap); ++i) out[i] = h->trace[i];
  return n;
}

int sdfs_apply_stage_gated_dev(sdfs_handle* h, int stage, int mode, const double* in, double* out,
                               const double* old, double* resid_dev, const double* gate_dev, double gate_tol) {
  int rc = check(h); if (rc) return rc;
  if (!h->sharded) return fail(h, SDFS_ERR_ARG, "not a sharded handle");
  if (stage < 0 || stage > 1 || mode < 0 || mode > 2) return fail(h, SDFS_ERR_ARG, "bad stage/mode");
  if (!in || !out) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  // (a closed gate leaves the cleared word at zero, so every later gate on it stays closed)
  if (resid_dev && stage == 1) HIPCHK(h, hipMemsetAsync(resid_dev, 0, 8, h->stream));
  Apply a(mode, in, out, old);
  a.resid = stage == 1 ? (unsigned long long*)resid_dev : nullptr;
  a.gate = (const unsigned long long*)gate_dev; a.gate_tol = gate_tol;
  a.minus_identity = (mode == MODE_JVP && old) ? 1 : 0;
  // the handle's stage settings (sdfs_set_krylov_f32, sdfs_set_t_f32)
  a.prec = mode == MODE_T ? (h->stage_t32 ? PREC_T32 : PREC_F64) : (h->stage_f32 ? PREC_F32 : PREC_F64);
  return run_plan(h, h->plan[stage], stage == 0, stage == 1, a);
}

int sdfs_apply_stage_dev(sdfs_handle* h, int stage, int mode, const double* in, double* out,
                         const double* old, double* resid_dev) {
  return sdfs_apply_stage_gated_dev(h, stage, mode, in, out, old, resid_dev, nullptr, 0.0);
}

static int pack_blocks_launch(sdfs_handle* h, int unpack, const void* src, void* dst, int64_t outer, int64_t n_axis, int64_t inner,
                              int nblocks, const int64_t* offs, int elem_bytes, const unsigned long long* gate) {
  int rc = check(h); if (rc) return rc;
  if (!src || !dst || !offs) return fail(h, SDFS_ERR_ARG, "NULL argument");
  if (nblocks < 1) return fail(h, SDFS_ERR_ARG, "at least one block");
  if (nblocks > PACK_MAX_BLOCKS) return fail(h, SDFS_ERR_UNSUPPORTED, "pack: at most %d blocks", PACK_MAX_BLOCKS);
  if (elem_bytes != 8 && elem_bytes != 4) return fail(h, SDFS_ERR_ARG, "elements of 4 or 8 bytes");
  if (outer < 1 || n_axis < 1 || inner < 1 || offs[0] != 0 || offs[nblocks] != n_axis) return fail(h, SDFS_ERR_ARG, "bad block table");
  PackBlocks B;
  memset(&B, 0, sizeof B);
  B.n = nblocks;
  for (int j = 0; j <= nblocks; ++j) {
    if (j > 0 && offs[j] <= offs[j - 1]) return fail(h, SDFS_ERR_ARG, "empty or unordered block");
    B.off[j] = (unsigned)offs[j];
  }
  const long long run_bytes = (long long)inner * elem_bytes;
  const int ub = (run_bytes % 16 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0) ? 16 : elem_bytes;
  const long long innerU = run_bytes / ub;
  const long long total = outer * n_axis * innerU;
  if (total >= (1LL << 31)) return fail(h, SDFS_ERR_UNSUPPORTED, "pack: more than 2^31 units");
  const unsigned grid = (unsigned)std::min<long long>((total + VEC_BLOCK - 1) / VEC_BLOCK, 8192);
#define SDFS_PACK_LAUNCH(U)                                                                                              \
  do {                                                                                                                   \
    if (unpack && gate) hipLaunchKernelGGL((k_pack_blocks<U, true, false, true>), dim3(grid), dim3(VEC_BLOCK), 0, h->stream,   \
                                           (const U*)src, (U*)dst, (unsigned)outer, (unsigned)n_axis, (unsigned)innerU, B,       \
                                           (const U*)nullptr, gate);                                                     \
    else if (unpack) hipLaunchKernelGGL((k_pack_blocks<U, true>), dim3(grid), dim3(VEC_BLOCK), 0, h->stream, (const U*)src, (U*)dst, \
                                   (unsigned)outer, (unsigned)n_axis, (unsigned)innerU, B);                              \
    else hipLaunchKernelGGL((k_pack_blocks<U, false>), dim3(grid), dim3(VEC_BLOCK), 0, h->stream, (const U*)src, (U*)dst,       \
                            (unsigned)outer, (unsigned)n_axis, (unsigned)innerU, B);                                     \
  } while (0)
  if (ub == 16) SDFS_PACK_LAUNCH(double2);
  else if (ub == 8) SDFS_PACK_LAUNCH(double);
  else SDFS_PACK_LAUNCH(float);
#undef SDFS_PACK_LAUNCH
  HIPCHK(h, hipGetLastError());
  return 0;
}

int sdfs_pack_blocks(sdfs_handle* h, int unpack, const void* src, void* dst, int64_t outer, int64_t n_axis, int64_t inner,
                     int nblocks, const int64_t* offs, int elem_bytes) {
  return pack_blocks_launch(h, unpack, src, dst, outer, n_axis, inner, nblocks, offs, elem_bytes, nullptr);
}

int sdfs_unpack_blocks_gated(sdfs_handle* h, const void* packed, void* grid_out, int64_t outer, int64_t n_axis, int64_t inner,
                             int nblocks, const int64_t* offs, int elem_bytes, const void* gate_dev) {
  if (!gate_dev) { int rc = check(h); if (rc) return rc; return fail(h, SDFS_ERR_ARG, "NULL gate"); }
  return pack_blocks_launch(h, 1, packed, grid_out, outer, n_axis, inner, nblocks, offs, elem_bytes, (const unsigned long long*)gate_dev);
}

int sdfs_stream_copy_dev(sdfs_handle* h, const double* src_dev, double* dst_dev, int64_t n) {
  int rc = check(h); if (rc) return rc;
  if (!src_dev || !dst_dev || n < 1) return fail(h, SDFS_ERR_ARG, "bad argument");
  if (((uintptr_t)src_dev | (uintptr_t)dst_dev) % 16 != 0) return fail(h, SDFS_ERR_ARG, "16-byte aligned buffers");
  const long long units = n / 2;
  const long long per = (long long)VEC_BLOCK * COPY_UNITS;
  const unsigned grid = (unsigned)std::max<long long>(1, (units + per - 1) / per);
  hipLaunchKernelGGL(k_stream_copy, dim3(grid), dim3(VEC_BLOCK), 0, h->stream, src_dev, dst_dev, units, (long long)n);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int sdfs_unpack_blocks_sub(sdfs_handle* h, const void* packed, void* dst, const void* sub, int64_t outer, int64_t n_axis,
                           int64_t inner, int nblocks, const int64_t* offs, int elem_bytes) {
  int rc = check(h); if (rc) return rc;
  if (!packed || !dst || !sub || !offs) return fail(h, SDFS_ERR_ARG, "NULL argument");
  if (nblocks < 1) return fail(h, SDFS_ERR_ARG, "at least one block");
  if (nblocks > PACK_MAX_BLOCKS) return fail(h, SDFS_ERR_UNSUPPORTED, "pack: at most %d blocks", PACK_MAX_BLOCKS);
  if (elem_bytes != 8 && elem_bytes != 4) return fail(h, SDFS_ERR_ARG, "elements of 4 or 8 bytes");
  if (outer < 1 || n_axis < 1 || inner < 1 || offs[0] != 0 || offs[nblocks] != n_axis) return fail(h, SDFS_ERR_ARG, "bad block table");
  PackBlocks B;
  memset(&B, 0, sizeof B);
  B.n = nblocks;
  for (int j = 0; j <= nblocks; ++j) {
    if (j > 0 && offs[j] <= offs[j - 1]) return fail(h, SDFS_ERR_ARG, "empty or unordered block");
    B.off[j] = (unsigned)offs[j];
  }
  const long long run_bytes = (long long)inner * elem_bytes;
  const bool wide = run_bytes % 16 == 0 && ((uintptr_t)packed % 16) == 0 && ((uintptr_t)dst % 16) == 0 && ((uintptr_t)sub % 16) == 0;
  const int ub = wide ? 16 : elem_bytes;
  const long long innerU = run_bytes / ub;
  const long long total = outer * n_axis * innerU;
  if (total >= (1LL << 31)) return fail(h, SDFS_ERR_UNSUPPORTED, "pack: more than 2^31 units");
  const unsigned grid = (unsigned)std::min<long long>((total + VEC_BLOCK - 1) / VEC_BLOCK, 8192);
#define SDFS_UNPACK_SUB(U)                                                                                               \
  hipLaunchKernelGGL((k_pack_blocks<U, true, true>), dim3(grid), dim3(VEC_BLOCK), 0, h->stream, (const U*)packed, (U*)dst,     \
                     (unsigned)outer, (unsigned)n_axis, (unsigned)innerU, B, (const U*)sub)
  if (ub == 16 && elem_bytes == 8) SDFS_UNPACK_SUB(double2);
  else if (ub == 16) SDFS_UNPACK_SUB(float4);
  else if (ub == 8) SDFS_UNPACK_SUB(double);
  else SDFS_UNPACK_SUB(float);
#undef SDFS_UNPACK_SUB
  HIPCHK(h, hipGetLastError());
  return 0;
}

static int ensure_bicg_gate(sdfs_handle* h) {
  if (!h->bicg_gate) {
    HIPCHK(h, hipMalloc((void**)&h->bicg_gate, 64));
    h->misc_allocs.push_back(h->bicg_gate);
    HIPCHK(h, hipHostMalloc((void**)&h->bicg_gate_host, 64));
  }
  return 0;
}

int sdfs_krylov_gate(sdfs_handle* h, const void** gate_dev) {
  int rc = check(h); if (rc) return rc;
  if (!gate_dev) return fail(h, SDFS_ERR_ARG, "NULL pointer");
  if ((rc = ensure_bicg_gate(h))) return rc;
  *gate_dev = h->bicg_gate;
  return 0;
}

int sdfs_krylov_step(sdfs_handle* h, int step, int64_t n, int f32, void* const* v, double* sums_dev, double rtol, double atol) {
  int rc = check(h); if (rc) return rc;
  if (!v || !sums_dev || n < 1) return fail(h, SDFS_ERR_ARG, "bad argument");
  if ((rc = ensure_scalars(h))) return rc;
  if ((step & SDFS_KS_GATED) && (rc = ensure_bicg_gate(h))) return rc;
  return f32 ? krylov_step_t<float>(h, step, (long long)n, v, sums_dev, rtol, atol)
             : krylov_step_t<double>(h, step, (long long)n, v, sums_dev, rtol, atol);
}

int sdfs_set_krylov_f32(sdfs_handle* h, int on, double w_ref) {
  int rc = check(h); if (rc) return rc;
  if (!h->sharded) return fail(h, SDFS_ERR_ARG, "sdfs_set_krylov_f32 is for sharded handles (opts.krylov_f32 otherwise)");
  if (on && !(w_ref > 0.0 && std::isfinite(w_ref))) return fail(h, SDFS_ERR_ARG, "reference value must be positive and finite");
  h->stage_f32 = on != 0;
  h->lin_ref = on ? w_ref : 0.0;
  return 0;
}

int sdfs_set_t_f32(sdfs_handle* h, int on, double w_ref) {
  int rc = check(h); if (rc) return rc;
  if (!h->sharded) return fail(h, SDFS_ERR_ARG, "sdfs_set_t_f32 is for sharded handles (opts.t_f32 otherwise)");
  if (!h->sfast[0].ok || !h->sfast[1].ok) return fail(h, SDFS_ERR_UNSUPPORTED, "fp32 intermediates need the stages on the pair plan's kernels");
  for (int st = 0; st < 2; ++st)
    for (const FastPass& P : h->sfast[st].passes)
      if (P.line && P.ld.lrest % LINE_R != 0) return fail(h, SDFS_ERR_UNSUPPORTED, "fp32 intermediates need whole 16-element chunks in every line pass");
  if (on && !(w_ref > 0.0 && std::isfinite(w_ref))) return fail(h, SDFS_ERR_ARG, "reference value must be positive and finite");
  h->stage_t32 = on != 0;
  h->t32_ref = on ? w_ref : 0.0;
  return 0;
}

int sdfs_krylov_scalars(sdfs_handle* h, double* out) {
  int rc = check(h); if (rc) return rc;
  if (!out) return fail(h, SDFS_ERR_ARG, "NULL pointer");
  if ((rc = ensure_scalars(h))) return rc;
  HIPCHK(h, hipMemcpyAsync(h->sc_host, h->sc, sizeof(double) * SC_COUNT, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  memcpy(out, h->sc_host, sizeof(double) * SC_COUNT);
  return 0;
}

int sdfs_set_profiling(sdfs_handle* h, int on) {
  if (!h) return SDFS_ERR_ARG;
  int rc = drain_events(h); if (rc) return rc;
  h->profiling = on != 0;
  // events are created here, not inside a timed region: enough for ~340 launches between two drains
  while (on && h->event_pool.size() < 2048) {
    hipEvent_t e;
    HIPCHK(h, hipEventCreate(&e));
    h->event_pool.push_back(e);
  }
  return 0;
}

int sdfs_reset_counters(sdfs_handle* h) {
  if (!h) return SDFS_ERR_ARG;
  int rc = drain_events(h); if (rc) return rc;
  for (int i = 0; i < h->counters.nkernels; ++i) { h->counters.k[i].launches = 0; h->counters.k[i].total_ms = 0; }
  return 0;
}

int sdfs_get_counters(sdfs_handle* h, sdfs_counters* out) {
  if (!h || !out) return SDFS_ERR_ARG;
  int rc = check(h); if (rc) return rc;
  if ((rc = drain_events(h))) return rc;
  *out = h->counters;
  return 0;
}

int sdfs_debug_pow(const double* x_host, double y, double* out_host, int64_t n, int device_id) {
  return sdfs_debug_powy(x_host, y, out_host, n, 0, device_id);
}

int sdfs_debug_powy(const double* x_host, double y, double* out_host, int64_t n, int degree, int device_id) {
  if (!x_host || !out_host || n < 1 || (degree != 0 && degree != 6 && degree != 7)) return SDFS_ERR_ARG;
  if (hipSetDevice(device_id) != hipSuccess) return fail(nullptr, SDFS_ERR_HIP, "hipSetDevice failed");
  double *dx = nullptr, *dy = nullptr;
  if (hipMalloc((void**)&dx, 8 * (size_t)n) != hipSuccess || hipMalloc((void**)&dy, 8 * (size_t)n) != hipSuccess)
    return fail(nullptr, SDFS_ERR_HIP, "hipMalloc failed");
  hipMemcpy(dx, x_host, 8 * (size_t)n, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(debug_pow_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, y, dy, (long long)n, degree);
  hipError_t e = hipMemcpy(out_host, dy, 8 * (size_t)n, hipMemcpyDeviceToHost);
  hipFree(dx); hipFree(dy);
  return e == hipSuccess ? 0 : fail(nullptr, SDFS_ERR_HIP, "debug_pow: %s", hipGetErrorString(e));
}

int sdfs_debug_jvp_storage_dev(sdfs_handle* h, int krylov_f32, const double* w_dev, const void* v_dev, void* out_dev,
                               int minus_identity) {
  int rc = check(h); if (rc) return rc;
  if (!w_dev || !v_dev || !out_dev) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  if (krylov_f32 < 0 || krylov_f32 > 3) return fail(h, SDFS_ERR_ARG, "krylov_f32 = %d: 0, 1, 2 or 3", krylov_f32);
  if (krylov_f32 != 0 && (h->cont || h->dense || h->sharded))
    return fail(h, SDFS_ERR_UNSUPPORTED, "reduced-precision J.v storage exists for unsharded discretised handles only");
  if (h->sharded) return fail(h, SDFS_ERR_ARG, "sharded handle: use sdfs_apply_stage_dev");
  if ((rc = ensure_buf(h, &h->hostio3))) return rc;
  // the storage solve_newton's inner solve uses for opts.krylov_f32 (PREC_* = opts.krylov_f32 for 0 ... 3)
  Apply lin(MODE_T_LIN, w_dev, h->hostio3, w_dev);
  lin.prec = krylov_f32;
  Apply jv(MODE_JVP, (const double*)v_dev, (double*)out_dev, (const double*)v_dev);
  jv.prec = krylov_f32; jv.minus_identity = minus_identity;
  // from here on c1 / c2 may hold scaled floats: an fp64 J.v must relinearise first
  if (krylov_f32 != 0) h->lin_stale = true;
  if ((rc = apply(h, lin))) return rc;
  if (krylov_f32 == 0) h->lin_stale = false;
  return apply(h, jv);
}

int sdfs_describe_plan(const sdfs_handle* h, char* buf, int64_t cap) {
  if (!h || !buf || cap < 1) return SDFS_ERR_ARG;
  std::string s;
  char line[384];
  if (h->dense) {
    snprintf(line, sizeof line, "dense single-index operator: N = %lld, one GEMV (8 N^2 = %.3g bytes) per application\n",
             h->N, 8.0 * (double)h->N * (double)h->N);
    s += line;
  }
  if (h->cont) {
    // cap / ucap / tq (0 = no pre-contraction) and the dynamic LDS are what launch_cont asks for
    const size_t lds = (size_t)(h->cd.cap + h->cd.ucap) * sizeof(double);
    snprintf(line, sizeof line, "continuous operator: %d-D grid of %lld points x %d nodes, one 256-thread block per point, "
             "%d-corner multilinear gather + pow per node, cap %d, ucap %d, tq %d, dynamic LDS %zu B (T) / %zu B (J.v)\n",
             h->cd.D, h->cd.N, h->cd.M, 1 << h->cd.D, h->cd.cap, h->cd.ucap, h->cd.tq, lds, 2 * lds);
    s += line;
  }
  if (h->fast.ok) {
    for (size_t i = 0; i < h->fast.passes.size(); ++i) {
      const FastPass& P = h->fast.passes[i];
      int occ = -1;
      if (P.pad) {
        snprintf(line, sizeof line, "padded pair plan pass %zu: %s %s\n", i, P.label.c_str(),
                 P.line ? (std::string("tiles ") + std::to_string(P.pd.ntiles) + " (rows of " + std::to_string(pad_line_r(P.nt)) + " positions, real strides)").c_str()
                        : (std::string("wave tiles ") + std::to_string((P.pd.nslices + pad_slice_g(P.nt) - 1) / pad_slice_g(P.nt)) + " of " +
                           std::to_string(pad_slice_g(P.nt)) + " slice(s)").c_str());
      } else if (P.small) {
        snprintf(line, sizeof line, "small-grid plan pass %zu: %s %d wave%s per tile, run %d, tiles %lld, workgroups %u\n", i,
                 P.label.c_str(), P.wpt, P.wpt == 1 ? "" : "s", P.r, P.sm.ntiles, small_grid(P.sm, P.wpt));
      } else if (!P.line) {
        // (the first pass of T)
        const PassLaunch L = select_pass(h, &h->fast, h->plan[0], (int)i, h->N, true, true, Apply(MODE_T, nullptr, nullptr, nullptr));
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, L.fn, L.block, L.lds);
        const long long nt = (P.sd.nslices + slice_tile_slices(P.n, S_TFIRST) - 1) / slice_tile_slices(P.n, S_TFIRST);
        snprintf(line, sizeof line, "pair plan pass %zu: %s lds %zu B block 256 (4 wave tiles) wave-tiles %lld blocks/CU %d\n", i,
                 P.label.c_str(), L.lds, nt, occ);
      } else {
        // (the occupancy of the plain middle form, one tile per workgroup)
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)line_variant(P.n, L_MID, P.ld.lrest % LINE_R == 0), line_block(P.n), line_lds_bytes(P.n));
        snprintf(line, sizeof line, "pair plan pass %zu: %s lds %zu B block %d tiles %lld (outer %lld x %d chunks of 128 B) %s grid %u blocks/CU %d\n", i,
                 P.label.c_str(), line_lds_bytes(P.n), line_block(P.n), P.ld.ntiles, P.ld.nouter, P.ld.nchunks,
                 P.stream == 3 ? (line_stream_early_side(P.n) ? "streamed (middle pass: persistent, next tile in flight; T's last pass: side stream in flight with the tile where it is read)"
                                                              : "streamed (middle pass: persistent, next tile in flight; T's last pass: side stream loaded early)") :
                 P.stream == 1 ? "streamed as a middle pass (persistent, next tile in flight)" :
                 P.stream == 2 ? (line_stream_early_side(P.n) ? "streamed as T's last pass (side stream in flight with the tile where it is read)"
                                                              : "streamed as T's last pass (side stream loaded early)") : "one tile per workgroup",
                 (unsigned)P.ld.ntiles, occ);
      }
      s += line;
    }
    if (h->fast.small && anderson_fused_ok(h, 10))
      s += "small-grid plan, Anderson: passes in reverse order, push on the last pass, control step + update of x on the first\n";
    // the fp32 J.v forms of each pass (opts.krylov_f32 = 1 / 2: fp32 streams on the fp64 tile; 3: the fp32-MFMA kernel
    // select_pass picks, with its row width and, for a middle pass, whether it runs persistent)
    Apply m32(MODE_JVP, nullptr, nullptr, nullptr);
    m32.prec = PREC_MFMA32; m32.minus_identity = 1;
    for (size_t i = 0; i < h->fast.passes.size() && h->fast.f32_ok && !h->fast.small && !h->fast.pad; ++i) {
      const FastPass& P = h->fast.passes[i];
      const bool last = i + 1 == h->fast.passes.size();
      const PassLaunch L = select_pass(h, &h->fast, h->plan[0], (int)i, h->N, true, true, m32);
      if (!P.line) {
        snprintf(line, sizeof line, "pair plan pass %zu fp32: %s mfma32 %s\n", i, P.label.c_str(), L.fn ? "slice32" : "none");
      } else {
        snprintf(line, sizeof line, "pair plan pass %zu fp32: %s mfma32 %s row %d floats %s\n", i, P.label.c_str(),
                 L.fn ? "line32" : "none", line32_row_floats(P.n, P.ld.lrest),
                 last ? "last pass" : L.persistent ? "persistent middle pass" : "one tile per workgroup");
      }
      s += line;
    }
    if (!h->fast.f32_ok || h->fast.small || h->fast.pad) s += "pair plan fp32: none (fp32 Krylov storage on the generic plan)\n";
    s += "generic plan (fp32 Krylov storage, sharded stages):\n";
  }
  if (h->sharded && h->sfast[0].ok) {
    for (int st = 0; st < 2; ++st)
      for (size_t i = 0; i < h->sfast[st].passes.size(); ++i) {
        const FastPass& P = h->sfast[st].passes[i];
        if (!P.line) {
          const long long nt = (P.sd.nslices + slice_tile_slices(P.n, S_TFIRST) - 1) / slice_tile_slices(P.n, S_TFIRST);
          snprintf(line, sizeof line, "stage %d pair-plan pass %zu: %s wave-tiles %lld\n", st, i, P.label.c_str(), nt);
        } else {
          snprintf(line, sizeof line, "stage %d pair-plan pass %zu: %s tiles %lld (outer %lld x %d chunks of 128 B)%s\n", st, i, P.label.c_str(),
                   P.ld.ntiles, P.ld.nouter, P.ld.nchunks, P.stream ? " streamed" : "");
        }
        s += line;
      }
    s += "generic stage plans (fp32 Krylov storage):\n";
  }
  for (int st = 0; st < 2; ++st) {
    const Plan& pl = h->plan[st];
    for (size_t i = 0; i < pl.passes.size(); ++i) {
      const Pass& P = pl.passes[i];
      int occ = -1;
      // (the middle form on aligned fp64 streams)
      const PassLaunch L = select_pass(h, nullptr, pl, (int)i, pl.nloc, false, false, Apply(MODE_T, nullptr, nullptr, nullptr));
      const TileForm tf = tile_form(P, true, false);
      pass_fn fn = pass_kernel_variant(tf.ept, tf.vec, L.kmode);
      if (fn) hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)fn, L.block, L.lds);
      snprintf(line, sizeof line, "stage %d pass %zu: %s tile %dx%dx%d lds %zu B block %d vec %d ept %d tiles %lld blocks/CU %d\n", st, i,
               P.label.c_str(), P.d.m[0], P.d.m[1], P.d.m[2], L.lds, L.block, tf.vec, tf.ept, (long long)L.grid, occ);
      s += line;
    }
  }
  snprintf(buf, (size_t)cap, "%s", s.c_str());
  return 0;
}

}  // extern "C"

#include "cont_sim.hpp"    // continuous-state paths (sdfs_cont_sdf_mean_dev, sdfs_cont_sim_*), built on the definitions above
#include "cont_price.hpp"  // continuous-state pricing (sdfs_cont_set_tilt_dev ... sdfs_cont_tilted_horizons_dev), likewise
#include "cont_sens.hpp"   // continuous-state parameter tangent (sdfs_cont_param_tangent_dev), likewise
#include "cont_adjoint.hpp"   // continuous-state J^T u and adjoint solve (sdfs_cont_apply_vjp_dev, sdfs_cont_solve_adjoint_dev), likewise
#include "batch_api.hpp"   // the batch API (sdfs_batch_*), built on the definitions above

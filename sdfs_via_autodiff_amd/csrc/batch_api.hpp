// batch_api.hpp -- host side of the batch API of include/sdfs_hip.h (sdfs_batch_*): B parameter vectors of one model on
// one grid shape, one workgroup per problem (batch_kernels.hpp, batch_newton.hpp, batch_adjoint.hpp, batch_price.hpp,
// batch_sim.hpp).
//
// Not a header of its own: sdfs_api.hip includes it once, as its last line, after the single-problem API.  It uses
// fill_model, ModelTables, read_knobs, g_create_error and sdfs_handle of that file, and its includes.
struct sdfs_batch {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  int model = 0, B = 0, num_cus = 256;
  BatchDesc d;
  BatchDesc* d_dev = nullptr;    // the kernel reads it from device memory
  batch_fn fn = nullptr;
  int nt = 0, k = 0;
  size_t lds_bytes = 0;
  double* tab = nullptr;         // [B][tabwords]
  double* scal = nullptr;        // [B][4]
  int* status = nullptr;         // [B]
  long long* it = nullptr;       // [B]
  double* err = nullptr;         // [B]
  int* status_host = nullptr;    // pinned
  // Newton-Krylov (batch_newton.hpp); the workspace is allocated at the first Newton solve
  batch_newton_fn nfn = nullptr;
  int newton_reg = 0;            // 1: the eight vectors live in registers, 0: in global memory
  long long ws_max = BATCH_NEWTON_WS_MAX;   // bytes the workspace of a group may take (SDFS_BATCH_WS_MAX at sdfs_batch_create)
  int ws_slots = 0;              // problems per group: the workspace holds this many
  double* ws = nullptr;          // [ws_slots][7][nwork]
  BatchNewtonState* nst = nullptr;   // [B]
  // adjoint moments (batch_adjoint.hpp): the Newton workspace, its own state; a2 is uploaded at the first gradient call
  batch_adjoint_fn afn = nullptr;
  int adjoint_reg = 0;
  int ax_lam = 0, ax_c = 0, na3 = 0;
  std::vector<double> a2_host;   // [B][n_c]: a2 = exp((1/2) ((1 - gamma) sigma_c)^2), as fill_model folds it into Q_c
  double* a2 = nullptr;          // [B][n_c]
  BatchAdjointState* ast = nullptr;  // [B]
  // pricing (batch_price.hpp): the Newton workspace, its own state; host copies of what the tilt tables are built from
  batch_price_fn pfn = nullptr;
  int price_reg = 0;
  std::vector<double> hlam_host;  // [B][n_lam]: h_lambda
  std::vector<double> sigc_host;  // [B][n_c]: sigma_c
  std::vector<double> muz_host;   // [B][na3]: mu_c + z in the a3 layout
  std::vector<double> gam_host, theta_host;   // [B]
  BatchPriceState* pst = nullptr;    // [B]
  // simulation (batch_sim.hpp): per-call tables staged on the host, device buffers that only grow
  std::vector<double> beta_host;  // [B]
  std::vector<double> sim_tab_host, sim_scal_host;
  std::vector<int> sim_skip_host;
  double* sim_zt = nullptr;       // [B][na3]: mu_c + z in the a3 layout
  double* sim_tab = nullptr;      // [B][simwords]
  double* sim_scal = nullptr;     // [B][4]: theta, theta ln beta, gamma, kappa
  int* sim_skip = nullptr;        // [B]
  double* sim_part = nullptr;     // [B][3 nser + 1][workgroups][3]
  size_t sim_part_cap = 0;        // doubles
  hipEvent_t sim_staged = nullptr; // recorded behind the uploads of a call: the next call waits for it before it restages
  std::string errmsg;
};

namespace {

int bfail(sdfs_batch* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->errmsg = buf; else g_create_error = buf;
  return code;
}
#define BHIPCHK(h, call)                                                                    \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return bfail((h), SDFS_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                   __FILE__, __LINE__);                                                     \
  } while (0)

// What the batch code needs to know of a model beyond its grid: the axes of h_lambda and sigma_c, the entries of the a3
// table and the length of a parameter vector (ssy_model.py:81, gcy_model.py:72-75).
struct BatchModelConsts { int ax_lam, ax_c, na3, nparams; };

BatchModelConsts batch_model_consts(int model, const BatchDesc& d) {
  const bool ssy = model == SDFS_MODEL_SSY;
  BatchModelConsts c{ssy ? 0 : 5, ssy ? 1 : 3, 1, ssy ? 13 : 18};
  for (int a = 0; a < d.ndim; ++a) if (d.a3s[a] != 0) c.na3 *= d.n[a];
  return c;
}

// Geometry of the batch plan for one shape and the model's constants on it; *lds = the dynamic LDS of a workgroup.  A
// refusal leaves its reason in g_create_error.  Host only.
int batch_geometry(int model, int ndim, const int64_t* shapes, BatchDesc& d, BatchModelConsts& c, long long* lds) {
  auto no = [&](int code, const char* fmt, long long a, long long b) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b);
    g_create_error = buf;
    return code;
  };
  if (!shapes) return no(SDFS_ERR_ARG, "shapes is NULL", 0, 0);
  if (!((model == SDFS_MODEL_SSY && ndim == 4) || (model == SDFS_MODEL_GCY && ndim == 6)))
    return no(SDFS_ERR_ARG, "model %lld with ndim %lld: SSY needs 4 axes, GCY 6", model, ndim);
  memset(&d, 0, sizeof d);
  long long N = 1;
  for (int a = 0; a < ndim; ++a) {
    if (shapes[a] < 2) return no(SDFS_ERR_ARG, "shapes[%lld] = %lld: every axis needs >= 2 states", a, shapes[a]);
    if (shapes[a] > MAXN) return no(SDFS_ERR_UNSUPPORTED, "shapes[%lld] = %lld exceeds the longest axis of the library", a, shapes[a]);
    N *= shapes[a];
    if (N * 8 > BATCH_LDS_MAX) return no(SDFS_ERR_UNSUPPORTED, "the grid does not fit the %lld bytes of LDS of one CU (axis %lld)", BATCH_LDS_MAX, a);
  }
  d.ndim = ndim; d.N = (int)N; d.nwork = (int)((N + 1) & ~1LL);
  int off = 0;
  long long st = N;
  for (int a = 0; a < ndim; ++a) {
    d.n[a] = (int)shapes[a];
    st /= shapes[a];
    d.stride[a] = (int)st;
    d.np[a] = batch_row_class(d.n[a]);
    d.qoff[a] = off;
    off += d.n[a] * d.np[a];
  }
  if (model == SDFS_MODEL_SSY) {       // a3[i, j] over (h_z, z)
    d.a3s[2] = d.n[3]; d.a3s[3] = 1;
  } else {                             // a3[b, c, e, a] over (z_pi, h_z, h_zpi, z)
    d.a3s[0] = 1; d.a3s[4] = d.n[0]; d.a3s[2] = d.n[4] * d.n[0]; d.a3s[1] = d.n[2] * d.n[4] * d.n[0];
  }
  c = batch_model_consts(model, d);
  d.a3off = off;
  d.tabwords = (off + c.na3 + 1) & ~1;
  const long long bytes = 8LL * ((long long)d.nwork + d.tabwords + BATCH_RED);
  if (bytes > BATCH_LDS_MAX)
    return no(SDFS_ERR_UNSUPPORTED, "grid and tables need %lld bytes of LDS, one CU has %lld", bytes, BATCH_LDS_MAX);
  int nt, k;
  if (!batch_kernel_for(d.N, &nt, &k)) return no(SDFS_ERR_UNSUPPORTED, "no kernel for %lld points", N, 0);
  *lds = bytes;
  return 0;
}

// Member b of a stacked family (array i: [B][array_sizes[i]], params: [B][nparams]) through the host code of sdfs_create
// (fill_model), and the fields the adjoint's a2, the pricing tilts and the simulation tables are built from (sdfs_set_tilt_dev
// reads the same fields of a single-problem handle), written to row b of `out`.  The findings are reported, not worded:
// sdfs_batch_create and sdfs_batch_sim_tables each keep their own messages.
struct BatchMember {
  sdfs_handle hh;                // host fields only: fill_model touches no device
  ModelTables M;
  int bad_array = -1;            // arrays[bad_array] is NULL or has a negative size: fill_model did not run
  int rc = 0;                    // fill_model's code (hh.err has its text)
  bool sizes_ok = false;         // h_lambda, sigma_c and z have the extents of their axes; only then is `out` written
};
struct BatchFields { double *hlam, *sigc, *muz, *theta, *beta, *gamma; };   // [B][n_lam], [B][n_c], [B][na3] (mu_c + z; may be NULL), [B] each

bool batch_member_fields(BatchMember& m, int model, int ndim, const int64_t* shapes, const BatchDesc& d, const BatchModelConsts& c,
                         int64_t b, const double* params, const double* const* arrays, const int64_t* array_sizes, int narrays,
                         const BatchFields& out) {
  m.hh.knobs = read_knobs();
  const double* arr[32];
  for (int i = 0; i < narrays; ++i) {
    if (!arrays[i] || array_sizes[i] < 0) { m.bad_array = i; return false; }
    arr[i] = arrays[i] + (size_t)b * (size_t)array_sizes[i];
  }
  m.rc = fill_model(&m.hh, model, ndim, shapes, params + (size_t)b * c.nparams, c.nparams, arr, array_sizes, narrays, m.M);
  if (m.rc) return false;
  const auto& s = m.hh.sens;
  const int nl = d.n[c.ax_lam], nc = d.n[c.ax_c];
  m.sizes_ok = (int)s.hlam.size() == nl && (int)s.sigc.size() == nc && (int)s.z.size() == c.na3;
  if (!m.sizes_ok) return false;
  std::copy(s.hlam.begin(), s.hlam.end(), out.hlam + (size_t)b * nl);
  std::copy(s.sigc.begin(), s.sigc.end(), out.sigc + (size_t)b * nc);
  if (out.muz)
    for (int i = 0; i < c.na3; ++i) out.muz[(size_t)b * c.na3 + i] = s.mu_c + s.z[i];
  out.theta[b] = m.hh.theta; out.beta[b] = m.hh.beta; out.gamma[b] = s.gamma;
  return true;
}

int bcheck(sdfs_batch* h) {
  if (!h) return SDFS_ERR_ARG;
  if (hipSetDevice(h->device) != hipSuccess) return bfail(h, SDFS_ERR_HIP, "hipSetDevice failed");
  return 0;
}

// Dynamic LDS above 64 KB has to be allowed per kernel and device; the attribute is the kernel's, not the handle's, so
// the grant only ever grows.  Every batch kernel asks here before its first launch, whatever its size.
int batch_allow_lds(sdfs_batch* h, const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> allowed;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = allowed[{fn, h->device}];
  if (bytes > have) {
    BHIPCHK(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    have = bytes;
  }
  return 0;
}

int batch_launch(sdfs_batch* h, const BatchArgs& A) {
  hipLaunchKernelGGL(h->fn, dim3(h->B), dim3(h->nt), h->lds_bytes, h->stream, (const BatchDesc*)h->d_dev, A);
  BHIPCHK(h, hipGetLastError());
  return 0;
}

// Iterations per launch when the caller leaves the choice to the library: a launch is to stay near 0.05 s (never
// above about 0.1 s).  An iteration of one workgroup was measured at 5.5 us (SSY 5^4), 35 us (SSY 10^4) and 62 us
// (GCY 5^6): about 3 us plus 3.8 ns per grid point (profiles/batch_times.txt); a batch beyond the CU count runs in rounds.
int batch_default_chunk(const sdfs_batch* h) {
  const double t_iter = 3e-6 + 3.8e-9 * h->d.N;
  const double rounds = (double)((h->B + h->num_cus - 1) / h->num_cus);
  const double c = 0.05 / (t_iter * rounds);
  return (int)std::min(4096.0, std::max(64.0, c));
}

// SDFS_BATCH_WS_MAX: bytes the workspace of a group may take; unset, empty or < 1: BATCH_NEWTON_WS_MAX
long long batch_ws_max() {
  const char* s = getenv("SDFS_BATCH_WS_MAX");
  const long long v = (s && *s) ? atoll(s) : 0;
  return v < 1 ? BATCH_NEWTON_WS_MAX : v;
}

// problems per group of a Newton solve: the workspace of a group stays within the handle's ws_max
int batch_newton_slots(const sdfs_batch* h) {
  const long long per = 8LL * BATCH_NEWTON_VECS * h->d.nwork;
  return (int)std::min<long long>(h->B, std::max<long long>(1, h->ws_max / per));
}

// Applications per launch of the Newton kernel when the caller leaves the choice to the library: a J.v is taken at the
// cost of an SA iteration (it has the contractions but no power; the vector updates take their place), so the launch
// stays near 0.05 s as on the SA path.
int batch_newton_default_budget(const sdfs_batch* h) {
  const double t_app = 3e-6 + 3.8e-9 * h->d.N;
  const int slots = batch_newton_slots(h);
  const double rounds = (double)((slots + h->num_cus - 1) / h->num_cus);
  return (int)std::min(4096.0, std::max(64.0, 0.05 / (t_app * rounds)));
}

// The inner (BiCGSTAB) options of the Newton, adjoint and pricing solves: checked, then in the form the kernels take.
struct BatchInner { double rtol2, atol2; long long inner_max; int budget; };

int batch_check_inner(sdfs_batch* h, const sdfs_opts* o, const char* what, BatchInner& in) {
  if (!(o->inner_rtol >= 0.0) || !(o->inner_atol >= 0.0)) return bfail(h, SDFS_ERR_ARG, "inner_rtol and inner_atol must be >= 0");
  if (o->inner_max_iter < 0) return bfail(h, SDFS_ERR_ARG, "inner_max_iter must be >= 0");
  if (o->krylov_f32 != 0) return bfail(h, SDFS_ERR_ARG, "the batch %s solve keeps its Krylov vectors in fp64: krylov_f32 must be 0", what);
  in.rtol2 = o->inner_rtol * o->inner_rtol; in.atol2 = o->inner_atol * o->inner_atol;
  in.inner_max = o->inner_max_iter > 0 ? (long long)o->inner_max_iter : 10LL * h->d.N;
  in.budget = o->check_every > 0 ? (int)o->check_every : batch_newton_default_budget(h);
  return 0;
}

// workspace, state and the LDS attribute of the Newton kernel, at the first Newton solve of the handle
int batch_newton_prepare(sdfs_batch* h) {
  if (h->ws) return 0;
  if (!h->nfn) return bfail(h, SDFS_ERR_UNSUPPORTED, "no Newton kernel for %d points", h->d.N);
  int rc = batch_allow_lds(h, (const void*)h->nfn, h->lds_bytes);
  if (rc) return rc;
  const int slots = batch_newton_slots(h);
  if (!h->nst) BHIPCHK(h, hipMalloc((void**)&h->nst, (size_t)h->B * sizeof(BatchNewtonState)));
  BHIPCHK(h, hipMalloc((void**)&h->ws, (size_t)slots * BATCH_NEWTON_VECS * h->d.nwork * 8));
  h->ws_slots = slots;
  return 0;
}

int batch_adjoint_words(const sdfs_batch* h) { return 3 + h->d.ndim + h->d.n[h->ax_lam] + h->d.n[h->ax_c] + h->na3; }

// the Newton workspace (the same seven vectors), the state, the a2 table and the LDS attribute of the adjoint kernel, at
// the first gradient call of the handle
int batch_adjoint_prepare(sdfs_batch* h) {
  if (h->ast) return 0;
  if (!h->afn) return bfail(h, SDFS_ERR_UNSUPPORTED, "no adjoint kernel for %d points", h->d.N);
  int rc = batch_newton_prepare(h);
  if (rc || (rc = batch_allow_lds(h, (const void*)h->afn, h->lds_bytes))) return rc;
  if (!h->a2) {
    BHIPCHK(h, hipMalloc((void**)&h->a2, h->a2_host.size() * 8));
    BHIPCHK(h, hipMemcpy(h->a2, h->a2_host.data(), h->a2_host.size() * 8, hipMemcpyHostToDevice));
  }
  BHIPCHK(h, hipMalloc((void**)&h->ast, (size_t)h->B * sizeof(BatchAdjointState)));
  return 0;
}

// the Newton workspace (the same seven vectors), the state and the LDS attribute of the pricing kernel, at the first
// pricing call of the handle
int batch_price_prepare(sdfs_batch* h) {
  if (h->pst) return 0;
  if (!h->pfn) return bfail(h, SDFS_ERR_UNSUPPORTED, "no pricing kernel for %d points", h->d.N);
  int rc = batch_newton_prepare(h);
  if (rc || (rc = batch_allow_lds(h, (const void*)h->pfn, h->lds_bytes))) return rc;
  BHIPCHK(h, hipMalloc((void**)&h->pst, (size_t)h->B * sizeof(BatchPriceState)));
  return 0;
}

// Problems B_first ... B_end - 1 through the kernel `fn` of the Newton family, group after group (one group unless the
// workspace would pass the handle's ws_max): workgroup i of a group runs problem A.b0 + i in slot i of the workspace.  Every
// launch is bounded by A.budget >= 1 applications per problem, the host reads the group's status words per launch, and
// every application moves its problem on within the finite counts of its kernel, so the loop ends.
template <class Fn, class Args>
int batch_run_groups(sdfs_batch* h, Fn fn, Args& A, int B_first, int B_end) {
  hipStream_t st = h->stream;
  for (int b0 = B_first; b0 < B_end; b0 += h->ws_slots) {
    const int G = std::min(h->ws_slots, B_end - b0);
    A.b0 = b0;
    bool open = true;
    while (open) {
      hipLaunchKernelGGL(fn, dim3(G), dim3(h->nt), h->lds_bytes, st, (const BatchDesc*)h->d_dev, A);
      BHIPCHK(h, hipGetLastError());
      BHIPCHK(h, hipMemcpyAsync(h->status_host + b0, h->status + b0, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, st));
      BHIPCHK(h, hipStreamSynchronize(st));
      open = false;
      for (int b = b0; b < b0 + G && !open; ++b) open = h->status_host[b] == BATCH_OPEN;
    }
  }
  return 0;
}

struct BatchDevBuf {                 // device memory of one call
  double* p = nullptr;
  ~BatchDevBuf() { if (p) hipFree(p); }
};

}  // namespace

extern "C" {

int64_t sdfs_batch_lds_bytes(int model, int ndim, const int64_t* shapes) {
  BatchDesc d;
  BatchModelConsts c;
  long long lds = 0;
  const int rc = batch_geometry(model, ndim, shapes, d, c, &lds);
  return rc ? rc : lds;
}

void sdfs_batch_destroy(sdfs_batch* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->tab, (void*)h->d_dev, (void*)h->scal, (void*)h->status, (void*)h->it, (void*)h->err})
    if (p) hipFree(p);
  if (h->status_host) hipHostFree(h->status_host);
  for (void* p : {(void*)h->ws, (void*)h->nst, (void*)h->a2, (void*)h->ast, (void*)h->pst, (void*)h->sim_zt, (void*)h->sim_tab,
                  (void*)h->sim_scal, (void*)h->sim_skip, (void*)h->sim_part})
    if (p) hipFree(p);
  if (h->sim_staged) hipEventDestroy(h->sim_staged);
  if (h->own_stream) hipStreamDestroy(h->own_stream);
  delete h;
}

int sdfs_batch_create(int model, int ndim, const int64_t* shapes, int64_t B, const double* params,
                      const double* const* arrays, const int64_t* array_sizes, int narrays, int device_id,
                      sdfs_batch** out) {
  if (!out) return bfail(nullptr, SDFS_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (!shapes || !params || !arrays || !array_sizes) return bfail(nullptr, SDFS_ERR_ARG, "NULL argument");
  if (B < 1 || B > (1 << 20)) return bfail(nullptr, SDFS_ERR_ARG, "batch of %lld problems: need 1 .. 2^20", (long long)B);
  if (narrays < 1 || narrays > 32) return bfail(nullptr, SDFS_ERR_ARG, "narrays %d out of range", narrays);
  BatchDesc d;
  BatchModelConsts c;
  long long lds = 0;
  int rc = batch_geometry(model, ndim, shapes, d, c, &lds);
  if (rc) return rc;
  // the tables of every problem, by the host code of sdfs_create (fill_model), packed into the kernel's layout
  const int nl = d.n[c.ax_lam], nc = d.n[c.ax_c];
  std::vector<double> tab((size_t)B * d.tabwords, 0.0), scal((size_t)B * 4, 0.0);
  std::vector<double> a2h((size_t)B * nc, 0.0);
  std::vector<double> hlh((size_t)B * nl, 0.0), sch((size_t)B * nc, 0.0), muzh((size_t)B * c.na3, 0.0);
  std::vector<double> gamh((size_t)B, 0.0), thh((size_t)B, 0.0), beth((size_t)B, 0.0);
  for (int64_t b = 0; b < B; ++b) {
    BatchMember m;
    const sdfs_handle& hh = m.hh;
    const ModelTables& M = m.M;
    batch_member_fields(m, model, ndim, shapes, d, c, b, params, arrays, array_sizes, narrays,
                        {hlh.data(), sch.data(), muzh.data(), thh.data(), beth.data(), gamh.data()});
    if (m.bad_array >= 0) return bfail(nullptr, SDFS_ERR_ARG, "arrays[%d] is NULL", m.bad_array);
    if (m.rc) return bfail(nullptr, m.rc, "problem %lld: %s", (long long)b, hh.err.c_str());
    if (!M.keep_a3) return bfail(nullptr, SDFS_ERR_UNSUPPORTED, "problem %lld: conditional transition tensors are not supported by the batch plan", (long long)b);
    for (int a = 0; a < ndim; ++a)
      if (hh.ax[a].qcount != 1) return bfail(nullptr, SDFS_ERR_UNSUPPORTED, "problem %lld: conditional transition tensors are not supported by the batch plan", (long long)b);
    double* t = tab.data() + (size_t)b * d.tabwords;
    for (int a = 0; a < ndim; ++a)
      for (int r = 0; r < d.n[a]; ++r)
        for (int k = 0; k < d.n[a]; ++k) t[d.qoff[a] + r * d.np[a] + k] = M.q[a][(size_t)r * d.n[a] + k];
    if ((long long)M.a3.size() + d.a3off > d.tabwords) return bfail(nullptr, SDFS_ERR_ARG, "a3 table of %zu entries", M.a3.size());
    std::copy(M.a3.begin(), M.a3.end(), t + d.a3off);
    scal[4 * b] = hh.beta; scal[4 * b + 1] = hh.theta; scal[4 * b + 2] = 1.0 / hh.theta;
    for (int k = 0; k < nc; ++k) {                // a2 as fill_model forms it
      const double s = (1 - hh.sens.gamma) * hh.sens.sigc[k];
      a2h[(size_t)b * nc + k] = std::exp(0.5 * s * s);
    }
    if (!m.sizes_ok)
      return bfail(nullptr, SDFS_ERR_ARG, "problem %lld: state arrays of %zu, %zu and %zu entries", (long long)b, hh.sens.hlam.size(),
                   hh.sens.sigc.size(), hh.sens.z.size());
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return bfail(nullptr, SDFS_ERR_HIP, "no HIP device available (libsdfs_hip has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return bfail(nullptr, SDFS_ERR_ARG, "device_id %d out of range (%d devices)", device_id, ndev);
  sdfs_batch* h = new sdfs_batch();
  h->device = device_id; h->model = model; h->B = (int)B; h->d = d; h->lds_bytes = (size_t)lds;
  h->ws_max = batch_ws_max();
  h->fn = batch_kernel_for(d.N, &h->nt, &h->k);
  {
    int nt = 0, k = 0;
    h->nfn = batch_newton_kernel_for(d.N, &nt, &k, &h->newton_reg);     // the threads and points of h->fn
    h->afn = batch_adjoint_kernel_for(d.N, &nt, &k, &h->adjoint_reg);
    h->pfn = batch_price_kernel_for(d.N, &nt, &k, &h->price_reg);
  }
  h->ax_lam = c.ax_lam; h->ax_c = c.ax_c; h->na3 = c.na3;
  h->a2_host.swap(a2h);
  h->hlam_host.swap(hlh); h->sigc_host.swap(sch); h->muz_host.swap(muzh); h->gam_host.swap(gamh); h->theta_host.swap(thh); h->beta_host.swap(beth);
  auto bail = [&](int rc_) { g_create_error = h->errmsg; sdfs_batch_destroy(h); return rc_; };
  auto hip = [&](hipError_t e, const char* what) { return e == hipSuccess ? 0 : bfail(h, SDFS_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e)); };
  if ((rc = hip(hipSetDevice(device_id), "hipSetDevice"))) return bail(rc);
  if ((rc = hip(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking), "hipStreamCreate"))) return bail(rc);
  h->stream = h->own_stream;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) h->num_cus = prop.multiProcessorCount;
  }
  if ((rc = batch_allow_lds(h, (const void*)h->fn, h->lds_bytes))) return bail(rc);
  if ((rc = hip(hipMalloc((void**)&h->tab, tab.size() * 8), "hipMalloc")) || (rc = hip(hipMalloc((void**)&h->scal, scal.size() * 8), "hipMalloc")) ||
      (rc = hip(hipMalloc((void**)&h->status, (size_t)B * sizeof(int)), "hipMalloc")) ||
      (rc = hip(hipMalloc((void**)&h->it, (size_t)B * sizeof(long long)), "hipMalloc")) ||
      (rc = hip(hipMalloc((void**)&h->err, (size_t)B * 8), "hipMalloc")) ||
      (rc = hip(hipHostMalloc((void**)&h->status_host, (size_t)B * sizeof(int)), "hipHostMalloc")) ||
      (rc = hip(hipMalloc((void**)&h->d_dev, sizeof(BatchDesc)), "hipMalloc")) ||
      (rc = hip(hipMemcpy(h->d_dev, &h->d, sizeof(BatchDesc), hipMemcpyHostToDevice), "hipMemcpy")) ||
      (rc = hip(hipMemcpy(h->tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice), "hipMemcpy")) ||
      (rc = hip(hipMemcpy(h->scal, scal.data(), scal.size() * 8, hipMemcpyHostToDevice), "hipMemcpy")))
    return bail(rc);
  *out = h;
  return 0;
}

const char* sdfs_batch_last_error(const sdfs_batch* h) { return h ? h->errmsg.c_str() : g_create_error.c_str(); }

int sdfs_batch_set_stream(sdfs_batch* h, void* s, int use_own) {
  int rc = bcheck(h); if (rc) return rc;
  h->stream = use_own ? h->own_stream : (hipStream_t)s;
  return 0;
}

int sdfs_batch_synchronize(sdfs_batch* h) {
  int rc = bcheck(h); if (rc) return rc;
  BHIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int sdfs_batch_apply_T_dev(sdfs_batch* h, const double* w_dev, double* Tw_dev, double* resid_dev) {
  int rc = bcheck(h); if (rc) return rc;
  if (!w_dev || !Tw_dev) return bfail(h, SDFS_ERR_ARG, "NULL argument");
  BatchArgs A;
  memset(&A, 0, sizeof A);
  A.tab = h->tab; A.scal = h->scal; A.w_in = w_dev; A.w_out = Tw_dev; A.resid = resid_dev;
  A.tol = 0.0; A.max_iter = 1; A.chunk = 1; A.apply = 1;
  return batch_launch(h, A);
}

int sdfs_batch_solve_dev(sdfs_batch* h, const sdfs_opts* opts, double* w_inout_dev, int64_t* n_iter, double* final_err,
                         int32_t* status) {
  int rc = bcheck(h); if (rc) return rc;
  if (!opts || !w_inout_dev || !n_iter || !final_err || !status) return bfail(h, SDFS_ERR_ARG, "NULL argument");
  if (!(opts->tol >= 0.0)) return bfail(h, SDFS_ERR_ARG, "tol must be >= 0");
  const int B = h->B;
  hipStream_t st = h->stream;
  BatchArgs A;
  memset(&A, 0, sizeof A);
  A.tab = h->tab; A.scal = h->scal; A.w_in = w_inout_dev; A.w_out = w_inout_dev;
  A.status = h->status; A.it = h->it; A.err = h->err;
  A.tol = opts->tol; A.max_iter = opts->max_iter;
  A.chunk = opts->check_every > 0 ? (int)opts->check_every : batch_default_chunk(h);
  hipLaunchKernelGGL(batch_init_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, h->status, h->it, h->err, A.tol, (long long)A.max_iter);
  BHIPCHK(h, hipGetLastError());
  // every launch is bounded by A.chunk iterations per problem; the host reads B status words per launch
  bool open = opts->max_iter > 0;
  while (open) {
    if ((rc = batch_launch(h, A))) return rc;
    BHIPCHK(h, hipMemcpyAsync(h->status_host, h->status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    BHIPCHK(h, hipStreamSynchronize(st));
    open = false;
    for (int b = 0; b < B && !open; ++b) open = h->status_host[b] == BATCH_OPEN;
  }
  std::vector<long long> it((size_t)B);
  BHIPCHK(h, hipMemcpyAsync(it.data(), h->it, (size_t)B * sizeof(long long), hipMemcpyDeviceToHost, st));
  BHIPCHK(h, hipMemcpyAsync(final_err, h->err, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  BHIPCHK(h, hipMemcpyAsync(h->status_host, h->status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
  BHIPCHK(h, hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) { n_iter[b] = it[b]; status[b] = h->status_host[b]; }
  return 0;
}

int sdfs_batch_newton_dev(sdfs_batch* h, const sdfs_opts* opts, double* w_inout_dev, int64_t* n_iter, int64_t* n_apply,
                          double* final_err, int32_t* status) {
  int rc = bcheck(h); if (rc) return rc;
  if (!opts || !w_inout_dev || !n_iter || !n_apply || !final_err || !status) return bfail(h, SDFS_ERR_ARG, "NULL argument");
  if (!(opts->tol >= 0.0)) return bfail(h, SDFS_ERR_ARG, "tol must be >= 0");
  BatchInner in;
  if ((rc = batch_check_inner(h, opts, "Newton", in)) || (rc = batch_newton_prepare(h))) return rc;
  const int B = h->B;
  hipStream_t st = h->stream;
  BatchNewtonArgs A;
  memset(&A, 0, sizeof A);
  A.tab = h->tab; A.scal = h->scal; A.w = w_inout_dev; A.ws = h->ws; A.st = h->nst;
  A.status = h->status; A.it = h->it; A.err = h->err;
  A.tol = opts->tol; A.max_iter = opts->max_iter;
  A.rtol2 = in.rtol2; A.atol2 = in.atol2; A.inner_max = in.inner_max; A.budget = in.budget;
  hipLaunchKernelGGL(batch_newton_init_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, h->status, h->it, h->err, h->nst, A.tol, (long long)A.max_iter);
  BHIPCHK(h, hipGetLastError());
  if ((rc = batch_run_groups(h, h->nfn, A, 0, opts->max_iter > 0 ? B : 0))) return rc;
  std::vector<long long> it((size_t)B);
  std::vector<BatchNewtonState> ns((size_t)B);
  BHIPCHK(h, hipMemcpyAsync(it.data(), h->it, (size_t)B * sizeof(long long), hipMemcpyDeviceToHost, st));
  BHIPCHK(h, hipMemcpyAsync(ns.data(), h->nst, (size_t)B * sizeof(BatchNewtonState), hipMemcpyDeviceToHost, st));
  BHIPCHK(h, hipMemcpyAsync(final_err, h->err, (size_t)B * 8, hipMemcpyDeviceToHost, st));
  BHIPCHK(h, hipMemcpyAsync(h->status_host, h->status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
  BHIPCHK(h, hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) { n_iter[b] = it[b]; n_apply[b] = ns[b].napply; status[b] = h->status_host[b]; }
  return 0;
}

int64_t sdfs_batch_adjoint_words(const sdfs_batch* h) {
  if (!h) return SDFS_ERR_ARG;
  return batch_adjoint_words(h);
}

int sdfs_batch_adjoint_dev(sdfs_batch* h, const sdfs_opts* opts, const double* w_dev, const double* g_dev, int64_t g_stride,
                           double* lam_dev, double* moments_dev, int64_t* n_iter, int64_t* n_apply, double* rel_resid,
                           double* resid_T, int32_t* status) {
  int rc = bcheck(h); if (rc) return rc;
  if (!opts || !w_dev || !g_dev || !moments_dev || !n_iter || !n_apply || !rel_resid || !resid_T || !status)
    return bfail(h, SDFS_ERR_ARG, "NULL argument");
  if (g_stride != 0 && g_stride != h->d.N) return bfail(h, SDFS_ERR_ARG, "g_stride %lld: 0 (one g for all) or %d", (long long)g_stride, h->d.N);
  BatchInner in;
  if ((rc = batch_check_inner(h, opts, "adjoint", in)) || (rc = batch_adjoint_prepare(h))) return rc;
  const int B = h->B;
  hipStream_t st = h->stream;
  BatchAdjointArgs A;
  memset(&A, 0, sizeof A);
  A.tab = h->tab; A.scal = h->scal; A.w = w_dev; A.g = g_dev; A.a2 = h->a2; A.lam = lam_dev; A.mom = moments_dev;
  A.ws = h->ws; A.st = h->ast; A.status = h->status;
  A.rtol2 = in.rtol2; A.atol2 = in.atol2; A.inner_max = in.inner_max; A.budget = in.budget;
  A.g_stride = g_stride;
  A.ax_lam = h->ax_lam; A.ax_c = h->ax_c; A.na3 = h->na3; A.words = batch_adjoint_words(h);
  hipLaunchKernelGGL(batch_adjoint_init_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, h->status, h->ast);
  BHIPCHK(h, hipGetLastError());
  if ((rc = batch_run_groups(h, h->afn, A, 0, B))) return rc;
  std::vector<BatchAdjointState> as((size_t)B);
  BHIPCHK(h, hipMemcpyAsync(as.data(), h->ast, (size_t)B * sizeof(BatchAdjointState), hipMemcpyDeviceToHost, st));
  BHIPCHK(h, hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) {
    n_iter[b] = as[b].k; n_apply[b] = as[b].napply; status[b] = h->status_host[b];
    resid_T[b] = as[b].resid_T;
    rel_resid[b] = as[b].gg > 0.0 ? std::sqrt(as[b].tr / as[b].gg) : (as[b].gg == 0.0 ? 0.0 : as[b].gg);
    if (status[b] == BATCH_NONFINITE) rel_resid[b] = std::numeric_limits<double>::quiet_NaN();
  }
  return 0;
}

int sdfs_batch_price_dev(sdfs_batch* h, const sdfs_opts* opts, const double* w_dev, const double* kappa, const double* kappa_ts,
                         const double* weights, int64_t n_max, double* EM_dev, double* EM2_dev, double* pd_dev, double* ER_dev,
                         double* moments_dev, double* horizons_dev, int64_t* n_iter, int64_t* n_apply, int64_t* n_horizons,
                         double* rel_resid, double* resid_T, int32_t* status) {
  int rc = bcheck(h); if (rc) return rc;
  if (!opts || !w_dev || !weights || !moments_dev || !n_iter || !n_apply || !n_horizons || !rel_resid || !resid_T || !status)
    return bfail(h, SDFS_ERR_ARG, "NULL argument");
  if (n_max < 0 || n_max > (1LL << 24)) return bfail(h, SDFS_ERR_ARG, "n_max = %lld: 0 .. 2^24", (long long)n_max);
  if (n_max > 0 && (!kappa_ts || !horizons_dev)) return bfail(h, SDFS_ERR_ARG, "n_max > 0 needs kappa_ts and horizons_dev");
  BatchInner in;
  if ((rc = batch_check_inner(h, opts, "pricing", in))) return rc;
  const int B = h->B, nl = h->d.n[h->ax_lam], nc = h->d.n[h->ax_c], na3 = h->na3;
  int gwords = 0;
  for (int a = 0; a < h->d.ndim; ++a) gwords += h->d.n[a];
  for (int b = 0; b < B; ++b) {
    if (kappa && !std::isfinite(kappa[b])) return bfail(h, SDFS_ERR_ARG, "kappa[%d] is not finite", b);
    if (n_max > 0 && !std::isfinite(kappa_ts[b])) return bfail(h, SDFS_ERR_ARG, "kappa_ts[%d] is not finite", b);
    for (int i = 0; i < gwords; ++i)
      if (!std::isfinite(weights[(size_t)b * gwords + i])) return bfail(h, SDFS_ERR_ARG, "weights of problem %d are not finite", b);
  }
  // the tilt tables of every stage (batch_price.hpp): t1[n_lam] t2[n_c] t3[na3], fp64 on the host; a stage that does
  // not run keeps 1
  const int tw = nl + nc + na3;
  std::vector<double> tilt((size_t)B * BP_STAGES * tw, 1.0);
  for (int b = 0; b < B; ++b) {
    const double th = h->theta_host[b], ga = h->gam_host[b], og = 1.0 - ga;
    const double* const hl = h->hlam_host.data() + (size_t)b * nl;
    const double* const sc = h->sigc_host.data() + (size_t)b * nc;
    const double* const mz = h->muz_host.data() + (size_t)b * na3;
    auto fill = [&](int stage, int p, double kl, double kc) {
      double* const t = tilt.data() + ((size_t)b * BP_STAGES + stage) * tw;
      const double xl = kl - th, xc = 0.5 * (kc * kc - og * og), xz = kc - p * og;
      for (int i = 0; i < nl; ++i) t[i] = std::exp(xl * hl[i]);
      for (int i = 0; i < nc; ++i) t[nl + i] = std::exp(xc * sc[i] * sc[i]);
      for (int i = 0; i < na3; ++i) t[nl + nc + i] = std::exp(xz * mz[i]);
    };
    if (kappa) { fill(0, 1, th, kappa[b] - ga); fill(3, 0, 0.0, kappa[b]); }
    fill(1, 1, th, -ga);
    fill(2, 2, 2.0 * th, -2.0 * ga);
    if (n_max > 0) fill(4, 1, th, kappa_ts[b] - ga);
  }
  if ((rc = batch_price_prepare(h))) return rc;
  hipStream_t st = h->stream;
  BatchDevBuf tiltd, gaxd;
  BHIPCHK(h, hipMalloc((void**)&tiltd.p, tilt.size() * 8));
  BHIPCHK(h, hipMalloc((void**)&gaxd.p, (size_t)B * gwords * 8));
  BHIPCHK(h, hipMemcpyAsync(tiltd.p, tilt.data(), tilt.size() * 8, hipMemcpyHostToDevice, st));
  BHIPCHK(h, hipMemcpyAsync(gaxd.p, weights, (size_t)B * gwords * 8, hipMemcpyHostToDevice, st));
  BatchPriceArgs A;
  memset(&A, 0, sizeof A);
  A.tab = h->tab; A.scal = h->scal; A.w = w_dev; A.tilt = tiltd.p; A.gax = gaxd.p;
  A.EM = EM_dev; A.EM2 = EM2_dev; A.pd = pd_dev; A.ER = ER_dev; A.mom = moments_dev; A.hz = n_max > 0 ? horizons_dev : nullptr;
  A.ws = h->ws; A.st = h->pst; A.status = h->status;
  A.rtol2 = in.rtol2; A.atol2 = in.atol2; A.inner_max = in.inner_max; A.budget = in.budget;
  A.n_max = n_max;
  A.ax_lam = h->ax_lam; A.ax_c = h->ax_c; A.na3 = na3; A.tiltwords = tw; A.gwords = gwords;
  A.claim = kappa ? 1 : 0;
  {
    const long long work = std::max<long long>((long long)B * std::max<long long>(BP_WORDS, 4 * n_max), (ER_dev || pd_dev) ? (long long)B * h->d.N : 0);
    const int blocks = (int)std::min<long long>((work + 255) / 256, (long long)h->num_cus * 8);
    hipLaunchKernelGGL(batch_price_init_kernel, dim3(std::max(1, blocks)), dim3(256), 0, st, B, h->d.N, h->status, h->pst, moments_dev,
                       A.hz, ER_dev, kappa ? (double*)nullptr : pd_dev, (long long)n_max, kappa ? 0 : 1);
    BHIPCHK(h, hipGetLastError());
  }
  if ((rc = batch_run_groups(h, h->pfn, A, 0, B))) return rc;
  std::vector<BatchPriceState> ps((size_t)B);
  BHIPCHK(h, hipMemcpyAsync(ps.data(), h->pst, (size_t)B * sizeof(BatchPriceState), hipMemcpyDeviceToHost, st));
  BHIPCHK(h, hipStreamSynchronize(st));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int b = 0; b < B; ++b) {
    n_iter[b] = ps[b].k; n_apply[b] = ps[b].napply; n_horizons[b] = ps[b].nh;
    // (BATCH_OPEN is 3 on the device, so the kernel reports "no finite price" as BATCH_NO_PRICE_DEV)
    status[b] = h->status_host[b] == BATCH_NO_PRICE_DEV ? (int)SDFS_BATCH_NO_PRICE : h->status_host[b];
    resid_T[b] = ps[b].resid_T;
    rel_resid[b] = !kappa ? nan : (ps[b].gg > 0.0 ? std::sqrt(ps[b].tr / ps[b].gg) : (ps[b].gg == 0.0 ? 0.0 : ps[b].gg));
    if (status[b] == BATCH_NONFINITE) rel_resid[b] = nan;
  }
  return 0;
}

// -- simulated paths of the batch (batch_sim.hpp) -----------------------------------------------------------------------
extern "C++" {
namespace {
constexpr int BSIM_K_DEFAULT = 2;            // record loads in flight per lane of the global form (tools/batch_simulation_times.py)
constexpr int BSIM_RECORDS_DEFAULT = 2;      // the form where both apply: 1 LDS records, 2 global gather (the same A/B: global won by 2.5 % at SSY 5^4)

// doubles of a member's table block: cumulative rows per axis, cumulative stationary marginals, h_lambda, sigma_c (even)
int batch_sim_words(const BatchDesc& d, int ax_lam, int ax_c) {
  int n = 0;
  for (int a = 0; a < d.ndim; ++a) n += d.n[a] * d.n[a] + d.n[a];
  return (n + d.n[ax_lam] + d.n[ax_c] + 1) & ~1;
}

// dynamic LDS of k_batch_sim_paths in the form `records` (1 LDS, 2 global)
long long batch_sim_lds(const BatchDesc& d, int simwords, int records) {
  return 8LL * ((long long)simwords + (records == 1 ? (long long)d.N * SIM_REC : 0) + BSIM_RED);
}

template <int ND, bool KAP>
batch_sim_fn batch_sim_kernel_of(bool ldsrec, bool store, int k) {
  if (ldsrec) return store ? k_batch_sim_paths<ND, KAP, true, true, 1> : k_batch_sim_paths<ND, KAP, true, false, 1>;
  if (store) return k_batch_sim_paths<ND, KAP, false, true, BSIM_K_DEFAULT>;
  return k == 1 ? k_batch_sim_paths<ND, KAP, false, false, 1> : k == 2 ? k_batch_sim_paths<ND, KAP, false, false, 2>
                                                                       : k_batch_sim_paths<ND, KAP, false, false, 4>;
}

batch_sim_fn batch_sim_kernel_for(int ndim, bool kap, bool ldsrec, bool store, int k) {
  if (ndim == 4) return kap ? batch_sim_kernel_of<4, true>(ldsrec, store, k) : batch_sim_kernel_of<4, false>(ldsrec, store, k);
  return kap ? batch_sim_kernel_of<6, true>(ldsrec, store, k) : batch_sim_kernel_of<6, false>(ldsrec, store, k);
}

// the table blocks [B][words], the scalars [B][4] = theta, theta ln beta, gamma, kappa and the skip flags [B] of a request,
// from the members' host fields (h_lambda [B][n_lam], sigma_c [B][n_c], theta, beta, gamma [B]).  Host only.
void batch_sim_stage(const BatchDesc& D, const SimArgs& a, int ncdf, int ncdf0, int words, int B, const sdfs_batch_sim_desc* d,
                     const double* hlam, const double* sigc, const double* theta, const double* beta, const double* gam,
                     double* tb, double* sc, int* sk) {
  const int nl = D.n[a.ax_lam], nc = D.n[a.ax_c];
  std::fill(tb, tb + (size_t)B * words, 0.0);
  for (int b = 0; b < B; ++b) {
    sim_fill_table(a, ncdf, ncdf0, d->cdf + (size_t)b * ncdf, d->start_fixed ? nullptr : d->cdf0 + (size_t)b * ncdf0, hlam + (size_t)b * nl,
                   sigc + (size_t)b * nc, tb + (size_t)b * words);
    const int skip = d->skip && d->skip[b] ? 1 : 0;
    if (sk) sk[b] = skip;
    sc[4 * b] = theta[b]; sc[4 * b + 1] = theta[b] * std::log(beta[b]); sc[4 * b + 2] = gam[b];
    sc[4 * b + 3] = d->has_kappa && !skip ? d->kappa[b] : 0.0;
  }
}

template <class T>
int batch_sim_grow(sdfs_batch* h, T** p, size_t* cap, size_t need) {
  if (*p && (!cap || *cap >= need)) return 0;
  if (*p) { BHIPCHK(h, hipStreamSynchronize(h->stream)); BHIPCHK(h, hipFree(*p)); *p = nullptr; }
  BHIPCHK(h, hipMalloc((void**)p, need * sizeof(T)));
  if (cap) *cap = need;
  return 0;
}
}  // namespace
}  // extern "C++"

int64_t sdfs_batch_sim_lds_bytes(int model, int ndim, const int64_t* shapes, int records) {
  BatchDesc d;
  BatchModelConsts c;
  long long lds = 0;
  const int rc = batch_geometry(model, ndim, shapes, d, c, &lds);
  if (rc) return rc;
  if (records != 1 && records != 2) { g_create_error = "records: 1 (LDS) or 2 (global)"; return SDFS_ERR_ARG; }
  const long long bytes = batch_sim_lds(d, batch_sim_words(d, c.ax_lam, c.ax_c), records);
  if (bytes > BATCH_LDS_MAX) {
    char buf[160];
    snprintf(buf, sizeof buf, "tables and %d records need %lld bytes of LDS, one CU has %d", d.N, bytes, BATCH_LDS_MAX);
    g_create_error = buf;
    return SDFS_ERR_UNSUPPORTED;
  }
  return bytes;
}

int64_t sdfs_batch_sim_tables(int model, int ndim, const int64_t* shapes, int64_t B, const double* params, const double* const* arrays,
                              const int64_t* array_sizes, int narrays, const sdfs_batch_sim_desc* d, double* tab_out, double* scal_out,
                              double* zt_out) {
  auto no = [](int code, const char* msg) { g_create_error = msg; return (int64_t)code; };
  BatchDesc D;
  BatchModelConsts c;
  long long lds = 0;
  const int rc = batch_geometry(model, ndim, shapes, D, c, &lds);
  if (rc) return rc;
  const int words = batch_sim_words(D, c.ax_lam, c.ax_c);
  if (!tab_out && !scal_out && !zt_out) return words;
  if (!params || !arrays || !array_sizes || !d || !tab_out || !scal_out) return no(SDFS_ERR_ARG, "NULL argument");
  if (B < 1 || narrays < 1 || narrays > 32) return no(SDFS_ERR_ARG, "B or narrays out of range");
  if (!d->cdf || (!d->start_fixed && !d->cdf0) || (d->has_kappa && !d->kappa)) return no(SDFS_ERR_ARG, "NULL table or kappa in desc");
  std::vector<double> hl((size_t)B * D.n[c.ax_lam]), sg((size_t)B * D.n[c.ax_c]), th((size_t)B), be((size_t)B), ga((size_t)B);
  for (int64_t b = 0; b < B; ++b) {          // the host fields sdfs_batch_create keeps
    BatchMember m;
    if (batch_member_fields(m, model, ndim, shapes, D, c, b, params, arrays, array_sizes, narrays,
                            {hl.data(), sg.data(), zt_out, th.data(), be.data(), ga.data()}))
      continue;
    if (m.bad_array >= 0) return no(SDFS_ERR_ARG, "arrays[i] is NULL");
    if (m.rc) { g_create_error = m.hh.err; return m.rc; }
    return no(SDFS_ERR_ARG, "state arrays of unexpected size");
  }
  SimArgs a{};
  int ncdf = 0, ncdf0 = 0;
  if (sim_layout(D.ndim, D.n, D.stride, c.ax_lam, c.ax_c, d, a, &ncdf, &ncdf0) >= 0) return no(SDFS_ERR_ARG, "start is not a state index");
  batch_sim_stage(D, a, ncdf, ncdf0, words, (int)B, d, hl.data(), sg.data(), th.data(), be.data(), ga.data(), tab_out, scal_out, nullptr);
  return words;
}

int sdfs_batch_sim_records_dev(sdfs_batch* h, const double* w_dev, const double* em_dev, const double* v_dev, double* records_dev) {
  int rc = bcheck(h); if (rc) return rc;
  if (!w_dev || !em_dev || !records_dev) return bfail(h, SDFS_ERR_ARG, "NULL grid pointer");
  if (!h->sim_zt) {
    BHIPCHK(h, hipMalloc((void**)&h->sim_zt, h->muz_host.size() * 8));
    BHIPCHK(h, hipMemcpy(h->sim_zt, h->muz_host.data(), h->muz_host.size() * 8, hipMemcpyHostToDevice));
  }
  const int gx = std::min((h->d.N + 255) / 256, 64);
  for (int b0 = 0; b0 < h->B; b0 += BSIM_YMAX) {
    hipLaunchKernelGGL(k_batch_sim_records, dim3(gx, std::min(BSIM_YMAX, h->B - b0)), dim3(256), 0, h->stream, h->d, h->na3, b0,
                       (const double*)h->sim_zt, w_dev, em_dev, v_dev, records_dev);
    BHIPCHK(h, hipGetLastError());
  }
  return 0;
}

int sdfs_batch_sim_paths_dev(sdfs_batch* h, const double* records_dev, const sdfs_batch_sim_desc* d, double* stats_dev,
                             double* moments_dev, uint8_t* idx_dev, double* series_dev) {
  int rc = bcheck(h); if (rc) return rc;
  if (!records_dev || !d) return bfail(h, SDFS_ERR_ARG, "NULL records or desc");
  if (!stats_dev && !moments_dev) return bfail(h, SDFS_ERR_ARG, "stats_dev and moments_dev are both NULL: nothing to write");
  if (!idx_dev != !series_dev) return bfail(h, SDFS_ERR_ARG, "idx and series are stored together: both NULL or neither");
  char msg[160];
  if (!sim_ranges_ok(msg, d->path_offset, d->n_paths, nullptr, d->burn_in, d->n_periods, 8)) return bfail(h, SDFS_ERR_ARG, "%s", msg);
  if (!d->cdf || (!d->start_fixed && !d->cdf0)) return bfail(h, SDFS_ERR_ARG, "NULL cumulative transition table");
  if (d->has_kappa && !d->kappa) return bfail(h, SDFS_ERR_ARG, "has_kappa needs kappa[B]");
  if (d->records < 0 || d->records > 2) return bfail(h, SDFS_ERR_ARG, "records = %d: 0 (default), 1 (LDS) or 2 (global)", d->records);
  const int k = d->lookahead ? d->lookahead : BSIM_K_DEFAULT;
  if (k != 1 && k != 2 && k != 4) return bfail(h, SDFS_ERR_ARG, "lookahead = %d: 1, 2 or 4", d->lookahead);
  if (d->search != 0 && d->search != 2)
    return bfail(h, d->search == 1 ? SDFS_ERR_UNSUPPORTED : SDFS_ERR_ARG, "search = %d: the batch kernels search by bisection (0 or 2)", d->search);
  if (idx_dev && k != BSIM_K_DEFAULT) return bfail(h, SDFS_ERR_ARG, "stored paths run with the default lookahead");
  const BatchDesc& D = h->d;
  const int B = h->B;
  const int words = batch_sim_words(D, h->ax_lam, h->ax_c);
  const bool fits = batch_sim_lds(D, words, 1) <= BATCH_LDS_MAX;
  if (d->records == 1 && !fits)
    return bfail(h, SDFS_ERR_ARG, "records = 1: tables and %d records need %lld bytes of LDS, one CU has %d", D.N, batch_sim_lds(D, words, 1), BATCH_LDS_MAX);
  const bool ldsrec = d->records ? d->records == 1 : (fits && BSIM_RECORDS_DEFAULT == 1);
  const long long G = (d->n_paths + SIM_BLOCK - 1) / SIM_BLOCK;
  const bool kap = d->has_kappa != 0;
  const int nstat = 3 * (kap ? 9 : 6) + 1;
  for (int b = 0; b < B; ++b)
    if (kap && !(d->skip && d->skip[b]) && !std::isfinite(d->kappa[b])) return bfail(h, SDFS_ERR_ARG, "kappa[%d] is not finite", b);

  // the members' table blocks, scalars and skip flags
  SimArgs a{};
  int ncdf = 0, ncdf0 = 0;
  const int bad = sim_layout(D.ndim, D.n, D.stride, h->ax_lam, h->ax_c, d, a, &ncdf, &ncdf0);
  if (bad >= 0) return bfail(h, SDFS_ERR_ARG, "start[%d] = %d: a state index of axis %d lies in 0 ... %d", bad, d->start[bad], bad, D.n[bad] - 1);
  // the previous call's uploads read the staging vectors: wait for them (not for the stream's kernels)
  if (h->sim_staged) BHIPCHK(h, hipEventSynchronize(h->sim_staged));
  else BHIPCHK(h, hipEventCreateWithFlags(&h->sim_staged, hipEventDisableTiming));
  auto& tb = h->sim_tab_host;
  auto& sc = h->sim_scal_host;
  auto& sk = h->sim_skip_host;
  tb.resize((size_t)B * words); sc.resize((size_t)B * 4); sk.resize((size_t)B);
  batch_sim_stage(D, a, ncdf, ncdf0, words, B, d, h->hlam_host.data(), h->sigc_host.data(), h->theta_host.data(), h->beta_host.data(),
                  h->gam_host.data(), tb.data(), sc.data(), sk.data());
  const size_t part_need = (size_t)B * nstat * (size_t)G * 3;
  if ((rc = batch_sim_grow(h, &h->sim_tab, (size_t*)nullptr, tb.size())) || (rc = batch_sim_grow(h, &h->sim_scal, (size_t*)nullptr, sc.size())) ||
      (rc = batch_sim_grow(h, &h->sim_skip, (size_t*)nullptr, sk.size())) || (rc = batch_sim_grow(h, &h->sim_part, &h->sim_part_cap, part_need)))
    return rc;
  hipStream_t st = h->stream;
  BHIPCHK(h, hipMemcpyAsync(h->sim_tab, tb.data(), tb.size() * 8, hipMemcpyHostToDevice, st));
  BHIPCHK(h, hipMemcpyAsync(h->sim_scal, sc.data(), sc.size() * 8, hipMemcpyHostToDevice, st));
  BHIPCHK(h, hipMemcpyAsync(h->sim_skip, sk.data(), sk.size() * sizeof(int), hipMemcpyHostToDevice, st));
  BHIPCHK(h, hipEventRecord(h->sim_staged, st));

  const batch_sim_fn fn = batch_sim_kernel_for(D.ndim, kap, ldsrec, idx_dev != nullptr, k);
  const size_t lds = (size_t)batch_sim_lds(D, words, ldsrec ? 1 : 2);
  if ((rc = batch_allow_lds(h, (const void*)fn, lds))) return rc;
  BatchSimArgs A;
  memset(&A, 0, sizeof A);
  A.s = a; A.tab = h->sim_tab; A.scal = h->sim_scal; A.skip = h->sim_skip; A.rec = records_dev;
  A.stats = stats_dev; A.part = h->sim_part; A.idx = idx_dev; A.ser = series_dev;
  A.simwords = words; A.N = D.N;
  for (int b0 = 0; b0 < B; b0 += BSIM_YMAX) {
    A.b0 = b0;
    hipLaunchKernelGGL(fn, dim3((unsigned)G, (unsigned)std::min(BSIM_YMAX, B - b0)), dim3(SIM_BLOCK), lds, st, A);
    BHIPCHK(h, hipGetLastError());
  }
  if (moments_dev) {
    hipLaunchKernelGGL(k_batch_sim_moments, dim3((B * nstat + 255) / 256), dim3(256), 0, st, B, nstat, (int)G, (const int*)h->sim_skip,
                       (const double*)h->sim_part, moments_dev);
    BHIPCHK(h, hipGetLastError());
  }
  return 0;
}

int sdfs_batch_describe(const sdfs_batch* h, char* buf, int64_t cap) {
  if (!h || !buf || cap < 1) return SDFS_ERR_ARG;
  std::string s;
  char line[512];
  snprintf(line, sizeof line, "batch plan: %d problems, one workgroup each; grid of %d points in LDS, %d threads x %d points in registers\n",
           h->B, h->d.N, h->nt, h->k);
  s += line;
  snprintf(line, sizeof line, "dynamic LDS %zu B: work %d + tables %d + %d doubles; default chunk %d iterations per launch\n",
           h->lds_bytes, h->d.nwork, h->d.tabwords, BATCH_RED, batch_default_chunk(h));
  s += line;
  for (int a = 0; a < h->d.ndim; ++a) {
    snprintf(line, sizeof line, "axis %d: extent %d stride %d, lines of fp64 FMAs unrolled to %d\n", a, h->d.n[a], h->d.stride[a], h->d.np[a]);
    s += line;
  }
  if (h->nfn) {
    const int slots = batch_newton_slots(h);
    snprintf(line, sizeof line, "newton: w, r, rhat, p, q, x, c_in, c_out %s; workspace 7 x %d doubles per problem, %d problems per group%s; default budget %d applications per launch\n",
             h->newton_reg ? "in registers (the workspace holds them between launches only)" : "in global memory (w in the caller's buffer, seven in the workspace)",
             h->d.nwork, slots, slots < h->B ? " (the batch runs group after group)" : "", batch_newton_default_budget(h));
    s += line;
  }
  if (h->afn) {
    snprintf(line, sizeof line, "adjoint: lambda with r, rhat, p, q, c_in, c_out and w %s; %d moments per problem (s0 s1 s2 | R[%d] | M1[%d] | M2[%d] | M3[%d]); default budget %d applications per launch\n",
             h->adjoint_reg ? "in registers (the Newton workspace holds them between launches only)" : "in global memory (w in the caller's buffer, seven in the Newton workspace)",
             batch_adjoint_words(h), h->d.ndim, h->d.n[h->ax_lam], h->d.n[h->ax_c], h->na3, batch_newton_default_budget(h));
    s += line;
  }
  if (h->pfn) {
    snprintf(line, sizeof line, "pricing: v, E_M, the point weights, P_n with c_in, c_out (rescaled per stage) and w %s; %d words per problem, tilt tables of %d + %d + %d doubles per stage; at most 2 inner_max + n_max + %d applications per problem\n",
             h->price_reg ? "in registers (the Newton workspace holds them between launches only)" : "in global memory (w in the caller's buffer, seven in the Newton workspace)",
             BP_WORDS, h->d.n[h->ax_lam], h->d.n[h->ax_c], h->na3, 2 * BP_RESTARTS + 11);
    s += line;
  }
  {
    const int words = batch_sim_words(h->d, h->ax_lam, h->ax_c);
    const bool fits = batch_sim_lds(h->d, words, 1) <= BATCH_LDS_MAX;
    const bool ldsrec = fits && BSIM_RECORDS_DEFAULT == 1;
    snprintf(line, sizeof line, "simulation: one path per lane, %d paths per workgroup, tables of %d doubles in LDS; records %s by default (the LDS form %s: %lld B); moments reduced per workgroup, then in workgroup order\n",
             SIM_BLOCK, words, ldsrec ? "in LDS" : "gathered from global memory", fits ? "fits" : "does not fit", batch_sim_lds(h->d, words, 1));
    s += line;
  }
  snprintf(buf, (size_t)cap, "%s", s.c_str());
  return 0;
}

}  // extern "C"

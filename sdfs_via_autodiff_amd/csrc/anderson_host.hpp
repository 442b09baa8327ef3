// anderson_host.hpp -- host side of Anderson acceleration (code/solvers.py:98-124, jaxopt's parametrisation) in its
// five forms: the host-controlled loop (solve_anderson_host, SDFS_AND_HOST=1), the device loop with one launch per step,
// the fused small-grid loop and the batched-Gram loop (solve_anderson: enqueue, enqueue_fused, enqueue_lazy) and the
// sharded step API (sdfs_anderson_begin / _gate / _step / _state).  What a run sets up is written once, in the helpers
// ahead of the loops.
//
// Not a header of its own: sdfs_api.hip includes it once, ahead of its extern "C" block.  It uses sdfs_handle (the
// `anderson` member), AndRun, Apply, apply, apply_T_dev, capture_graph, check, counter_id, dev_alloc, ensure_buf /
// ensure_scalars / ensure_tmp, fail, FastPass, HIPCHK, lcm, ProfScope, small_grid and vec_grid of that file, and its includes.
namespace {

// dense solve of the (m+1) x (m+1) bordered Anderson system, partial pivoting
bool solve_dense(std::vector<double>& A, std::vector<double>& b, int n) {
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r) if (std::fabs(A[r * n + c]) > std::fabs(A[piv * n + c])) piv = r;
    if (A[piv * n + c] == 0.0) return false;
    if (piv != c) { for (int k = 0; k < n; ++k) std::swap(A[c * n + k], A[piv * n + k]); std::swap(b[c], b[piv]); }
    for (int r = c + 1; r < n; ++r) {
      const double f = A[r * n + c] / A[c * n + c];
      if (f == 0.0) continue;
      for (int k = c; k < n; ++k) A[r * n + k] -= f * A[c * n + k];
      b[r] -= f * b[c];
    }
  }
  for (int r = n - 1; r >= 0; --r) {
    double s = b[r];
    for (int k = r + 1; k < n; ++k) s -= A[r * n + k] * b[k];
    b[r] = s / A[r * n + r];
  }
  return true;
}

// history length (at most `cap`: AND_MAX_M in the loops, AND_LAZY_M in the step API) and mixing frequency of a run
int check_and_args(sdfs_handle* h, int history, int mixing_freq, int cap) {
  if (history < 1 || history > cap) return fail(h, SDFS_ERR_ARG, "Anderson history must be in 1..%d", cap);
  if (mixing_freq < 1) return fail(h, SDFS_ERR_ARG, "mixing_freq must be >= 1");
  return 0;
}

// the pointers of a history of m slots: slot j keeps the vectors x(j) and r(j)
template <typename FX, typename FR>
AndPtrs and_ptrs(int m, FX x, FR r) {
  AndPtrs hp;
  memset(&hp, 0, sizeof hp);
  for (int j = 0; j < m; ++j) { hp.X[j] = x(j); hp.R[j] = r(j); }
  return hp;
}

// the history of the two solve loops: m slots on the handle (they only grow), *hp pointing at them, the start value w
// in the iterate buf0, the residuals zeroed
int and_history(sdfs_handle* h, int m, const double* w, AndPtrs* hp) {
  int rc;
  auto& A = h->anderson;
  while ((int)A.X.size() < m) {
    double *a = nullptr, *b = nullptr;
    if ((rc = dev_alloc(h, &a, (size_t)h->N)) || (rc = dev_alloc(h, &b, (size_t)h->N))) return rc;
    A.X.push_back(a); A.R.push_back(b);
  }
  *hp = and_ptrs(m, [&](int j) { return A.X[j]; }, [&](int j) { return A.R[j]; });
  const size_t nb = sizeof(double) * (size_t)h->N;
  HIPCHK(h, hipMemcpyAsync(h->buf0, w, nb, hipMemcpyDeviceToDevice, h->stream));
  for (int j = 0; j < m; ++j) HIPCHK(h, hipMemsetAsync(A.R[j], 0, nb, h->stream));
  return 0;
}

// the control state of the device-resident forms and its pinned mirror
int ensure_and_state(sdfs_handle* h) {
  auto& A = h->anderson;
  if (A.state) return 0;
  HIPCHK(h, hipMalloc((void**)&A.state, 2 * sizeof(AndState)));
  h->misc_allocs.push_back(A.state);
  HIPCHK(h, hipHostMalloc((void**)&A.state_host, sizeof(AndState)));
  return 0;
}

// Per-pass records and their mirrors for n passes.  A captured chunk has the old addresses baked in and goes; the freed
// mirrors are nulled first, so that the handle can still be destroyed when an allocation below fails.
int ensure_and_slots(sdfs_handle* h, int n) {
  auto& A = h->anderson;
  if (A.slots >= n) return 0;
  if (A.graph) { hipGraphExecDestroy(A.graph); A.graph = nullptr; }
  if (A.err_host) { hipHostFree(A.err_host); A.err_host = nullptr; }
  if (A.kind_host) { hipHostFree(A.kind_host); A.kind_host = nullptr; }
  HIPCHK(h, hipMalloc((void**)&A.err, sizeof(double) * n));
  h->misc_allocs.push_back(A.err);
  HIPCHK(h, hipMalloc((void**)&A.kind, sizeof(int) * n));
  h->misc_allocs.push_back(A.kind);
  HIPCHK(h, hipMalloc((void**)&A.flag, sizeof(unsigned) * n));
  h->misc_allocs.push_back(A.flag);
  HIPCHK(h, hipHostMalloc((void**)&A.err_host, sizeof(double) * n));
  HIPCHK(h, hipHostMalloc((void**)&A.kind_host, sizeof(int) * n));
  A.slots = n;
  return 0;
}

// workgroups of k_and_gram_full on n points, and the partial sums they leave
int and_gram_blocks(long long n) { return (int)std::min<long long>(AND_LAZY_BLOCKS, std::max<long long>(1, (n + 2 * VEC_BLOCK - 1) / (2 * VEC_BLOCK))); }
int ensure_and_gram_partial(sdfs_handle* h) {
  auto& A = h->anderson;
  if (A.gram_partial) return 0;
  HIPCHK(h, hipMalloc((void**)&A.gram_partial, sizeof(double) * (size_t)AND_LAZY_PAIRS * AND_LAZY_BLOCKS));
  h->misc_allocs.push_back(A.gram_partial);
  return 0;
}

// the state a run starts from (nothing pushed, infinite error, the gate open unless there is nothing to do) in the
// pinned mirror and in the first `copies` device buffers; returns once it is there
int and_init_state(sdfs_handle* h, double tol, long long max_iter, int copies) {
  AndState& I = *h->anderson.state_host;
  memset(&I, 0, sizeof I);
  I.err = std::numeric_limits<double>::infinity();
  I.prev_pos = -1.0; I.mix_rel = -1;
  I.gate = (max_iter > 0 && I.err > tol) ? ~0ULL : 0ULL;
  for (int c = 0; c < copies; ++c) HIPCHK(h, hipMemcpyAsync(h->anderson.state + c, &I, sizeof I, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}

// The launches of the batched-Gram form (vec_kernels.hpp), shared by enqueue_lazy and sdfs_anderson_step.  `sums` is where
// the step API wants this rank's totals; the single-GPU loop passes nullptr and hands the partials themselves to the step.
// Y[pos] = x_in + beta r, R[pos] = r = x_out - x_in, <r, r> per workgroup in h->partial
void and_push_lite(sdfs_handle* h, const AndRun& D, int pos, const double* x_in, const double* x_out, double* sums) {
  const int g = vec_grid(D.n);
  const unsigned long long* gate = &h->anderson.state->gate;
  hipLaunchKernelGGL(k_and_push_lite, dim3(g), dim3(VEC_BLOCK), 0, h->stream, x_in, x_out, D.hp.X[pos], D.hp.R[pos], D.beta, D.n, h->partial, gate);
  if (sums) hipLaunchKernelGGL(k_presum, dim3(1), dim3(VEC_BLOCK), 0, h->stream, (const double*)h->partial, g, 1, sums, gate);
}
// the whole Gram matrix in one sweep (pairs i <= j in k_and_gram_full's order), per workgroup in gram_partial
void and_gram_full(sdfs_handle* h, const AndRun& D, double* sums) {
  const auto& A = h->anderson;
  const int gb = and_gram_blocks(D.n);
  hipLaunchKernelGGL(k_and_gram_full, dim3(gb), dim3(VEC_BLOCK), 0, h->stream, D.hp, D.m, D.mixing_freq, D.n, A.gram_partial, (const AndState*)A.state);
  if (sums) hipLaunchKernelGGL(k_presum, dim3(1), dim3(VEC_BLOCK), 0, h->stream, (const double*)A.gram_partial, gb, AND_LAZY_PAIRS, sums, (const unsigned long long*)&A.state->gate);
}
// the control step of pass `rel` from <r, r> in rr (nb_rr partials; 0: a total) and, where `refresh`, the Gram sums in
// gram (nb_gram partials per pair); error and step kind go to record `slot`
void and_step_lazy(sdfs_handle* h, const AndRun& D, const double* rr, int nb_rr, const double* gram, int nb_gram, int refresh, int pos, int rel, int slot) {
  const auto& A = h->anderson;
  hipLaunchKernelGGL(k_and_step_lazy, dim3(1), dim3(nb_rr > 4096 ? 1024 : VEC_BLOCK), 0, h->stream, rr, nb_rr, gram, nb_gram, refresh,
                     D.m, pos, rel, A.state, A.err + slot, A.kind + slot, D.tol, D.max_iter, D.mixing_freq, D.ridge);
}
// the update of x the step decided on, in place in x (= T x_in on entry)
void and_mix_y(sdfs_handle* h, const AndRun& D, double* x, int pos, int rel) {
  hipLaunchKernelGGL(k_and_mix_y, dim3(vec_grid(D.n)), dim3(VEC_BLOCK), 0, h->stream, D.hp, (const AndState*)h->anderson.state, D.m, D.beta, x, (const double*)x, pos, rel, D.n);
}

// AndArgs of the fused small-grid form (anderson_step.hpp): what every launch of a run shares ...
AndArgs and_args(const AndPtrs& hp, const AndStepPar& par, double beta, int m, int nb) {
  AndArgs an;
  memset(&an, 0, sizeof an);
  an.h = hp; an.par = par; an.beta = beta; an.m = m; an.nb = nb;
  return an;
}
// ... and the fields of pass `rel` of a chunk.  S given: the control step of that pass (SM_AND_FIRST of the pass after
// it, small_and_finish) -- state S[rel & 1] -> S[(rel + 1) & 1], the sums its push left, the mixed iterate to x.  S null:
// its push (SM_AND_LAST), which leaves those sums; the fields it does not read stay as they are.
void and_args_pass(AndArgs& an, const sdfs_handle* h, int rel, int step_kind, AndState* S, double* x) {
  const auto& A = h->anderson;
  const int pos = rel % an.m;
  if (S) {
    an.Sin = S + (rel & 1); an.Sout = S + ((rel + 1) & 1); an.partial = h->partial; an.x = x;
    an.err_slot = A.err + rel; an.kind_slot = A.kind + rel;
  } else {
    an.Sin = nullptr; an.Sout = nullptr; an.partial = nullptr; an.partial_out = h->partial;
  }
  an.x_pos = an.h.X[pos]; an.r_pos = an.h.R[pos]; an.pos = pos; an.rel = rel; an.step_kind = step_kind; an.flag = A.flag + rel;
}

// Anderson acceleration with jaxopt's parametrisation (code/solvers.py:98-124).
int solve_anderson_host(sdfs_handle* h, const sdfs_opts& o, double* w, int64_t* n_iter, int64_t* n_apply, double* final_err) {
  int rc;
  auto& A = h->anderson;
  const int m = o.history;
  if ((rc = check_and_args(h, m, o.mixing_freq, AND_MAX_M))) return rc;
  if ((rc = ensure_buf(h, &h->buf0)) || (rc = ensure_buf(h, &h->buf1)) || (rc = ensure_scalars(h))) return rc;
  if (!A.gram_row) {
    if ((rc = dev_alloc(h, &A.gram_row, AND_MAX_M))) return rc;
    HIPCHK(h, hipHostMalloc((void**)&A.gram_row_host, sizeof(double) * AND_MAX_M));
  }
  AndPtrs hp;
  if ((rc = and_history(h, m, w, &hp))) return rc;
  const long long n = h->N;
  const int g = vec_grid(n);
  const size_t nb = sizeof(double) * (size_t)n;
  hipStream_t st = h->stream;
  double* x = h->buf0;
  double* fx = h->buf1;
  std::vector<double> G((size_t)m * m, 0.0);
  h->trace.clear();
  long long it = 0;
  double err = std::numeric_limits<double>::infinity();
  int status = 0;
  const int cvec = h->profiling ? counter_id(h, "anderson_blas1", 0, 0) : -1;
  // Safeguard (not in jaxopt): when a mixing step leaves the domain (w <= 0 -> NaN in the next
  // application; the (m+1)^2 system is badly conditioned once the residual history is nearly
  // collinear and N r^2 dwarfs the absolute ridge), fall back to the plain step x_prev + r_prev from
  // the last good iterate, drop the poisoned history slot and pause mixing until the history refills.
  bool last_mixed = false;
  int prev_pos = -1, rejected = 0;
  long long no_mix_until = 0;
  while (err > o.tol && it < o.max_iter) {
    if ((rc = apply_T_dev(h, x, fx, nullptr, nullptr, 0.0))) return rc;
    const int pos = (int)(it % m);
    { ProfScope ps(h, cvec);
      hipLaunchKernelGGL(k_and_push, dim3(g), dim3(VEC_BLOCK), 0, st, x, fx, hp, m, pos, n, h->partial);
      hipLaunchKernelGGL(k_and_push_finish, dim3(1), dim3(VEC_BLOCK), 0, st, h->partial, g, m, A.gram_row); }
    HIPCHK(h, hipMemcpyAsync(A.gram_row_host, A.gram_row, sizeof(double) * m, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    for (int j = 0; j < m; ++j) { G[(size_t)pos * m + j] = A.gram_row_host[j]; G[(size_t)j * m + pos] = A.gram_row_host[j]; }
    err = std::sqrt(G[(size_t)pos * m + pos]);
    if (!std::isfinite(err) && last_mixed && prev_pos >= 0 && rejected < 1000) {
      for (int j = 0; j < m; ++j) { G[(size_t)pos * m + j] = 0.0; G[(size_t)j * m + pos] = 0.0; }
      HIPCHK(h, hipMemsetAsync(A.R[pos], 0, nb, st));
      AndCoef c;
      memset(&c, 0, sizeof c);
      c.a[prev_pos] = 1.0;
      { ProfScope ps(h, cvec);
        hipLaunchKernelGGL(k_and_mix, dim3(g), dim3(VEC_BLOCK), 0, st, hp, c, m, 1.0, x, n); }   // x = X_prev + R_prev
      err = std::sqrt(G[(size_t)prev_pos * m + prev_pos]);
      last_mixed = false; ++rejected; ++it;
      no_mix_until = it + m;
      continue;
    }
    if (o.record_errors) h->trace.push_back(err);
    bool mixed = false;
    if (it + 1 >= m && it + 1 >= no_mix_until && (it + 1) % o.mixing_freq == 0 && std::isfinite(err)) {
      const int d = m + 1;
      std::vector<double> M((size_t)d * d, 0.0), b(d, 0.0);
      for (int j = 1; j < d; ++j) { M[j] = 1.0; M[(size_t)j * d] = 1.0; }
      double rg = o.ridge;                     // (< 0: relative to trace(G) / m, as in and_step_wave)
      if (rg < 0.0) { double tr = 0.0; for (int j = 0; j < m; ++j) tr += G[(size_t)j * m + j]; rg = -rg * tr / m; }
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) M[(size_t)(i + 1) * d + j + 1] = G[(size_t)i * m + j] + (i == j ? rg : 0.0);
      b[0] = 1.0;
      if (solve_dense(M, b, d)) {
        AndCoef c;
        memset(&c, 0, sizeof c);
        for (int j = 0; j < m; ++j) c.a[j] = b[j + 1];
        ProfScope ps(h, cvec);
        hipLaunchKernelGGL(k_and_mix, dim3(g), dim3(VEC_BLOCK), 0, st, hp, c, m, o.beta, x, n);
        mixed = true;
      }
    }
    if (!mixed) std::swap(x, fx);
    last_mixed = mixed; prev_pos = pos;
    ++it;
    if (!std::isfinite(err)) { status = SDFS_ERR_NUMERIC; break; }
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(w, x, nb, hipMemcpyDeviceToDevice, st));
  HIPCHK(h, hipStreamSynchronize(st));
  *n_iter = it; *n_apply = it; *final_err = err;
  if (status) return fail(h, status, "non-finite Anderson residual at iteration %lld", it);
  return 0;
}

// Small-grid plan: can the Anderson loop run its fused form (fast_kernels.hpp, SM_AND_FIRST / SM_AND_LAST) with history m?
bool anderson_fused_ok(const sdfs_handle* h, int m) {
  if (!(h->knobs.and_fused && h->fast.ok && h->fast.small && h->fast.passes.size() >= 2 && m <= AND_FUSE_M)) return false;
  // (pair order reversed: the application ends on the fastest pair, whose tiles are contiguous -- the push's history
  // streams then cost 4 lines per wave request instead of 64)
  const FastPass& L = h->fast.passes.front();
  const FastPass& F = h->fast.passes.back();
  return (int)small_grid(L.sm, L.wpt) <= AND_FUSE_RING && L.sm.a3 != nullptr && F.sm.a3 != nullptr &&
         small_and_variant(SM_AND_FIRST, F.r, F.wpt) != nullptr && small_and_variant(SM_AND_LAST, L.r, L.wpt) != nullptr;
}

// The same loop with its control on the device (vec_kernels.hpp, AndState / k_and_step / k_and_mix_dev): per pass
// T, push, one single-workgroup step kernel (Gram row, solve, safeguard, stopping test) and the update of x, every
// launch gated on the loop's own flag; `chunk` passes per host synchronisation, replayed from a hipGraph.
int solve_anderson(sdfs_handle* h, const sdfs_opts& o, double* w, int64_t* n_iter, int64_t* n_apply, double* final_err) {
  if (h->knobs.and_host) return solve_anderson_host(h, o, w, n_iter, n_apply, final_err);
  int rc;
  auto& A = h->anderson;
  const int m = o.history;
  if ((rc = check_and_args(h, m, o.mixing_freq, AND_MAX_M))) return rc;
  if ((rc = ensure_buf(h, &h->buf0)) || (rc = ensure_buf(h, &h->buf1)) || (rc = ensure_scalars(h)) || (rc = ensure_tmp(h))) return rc;
  // passes per synchronisation: a multiple of the history length, so that the slot of pass i of a chunk is fixed
  int chunk = std::max(1, o.check_every);
  chunk = ((chunk + m - 1) / m) * m;
  // Small-grid plan: the push rides on T's last pass, the control step and the update of x on the first pass of the next
  // application (fast_kernels.hpp, SM_AND_LAST / SM_AND_FIRST): D/2 launches per pass instead of D/2 + 3.  The state
  // alternates between two buffers (even chunks end where they began) and the passes whose step can mix are fixed at
  // capture time (chunks are multiples of the mixing frequency).
  bool fusedp = !h->profiling && anderson_fused_ok(h, m);
  // large grids (the loop is HBM-bound there): the Gram matrix in one sweep where a solve is due (vec_kernels.hpp)
  const bool lazyp = h->knobs.and_fused && !fusedp && !h->sharded && m <= AND_LAZY_M && h->N >= (1LL << 21);
  if (lazyp) {
    const long long unit = lcm(lcm(m, o.mixing_freq), 2);
    chunk = (int)(((chunk + unit - 1) / unit) * unit);
    if ((rc = ensure_and_gram_partial(h))) return rc;
  }
  if (fusedp) {
    const long long unit = lcm(lcm(m, 2), o.mixing_freq);
    // (a chunk of this form ends with a launch of its own and the passes do not depend on the chunking: the default
    // polling interval is stretched, an explicit one is honoured)
    if (h->check_every_default) chunk = 120;
    if (unit > 4096) fusedp = false;
    else chunk = (int)(((chunk + unit - 1) / unit) * unit);      // (a chunk ends with one launch of its own: the longer the better)
  }
  if ((rc = ensure_and_state(h)) || (rc = ensure_and_slots(h, chunk))) return rc;
  AndPtrs hp;
  if ((rc = and_history(h, m, w, &hp))) return rc;
  const long long n = h->N;
  const int g = vec_grid(n);
  const size_t nb = sizeof(double) * (size_t)n;
  hipStream_t st = h->stream;
  double* x = h->buf0;
  double* fx = h->buf1;
  AndState* S = A.state;
  if ((rc = and_init_state(h, o.tol, o.max_iter, 2))) return rc;
  h->trace.clear();
  const int cvec = h->profiling ? counter_id(h, "anderson_blas1", 0, 0) : -1;
  // the end of every form of a chunk: the launches' error check, then errors, step kinds and the state go to the host
  auto read_back = [&](int count, const AndState* state) -> int {
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(A.err_host, A.err, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(A.kind_host, A.kind, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(A.state_host, state, sizeof(AndState), hipMemcpyDeviceToHost, st));
    return 0;
  };
  auto enqueue = [&](int count) -> int {
    HIPCHK(h, hipMemsetAsync(A.kind, 0, sizeof(int) * (size_t)chunk, st));
    for (int i = 0; i < count; ++i) {
      const int pos = i % m;                       // chunks start on multiples of m
      int r2 = apply_T_dev(h, x, fx, nullptr, &S->gate, 0.0);
      if (r2) return r2;
      ProfScope ps(h, cvec);
      hipLaunchKernelGGL(k_and_push, dim3(g), dim3(VEC_BLOCK), 0, st, (const double*)x, (const double*)fx, hp, m, pos, n, h->partial, (const unsigned long long*)&S->gate);
      hipLaunchKernelGGL(k_and_step, dim3(1), dim3(VEC_BLOCK), 0, st, (const double*)h->partial, g, m, pos, i, (const AndState*)S, S, A.err + i, A.kind + i,
                         o.tol, (double)o.max_iter, (int)o.mixing_freq, o.ridge);
      hipLaunchKernelGGL(k_and_mix_dev, dim3(g), dim3(VEC_BLOCK), 0, st, hp, (const AndState*)S, m, o.beta, x, (const double*)fx, pos, i, n);
    }
    return read_back(count, S);
  };
  // the fused form of a chunk: pass 0 starts from x as it stands, pass i > 0 opens with the step of pass i - 1; the step
  // and the update of the chunk's last pass are the two launches of the unfused form.  State of pass i: S[i & 1].
  auto enqueue_fused = [&](int count) -> int {
    HIPCHK(h, hipMemsetAsync(A.kind, 0, sizeof(int) * (size_t)chunk, st));
    HIPCHK(h, hipMemsetAsync(A.flag, 0, sizeof(unsigned) * (size_t)chunk, st));
    const int np = (int)h->fast.passes.size();
    const FastPass& PF = h->fast.passes[np - 1];
    const FastPass& PL = h->fast.passes[0];
    const int nbl = (int)small_grid(PL.sm, PL.wpt);
    AndStepPar par;
    par.tol = o.tol; par.max_iter = (double)o.max_iter; par.ridge = o.ridge; par.mixing_freq = (int)o.mixing_freq;
    for (int i = 0; i < count; ++i) {
      AndState* Si = S + (i & 1);
      SmallIO io;
      AndArgs an = and_args(hp, par, o.beta, m, nbl);
      // first pass
      memset(&io, 0, sizeof io);
      io.out = h->tmp;
      if (i == 0) {
        io.in = x; io.gate = &Si->gate;
        hipLaunchKernelGGL(small_variant(SM_FIRST_T, PF.r, PF.wpt), dim3(small_grid(PF.sm, PF.wpt)), dim3(256), 0, st, PF.sm, io);
      } else {
        io.in = fx;
        and_args_pass(an, h, i - 1, (i % (int)o.mixing_freq) == 0 ? 2 : (((i - 1) % (int)o.mixing_freq) == 0 ? 1 : 0), S, x);
        // (+ 1: the workgroup that writes the state)
        hipLaunchKernelGGL(small_and_variant(SM_AND_FIRST, PF.r, PF.wpt), dim3(small_grid(PF.sm, PF.wpt) + 1), dim3(256), 0, st, PF.sm, io, an);
      }
      for (int q = np - 2; q >= 1; --q) {
        const FastPass& PM = h->fast.passes[q];
        memset(&io, 0, sizeof io);
        io.in = h->tmp; io.out = h->tmp; io.gate = &Si->gate;
        hipLaunchKernelGGL(small_variant(SM_MID, PM.r, PM.wpt), dim3(small_grid(PM.sm, PM.wpt)), dim3(256), 0, st, PM.sm, io);
      }
      memset(&io, 0, sizeof io);
      io.in = h->tmp; io.out = fx; io.old = x; io.gate = &Si->gate;
      and_args_pass(an, h, i, 0, nullptr, nullptr);
      hipLaunchKernelGGL(small_and_variant(SM_AND_LAST, PL.r, PL.wpt), dim3(nbl), dim3(256), 0, st, PL.sm, io, an);
    }
    const int lastp = count - 1;
    AndArgs an = and_args(hp, par, o.beta, m, nbl);
    and_args_pass(an, h, lastp, 2, S, x);
    hipLaunchKernelGGL(small_and_finish, dim3((unsigned)std::min<long long>((n + 255) / 256, 512)), dim3(256), 0, st, an, (const double*)fx, n);
    return read_back(count, S + (count & 1));
  };
  // Large grids: <r, r> per pass, the whole Gram matrix in one sweep where a solve is due, history as Y_j (vec_kernels.hpp)
  auto enqueue_lazy = [&](int count) -> int {
    HIPCHK(h, hipMemsetAsync(A.kind, 0, sizeof(int) * (size_t)chunk, st));
    const AndRun run{n, m, (int)o.mixing_freq, o.tol, (double)o.max_iter, o.beta, o.ridge, hp};
    for (int i = 0; i < count; ++i) {
      const int pos = i % m;
      // the iterate alternates between the two buffers (chunks are even): a plain step x = T x is then no copy at all,
      // a mixing step writes over T x, which the push has consumed
      double* const xi = (i & 1) ? fx : x;
      double* const xo = (i & 1) ? x : fx;
      // the push rides on T's last pass where that is the streamed form (stream_kernels.hpp, LineIO::and_*): x is read
      // once, T x is not read back -- 9 grid streams per pass instead of 10, on a pass that is bound by its power, not its bytes
      long long ptiles = 0;
      Apply a(MODE_T, xi, xo, xi);
      a.gate = &S->gate;
      if (!h->knobs.no_and_push_fusion) {
        a.push.y = hp.X[pos]; a.push.r = hp.R[pos]; a.push.beta = o.beta; a.push.dot = h->partial; a.push.tiles = &ptiles;
      }
      if (int r2 = apply(h, a)) return r2;
      ProfScope ps(h, cvec);
      if (ptiles == 0) and_push_lite(h, run, pos, xi, xo, nullptr);
      const int gpush = ptiles ? (int)ptiles : g;
      const int refresh = ((i + 1) % (int)o.mixing_freq) == 0 ? 1 : 0;
      if (refresh) and_gram_full(h, run, nullptr);
      and_step_lazy(h, run, h->partial, gpush, A.gram_partial, and_gram_blocks(n), refresh, pos, i, i);
      and_mix_y(h, run, xo, pos, i);
    }
    return read_back(count, S);
  };
  auto enqueue_any = [&](int count) -> int { return fusedp ? enqueue_fused(count) : (lazyp ? enqueue_lazy(count) : enqueue(count)); };
  const bool graph = o.use_graph && !h->profiling && st != nullptr && chunk > 1;
  const double key[4] = {o.tol, (double)o.max_iter, o.beta, o.ridge};
  if (graph && (A.graph == nullptr || A.graph_chunk != chunk || A.graph_m != m || A.graph_freq != (int)o.mixing_freq ||
                memcmp(key, A.graph_key, sizeof key) != 0)) {
    if ((rc = capture_graph(h, &A.graph, [&] { return enqueue_any(chunk); }))) return rc;
    A.graph_chunk = chunk; A.graph_m = m; A.graph_freq = (int)o.mixing_freq;
    memcpy(A.graph_key, key, sizeof key);
  }
  long long enq = 0;          // passes enqueued so far (a multiple of chunk while the loop runs)
  bool running = A.state_host->gate != 0ULL;
  while (running && enq < o.max_iter) {
    const int count = (int)std::min<long long>(chunk, o.max_iter - enq);
    if (graph && count == chunk) { HIPCHK(h, hipGraphLaunch(A.graph, st)); }
    else if ((rc = enqueue_any(count))) return rc;
    HIPCHK(h, hipStreamSynchronize(st));
    enq += count;
    if (o.record_errors)
      for (int i = 0; i < count; ++i) if (A.kind_host[i] == 1) h->trace.push_back(A.err_host[i]);
    running = A.state_host->gate != 0ULL;
  }
  const AndState& F = *A.state_host;
  const long long it = (long long)F.it;
  const double err = F.err;
  // (batched-Gram loop: pass i leaves the iterate in buffer (i + 1) & 1)
  HIPCHK(h, hipMemcpyAsync(w, (lazyp && (it & 1)) ? fx : x, nb, hipMemcpyDeviceToDevice, st));
  HIPCHK(h, hipStreamSynchronize(st));
  *n_iter = it; *n_apply = it; *final_err = err;
  if (F.status != 0.0) return fail(h, SDFS_ERR_NUMERIC, "non-finite Anderson residual at iteration %lld", it);
  return 0;
}

constexpr int DAND_SLOTS = 256;       // sharded step API: error ring (one slot per pass, read back by sdfs_anderson_state)
static_assert(AND_LAZY_PAIRS == SDFS_AND_NPAIRS, "include/sdfs_hip.h states the length of the Gram sums");

}  // namespace

// ---- Anderson acceleration on a sharded grid: the single-GPU loop's batched-Gram kernels on this rank's shard -----------
extern "C" {

int sdfs_anderson_begin(sdfs_handle* h, int64_t n, int history, double* y_hist_dev, double* r_hist_dev, double tol,
                        int64_t max_iter, double beta, double ridge, int mixing_freq) {
  int rc = check(h); if (rc) return rc;
  if (n < 1 || !y_hist_dev || !r_hist_dev) return fail(h, SDFS_ERR_ARG, "bad argument");
  if ((rc = check_and_args(h, history, mixing_freq, AND_LAZY_M))) return rc;
  if ((n & 1) && history > 0 && ((uintptr_t)r_hist_dev % 16 != 0)) return fail(h, SDFS_ERR_ARG, "history buffers must be 16-byte aligned");
  if ((rc = ensure_scalars(h)) || (rc = ensure_and_state(h)) || (rc = ensure_and_slots(h, DAND_SLOTS)) || (rc = ensure_and_gram_partial(h))) return rc;
  auto& D = h->anderson.dand;
  D.on = true; D.n = n; D.m = history; D.mixing_freq = mixing_freq; D.tol = tol; D.max_iter = (double)max_iter; D.beta = beta; D.ridge = ridge;
  D.hp = and_ptrs(history, [&](int j) { return y_hist_dev + (size_t)j * (size_t)n; }, [&](int j) { return r_hist_dev + (size_t)j * (size_t)n; });
  hipStream_t st = h->stream;
  HIPCHK(h, hipMemsetAsync(r_hist_dev, 0, sizeof(double) * (size_t)history * (size_t)n, st));
  HIPCHK(h, hipMemsetAsync(h->anderson.kind, 0, sizeof(int) * DAND_SLOTS, st));
  return and_init_state(h, tol, max_iter, 1);
}

int sdfs_anderson_gate(sdfs_handle* h, const void** gate_dev) {
  int rc = check(h); if (rc) return rc;
  if (!gate_dev || !h->anderson.dand.on) return fail(h, SDFS_ERR_ARG, "sdfs_anderson_begin first");
  *gate_dev = &h->anderson.state->gate;
  return 0;
}

int sdfs_anderson_step(sdfs_handle* h, int step, int64_t pass, const double* x_in, double* x_out, double* sums_dev) {
  int rc = check(h); if (rc) return rc;
  const auto& D = h->anderson.dand;
  if (!D.on) return fail(h, SDFS_ERR_ARG, "sdfs_anderson_begin first");
  if (pass < 0 || !sums_dev) return fail(h, SDFS_ERR_ARG, "bad argument");
  const int pos = (int)(pass % D.m), slot = (int)(pass % DAND_SLOTS), rel = (int)(pass & 0x3fffffff);
  switch (step) {
    case SDFS_AND_PUSH:       // Y[pos] = x + beta r, R[pos] = r = x_out - x_in, sums[0] = this rank's <r, r>
      if (!x_in || !x_out) return fail(h, SDFS_ERR_ARG, "NULL iterate");
      and_push_lite(h, D, pos, x_in, x_out, sums_dev);
      break;
    case SDFS_AND_GRAM:       // sums[1 ..] = this rank's part of the whole Gram matrix (pairs i <= j in k_and_gram_full's order)
      and_gram_full(h, D, sums_dev + 1);
      break;
    case SDFS_AND_STEP:       // the control step from the all-reduced sums (nb = 0: totals, not partials)
      and_step_lazy(h, D, sums_dev, 0, sums_dev + 1, 1, ((pass + 1) % D.mixing_freq) == 0 ? 1 : 0, pos, rel, slot);
      break;
    case SDFS_AND_MIX:        // the update of x the step decided on, in place in x_out (= T x_in on entry)
      if (!x_out) return fail(h, SDFS_ERR_ARG, "NULL iterate");
      and_mix_y(h, D, x_out, pos, rel);
      break;
    default:
      return fail(h, SDFS_ERR_ARG, "unknown Anderson step %d", step);
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

int sdfs_anderson_state(sdfs_handle* h, double* out8_host, double* errs_host, int64_t first_pass, int64_t count) {
  int rc = check(h); if (rc) return rc;
  auto& A = h->anderson;
  if (!A.dand.on || !out8_host) return fail(h, SDFS_ERR_ARG, "sdfs_anderson_begin first");
  if (count < 0 || count > DAND_SLOTS || first_pass < 0 || (count > 0 && !errs_host)) return fail(h, SDFS_ERR_ARG, "bad error window");
  hipStream_t st = h->stream;
  HIPCHK(h, hipMemcpyAsync(A.state_host, A.state, sizeof(AndState), hipMemcpyDeviceToHost, st));
  if (count > 0) HIPCHK(h, hipMemcpyAsync(A.err_host, A.err, sizeof(double) * DAND_SLOTS, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  const AndState& F = *A.state_host;
  out8_host[0] = F.it; out8_host[1] = F.err; out8_host[2] = F.gate != 0ULL ? 1.0 : 0.0; out8_host[3] = F.status;
  out8_host[4] = F.rejected; out8_host[5] = F.no_mix_until; out8_host[6] = F.last_mixed; out8_host[7] = F.prev_pos;
  for (int64_t i = 0; i < count; ++i) errs_host[i] = A.err_host[(first_pass + i) % DAND_SLOTS];
  return 0;
}

}  // extern "C"

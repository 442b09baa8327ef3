// cont_adjoint.hpp -- the transposed Jacobian of the continuous-state operator and the adjoint solve on it
// (sdfs_cont_apply_vjp_dev, sdfs_cont_solve_adjoint_dev).
//
// Not a header of its own: sdfs_api.hip includes it once, after cont_sens.hpp, and it uses sdfs_handle, Apply, apply,
// linear_solve, check, fail and cont_handle_ok of those files.
//
// J^T u is one launch of the C_VJP form of cont_kernel.hpp, which cont_vjp.hip instantiates (a translation unit of its
// own; that file says why) and cont_vjp_launch starts behind the in-stream zeroing of the output.  run_cont
// (sdfs_api.hip) calls it for a MODE_VJP request, so the device BiCGSTAB's transposed iteration serves the adjoint solve.
//
// The form accumulates with hardware fp64 atomic adds: THE LAST BITS OF ITS RESULT DEPEND ON THE ORDER IN WHICH THE ADDS
// ARRIVE.  These two entry points are the library's only ones whose results are reproducible to rounding, not to the bit.
// The discretised handles' sdfs_apply_vjp_dev / sdfs_solve_linear_dev(transpose = 1) keep refusing continuous handles.
#pragma once

#include <hip/hip_runtime.h>

#include "cont_kernel.hpp"

extern "C" {

int sdfs_cont_apply_vjp_dev(sdfs_handle* h, const double* u, double* out, int minus_identity) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_handle_ok(h, "sdfs_cont_apply_vjp_dev"))) return rc;
  if (!u || !out) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  if (u == out) return fail(h, SDFS_ERR_ARG, "the continuous operator cannot run in place");
  if (!h->c1 || !h->c2 || h->lin_stale) return fail(h, SDFS_ERR_ARG, "sdfs_cont_apply_vjp_dev before a linearisation (sdfs_linearize_dev, "
                                    "sdfs_cont_param_tangent_dev)");
  Apply a(MODE_VJP, u, out, u);
  a.minus_identity = minus_identity;
  return apply(h, a);
}

int sdfs_cont_solve_adjoint_dev(sdfs_handle* h, const sdfs_opts* opts, const double* rhs, double* x, int64_t* n_iter,
                                double* final_rel_resid) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_handle_ok(h, "sdfs_cont_solve_adjoint_dev"))) return rc;
  if (!rhs || !x) return fail(h, SDFS_ERR_ARG, "NULL grid pointer");
  if (!h->c1 || !h->c2 || h->lin_stale) return fail(h, SDFS_ERR_ARG, "sdfs_cont_solve_adjoint_dev before a linearisation (sdfs_linearize_dev, "
                                    "sdfs_cont_param_tangent_dev)");
  sdfs_opts o;
  if (opts) o = *opts; else sdfs_default_opts(&o);
  if (o.krylov_f32 != 0) return fail(h, SDFS_ERR_ARG, "sdfs_cont_solve_adjoint_dev is fp64 only (opts.krylov_f32 = %d)", o.krylov_f32);
  return linear_solve(h, o, MODE_VJP, rhs, x, n_iter, final_rel_resid, nullptr, nullptr, "adjoint");
}

}  // extern "C"

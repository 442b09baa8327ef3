// cont_sens.hpp -- the parameter tangent of the continuous-state operator (sdfs_cont_param_tangent_dev).
//
// Not a header of its own: sdfs_api.hip includes it once, after cont_price.hpp, and it uses sdfs_handle, launch_kernel,
// counter_id, ProfScope, check, fail, ensure_lin and cont_handle_ok of those files.
//
// What is differentiated is T(w; p) of the handle with its grids, nodes and weights held fixed -- jax.jvp of the
// reference's T with respect to the parameter vector, `grids, nodes, weights` closed over.  build_grid also depends on the
// parameters; the movement of the grid is NOT part of this derivative.
//
// The work is one launch of the C_PTAN form of cont_kernel.hpp, which cont_ptan.hip instantiates (a translation unit of
// its own; that file says why) and cont_ptan_launch starts.  Like sdfs_param_tangent_dev on a discretised handle the
// call linearises at w (c1 = w, c2 = beta C u / Kg, lin_stale cleared), so sdfs_solve_linear_dev can follow directly:
// dw*/dp = (I - J(w*))^{-1} dT/dp, one BiCGSTAB solve per parameter, the persistences included.
#pragma once

#include <hip/hip_runtime.h>

#include "cont_kernel.hpp"

extern "C++" {
namespace sdfs {
hipError_t cont_ptan_launch(hipStream_t stream, const ContDesc& cd, const ContIO& io, const ContTan& tan, int log_from_pow);   // cont_ptan.hip
}
namespace {
// ln g per node: 1 = from the power's own log2 (C_PTANL), 0 = libm's log (C_PTAN); SDFS_PTAN_LOG_FROM_POW overrides, read
// at every call (the A/B of tools/continuous_sensitivity_times.py)
constexpr int CONT_PTAN_LOG_FROM_POW = 1;      // (0.85 - 0.92 of the time with libm's log: profiles/continuous_sensitivity_times.txt)

// dparams in sdfs_create_continuous's parameter order -> the direction in the descriptor's terms
sdfs::ContTan cont_direction(const sdfs_handle* h, const double* q) {
  sdfs::ContTan t;
  memset(&t, 0, sizeof t);
  double dgamma, dpsi;
  if (h->model == SDFS_MODEL_SSY) {
    // beta, gamma, psi, mu_c, rho, phi_z, phi_c, rho_z, rho_c, rho_lam, s_z, s_c, s_lam; dims h_lam, h_c, h_z, z
    t.beta = q[0]; dgamma = q[1]; dpsi = q[2]; t.mu_c = q[3]; t.phi_c = q[6];
    t.rho[0] = q[9]; t.sconst[0] = q[12];
    t.rho[1] = q[8]; t.sconst[1] = q[11];
    t.rho[2] = q[7]; t.sconst[2] = q[10];
    t.rho[3] = q[4]; t.phi[3] = q[5];
  } else {
    // beta, psi, gamma, rho_lam, s_lam, mu_c, phi_c, rho, rho_pi, phi_z, rho_c, s_c, rho_z, s_z, rho_pipi, phi_zpi, rho_zpi,
    // s_zpi; dims h_lam, h_c, h_z, h_zpi, z, z_pi
    t.beta = q[0]; dpsi = q[1]; dgamma = q[2]; t.mu_c = q[5]; t.phi_c = q[6];
    t.rho[0] = q[3]; t.sconst[0] = q[4];
    t.rho[1] = q[10]; t.sconst[1] = q[11];
    t.rho[2] = q[12]; t.sconst[2] = q[13];
    t.rho[3] = q[16]; t.sconst[3] = q[17];
    t.rho[4] = q[7]; t.xcoef[4] = q[8]; t.phi[4] = q[9];
    t.rho[5] = q[14]; t.phi[5] = q[15];
  }
  // theta = (1 - gamma) psi / (psi - 1)
  const double psi = h->cont_psi, pm1 = psi - 1.0;
  t.gamma = dgamma;
  t.theta = -dgamma * psi / pm1 - dpsi * (1.0 - h->cont_gamma) / (pm1 * pm1);
  return t;
}
}  // namespace
}  // extern "C++"

extern "C" {

int sdfs_cont_param_tangent_dev(sdfs_handle* h, const double* w, const double* dparams, double* out, double* Tw) {
  int rc = check(h); if (rc) return rc;
  if ((rc = cont_handle_ok(h, "sdfs_cont_param_tangent_dev"))) return rc;
  if (!w || !dparams || !out) return fail(h, SDFS_ERR_ARG, "NULL argument");
  if (out == w || Tw == w || Tw == out) return fail(h, SDFS_ERR_ARG, "w, out and Tw: distinct grids");
  const int np = h->model == SDFS_MODEL_SSY ? 13 : 18;
  for (int i = 0; i < np; ++i)
    if (!std::isfinite(dparams[i])) return fail(h, SDFS_ERR_ARG, "dparams[%d] is not finite", i);
  if ((rc = ensure_lin(h))) return rc;
  const sdfs::ContDesc& cd = h->cd;
  sdfs::ContTan t = cont_direction(h, dparams);
  t.Tw = Tw;
  h->lin_stale = true;                     // (until the launch below is in place)
  // keep the linearisation point, as MODE_T_LIN does (run_cont): J.v re-evaluates interp(w)^(theta-1) at every node
  HIPCHK(h, hipMemcpyAsync(h->c1, w, (size_t)cd.N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  sdfs::ContIO io;
  memset(&io, 0, sizeof io);
  io.w = w; io.out = out; io.c2_out = h->c2;
  const double n8 = 8.0 * (double)cd.N;
  const int cid = h->profiling ? counter_id(h, "cont:ptan", (Tw ? 5 : 4) * n8,
                                            (double)cd.N * cd.M * (3.0 * (double)(1 << cd.D) + 4.0 * cd.D + 8.0)) : -1;
  {
    ProfScope ps(h, cid);
    HIPCHK(h, sdfs::cont_ptan_launch(h->stream, cd, io, t, env_int("SDFS_PTAN_LOG_FROM_POW", CONT_PTAN_LOG_FROM_POW)));
  }
  h->lin_stale = false;
  return 0;
}

}  // extern "C"

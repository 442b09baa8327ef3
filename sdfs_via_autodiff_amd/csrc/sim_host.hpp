// sim_host.hpp -- host side of the path simulators (sdfs_sim_paths_dev, sdfs_batch_sim_paths_dev, sdfs_cont_sim_paths_dev):
// the range checks of a request and the layout of SimArgs' LDS table (cumulative rows, marginals, h_lambda, sigma_c).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "sim_kernels.hpp"

// The path numbers and step numbers of a request.  step_offset: nullptr where the call has none; margin: the step numbers
// kept free below 2^32 (the batch keeps 8, the single-problem calls none).  false, and the message, where they leave their ranges.
inline bool sim_ranges_ok(char (&msg)[160], long long path_offset, long long n_paths, const int64_t* step_offset, long long burn_in,
                          long long n_periods, int margin) {
  if (n_paths < 1 || path_offset < 0 || path_offset + n_paths > (1LL << 32)) {
    snprintf(msg, sizeof msg, "paths %lld ... %lld: numbers lie in 0 ... 2^32 - 1", path_offset, path_offset + n_paths - 1);
    return false;
  }
  const long long s0 = step_offset ? (long long)*step_offset : 0;
  if (n_periods >= 2 && burn_in >= 0 && s0 >= 0 && s0 + burn_in + n_periods < (1LL << 32) - margin) return true;
  if (step_offset)
    snprintf(msg, sizeof msg, "step_offset = %lld, burn_in = %lld, n_periods = %lld: T >= 2 and s0 + B + T < 2^32", s0, burn_in, n_periods);
  else if (margin)
    snprintf(msg, sizeof msg, "burn_in = %lld, n_periods = %lld: T >= 2 and B + T < 2^32 - %d", burn_in, n_periods, margin);
  else
    snprintf(msg, sizeof msg, "burn_in = %lld, n_periods = %lld: T >= 2 and B + T < 2^32", burn_in, n_periods);
  return false;
}

// The offsets of one table block and the words of the request d (an sdfs_sim_desc or an sdfs_batch_sim_desc) into `a`; *ncdf,
// *ncdf0: doubles of the rows and of the marginals of one block.  Returns the axis of a start index that is no state, or -1.
template <class Desc>
int sim_layout(int ndim, const int* n, const int* stride, int ax_lam, int ax_c, const Desc* d, SimArgs& a, int* ncdf, int* ncdf0) {
  int off = 0, bad = -1;
  for (int ax = 0; ax < ndim; ++ax) {
    a.n[ax] = n[ax]; a.stride[ax] = stride[ax];
    a.cdf_off[ax] = off; off += n[ax] * n[ax];
    if (d->start_fixed && (d->start[ax] < 0 || d->start[ax] >= n[ax]) && bad < 0) bad = ax;
    a.start[ax] = d->start_fixed ? d->start[ax] : 0;
  }
  *ncdf = off; *ncdf0 = 0;
  for (int ax = 0; ax < ndim; ++ax) { a.cdf0_off[ax] = off; off += n[ax]; *ncdf0 += n[ax]; }
  a.ax_lam = ax_lam; a.ax_c = ax_c;
  a.hl_off = off; off += n[ax_lam];
  a.sc_off = off; off += n[ax_c];
  a.lds_n = off;
  a.start_fixed = d->start_fixed ? 1 : 0;
  a.key0 = (unsigned)(d->seed & 0xffffffffu); a.key1 = (unsigned)(d->seed >> 32);
  a.path0 = (unsigned long long)d->path_offset; a.n_paths = d->n_paths;
  a.burn_in = (unsigned)d->burn_in; a.n_periods = (unsigned)d->n_periods;
  return bad;
}

// one block at t in that layout; cdf0 == nullptr (a fixed start): the marginals are 2.0 fillers
inline void sim_fill_table(const SimArgs& a, int ncdf, int ncdf0, const double* cdf, const double* cdf0, const double* hlam,
                           const double* sigc, double* t) {
  std::copy(cdf, cdf + ncdf, t);
  if (cdf0) std::copy(cdf0, cdf0 + ncdf0, t + ncdf);
  else std::fill(t + ncdf, t + ncdf + ncdf0, 2.0);
  std::copy(hlam, hlam + a.n[a.ax_lam], t + a.hl_off);
  std::copy(sigc, sigc + a.n[a.ax_c], t + a.sc_off);
}

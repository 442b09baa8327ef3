// cont_vjp.hip -- the C_VJP form of cont_kernel (cont_kernel.hpp) in a translation unit of its own, for the
// reason cont_ptan.hip gives: compiled here, the new form leaves the register allocation of every other kernel of the
// library exactly as it was.  sdfs_api.hip reaches it through cont_vjp_launch (run_cont's MODE_VJP branch), which owns the
// grid, the block and the LDS size of the form, the initialisation of the output and the "- u" of minus_identity.
//
// The form accumulates with hardware fp64 atomic adds (unsafeAtomicAdd: ds_add_f64 on the LDS accumulators,
// global_atomic_add_f64 on out; no compare-and-swap loop), so its result is reproducible to rounding only and out must be
// ordinary (coarse-grained) device memory.
#include <hip/hip_runtime.h>

#define SDFS_NO_DEBUG_POW_KERNEL                // (pass_kernel.hpp's one non-template kernel belongs to sdfs_api.hip)
#include "cont_kernel.hpp"

namespace sdfs {

// SUB = false: out = 0, what the atomic adds of the C_VJP form start from.  SUB = true: out -= u, behind the form.
// minus_identity is this second pass and not a start from -u: J^T u - u is then one rounding away from J^T u, whatever
// the number of adds, and small contributions are not rounded against a large u one by one.  Gated like the form itself.
template <bool SUB>
__global__ void __launch_bounds__(256) k_cont_vjp_edge(const double* __restrict__ u, double* __restrict__ out, long long n,
                                                       const unsigned long long* gate, double gate_tol) {
  if (gate != nullptr) {
    const unsigned long long g = *gate;
    if (g <= (unsigned long long)__double_as_longlong(gate_tol)) return;
  }
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = SUB ? out[i] - u[i] : 0.0;
}

hipError_t cont_vjp_launch(hipStream_t stream, const ContDesc& cd, const ContIO& io) {
  const dim3 grid((unsigned)cd.N), block(256), vgrid((unsigned)((cd.N + 255) / 256));
  hipLaunchKernelGGL(k_cont_vjp_edge<false>, vgrid, block, 0, stream, io.v, io.out, cd.N, io.gate, io.gate_tol);
  // the two-field forms' LDS: the box and its pre-contracted form, each beside its accumulator
  const size_t lds = 2 * (size_t)(cd.cap + cd.ucap) * sizeof(double);
  if (cd.D == 4) hipLaunchKernelGGL((cont_kernel<4, C_VJP>), grid, block, lds, stream, cd, io, ContNoTan{});
  else hipLaunchKernelGGL((cont_kernel<6, C_VJP>), grid, block, lds, stream, cd, io, ContNoTan{});
  if (io.minus_identity)
    hipLaunchKernelGGL(k_cont_vjp_edge<true>, vgrid, block, 0, stream, io.v, io.out, cd.N, io.gate, io.gate_tol);
  return hipGetLastError();
}

}  // namespace sdfs

// cont_ptan.hip -- the C_PTAN / C_PTANL forms of cont_kernel (cont_kernel.hpp) in a translation unit of
// their own.
//
// Instantiated beside the library's other kernels in sdfs_api.hip, the tangent form moved the register allocation of 36
// kernels that share no code with it (-Rpass-analysis=kernel-resource-usage: line_stream_kernel<20, ...> 128 -> 134 VGPRs
// and occupancy 4 -> 3, line_kernel<32, ...> 122 -> 132 and 4 -> 3, pass_kernel, slice_kernel and others by a few
// registers).  Compiled here, it leaves every other kernel of the library exactly as it was.  sdfs_api.hip reaches it
// through cont_ptan_launch (cont_sens.hpp), which owns the grid, the block and the LDS size of the form.
#include <hip/hip_runtime.h>

#define SDFS_NO_DEBUG_POW_KERNEL                // (pass_kernel.hpp's one non-template kernel belongs to sdfs_api.hip)
#include "cont_kernel.hpp"

namespace sdfs {

hipError_t cont_ptan_launch(hipStream_t stream, const ContDesc& cd, const ContIO& io, const ContTan& tan, int log_from_pow) {
  const dim3 grid((unsigned)cd.N), block(256);
  // T's box, its pre-contracted form and the tangent of that form
  const size_t lds = (size_t)(cd.cap + 2 * cd.ucap) * sizeof(double);
  if (log_from_pow) {
    if (cd.D == 4) hipLaunchKernelGGL((cont_kernel<4, C_PTANL>), grid, block, lds, stream, cd, io, tan);
    else hipLaunchKernelGGL((cont_kernel<6, C_PTANL>), grid, block, lds, stream, cd, io, tan);
  } else {
    if (cd.D == 4) hipLaunchKernelGGL((cont_kernel<4, C_PTAN>), grid, block, lds, stream, cd, io, tan);
    else hipLaunchKernelGGL((cont_kernel<6, C_PTAN>), grid, block, lds, stream, cd, io, tan);
  }
  return hipGetLastError();
}

}  // namespace sdfs

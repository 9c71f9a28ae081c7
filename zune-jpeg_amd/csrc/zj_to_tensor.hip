// zj_to_tensor.hip -- gfx950 kernel of the u8-images-to-tensor stage (zj_to_tensor_device) and its launcher.
//
//   zj_to_tensor_kernel   u8 images of one size, their own bases and pitches -> consecutive images of a normalised tensor
// ONE kernel: dtype, layout, flip and the channel counts are run-time switches, uniform over a workgroup.  A translation
// unit of its own: every other kernel keeps its code object instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_to_tensor.h"
#include "zj_to_tensor_launch.h"

namespace zj {

// One lane per aligned block of TT_RUN tensor elements: blockIdx.x x TT_NT + threadIdx.x counts the blocks of image
// blockIdx.z row by row, run by run.
__global__ __launch_bounds__(TT_NT) void zj_to_tensor_kernel(const ToTensorParams p)
{
    tt_lane(p, (int)blockIdx.z, blockIdx.x * (uint32_t)TT_NT + threadIdx.x);
}

hipError_t launch_to_tensor(const ToTensorParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > TT_BATCH || p.w <= 0 || p.h <= 0 || p.w > 65535 || p.h > 65535) return hipErrorInvalidValue;
    if (!((p.cin == 1 && (p.cout == 1 || p.cout == 3)) || (p.cin == 3 && p.cout == 3)) || !resize_elem_bytes(p.dtype))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)tt_grid(p), 1, (unsigned)p.nimg);
    hipLaunchKernelGGL(zj_to_tensor_kernel, grid, dim3(TT_NT), 0, s, p);
    return hipGetLastError();
}

} // namespace zj

// zj_warp.hip -- gfx950 kernels of the affine-warp stage (zj_warp_device) and their launcher.
//
//   zj_warp_kernel<C>   u8 images of their own sizes, each under its own inverse affine map -> consecutive images of a
//                       normalised tensor
// One kernel per channel count: dtype, layout and edge mode are run-time switches, uniform over a workgroup.  A translation
// unit of its own: every other kernel keeps its code object instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_warp.h"
#include "zj_warp_launch.h"

namespace zj {

// One workgroup per block of WARP_BX groups x WARP_BY rows of image blockIdx.z; a lane gathers the taps of its group's
// pixels byte by byte through the vector L1 and stores the group.
template <int C>
__global__ __launch_bounds__(WARP_NT) void zj_warp_kernel(const WarpParams p)
{
    warp_lane<C>(p, (int)blockIdx.z, blockIdx.x, blockIdx.y, threadIdx.x);
}

hipError_t launch_warp(int channels, const WarpParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > WARP_BATCH || p.out_w <= 0 || p.out_h <= 0 || p.out_w > RESIZE_MAX_OUT || p.out_h > RESIZE_MAX_OUT)
        return hipErrorInvalidValue;
    if ((channels != 1 && channels != 3) || !resize_elem_bytes(p.dtype) || (p.edge != WARP_FILL && p.edge != WARP_REPLICATE))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)warp_grid_x(p.out_w), (unsigned)warp_grid_y(p.out_h), (unsigned)p.nimg);
    if (channels == 1) hipLaunchKernelGGL(zj_warp_kernel<1>, grid, dim3(WARP_NT), 0, s, p);
    else hipLaunchKernelGGL(zj_warp_kernel<3>, grid, dim3(WARP_NT), 0, s, p);
    return hipGetLastError();
}

} // namespace zj

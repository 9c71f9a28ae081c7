// zj_expand.hip -- gfx950 kernel of the gray-to-RGB stage (zj_gray_to_rgb_device) and its launcher.
//
//   zj_gray_expand_kernel<OUT_CHW>   u8 planes of their own sizes and pitches -> 3-channel u8 images, every channel the plane
// A translation unit of its own: the fused, crop, scaled, orient and resize kernels keep their code objects instruction for
// instruction.
#include <hip/hip_runtime.h>

#include "zj_expand.h"
#include "zj_expand_launch.h"

namespace zj {

// One lane per run of EXPAND_RUN pixels of a row: blockIdx.x x EXPAND_NT + threadIdx.x counts the runs of image blockIdx.z row
// by row.  The grid is sized for the launch's largest image; the lanes beyond a smaller one leave at once.
template <bool OUT_CHW>
__global__ __launch_bounds__(EXPAND_NT) void zj_gray_expand_kernel(const ExpandParams p)
{
    expand_lane<OUT_CHW>(p, (int)blockIdx.z, blockIdx.x * (uint32_t)EXPAND_NT + threadIdx.x);
}

hipError_t launch_expand(int out_chw, const ExpandParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > EXPAND_BATCH) return hipErrorInvalidValue;
    for (int i = 0; i < p.nimg; i++)
        if ((p.wh[i] & 0xffffu) == 0 || (p.wh[i] >> 16) == 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)expand_grid(p), 1, (unsigned)p.nimg);
    if (out_chw) hipLaunchKernelGGL((zj_gray_expand_kernel<true>), grid, dim3(EXPAND_NT), 0, s, p);
    else hipLaunchKernelGGL((zj_gray_expand_kernel<false>), grid, dim3(EXPAND_NT), 0, s, p);
    return hipGetLastError();
}

} // namespace zj

// zj_cmyk.hip -- gfx950 kernel of the CMYK-to-RGB stage (zj_cmyk_to_rgb_device) and its launcher.
//
//   zj_cmyk_combine_kernel<CHW>   3-channel u8 images and u8 planes of their own sizes and pitches -> 3-channel u8 images,
//                                 out[c] = (a[c] * k + 127) / 255, the samples complemented first where the image says so
// A translation unit of its own: the fused, crop, scaled, orient, expand and resize kernels keep their code objects
// instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_cmyk.h"
#include "zj_cmyk_launch.h"

namespace zj {

// One lane per run of CMYK_RUN pixels of a row: blockIdx.x x CMYK_NT + threadIdx.x counts the runs of image blockIdx.z row by
// row.  The grid is sized for the launch's largest image; the lanes beyond a smaller one leave at once.
template <bool CHW>
__global__ __launch_bounds__(CMYK_NT) void zj_cmyk_combine_kernel(const CmykParams p)
{
    cmyk_lane<CHW>(p, (int)blockIdx.z, blockIdx.x * (uint32_t)CMYK_NT + threadIdx.x);
}

hipError_t launch_cmyk(int chw, const CmykParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > CMYK_BATCH) return hipErrorInvalidValue;
    for (int i = 0; i < p.nimg; i++)
        if ((p.wh[i] & 0xffffu) == 0 || (p.wh[i] >> 16) == 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)cmyk_grid(p), 1, (unsigned)p.nimg);
    if (chw) hipLaunchKernelGGL((zj_cmyk_combine_kernel<true>), grid, dim3(CMYK_NT), 0, s, p);
    else hipLaunchKernelGGL((zj_cmyk_combine_kernel<false>), grid, dim3(CMYK_NT), 0, s, p);
    return hipGetLastError();
}

} // namespace zj

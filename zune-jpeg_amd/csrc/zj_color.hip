// zj_color.hip -- gfx950 kernel of the colour-matrix stage (zj_color_device) and its launcher.
//
//   zj_color_kernel<CHW>   3-channel u8 images of their own sizes and pitches -> 3-channel u8 images,
//                          out[c] = clamp((q[c][0] R + q[c][1] G + q[c][2] B + q[c][3] + 32768) >> 16, 0, 255)
// A translation unit of its own: the other kernels keep their code objects instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_color.h"
#include "zj_color_launch.h"

namespace zj {

// One lane per run of COLOR_RUN pixels of a row: blockIdx.x x COLOR_NT + threadIdx.x counts the runs of image blockIdx.z row
// by row.  The grid is sized for the launch's largest image; the lanes beyond a smaller one leave at once.  blockIdx.z is the
// same over a workgroup: the image's record, its 12 integers among it, is read with scalar loads.
template <bool CHW>
__global__ __launch_bounds__(COLOR_NT) void zj_color_kernel(const ColorParams p)
{
    color_lane<CHW>(p, (int)blockIdx.z, blockIdx.x * (uint32_t)COLOR_NT + threadIdx.x);
}

hipError_t launch_color(int chw, const ColorParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > COLOR_BATCH) return hipErrorInvalidValue;
    for (int i = 0; i < p.nimg; i++)
        if ((p.wh[i] & 0xffffu) == 0 || (p.wh[i] >> 16) == 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)color_grid(p), 1, (unsigned)p.nimg);
    if (chw) hipLaunchKernelGGL((zj_color_kernel<true>), grid, dim3(COLOR_NT), 0, s, p);
    else hipLaunchKernelGGL((zj_color_kernel<false>), grid, dim3(COLOR_NT), 0, s, p);
    return hipGetLastError();
}

} // namespace zj

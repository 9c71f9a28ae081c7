// zj_planes.hip -- gfx950 kernel of the planes-to-RGB stage (zj_planes_to_rgb_device) and its launcher.
//
//   zj_planes_combine_kernel<CHW, STORED_RGB>   three u8 component planes per image, each at its own resolution (ratios 1, 2
//                                               or 4 each way, any phase) -> 3-channel u8 images: the samples box-replicated
//                                               and run through the full decode's YCbCr -> RGB (STORED_RGB: as they are)
// A translation unit of its own: the fused, crop, scaled, orient, expand, cmyk and resize kernels keep their code objects
// instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_planes.h"
#include "zj_planes_launch.h"

namespace zj {

// One lane per run of PLANES_RUN pixels of a row: blockIdx.x x PLANES_NT + threadIdx.x counts the runs of image blockIdx.z
// row by row.  The grid is sized for the launch's largest image; the lanes beyond a smaller one leave at once.
template <bool CHW, bool STORED_RGB>
__global__ __launch_bounds__(PLANES_NT) void zj_planes_combine_kernel(const PlanesParams p)
{
    planes_lane<CHW, STORED_RGB>(p, (int)blockIdx.z, blockIdx.x * (uint32_t)PLANES_NT + threadIdx.x);
}

hipError_t launch_planes(int chw, int stored_rgb, const PlanesParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > PLANES_BATCH) return hipErrorInvalidValue;
    for (int i = 0; i < p.nimg; i++)
        if ((p.wh[i] & 0xffffu) == 0 || (p.wh[i] >> 16) == 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)planes_grid(p), 1, (unsigned)p.nimg);
    if (chw && stored_rgb) hipLaunchKernelGGL((zj_planes_combine_kernel<true, true>), grid, dim3(PLANES_NT), 0, s, p);
    else if (chw) hipLaunchKernelGGL((zj_planes_combine_kernel<true, false>), grid, dim3(PLANES_NT), 0, s, p);
    else if (stored_rgb) hipLaunchKernelGGL((zj_planes_combine_kernel<false, true>), grid, dim3(PLANES_NT), 0, s, p);
    else hipLaunchKernelGGL((zj_planes_combine_kernel<false, false>), grid, dim3(PLANES_NT), 0, s, p);
    return hipGetLastError();
}

} // namespace zj

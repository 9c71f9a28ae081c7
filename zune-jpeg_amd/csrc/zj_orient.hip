// zj_orient.hip -- gfx950 kernel of the EXIF orientation stage (zj_orient_device) and its launcher.
//
//   zj_orient_kernel<C, IN_CHW>   u8 images of their own sizes, pitches and orientations -> their displayed form
// A translation unit of its own: zj_kernels.hip, zj_crop.hip, zj_resize.hip, zj_resize_aa.hip and zj_scaled.hip keep their code
// objects instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_orient.h"
#include "zj_orient_launch.h"

namespace zj {

// One workgroup per (ORIENT_T displayed columns, ORIENT_T displayed rows, image x plane of the launch): blockIdx.x, .y, .z.
// The grid is sized for the launch's largest image; the workgroups beyond a smaller one leave at once.
template <int C, bool IN_CHW>
__global__ __launch_bounds__(ORIENT_NT) void zj_orient_kernel(const OrientParams p)
{
    constexpr int BPP = IN_CHW ? 1 : C, NPL = IN_CHW ? C : 1;
    __shared__ uint32_t lds[orient_lds_bytes<BPP>() / 4];
    const int tid = (int)threadIdx.x, img = (int)blockIdx.z / NPL, plane = (int)blockIdx.z - img * NPL;
    const OrientBlock b = orient_block<BPP>(p, img, plane, (int)blockIdx.x, (int)blockIdx.y);
    if (b.th == 0) return; // (uniform)
    orient_load_phase<BPP>(b, lds, tid);
    __syncthreads();
    orient_store_phase<BPP>(b, reinterpret_cast<const uint8_t*>(lds), tid);
}

template <int C, bool IN_CHW>
static hipError_t launch_orient_t(const OrientParams& p, hipStream_t s)
{
    int gx, gy;
    orient_grid(p, &gx, &gy);
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)(p.nimg * (IN_CHW ? C : 1)));
    hipLaunchKernelGGL((zj_orient_kernel<C, IN_CHW>), grid, dim3(ORIENT_NT), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_orient(int channels, int in_chw, const OrientParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > ORIENT_BATCH) return hipErrorInvalidValue;
    for (int i = 0; i < p.nimg; i++)
        if (!orient_valid(p.o[i]) || (p.wh[i] & 0xffffu) == 0 || (p.wh[i] >> 16) == 0) return hipErrorInvalidValue;
    if (channels == 1) return launch_orient_t<1, false>(p, s); // (one channel: every layout is the same)
    if (channels != 3) return hipErrorInvalidValue;
    return in_chw ? launch_orient_t<3, true>(p, s) : launch_orient_t<3, false>(p, s);
}

} // namespace zj

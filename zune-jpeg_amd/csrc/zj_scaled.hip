// zj_scaled.hip -- gfx950 kernels of the reduced-size decode (zj_decode_crops_scaled_device) and their launcher.
//
//   zj_scaled_kernel<HS,VS,OUT,SL>   one tile (TM MCUs of one MCU row) of a frame's window at scale 1 / 2^SL: one lane per
//                                    block -> the components' samples on the reduced grid in LDS -> the pixels' bytes in
//                                    LDS -> the window's part of them to the crop, lane-contiguous (zj_scaled.h)
// A translation unit of its own: the kernels of the other translation units keep their code objects instruction for
// instruction.
#include <hip/hip_runtime.h>

#include "zj_scaled.h"
#include "zj_scaled_launch.h"

namespace zj {

// blockIdx.z = frame of the launch, blockIdx.y / x = MCU row / tile counted from the window's first.  The second launch
// bound is a MINIMUM of waves per execution unit the compiler has to leave room for: it caps the registers at that
// occupancy's budget (4 waves per SIMD: 128 VGPRs).  The kernels need 48-80, i.e. 6-8 waves per SIMD by
// registers; LDS (1-19 KB per workgroup) allows 8 workgroups per CU at worst.
template <int HS, int VS, int OUT, int SL>
__global__ __launch_bounds__((ScaledCfg<HS, VS, OUT, SL>::NT), 4) void zj_scaled_kernel(const ScaledParams p)
{
    using C = ScaledCfg<HS, VS, OUT, SL>;
    __shared__ __attribute__((aligned(16))) char lds[C::LDS];
    ScaledTile t;
    if (!scaled_locate<C>(p, (int)blockIdx.z, (int)blockIdx.y, (int)blockIdx.x, t)) return; // uniform
    const int tid = (int)threadIdx.x;
    const ScaledLoc L = scaled_block_loc<C, HS, VS>(p, t, tid, lds);
    U4 raw[8];
    scaled_load<C>(L, raw);
    scaled_setup<C>(p, tid, lds);
    __syncthreads();
    scaled_finish<C, HS, VS>(L, raw, lds, p.clamp_dc);
    __syncthreads();
    scaled_color<C, OUT>(t, tid, lds);
    __syncthreads();
    scaled_copyout<C>(p, t, tid, lds);
}

template <int HS, int VS, int OUT, int SL>
static hipError_t launch_scaled_t(const ScaledParams& p, hipStream_t s)
{
    if (p.nframes <= 0 || p.ncols <= 0 || p.nrows <= 0) return hipSuccess;
    hipLaunchKernelGGL((zj_scaled_kernel<HS, VS, OUT, SL>), dim3((unsigned)p.ncols, (unsigned)p.nrows, (unsigned)p.nframes),
                       dim3(ScaledCfg<HS, VS, OUT, SL>::NT), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_scaled(int hs, int vs, int out, int scale_log2, const ScaledParams& p, hipStream_t s)
{
#define ZJ_CASE1(H, V, O, L) if (hs == H && vs == V && out == O && scale_log2 == L) return launch_scaled_t<H, V, O, L>(p, s);
#define ZJ_CASE(H, V, O) ZJ_CASE1(H, V, O, 1) ZJ_CASE1(H, V, O, 2) ZJ_CASE1(H, V, O, 3)
    ZJ_CASE(1, 1, OUT_RGB) ZJ_CASE(1, 1, OUT_GRAY) ZJ_CASE(1, 1, OUT_YCBCR) ZJ_CASE(1, 1, OUT_RGB_CHW)
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_GRAY) ZJ_CASE(2, 1, OUT_YCBCR) ZJ_CASE(2, 1, OUT_RGB_CHW)
    ZJ_CASE(1, 2, OUT_RGB) ZJ_CASE(1, 2, OUT_GRAY) ZJ_CASE(1, 2, OUT_YCBCR) ZJ_CASE(1, 2, OUT_RGB_CHW)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_GRAY) ZJ_CASE(2, 2, OUT_YCBCR) ZJ_CASE(2, 2, OUT_RGB_CHW)
#undef ZJ_CASE
#undef ZJ_CASE1
    return hipErrorInvalidValue;
}

} // namespace zj

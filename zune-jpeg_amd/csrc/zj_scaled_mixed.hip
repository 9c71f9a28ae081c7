// zj_scaled_mixed.hip -- gfx950 kernels of the mixed-geometry reduced-size decode (zj_decode_crops_resized_mixed_device;
// DESIGN.md 3.10) and their launcher.
//
//   zj_scaled_mixed_kernel<HS,VS,OUT,SL>   zj_scaled_kernel (zj_scaled.hip) with the frame's ScaledParams read from a table
//                                          in device memory, indexed by blockIdx.z, instead of from the kernel arguments
// A translation unit of its own: the kernels of the other translation units keep their code objects instruction for
// instruction.
#include <hip/hip_runtime.h>

#include "zj_scaled.h"
#include "zj_mixed_launch.h"

namespace zj {

// (zj_crop_mixed.hip: the table through the constant address space)
#define ZJ_TABLE_REF(T, tab, i) (*(const T*)((const __attribute__((address_space(4))) T*)(tab) + (i)))

// blockIdx.z = the frame's record (ONE frame, index 0), blockIdx.y / x = MCU row / tile counted from the window's first; the
// grid is the widest range over the launch's frames (scaled_locate: a workgroup outside its frame's returns at once)
template <int HS, int VS, int OUT, int SL>
__global__ __launch_bounds__((ScaledCfg<HS, VS, OUT, SL>::NT), 4) void zj_scaled_mixed_kernel(const ScaledParams* __restrict__ const tab)
{
    using C = ScaledCfg<HS, VS, OUT, SL>;
    __shared__ __attribute__((aligned(16))) char lds[C::LDS];
    const ScaledParams& p = ZJ_TABLE_REF(ScaledParams, tab, blockIdx.z);
    ScaledTile t;
    if (!scaled_locate<C>(p, 0, (int)blockIdx.y, (int)blockIdx.x, t)) return; // uniform
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
static hipError_t launch_scaled_mixed_t(const ScaledParams* d_tab, int n, int ncols, int nrows, hipStream_t s)
{
    for (int z0 = 0; z0 < n; z0 += MIXED_MAX_Z) {
        const int m = n - z0 < MIXED_MAX_Z ? n - z0 : MIXED_MAX_Z;
        hipLaunchKernelGGL((zj_scaled_mixed_kernel<HS, VS, OUT, SL>), dim3((unsigned)ncols, (unsigned)nrows, (unsigned)m),
                           dim3(ScaledCfg<HS, VS, OUT, SL>::NT), 0, s, d_tab + z0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_scaled_mixed(int hs, int vs, int out, int scale_log2, const ScaledParams* d_tab, int n, int ncols, int nrows,
                               hipStream_t s)
{
    if (n <= 0 || ncols <= 0 || nrows <= 0) return hipSuccess;
#define ZJ_CASE1(H, V, O, L) if (hs == H && vs == V && out == O && scale_log2 == L) return launch_scaled_mixed_t<H, V, O, L>(d_tab, n, ncols, nrows, s);
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

// zj_crop_mixed.hip -- gfx950 kernels of the mixed-geometry crop decode (zj_decode_crops_resized_mixed_device; DESIGN.md
// 3.10) and their launchers.
//
//   zj_fused_crop_mixed_kernel<HS,VS,OUT>   zj_fused_crop_kernel (zj_crop.hip) with the frame's CropParams read from a table
//                                           in device memory, indexed by blockIdx.z, instead of from the kernel arguments
//   zj_crop_zero_mixed_kernel               the window rows at or below each frame's own rows_covered (Q6)
// A translation unit of its own: the kernels of zj_kernels.hip, zj_crop.hip and zj_scaled.hip keep their code objects
// instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_device.h"
#include "zj_mixed_launch.h"

#ifndef ZJ_WAVES_PER_SIMD_PACKED
#define ZJ_WAVES_PER_SIMD_PACKED 6
#endif

namespace zj {

// the table in the constant address space: nothing on the device writes it, and a record's index is workgroup-uniform, so
// what is read of a record with a uniform offset comes through the scalar cache
#define ZJ_TABLE_REF(T, tab, i) (*(const T*)((const __attribute__((address_space(4))) T*)(tab) + (i)))

// (zj_crop.hip: the same bound by the LDS a workgroup holds)
constexpr int CROP_MIXED_LDS_PER_CU = 160 * 1024;
template <int HS, int VS, int OUT>
struct CropMixedOccupancy {
    using C = Cfg<HS, VS, OUT>;
    static constexpr int WGS = CROP_MIXED_LDS_PER_CU / (C::LDS_PACKED + CropStage<HS, VS, OUT>::BYTES);
    static constexpr int W = (WGS * C::NW + 3) / 4;
    static constexpr int W0 = W < 1 ? 1 : (W > ZJ_WAVES_PER_SIMD_PACKED ? ZJ_WAVES_PER_SIMD_PACKED : W);
    // 4:2:2 YCbCr with the record's address live spills 8 VGPRs at the 128 registers of four waves: it takes three waves'
    static constexpr int WAVES = (HS == 2 && VS == 1 && OUT == OUT_YCBCR && W0 > 3) ? 3 : W0;
};

// One workgroup per (frame, strip, tile column): blockIdx.z = the frame's record, blockIdx.y / x = strip / column counted
// from the frame's first.  The record holds ONE frame (index 0); the grid is the widest range over the launch's frames, and
// a workgroup outside its own frame's range returns at once (crop_locate).  The body is zj_fused_crop_kernel's.
template <int HS, int VS, int OUT>
__global__ __launch_bounds__((Cfg<HS, VS, OUT>::NT), (CropMixedOccupancy<HS, VS, OUT>::WAVES)) void zj_fused_crop_mixed_kernel(
    const CropParams* __restrict__ const tab)
{
    using C = Cfg<HS, VS, OUT>;
    using S = CropStage<HS, VS, OUT>;
    __shared__ __attribute__((aligned(16))) char lds[C::LDS_PACKED];
    __shared__ __attribute__((aligned(16))) uint8_t stage[S::BYTES];
    const CropParams& cp = ZJ_TABLE_REF(CropParams, tab, blockIdx.z);
    CropSpan s;
    if (!crop_locate<HS, VS, OUT>(cp, 0, (int)blockIdx.y, (int)blockIdx.x, s)) return; // uniform
    const Params& p = cp.p;
    TileId t;
    t.frame = 0; t.strip = s.strip; t.tile = s.tile;
    t.y = ZJ_GLOBAL_PTR(const int16_t, p.fptr[0][0]);
    t.cb = ZJ_GLOBAL_PTR(const int16_t, p.fptr[0][1]);
    t.cr = ZJ_GLOBAL_PTR(const int16_t, p.fptr[0][2]);
    t.out = crop_stage_base<HS, VS, OUT>(stage, s);
    constexpr bool NEED_Y16 = OUT == OUT_RGB || OUT == OUT_RGBA || OUT == OUT_RGB_CHW;
    const int tid = (int)threadIdx.x;
    const bool halo_wave = C::HALO_PURE && (__builtin_amdgcn_readfirstlane(tid) >> 6) == C::HALO_T0 / 64;
    if (halo_wave) {
        HaloLane H = halo_locate<C>(p, t, tid - C::HALO_T0, lds);
        int32_t hs8[8];
        halo_load(H, hs8);
        phase_setup<C, HS, VS, GEN_PACKED>(p, tid, lds);
        __syncthreads();
        halo_pass1<C>(H, hs8, lds);
        ZJ_WAVE_FENCE();
        halo_pass2<C>(H, lds, p.clamp_dc);
        ZJ_WAVE_FENCE();
        halo_filter<C, HS, VS>(p, t, tid - C::HALO_T0, lds);
    } else {
        const BlockLoc L = locate<C, GEN_PACKED>(p, t, tid, lds);
        U4 raw[8];
        load_block(L, raw, 0);
        phase_setup<C, HS, VS, GEN_PACKED>(p, tid, lds);
        __syncthreads();
        finish_block<C, GEN_PACKED, NEED_Y16>(L, raw, lds, 0, p.clamp_dc);
    }
    __builtin_amdgcn_s_waitcnt(0x0f70); // vmcnt(0), as zj_fused_crop_kernel
    __syncthreads();
    const bool redo = (NEED_Y16 || C::CBYTE) && __builtin_amdgcn_readfirstlane((int)*lds_flag<C>(lds)) != 0;
    if (redo) {
        __syncthreads();
        const BlockLoc L = locate<C, GEN_WIDE>(p, t, tid, lds);
        U4 raw[8];
        load_block(L, raw, 0);
        phase_setup<C, HS, VS, GEN_WIDE>(p, tid, lds);
        __syncthreads();
        finish_block<C, GEN_WIDE, false>(L, raw, lds, 0, p.clamp_dc);
        __syncthreads();
        phase_color<C, HS, VS, OUT, GEN_WIDE, false, false, false>(p, t, tid, lds);
    } else {
        phase_color<C, HS, VS, OUT, GEN_PACKED, false, false, false>(p, t, tid, lds);
    }
    __syncthreads();
    uint8_t* const out = ZJ_GLOBAL_PTR(uint8_t, p.fptr[0][3]);
    if (s.b0 < s.b1) crop_copyout<HS, VS, OUT>(cp, s, tid, C::NT, stage, out); // (both uniform)
    if (s.c0 < s.c1) {                                                       // the second interval the tile owns
        s.b0 = s.c0; s.b1 = s.c1;
        crop_copyout<HS, VS, OUT>(cp, s, tid, C::NT, stage, out);
    }
}

// zeros for the rows of each frame's tight crop at or below that frame's rows_covered: blockIdx.z = the record, .y = plane,
// .x = crop row (the grid: the tallest window, the most planes)
__global__ __launch_bounds__(256) void zj_crop_zero_mixed_kernel(const MixedZero* __restrict__ const tab)
{
    const MixedZero& z = ZJ_TABLE_REF(MixedZero, tab, blockIdx.z);
    const int pl = (int)blockIdx.y, r = (int)blockIdx.x;
    const int h = z.h, nbytes = z.nbytes;
    if (pl >= z.nplanes || r >= h || z.y0 + r < z.rows_covered) return;
    uint8_t* const p = ZJ_GLOBAL_PTR(uint8_t, z.out) + ((long long)pl * h + r) * nbytes;
    const unsigned n = (unsigned)nbytes;
    unsigned head = (16u - ((unsigned)reinterpret_cast<uintptr_t>(p) & 15u)) & 15u;
    if (head > n) head = n;
    const unsigned nq = (n - head) >> 4, tail = head + (nq << 4);
    const unsigned tid = threadIdx.x;
    if (tid < head) p[tid] = 0;
    const U4 zero = {0, 0, 0, 0};
    for (unsigned i = tid; i < nq; i += 256) *reinterpret_cast<U4*>(p + head + 16u * i) = zero;
    if (tail + tid < n) p[tail + tid] = 0;
}

hipError_t launch_crop_zero_mixed(const MixedZero* d_tab, int n, int max_h, int max_planes, hipStream_t s)
{
    if (n <= 0 || max_h <= 0 || max_planes <= 0) return hipSuccess;
    for (int z0 = 0; z0 < n; z0 += MIXED_MAX_Z) {
        const int m = n - z0 < MIXED_MAX_Z ? n - z0 : MIXED_MAX_Z;
        hipLaunchKernelGGL(zj_crop_zero_mixed_kernel, dim3((unsigned)max_h, (unsigned)max_planes, (unsigned)m), dim3(256), 0, s, d_tab + z0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int HS, int VS, int OUT>
static hipError_t launch_crop_mixed_t(const CropParams* d_tab, int n, int ncols, int nstrips, hipStream_t s)
{
    for (int z0 = 0; z0 < n; z0 += MIXED_MAX_Z) {
        const int m = n - z0 < MIXED_MAX_Z ? n - z0 : MIXED_MAX_Z;
        hipLaunchKernelGGL((zj_fused_crop_mixed_kernel<HS, VS, OUT>), dim3((unsigned)ncols, (unsigned)nstrips, (unsigned)m),
                           dim3(Cfg<HS, VS, OUT>::NT), 0, s, d_tab + z0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// (the outputs a resized crop can have: RGBA / RGBX have no resized form, zj_geom.h: resize_channels)
hipError_t launch_crop_mixed(int hs, int vs, int out, const CropParams* d_tab, int n, int ncols, int nstrips, hipStream_t s)
{
    if (n <= 0 || ncols <= 0 || nstrips <= 0) return hipSuccess;
#define ZJ_CASE(H, V, O) if (hs == H && vs == V && out == O) return launch_crop_mixed_t<H, V, O>(d_tab, n, ncols, nstrips, s);
    ZJ_CASE(1, 1, OUT_RGB) ZJ_CASE(1, 1, OUT_GRAY) ZJ_CASE(1, 1, OUT_YCBCR) ZJ_CASE(1, 1, OUT_RGB_CHW)
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_GRAY) ZJ_CASE(2, 1, OUT_YCBCR) ZJ_CASE(2, 1, OUT_RGB_CHW)
    ZJ_CASE(1, 2, OUT_RGB) ZJ_CASE(1, 2, OUT_GRAY) ZJ_CASE(1, 2, OUT_YCBCR) ZJ_CASE(1, 2, OUT_RGB_CHW)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_GRAY) ZJ_CASE(2, 2, OUT_YCBCR) ZJ_CASE(2, 2, OUT_RGB_CHW)
#undef ZJ_CASE
    return hipErrorInvalidValue;
}

} // namespace zj

// zj_crop_tensor.hip -- gfx950 kernels of the crop-window decode into a normalised tensor (zj_decode_crops_tensor_device;
// DESIGN.md 3.14) and their launchers.
//
//   zj_fused_crop_tensor_kernel<HS,VS,OUT>   zj_fused_crop_kernel (zj_crop.hip) up to the barrier before its copy-out, then
//                                            the owned bytes of the staging converted into tensor elements (zj_crop_tensor.h)
//   zj_crop_zero_tensor_kernel               the converted zero for the window rows at or below rows_covered (Q6)
// ONE kernel set serves the one-geometry call and the mixed-geometry call (zj_decode_crops_tensor_mixed_device): the
// launch's records lie in a table in device memory, as zj_crop_mixed.hip's.  A record holds up to
// 2^shift frames of one geometry: blockIdx.z >> shift is the record, the low bits the frame in it.  The one-geometry call
// launches records of SCATTER_MAX frames (shift 5), the mixed call records of one frame (shift 0).
// A translation unit of its own: the kernels of every other translation unit keep their code objects instruction for
// instruction.
#include <hip/hip_runtime.h>

#include "zj_crop_tensor.h"
#include "zj_crop_tensor_launch.h"

#ifndef ZJ_WAVES_PER_SIMD_PACKED
#define ZJ_WAVES_PER_SIMD_PACKED 6
#endif

namespace zj {

// the table in the constant address space: nothing on the device writes it, and a record's index is workgroup-uniform, so
// what is read of a record with a uniform offset comes through the scalar cache (zj_crop_mixed.hip)
#define ZJ_TABLE_REF(T, tab, i) (*(const T*)((const __attribute__((address_space(4))) T*)(tab) + (i)))

// (zj_crop.hip: the same bound by the LDS a workgroup holds; the copy-out adds no LDS)
constexpr int CROP_TENSOR_LDS_PER_CU = 160 * 1024;
template <int HS, int VS, int OUT>
struct CropTensorOccupancy {
    using C = Cfg<HS, VS, OUT>;
    static constexpr int WGS = CROP_TENSOR_LDS_PER_CU / (C::LDS_PACKED + CropStage<HS, VS, OUT>::BYTES);
    static constexpr int W = (WGS * C::NW + 3) / 4;
    static constexpr int W0 = W < 1 ? 1 : (W > ZJ_WAVES_PER_SIMD_PACKED ? ZJ_WAVES_PER_SIMD_PACKED : W);
    // 4:2:2 RGB / YCbCr with the record's address live spill 45 / 19 VGPRs to scratch at the 128 registers of four waves
    // (as zj_crop_mixed.hip's 4:2:2 YCbCr): they take three waves' registers
    static constexpr int WAVES = (HS == 2 && VS == 1 && OUT != OUT_GRAY && W0 > 3) ? 3 : W0;
};

// One workgroup per (frame, strip, tile column) the window needs, as zj_fused_crop_kernel: the body is that kernel's up to
// the barrier in front of its copy-out.
template <int HS, int VS, int OUT>
__global__ __launch_bounds__((Cfg<HS, VS, OUT>::NT), (CropTensorOccupancy<HS, VS, OUT>::WAVES)) void zj_fused_crop_tensor_kernel(
    const CropTensorParams* __restrict__ const tab, const int shift)
{
    using C = Cfg<HS, VS, OUT>;
    using S = CropStage<HS, VS, OUT>;
    __shared__ __attribute__((aligned(16))) char lds[C::LDS_PACKED];
    __shared__ __attribute__((aligned(16))) uint8_t stage[S::BYTES];
    const CropTensorParams& tp = ZJ_TABLE_REF(CropTensorParams, tab, blockIdx.z >> shift);
    const int fz = (int)(blockIdx.z & ((1u << shift) - 1u));
    const CropParams& cp = tp.cp;
    CropSpan s;
    if (!crop_locate<HS, VS, OUT>(cp, fz, (int)blockIdx.y, (int)blockIdx.x, s)) return; // uniform
    const Params& p = cp.p;
    TileId t;
    t.frame = s.frame; t.strip = s.strip; t.tile = s.tile;
    t.y = ZJ_GLOBAL_PTR(const int16_t, p.fptr[s.frame][0]);
    t.cb = ZJ_GLOBAL_PTR(const int16_t, p.fptr[s.frame][1]);
    t.cr = ZJ_GLOBAL_PTR(const int16_t, p.fptr[s.frame][2]);
    t.out = crop_stage_base<HS, VS, OUT>(stage, s);
    constexpr bool NEED_Y16 = OUT == OUT_RGB;
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
    uint8_t* const img = ZJ_GLOBAL_PTR(uint8_t, p.fptr[s.frame][3]);
    const CropTensorOut o = crop_tensor_out(tp, fz);
    // the two intervals the tile owns (either may be empty; uniform), through ONE copy of the copy-out's code
#pragma nounroll
    for (int k = 0; k < 2; k++) {
        if (k) { s.b0 = s.c0; s.b1 = s.c1; }
        if (s.b0 < s.b1) crop_copyout_tensor<HS, VS, OUT>(o, s, tid, C::NT, stage, img);
    }
}

// the converted zero for the window rows at or below rows_covered (Q6): blockIdx.z = record, blockIdx.y = frame of the
// record, blockIdx.x = window row - rmin (the grid: the widest ranges over the launch's records)
__global__ __launch_bounds__(256) void zj_crop_zero_tensor_kernel(const CropTensorZero* __restrict__ const tab)
{
    const CropTensorZero& z = ZJ_TABLE_REF(CropTensorZero, tab, blockIdx.z);
    if ((int)blockIdx.y >= z.nframes) return;
    crop_tensor_zero(z, (int)blockIdx.y, z.rmin + (int)blockIdx.x, (int)threadIdx.x, 256);
}

hipError_t launch_crop_tensor_zero(const CropTensorZero* d_tab, int nrec, int max_rows, int max_frames, hipStream_t s)
{
    if (nrec <= 0 || max_rows <= 0 || max_frames <= 0) return hipSuccess;
    for (int z0 = 0; z0 < nrec; z0 += CROP_TENSOR_MAX_Z) {
        const int m = nrec - z0 < CROP_TENSOR_MAX_Z ? nrec - z0 : CROP_TENSOR_MAX_Z;
        hipLaunchKernelGGL(zj_crop_zero_tensor_kernel, dim3((unsigned)max_rows, (unsigned)max_frames, (unsigned)m), dim3(256), 0, s, d_tab + z0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int HS, int VS, int OUT>
static hipError_t launch_crop_tensor_t(const CropTensorParams* d_tab, int nrec, int shift, int ncols, int nstrips, hipStream_t s)
{
    const int per = CROP_TENSOR_MAX_Z >> shift; // records of one launch: the grid's z extent
    for (int z0 = 0; z0 < nrec; z0 += per) {
        const int m = nrec - z0 < per ? nrec - z0 : per;
        hipLaunchKernelGGL((zj_fused_crop_tensor_kernel<HS, VS, OUT>), dim3((unsigned)ncols, (unsigned)nstrips, (unsigned)(m << shift)),
                           dim3(Cfg<HS, VS, OUT>::NT), 0, s, d_tab + z0, shift);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// (the outputs a tensor can have: RGBA / RGBX and CHW planes have none, zj_geom.h: resize_channels)
hipError_t launch_crop_tensor(int hs, int vs, int out, const CropTensorParams* d_tab, int nrec, int shift, int ncols, int nstrips,
                              hipStream_t s)
{
    if (nrec <= 0 || ncols <= 0 || nstrips <= 0) return hipSuccess;
#define ZJ_CASE(H, V, O) if (hs == H && vs == V && out == O) return launch_crop_tensor_t<H, V, O>(d_tab, nrec, shift, ncols, nstrips, s);
    ZJ_CASE(1, 1, OUT_RGB) ZJ_CASE(1, 1, OUT_GRAY) ZJ_CASE(1, 1, OUT_YCBCR)
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_GRAY) ZJ_CASE(2, 1, OUT_YCBCR)
    ZJ_CASE(1, 2, OUT_RGB) ZJ_CASE(1, 2, OUT_GRAY) ZJ_CASE(1, 2, OUT_YCBCR)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_GRAY) ZJ_CASE(2, 2, OUT_YCBCR)
#undef ZJ_CASE
    return hipErrorInvalidValue;
}

} // namespace zj

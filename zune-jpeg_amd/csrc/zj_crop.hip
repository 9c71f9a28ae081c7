// zj_crop.hip -- gfx950 kernels of the crop-window decode (zj_decode_crops_device) and their launchers.
//
//   zj_fused_crop_kernel<HS,VS,OUT>   one tile of a window: the packed generation's tile decode with the generic stores into
//                                     a staging area in LDS, then the window's bytes of it to the crop (zj_device.h)
//   zj_crop_zero_kernel               the window rows below the last complete strip (Q6)
// A translation unit of its own: the fused kernels of zj_kernels.hip keep their code objects instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_device.h"
#include "zj_launch.h"

#ifndef ZJ_WAVES_PER_SIMD_PACKED
#define ZJ_WAVES_PER_SIMD_PACKED 6
#endif

namespace zj {

// ------------------------------------------------------------------------------------------------
// crop-window kernels (zj_device.h: CropParams, crop_copyout)
// ------------------------------------------------------------------------------------------------
// One workgroup per (frame, strip, tile column) the window needs: blockIdx.z = frame of the launch, blockIdx.y / x = strip
// / column counted from the frame's first.  The tile is decoded by the packed generation with the generic stores (any
// width, every flag, the early tail and its zeros), into a staging area in LDS laid out like the frame's rows; the
// workgroup then copies the window's part of the bytes it owns (one or two intervals of a row, zj_device.h:
// crop_own_spans).  One instantiation per (HS, VS, OUT).
// The launch bound follows from the LDS a workgroup holds (tile + staging, 30-62 KB: 2 to 5 workgroups on the 160 KB of a
// CU): the waves per SIMD that can actually be resident, so that the register budget is that occupancy's, not the full
// kernels' six.
constexpr int CROP_LDS_PER_CU = 160 * 1024;
template <int HS, int VS, int OUT>
struct CropOccupancy {
    using C = Cfg<HS, VS, OUT>;
    static constexpr int WGS = CROP_LDS_PER_CU / (C::LDS_PACKED + CropStage<HS, VS, OUT>::BYTES); // workgroups per CU
    static constexpr int W = (WGS * C::NW + 3) / 4;                                               // waves per SIMD
    static constexpr int WAVES = W < 1 ? 1 : (W > ZJ_WAVES_PER_SIMD_PACKED ? ZJ_WAVES_PER_SIMD_PACKED : W);
};

template <int HS, int VS, int OUT>
__global__ __launch_bounds__((Cfg<HS, VS, OUT>::NT), (CropOccupancy<HS, VS, OUT>::WAVES)) void zj_fused_crop_kernel(const CropParams cp)
{
    using C = Cfg<HS, VS, OUT>;
    using S = CropStage<HS, VS, OUT>;
    __shared__ __attribute__((aligned(16))) char lds[C::LDS_PACKED];
    __shared__ __attribute__((aligned(16))) uint8_t stage[S::BYTES];
    CropSpan s;
    if (!crop_locate<HS, VS, OUT>(cp, (int)blockIdx.z, (int)blockIdx.y, (int)blockIdx.x, s)) return; // uniform
    const Params& p = cp.p;
    TileId t;
    t.frame = s.frame; t.strip = s.strip; t.tile = s.tile;
    t.y = ZJ_GLOBAL_PTR(const int16_t, p.fptr[s.frame][0]);
    t.cb = ZJ_GLOBAL_PTR(const int16_t, p.fptr[s.frame][1]);
    t.cr = ZJ_GLOBAL_PTR(const int16_t, p.fptr[s.frame][2]);
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
    __builtin_amdgcn_s_waitcnt(0x0f70); // vmcnt(0), see fused_body
    __syncthreads();
    const bool redo = (NEED_Y16 || C::CBYTE) && __builtin_amdgcn_readfirstlane((int)*lds_flag<C>(lds)) != 0;
    if (redo) { // (the wide code over the same tile, as fused_body's tile_wide)
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
    uint8_t* const out = ZJ_GLOBAL_PTR(uint8_t, p.fptr[s.frame][3]);
    if (s.b0 < s.b1) crop_copyout<HS, VS, OUT>(cp, s, tid, C::NT, stage, out); // (both uniform)
    if (s.c0 < s.c1) {                                                       // the second interval the tile owns
        s.b0 = s.c0; s.b1 = s.c1;
        crop_copyout<HS, VS, OUT>(cp, s, tid, C::NT, stage, out);
    }
}

// zeros for the window rows at or below rows_covered (Q6); only the window's bytes of each row, never the pitch padding
__global__ __launch_bounds__(256) void zj_crop_zero_kernel(const CropZero z)
{
    const int fr = (int)blockIdx.y / z.nplanes, pl = (int)blockIdx.y - fr * z.nplanes, r = (int)blockIdx.x;
    const uint32_t wh = z.size[fr];
    const int h = wh ? (int)(wh >> 16) : z.crop_h, nbytes = wh ? (int)(wh & 0xffffu) * z.bpp : z.nbytes;
    if (r >= h || (int)z.y0[fr] + r < z.rows_covered) return;
    const int pitch = z.out_pitch ? z.out_pitch : nbytes;
    const long long plane = z.out_pitch ? z.crop_plane : (long long)pitch * h;
    uint8_t* const p = ZJ_GLOBAL_PTR(uint8_t, z.fptr[fr]) + (long long)pl * plane + (long long)r * pitch;
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

hipError_t launch_crop_zero(const CropZero& z, hipStream_t s)
{
    if (z.nframes <= 0 || z.crop_h <= 0 || z.nbytes <= 0) return hipSuccess;
    hipLaunchKernelGGL(zj_crop_zero_kernel, dim3((unsigned)z.crop_h, (unsigned)(z.nframes * z.nplanes)), dim3(256), 0, s, z);
    return hipGetLastError();
}

template <int HS, int VS, int OUT>
static hipError_t launch_crop_t(const CropParams& cp, hipStream_t s)
{
    const int nframes = cp.p.nframes;
    if (nframes <= 0 || cp.ncols <= 0 || cp.nstrips <= 0) return hipSuccess;
    hipLaunchKernelGGL((zj_fused_crop_kernel<HS, VS, OUT>), dim3((unsigned)cp.ncols, (unsigned)cp.nstrips, (unsigned)nframes),
                       dim3(Cfg<HS, VS, OUT>::NT), 0, s, cp);
    return hipGetLastError();
}

hipError_t launch_crop(int hs, int vs, int out, const CropParams& cp, hipStream_t s)
{
#define ZJ_CASE(H, V, O) if (hs == H && vs == V && out == O) return launch_crop_t<H, V, O>(cp, s);
    ZJ_CASE(1, 1, OUT_RGB) ZJ_CASE(1, 1, OUT_GRAY) ZJ_CASE(1, 1, OUT_YCBCR)
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_GRAY) ZJ_CASE(2, 1, OUT_YCBCR)
    ZJ_CASE(1, 2, OUT_RGB) ZJ_CASE(1, 2, OUT_GRAY) ZJ_CASE(1, 2, OUT_YCBCR)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_GRAY) ZJ_CASE(2, 2, OUT_YCBCR)
    ZJ_CASE(1, 1, OUT_RGBA) ZJ_CASE(2, 1, OUT_RGBA) ZJ_CASE(1, 2, OUT_RGBA) ZJ_CASE(2, 2, OUT_RGBA)
    ZJ_CASE(1, 1, OUT_RGB_CHW) ZJ_CASE(2, 1, OUT_RGB_CHW) ZJ_CASE(1, 2, OUT_RGB_CHW) ZJ_CASE(2, 2, OUT_RGB_CHW)
#undef ZJ_CASE
    return hipErrorInvalidValue;
}

} // namespace zj

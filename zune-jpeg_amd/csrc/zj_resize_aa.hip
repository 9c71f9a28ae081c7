// zj_resize_aa.hip -- gfx950 kernel of the antialiased resize (zj_resize_filtered_device with ZJ_RESIZE_BILINEAR_AA,
// DESIGN.md 3.6) and its launcher.
//
//   zj_resize_aa_kernel<IN_CHW, C, DT, NHWC>   u8 images of their own sizes -> one dense [N, C, OH, OW] / [N, OH, OW, C] tensor
// A translation unit of its own: zj_kernels.hip, zj_crop.hip and zj_resize.hip keep their code objects instruction for
// instruction.
#include <hip/hip_runtime.h>

#include "zj_resize_aa.h"
#include "zj_resize_launch.h"

namespace zj {

// One workgroup per (AA_COLS output columns, AA_ROWS output rows, image of the launch): blockIdx.x, .y, .z.  The phases
// of zj_resize_aa.h with the barriers between them; the lane's sums stay in registers across the source-column pieces.
template <bool IN_CHW, int C, int DT, bool NHWC>
__global__ __launch_bounds__(AA_NT) void zj_resize_aa_kernel(const ResizeParams p)
{
    __shared__ AaShared s;
    const int tid = (int)threadIdx.x, img = (int)blockIdx.z;
    const AaBlock b = aa_block(p, img, (int)blockIdx.x, (int)blockIdx.y, IN_CHW);
    const long long img_bytes = (long long)C * b.oh * b.ow * resize_elem_bytes(DT);
    uint8_t* const out = ZJ_RZ_GLOBAL(uint8_t, p.out) + (long long)img * img_bytes;
    AaLane l;
#pragma unroll
    for (int q = 0; q < AA_WORD; q++) l.v[q] = 0;
#pragma unroll
    for (int q = 0; q < AA_GROUP * 3; q++) l.h[q] = 0;
    aa_col_axes_phase(b, s, tid);
    __syncthreads();
    int sx0, sx1;
    aa_span(b, s, sx0, sx1);
    constexpr int PW = aa_piece_w<IN_CHW, C>();
    for (int px0 = sx0; px0 <= sx1; px0 += PW) {
        const int px1 = sx1 + 1 - px0 < PW ? sx1 + 1 : px0 + PW;
        aa_col_count_phase(b, s, px0, px1, tid);
        __syncthreads();
        aa_col_offset_phase(b, s, tid);
        __syncthreads();
        aa_col_weights_phase(b, s, tid);
        for (int rr = 0; rr < b.nrows; rr++) {
            const AaAxis ra = aa_axis((uint32_t)(b.r0 + rr), (uint32_t)b.n_h, (uint32_t)b.oh);
            const int ntaps = ra.hi - ra.lo + 1;
            for (int j0 = 0; j0 < ntaps; j0 += AA_NT) {
                __syncthreads();
                aa_row_weights_phase(ra, s, j0, tid);
                __syncthreads();
                aa_vertical_phase<IN_CHW, C>(b, s, l, ra.lo, j0, ntaps - j0 < AA_NT ? ntaps - j0 : AA_NT, px0, px1, tid);
            }
            aa_vertical_store<IN_CHW, C>(s, l, rr, px0, px1, tid);
        }
        __syncthreads();
        aa_horizontal_phase<IN_CHW, C>(b, s, l, px0, tid);
        __syncthreads();
    }
    aa_store_phase<C, DT, NHWC>(p, b, l, out, tid);
}

template <bool IN_CHW, int C, int DT, bool NHWC>
static hipError_t launch_resize_aa_t(const ResizeParams& p, hipStream_t s)
{
    const dim3 grid((unsigned)((p.out_w + AA_COLS - 1) / AA_COLS), (unsigned)((p.out_h + AA_ROWS - 1) / AA_ROWS), (unsigned)p.nimg);
    hipLaunchKernelGGL((zj_resize_aa_kernel<IN_CHW, C, DT, NHWC>), grid, dim3(AA_NT), 0, s, p);
    return hipGetLastError();
}

template <bool IN_CHW, int C, bool NHWC>
static hipError_t launch_resize_aa_dt(int dtype, const ResizeParams& p, hipStream_t s)
{
    switch (dtype) {
    case RZ_F32: return launch_resize_aa_t<IN_CHW, C, RZ_F32, NHWC>(p, s);
    case RZ_F16: return launch_resize_aa_t<IN_CHW, C, RZ_F16, NHWC>(p, s);
    case RZ_BF16: return launch_resize_aa_t<IN_CHW, C, RZ_BF16, NHWC>(p, s);
    case RZ_U8: return launch_resize_aa_t<IN_CHW, C, RZ_U8, NHWC>(p, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_resize_aa(int channels, int in_chw, int dtype, int nhwc, const ResizeParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > RESIZE_BATCH || p.out_w <= 0 || p.out_h <= 0 || p.out_w > RESIZE_MAX_OUT || p.out_h > RESIZE_MAX_OUT)
        return hipErrorInvalidValue;
    if (channels == 1) return launch_resize_aa_dt<false, 1, false>(dtype, p, s); // (one channel: every layout is the same)
    if (channels != 3) return hipErrorInvalidValue;
    if (in_chw) return nhwc ? launch_resize_aa_dt<true, 3, true>(dtype, p, s) : launch_resize_aa_dt<true, 3, false>(dtype, p, s);
    return nhwc ? launch_resize_aa_dt<false, 3, true>(dtype, p, s) : launch_resize_aa_dt<false, 3, false>(dtype, p, s);
}

} // namespace zj

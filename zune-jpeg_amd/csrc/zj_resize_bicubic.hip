// zj_resize_bicubic.hip -- gfx950 kernel of the bicubic antialiased resize (zj_resize_filtered_device with
// ZJ_RESIZE_BICUBIC_AA) and its launcher.
//
//   zj_resize_bicubic_kernel<IN_CHW, C, DT, NHWC>   u8 images of their own sizes -> one dense [N, C, OH, OW] / [N, OH, OW, C] tensor
// A translation unit of its own: the other kernels' code objects stay instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_resize_bicubic.h"
#include "zj_resize_launch.h"

namespace zj {

// One workgroup per (AA_COLS output columns, AA_ROWS output rows, image of the launch): blockIdx.x, .y, .z.  The phases
// of zj_resize_bicubic.h with the barriers between them; the lane's sums stay in registers across the source-column pieces.
template <bool IN_CHW, int C, int DT, bool NHWC>
__global__ __launch_bounds__(AA_NT) void zj_resize_bicubic_kernel(const ResizeParams p)
{
    __shared__ BcShared s;
    const int tid = (int)threadIdx.x, img = (int)blockIdx.z;
    const AaBlock b = aa_block(p, img, (int)blockIdx.x, (int)blockIdx.y, IN_CHW);
    const long long img_bytes = (long long)C * b.oh * b.ow * resize_elem_bytes(DT);
    uint8_t* const out = ZJ_RZ_GLOBAL(uint8_t, p.out) + (long long)img * img_bytes;
    BcLane l;
#pragma unroll
    for (int rr = 0; rr < AA_ROWS; rr++)
#pragma unroll
        for (int q = 0; q < BC_WORD; q++) l.v[rr][q] = 0;
#pragma unroll
    for (int q = 0; q < AA_GROUP * 3; q++) l.h[q] = 0;
    // every output's S, over all of its taps
    bc_axes_phase(b, s, tid);
    __syncthreads();
    bc_sum_phase(s.col, s.cpart, b.ncols, tid);
    bc_sum_phase(s.row, s.rpart, b.nrows, tid);
    __syncthreads();
    bc_S_phase(s.col, s.cpart, b.ncols, tid);
    bc_S_phase(s.row, s.rpart, b.nrows, tid);
    int sx0, sx1;
    bc_span(b, s, sx0, sx1);
    const int rtaps = bc_row_taps(b, s);
    constexpr int PW = bc_piece_w<IN_CHW, C>();
    for (int px0 = sx0; px0 <= sx1; px0 += PW) {
        const int px1 = sx1 + 1 - px0 < PW ? sx1 + 1 : px0 + PW;
        __syncthreads();
        bc_col_window_phase(b, s, px0, px1, tid);
        __syncthreads();
        bc_col_offset_phase(b, s, tid);
        bc_sum_phase(s.col, s.cpart, b.ncols, tid);
        __syncthreads();
        bc_weights_phase(s.col, s.cpart, s.cw, b.ncols, tid);
        for (int j0 = 0; j0 < rtaps; j0 += BC_RCH) {
            __syncthreads();
            bc_row_window_phase(b, s, j0, tid);
            __syncthreads();
            bc_sum_phase(s.row, s.rpart, b.nrows, tid);
            __syncthreads();
            bc_weights_phase(s.row, s.rpart, s.rw, b.nrows, tid);
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < AA_ROWS; rr++)
                if (rr < b.nrows) bc_vertical_phase<IN_CHW, C>(b, s, l.v[rr], rr, px0, px1, tid);
        }
        bc_vertical_store<IN_CHW, C>(b, s, l, px0, px1, tid);
        __syncthreads();
        bc_carry_phase(s.col, s.cpart, b.ncols, tid);
        bc_horizontal_phase<IN_CHW, C>(b, s, l, px0, tid);
    }
    bc_store_phase<C, DT, NHWC>(p, b, l, out, tid);
}

template <bool IN_CHW, int C, int DT, bool NHWC>
static hipError_t launch_resize_bicubic_t(const ResizeParams& p, hipStream_t s)
{
    const dim3 grid((unsigned)((p.out_w + AA_COLS - 1) / AA_COLS), (unsigned)((p.out_h + AA_ROWS - 1) / AA_ROWS), (unsigned)p.nimg);
    hipLaunchKernelGGL((zj_resize_bicubic_kernel<IN_CHW, C, DT, NHWC>), grid, dim3(AA_NT), 0, s, p);
    return hipGetLastError();
}

template <bool IN_CHW, int C, bool NHWC>
static hipError_t launch_resize_bicubic_dt(int dtype, const ResizeParams& p, hipStream_t s)
{
    switch (dtype) {
    case RZ_F32: return launch_resize_bicubic_t<IN_CHW, C, RZ_F32, NHWC>(p, s);
    case RZ_F16: return launch_resize_bicubic_t<IN_CHW, C, RZ_F16, NHWC>(p, s);
    case RZ_BF16: return launch_resize_bicubic_t<IN_CHW, C, RZ_BF16, NHWC>(p, s);
    case RZ_U8: return launch_resize_bicubic_t<IN_CHW, C, RZ_U8, NHWC>(p, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_resize_bicubic(int channels, int in_chw, int dtype, int nhwc, const ResizeParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > RESIZE_BATCH || p.out_w <= 0 || p.out_h <= 0 || p.out_w > RESIZE_MAX_OUT || p.out_h > RESIZE_MAX_OUT)
        return hipErrorInvalidValue;
    if (channels == 1) return launch_resize_bicubic_dt<false, 1, false>(dtype, p, s); // (one channel: every layout is the same)
    if (channels != 3) return hipErrorInvalidValue;
    if (in_chw) return nhwc ? launch_resize_bicubic_dt<true, 3, true>(dtype, p, s) : launch_resize_bicubic_dt<true, 3, false>(dtype, p, s);
    return nhwc ? launch_resize_bicubic_dt<false, 3, true>(dtype, p, s) : launch_resize_bicubic_dt<false, 3, false>(dtype, p, s);
}

} // namespace zj

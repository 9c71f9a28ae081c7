// zj_resize.hip -- gfx950 kernel of the resize + normalise stage (zj_resize_device) and its launcher.
//
//   zj_resize_kernel<IN_CHW, C, DT, NHWC>   u8 images of their own sizes -> one dense [N, C, OH, OW] / [N, OH, OW, C] tensor
// A translation unit of its own: the fused kernels of zj_kernels.hip keep their code objects instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_resize.h"
#include "zj_resize_launch.h"

namespace zj {

// One workgroup per (block of p.rows output rows, image): blockIdx.x = row block, blockIdx.y = image of the launch.  The
// column taps of the image are computed once per workgroup into LDS (flip applied there), the row taps of its rows too; a
// lane then writes RESIZE_GROUP consecutive pixels of one output row, every channel.  The input is gathered byte by byte
// (a crop's rows are small and L2-resident); the stores are 16 bytes wide wherever the address and the run allow
// (zj_resize.h: resize_store), and a wave's lanes write consecutive runs of a row.
template <bool IN_CHW, int C, int DT, bool NHWC>
__global__ __launch_bounds__(RESIZE_NT) void zj_resize_kernel(const ResizeParams p)
{
    extern __shared__ uint32_t ctap[];   // out_w column taps
    __shared__ uint32_t rtap[RESIZE_ITEMS]; // p.rows row taps
    const int img = (int)blockIdx.y;
    const int r0 = (int)blockIdx.x * p.rows;
    const int ow = p.out_w, oh = p.out_h;
    const uint32_t wh = p.wh[img];
    const uint32_t n_w = wh & 0xffffu, n_h = wh >> 16;
    const bool flip = (p.flip[img >> 5] >> (img & 31)) & 1u;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < ow; i += RESIZE_NT) ctap[i] = resize_tap((uint32_t)(flip ? ow - 1 - i : i), n_w, (uint32_t)ow);
    int nr = oh - r0;
    if (nr > p.rows) nr = p.rows;
    for (int i = tid; i < nr; i += RESIZE_NT) rtap[i] = resize_tap((uint32_t)(r0 + i), n_h, (uint32_t)oh);
    __syncthreads();
    const uint8_t* const src = ZJ_RZ_GLOBAL(const uint8_t, p.in[img]);
    const long long img_bytes = (long long)C * oh * ow * resize_elem_bytes(DT);
    uint8_t* const out = ZJ_RZ_GLOBAL(uint8_t, p.out) + (long long)img * img_bytes;
    const int pitch = (int)p.pitch[img], groups = p.groups;
    const int items = nr * groups;
    for (int it = tid; it < items; it += RESIZE_NT) {
        const int rr = it / groups, g = it - rr * groups;
        const int x0 = g * RESIZE_GROUP;
        resize_group<IN_CHW, C, DT, NHWC>(p, src, pitch, (int)n_h, ctap + x0, rtap[rr], r0 + rr, x0, out);
    }
}

template <bool IN_CHW, int C, int DT, bool NHWC>
static hipError_t launch_resize_t(const ResizeParams& p, hipStream_t s)
{
    const unsigned blocks = (unsigned)((p.out_h + p.rows - 1) / p.rows);
    hipLaunchKernelGGL((zj_resize_kernel<IN_CHW, C, DT, NHWC>), dim3(blocks, (unsigned)p.nimg), dim3(RESIZE_NT),
                       (size_t)p.out_w * 4, s, p);
    return hipGetLastError();
}

template <bool IN_CHW, int C, bool NHWC>
static hipError_t launch_resize_dt(int dtype, const ResizeParams& p, hipStream_t s)
{
    switch (dtype) {
    case RZ_F32: return launch_resize_t<IN_CHW, C, RZ_F32, NHWC>(p, s);
    case RZ_F16: return launch_resize_t<IN_CHW, C, RZ_F16, NHWC>(p, s);
    case RZ_BF16: return launch_resize_t<IN_CHW, C, RZ_BF16, NHWC>(p, s);
    case RZ_U8: return launch_resize_t<IN_CHW, C, RZ_U8, NHWC>(p, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_resize(int channels, int in_chw, int dtype, int nhwc, const ResizeParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > RESIZE_BATCH || p.out_w <= 0 || p.out_h <= 0 || p.rows <= 0 || p.rows > RESIZE_ITEMS)
        return hipErrorInvalidValue;
    if (channels == 1) return launch_resize_dt<false, 1, false>(dtype, p, s); // (one channel: every layout is the same)
    if (channels != 3) return hipErrorInvalidValue;
    if (in_chw) return nhwc ? launch_resize_dt<true, 3, true>(dtype, p, s) : launch_resize_dt<true, 3, false>(dtype, p, s);
    return nhwc ? launch_resize_dt<false, 3, true>(dtype, p, s) : launch_resize_dt<false, 3, false>(dtype, p, s);
}

} // namespace zj

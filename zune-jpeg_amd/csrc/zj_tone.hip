// zj_tone.hip -- gfx950 kernels of the tone stages (zj_histogram_device, zj_tone_luts_device, zj_lut_device, zj_tone_device;
// DESIGN.md 3.18) and their launchers.
//
//   zj_hist_kernel<C, CHW>      u8 images of their own sizes and pitches -> uint32 hist[image][channel][256]
//   zj_tone_lut_kernel          an op and, where it needs one, a histogram per image -> uint8 lut[image][channel][256]
//   zj_lut_kernel<C, CHW>       out[c] = lut[image][c][in[c]]
// A translation unit of its own: the other kernels keep their code objects instruction for instruction.
#include <hip/hip_runtime.h>

#include "zj_tone.h"
#include "zj_tone_launch.h"

namespace zj {

// One workgroup per HIST_ITEMS runs of image blockIdx.z, counted row by row.  The grid is sized for the launch's largest
// image; the workgroups beyond a smaller one leave at once (blockIdx is the same over a workgroup).  The counters are one
// copy per workgroup in LDS (ds_add_u32 without a returned value); the flush is one global atomic per non-empty counter.
template <int C, bool CHW>
__global__ __launch_bounds__(TONE_NT) void zj_hist_kernel(const HistParams p)
{
    __shared__ uint32_t lds[C * 256];
    const int img = (int)blockIdx.z, tid = (int)threadIdx.x;
    if (!hist_block_active(p, img, blockIdx.x)) return; // (uniform)
    hist_zero_phase<C>(lds, tid);
    __syncthreads();
    hist_count_phase<C, CHW>(p, img, blockIdx.x, tid, lds);
    __syncthreads();
    hist_flush_phase<C>(p, img, tid, lds);
}

// One workgroup of 256 lanes per image, lane i owns entry i; the channels one after the other.  The op is the same over the
// workgroup, so every branch on it is uniform and every barrier is met by all lanes.
__global__ __launch_bounds__(TONE_NT) void zj_tone_lut_kernel(const ToneLutParams p)
{
    __shared__ ToneLutLds l;
    const int img = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int32_t op = p.op[img];
    for (int c = 0; c < p.channels; c++) {
        if (tone_needs_hist(op)) {
            const uint32_t hv = tone_lut_load_phase(p, img, c, tid, l);
            __syncthreads();
            tone_lut_reduce_phase(tid, hv, l);
            __syncthreads();
            if (op == TONE_EQUALIZE)
                for (int step = 0; step < 8; step++) {
                    tone_lut_scan_phase(tid, step, l);
                    __syncthreads();
                }
        }
        tone_lut_entry_phase(p, img, c, tid, l);
        __syncthreads(); // (the next channel's load phase overwrites what this one's entries read)
    }
}

// One lane per run of TONE_RUN pixels of a row: blockIdx.x x TONE_NT + threadIdx.x counts the runs of image blockIdx.z row by
// row.  The workgroup copies its image's table into LDS once; the workgroups beyond a smaller image leave at once.
template <int C, bool CHW>
__global__ __launch_bounds__(TONE_NT) void zj_lut_kernel(const LutParams p)
{
    __shared__ uint32_t lds[C * 64];
    const int img = (int)blockIdx.z, tid = (int)threadIdx.x;
    if (!lut_block_active(p, img, blockIdx.x)) return; // (uniform)
    lut_table_phase<C>(p, img, tid, lds);
    __syncthreads();
    lut_map_phase<C, CHW>(p, img, blockIdx.x * (uint32_t)TONE_NT + threadIdx.x, reinterpret_cast<const uint8_t*>(lds));
}

template <class P>
static bool tone_sizes_ok(const P& p)
{
    for (int i = 0; i < p.nimg; i++)
        if ((p.wh[i] & 0xffffu) == 0 || (p.wh[i] >> 16) == 0) return false;
    return true;
}

hipError_t launch_hist(int channels, int chw, const HistParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > HIST_BATCH || !tone_sizes_ok(p) || (channels != 1 && channels != 3)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)hist_grid(p), 1, (unsigned)p.nimg);
    if (channels == 1) hipLaunchKernelGGL((zj_hist_kernel<1, false>), grid, dim3(TONE_NT), 0, s, p);
    else if (chw) hipLaunchKernelGGL((zj_hist_kernel<3, true>), grid, dim3(TONE_NT), 0, s, p);
    else hipLaunchKernelGGL((zj_hist_kernel<3, false>), grid, dim3(TONE_NT), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_tone_lut(const ToneLutParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > TONE_LUT_BATCH || (p.channels != 1 && p.channels != 3) || !p.luts) return hipErrorInvalidValue;
    for (int i = 0; i < p.nimg; i++)
        if (!tone_op_valid(p.op[i], p.param[i]) || (tone_needs_hist(p.op[i]) && !p.hist)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zj_tone_lut_kernel, dim3((unsigned)p.nimg), dim3(TONE_NT), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_lut(int channels, int chw, const LutParams& p, hipStream_t s)
{
    if (p.nimg <= 0 || p.nimg > LUT_BATCH || !tone_sizes_ok(p) || (channels != 1 && channels != 3) || !p.luts) return hipErrorInvalidValue;
    const dim3 grid((unsigned)lut_grid(p), 1, (unsigned)p.nimg);
    if (channels == 1) hipLaunchKernelGGL((zj_lut_kernel<1, false>), grid, dim3(TONE_NT), 0, s, p);
    else if (chw) hipLaunchKernelGGL((zj_lut_kernel<3, true>), grid, dim3(TONE_NT), 0, s, p);
    else hipLaunchKernelGGL((zj_lut_kernel<3, false>), grid, dim3(TONE_NT), 0, s, p);
    return hipGetLastError();
}

} // namespace zj

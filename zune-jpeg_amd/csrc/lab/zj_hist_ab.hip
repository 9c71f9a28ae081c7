// zj_hist_ab.hip -- tools only (`make hist_ab`, profiles/tone.txt): the histogram kernel's two ways of counting a lane's run,
// one LDS add per byte against one add per stretch of equal neighbours (zj_tone.h: hist_count_phase<C, CHW, MERGE>), timed in
// one process on 16 interleaved RGB images of 4096 x 4096 of three kinds: uniformly random bytes, one value, and a smooth
// ramp with two bits of noise (neighbours often equal, as in sky or a dark border).  The variants alternate in every round,
// HIP events around memset + launch, and their tables are compared.  Nothing of it is linked into the library.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../zj_tone.h"

using namespace zj;

#define CHECK(call)                                                                              \
    do {                                                                                         \
        const hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) { printf("%s: %s\n", #call, hipGetErrorString(e_)); return 1; }    \
    } while (0)

template <bool MERGE>
__global__ __launch_bounds__(TONE_NT) void hist_ab_kernel(const HistParams p)
{
    __shared__ uint32_t lds[3 * 256];
    const int img = (int)blockIdx.z, tid = (int)threadIdx.x;
    if (!hist_block_active(p, img, blockIdx.x)) return;
    hist_zero_phase<3>(lds, tid);
    __syncthreads();
    hist_count_phase<3, false, MERGE>(p, img, blockIdx.x, tid, lds);
    __syncthreads();
    hist_flush_phase<3>(p, img, tid, lds);
}

// kind 0: random bytes (a hash of the byte's index), 1: one value per image, 2: a ramp of 8 x 8 steps with two bits of noise
__global__ void fill(uint8_t* a, const size_t n, const int side, const int kind)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t h = (uint32_t)i * 2654435761u ^ (uint32_t)(i >> 32);
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        const size_t px = i / 3;
        const uint32_t x = (uint32_t)(px % side), y = (uint32_t)(px / side % side), c = (uint32_t)(i % 3);
        a[i] = kind == 0 ? (uint8_t)h : kind == 1 ? (uint8_t)(90 + px / ((size_t)side * side)) : (uint8_t)(((x >> 3) + (y >> 3) + 40 * c) + ((h >> 8 & 3) == 0));
    }
}

int main()
{
    const int n = 16, side = 4096, rounds = 12;
    const size_t img = (size_t)3 * side * side;
    uint8_t* a = nullptr;
    uint32_t* hist = nullptr;
    CHECK(hipMalloc(&a, n * img));
    CHECK(hipMalloc(&hist, (size_t)n * 768 * 4));
    HistParams p{};
    p.nimg = n;
    for (int i = 0; i < n; i++) {
        p.in[i] = (uint64_t)(uintptr_t)(a + i * img); p.hist[i] = (uint64_t)(uintptr_t)(hist + i * 768);
        p.wh[i] = (uint32_t)side | (uint32_t)side << 16; p.pitch[i] = 3 * side;
    }
    const dim3 grid((unsigned)hist_grid(p), 1, n);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const char* names[3] = {"random", "flat", "ramp + noise"};
    for (int kind = 0; kind < 3; kind++) {
        hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, a, n * img, side, kind);
        CHECK(hipDeviceSynchronize());
        std::vector<float> t[2];
        std::vector<uint32_t> got[2] = {std::vector<uint32_t>(n * 768), std::vector<uint32_t>(n * 768)};
        for (int r = 0; r < rounds + 2; r++)
            for (int v = 0; v < 2; v++) {
                CHECK(hipEventRecord(e0, 0));
                CHECK(hipMemsetAsync(hist, 0, (size_t)n * 768 * 4, 0));
                if (v) hipLaunchKernelGGL(hist_ab_kernel<true>, grid, dim3(TONE_NT), 0, 0, p);
                else hipLaunchKernelGGL(hist_ab_kernel<false>, grid, dim3(TONE_NT), 0, 0, p);
                CHECK(hipGetLastError());
                CHECK(hipEventRecord(e1, 0));
                CHECK(hipEventSynchronize(e1));
                float ms = 0;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r >= 2) t[v].push_back(ms);
                if (r == 0) CHECK(hipMemcpy(got[v].data(), hist, (size_t)n * 768 * 4, hipMemcpyDeviceToHost));
            }
        unsigned long long sum = 0;
        for (uint32_t x : got[0]) sum += x;
        const bool same = got[0] == got[1] && sum == (unsigned long long)n * img;
        for (int v = 0; v < 2; v++) {
            std::sort(t[v].begin(), t[v].end());
            printf("hist_ab: 16 x 4096x4096 HWC %-13s %-20s median %8.1f us  min %8.1f us\n", names[kind],
                   v ? "one add per stretch" : "one add per byte", t[v][t[v].size() / 2] * 1000, t[v][0] * 1000);
        }
        printf("hist_ab: %-13s tables %s\n", names[kind], same ? "equal, every byte counted" : "DIFFER");
        if (!same) return 1;
    }
    return 0;
}

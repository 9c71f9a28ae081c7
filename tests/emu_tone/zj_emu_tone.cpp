// zj_emu_tone.cpp -- CPU EMULATION of the tone stages' kernels (zune-jpeg_amd/csrc/zj_tone.hip: zj_hist_kernel,
// zj_tone_lut_kernel, zj_lut_kernel).
//
// TEST INFRASTRUCTURE ONLY, like tests/emu_color and tests/emu_orient: the kernels' ZJ_HD phases (zj_tone.h) built by g++ with
// ZJ_EMU and -ffp-contract=off, every lane of every workgroup of the launch's grid run one after the other, phase by phase
// (a phase ends where the kernel has a barrier).  The workgroup's LDS is poisoned before each workgroup.  Every store of the
// lookup is counted in a write map over the caller's destination arena, every load of an image byte in a read map over the
// caller's source arena; a store or a load that falls outside its arena is counted apart and NOT performed (the load yields
// 0).  The tables and the histograms are the caller's own arrays and are accessed as they are.  Never linked into
// libzjhip.so.
#define ZJ_EMU 1
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../emu_common/zj_emu_arena.h"

static uint8_t* g_rmap = nullptr; // one count per byte of [g_rlo, g_rhi)
static uint64_t g_rlo = 0, g_rhi = 0;
#define ZJ_EXPAND_PUT(T, addr, v) emu_put<T>((addr), (v))
#define ZJ_TONE_TABLE(T, addr) (*reinterpret_cast<const T*>((uintptr_t)(addr)))
#define ZJ_TONE_TABLE_PUT(addr, v) (*reinterpret_cast<uint8_t*>((uintptr_t)(addr)) = (v))

// a load of an image byte: the address it may read from, counted; outside the source arena: zeros, counted apart
static const uint8_t g_zero[16] __attribute__((aligned(16))) = {0};
template <typename T>
static inline T* emu_at(uint64_t a)
{
    if (a < g_rlo || a + sizeof(T) > g_rhi) { g_outside++; return reinterpret_cast<T*>(const_cast<uint8_t*>(g_zero)); }
    for (size_t k = 0; k < sizeof(T); k++)
        if (g_rmap[a - g_rlo + k] < 255) g_rmap[a - g_rlo + k]++;
    return reinterpret_cast<T*>((uintptr_t)a);
}

#include "../../zune-jpeg_amd/csrc/zj_resize.h"
// (every image load of zj_tone.h goes through cmyk_get, which forms its addresses with this macro; the lookup's stores go
// through ZJ_EXPAND_PUT above)
#undef ZJ_RZ_GLOBAL
#define ZJ_RZ_GLOBAL(T, v) (emu_at<T>((uint64_t)(v)))
#include "../../zune-jpeg_amd/csrc/zj_tone.h"
// (the other stages' headers, which come with zj_stage_pack.h and are not run here, load as they are written)
#undef ZJ_RZ_GLOBAL
#define ZJ_RZ_GLOBAL(T, v) (reinterpret_cast<T*>(v))
#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

static const int POISON = 0xA5;

template <int C, bool CHW>
static void run_hist(const HistParams& p)
{
    const int gx = hist_grid(p);
    for (int z = 0; z < p.nimg; z++)
        for (int bx = 0; bx < gx; bx++) {
            if (!hist_block_active(p, z, (uint32_t)bx)) continue;
            uint32_t lds[C * 256];
            memset(lds, POISON, sizeof lds);
            for (int t = 0; t < TONE_NT; t++) hist_zero_phase<C>(lds, t);
            for (int t = 0; t < TONE_NT; t++) hist_count_phase<C, CHW>(p, z, (uint32_t)bx, t, lds);
            for (int t = 0; t < TONE_NT; t++) hist_flush_phase<C>(p, z, t, lds);
        }
}

static void run_tone_lut(const ToneLutParams& p)
{
    for (int img = 0; img < p.nimg; img++) {
        ToneLutLds l;
        memset(&l, POISON, sizeof l);
        const int32_t op = p.op[img];
        for (int c = 0; c < p.channels; c++) {
            if (tone_needs_hist(op)) {
                uint32_t hv[TONE_NT];
                for (int t = 0; t < TONE_NT; t++) hv[t] = tone_lut_load_phase(p, img, c, t, l);
                for (int t = 0; t < TONE_NT; t++) tone_lut_reduce_phase(t, hv[t], l);
                if (op == TONE_EQUALIZE)
                    for (int step = 0; step < 8; step++)
                        for (int t = 0; t < TONE_NT; t++) tone_lut_scan_phase(t, step, l);
            }
            for (int t = 0; t < TONE_NT; t++) tone_lut_entry_phase(p, img, c, t, l);
        }
    }
}

template <int C, bool CHW>
static void run_lut(const LutParams& p)
{
    const int gx = lut_grid(p);
    for (int z = 0; z < p.nimg; z++)
        for (int bx = 0; bx < gx; bx++) {
            if (!lut_block_active(p, z, (uint32_t)bx)) continue;
            uint32_t lds[C * 64];
            memset(lds, POISON, sizeof lds);
            for (int t = 0; t < TONE_NT; t++) lut_table_phase<C>(p, z, t, lds);
            for (int t = 0; t < TONE_NT; t++) lut_map_phase<C, CHW>(p, z, (uint32_t)bx * TONE_NT + (uint32_t)t, reinterpret_cast<const uint8_t*>(lds));
        }
}

// 0: TONE_RUN, 1: TONE_NT, 2: HIST_RUNS, 3: HIST_BATCH, 4: TONE_LUT_BATCH, 5: LUT_BATCH, 6..8: the records' sizes
extern "C" int zjtn_const(int k)
{
    const int v[] = {TONE_RUN, TONE_NT, HIST_RUNS, HIST_BATCH, TONE_LUT_BATCH, LUT_BATCH, (int)sizeof(HistParams), (int)sizeof(ToneLutParams),
                     (int)sizeof(LutParams)};
    return k >= 0 && k < 9 ? v[k] : -1;
}

extern "C" int zjtn_op_valid(int op, int param) { return tone_op_valid(op, param) ? 1 : 0; }

static bool args_ok(int n, int channels, const unsigned* wh) { return n > 0 && (channels == 1 || channels == 3) && stage_sizes((size_t)n, wh); }

// n images as the launches of the library's call (HIST_BATCH images each): hist, uint32 [n][channels][256], zeroed first as the
// library zeroes it on the stream.  Every source byte must lie in [src, src + src_len): rmap gets the number of times each
// byte was loaded; returns the loads that fell outside (not performed), < 0: arguments
extern "C" long long zjtn_hist(int n, const uint8_t* const* in, const unsigned* wh, const unsigned* pitch, int channels, int chw,
                               uint32_t* hist, const uint8_t* src, size_t src_len, uint8_t* rmap)
{
    if (!args_ok(n, channels, wh)) return -1;
    emu_arena(nullptr, 0, nullptr);
    g_rmap = rmap; g_rlo = (uint64_t)(uintptr_t)src; g_rhi = g_rlo + src_len;
    memset(hist, 0, (size_t)n * channels * 1024);
    std::vector<const uint8_t*> tabs((size_t)n);
    for (int f = 0; f < n; f++) tabs[f] = (const uint8_t*)(hist + (size_t)f * channels * 256);
    HistParams p{};
    stage_batches<HIST_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_hist(p, in, wh, pitch, tabs.data(), f0, m);
        if (channels == 1) run_hist<1, false>(p);
        else if (chw) run_hist<3, true>(p);
        else run_hist<3, false>(p);
        return 0;
    });
    return g_outside;
}

// the tables of n ops (op, param pairs) from hist (nullptr: no op needs it) into luts, uint8 [n][channels][256]; < 0: an op the
// stage refuses, or one that needs the bins without any
extern "C" int zjtn_luts(int n, int channels, const int32_t* ops, const uint32_t* hist, uint8_t* luts)
{
    if (n <= 0 || (channels != 1 && channels != 3)) return -1;
    for (int f = 0; f < n; f++)
        if (!tone_op_valid(ops[2 * f], ops[2 * f + 1]) || (tone_needs_hist(ops[2 * f]) && !hist)) return -1;
    ToneLutParams p{};
    stage_batches<TONE_LUT_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_tone_lut(p, ops, hist, luts, channels, f0, m);
        run_tone_lut(p);
        return 0;
    });
    return 0;
}

// n images through their tables as the launches of the library's call (LUT_BATCH images each).  Every source byte must lie in
// [src, src + src_len), every destination byte in [arena, arena + len) (in place: the same range): rmap / wmap get the number
// of times each byte was loaded / stored; returns the loads and stores that fell outside (not performed), < 0: arguments
extern "C" long long zjtn_lut(int n, const uint8_t* const* in, const unsigned* wh, const unsigned* in_pitch, int channels, int chw,
                              const uint8_t* luts, uint8_t* const* out, const unsigned* out_pitch, const uint8_t* src, size_t src_len,
                              uint8_t* rmap, uint8_t* arena, size_t len, uint8_t* wmap)
{
    if (!args_ok(n, channels, wh)) return -1;
    emu_arena(arena, len, wmap);
    g_rmap = rmap; g_rlo = (uint64_t)(uintptr_t)src; g_rhi = g_rlo + src_len;
    LutParams p{};
    stage_batches<LUT_BATCH>((size_t)n, [&](size_t f0, int m) {
        pack_lut(p, in, wh, in_pitch, luts, channels, out, out_pitch, f0, m);
        if (channels == 1) run_lut<1, false>(p);
        else if (chw) run_lut<3, true>(p);
        else run_lut<3, false>(p);
        return 0;
    });
    return g_outside;
}

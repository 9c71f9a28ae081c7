// zj_emu_cbyte.cpp -- CPU EMULATION of the fused tile kernel with byte chroma (Cfg::CBYTE, zune-jpeg_amd/csrc/zj_device.h).
//
// TEST INFRASTRUCTURE ONLY (tests/test_chroma_bytes_emu.py).  It runs the workgroup phases thread by thread as tests/emu
// does, and differs from it where the byte path differs from the pair path: the tile's redo flag is honoured for EVERY
// output, as fused_body of zj_kernels.hip honours it (a DC-only chroma value outside 0..255 cannot be staged as a byte,
// whatever happens to the pixels afterwards), so the YCbCr instantiations take the byte path here as they do on the GPU.
#define ZJ_EMU 1
#define ZJ_EMU_REDO_ANY 1
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_plan.h"

using namespace zj;

static int g_variant = 0; // 0 packed generation (staged stores where they apply), 2 packed with direct stores
extern "C" void zjc_set_variant(int v) { g_variant = v; }
// of the last zjc_decode_planes call: tiles decoded, tiles redone wide, tiles whose chroma was staged as bytes
static long long g_tiles = 0, g_redo = 0, g_byte_tiles = 0;
extern "C" void zjc_stats(long long out[3]) { out[0] = g_tiles; out[1] = g_redo; out[2] = g_byte_tiles; }

// tri_b (two byte averages) over n bytes, n a multiple of 4: the filter by itself
extern "C" void zjc_tri_b(const uint8_t* near_, const uint8_t* far_, uint8_t* out, size_t n)
{
    for (size_t i = 0; i + 4 <= n; i += 4) {
        uint32_t a, b;
        memcpy(&a, near_ + i, 4);
        memcpy(&b, far_ + i, 4);
        const uint32_t r = tri_b(a, b);
        memcpy(out + i, &r, 4);
    }
}

template <class C, int HS, int VS, int OUT, bool FAST, bool RAG>
static void tile_wide(const Params& p, const TileId t, char* lds)
{
    for (int tid = 0; tid < C::NT; tid++) phase_setup<C, HS, VS, GEN_WIDE>(p, tid, lds);
    /* __syncthreads() */
    for (int tid = 0; tid < C::NT; tid++) {
        const BlockLoc L = locate<C, GEN_WIDE>(p, t, tid, lds);
        U4 raw[8];
        load_block(L, raw);
        finish_block<C, GEN_WIDE, false>(L, raw, lds, 0, p.clamp_dc);
    }
    /* __syncthreads() */
    for (int tid = 0; tid < C::NT; tid++) phase_color<C, HS, VS, OUT, GEN_WIDE, FAST, false, RAG>(p, t, tid, lds);
}

template <int HS, int VS, int OUT, bool FAST, bool RAG = false>
static void run(const Params& p)
{
    using C = Cfg<HS, VS, OUT>;
    constexpr bool NEED_Y16 = OUT == OUT_RGB || OUT == OUT_RGBA || OUT == OUT_RGB_CHW;
    constexpr bool CAN_TS = FAST && C::TSCAP;
    std::vector<char> lds_store(C::LDS_PACKED + 32);
    char* lds = (char*)(((uintptr_t)lds_store.data() + 15) & ~(uintptr_t)15); // 16-byte aligned like a real LDS allocation
    const bool ts = CAN_TS && g_variant == 0 && ts_eligible<C>(p, OUT, FAST, RAG);
    for (int bid = 0; bid < p.total_tiles; bid++) {
        memset(lds, 0x7B, C::LDS_PACKED); // poison: unwritten LDS must not matter
        const TileId t = decode_tile(p, bid);
        g_tiles++;
        if (C::CBYTE) g_byte_tiles++;
        for (int tid = 0; tid < C::NT; tid++) phase_setup<C, HS, VS, GEN_PACKED>(p, tid, lds);
        /* __syncthreads() */
        const int nblock_lanes = C::HALO_PURE ? C::HALO_T0 : C::NT;
        for (int tid = 0; tid < nblock_lanes; tid++) {
            const BlockLoc L = locate<C, GEN_PACKED>(p, t, tid, lds);
            U4 raw[8];
            load_block(L, raw);
            finish_block<C, GEN_PACKED, NEED_Y16>(L, raw, lds, 0, p.clamp_dc);
        }
        if (C::HALO_PURE) { // the halo wave: one lane per block column; all lanes do pass 1, then all do pass 2
            HaloLane H[64];
            for (int hl = 0; hl < 64; hl++) {
                H[hl] = halo_locate<C>(p, t, hl, lds);
                int32_t s8[8];
                halo_load(H[hl], s8);
                halo_pass1<C>(H[hl], s8, lds);
            }
            for (int hl = 0; hl < 64; hl++) halo_pass2<C>(H[hl], lds, p.clamp_dc);
            for (int hl = 0; hl < 64; hl++) halo_filter<C, HS, VS>(p, t, hl, lds);
        }
        /* __syncthreads() */
        if ((NEED_Y16 || C::CBYTE) && *lds_flag<C>(lds) != 0) { // a Q1 value outside a byte: the whole tile again, wide
            g_redo++;
            memset(lds, 0x7B, C::LDS_PACKED);
            tile_wide<C, HS, VS, OUT, FAST, RAG>(p, t, lds);
            continue;
        }
        if (ts) {
            for (int round = 0; round * C::NT < C::NITEMS; round++)
                for (int w = 0; w < C::NW; w++) {
                    ItemOut io[64];
                    for (int l = 0; l < 64; l++) phase_color<C, HS, VS, OUT, GEN_PACKED, FAST, CAN_TS, RAG>(p, t, round_tid<C>(64 * w + l, round), lds, round, &io[l]);
                    for (int l = 0; l < 64; l++) stage_item<C>(io[l], round_tid<C>(64 * w + l, round), lds, round, w);
                    for (int l = 0; l < 64; l++) color_copyout<C, OUT, RAG>(p, t, round_tid<C>(64 * w + l, round), lds, round, w);
                }
        } else {
            for (int tid = 0; tid < C::NT; tid++) phase_color<C, HS, VS, OUT, GEN_PACKED, FAST, false, RAG>(p, t, tid, lds);
        }
    }
}

// the horizontally sub-sampled modes with chroma: the instantiations the byte path exists in
static int dispatch(const Plan& pl, const Params& p)
{
    const int mode = launch_mode(pl, g_variant);
#define ZJ_CASE(H, V, O) if (pl.hs == H && pl.vs == V && pl.out == O) { if (mode == 2) run<H, V, O, true, true>(p); else if (mode == 1) run<H, V, O, true>(p); else run<H, V, O, false>(p); return ZJ_OK; }
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_YCBCR) ZJ_CASE(2, 1, OUT_RGBA) ZJ_CASE(2, 1, OUT_RGB_CHW)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_YCBCR) ZJ_CASE(2, 2, OUT_RGBA) ZJ_CASE(2, 2, OUT_RGB_CHW)
#undef ZJ_CASE
    return ZJ_ERR_UNSUPPORTED;
}

extern "C" int zjc_decode_planes(const zj_frame_desc* d, size_t nframes, const int16_t* y, const int16_t* cb, const int16_t* cr,
                                 uint8_t* out, int zero_fill)
{
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    if (g_variant != 0 && g_variant != 2) return ZJ_ERR_UNSUPPORTED;
    Params p;
    fill_params(d, pl, nframes, y, cb, cr, out, zero_fill, p);
    g_tiles = g_redo = g_byte_tiles = 0;
    if (zero_fill) { // same remainder memset as zj_api.cpp
        size_t off[3], len[3];
        const int nr = uncovered_ranges(d, pl, off, len);
        for (size_t f = 0; f < nframes; f++)
            for (int r = 0; r < nr; r++) memset(out + f * pl.out_len + off[r], 0, len[r]);
    }
    return dispatch(pl, p);
}

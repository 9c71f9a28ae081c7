// zj_emu_interior.cpp -- CPU EMULATION of the fused tile kernel with the interior form of its colour rounds (Cfg::INTERIOR,
// interior_tile; zune-jpeg_amd/csrc/zj_device.h, fused_body of zj_kernels.hip).
//
// TEST INFRASTRUCTURE ONLY (tests/test_interior_emu.py).  It runs the workgroup phases thread by thread as tests/emu_cbyte
// does (the redo flag honoured for every output), takes the branch at the head of the colour phase as fused_body takes it,
// and records for every tile which way it went.  Built twice: with -DZJ_INTERIOR=1 and with -DZJ_INTERIOR=0.
#define ZJ_EMU 1
#define ZJ_EMU_REDO_ANY 1
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_plan.h"

using namespace zj;

// of the last zjc_decode_planes call, four numbers per tile: frame, strip, tile, and the way its colour phase went -- 0 general
// rounds, 1 interior rounds, 2 redone by the wide code, 3 direct stores (the launch was not eligible for staged stores)
static std::vector<int32_t> g_way;
static void record(const TileId& t, const int way) { g_way.insert(g_way.end(), {t.frame, t.strip, t.tile, way}); }
extern "C" long long zjc_tiles(void) { return (long long)(g_way.size() / 4); }
extern "C" void zjc_ways(int32_t* out) { memcpy(out, g_way.data(), g_way.size() * sizeof(int32_t)); }
extern "C" int zjc_knob(void) { return ZJ_INTERIOR; }

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

// fused_body's interior_rounds: a wave's three steps of a round one after the other, lane by lane
template <class C, int HS, int VS, int OUT>
static void interior_rounds(const Params& p, const TileId t, char* lds)
{
    if constexpr (C::INTERIOR) {
        for (int round = 0; round * C::NT < C::NITEMS; round++)
            for (int w = 0; w < C::NW; w++) {
                ItemOut io[64];
                for (int l = 0; l < 64; l++) phase_color<C, HS, VS, OUT, GEN_PACKED, true, true, false, true>(p, t, 64 * w + l, lds, round, &io[l]);
                for (int l = 0; l < 64; l++) stage_item<C, true>(io[l], 64 * w + l, lds, round);
                for (int l = 0; l < 64; l++) color_copyout<C, OUT, false, false, true>(p, t, 64 * w + l, lds, round);
            }
    }
}

template <int HS, int VS, int OUT, bool FAST, bool RAG = false>
static void run(const Params& p)
{
    using C = Cfg<HS, VS, OUT>;
    constexpr bool NEED_Y16 = OUT == OUT_RGB || OUT == OUT_RGBA || OUT == OUT_RGB_CHW;
    constexpr bool CAN_TS = FAST && C::TSCAP;
    constexpr bool INTERIOR = C::INTERIOR && FAST && !RAG; // as in fused_body (the emulation has no seam family)
    std::vector<char> lds_store(C::LDS_PACKED + 32);
    char* lds = (char*)(((uintptr_t)lds_store.data() + 15) & ~(uintptr_t)15); // 16-byte aligned like a real LDS allocation
    const bool ts = CAN_TS && ts_eligible<C>(p, OUT, FAST, RAG);
    for (int bid = 0; bid < p.total_tiles; bid++) {
        memset(lds, 0x7B, C::LDS_PACKED); // poison: unwritten LDS must not matter
        const TileId t = decode_tile(p, bid);
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
            record(t, 2);
            memset(lds, 0x7B, C::LDS_PACKED);
            tile_wide<C, HS, VS, OUT, FAST, RAG>(p, t, lds);
            continue;
        }
        if (!ts) {
            record(t, 3);
            for (int tid = 0; tid < C::NT; tid++) phase_color<C, HS, VS, OUT, GEN_PACKED, FAST, false, RAG>(p, t, tid, lds);
            continue;
        }
        if (INTERIOR && interior_tile<C>(p, t)) { // the one branch at the head of the colour phase
            record(t, 1);
            interior_rounds<C, HS, VS, OUT>(p, t, lds);
            continue;
        }
        record(t, 0);
        for (int round = 0; round * C::NT < C::NITEMS; round++)
            for (int w = 0; w < C::NW; w++) {
                ItemOut io[64];
                for (int l = 0; l < 64; l++) phase_color<C, HS, VS, OUT, GEN_PACKED, FAST, CAN_TS, RAG>(p, t, round_tid<C>(64 * w + l, round), lds, round, &io[l]);
                for (int l = 0; l < 64; l++) stage_item<C>(io[l], round_tid<C>(64 * w + l, round), lds, round, w);
                for (int l = 0; l < 64; l++) color_copyout<C, OUT, RAG>(p, t, round_tid<C>(64 * w + l, round), lds, round, w);
            }
    }
}

// the horizontally sub-sampled modes with the interleaved outputs: the instantiations that stage their stores
static int dispatch(const Plan& pl, const Params& p)
{
    const int mode = launch_mode(pl, 0);
#define ZJ_CASE(H, V, O) if (pl.hs == H && pl.vs == V && pl.out == O) { if (mode == 2) run<H, V, O, true, true>(p); else if (mode == 1) run<H, V, O, true>(p); else run<H, V, O, false>(p); return ZJ_OK; }
    ZJ_CASE(2, 1, OUT_RGB) ZJ_CASE(2, 1, OUT_YCBCR) ZJ_CASE(2, 1, OUT_RGBA)
    ZJ_CASE(2, 2, OUT_RGB) ZJ_CASE(2, 2, OUT_YCBCR) ZJ_CASE(2, 2, OUT_RGBA)
#undef ZJ_CASE
    return ZJ_ERR_UNSUPPORTED;
}

extern "C" int zjc_decode_planes(const zj_frame_desc* d, size_t nframes, const int16_t* y, const int16_t* cb, const int16_t* cr,
                                 uint8_t* out, int zero_fill)
{
    Plan pl;
    int rc = make_plan(d, pl);
    if (rc) return rc;
    Params p;
    fill_params(d, pl, nframes, y, cb, cr, out, zero_fill, p);
    g_way.clear();
    if (zero_fill) { // same remainder memset as zj_api.cpp
        size_t off[3], len[3];
        const int nr = uncovered_ranges(d, pl, off, len);
        for (size_t f = 0; f < nframes; f++)
            for (int r = 0; r < nr; r++) memset(out + f * pl.out_len + off[r], 0, len[r]);
    }
    return dispatch(pl, p);
}

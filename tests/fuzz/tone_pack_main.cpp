// tone_pack_main.cpp -- a stand-alone check of the tone stages' part of zune-jpeg_amd/csrc/zj_stage_pack.h (pack_hist,
// pack_tone_lut, pack_lut) for tests/test_tone_pack.py, built by g++ under AddressSanitizer + UBSan: the
// three records of random calls -- 1, BATCH, BATCH + 1, 2 BATCH + 5 and random numbers of images, one or three channels --
// packed over a poisoned record and compared field by field with the inputs, the tail slots zero; the ops' argument rule and
// the size / pitch rule through their refusals, each next to a good neighbour.
// TEST INFRASTRUCTURE ONLY; nothing of HIP, never linked into libzjhip.so.  No pointer in here is ever followed.
#define ZJ_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

static int g_fail = 0;
static unsigned g_pitch_max = 1u << 24; // argv[1]: the limit the tests assume
#define CHECK(x)                                                                         \
    do {                                                                                 \
        if (!(x) && g_fail++ < 20) printf("FAILED line %d: %s\n", __LINE__, #x);         \
    } while (0)
#define SLOT(field, value) CHECK(p.field == (i < m ? (value) : 0))

static std::mt19937_64 g_rng(20261021);
static uint64_t rnd(uint64_t lo, uint64_t hi) { return lo + g_rng() % (hi - lo + 1); }

// a random call: a pointer per array, a size, a pitch on each side, a table and an op per image
struct Call {
    size_t n;
    int channels;
    std::vector<const uint8_t*> in, hist;
    std::vector<uint8_t*> out;
    std::vector<unsigned> wh, in_pitch, out_pitch;
    std::vector<int32_t> ops;
    Call(size_t n_, int channels_) : n(n_), channels(channels_)
    {
        for (size_t f = 0; f < n; f++) {
            in.push_back((const uint8_t*)(uintptr_t)rnd(1, ~0ull >> 1)); out.push_back((uint8_t*)(uintptr_t)rnd(1, ~0ull >> 1));
            hist.push_back((const uint8_t*)(uintptr_t)(rnd(1, ~0ull >> 3) * 4));
            const unsigned w = (unsigned)rnd(1, 65535), h = (unsigned)rnd(1, 65535);
            wh.push_back(w); wh.push_back(h);
            in_pitch.push_back((unsigned)rnd(w * 3, g_pitch_max)); out_pitch.push_back((unsigned)rnd(w * 3, g_pitch_max));
            const int32_t op = (int32_t)rnd(0, 5);
            ops.push_back(op);
            ops.push_back(op == TONE_POSTERIZE ? (int32_t)rnd(1, 8) : op == TONE_SOLARIZE ? (int32_t)rnd(0, 256) : 0);
        }
    }
};

template <int BATCH, class P, class Pack, class Check>
static void launches(size_t n, Pack pack, Check check)
{
    size_t next = 0;
    const int rc = stage_batches<BATCH>(n, [&](size_t f0, int m) {
        CHECK(f0 == next && m == (int)(n - f0 < (size_t)BATCH ? n - f0 : (size_t)BATCH));
        next = f0 + m;
        P p;
        memset(&p, 0xA5, sizeof p);
        pack(p, f0, m);
        CHECK(p.nimg == m);
        check(p, f0, m);
        return 0;
    });
    CHECK(rc == 0 && next == n);
}

static void one(size_t n, int channels)
{
    const Call c(n, channels);
    launches<HIST_BATCH, HistParams>(
        n, [&](HistParams& p, size_t f0, int m) { pack_hist(p, c.in.data(), c.wh.data(), c.in_pitch.data(), c.hist.data(), f0, m); },
        [&](const HistParams& p, size_t f0, int m) {
            for (int i = 0; i < HIST_BATCH; i++) {
                const size_t f = f0 + i;
                SLOT(in[i], stage_ptr(c.in[f])); SLOT(hist[i], stage_ptr(c.hist[f]));
                SLOT(wh[i], c.wh[2 * f] | c.wh[2 * f + 1] << 16); SLOT(pitch[i], c.in_pitch[f]);
            }
            CHECK(hist_grid(p) >= 1);
        });
    uint32_t* const hist = (uint32_t*)(uintptr_t)0x7000000000ull;
    uint8_t* const luts = (uint8_t*)(uintptr_t)0x6000000001ull;
    for (const uint32_t* h : {(const uint32_t*)hist, (const uint32_t*)nullptr})
        launches<TONE_LUT_BATCH, ToneLutParams>(
            n, [&](ToneLutParams& p, size_t f0, int m) { pack_tone_lut(p, c.ops.data(), h, luts, channels, f0, m); },
            [&](const ToneLutParams& p, size_t f0, int m) {
                CHECK(p.channels == channels);
                CHECK(p.hist == (h ? stage_ptr(hist) + f0 * (uint64_t)channels * 1024 : 0));
                CHECK(p.luts == stage_ptr(luts) + f0 * (uint64_t)channels * 256);
                for (int i = 0; i < TONE_LUT_BATCH; i++) {
                    const size_t f = f0 + i;
                    SLOT(op[i], c.ops[2 * f]); SLOT(param[i], c.ops[2 * f + 1]);
                    if (i < m) CHECK(tone_op_valid(p.op[i], p.param[i]));
                }
            });
    launches<LUT_BATCH, LutParams>(
        n, [&](LutParams& p, size_t f0, int m) { pack_lut(p, c.in.data(), c.wh.data(), c.in_pitch.data(), luts, channels, c.out.data(), c.out_pitch.data(), f0, m); },
        [&](const LutParams& p, size_t f0, int m) {
            CHECK(p.luts == stage_ptr(luts) + f0 * (uint64_t)channels * 256);
            for (int i = 0; i < LUT_BATCH; i++) {
                const size_t f = f0 + i;
                SLOT(in[i], stage_ptr(c.in[f])); SLOT(out[i], stage_ptr(c.out[f]));
                SLOT(wh[i], c.wh[2 * f] | c.wh[2 * f + 1] << 16);
                SLOT(in_pitch[i], c.in_pitch[f]); SLOT(out_pitch[i], c.out_pitch[f]);
            }
            CHECK(lut_grid(p) >= 1);
        });
}

static void rules()
{
    // the ops: every (op, param) of a range around the valid ones against the table of the header
    for (int32_t op = -3; op <= 9; op++)
        for (int32_t param = -3; param <= 300; param++) {
            const bool want = op == 2 ? param >= 1 && param <= 8 : op == 3 ? param >= 0 && param <= 256 : op >= 0 && op <= 5 && param == 0;
            CHECK(tone_op_valid(op, param) == want);
        }
    CHECK(!tone_op_valid(INT32_MIN, 0) && !tone_op_valid(INT32_MAX, 0) && !tone_op_valid(2, INT32_MAX) && !tone_op_valid(3, INT32_MIN));
    for (int32_t op = 0; op <= 5; op++) CHECK(tone_needs_hist(op) == (op == 4 || op == 5));
    // the size / pointer / pitch rule as the tone calls use it: a bad image behind a good one
    const uint8_t* const ptr[2] = {(const uint8_t*)16, (const uint8_t*)32};
    const uint8_t* const hole[2] = {(const uint8_t*)16, nullptr};
    std::vector<unsigned> r;
    const unsigned ok[4] = {4, 4, 65535, 65535};
    CHECK(stage_images(2, ptr, ok, nullptr, 3, r) && r[0] == 12 && r[1] == 3 * 65535);
    CHECK(!stage_images(2, hole, ok, nullptr, 3, r));
    for (unsigned bad : {0u, 65536u}) {
        const unsigned w[4] = {4, 4, bad, 4}, h[4] = {4, 4, 4, bad};
        CHECK(!stage_images(2, ptr, w, nullptr, 1, r) && !stage_images(2, ptr, h, nullptr, 1, r));
    }
    const unsigned small[4] = {4, 4, 4, 4};
    const unsigned below[2] = {12, 11}, limit[2] = {g_pitch_max, 0}, over[2] = {12, g_pitch_max + 1};
    CHECK(!stage_side(2, ptr, below, small, 3, r) && !stage_side(2, ptr, over, small, 3, r));
    CHECK(stage_side(2, ptr, limit, small, 3, r) && r[0] == g_pitch_max && r[1] == 12);
    CHECK(stage_side(2, ptr, below, small, 1, r)); // (one byte a pixel: 11 is a pitch)
    // the grids: a workgroup's share of the histogram, a lane's run of the lookup
    HistParams hp{};
    hp.nimg = 2;
    hp.wh[0] = 16u | 1u << 16; hp.wh[1] = (16u * HIST_ITEMS + 1) | 1u << 16;
    CHECK(hist_grid(hp) == 2 && hist_block_active(hp, 0, 0) && !hist_block_active(hp, 0, 1) && hist_block_active(hp, 1, 1) && !hist_block_active(hp, 1, 2));
    hp.wh[1] = 65535u | 65535u << 16;
    CHECK(hist_grid(hp) == (int)((4096ull * 65535 + HIST_ITEMS - 1) / HIST_ITEMS));
    LutParams lp{};
    lp.nimg = 1;
    lp.wh[0] = 65535u | 65535u << 16;
    CHECK(lut_grid(lp) == (int)((4096ull * 65535 + TONE_NT - 1) / TONE_NT) && lut_block_active(lp, 0, (uint32_t)lut_grid(lp) - 1) &&
          !lut_block_active(lp, 0, (uint32_t)lut_grid(lp)));
}

int main(int argc, char** argv)
{
    if (argc > 1) g_pitch_max = (unsigned)strtoul(argv[1], nullptr, 10);
    static_assert(HIST_BATCH == 128 && TONE_LUT_BATCH == 256 && LUT_BATCH == 128, "the batches the header documents");
    for (int channels : {1, 3}) {
        for (size_t n : {(size_t)1, (size_t)HIST_BATCH, (size_t)HIST_BATCH + 1, (size_t)2 * HIST_BATCH + 5, (size_t)TONE_LUT_BATCH,
                         (size_t)TONE_LUT_BATCH + 1, (size_t)2 * TONE_LUT_BATCH + 5})
            one(n, channels);
        for (int k = 0; k < 40; k++) one((size_t)rnd(1, 700), channels);
    }
    rules();
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("tone-pack-clean\n");
    return 0;
}

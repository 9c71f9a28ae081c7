// stage_pack_main.cpp -- a stand-alone check of zune-jpeg_amd/csrc/zj_stage_pack.h for tests/test_stage_pack.py, built by g++
// under AddressSanitizer + UBSan: every launch record of calls of 1, BATCH, BATCH + 1 and 2 BATCH + 5 images, packed over a
// poisoned record and compared field by field with the inputs, and the argument rules through the refusal lists of the
// GPU tests (test_gpu_color, test_gpu_cmyk, test_gpu_gray_rgb, test_gpu_sampling), each next to a good neighbour.
// TEST INFRASTRUCTURE ONLY; nothing of HIP, never linked into libzjhip.so.  No pointer in here is ever followed.
#define ZJ_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_stage_pack.h"

using namespace zj;

static int g_fail = 0;
static unsigned g_pitch_max = 1u << 24; // argv[1]: the limit the tests assume
#define CHECK(x)                                                                         \
    do {                                                                                 \
        if (!(x) && g_fail++ < 20) printf("FAILED line %d: %s\n", __LINE__, #x);         \
    } while (0)

// image f of a call: a pointer per array, a size, a pitch per array, a flag on every third image
static const uint64_t IN = 0x10000000ull, IN2 = 0x20000000ull, IN3 = 0x30000000ull, OUT = 0x40000000ull, TENSOR = 0x50000000ull;
static uint64_t at(uint64_t base, size_t f) { return base + 4096 * f; }
static unsigned W(size_t f) { return 3 + (unsigned)(f % 61); }
static unsigned H(size_t f) { return 2 + (unsigned)(f % 37); }
static unsigned pitch_of(size_t f, unsigned bpp) { return W(f) * bpp + (unsigned)(f % 7); }
static bool flag(size_t f) { return f % 3 == 0; }
static bool bit(const uint32_t* set, int i) { return (set[i >> 5] >> (i & 31)) & 1u; }

struct Call {
    size_t n;
    std::vector<const uint8_t*> in, in2, in3;
    std::vector<uint8_t*> out;
    std::vector<unsigned> wh, pitch, pitch1, pitch3, out_pitch;
    std::vector<uint8_t> flags, o;
    std::vector<int32_t> cq;
    std::vector<int64_t> wq;
    std::vector<uint32_t> geo;
    explicit Call(size_t n_) : n(n_)
    {
        for (size_t f = 0; f < n; f++) {
            in.push_back((const uint8_t*)(uintptr_t)at(IN, f)); in2.push_back((const uint8_t*)(uintptr_t)at(IN2, f));
            in3.push_back((const uint8_t*)(uintptr_t)at(IN3, f)); out.push_back((uint8_t*)(uintptr_t)at(OUT, f));
            wh.push_back(W(f)); wh.push_back(H(f));
            pitch.push_back(pitch_of(f, 3)); pitch1.push_back(pitch_of(f, 1)); out_pitch.push_back(pitch_of(f, 3) + 16);
            for (unsigned k = 0; k < 3; k++) pitch3.push_back(pitch_of(f, 1) + 100 * k);
            flags.push_back(flag(f) ? 1 : 0); o.push_back((uint8_t)(1 + f % 8));
            for (int k = 0; k < 12; k++) cq.push_back((int32_t)(1000 * f + k) - 7);
            for (int k = 0; k < 6; k++) wq.push_back(((int64_t)f << 33) + k - 3);
            geo.push_back((uint32_t)(0x010203u * (f % 5) + f));
        }
    }
};

static StageTensor tensor(int out_w, int out_h, size_t img_bytes)
{
    return StageTensor{(uint8_t*)(uintptr_t)TENSOR, img_bytes, out_w, out_h, RZ_F16, 1, {0.5f, 0.25f, 2.f}, {1.f, -2.f, 3.f}};
}

// the launches of a call of n images through stage_batches<BATCH>: check(p, f0, m) sees each record, packed over poison
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
    // a status that is not 0 ends the call where it is
    int calls = 0;
    CHECK(stage_batches<BATCH>(n, [&](size_t, int) { return ++calls == 1 ? -3 : 0; }) == -3 && calls == 1);
}

#define SLOT(field, value) CHECK(p.field == (i < m ? (value) : 0))

template <int BATCH>
static void sizes(void (*one)(size_t))
{
    for (size_t n : {(size_t)1, (size_t)BATCH, (size_t)BATCH + 1, (size_t)2 * BATCH + 5}) one(n);
}

static void orient(size_t n)
{
    const Call c(n);
    launches<ORIENT_BATCH, OrientParams>(
        n, [&](OrientParams& p, size_t f0, int m) { pack_orient(p, c.in.data(), c.wh.data(), c.pitch.data(), c.o.data(), c.out.data(), c.out_pitch.data(), f0, m); },
        [&](const OrientParams& p, size_t f0, int m) {
            for (int i = 0; i < ORIENT_BATCH; i++) {
                const size_t f = f0 + i;
                SLOT(in[i], at(IN, f)); SLOT(out[i], at(OUT, f)); SLOT(wh[i], W(f) | H(f) << 16);
                SLOT(in_pitch[i], pitch_of(f, 3)); SLOT(out_pitch[i], pitch_of(f, 3) + 16);
                CHECK(p.o[i] == (i < m ? 1 + f % 8 : 1));
            }
        });
}

static void expand(size_t n)
{
    const Call c(n);
    launches<EXPAND_BATCH, ExpandParams>(
        n, [&](ExpandParams& p, size_t f0, int m) { pack_expand(p, c.in.data(), c.wh.data(), c.pitch1.data(), c.out.data(), c.out_pitch.data(), f0, m); },
        [&](const ExpandParams& p, size_t f0, int m) {
            for (int i = 0; i < EXPAND_BATCH; i++) {
                const size_t f = f0 + i;
                SLOT(in[i], at(IN, f)); SLOT(out[i], at(OUT, f)); SLOT(wh[i], W(f) | H(f) << 16);
                SLOT(in_pitch[i], pitch_of(f, 1)); SLOT(out_pitch[i], pitch_of(f, 3) + 16);
            }
        });
}

static void cmyk(size_t n)
{
    const Call c(n);
    for (const uint8_t* inverted : {c.flags.data(), (const uint8_t*)nullptr})
        launches<CMYK_BATCH, CmykParams>(
            n, [&](CmykParams& p, size_t f0, int m) { pack_cmyk(p, c.in.data(), c.in2.data(), c.wh.data(), c.pitch.data(), c.pitch1.data(), inverted, c.out.data(), c.out_pitch.data(), f0, m); },
            [&](const CmykParams& p, size_t f0, int m) {
                for (int i = 0; i < CMYK_BATCH; i++) {
                    const size_t f = f0 + i;
                    SLOT(a[i], at(IN, f)); SLOT(k[i], at(IN2, f)); SLOT(out[i], at(OUT, f)); SLOT(wh[i], W(f) | H(f) << 16);
                    SLOT(a_pitch[i], pitch_of(f, 3)); SLOT(k_pitch[i], pitch_of(f, 1)); SLOT(out_pitch[i], pitch_of(f, 3) + 16);
                    CHECK(bit(p.inverted, i) == (i < m && inverted && flag(f)));
                }
            });
}

static void color(size_t n)
{
    const Call c(n);
    launches<COLOR_BATCH, ColorParams>(
        n, [&](ColorParams& p, size_t f0, int m) { pack_color(p, c.in.data(), c.wh.data(), c.pitch.data(), c.cq.data(), c.out.data(), c.out_pitch.data(), f0, m); },
        [&](const ColorParams& p, size_t f0, int m) {
            for (int i = 0; i < COLOR_BATCH; i++) {
                const size_t f = f0 + i;
                SLOT(in[i], at(IN, f)); SLOT(out[i], at(OUT, f)); SLOT(wh[i], W(f) | H(f) << 16);
                SLOT(in_pitch[i], pitch_of(f, 3)); SLOT(out_pitch[i], pitch_of(f, 3) + 16);
                for (int k = 0; k < 12; k++) SLOT(q[i][k], (int32_t)(1000 * f + k) - 7);
            }
        });
}

static void planes(size_t n)
{
    const Call c(n);
    // the library's three arrays, and the emulation's one array of three per image
    std::vector<const uint8_t*> three;
    for (size_t f = 0; f < n; f++) { three.push_back(c.in[f]); three.push_back(c.in2[f]); three.push_back(c.in3[f]); }
    const uint8_t* const* const apart[3] = {c.in.data(), c.in2.data(), c.in3.data()};
    const uint8_t* const* const together[3] = {three.data(), three.data() + 1, three.data() + 2};
    for (int step : {1, 3})
        launches<PLANES_BATCH, PlanesParams>(
            n, [&](PlanesParams& p, size_t f0, int m) { pack_planes(p, step == 1 ? apart : together, (size_t)step, c.pitch3.data(), c.wh.data(), c.geo.data(), c.out.data(), c.out_pitch.data(), f0, m); },
            [&](const PlanesParams& p, size_t f0, int m) {
                const uint64_t base[3] = {IN, IN2, IN3};
                for (int i = 0; i < PLANES_BATCH; i++) {
                    const size_t f = f0 + i;
                    for (unsigned k = 0; k < 3; k++) { SLOT(p[k][i], at(base[k], f)); SLOT(pitch[k][i], pitch_of(f, 1) + 100 * k); }
                    SLOT(out[i], at(OUT, f)); SLOT(out_pitch[i], pitch_of(f, 3) + 16); SLOT(wh[i], W(f) | H(f) << 16);
                    SLOT(geo[i], (uint32_t)(0x010203u * (f % 5) + f));
                }
            });
}

static void resize(size_t n)
{
    const Call c(n);
    // out_w, out_h, the groups of a row, the rows of a workgroup: ceil(out_w / 8), 1024 / groups within [1, out_h]
    static const int shape[4][4] = {{1, 224, 1, 224}, {8, 2000, 1, 1024}, {9, 600, 2, 512}, {224, 224, 28, 36}};
    for (const int* s : shape)
        for (size_t first : {(size_t)0, (size_t)7})
            for (const uint8_t* flip : {c.flags.data(), (const uint8_t*)nullptr}) {
                const StageTensor t = tensor(s[0], s[1], (size_t)3 * s[0] * s[1] * 2);
                launches<RESIZE_BATCH, ResizeParams>(
                    n, [&](ResizeParams& p, size_t f0, int m) { pack_resize(p, c.in.data(), c.wh.data(), c.pitch.data(), flip, t, first, f0, m); },
                    [&](const ResizeParams& p, size_t f0, int m) {
                        CHECK(p.out_w == s[0] && p.out_h == s[1] && p.groups == s[2] && p.rows == s[3]);
                        CHECK(p.out == TENSOR + (first + f0) * t.img_bytes);
                        for (int k = 0; k < 3; k++) CHECK(p.scale[k] == t.s[k] && p.bias[k] == t.b[k]);
                        for (int i = 0; i < RESIZE_BATCH; i++) {
                            const size_t f = f0 + i;
                            SLOT(in[i], at(IN, f)); SLOT(wh[i], W(f) | H(f) << 16); SLOT(pitch[i], pitch_of(f, 3));
                            CHECK(bit(p.flip, i) == (i < m && flip && flag(f)));
                        }
                    });
            }
}

static void to_tensor(size_t n)
{
    const Call c(n);
    for (const uint8_t* flip : {c.flags.data(), (const uint8_t*)nullptr}) {
        const StageTensor t = tensor(33, 17, (size_t)3 * 33 * 17 * 2);
        launches<TT_BATCH, ToTensorParams>(
            n, [&](ToTensorParams& p, size_t f0, int m) { pack_to_tensor(p, c.in.data(), c.pitch.data(), flip, 1, 3, t, f0, m); },
            [&](const ToTensorParams& p, size_t f0, int m) {
                CHECK(p.w == 33 && p.h == 17 && p.cin == 1 && p.cout == 3 && p.dtype == RZ_F16 && p.nhwc == 1);
                CHECK(p.out == TENSOR + f0 * t.img_bytes);
                for (int k = 0; k < 3; k++) CHECK(p.scale[k] == t.s[k] && p.bias[k] == t.b[k]);
                for (int i = 0; i < TT_BATCH; i++) {
                    const size_t f = f0 + i;
                    SLOT(in[i], at(IN, f)); SLOT(pitch[i], pitch_of(f, 3));
                    CHECK(bit(p.flip, i) == (i < m && flip && flag(f)));
                }
            });
    }
}

static void warp(size_t n)
{
    Call c(n);
    for (size_t f = 0; f < n; f++)
        if (f % 5 == 2) c.wh[2 * f] = 0; // an empty window: no image at all
    const StageTensor t = tensor(40, 30, (size_t)3 * 40 * 30 * 2);
    for (size_t first : {(size_t)0, (size_t)7})
        launches<WARP_BATCH, WarpParams>(
            n, [&](WarpParams& p, size_t f0, int m) { pack_warp(p, c.in.data(), c.wh.data(), c.pitch.data(), c.wq.data(), 0x030201u, 1, t, first, f0, m); },
            [&](const WarpParams& p, size_t f0, int m) {
                CHECK(p.out_w == 40 && p.out_h == 30 && p.dtype == RZ_F16 && p.nhwc == 1 && p.fill == 0x030201u && p.edge == 1);
                CHECK(p.out == TENSOR + (first + f0) * t.img_bytes);
                for (int k = 0; k < 3; k++) CHECK(p.scale[k] == t.s[k] && p.bias[k] == t.b[k]);
                for (int i = 0; i < WARP_BATCH; i++) {
                    const size_t f = f0 + i;
                    const WarpImage& im = p.img[i];
                    const bool empty = i < m && f % 5 == 2;
                    CHECK(im.in == (i >= m ? 0 : empty ? TENSOR : at(IN, f)));
                    CHECK(im.wh == (i >= m ? 0 : empty ? (1u | 1u << 16) : (W(f) | H(f) << 16)));
                    CHECK(im.pitch == (i >= m ? 0 : empty ? 1 : pitch_of(f, 3)));
                    for (int k = 0; k < 6; k++)
                        CHECK(im.m[k] == (i >= m ? 0 : empty ? (k % 3 == 2 ? -((int64_t)4 << 24) : 0) : ((int64_t)f << 33) + k - 3));
                }
            });
}

// the size / pointer / pitch rule and the other argument rules: each refusal of the GPU tests' lists, next to a good neighbour
static void rules()
{
    const uint8_t* const a = (const uint8_t*)(uintptr_t)IN;
    std::vector<unsigned> r;
    const uint8_t* one[1] = {a};
    const uint8_t* two[2] = {a, a};
    const uint8_t* hole[2] = {a, nullptr};
    const unsigned w44[4] = {4, 4, 4, 4}, empty_w[4] = {4, 4, 0, 4}, empty_h[4] = {4, 4, 4, 0}, wide[2] = {65536, 1}, tall[2] = {1, 65536},
                   widest[2] = {65535, 65535};
    // sizes: 1..65535 each way, an empty image behind a good one
    CHECK(stage_images(2, two, w44, nullptr, 3, r) && r[0] == 12 && r[1] == 12);
    CHECK(!stage_images(2, two, empty_w, nullptr, 3, r) && !stage_images(2, two, empty_h, nullptr, 3, r));
    CHECK(!stage_images(1, one, wide, nullptr, 3, r) && !stage_images(1, one, tall, nullptr, 3, r));
    CHECK(stage_images(1, one, widest, nullptr, 3, r) && r[0] == 3 * 65535);
    CHECK(!stage_size(0, 1) && !stage_size(1, 0) && stage_size(1, 1) && stage_size(65535, 65535) && !stage_size(65536, 65535));
    // NULL behind a good image, on the side that reads and the side that writes
    CHECK(!stage_images(2, hole, w44, nullptr, 3, r) && !stage_side(2, hole, nullptr, w44, 3, r) && stage_side(2, two, nullptr, w44, 3, r));
    // pitches: nullptr or 0 is tight, from a row up to 2^24 (g_pitch_max: what the far-offset tests take the limit to be)
    const unsigned p11[1] = {11}, p12[1] = {12}, p0[1] = {0}, p3[1] = {3}, p4[1] = {4}, top[1] = {g_pitch_max}, over[1] = {g_pitch_max + 1};
    CHECK(!stage_images(1, one, w44, p11, 3, r) && stage_images(1, one, w44, p12, 3, r) && r[0] == 12);
    CHECK(stage_images(1, one, w44, p0, 3, r) && r[0] == 12);
    CHECK(!stage_side(1, one, p11, w44, 3, r) && stage_side(1, one, p12, w44, 3, r));
    CHECK(!stage_side(1, one, p3, w44, 1, r) && stage_side(1, one, p4, w44, 1, r) && r[0] == 4); // (planes: a row is w bytes)
    CHECK(g_pitch_max == 1u << 24 && stage_side(1, one, top, w44, 3, r) && r[0] == g_pitch_max && !stage_side(1, one, over, w44, 3, r));
    const unsigned second[2] = {0, 11};
    CHECK(!stage_images(2, two, w44, second, 3, r)); // (behind a good image)
    // orient: the output's rows are the displayed width -- a 4 x 9 image turned on its side shows rows of 9
    const unsigned w49[2] = {4, 9}, p26[1] = {26}, p27[1] = {27};
    const auto shown = [&](size_t) { return (size_t)w49[1] * 3; };
    CHECK(!stage_side(1, one, p26, shown, r) && stage_side(1, one, p27, shown, r) && stage_side(1, one, nullptr, shown, r) && r[0] == 27);
    // to-tensor: one w, h for every image
    const auto row = [](size_t) { return (size_t)5 * 3; };
    const unsigned p14_15[2] = {15, 14};
    CHECK(stage_side(2, two, nullptr, row, r) && r[1] == 15 && !stage_side(2, two, p14_15, row, r) && !stage_side(2, hole, nullptr, row, r));

    // the planes call: ratios of 1, 2, 4, phases below them, the samples of a row, the component's byte
    unsigned pw;
    uint32_t g;
    for (unsigned bad : {3u, 8u, 0u, 5u})
        CHECK(!planes_component(4, bad, 1, 0, 0, pw, g) && !planes_component(4, 1, bad, 0, 0, pw, g));
    for (unsigned rx : {1u, 2u, 4u})
        for (unsigned ry : {1u, 2u, 4u})
            for (unsigned px = 0; px <= rx; px++)
                for (unsigned py = 0; py <= ry; py++) {
                    const bool ok = planes_component(8, rx, ry, px, py, pw, g);
                    CHECK(ok == (px < rx && py < ry));
                    if (ok) CHECK(pw == (px + 8 + rx - 1) / rx && g == ((rx >> 1) | (ry >> 1) << 2 | px << 4 | py << 6) && g < 256);
                }
    CHECK(planes_component(8, 4, 1, 0, 0, pw, g) && pw == 2); // (a pitch of 1 is below ceil(8 / 4) ...)
    const unsigned p1[1] = {1}, p2[1] = {2};
    unsigned res;
    CHECK(!stage_pitch(p1, 0, pw, res) && stage_pitch(p2, 0, pw, res) && res == 2 && stage_pitch(nullptr, 0, pw, res) && res == 2);
    CHECK(planes_component(4, 4, 4, 0, 0, pw, g) && pw == 1 && planes_component(8, 4, 1, 3, 0, pw, g) && pw == 3);

    // the tensor factors: s_c = scale_c * 2^-16, nullptr: 1 and 0, read for the first `channels` only, finite
    float s[3], b[3];
    const float sc[3] = {2.f, -0.5f, NAN}, bi[3] = {1.f, -1.f, INFINITY};
    CHECK(kernel_factors(nullptr, nullptr, 3, s, b) && s[0] == 1.f / 65536.f && s[2] == 1.f / 65536.f && b[1] == 0.f);
    CHECK(kernel_factors(sc, bi, 2, s, b) && s[0] == 2.f / 65536.f && s[1] == -0.5f / 65536.f && s[2] == 1.f / 65536.f && b[0] == 1.f &&
          b[1] == -1.f && b[2] == 0.f);
    CHECK(!kernel_factors(sc, nullptr, 3, s, b) && !kernel_factors(nullptr, bi, 3, s, b));

    // the warp's fill
    const uint8_t fill[3] = {1, 2, 3};
    CHECK(warp_fill(fill, 3) == 0x030201u && warp_fill(fill, 1) == 1u && warp_fill(nullptr, 3) == 0);
}

int main(int argc, char** argv)
{
    if (argc > 1) g_pitch_max = (unsigned)strtoul(argv[1], nullptr, 10);
    sizes<ORIENT_BATCH>(orient);
    sizes<EXPAND_BATCH>(expand);
    sizes<CMYK_BATCH>(cmyk);
    sizes<COLOR_BATCH>(color);
    sizes<PLANES_BATCH>(planes);
    sizes<RESIZE_BATCH>(resize);
    sizes<TT_BATCH>(to_tensor);
    sizes<WARP_BATCH>(warp);
    rules();
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("stage-pack-clean\n");
    return 0;
}

// zj_resize.h -- resize + normalise of u8 images into a dense tensor (zj_resize_device).
//
// The definition's arithmetic as ZJ_HD functions, shared by the kernel (zj_resize.hip) and its CPU emulation
// (tests/emu_resize, a g++ ZJ_EMU build), and the launch's arguments:
//   resize_tap    one axis: destination index -> source index, weight in 1/256, step to the second tap
//   resize_value  the bilinear value of one channel, in 1/65536 units, integer only
//   resize_*      the output conversions (float32 two separately rounded operations; f16 / bf16 nearest-even; u8)
//   resize_group  one lane's work: GROUP consecutive output pixels of one output row, every channel, stored
#pragma once
#include <stdint.h>
#include <string.h>

#include "zj_geom.h" // RESIZE_MAX_OUT, resize_elem_bytes: the output's size rules, shared with the front-end

#if defined(ZJ_EMU)
#ifndef ZJ_DEV
#define ZJ_DEV inline
#define ZJ_HD inline
#endif
#define ZJ_RZ_GLOBAL(T, v) (reinterpret_cast<T*>(v))
#else
#include <hip/hip_runtime.h>
#ifndef ZJ_DEV
#define ZJ_DEV __device__ __forceinline__
#define ZJ_HD __host__ __device__ __forceinline__
#endif
#define ZJ_RZ_GLOBAL(T, v) ((T*)(__attribute__((address_space(1))) T*)(v))
#endif

namespace zj {

constexpr int RESIZE_BATCH = 128;     // images per launch (their pointers, sizes and pitches are kernel arguments)
constexpr int RESIZE_GROUP = 8;       // output pixels of one row per lane
constexpr int RESIZE_ITEMS = 1024;    // (row, group) items per workgroup, about
constexpr int RESIZE_NT = 256;        // threads per workgroup
enum { RZ_F32 = ZJ_DTYPE_F32, RZ_F16 = ZJ_DTYPE_F16, RZ_BF16 = ZJ_DTYPE_BF16, RZ_U8 = ZJ_DTYPE_U8 };

// One axis, destination index i of m, source length n (1..65535, m 1..8192):
//   u = floor((2i + 1) * n * 256 / (2m)) - 128, clamped to [0, (n - 1) * 256]; i0 = u >> 8, f = u & 255,
//   i1 = min(i0 + 1, n - 1).
// The 64-bit quotient floor((2i + 1) n 128 / m) is exact in 32-bit integers: a = (2i + 1) n < 2^30 = qa m + ra, and
// floor(a 128 / m) = 128 qa + floor(128 ra / m) with 128 ra < 2^20.  Packed: i0 | f << 16 | (i1 - i0) << 24.
ZJ_HD uint32_t resize_tap(const uint32_t i, const uint32_t n, const uint32_t m)
{
    const uint32_t a = (2u * i + 1u) * n;
    const uint32_t qa = a / m, ra = a - qa * m;
    int u = (int)(qa * 128u + (ra * 128u) / m) - 128;
    const int hi = (int)(n - 1u) * 256;
    u = u < 0 ? 0 : (u > hi ? hi : u);
    const uint32_t i0 = (uint32_t)u >> 8, f = (uint32_t)u & 255u;
    const uint32_t step = i0 + 1u < n ? 1u : 0u;
    return i0 | (f << 16) | (step << 24);
}
ZJ_HD uint32_t tap_i0(const uint32_t t) { return t & 0xffffu; }
ZJ_HD uint32_t tap_f(const uint32_t t) { return (t >> 16) & 255u; }
ZJ_HD uint32_t tap_step(const uint32_t t) { return t >> 24; }

// top = p00 (256 - fx) + p01 fx, bot likewise, v = top (256 - fy) + bot fy: 0 <= v <= 255 * 65536 < 2^24
ZJ_HD uint32_t resize_value(const uint32_t p00, const uint32_t p01, const uint32_t p10, const uint32_t p11, const uint32_t fx,
                            const uint32_t fy)
{
    const uint32_t top = p00 * (256u - fx) + p01 * fx;
    const uint32_t bot = p10 * (256u - fx) + p11 * fx;
    return top * (256u - fy) + bot * fy;
}

// float32: fl32(fl32(fl32(v) * s) + b), two separately rounded operations (s = scale * 2^-16, formed on the host)
ZJ_HD float resize_f32(const uint32_t v, const float s, const float b)
{
#if defined(ZJ_EMU)
    volatile float t = (float)v * s; // (the emulation is built with -ffp-contract=off as well)
    return t + b;
#else
#pragma clang fp contract(off) // (hipcc contracts __fmul_rn + __fadd_rn into v_fma_f32 otherwise)
    const float t = (float)v * s;
    return t + b;
#endif
}

ZJ_HD uint32_t f32_bits(const float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// float32 -> bfloat16, nearest-even (y is never NaN: v, s and b are finite, so y is finite or +-inf)
ZJ_HD uint32_t resize_bf16_bits(const float y)
{
    const uint32_t u = f32_bits(y);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// float32 -> float16, nearest-even, overflow to inf (the emulation's; the kernel converts with v_cvt_pk_f16_f32, resize_pack2)
ZJ_HD uint32_t resize_f16_bits(const float y)
{
    const uint32_t u = f32_bits(y);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const uint32_t a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0u);
    if (a >= 0x477ff000u) return sign | 0x7c00u;  // >= 65520: rounds to inf
    if (a < 0x38800000u) {                        // below 2^-14: a subnormal half (or zero)
        if (a < 0x33000000u) return sign;          // below 2^-25: zero (2^-25 itself ties to even: zero)
        const uint32_t e = a >> 23, mant = (a & 0x7fffffu) | 0x800000u;
        const uint32_t shift = 126u - e;           // mant * 2^(e - 150) in units of 2^-24
        const uint32_t q = mant >> shift, rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        return sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
    }
    const uint32_t r = a + 0xfffu + ((a >> 13) & 1u) - 0x38000000u;
    return sign | (r >> 13);
}

ZJ_HD uint32_t resize_u8(const uint32_t v) { return (v + 32768u) >> 16; }

// One launch: up to RESIZE_BATCH images of their own sizes and pitches to one out_w x out_h, into a dense tensor.
struct ResizeParams {
    uint64_t in[RESIZE_BATCH];        // per image: first byte (CHW: of plane 0)
    uint32_t wh[RESIZE_BATCH];        // per image: w | h << 16 (1..65535 each)
    uint32_t pitch[RESIZE_BATCH];     // per image: bytes between rows (CHW: planes lie pitch x h apart)
    uint32_t flip[RESIZE_BATCH / 32]; // per image: a bit, horizontal flip
    uint64_t out;                     // the launch's first image
    float scale[3], bias[3];          // per channel: s_c = scale_c * 2^-16, bias_c
    int out_w, out_h, nimg;
    int rows;                         // output rows per workgroup
    int groups;                       // RESIZE_GROUP-pixel groups per output row
};

// The element (channel c, output row r, column x) of an image, counted from the image's first
template <int C, bool NHWC>
ZJ_HD long long resize_elem(const int c, const int r, const int x, const int ow, const int oh)
{
    return NHWC ? ((long long)r * ow + x) * C + c : ((long long)c * oh + r) * ow + x;
}

// the NB bytes of w to dst, or its first nb < NB bytes: the widest stores the address and the length allow (16, 8, 4 bytes),
// else one element at a time (the indices are compile-time constants: w stays in registers)
template <int E, int NB>
ZJ_HD void resize_store(uint8_t* dst, const uint32_t (&w)[(NB + 3) / 4], const int nb)
{
#if defined(ZJ_EMU)
    memcpy(dst, w, (size_t)nb);
#else
    const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
    if (nb == NB && NB % 16 == 0 && (a & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < NB / 16; k++) {
            const uint4 v = {w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
            *reinterpret_cast<uint4*>(dst + 16 * k) = v;
        }
    } else if (nb == NB && NB % 8 == 0 && (a & 7u) == 0) {
#pragma unroll
        for (int k = 0; k < NB / 8; k++) *reinterpret_cast<uint2*>(dst + 8 * k) = uint2{w[2 * k], w[2 * k + 1]};
    } else if (nb == NB && NB % 4 == 0 && (a & 3u) == 0) {
#pragma unroll
        for (int k = 0; k < NB / 4; k++) reinterpret_cast<uint32_t*>(dst)[k] = w[k];
    } else {
#pragma unroll
        for (int k = 0; k < NB; k += E) {
            if (k >= nb) continue;
            const uint32_t x = w[k / 4] >> (8 * (k % 4));
            if (E == 1) dst[k] = (uint8_t)x;
            else if (E == 2) *reinterpret_cast<uint16_t*>(dst + k) = (uint16_t)x;
            else *reinterpret_cast<uint32_t*>(dst + k) = x;
        }
    }
#endif
}

// the converted elements k and k + 1 of a lane's run, packed into one dword (E == 2: two halves; E == 4: k alone; E == 1:
// the caller packs four)
template <int DT>
ZJ_HD uint32_t resize_pack2(const float a, const float b)
{
#if defined(ZJ_EMU)
    if (DT == RZ_BF16) return resize_bf16_bits(a) | resize_bf16_bits(b) << 16;
    return resize_f16_bits(a) | resize_f16_bits(b) << 16;
#else
    if (DT == RZ_BF16) {
        typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
        typedef float f2 __attribute__((ext_vector_type(2)));
        const bf2 r = __builtin_convertvector((f2){a, b}, bf2); // v_cvt_pk_bf16_f32, nearest-even
        return __builtin_bit_cast(uint32_t, r);
    }
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    // v_cvt_pk_f16_f32: nearest-even, subnormal results kept (v_cvt_f16_f32 where one of the two is a constant)
    const h2 r = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(uint32_t, r);
#endif
}

// One lane's work: output pixels [x0, x0 + GROUP) of output row r (the columns past out_w are not written), every channel.
// ctap: the column taps of the image (flip applied: entry x is the tap of destination column m - 1 - x), ty: the row's tap.
// src: the image's first byte, in its own layout (HWC: channel c of pixel x at x * C + c; CHW: plane c at c * pitch * h).
template <bool IN_CHW, int C, int DT, bool NHWC>
ZJ_HD void resize_group(const ResizeParams& p, const uint8_t* src, const int pitch, const int h, const uint32_t* ctap,
                        const uint32_t ty, const int r, const int x0, uint8_t* img_out)
{
    constexpr int G = RESIZE_GROUP, E = resize_elem_bytes(DT);
    const int ow = p.out_w, oh = p.out_h;
    const int cnt = ow - x0 < G ? ow - x0 : G;
    const uint32_t y0 = tap_i0(ty), fy = tap_f(ty);
    const uint8_t* const row0 = src + (long long)y0 * pitch;
    const uint8_t* const row1 = row0 + (long long)tap_step(ty) * pitch;
    const long long plane = IN_CHW ? (long long)pitch * h : 0;
    uint32_t t[G];
#pragma unroll
    for (int k = 0; k < G; k++) t[k] = ctap[k < cnt ? k : 0];
    // the runs of contiguous output elements: NHWC one run of cnt * C, NCHW one run of cnt per channel (converted and
    // stored channel by channel: fewer live registers)
    constexpr int RUNS = NHWC ? 1 : C, RUN = NHWC ? G * C : G, NB = RUN * E;
#pragma unroll
    for (int q = 0; q < RUNS; q++) {
        uint32_t v[RUN];
#pragma unroll
        for (int j = 0; j < RUN; j++) {
            const int k = NHWC ? j / C : j, c = NHWC ? j % C : q;
            const uint32_t xa = tap_i0(t[k]), xb = xa + tap_step(t[k]);
            const long long o0 = IN_CHW ? c * plane + xa : (long long)xa * C + c;
            const long long o1 = IN_CHW ? c * plane + xb : (long long)xb * C + c;
            v[j] = resize_value(row0[o0], row0[o1], row1[o0], row1[o1], tap_f(t[k]), fy);
        }
        uint32_t w[(NB + 3) / 4];
#pragma unroll
        for (int wi = 0; wi < (NB + 3) / 4; wi++) {
            if (DT == RZ_F32) {
                const int c = NHWC ? wi % C : q;
                w[wi] = f32_bits(resize_f32(v[wi], p.scale[c], p.bias[c]));
            } else if (DT == RZ_U8) {
                uint32_t d = 0;
#pragma unroll
                for (int b = 0; b < 4; b++)
                    if (4 * wi + b < RUN) d |= resize_u8(v[4 * wi + b]) << (8 * b);
                w[wi] = d;
            } else {
                const int j0 = 2 * wi, j1 = 2 * wi + 1;
                const int c0 = NHWC ? j0 % C : q, c1 = NHWC ? j1 % C : q;
                const float a = resize_f32(v[j0], p.scale[c0], p.bias[c0]);
                const float b = j1 < RUN ? resize_f32(v[j1], p.scale[c1], p.bias[c1]) : 0.f;
                w[wi] = resize_pack2<DT>(a, b);
            }
        }
        uint8_t* const dst = img_out + resize_elem<C, NHWC>(NHWC ? 0 : q, r, x0, ow, oh) * E;
        resize_store<E, NB>(dst, w, (NHWC ? cnt * C : cnt) * E);
    }
}

} // namespace zj

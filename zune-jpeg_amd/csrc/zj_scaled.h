// zj_scaled.h -- device-side code of the reduced-size decode: scale 1/2, 1/4, 1/8 (SL = 1, 2, 3).
//
// A block yields N = min(8, (8 >> SL) * f_max / f_c) samples per axis, each the mean of 8 / N consecutive outputs of the exact
// 8-point IDCT, taken before rounding.  tests/scaled_model.py is the definition, in float64 and in the integers computed here:
//   pass 1 (columns)  t = (sum_k s[k][col] K_Ny[m][k] + 512) >> 10                          s = coefficient x q
//   pass 2 (rows)     v = (sum_k t[m][k] K_Nx[n][k] + 32768 + (128 << 16)) >> 16, clamped to 0..255
//   N_x = N_y = 1     v = ((s[0][0] + 4) >> 3) + 128, clamped
// K_N[m][k] = round(2^13 C_k/2 mean_j cos((2 (8/N m + j) + 1) k pi / 16)); K_N[N-1-m][k] = (-1)^k K_N[m][k], so a pair of
// outputs shares its even and its odd sum.  Every multiplicand fits 24 bits (|s| < 2^23, |t| < 2^21): v_mad_i32_i24 gives
// the wrapping 32-bit sums of the model for EVERY input.  A component with N = 8 on both axes (chroma of 4:2:0 at 1/2) is
// not reduced: it takes the full path's block transforms (zj_device.h), Q1 and ZJ_FLAG_CLAMP_DC as they are.
//
// Like zj_device.h this header is compiled by hipcc into libzjhip.so and by g++ (ZJ_EMU) into tests/emu_scaled, which runs
// the phases of a workgroup thread by thread.
#pragma once

#include "zj_device.h"

namespace zj {

// K_N[m][k] for m < max(N / 2, 1) (tests/scaled_model.py: int_matrix)
ZJ_HD constexpr int scaled_k(const int n, const int m, const int k)
{
    constexpr int K1[8] = {2896, 0, 0, 0, 0, 0, 0, 0};
    constexpr int K2[8] = {2896, 2624, 0, -922, 0, 616, 0, -522};
    constexpr int K4[2][8] = {{2896, 3711, 2676, 1303, 0, -871, -1108, -738}, {2896, 1537, -2676, -3146, 0, 2102, 1108, -306}};
    constexpr int K8[4][8] = {{2896, 4017, 3784, 3406, 2896, 2276, 1567, 799}, {2896, 3406, 1567, -799, -2896, -4017, -3784, -2276},
                              {2896, 2276, -1567, -4017, -2896, 799, 3784, 3406}, {2896, 799, -3784, -2276, 2896, 3406, -1567, -4017}};
    return n == 1 ? K1[k] : (n == 2 ? K2[k] : (n == 4 ? K4[m][k] : K8[m][k]));
}
// bit k: coefficient row (column) k has a non-zero entry in K_N -- the rows of a block a transform of N outputs reads
ZJ_HD constexpr unsigned scaled_need(const int n) { return n == 1 ? 0x01u : (n == 2 ? 0xabu : (n == 4 ? 0xefu : 0xffu)); }

// one axis: N outputs of 8 inputs (each within 24 bits), o[m] = sum_k s[k] K_N[m][k] + bias, wrapping
template <int N>
ZJ_DEV void scaled_1d(const int32_t s[8], const int32_t bias, int32_t o[N])
{
    constexpr int H = N > 1 ? N / 2 : 1;
#pragma unroll
    for (int m = 0; m < H; m++) {
        int32_t e = bias, d = 0;
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            const int c = scaled_k(N, m, k);
            if (c != 0) e = mad24(s[k], c, e);
        }
#pragma unroll
        for (int k = 1; k < 8; k += 2) {
            const int c = scaled_k(N, m, k);
            if (c != 0) d = mad24(s[k], c, d);
        }
        if (N == 1) o[0] = e;
        else { o[m] = wadd(e, d); o[N - 1 - m] = wsub(e, d); }
    }
}

ZJ_DEV int32_t scaled_clamp(const int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// raw[r] = coefficient row r (8 x i16, natural order; only the rows of scaled_need(NY) are read), qt = the component's 64
// table entries.  out[m * NX + n] = sample (row m, column n), 0..255.
template <int NX, int NY>
ZJ_DEV void scaled_block(const U4 raw[8], const uint16_t* qt, int32_t out[NX * NY])
{
    const uint32_t* w = reinterpret_cast<const uint32_t*>(raw);
    if (NX == 1 && NY == 1) {
        const int32_t s = mul24(lo16s(w[0]), (int32_t)qt[0]);
        out[0] = scaled_clamp(((s + 4) >> 3) + 128);
        return;
    }
    int32_t tmp[NY][8];
#pragma unroll
    for (int col = 0; col < 8; col++) {
        if (!((scaled_need(NX) >> col) & 1u)) continue; // pass 2 never reads this column
        int32_t s[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (!((scaled_need(NY) >> k) & 1u)) { s[k] = 0; continue; }
            const uint32_t pair = w[k * 4 + (col >> 1)];
            const int32_t cf = (col & 1) ? hi16s(pair) : lo16s(pair);
            s[k] = mul24(cf, (int32_t)qt[k * 8 + col]); // dequantise; q is 0..255
        }
        int32_t o[NY];
        scaled_1d<NY>(s, 512, o);
#pragma unroll
        for (int m = 0; m < NY; m++) tmp[m][col] = o[m] >> 10;
    }
#pragma unroll
    for (int m = 0; m < NY; m++) {
#pragma unroll
        for (int col = 0; col < 8; col++)
            if (!((scaled_need(NX) >> col) & 1u)) tmp[m][col] = 0;
        int32_t o[NX];
        scaled_1d<NX>(tmp[m], 32768 + (128 << 16), o);
#pragma unroll
        for (int n = 0; n < NX; n++) out[m * NX + n] = scaled_clamp(o[n] >> 16);
    }
}

// ------------------------------------------------------------------------------------------------
// Tile geometry.  A workgroup owns TM MCUs of one MCU row: one lane per block -- the luma blocks first, then Cb, then Cr, so
// that a wave holds one kind of transform wherever the counts allow.  Every component lands on the reduced grid (an MCU is
// MW x MH pixels for all of them): no up-sampling, no halo, no strips.
//   LDS:  Y | Cb | Cr sample planes [MH][TW] i16  |  the three tables  |  the tile's bytes as the output lays them out
// ------------------------------------------------------------------------------------------------
template <int HS, int VS, int OUT, int SL>
struct ScaledCfg {
    static_assert(SL >= 1 && SL <= 3, "1/2, 1/4, 1/8");
    static constexpr bool CHROMA = OUT != OUT_GRAY;
    static constexpr int LN = 8 >> SL;                 // luma samples per block and axis
    static constexpr int MW = LN * HS, MH = LN * VS;   // reduced pixels per MCU = chroma samples per block (<= 8)
    static constexpr bool C_FULL = MW == 8 && MH == 8; // chroma is the full transform
    static constexpr int YPM = HS * VS;                // luma blocks per MCU
    static constexpr int TM = CHROMA ? (YPM == 4 ? 32 : 64) : 256 / YPM; // MCUs per tile
    static constexpr int NYB = TM * YPM;
    static constexpr int NBLK = NYB + (CHROMA ? 2 * TM : 0);
    static constexpr int NT = (NBLK + 63) / 64 * 64;   // 192 (4:2:0, 4:4:4) or 256 threads
    static constexpr int TW = TM * MW;                 // pixels per tile row
    static constexpr int BPP = crop_bpp(OUT);
    static constexpr int NPL = OUT == OUT_RGB_CHW ? 3 : 1;
    static constexpr int PLANE = MH * TW * 2;          // bytes of a sample plane
    static constexpr int TAB_OFF = (CHROMA ? 3 : 1) * PLANE;
    static constexpr int STAGE_OFF = TAB_OFF + TAB_BYTES;
    static constexpr int SPITCH = TW * BPP;            // bytes per staged row
    static constexpr int LDS = STAGE_OFF + NPL * MH * SPITCH + 32; // (+ the dwords the copy-out's shifted reads look ahead)
    static constexpr int NPAIR = MH * TW / 2;          // pixel pairs of a tile
    static_assert(PLANE % 16 == 0 && SPITCH % 4 == 0 && (TW & (TW - 1)) == 0, "aligned planes, power-of-two rows");
};

// The launch's arguments.  Frames are independent allocations (Params::fptr's form): y | cb | cr | out.
struct ScaledParams {
    int mcu_x;                    // MCUs per row of the coefficient planes
    int rw, rh;                   // the reduced frame, pixels
    int ncols, nrows;             // grid: tiles / MCU rows per frame (the widest range over the launch's frames)
    int out_pitch;                // bytes between crop rows (CHW: of a plane); 0: each crop tight (w x bpp)
    int clamp_dc;                 // ZJ_FLAG_CLAMP_DC, for the components that take the full transform
    int nframes;
    uint32_t tab[3 * TAB_DW];     // build_table
    uint64_t fptr[SCATTER_MAX][4];
    uint32_t origin[SCATTER_MAX]; // per frame: the window in reduced pixels, x | y << 16
    uint32_t size[SCATTER_MAX];   // ... w | h << 16
    uint32_t first[SCATTER_MAX];  // ... its first MCU column | first MCU row << 16
};

// what one workgroup works on (all uniform); scaled_locate false: nothing
struct ScaledTile { int frame, mrow, mcol0, mcol1, x, y, w, h; };

template <class C>
ZJ_DEV bool scaled_locate(const ScaledParams& p, const int fz, const int by, const int bx, ScaledTile& t)
{
    const uint32_t o = p.origin[fz], wh = p.size[fz], f = p.first[fz];
    t.frame = fz;
    t.x = (int)(o & 0xffffu); t.y = (int)(o >> 16); t.w = (int)(wh & 0xffffu); t.h = (int)(wh >> 16);
    t.mrow = (int)(f >> 16) + by;
    t.mcol0 = (int)(f & 0xffffu) + bx * C::TM;
    if (t.mrow * C::MH >= t.y + t.h || t.mcol0 * C::MW >= t.x + t.w) return false;
    int m1 = (t.x + t.w + C::MW - 1) / C::MW; // the MCU columns the window ends in, the planes have, the tile holds
    if (m1 > p.mcu_x) m1 = p.mcu_x;
    if (m1 > t.mcol0 + C::TM) m1 = t.mcol0 + C::TM;
    t.mcol1 = m1;
    return true;
}

// lane b of a tile: its block's coefficients, its component, where its samples go in LDS
struct ScaledLoc { const U4* src; int16_t* dst; int comp; bool valid; };

template <class C, int HS, int VS>
ZJ_DEV ScaledLoc scaled_block_loc(const ScaledParams& p, const ScaledTile& t, const int b, char* lds)
{
    ScaledLoc L;
    L.valid = false; L.src = nullptr; L.dst = reinterpret_cast<int16_t*>(lds); L.comp = 0;
    if (b < C::NYB) {
        const int mcu = b / C::YPM, sub = b % C::YPM, sy = sub / HS, sx = sub % HS;
        if (t.mcol0 + mcu >= t.mcol1) return L;
        const long long blk = (long long)(t.mrow * VS + sy) * (p.mcu_x * HS) + (t.mcol0 + mcu) * HS + sx;
        L.src = reinterpret_cast<const U4*>(ZJ_GLOBAL_PTR(const int16_t, p.fptr[t.frame][0]) + blk * 64);
        L.dst = reinterpret_cast<int16_t*>(lds) + (sy * C::LN) * C::TW + (mcu * HS + sx) * C::LN;
        L.valid = true;
        return L;
    }
    if (!C::CHROMA || b >= C::NBLK) return L;
    const int cb_ = b - C::NYB, comp = cb_ < C::TM ? 1 : 2, mcu = comp == 1 ? cb_ : cb_ - C::TM;
    if (t.mcol0 + mcu >= t.mcol1) return L;
    const long long blk = (long long)t.mrow * p.mcu_x + t.mcol0 + mcu;
    const int16_t* plane = comp == 1 ? ZJ_GLOBAL_PTR(const int16_t, p.fptr[t.frame][1]) : ZJ_GLOBAL_PTR(const int16_t, p.fptr[t.frame][2]);
    L.src = reinterpret_cast<const U4*>(plane + blk * 64);
    L.dst = reinterpret_cast<int16_t*>(lds + comp * C::PLANE) + mcu * C::MW;
    L.comp = comp;
    L.valid = true;
    return L;
}

// the rows of its block a lane reads: those its transform needs (all the loads are issued before the table barrier)
template <class C>
ZJ_DEV void scaled_load(const ScaledLoc& L, U4 raw[8])
{
    const unsigned need = L.comp == 0 ? scaled_need(C::LN) : scaled_need(C::MH);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        raw[i] = U4{0, 0, 0, 0};
        if (!L.valid || !((need >> i) & 1u)) continue;
#if !defined(ZJ_EMU)
        if (ZJ_NT & 2) { const V4 v = __builtin_nontemporal_load(reinterpret_cast<const V4*>(L.src + i)); raw[i].x = v[0]; raw[i].y = v[1]; raw[i].z = v[2]; raw[i].w = v[3]; continue; }
#endif
        raw[i] = L.src[i];
    }
}

template <class C>
ZJ_DEV void scaled_setup(const ScaledParams& p, const int tid, char* lds)
{
    uint32_t* tab = reinterpret_cast<uint32_t*>(lds + C::TAB_OFF);
    for (int i = tid; i < 3 * TAB_DW; i += C::NT) tab[i] = p.tab[i];
}

template <int NX, int NY>
ZJ_DEV void scaled_emit(const U4 raw[8], const uint16_t* qt, int16_t* dst, const int pitch)
{
    int32_t v[NX * NY];
    scaled_block<NX, NY>(raw, qt, v);
#pragma unroll
    for (int m = 0; m < NY; m++) {
        if (NX == 1) dst[m * pitch] = (int16_t)v[m];
        else {
#pragma unroll
            for (int n = 0; n < NX; n += 2)
                *reinterpret_cast<uint32_t*>(dst + m * pitch + n) = ((uint32_t)v[m * NX + n] & 0xffffu) | ((uint32_t)v[m * NX + n + 1] << 16);
        }
    }
}

// phase 1: the lane's block -> its samples in LDS
template <class C, int HS, int VS>
ZJ_DEV void scaled_finish(const ScaledLoc& L, const U4 raw[8], char* lds, const int clamp_dc)
{
    if (!L.valid) return;
    const uint32_t* tab = reinterpret_cast<const uint32_t*>(lds + C::TAB_OFF) + TAB_DW * L.comp;
    const uint16_t* qt = reinterpret_cast<const uint16_t*>(tab);
    if (L.comp == 0) { scaled_emit<C::LN, C::LN>(raw, qt, L.dst, C::TW); return; }
    if (!C::C_FULL) { scaled_emit<C::MW, C::MH>(raw, qt, L.dst, C::TW); return; }
    // the full path's transforms (finish_block's three arms), rows of 8 i16
    const uint32_t* w = reinterpret_cast<const uint32_t*>(raw);
    const int cls = classify_block(w, tab + 32);
    U4 px[8];
    if (cls == 0) {
        const uint32_t v = dc_only_value(w[0], (int32_t)(tab[0] & 0xffffu), clamp_dc);
#pragma unroll
        for (int r = 0; r < 8; r++) px[r] = U4{v, v, v, v};
    } else if (cls == 1) {
        uint32_t b[16];
        idct_block_packed(raw, tab, b);
        bytes_to_rows(b, px);
    } else {
        ZJ_NO_IF_CONVERT();
        idct_block(raw, qt, px);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) *reinterpret_cast<U4*>(L.dst + r * C::TW) = px[r];
}

// phase 2: pixel pairs of the tile -> the staged bytes (the full path's per-pixel arithmetic: ycc_to_rgb_pair, Q7)
// Only the columns of the MCUs the tile loaded (t.mcol0 .. t.mcol1) are converted: a window narrower than a tile -- the
// usual case under a resize -- does not pay for the rest of the tile's width.
template <class C, int OUT>
ZJ_DEV void scaled_color(const ScaledTile& t, const int tid, char* lds)
{
    uint8_t* const stage = reinterpret_cast<uint8_t*>(lds + C::STAGE_OFF);
    const int npc = ((t.mcol1 - t.mcol0) * C::MW + 1) >> 1; // pixel pairs per row that hold a loaded column
    for (int i = tid; i < C::MH * npc; i += C::NT) {
        const int row = i / npc, pc = i - row * npc;
        const uint32_t y = *reinterpret_cast<const uint32_t*>(lds + (row * C::TW + 2 * pc) * 2);
        if (OUT == OUT_GRAY) {
            *reinterpret_cast<uint16_t*>(stage + row * C::SPITCH + 2 * pc) = (uint16_t)((y & 0xffu) | ((y >> 8) & 0xff00u));
            continue;
        }
        const uint32_t cb = *reinterpret_cast<const uint32_t*>(lds + C::PLANE + (row * C::TW + 2 * pc) * 2);
        const uint32_t cr = *reinterpret_cast<const uint32_t*>(lds + 2 * C::PLANE + (row * C::TW + 2 * pc) * 2);
        uint32_t a, b, c; // the pair's bytes per channel: px0 | px1 << 8
        if (OUT == OUT_YCBCR) {
            a = (y & 0xffu) | ((y >> 8) & 0xff00u); b = (cb & 0xffu) | ((cb >> 8) & 0xff00u); c = (cr & 0xffu) | ((cr >> 8) & 0xff00u);
        } else {
            const RGB2 v = ycc_to_rgb_pair(y, cb, cr);
            a = sat_pk_u8(v.r); b = sat_pk_u8(v.g); c = sat_pk_u8(v.b);
        }
        if (OUT == OUT_RGB_CHW) {
            uint8_t* const s = stage + row * C::SPITCH + 2 * pc;
            *reinterpret_cast<uint16_t*>(s) = (uint16_t)a;
            *reinterpret_cast<uint16_t*>(s + C::MH * C::SPITCH) = (uint16_t)b;
            *reinterpret_cast<uint16_t*>(s + 2 * C::MH * C::SPITCH) = (uint16_t)c;
        } else {
            uint16_t* const s = reinterpret_cast<uint16_t*>(stage + row * C::SPITCH + 6 * pc);
            s[0] = (uint16_t)((a & 0xffu) | ((b & 0xffu) << 8));
            s[1] = (uint16_t)((c & 0xffu) | ((a >> 8) << 8));
            s[2] = (uint16_t)((b >> 8) | ((c >> 8) << 8));
        }
    }
}

// phase 3: the window's part of the staged tile -> the crop.  One lane per 16 bytes of a crop row; a window row starts at
// any byte: dwords aligned in the DESTINATION, each assembled from two staged dwords, the bytes before the row segment's
// first dword boundary and after its last from one extra lane per segment (crop_copyout's scheme).
template <class C>
ZJ_DEV void scaled_copyout(const ScaledParams& p, const ScaledTile& t, const int tid, const char* lds)
{
    const uint8_t* const stage = reinterpret_cast<const uint8_t*>(lds + C::STAGE_OFF);
    uint8_t* const out = ZJ_GLOBAL_PTR(uint8_t, p.fptr[t.frame][3]);
    const int pitch = p.out_pitch ? p.out_pitch : t.w * C::BPP;
    const long long plane = (long long)pitch * t.h;
    const int row0 = t.mrow * C::MH, byte0 = t.mcol0 * C::MW * C::BPP;
    const int r0 = row0 > t.y ? row0 : t.y, r1 = row0 + C::MH < t.y + t.h ? row0 + C::MH : t.y + t.h;
    const int b0 = byte0 > t.x * C::BPP ? byte0 : t.x * C::BPP;
    const int b1 = byte0 + C::SPITCH < (t.x + t.w) * C::BPP ? byte0 + C::SPITCH : (t.x + t.w) * C::BPP;
    const int n = b1 - b0, nr = r1 - r0;
    if (n <= 0 || nr <= 0) return;
    const int sbase = (r0 - row0) * C::SPITCH + (b0 - byte0);
    const long long obase = (long long)(r0 - t.y) * pitch + (b0 - t.x * C::BPP);
    const int nq_max = ((n >> 2) + 3) >> 2, per = nq_max + 1, total = C::NPL * nr * per;
    for (int i = tid; i < total; i += C::NT) {
        const int seg = i / per, q = i - seg * per;
        const int pl = seg / nr, r = seg - pl * nr;
        const int so = pl * C::MH * C::SPITCH + sbase + r * C::SPITCH;
        uint8_t* const d = out + pl * plane + obase + (long long)r * pitch;
        int h = (int)((4u - ((unsigned)reinterpret_cast<uintptr_t>(d) & 3u)) & 3u);
        if (h > n) h = n;
        const int ndw = (n - h) >> 2;
        if (q == nq_max) {
            for (int b = 0; b < h; b++) d[b] = stage[so + b];
            for (int b = h + 4 * ndw; b < n; b++) d[b] = stage[so + b];
            continue;
        }
        const int j0 = 4 * q;
        if (j0 >= ndw) continue;
        const int sp = so + h + 4 * j0;
        const uint32_t* const a = reinterpret_cast<const uint32_t*>(stage + (sp & ~3));
        const uint32_t sh = (uint32_t)sp & 3u;
        uint32_t w[5];
#pragma unroll
        for (int k = 0; k < 5; k++) w[k] = a[k];
        const U4 v = {alignbyte(w[1], w[0], sh), alignbyte(w[2], w[1], sh), alignbyte(w[3], w[2], sh), alignbyte(w[4], w[3], sh)};
        uint8_t* const dq = d + h + 4 * j0;
        if (j0 + 4 <= ndw) store16(dq, v);
        else {
            const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
            for (int k = 0; k < ndw - j0; k++) *reinterpret_cast<uint32_t*>(dq + 4 * k) = vv[k];
        }
    }
}

} // namespace zj

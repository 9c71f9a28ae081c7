// zj_orient.h -- EXIF orientation of u8 images in device memory (zj_orient_device).
//
// The launch's arguments and the phases of one workgroup as ZJ_HD functions, shared by the kernel (zj_orient.hip) and its CPU
// emulation (tests/emu_orient, a g++ ZJ_EMU build that runs them thread by thread).  The rule itself -- which stored pixel a
// displayed one is -- is zj_geom.h's (orient_transposes, orient_turns_rows, orient_turns_cols).
//   OrientParams        one launch: up to ORIENT_BATCH images of their own sizes, pitches, orientations and destinations
//   orient_block        the workgroup's tile: ORIENT_T x ORIENT_T displayed pixels and the stored rectangle they come from
//   orient_load_phase   the rectangle's rows -> LDS, aligned dwords, lane-contiguous
//   orient_store_phase  the tile's displayed rows <- LDS, dwords aligned in the DESTINATION and lane-contiguous, the bytes
//                       before a row segment's first dword boundary and after its last singly from one extra lane per
//                       segment (crop_copyout's scheme, zj_device.h)
// Every orientation takes the same two phases: 1..4 read the LDS rows along their length (2 and 3 from the far end), 5..8
// read them across -- one byte per LDS row and displayed pixel -- which is what the row padding below is for.
#pragma once
#include "zj_resize.h" // ZJ_HD, ZJ_RZ_GLOBAL; zj_geom.h

namespace zj {

constexpr int ORIENT_T = 64;       // tile side in pixels: 192-byte row segments on both sides of an RGB transpose
constexpr int ORIENT_NT = 256;     // threads per workgroup
constexpr int ORIENT_BATCH = 128;  // images per launch (29 bytes of kernel arguments each)

struct OrientParams {
    uint64_t in[ORIENT_BATCH], out[ORIENT_BATCH];
    uint32_t wh[ORIENT_BATCH];                                // STORED w | h << 16
    uint32_t in_pitch[ORIENT_BATCH], out_pitch[ORIENT_BATCH]; // bytes between rows (CHW: of a plane's rows)
    uint8_t o[ORIENT_BATCH];                                  // 1..8
    int nimg;
};
static_assert(sizeof(OrientParams) <= 4096, "kernel arguments: 4 KB");

// LDS tile.  A stored row segment of up to T x BPP bytes is loaded as the aligned dwords that hold it: up to 3 bytes of skew
// in front, so ORIENT_RDW dwords: 49 (BPP 3), 17 (BPP 1).  That is the row stride, and it is odd on purpose: the transposing
// orientations read one byte per lane from consecutive LDS rows (BPP 3: a lane's 4 bytes come from 2 pixels, consecutive lanes
// are 4/3 rows apart), banks = dword index mod 32, so 32 consecutive rows fall on 32 banks.  BPP 1: a lane's 4 bytes are 4
// rows, consecutive lanes are 4 rows = 68 dwords = 4 banks apart, so the 16 lanes of a displayed row segment share 8 banks
// two by two -- one more dword after every 4 rows makes it 69 dwords = 5 banks: 16 lanes, 16 banks; the half-wave's second
// segment reads the neighbouring bytes, mostly of the same dwords.
template <int BPP> ZJ_HD constexpr int orient_rdw() { return (ORIENT_T * BPP + 3 + 3) / 4; }
template <int BPP> ZJ_HD constexpr int orient_lds_row(const int lr) { return lr * orient_rdw<BPP>() * 4 + (BPP == 1 ? (lr >> 2) * 4 : 0); }
template <int BPP> ZJ_HD constexpr int orient_lds_bytes() { return orient_lds_row<BPP>(ORIENT_T); } // 12544 (BPP 3), 4416 (BPP 1)

struct OrientBlock {
    uint64_t src, dst;            // first byte of the stored rectangle's first row / of the tile's first displayed row
    uint32_t in_pitch, out_pitch;
    int o;
    int th, tw;                   // the tile: displayed rows, displayed pixels per row (0: nothing of this image here)
    int na, nb;                   // the stored rectangle: rows, pixels per row
};

// tile (bx, by) of plane `plane` (HWC: 0) of image img; BPP: bytes per pixel of a row (CHW: 1)
template <int BPP>
ZJ_HD OrientBlock orient_block(const OrientParams& p, const int img, const int plane, const int bx, const int by)
{
    OrientBlock b;
    const int w = (int)(p.wh[img] & 0xffffu), h = (int)(p.wh[img] >> 16);
    b.o = p.o[img];
    const bool t = orient_transposes(b.o);
    const int dw = t ? h : w, dh = t ? w : h;
    const int r0 = by * ORIENT_T, c0 = bx * ORIENT_T;
    b.th = b.tw = b.na = b.nb = 0;
    b.in_pitch = p.in_pitch[img]; b.out_pitch = p.out_pitch[img];
    b.src = b.dst = 0;
    if (r0 >= dh || c0 >= dw) return b;
    b.th = dh - r0 < ORIENT_T ? dh - r0 : ORIENT_T;
    b.tw = dw - c0 < ORIENT_T ? dw - c0 : ORIENT_T;
    const int a0 = t ? c0 : r0, b0 = t ? r0 : c0;
    b.na = t ? b.tw : b.th; b.nb = t ? b.th : b.tw;
    const int sr = orient_turns_rows(b.o) ? h - a0 - b.na : a0, sc = orient_turns_cols(b.o) ? w - b0 - b.nb : b0;
    b.src = p.in[img] + (uint64_t)plane * b.in_pitch * (uint64_t)h + (uint64_t)sr * b.in_pitch + (uint64_t)(sc * BPP);
    b.dst = p.out[img] + (uint64_t)plane * b.out_pitch * (uint64_t)dh + (uint64_t)r0 * b.out_pitch + (uint64_t)(c0 * BPP);
    return b;
}

// The stored rectangle's rows into LDS: row lr as the aligned dwords from (its first byte's address & ~3) on, so the bytes of
// a dword that lie outside the row are read with it -- they share its aligned dword, hence its page -- and never used.
template <int BPP>
ZJ_HD void orient_load_phase(const OrientBlock& b, uint32_t* lds, const int tid)
{
    constexpr int RDW = orient_rdw<BPP>();
    const int n = b.nb * BPP;
    for (int i = tid; i < b.na * RDW; i += ORIENT_NT) {
        const int lr = i / RDW, q = i - lr * RDW;
        const uint64_t s = b.src + (uint64_t)lr * b.in_pitch;
        const int skew = (int)(s & 3u);
        if (4 * q < skew + n) lds[orient_lds_row<BPP>(lr) / 4 + q] = *ZJ_RZ_GLOBAL(const uint32_t, s - (uint64_t)skew + (uint64_t)(4 * q));
    }
}

// byte `byte` of the tile's displayed row dr, from LDS
template <int BPP>
ZJ_HD uint32_t orient_byte(const OrientBlock& b, const uint8_t* lds, const int dr, const int byte)
{
    const int dc = byte / BPP, ch = byte - dc * BPP;
    const bool t = orient_transposes(b.o);
    const int al = t ? dc : dr, bl = t ? dr : dc;
    const int lr = orient_turns_rows(b.o) ? b.na - 1 - al : al, lc = orient_turns_cols(b.o) ? b.nb - 1 - bl : bl;
    const int skew = (int)(((uint32_t)b.src + (uint32_t)lr * b.in_pitch) & 3u);
    return lds[orient_lds_row<BPP>(lr) + skew + lc * BPP + ch];
}

// a store of the kernel (the emulation counts them in its write map here)
#if !defined(ZJ_ORIENT_PUT)
#define ZJ_ORIENT_PUT(T, addr, v) (*ZJ_RZ_GLOBAL(T, addr) = (v))
#endif

// The tile's displayed rows out of LDS.  A row segment of n = tw x BPP bytes starts at any byte: head = the bytes up to the
// destination's first dword boundary, then ndw aligned dwords, one per lane, then the tail; head and tail go out singly from
// the segment's extra lane.  (The head differs from row to row unless the pitch is a multiple of 4.)
template <int BPP>
ZJ_HD void orient_store_phase(const OrientBlock& b, const uint8_t* lds, const int tid)
{
    constexpr int PER = ORIENT_T * BPP / 4 + 1; // the dwords of a segment at most, + the lane of the single bytes
    const int n = b.tw * BPP;
    for (int i = tid; i < b.th * PER; i += ORIENT_NT) {
        const int dr = i / PER, q = i - dr * PER;
        const uint64_t d = b.dst + (uint64_t)dr * b.out_pitch;
        int h = (int)((4u - ((uint32_t)d & 3u)) & 3u);
        if (h > n) h = n;
        const int ndw = (n - h) >> 2;
        if (q == PER - 1) {
            for (int k = 0; k < h; k++) ZJ_ORIENT_PUT(uint8_t, d + (uint64_t)k, (uint8_t)orient_byte<BPP>(b, lds, dr, k));
            for (int k = h + 4 * ndw; k < n; k++) ZJ_ORIENT_PUT(uint8_t, d + (uint64_t)k, (uint8_t)orient_byte<BPP>(b, lds, dr, k));
            continue;
        }
        if (q >= ndw) continue;
        const int k0 = h + 4 * q;
        const uint32_t v = orient_byte<BPP>(b, lds, dr, k0) | (orient_byte<BPP>(b, lds, dr, k0 + 1) << 8) |
                           (orient_byte<BPP>(b, lds, dr, k0 + 2) << 16) | (orient_byte<BPP>(b, lds, dr, k0 + 3) << 24);
        ZJ_ORIENT_PUT(uint32_t, d + (uint64_t)k0, v);
    }
}

// the launch's grid: the tiles of the widest and of the tallest displayed image, the images (x planes)
ZJ_HD void orient_grid(const OrientParams& p, int* gx, int* gy)
{
    int mx = 1, my = 1;
    for (int i = 0; i < p.nimg; i++) {
        const int w = (int)(p.wh[i] & 0xffffu), h = (int)(p.wh[i] >> 16);
        const bool t = orient_transposes(p.o[i]);
        const int tx = ((t ? h : w) + ORIENT_T - 1) / ORIENT_T, ty = ((t ? w : h) + ORIENT_T - 1) / ORIENT_T;
        if (tx > mx) mx = tx;
        if (ty > my) my = ty;
    }
    *gx = mx; *gy = my;
}

} // namespace zj

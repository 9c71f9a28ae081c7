// zj_mixed.h -- mixed-geometry resized crops (zj_decode_crops_resized_mixed_device): frames that each bring
// their own descriptor through ONE crop launch per sampling mode and ONE reduced-decode launch per (mode, scale).
//
// The kernels (zj_crop_mixed.hip, zj_scaled_mixed.hip) read a frame's record from a table in device memory indexed by
// blockIdx.z instead of from the kernel arguments.  A record is a whole CropParams / ScaledParams holding ONE frame, used
// with frame index 0: the device functions of zj_device.h and zj_scaled.h take `const CropParams&` / `const ScaledParams&`
// and run on it as they are, and the host fills it with the one-geometry fill functions (zj_plan.h) as they are.  Nothing
// of HIP in this header: the library's host side (zj_api.cpp) and the CPU emulation (tests/emu_crop_mixed) share it.
#pragma once

#include <vector>

#include "zj_plan.h"

namespace zj {

constexpr int MIXED_MAX_Z = 65535;        // frames of one mixed launch: the grid's z extent
constexpr size_t MIXED_TAB_ALIGN = 256;   // every run of records starts on such a boundary of the table

// Zeros for the rows of one tight crop at or below rows_covered (Q6): the per-frame record of zj_crop_zero_mixed_kernel
struct MixedZero {
    uint64_t out;                 // the crop
    int y0;                       // the window's first frame row
    int rows_covered;             // of the frame (zj_plan.h: Plan)
    int h;                        // window rows
    int nbytes;                   // bytes of a window row (CHW: of a plane's row)
    int nplanes;                  // 3 for CHW, else 1
    int pad;
};

// one frame of a mixed call, planned: its own plans, its scale and the windows of each stage
struct MixedFrame {
    Plan pl;
    CropPlan cp;
    ScaledPlan sp;                // of scale k (k > 0)
    int k;                        // prescale_pick
    int o;                        // orientation 1..8 (1: none given)
    bool gray;                    // a one-component frame of an RGB call (ZJ_FLAG_GRAY_TO_RGB): planned as GRAYSCALE, expanded later
    unsigned stored[4];           // the window in stored pixels
    unsigned cwin[4];             // the window the crop stage decodes: `stored` at scale 1, else its reduced cover
};

// The checks of one frame in the order of the one-geometry call (zj_api.cpp: crops_resized_impl), first half: the
// orientation's window, the channel count, the crop plan.  shown: the caller's window; o: 0 = no orientation array (an entry
// of the array that is 0 comes as -1: not an orientation).
inline int mixed_frame_plan(const zj_frame_desc* d, const unsigned shown[4], int o, MixedFrame& m)
{
    m.o = 1;
    for (int i = 0; i < 4; i++) m.stored[i] = shown[i];
    if (o) {
        if (!d->width || !d->height) return ZJ_ERR_ARG;
        if (!orient_window(o, d->width, d->height, shown, m.stored)) return ZJ_ERR_ARG;
        m.o = o;
    }
    if (!resize_channels(d) || gray_to_rgb_refused(d)) return ZJ_ERR_UNSUPPORTED;
    m.gray = gray_to_rgb(d);
    const zj_frame_desc e = resized_stage_desc(d); // (what the stages in front of the resize decode: DESIGN.md 3.11)
    return make_crop_plan(&e, 1, 1, 0, m.pl, m.cp);
}

// ... second half: the window inside the frame, the reduced plans up to max_k, the frame's scale and crop-stage window
inline int mixed_frame_window(const zj_frame_desc* d, const unsigned shown[4], unsigned out_w, unsigned out_h, int max_k, MixedFrame& m)
{
    const unsigned* const w = m.stored;
    if (w[2] == 0 || w[3] == 0) return ZJ_ERR_ARG;
    if ((size_t)w[2] > d->width || (size_t)w[3] > d->height) return ZJ_ERR_ARG;
    m.cp.w = (int)w[2]; m.cp.h = (int)w[3];
    int s0, s1, k0, k1, rc;
    if ((rc = crop_window(d, m.pl, m.cp, w[0], w[1], s0, s1, k0, k1))) return rc;
    m.k = max_k > 0 ? prescale_pick(shown[2], shown[3], out_w, out_h, max_k) : 0;
    Plan spl;
    ScaledPlan sp;
    const zj_frame_desc e = resized_stage_desc(d);
    for (int k = 1; k <= max_k; k++) {
        if ((rc = make_scaled_plan(&e, k, spl, sp))) return rc;
        if (k == m.k) m.sp = sp;
    }
    for (int i = 0; i < 4; i++) m.cwin[i] = w[i];
    if (m.k) prescale_window(w, m.k, d->width, d->height, m.cwin);
    return ZJ_OK;
}

// out_colorspace and out_layout are the call's: one output tensor, one channel count, one layout of the crops
inline bool mixed_descs_agree(const zj_frame_desc* descs, size_t n)
{
    for (size_t f = 1; f < n; f++)
        if (descs[f].out_colorspace != descs[0].out_colorspace || descs[f].out_layout != descs[0].out_layout) return false;
    return true;
}

// Every frame's checks of a mixed call, before anything is launched, in the order that decides a bad call's status: the
// descriptors agree; then frame by frame mixed_frame_plan, out_rc (the status of the call's output arguments: one output,
// checked once by the caller), the frame's plane pointers (planes(f, chroma): the caller's check, a status) and
// mixed_frame_window.  The status is the one the single-frame call gives for the first failing frame.  fr: n of them.
template <class Planes>
inline int mixed_check_frames(const zj_frame_desc* descs, size_t n, const unsigned* windows, const uint8_t* orientation,
                              int out_rc, unsigned out_w, unsigned out_h, int max_k, Planes planes, MixedFrame* fr)
{
    if (!mixed_descs_agree(descs, n)) return ZJ_ERR_ARG;
    for (size_t f = 0; f < n; f++) {
        const zj_frame_desc* const d = &descs[f];
        int rc = mixed_frame_plan(d, windows + 4 * f, orientation ? (orientation[f] ? orientation[f] : -1) : 0, fr[f]);
        if (rc) return rc;
        if (out_rc) return out_rc;
        if ((rc = planes(f, fr[f].pl.out != OUT_GRAY))) return rc;
        if ((rc = mixed_frame_window(d, windows + 4 * f, out_w, out_h, max_k, fr[f]))) return rc;
    }
    return ZJ_OK;
}

// The plane rows frame m's crop stage reads: strips [r0, r1) of yrow / crow i16 elements (scale 1), or MCU rows (k > 0).
// Whole strips and MCU rows are contiguous ranges of a plane, and no kernel reads across one (zjint_crop_frame,
// zjint_scaled_frame).
inline void mixed_plane_rows(const zj_frame_desc* d, const MixedFrame& m, size_t& r0, size_t& r1, size_t& yrow, size_t& crow)
{
    const Plan& pl = m.pl;
    if (m.k) {
        r0 = m.cwin[1] / m.sp.mh; r1 = ((size_t)m.cwin[1] + m.cwin[3] + m.sp.mh - 1) / m.sp.mh;
        yrow = (size_t)pl.mcu_x * pl.hs * pl.vs * 64; crow = (size_t)pl.mcu_x * 64;
        return;
    }
    int s0, s1, k0, k1;
    crop_window(d, pl, m.cp, m.stored[0], m.stored[1], s0, s1, k0, k1);
    r0 = (size_t)s0; r1 = (size_t)s1;
    plan_strip_elems(pl, yrow, crow);
}

// One launch of a group: the n records at byte offset `off` of the table, its grid the widest ranges over them.  (The
// launchers cut a run longer than MIXED_MAX_Z frames, the grid's z extent, into launches of that many.)
struct MixedLaunch { int hs, vs, out, sl; size_t off; int n, gx, gy; };

// The tables of one group's frames: runs of CropParams (scale 1) by sampling mode, runs of ScaledParams by (sampling mode,
// scale), one run of MixedZero; every run starts on a MIXED_TAB_ALIGN boundary.  A run's frames have one kernel: where a mode
// holds frames with and without chroma (the gray frames of an RGB call beside its 4:4:4 frames), each kind
// has a run of its own, the colour frames' first.
struct MixedTables {
    std::vector<MixedLaunch> crop, scaled;
    MixedLaunch zero{};           // n == 0: none; gx: the tallest window, gy: the most planes
    size_t bytes = 0;             // of the table that are in use
};

inline size_t mixed_align(size_t v) { return (v + MIXED_TAB_ALIGN - 1) & ~(MIXED_TAB_ALIGN - 1); }

// bytes the tables of frames fr[0 .. n) take at most (32 runs + the zeros, each starting up to one unit late)
inline size_t mixed_table_bytes(const MixedFrame* fr, size_t n)
{
    size_t nc = 0, ns = 0;
    for (size_t f = 0; f < n; f++) (fr[f].k ? ns : nc)++;
    return nc * (sizeof(CropParams) + sizeof(MixedZero)) + ns * sizeof(ScaledParams) + 33 * MIXED_TAB_ALIGN;
}

// Fill `tab` (mixed_table_bytes of it, 16-byte aligned) for frames [0, n) and list the launches.  y / cb / cr / out: the
// frames' addresses as the DEVICE sees them.
inline void mixed_fill_tables(const zj_frame_desc* descs, const MixedFrame* fr, size_t n, const int16_t* const* y,
                              const int16_t* const* cb, const int16_t* const* cr, uint8_t* const* out, uint8_t* tab,
                              MixedTables& t)
{
    t.crop.clear(); t.scaled.clear(); t.zero = MixedLaunch{};
    size_t off = 0;
    for (int mode = 0; mode < 4; mode++) {
        const int hs = 1 + (mode & 1), vs = 1 + (mode >> 1);
        for (int kg = 0; kg < 8; kg++) {
            const int k = kg >> 1;
            const bool chroma = !(kg & 1);
            MixedLaunch run{};
            run.hs = hs; run.vs = vs; run.sl = k; run.off = off;
            for (size_t f = 0; f < n; f++) {
                const MixedFrame& m = fr[f];
                if (m.pl.hs != hs || m.pl.vs != vs || m.k != k || (m.pl.out != OUT_GRAY) != chroma) continue;
                const int16_t* const py = y[f];
                const int16_t* const pcb = chroma ? cb[f] : nullptr;
                const int16_t* const pcr = chroma ? cr[f] : nullptr;
                uint8_t* const po = out[f];
                int gx = 0, gy = 0;
                run.out = m.pl.out;
                if (k == 0) {
                    CropParams& rec = *reinterpret_cast<CropParams*>(tab + off);
                    fill_crop_params_win(&descs[f], m.pl, m.cp, &py, chroma ? &pcb : nullptr, chroma ? &pcr : nullptr, &po, m.cwin, 4, 0, 1, rec, gy, gx);
                    off += sizeof(CropParams);
                } else {
                    ScaledParams& rec = *reinterpret_cast<ScaledParams*>(tab + off);
                    fill_scaled_params(&descs[f], m.pl, m.sp, &py, chroma ? &pcb : nullptr, chroma ? &pcr : nullptr, &po, m.cwin, 0, 0, 1, rec);
                    gx = rec.ncols; gy = rec.nrows;
                    off += sizeof(ScaledParams);
                }
                if (gx > run.gx) run.gx = gx;
                if (gy > run.gy) run.gy = gy;
                run.n++;
            }
            if (run.n) (k ? t.scaled : t.crop).push_back(run);
            off = mixed_align(off);
        }
    }
    // the zeros: every scale-1 frame whose window reaches a row at or below rows_covered
    t.zero.off = off;
    for (size_t f = 0; f < n; f++) {
        const MixedFrame& m = fr[f];
        if (m.k || (long long)m.stored[1] + m.stored[3] <= m.pl.rows_covered) continue;
        MixedZero& z = *reinterpret_cast<MixedZero*>(tab + off);
        z.out = (uint64_t)(uintptr_t)out[f];
        z.y0 = (int)m.stored[1]; z.rows_covered = m.pl.rows_covered; z.h = (int)m.stored[3];
        z.nbytes = (int)m.stored[2] * m.cp.bpp; z.nplanes = m.cp.nplanes; z.pad = 0;
        if (z.h > t.zero.gx) t.zero.gx = z.h;
        if (z.nplanes > t.zero.gy) t.zero.gy = z.nplanes;
        t.zero.n++;
        off += sizeof(MixedZero);
    }
    t.bytes = off;
}

} // namespace zj

// zj_rzgroup.h -- the host-side rules of the resized-crop calls: which filters there are, and how
// the u8 crops of a call pass through the context's scratch buffer in launch groups.  THE one place of the group rule: the
// one-geometry call, the mixed call (zj_api.cpp: rz_finish_group's callers) and the single-file call (zj_jpeg.cpp:
// finish_resized) lay their crops out with rz_group_next and size the buffer with rz_scratch_need.  Nothing of HIP here,
// and no kernel file includes it; tests/emu_crop_mixed exposes the planner to a CPU test at a cap of a few KB.
#pragma once

#include "zj_geom.h"

namespace zj {

inline bool resize_filter_valid(int filter)
{
    return filter == ZJ_RESIZE_BILINEAR || filter == ZJ_RESIZE_BILINEAR_AA || filter == ZJ_RESIZE_BICUBIC_AA;
}

constexpr size_t RZ_GROUP_CAP = (size_t)256 << 20; // u8 crop bytes per launch group of the library's calls

// bytes a tight u8 image takes in the buffer: every image starts on a 16-byte boundary
inline size_t crop_bytes(unsigned w, unsigned h, int channels) { return ((size_t)w * h * channels + 15) & ~(size_t)15; }

// one frame as the planner sees it: the size of the window its crop stage decodes, its orientation (1: not turned), and
// whether it is a one-component frame of a 3-channel call (ZJ_FLAG_GRAY_TO_RGB): its crop stage then writes ONE
// channel, and the image the resize reads is made from that by the expand stage
struct RzFrame { unsigned w, h; int o; int gray = 0; };

// a tight u8 image in the buffer: its byte offset, size and the bytes between its rows (CHW: of a plane's rows)
struct RzImage { size_t off; unsigned w, h, pitch; };

// Where a frame of a group lies.  crop: what the crop stage writes, in the first region.  in: what the resize reads -- the
// crop itself, or, turned, its displayed form (orient_size of the crop's size), in the second region behind all the group's
// crops, the turned frames in order.  A gray frame (expand): crop and, turned, its displayed form are 1-channel images in the
// first and second region; gray names the displayed one of the two, which the expand stage reads; in is the 3-channel image
// it writes, in a third region behind the second, the gray frames in order.
struct RzPlace { RzImage crop, in; bool turned; RzImage gray; bool expand; };

// The group that starts at frame g0, returned as its end g1 > g0.  Greedy and in order: frames are added while the group's
// bytes stay within cap, a turned frame counting its crop's bytes twice (the crop and its displayed form, which has the same
// bytes), a gray frame its 1-channel bytes once or twice and its 3-channel image; a frame that alone exceeds cap forms a group
// of its own.  bytes: of all regions together.  place (nullptr: the sizes alone): place[f] filled for every frame f of the
// group (indexed by frame, not from g0).  Without a gray frame there is no third region and nothing differs.
inline size_t rz_group_next(const RzFrame* fr, size_t n, size_t g0, int channels, bool chw, size_t cap, RzPlace* place,
                            size_t* bytes)
{
    const unsigned bpp = chw ? 1 : (unsigned)channels;
    size_t g1 = g0, first = 0, second = 0, third = 0; // bytes of the regions
    for (; g1 < n; g1++) {
        const bool expand = fr[g1].gray && channels == 3;
        const size_t cb = crop_bytes(fr[g1].w, fr[g1].h, expand ? 1 : channels);
        const size_t eb = expand ? crop_bytes(fr[g1].w, fr[g1].h, channels) : 0;
        const bool turned = fr[g1].o != 1;
        if (g1 > g0 && first + second + third + cb * (turned ? 2 : 1) + eb > cap) break;
        if (place) {
            RzPlace& p = place[g1];
            p.crop = RzImage{first, fr[g1].w, fr[g1].h, fr[g1].w * (expand ? 1 : bpp)};
            p.turned = turned;
            p.expand = expand;
            p.gray.off = second; // (within the second and third region: their starts are known once the group is)
            p.in.off = third;
        }
        first += cb;
        if (turned) second += cb;
        third += eb;
    }
    if (place)
        for (size_t f = g0; f < g1; f++) {
            RzPlace& p = place[f];
            RzImage shown = p.crop; // the displayed form of what the crop stage wrote
            if (p.turned) {
                orient_size(fr[f].o, p.crop.w, p.crop.h, &shown.w, &shown.h);
                shown.off = first + p.gray.off;
                shown.pitch = shown.w * (p.expand ? 1 : bpp);
            }
            const size_t at = first + second + p.in.off;
            p.gray = p.in = shown;
            if (p.expand) { p.in.off = at; p.in.pitch = shown.w * bpp; }
        }
    *bytes = first + second + third;
    return g1;
}

// bytes of the buffer a call over frames [0, n) needs: its largest group's
inline size_t rz_scratch_need(const RzFrame* fr, size_t n, int channels, bool chw, size_t cap)
{
    size_t need = 0, bytes = 0;
    for (size_t g0 = 0; g0 < n;) {
        g0 = rz_group_next(fr, n, g0, channels, chw, cap, nullptr, &bytes);
        if (bytes > need) need = bytes;
    }
    return need;
}

} // namespace zj

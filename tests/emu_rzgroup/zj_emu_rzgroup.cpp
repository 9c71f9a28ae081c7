// zj_emu_rzgroup.cpp -- the launch-group planner of the resized-crop calls (zune-jpeg_amd/csrc/zj_rzgroup.h) for a CPU test,
// gray-to-RGB frames included, at a cap the caller chooses.
//
// TEST INFRASTRUCTURE ONLY: nothing of HIP, never linked into libzjhip.so.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zune-jpeg_amd/csrc/zj_rzgroup.h"

using namespace zj;

// frames of wh[2f], wh[2f + 1], orientation o[f], gray[f] (nullptr: the three-member RzFrame the callers without gray frames
// build) at `cap` bytes (0: the library's).  group[f]: the frame's group; place[16 f ..]: offset, w, h, pitch of its crop, of the
// image the expand stage reads, of the image the resize reads, then turned, expand, 0, 0; gbytes[g]: the group's bytes.  Returns
// rz_scratch_need.
extern "C" size_t zjer_groups(const unsigned* wh, const uint8_t* o, const uint8_t* gray, size_t n, int channels, int chw, size_t cap,
                              int* group, unsigned long long* place, unsigned long long* gbytes)
{
    if (cap == 0) cap = RZ_GROUP_CAP;
    std::vector<RzFrame> fr(n);
    for (size_t f = 0; f < n; f++) {
        if (gray) fr[f] = RzFrame{wh[2 * f], wh[2 * f + 1], o[f], gray[f]};
        else fr[f] = RzFrame{wh[2 * f], wh[2 * f + 1], o[f]};
    }
    std::vector<RzPlace> pl(n);
    int g = 0;
    for (size_t g0 = 0, g1; g0 < n; g0 = g1, g++) {
        size_t bytes = 0;
        g1 = rz_group_next(fr.data(), n, g0, channels, chw != 0, cap, pl.data(), &bytes);
        gbytes[g] = bytes;
        for (size_t f = g0; f < g1; f++) {
            group[f] = g;
            const RzImage im[3] = {pl[f].crop, pl[f].gray, pl[f].in};
            for (int k = 0; k < 3; k++) {
                place[16 * f + 4 * k] = im[k].off; place[16 * f + 4 * k + 1] = im[k].w;
                place[16 * f + 4 * k + 2] = im[k].h; place[16 * f + 4 * k + 3] = im[k].pitch;
            }
            place[16 * f + 12] = pl[f].turned; place[16 * f + 13] = pl[f].expand; place[16 * f + 14] = place[16 * f + 15] = 0;
        }
    }
    return rz_scratch_need(fr.data(), n, channels, chw != 0, cap);
}

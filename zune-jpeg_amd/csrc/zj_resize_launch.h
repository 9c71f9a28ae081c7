// zj_resize_launch.h -- the resize stage's launcher (zj_resize.hip), for zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_resize.h"

namespace zj {
// channels 1 or 3; in_chw: the input's planes (3 channels only); dtype RZ_*; nhwc: the output's layout.  p.rows, p.groups
// and p.nimg filled by the caller (zj_api.cpp: resize_launches)
hipError_t launch_resize(int channels, int in_chw, int dtype, int nhwc, const ResizeParams& p, hipStream_t s);
// the antialiased filter (zj_resize_aa.hip): the same arguments; p.rows and p.groups are not read
hipError_t launch_resize_aa(int channels, int in_chw, int dtype, int nhwc, const ResizeParams& p, hipStream_t s);
// the bicubic antialiased filter (zj_resize_bicubic.hip): as launch_resize_aa
hipError_t launch_resize_bicubic(int channels, int in_chw, int dtype, int nhwc, const ResizeParams& p, hipStream_t s);
} // namespace zj

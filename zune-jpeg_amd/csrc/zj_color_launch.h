// zj_color_launch.h -- the colour-matrix stage's launcher (zj_color.hip), for zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_color.h"

namespace zj {
// chw: the input and the output are three planes, their pitch x h apart, instead of interleaved pixels.  p.nimg
// 1..COLOR_BATCH, every size 1..65535
hipError_t launch_color(int chw, const ColorParams& p, hipStream_t s);
} // namespace zj

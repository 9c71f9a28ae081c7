// zj_expand_launch.h -- the gray-to-RGB stage's launcher (zj_expand.hip), for zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_expand.h"

namespace zj {
// out_chw: three planes, out_pitch x h apart, instead of interleaved pixels.  p.nimg 1..EXPAND_BATCH, every size 1..65535
hipError_t launch_expand(int out_chw, const ExpandParams& p, hipStream_t s);
} // namespace zj

// zj_cmyk_launch.h -- the CMYK-to-RGB stage's launcher (zj_cmyk.hip), for zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_cmyk.h"

namespace zj {
// chw: a and the output are three planes, their pitch x h apart, instead of interleaved pixels.  p.nimg 1..CMYK_BATCH, every
// size 1..65535
hipError_t launch_cmyk(int chw, const CmykParams& p, hipStream_t s);
} // namespace zj

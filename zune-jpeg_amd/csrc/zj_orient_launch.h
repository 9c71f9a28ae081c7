// zj_orient_launch.h -- the orient stage's launcher (zj_orient.hip), for zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_orient.h"

namespace zj {
// channels 1 or 3; in_chw: planes (3 channels only), oriented one by one.  p.nimg 1..ORIENT_BATCH, every p.o[i] 1..8
hipError_t launch_orient(int channels, int in_chw, const OrientParams& p, hipStream_t s);
} // namespace zj

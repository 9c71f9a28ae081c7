// zj_warp_launch.h -- the affine-warp stage's launcher (zj_warp.hip), for zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_warp.h"

namespace zj {
// p.nimg 1..WARP_BATCH images of 1..65535 a side, `channels` 1 or 3 (interleaved), into p.out_w x p.out_h (1..8192 each)
hipError_t launch_warp(int channels, const WarpParams& p, hipStream_t s);
} // namespace zj

// zj_scaled_launch.h -- launcher prototype shared by zj_scaled.hip and zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_scaled.h"

namespace zj {
// reduced-size decode (zj_decode_crops_scaled_device): the tile kernel over a launch's frames
hipError_t launch_scaled(int hs, int vs, int out, int scale_log2, const ScaledParams& p, hipStream_t s);
} // namespace zj

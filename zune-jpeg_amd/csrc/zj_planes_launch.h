// zj_planes_launch.h -- the planes-to-RGB stage's launcher (zj_planes.hip), for zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_planes.h"

namespace zj {
// chw: the output is three planes, its pitch x h apart, instead of interleaved pixels; stored_rgb: the samples are R, G, B
// as they are, not Y, Cb, Cr.  p.nimg 1..PLANES_BATCH, every size 1..65535
hipError_t launch_planes(int chw, int stored_rgb, const PlanesParams& p, hipStream_t s);
} // namespace zj

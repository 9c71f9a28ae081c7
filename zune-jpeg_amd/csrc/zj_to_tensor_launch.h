// zj_to_tensor_launch.h -- the u8-images-to-tensor stage's launcher (zj_to_tensor.hip), for zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_to_tensor.h"

namespace zj {
// p.nimg 1..TT_BATCH images of p.w x p.h (1..65535), p.cin -> p.cout channels 1 -> 1, 1 -> 3 or 3 -> 3
hipError_t launch_to_tensor(const ToTensorParams& p, hipStream_t s);
} // namespace zj

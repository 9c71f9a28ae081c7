// zj_mixed_launch.h -- launcher prototypes shared by zj_crop_mixed.hip, zj_scaled_mixed.hip and zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_mixed.h"

namespace zj {
// mixed-geometry crops (zj_decode_crops_resized_mixed_device).  d_tab: n records in DEVICE memory, one
// per frame, each a one-frame CropParams / ScaledParams / MixedZero; ncols x nstrips (ncols x nrows, max_h x max_planes):
// the widest ranges over the records.  More than MIXED_MAX_Z records go out as launches of that many.
hipError_t launch_crop_mixed(int hs, int vs, int out, const CropParams* d_tab, int n, int ncols, int nstrips, hipStream_t s);
hipError_t launch_crop_zero_mixed(const MixedZero* d_tab, int n, int max_h, int max_planes, hipStream_t s);
hipError_t launch_scaled_mixed(int hs, int vs, int out, int scale_log2, const ScaledParams* d_tab, int n, int ncols, int nrows,
                               hipStream_t s);
} // namespace zj

// zj_crop_tensor_launch.h -- launcher prototypes shared by zj_crop_tensor.hip and zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_crop_tensor.h"

namespace zj {
// crop windows into a normalised tensor (zj_decode_crops_tensor_device, zj_decode_crops_tensor_mixed_device).
// d_tab: nrec records in DEVICE memory, each holding up to 2^shift frames of one geometry; ncols x nstrips (max_rows x
// max_frames): the widest ranges over the records.  More records than a grid's z extent holds go out as several launches.
hipError_t launch_crop_tensor(int hs, int vs, int out, const CropTensorParams* d_tab, int nrec, int shift, int ncols, int nstrips,
                              hipStream_t s);
hipError_t launch_crop_tensor_zero(const CropTensorZero* d_tab, int nrec, int max_rows, int max_frames, hipStream_t s);
} // namespace zj

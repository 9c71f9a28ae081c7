// zj_tone_launch.h -- the tone stages' launchers (zj_tone.hip), for zj_api.cpp
#pragma once
#include <hip/hip_runtime.h>

#include "zj_tone.h"

namespace zj {
// channels 1 or 3; chw: three planes, their pitch x h apart, instead of interleaved pixels (one channel: either).  p.nimg
// 1..HIST_BATCH, every size 1..65535, every table zeroed on the stream in front of the launch
hipError_t launch_hist(int channels, int chw, const HistParams& p, hipStream_t s);
// p.nimg 1..TONE_LUT_BATCH, p.channels 1 or 3, every op valid (tone_op_valid), p.hist set where an op needs it
hipError_t launch_tone_lut(const ToneLutParams& p, hipStream_t s);
// as launch_hist; p.nimg 1..LUT_BATCH
hipError_t launch_lut(int channels, int chw, const LutParams& p, hipStream_t s);
} // namespace zj

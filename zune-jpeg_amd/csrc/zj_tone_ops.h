// zj_tone_ops.h -- the ops of the tone stage and their argument rule.  Nothing of HIP here: the kernels'
// header (zj_tone.h), zj_api.cpp's entry points, the front-end (zj_jpeg.cpp) and tests/emu_tone use the same functions
// (constexpr: callable from host and device code alike).
#pragma once

#include <stdint.h>

namespace zj {

// the values of include/zjhip.h's ZJ_TONE_*
constexpr int TONE_IDENTITY = 0, TONE_INVERT = 1, TONE_POSTERIZE = 2, TONE_SOLARIZE = 3, TONE_AUTOCONTRAST = 4, TONE_EQUALIZE = 5;

// an op the stage takes: posterize bits 1..8, solarize threshold 0..256, every other op with param 0
constexpr bool tone_op_valid(const int32_t op, const int32_t param)
{
    return op == TONE_POSTERIZE  ? param >= 1 && param <= 8
           : op == TONE_SOLARIZE ? param >= 0 && param <= 256
                                 : op >= TONE_IDENTITY && op <= TONE_EQUALIZE && param == 0;
}
// its table is computed from the image's histogram
constexpr bool tone_needs_hist(const int32_t op) { return op == TONE_AUTOCONTRAST || op == TONE_EQUALIZE; }

} // namespace zj

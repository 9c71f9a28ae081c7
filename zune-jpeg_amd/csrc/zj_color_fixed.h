// zj_color_fixed.h -- the host-side rule of the colour-matrix stage: a matrix of 12 doubles as the 12
// integers the kernel takes.  Nothing of HIP here: zj_api.cpp's entry points (zj_color_fixed, zj_color_device), the front-end
// (zj_jpeg.cpp) and tests/emu_color call the same functions.
#pragma once

#include <stdint.h>

namespace zj {

constexpr int COLOR_ONE = 65536; // 1.0 of a matrix entry

// m[4 c + k], k = 0..2: what multiplies R, G, B in output channel c; k = 3: an offset in grey levels.
// q = floor(m 65536 + 1/2), the product, the sum and the floor in doubles.  false: an entry that is not finite,
// |m[c][0..2]| > 16 or |m[c][3]| > 4096 -- under these |q[c][0..2]| <= 2^20 and |q[c][3]| <= 2^28.
inline bool color_fixed(const double* m, int32_t* q)
{
    for (int k = 0; k < 12; k++) {
        const double v = m[k], lim = (k & 3) == 3 ? 4096.0 : 16.0;
        if (!(v >= -lim && v <= lim)) return false; // (a NaN fails both)
        const double t = v * 65536.0 + 0.5;
        double f = (double)(long long)t; // (|t| < 2^29)
        if (f > t) f -= 1.0;
        q[k] = (int32_t)f;
    }
    return true;
}

// the identity's integers: such an image is left as it is
inline bool color_is_identity(const int32_t* q)
{
    for (int k = 0; k < 12; k++)
        if (q[k] != ((k >> 2) == (k & 3) ? COLOR_ONE : 0)) return false;
    return true;
}

} // namespace zj

// Library-internal calls: defined in zj_api.cpp (the pixel path), used by the front-end zj_jpeg.cpp.  Hidden like everything
// the public header does not declare.  Both files include this one header, so a definition that drifts from what the
// front-end calls no longer compiles.
// ZJINT_DECL: what stands in front of every declaration.  zj_api.cpp leaves it empty.  zj_jpeg.cpp defines it as the weak
// attribute: the front-end's CPU-only builds (the sanitizer and fuzz harnesses, the routing stub of the tests) link without
// the pixel path, and its entry points test the symbols they need (ZJ_ERR_UNSUPPORTED: a build without the pixel path).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zjhip.h"

#ifndef ZJINT_DECL
#define ZJINT_DECL
#endif

extern "C" {
// crop windows from host or device planes, the entropy stage alone, an all-zero window
ZJINT_DECL int zjint_crop_frame(zj_ctx* c, const zj_frame_desc* d, const int16_t* y, const int16_t* cb, const int16_t* cr,
                                int planes_on_device, unsigned x, unsigned yy, unsigned w, unsigned h, uint8_t* d_out, unsigned out_pitch);
ZJINT_DECL int zjint_scan_to_planes(zj_ctx* c, const zj_frame_desc* d, const void* blob, size_t blob_bytes, const int16_t* planes[3],
                                    unsigned* status_bits);
ZJINT_DECL int zjint_crop_zeros(zj_ctx* c, const zj_frame_desc* d, unsigned x, unsigned yy, unsigned w, unsigned h, uint8_t* d_out,
                                unsigned out_pitch);
// ... and the resized crop's buffer and resize
ZJINT_DECL int zjint_resize_scratch(zj_ctx* c, size_t bytes, uint8_t** p);
ZJINT_DECL int zjint_resize_one(zj_ctx* c, const uint8_t* in, unsigned w, unsigned h, int channels, int in_layout, unsigned out_w,
                                unsigned out_h, int dtype, int out_layout, const float* scale, const float* bias, int flip, int filter,
                                void* d_out);
// ... and one image turned to its displayed form
ZJINT_DECL int zjint_scratch_idle(zj_ctx* c, size_t bytes, uint8_t** p);
ZJINT_DECL int zjint_orient_one(zj_ctx* c, const uint8_t* in, unsigned w, unsigned h, int channels, int in_layout, int o, uint8_t* d_out);
// ... and one plane expanded to an RGB image with R = G = B
ZJINT_DECL int zjint_gray_to_rgb_one(zj_ctx* c, const uint8_t* in, unsigned w, unsigned h, int out_layout, uint8_t* d_out);
// ... and one image combined in place with one plane, (a * k + 127) / 255
ZJINT_DECL int zjint_cmyk_to_rgb_one(zj_ctx* c, uint8_t* a, const uint8_t* k, unsigned w, unsigned h, int layout, int inverted);
// ... and three component planes box-replicated and converted into one image
ZJINT_DECL int zjint_planes_to_rgb_one(zj_ctx* c, const uint8_t* const planes[3], unsigned w, unsigned h, const uint8_t ratios[6],
                                       const uint8_t phases[6], int stored_rgb, int layout, uint8_t* d_out);
// ... and the reduced-size decode of one frame's window
ZJINT_DECL int zjint_scaled_frame(zj_ctx* c, const zj_frame_desc* d, const int16_t* y, const int16_t* cb, const int16_t* cr,
                                  int planes_on_device, int scale_log2, unsigned x, unsigned yy, unsigned w, unsigned h, uint8_t* d_out,
                                  unsigned out_pitch);
// ... and one frame's window converted straight into a tensor image
ZJINT_DECL int zjint_crop_tensor_frame(zj_ctx* c, const zj_frame_desc* d, const int16_t* y, const int16_t* cb, const int16_t* cr,
                                       int planes_on_device, unsigned x, unsigned yy, unsigned w, unsigned h, int dtype, int out_layout,
                                       const float* scale, const float* bias, int flip, void* d_out);
// ... and one u8 image converted into a tensor image at its own size
ZJINT_DECL int zjint_to_tensor_one(zj_ctx* c, const uint8_t* in, unsigned w, unsigned h, int in_channels, int channels, int dtype,
                                   int out_layout, const float* scale, const float* bias, int flip, void* d_out);
// ... and one u8 image warped into a tensor image under six integers (w == 0: no image, all fill)
ZJINT_DECL int zjint_warp_one(zj_ctx* c, const uint8_t* in, unsigned w, unsigned h, int channels, const int64_t q[6], unsigned out_w,
                              unsigned out_h, int dtype, int out_layout, const float* scale, const float* bias, const uint8_t* fill,
                              int edge, void* d_out);
// ... and one image mapped in place under the 12 integers of a colour matrix (the identity's: no launch)
ZJINT_DECL int zjint_color_one(zj_ctx* c, uint8_t* img, unsigned w, unsigned h, int layout, const int32_t q[12]);
// ... and under a tone op of two int32 (ZJ_TONE_IDENTITY: no launch): channels 1 or 3
ZJINT_DECL int zjint_tone_one(zj_ctx* c, uint8_t* img, unsigned w, unsigned h, int channels, int layout, const int32_t op[2]);

// The mixed-geometry calls over several files' planes in HOST memory, each file of its own geometry; d_out: the first file's
// image, the others behind it.  Synchronous: the planes may be reused when they return.
// ... the resized crops
ZJINT_DECL int zjint_crops_resized_mixed_host(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                              const int16_t* const* cb, const int16_t* const* cr, const unsigned* windows,
                                              unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                              const float* bias, const uint8_t* flip, int filter, int max_prescale_log2,
                                              const uint8_t* orientation, void* d_out);
// ... the resized crops with file f's image under the integers color_q[12f .. 12f + 11] first (nullptr: none)
ZJINT_DECL int zjint_crops_resized_mixed_colored_host(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                                      const int16_t* const* cb, const int16_t* const* cr, const unsigned* windows,
                                                      unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                                      const float* bias, const uint8_t* flip, int filter, int max_prescale_log2,
                                                      const uint8_t* orientation, const int32_t* color_q, void* d_out);
// ... and under the op tone[2f], tone[2f + 1] behind that (nullptr: none)
ZJINT_DECL int zjint_crops_resized_mixed_toned_host(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                                    const int16_t* const* cb, const int16_t* const* cr, const unsigned* windows,
                                                    unsigned out_w, unsigned out_h, int dtype, int out_layout, const float* scale,
                                                    const float* bias, const uint8_t* flip, int filter, int max_prescale_log2,
                                                    const uint8_t* orientation, const int32_t* color_q, const int32_t* tone,
                                                    void* d_out);
// ... the crop tensors, every window w x h
ZJINT_DECL int zjint_crops_tensor_mixed_host(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                             const int16_t* const* cb, const int16_t* const* cr, const unsigned* origins, unsigned w,
                                             unsigned h, int dtype, int out_layout, const float* scale, const float* bias,
                                             const uint8_t* flip, void* d_out);
// ... the crops of each launch group warped
ZJINT_DECL int zjint_crops_warped_mixed_host(zj_ctx* c, const zj_frame_desc* descs, size_t nframes, const int16_t* const* y,
                                             const int16_t* const* cb, const int16_t* const* cr, const unsigned* windows,
                                             const int64_t* q, unsigned out_w, unsigned out_h, int dtype, int out_layout,
                                             const float* scale, const float* bias, const uint8_t* fill, int edge,
                                             const uint8_t* orientation, void* d_out);
}

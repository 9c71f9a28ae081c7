/*
 * zjhip.h -- C ABI of libzjhip.so: zune-jpeg's post-entropy pixel path on MI355X (gfx950).
 *
 * The library replaces, for the `hip` arm of the reference's function-pointer dispatch, exactly
 * the functions that sit behind these reference interfaces (paths relative to the zune-jpeg tree):
 *
 *   IDCTPtr            = fn(&[i16], &Aligned32<[i32;64]>, usize, usize, usize) -> Vec<i16>
 *                        src/decoder.rs:56, chosen by choose_idct_func          src/idct.rs:40
 *   UpSampler          = fn(&[i16], usize) -> Vec<i16>
 *                        src/components.rs:14, chosen in Decoder::set_upsampling src/decoder.rs:468
 *   ColorConvert16Ptr  = fn(&[i16;16], &[i16;16], &[i16;16], &mut [u8], &mut usize)
 *                        src/decoder.rs:47, chosen by choose_ycbcr_to_rgb_convert_func
 *                                                                         src/color_convert.rs:61
 *   post_process(coeff, component_data, idct_func, color_convert_16, in_cs, out_cs, output, width)
 *                        src/worker.rs:32, called per strip from src/mcu.rs:364 and
 *                        src/mcu_prog.rs:214,228
 *
 * plus the frame/batch-level entry points the GPU actually wants (whole-image coefficient planes,
 * the layout src/mcu_prog.rs:73-79 allocates; baseline strips concatenate to the same planes).
 *
 * Conventions: plain C types, caller-owned buffers, int status (0 = ZJ_OK, negative = error), no
 * exceptions or aborts across the boundary.  Where the reference would panic (slice bounds,
 * unwrap, assert!) the call returns ZJ_ERR_PANIC and leaves the output unspecified.  Results are
 * bit-exact with the reference's SCALAR arms (ZuneJpegOptions::set_use_unsafe(false)).
 * Everything runs on the GPU: there is no CPU fallback; without a usable HIP device every
 * entry point that computes returns ZJ_ERR_NO_DEVICE.
 *
 * Thread safety: a zj_ctx owns one HIP stream and scratch buffers; use one ctx per (thread, device).
 */
#ifndef ZJHIP_H
#define ZJHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZJ_ABI_VERSION 8

/* libzjhip.so is built with -fvisibility=hidden: the functions declared here are its whole dynamic symbol table */
#if defined(__GNUC__) || defined(__clang__)
#define ZJ_API __attribute__((visibility("default")))
#else
#define ZJ_API
#endif

/* ColorSpace, same order as src/misc.rs:88-106 */
typedef enum zj_colorspace {
    ZJ_CS_RGB = 0,
    ZJ_CS_GRAYSCALE = 1,
    ZJ_CS_YCBCR = 2,
    ZJ_CS_CMYK = 3,
    ZJ_CS_YCCK = 4,
    ZJ_CS_RGBA = 5,
    ZJ_CS_RGBX = 6
} zj_colorspace;

/* Arms of the reference's dispatch (src/idct.rs:40-61, src/upsampler.rs:82-112,
 * src/color_convert.rs:61-107).  SCALAR and AVX2 stay in the host application (the Rust crate);
 * this library implements only the HIP arm and reports ZJ_ERR_BACKEND for the others. */
typedef enum zj_backend { ZJ_BACKEND_SCALAR = 0, ZJ_BACKEND_AVX2 = 1, ZJ_BACKEND_HIP = 2 } zj_backend;

typedef enum zj_status {
    ZJ_OK = 0,
    ZJ_ERR_ARG = -1,         /* null pointer / inconsistent sizes */
    ZJ_ERR_UNSUPPORTED = -2, /* valid for the reference, not implemented by this library */
    ZJ_ERR_HIP = -3,         /* a HIP runtime call failed; see zj_last_error() */
    ZJ_ERR_NOMEM = -4,
    ZJ_ERR_PANIC = -5,       /* the reference would panic on these arguments */
    ZJ_ERR_NO_DEVICE = -6,   /* no usable HIP device / kernels could not be loaded */
    ZJ_ERR_BACKEND = -7,     /* backend other than ZJ_BACKEND_HIP requested */
    /* zj_decoder_* only: the variants of DecodeErrors (src/errors.rs:16-43); text via zj_decoder_error() */
    ZJ_ERR_FORMAT = -20,             /* Format / FormatStatic */
    ZJ_ERR_MAGIC = -21,              /* IllegalMagicBytes */
    ZJ_ERR_HUFFMAN = -22,            /* HuffmanDecode */
    ZJ_ERR_ZERO = -23,               /* ZeroError */
    ZJ_ERR_DQT = -24,                /* DqtError */
    ZJ_ERR_SOS = -25,                /* SosError */
    ZJ_ERR_SOF = -26,                /* SofError */
    ZJ_ERR_UNSUPPORTED_SCHEME = -27, /* Unsupported(UnsupportedSchemes) */
    ZJ_ERR_MCU = -28,                /* MCUError */
    ZJ_ERR_EXHAUSTED = -29,          /* ExhaustedData */
    ZJ_ERR_LARGE_DIM = -30,          /* LargeDimensions */
    /* zj_decode_scan only (not an error): the device met something in the scan that only the CPU walker treats the way
     * the reference does (a damaged stream, the reference's early exit before the last row loop): decode on the CPU */
    ZJ_RETRY_CPU = 1
} zj_status;

/* The fields of `Components` (src/components.rs:18-43) the pixel path reads. */
typedef struct zj_component {
    size_t horizontal_sample;       /* components.rs:25 */
    size_t vertical_sample;         /* components.rs:23 */
    size_t width_stride;            /* components.rs:40; headers.rs:338 = h_samp * mcu_x * 8 */
    int32_t quantization_table[64]; /* components.rs:33, natural order, values 0..255 */
} zj_component;

/* One frame of whole-image coefficient planes (src/mcu_prog.rs:62-79). */
typedef struct zj_frame_desc {
    uint32_t width, height;  /* pixels */
    uint32_t h_max, v_max;   /* luma sampling factors: (1,1) (2,1) (1,2) (2,2); chroma is (1,1) */
    uint32_t in_components;  /* 1 (grayscale JPEG) or 3 (YCbCr) */
    int32_t out_colorspace;  /* ZJ_CS_RGB, ZJ_CS_GRAYSCALE or ZJ_CS_YCBCR; extension: ZJ_CS_RGBA / ZJ_CS_RGBX */
    int32_t qt[3][64];       /* per component, natural order, values 0..255 (8-bit DQT only,
                                src/headers.rs:154-174) */
    uint32_t flags;          /* 0 = the reference's bytes exactly; ZJ_FLAG_* below */
    uint32_t out_layout;     /* ZJ_LAYOUT_HWC (0, the reference's interleaved bytes) or ZJ_LAYOUT_CHW */
    uint32_t out_pitch;      /* bytes between the starts of consecutive output rows (CHW: of a plane's rows); 0 = tight,
                                width x components: the reference's layout (src/mcu.rs:375-379).  Device outputs only
                                (zj_decode_planes_device*, zj_decode_frames_device, zj_multi_decode_frames_device). */
} zj_frame_desc;

/* Extensions beyond the reference, all off by default.  They keep the reference's strips and its
 * per-pixel arithmetic (Q3 and Q7 always hold) and have no reference output; the checker is the oracle's
 * zjo_decode_planes_ext:
 *   ZJ_FLAG_PLAIN_TAIL      (RGB) every pixel x < width of a converted row is written at 3x: the last 16 samples
 *                           are not written 16 bytes early (Q5) and no byte of the row stays 0 (Q6);
 *   ZJ_FLAG_CLAMP_DC        the DC-only shortcut value is clamped to 0..255 (Q1 corrected; the reference's AVX2 arm
 *                           does this, src/idct/avx2.rs:163-167, its scalar arm does not);
 *   ZJ_FLAG_EDGE_REPLICATE  (h2v1 / h2v2) the horizontal chroma filter runs row by row with replicated edges
 *                           instead of over the strip as one flat array (Q4 corrected);
 *   ZJ_FLAG_CORRECTED       all three: the "non-quirk" mode.  What stays: the vertical schedule (Q3) and the
 *                           dropped odd MCU row are properties of the reference's strip geometry (a corrected
 *                           vertical filter needs taps across strips);
 *   ZJ_CS_RGBA / RGBX       4 bytes per pixel, R G B 255 (the reference's own RGBA arm is malformed),
 *                           plain placement;
 *   ZJ_LAYOUT_CHW           (RGB) three u8 planes of width*height bytes per frame, the tensor layout ML consumers
 *                           want, plain placement.  GRAYSCALE is accepted (one plane: identical to HWC);
 *   out_pitch               rows laid out wider than they are, for outputs that stay in HBM: >= the row's bytes, a
 *                           multiple of 16 when width % 16 == 0, at most 1 MiB; zj_out_len() = out_pitch x height
 *                           (x 3 for CHW).  The bytes between a row's end and the next row's start are never
 *                           written.  A tile's row segment then starts on a cache-line boundary whenever the pitch is
 *                           a multiple of 128: frames whose tight pitch is not (any RGB width that is not a multiple
 *                           of 128 pixels) decode 10-20 % faster into such a pitch.  Host-output
 *                           entry points return ZJ_ERR_UNSUPPORTED for a padded pitch. */
#define ZJ_FLAG_PLAIN_TAIL 1u
#define ZJ_FLAG_CLAMP_DC 2u
#define ZJ_FLAG_EDGE_REPLICATE 4u
#define ZJ_FLAG_CORRECTED 7u
/* zj_options.flags only (the CPU front-end; never passed on to a zj_frame_desc): AC values as the file codes them.  The
 * reference packs a fast-AC value as `k << 10` into an i16 (src/huffman.rs:251) and reads it back with `>> 10`
 * (src/bitstream.rs:343,466): a value of size 6..8 whose code and magnitude fit its 9-bit look-ahead (a code of 1..3 bits --
 * optimised tables, progressive files) keeps six bits, sign-extended: +104 decodes as -24.  The default reproduces that
 * (the reference's own test-images/test-progressive.jpg: 958 coefficients in 649 of 97 200 blocks); with this flag the
 * front-end yields the coded values, which is what libjpeg decodes. */
#define ZJ_FLAG_FULL_AC_VALUES 8u
/* Gray to RGB: a one-component JPEG shown as an RGB image with R = G = B, what image viewers and
 * Pillow's convert("RGB") give.  Off by default, and honoured by the RESIZED-CROP family and, for files, by the crop-tensor
 * file calls (zj_decoder_finish_pixels_crop_tensor*_device: the GRAYSCALE u8 crop through zj_to_tensor_device, 1 -> 3
 * channels) only:
 *   zj_frame_desc.flags   zj_decode_crops_resized_device, _filtered_, _prescaled_, _oriented_ and _mixed_, and
 *                         zj_resized_out_len: a descriptor with in_components == 1 and out_colorspace == ZJ_CS_RGB is decoded
 *                         as GRAYSCALE and expanded to 3 channels in front of the resize (without the flag such a descriptor
 *                         is refused: ZJ_ERR_UNSUPPORTED).  Every other entry point returns what it returns for an unknown
 *                         flag bit (ZJ_ERR_ARG);
 *   zj_options.flags      a one-component file finished through zj_decoder_finish_pixels_resized_crop*_device, the batch
 *                         call or the crop-tensor file calls by a decoder whose out_colorspace is ZJ_CS_RGB gives a 3-channel image: the slot size,
 *                         *out_len and the capacity check all use 3 channels.  (Without the flag the file is GRAYSCALE
 *                         whatever the decoder asks for, src/headers.rs:283-290: a 1-channel image.)
 * DEFINITION: the image equals, byte for byte, zj_resize_filtered_device applied to the 3-channel u8 image E, in the layout
 * (HWC or CHW) the call's colour crops have, every channel of which is the displayed u8 crop the same call writes for that
 * frame with out_colorspace = ZJ_CS_GRAYSCALE -- same filter, prescale pick, orientation, flip, scale, bias, dtype and tensor
 * layout.  Three-component frames and files: the flag does nothing, so a caller can set it everywhere; in a mixed call gray
 * and colour frames share the launch groups and the resize launches, and the colour frames keep the bytes they have without
 * the gray ones.  One component with ZJ_CS_YCBCR: ZJ_ERR_UNSUPPORTED. */
#define ZJ_FLAG_GRAY_TO_RGB 16u
/* CMYK to RGB: a four-component JPEG (Adobe CMYK or YCCK) shown as an RGB image, what Pillow's convert("RGB")
 * and the common tensor loaders' RGB mode give.  zj_options.flags ONLY (on a zj_frame_desc it is an unknown bit, ZJ_ERR_ARG).
 * Without it a four-component file is refused at its SOF segment as ever (ZJ_ERR_SOF, the reference's text).  With it the
 * front-end accepts Nf = 4 in SOF0 / SOF2 -- any component ids; components 2 and 3 at (1,1), components 1 and 4 both at the
 * (h_max, v_max) of one of the four known modes, anything else ZJ_ERR_UNSUPPORTED -- reads the Adobe APP14 segment
 * (zj_decoder_adobe_transform) and decodes the scans in a serial walk of its own: the coefficients are the values the file
 * codes (no six-bit cut, none of the reference reader's quirks: the reference has no such path).  The parallel scan, restart
 * threads, streaming and the device entropy stage leave such a file to that walk, whatever zj_options.entropy says.
 * Component 4's plane has the layout of a one-component frame of the same size, ceil(w/8) x ceil(h/8) blocks.
 * The zj_frame_desc that zj_decoder_prepare / zj_decoder_decode_coefficients fill for such a file (in_components = 4) does
 * NOT describe a frame any frame-level call accepts: callers that want the stages themselves take the planes from
 * zj_decoder_plane and build descriptors of their own -- three components for planes 0-2, one component for plane 3.
 * A file whose width is below 57 and no multiple of 8 is ZJ_ERR_PANIC at full resolution, as a one-component frame of that
 * width is (component 4's GRAYSCALE decode); a reduced-size decode under the resize (max_prescale_log2) decodes it.
 * Such a file is finished by the RESIZED-CROP family (zj_decoder_finish_pixels_resized_crop*_device and the batch call) and
 * by the crop-tensor file calls (zj_decoder_finish_pixels_crop_tensor*_device: E below through zj_to_tensor_device, DESIGN.md
 * 3.15) only, by a decoder whose out_colorspace is ZJ_CS_RGB; every other finish call, zj_decoder_decode_buffer and the pool, and a decoder
 * that asks for GRAYSCALE or YCBCR, return ZJ_ERR_UNSUPPORTED.
 * DEFINITION: the image equals, byte for byte, zj_resize_filtered_device applied to the 3-channel u8 image E with
 * E[c] = zj_cmyk_to_rgb_device(A[c], K): A the displayed u8 crop the same call writes for a three-component frame made of the
 * file's components 1-3 (their tables, the file's sampling, the decoder's flags and layout), decoded as ZJ_CS_RGB when the
 * Adobe transform is 2 (YCCK) and as ZJ_CS_YCBCR -- the stored samples, up-sampled, always HWC -- otherwise; K the displayed
 * u8 crop of the GRAYSCALE decode of a one-component frame made of component 4; `inverted` set when an Adobe segment was
 * seen (Adobe files store complemented samples; without the segment the samples are complemented first, Pillow's rule);
 * same filter, prescale pick, orientation, flip, scale, bias, dtype and tensor layout.  One- and three-component files: the
 * flag does nothing (their Adobe segment stays ignored), so a loader sets it once.  In the batch call a four-component file
 * goes through its single-file call; the files around it keep the bytes they have without it. */
#define ZJ_FLAG_CMYK_TO_RGB 32u
/* Any sampling: three-component JPEGs the reference refuses -- 4:1:1 and 4:1:0 files, chroma that is not
 * (1,1), component ids outside 1..3 -- and files whose samples are stored RGB, shown as RGB images.  zj_options.flags ONLY (on
 * a zj_frame_desc it is an unknown bit, ZJ_ERR_ARG).  Without it every file gives the status and the text it always gave.
 * With it a three-component SOF0 / SOF2 frame is accepted with any component ids and every h and v in {1, 2, 4} (any other
 * factor: ZJ_ERR_UNSUPPORTED, the three (h,v) pairs in its text), so that every ratio rx = h_max / h, ry = v_max / v is 1, 2 or 4.
 * A file is NON-STANDARD when its sampling is outside the four known modes (chroma (1,1) under luma (1,1) / (2,1) / (1,2) /
 * (2,2)), or an id is outside 1..3, or it is STORED RGB: its Adobe APP14 segment says transform 0 (zj_decoder_stored_rgb;
 * Pillow's save(keep_rgb=True) writes this).  A standard file goes through exactly the walkers and kernels it goes through
 * without the flag, byte for byte.  A non-standard one is decoded by the serial T.81 walk of four-component files (the values
 * the file codes, none of the reference reader's quirks; the parallel scan, restart threads, streaming and the device entropy
 * stage are never entered, whatever zj_options.entropy says), and EVERY component's plane has the layout of a one-component
 * frame of the component's own size: ceil(cw/8) x ceil(ch/8) blocks, cw = ceil(W h / h_max), ch = ceil(H v / v_max)
 * (zj_decoder_plane, zj_decoder_component_sampling).  The zj_frame_desc filled for such a file does NOT describe a frame
 * any frame-level call accepts.
 * Such a file is finished by the RESIZED-CROP family and the crop-tensor file calls (E below through zj_to_tensor_device,
 * DESIGN.md 3.15) only, by a decoder whose out_colorspace is ZJ_CS_RGB; every other finish
 * call, zj_decoder_decode_buffer and the pool return ZJ_ERR_UNSUPPORTED.
 * DEFINITION (bit-exact): the image is zj_resize_filtered_device applied to the displayed form of the 3-channel u8 image E over
 * the stored window (x, y, w, h): E[r][c] = colour(S_0[(y+r) / ry_0][(x+c) / rx_0], S_1[...], S_2[...]), integer divisions
 * (box replication, libjpeg's rule for every ratio but 2); S_i the clamped 8-point IDCT of component i's blocks with its own
 * table, the DC-only shortcut clamped too (the GRAYSCALE crop, ZJ_FLAG_CLAMP_DC, of a one-component frame of the plane's padded
 * size 8 bw x 8 bh); colour the full decode's per-pixel YCbCr -> RGB, the identity for stored RGB.  Same filter, orientation,
 * flip, scale, bias, dtype and tensor layout as for any file.  max_prescale_log2 is taken as 0 for such a file: the reduced
 * decode is isotropic and these ratios are not, and the pick s = 1 is "decoded and resized exactly as before".  A component
 * whose padded plane is wider or higher than 65535 samples is ZJ_ERR_ARG from its crop.  In the batch call such a file goes
 * through its single-file call; the files around it keep the bytes they have without it. */
#define ZJ_FLAG_ANY_SAMPLING 64u
#define ZJ_LAYOUT_HWC 0u
#define ZJ_LAYOUT_CHW 1u

typedef struct zj_ctx zj_ctx;

/* ---- lifecycle ------------------------------------------------------------------------------ */
ZJ_API int zj_abi_version(void);
ZJ_API int zj_device_count(void);                              /* <0: zj_status */
ZJ_API zj_ctx *zj_ctx_create(int backend, int device, int *status);
ZJ_API void zj_ctx_destroy(zj_ctx *ctx);
ZJ_API zj_ctx *zj_default_ctx(void);        /* the calling thread's own lazily created ctx on device 0, for the fn-pointer
                                        shims (the reference calls them from several worker threads at once);
                                        recycled to the next new thread when its thread ends; never destroy it */
ZJ_API const char *zj_strerror(int status);
ZJ_API const char *zj_last_error(const zj_ctx *ctx);           /* detail of the last ZJ_ERR_HIP */

/* ---- strip level: pointer-compatible with the reference's fn types (host buffers) ----------- */
/* IDCTPtr, src/idct/scalar.rs:19 dequantize_and_idct_int(vector, qt_table, stride, samp_factors, v_samp) */
ZJ_API int zj_idct_strip(zj_ctx *ctx, const int16_t *coeff, size_t n, const int32_t qt[64], size_t stride,
                  size_t samp_factors, size_t v_samp, int16_t *out /* n */);
/* UpSampler, src/upsampler/scalar.rs:5 / :64 / :148 (input, output_len) */
ZJ_API int zj_upsample_h(zj_ctx *ctx, const int16_t *in, size_t n, int16_t *out, size_t out_len);
ZJ_API int zj_upsample_v(zj_ctx *ctx, const int16_t *in, size_t n, int16_t *out, size_t out_len);
ZJ_API int zj_upsample_hv(zj_ctx *ctx, const int16_t *in, size_t n, int16_t *out, size_t out_len);
/* ColorConvert16Ptr, src/color_convert/scalar.rs:52 ycbcr_to_rgb_16_scalar(y, cb, cr, output, pos) */
ZJ_API int zj_ycbcr_to_rgb16(zj_ctx *ctx, const int16_t y[16], const int16_t cb[16], const int16_t cr[16],
                      uint8_t *out, size_t out_len, size_t *pos);
/* post_process, src/worker.rs:32.  `out` must be zero-filled by the caller exactly as the
 * reference's callers do (src/mcu.rs:222, src/mcu_prog.rs:176): bytes the reference never writes
 * are left untouched. */
ZJ_API int zj_post_process_strip(zj_ctx *ctx, const int16_t *const coeff[3], const size_t len[3],
                          const zj_component comps[3], int in_cs, int out_cs, uint8_t *out,
                          size_t out_len, size_t width);

/* Function-pointer dispatch mirror of choose_idct_func & friends: returns the HIP arm. */
typedef int (*zj_idct_fn)(zj_ctx *, const int16_t *, size_t, const int32_t *, size_t, size_t, size_t,
                          int16_t *);
typedef int (*zj_upsample_fn)(zj_ctx *, const int16_t *, size_t, int16_t *, size_t);
typedef int (*zj_color_convert16_fn)(zj_ctx *, const int16_t *, const int16_t *, const int16_t *,
                                     uint8_t *, size_t, size_t *);
ZJ_API zj_idct_fn zj_choose_idct_func(int backend);                        /* src/idct.rs:40 */
ZJ_API zj_upsample_fn zj_choose_upsample_func(int backend, int h_max, int v_max); /* decoder.rs:468 */
ZJ_API zj_color_convert16_fn zj_choose_ycbcr_to_rgb_convert_func(int backend, int out_cs); /* color_convert.rs:61 */

/* ---- frame / batch level -------------------------------------------------------------------- */
ZJ_API size_t zj_plane_len(const zj_frame_desc *d, int comp); /* int16 elements; mcu_prog.rs:76 */
ZJ_API size_t zj_out_len(const zj_frame_desc *d);             /* bytes = width*height*ncomp */
ZJ_API int zj_num_components(int colorspace);                 /* misc.rs:113 */

/* Host buffers; H2D copy, fused kernel(s), D2H copy, synchronous.  Output is fully written
 * (including the bytes the reference leaves at their initial 0). */
ZJ_API int zj_decode_planes(zj_ctx *ctx, const zj_frame_desc *d, const int16_t *y, const int16_t *cb,
                     const int16_t *cr, uint8_t *out);
/* nframes frames of identical geometry, planes and outputs contiguous frame after frame. */
ZJ_API int zj_decode_planes_batch(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes, const int16_t *y,
                           const int16_t *cb, const int16_t *cr, uint8_t *out);
/* The same for frames that are INDEPENDENT allocations, the way the reference's callers own them (a fresh Vec per strip,
 * src/mcu.rs:238-250; one Vec<u8> per decode, src/decoder.rs:178): y[f] / cb[f] / cr[f] / out[f] are frame f's host
 * buffers (cb / cr may be NULL for ZJ_CS_GRAYSCALE output).  Same pipeline, one copy per frame and plane. */
ZJ_API int zj_decode_frames(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes, const int16_t *const *y,
                     const int16_t *const *cb, const int16_t *const *cr, uint8_t *const *out);
/* Device-resident variant (kernel-only path used by bench.py): all pointers are device pointers
 * on ctx's device, 16-byte aligned (the pixels of a frame whose width is not a multiple of 16 may start at any byte:
 * its rows do anyway); frames contiguous.  Asynchronous on `stream` (a hipStream_t;
 * NULL = the ctx stream).  The frame's quantisation tables travel by value in the kernel arguments:
 * nothing is uploaded, cached or ordered against other streams. */
ZJ_API int zj_decode_planes_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes,
                            const int16_t *d_y, const int16_t *d_cb, const int16_t *d_cr,
                            uint8_t *d_out, void *stream);
/* Frames at a uniform distance instead of back to back (the images of one tensor with padding, the slots of an arena):
 * y_stride / c_stride in int16 elements (multiples of 8), out_stride in bytes (a multiple of 16); 0 = packed.  ONE launch. */
ZJ_API int zj_decode_planes_device_strided(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes, const int16_t *d_y,
                                    const int16_t *d_cb, const int16_t *d_cr, uint8_t *d_out, size_t y_stride,
                                    size_t c_stride, size_t out_stride, void *stream);
/* Scattered batch: nframes frames of ONE geometry whose planes and pixels are independent device allocations, in any
 * order.  d_y / d_cb / d_cr / d_out are HOST arrays of nframes device pointers (each 16-byte aligned; d_cb / d_cr may be
 * NULL for ZJ_CS_GRAYSCALE output); they are read during the call -- the addresses travel in the kernel arguments, up to
 * ZJ_SCATTER_MAX frames per launch, nothing is staged and nothing has to outlive the call.  Frames that turn out to be
 * equally spaced share one launch whatever their number.  A caller with two or more frames in hand should use this (or a
 * contiguous batch) instead of one launch per frame: a launch of one 4096x4096 frame is 1.3 waves of workgroups and runs
 * at 0.49-0.54 of the HBM peak, a launch of 16 at 0.70.  Asynchronous on `stream`. */
#define ZJ_SCATTER_MAX 32
ZJ_API int zj_decode_frames_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes, const int16_t *const *d_y,
                            const int16_t *const *d_cb, const int16_t *const *d_cr, uint8_t *const *d_out, void *stream);
/* Crop windows (region of interest) of frames left in HBM, for consumers on the GPU (a data loader's random or centre
 * crop).  A crop is EXACTLY the bytes zj_decode_planes_device writes inside the window: crop row r, byte b == full-frame
 * row y + r, byte x * C + b (C = bytes per pixel; CHW: the same per plane with C = 1) -- the zeros of the full decode
 * included (the early RGB tail, ragged rows, the rows below the last complete strip), every flag, colour space and layout.
 * Only the tiles whose bytes the window needs are decoded.  The crop's rows lie out_pitch bytes apart (0 = tight: w * C);
 * the padding between them and everything outside zj_crop_out_len() bytes is never written.  d->out_pitch must be 0 (the
 * crop's pitch is its own argument); an empty window, one that leaves the frame or a pitch below a row is ZJ_ERR_ARG and
 * nothing is launched.
 * zj_crop_out_len: bytes of one crop (out_pitch, 0 = tight, x h; x 3 for CHW); 0 = not a valid window for d.  A
 * single-component d with a colour output (all zeros, as zj_out_len counts them) has crops of that output's size. */
ZJ_API size_t zj_crop_out_len(const zj_frame_desc *d, unsigned crop_w, unsigned crop_h, unsigned out_pitch);
/* nframes frames of ONE geometry, each cut to the crop_w x crop_h window at origins[2f], origins[2f+1]; pointers as in
 * zj_decode_frames_device (host arrays of device pointers; planes 16-byte aligned, outputs at any byte); batches larger
 * than ZJ_SCATTER_MAX are split into several launches.  There is one crop kernel generation: zj_set_variant does not
 * apply.  Asynchronous on `stream`. */
ZJ_API int zj_decode_crops_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes, const int16_t *const *d_y,
                                  const int16_t *const *d_cb, const int16_t *const *d_cr, const unsigned *origins,
                                  unsigned crop_w, unsigned crop_h, uint8_t *const *d_out, unsigned out_pitch, void *stream);
/* Resize + normalise into a dense tensor: images of their own sizes to ONE out_w x out_h (1..8192), bilinear
 * with half-pixel centres (align_corners=False, no antialiasing: strong downscales alias; ZJ_RESIZE_BILINEAR_AA below
 * antialiases), in integer arithmetic with the source position truncated to 1/256 pixel.  Per channel c, v = the interpolated value x 65536 (0 .. 255 x 65536):
 *   ZJ_DTYPE_F32   fl32(fl32(v * (scale[c] / 65536)) + bias[c]), two separately rounded float32 operations;
 *                  scale = 1 / (255 std), bias = -mean / std is (x / 255 - mean) / std, the usual normalisation
 *   ZJ_DTYPE_F16 / ZJ_DTYPE_BF16   that float32 rounded to nearest-even
 *   ZJ_DTYPE_U8    (v + 32768) >> 16 (scale and bias unused)
 * scale / bias: `channels` floats each (NULL: 1 / 0); one that is not finite is ZJ_ERR_ARG.  flip: one byte per image
 * (NULL: none), non-zero mirrors the image's output columns.  The output is [N, C, out_h, out_w] (ZJ_TENSOR_NCHW) or
 * [N, out_h, out_w, C] (ZJ_TENSOR_NHWC) of the dtype, image i at d_out + i * zj_resized_out_len's bytes.  Asynchronous on
 * `stream` (NULL: the context's); nothing is launched after an argument error. */
#define ZJ_DTYPE_F32 0
#define ZJ_DTYPE_F16 1
#define ZJ_DTYPE_BF16 2
#define ZJ_DTYPE_U8 3
#define ZJ_TENSOR_NCHW 0
#define ZJ_TENSOR_NHWC 1
/* bytes of one resized output of a frame of d (channels: 3 for RGB / YCbCr, 1 for GRAYSCALE); 0: not supported (RGBA /
 * RGBX) or not a valid descriptor, size or dtype */
ZJ_API size_t zj_resized_out_len(const zj_frame_desc *d, unsigned out_w, unsigned out_h, int dtype);
/* n u8 images in device memory: d_in[i] its first byte, in_wh[2i], in_wh[2i + 1] its width and height (1..65535),
 * in_pitch[i] the bytes between its rows (NULL or 0: tight); channels 1 or 3, in_layout ZJ_LAYOUT_HWC (interleaved) or
 * ZJ_LAYOUT_CHW (3 planes, pitch x height bytes apart) */
ZJ_API int zj_resize_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_in, const unsigned *in_wh, const unsigned *in_pitch,
                            int channels, int in_layout, unsigned out_w, unsigned out_h, int dtype, int out_layout,
                            const float *scale, const float *bias, const uint8_t *flip, void *d_out, void *stream);
/* crop windows resized: frame f's window windows[4f .. 4f + 3] = x, y, w, h (each its own size, checked as in
 * zj_decode_crops_device) and its output is zj_resize_device applied to EXACTLY the u8 crop zj_decode_crops_device writes
 * for that window, in d's layout.  Planes and pointers as zj_decode_crops_device; RGBA / RGBX outputs are
 * ZJ_ERR_UNSUPPORTED.  The crops pass through a device buffer of the context (launch groups of at most 256 MB of crops),
 * whose reuse is ordered on the caller's stream.  Asynchronous on `stream`. */
ZJ_API int zj_decode_crops_resized_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes, const int16_t *const *d_y,
                                          const int16_t *const *d_cb, const int16_t *const *d_cr, const unsigned *windows,
                                          unsigned out_w, unsigned out_h, int dtype, int out_layout, const float *scale,
                                          const float *bias, const uint8_t *flip, void *d_out, void *stream);
/* Crop windows straight into a normalised tensor, NOT resized: a RandomCrop / CenterCrop at native
 * resolution, a segmentation or detection crop, a whole frame.  d: out_colorspace RGB / YCbCr (C = 3) or GRAYSCALE (C = 1),
 * out_layout ZJ_LAYOUT_HWC and out_pitch 0 (the tensor's layout is the call's; anything else, RGBA / RGBX included, is
 * ZJ_ERR_UNSUPPORTED).  Frame f's window is crop_w x crop_h at origins[2f], origins[2f + 1], checked as in
 * zj_decode_crops_device.  With p[r][i][c] the byte zj_decode_crops_device writes for that window (its zeros included), the
 * element of image f, channel c, row r, column (flip[f] ? crop_w - 1 - i : i) is the conversion above of v = p << 16:
 * ZJ_DTYPE_F32 fl32(fl32(v * (scale[c] / 65536)) + bias[c]), F16 / BF16 its nearest-even rounding, U8 the byte itself.  A
 * zero byte therefore becomes bias[c].  For crop_w, crop_h <= 8192 this is, byte for byte, zj_decode_crops_resized_device
 * with out_w = crop_w, out_h = crop_h -- written once by one launch, with no buffer of the context in between, no ordering
 * events and no 8192 limit.  dtype, out_layout, scale, bias, flip as zj_resize_device; image f lies at d_out + f *
 * zj_crop_tensor_out_len() bytes, d_out aligned to the element.  Batches larger than ZJ_SCATTER_MAX are split into several
 * launches.  Asynchronous on `stream`; nothing is launched after an error.
 * Frames of several geometries: zj_decode_crops_tensor_mixed_device below.  A decoder's file, several decoders' files:
 * zj_decoder_finish_pixels_crop_tensor_device, zj_decoder_finish_pixels_crop_tensor_batch_device.  d->flags takes what
 * zj_decode_crops_device takes: a one-component frame shown as RGB or a turned one is made of the u8 crop and
 * zj_to_tensor_device below (the decoder's file calls do that); a prescale is the resized-crop calls'.  The launch's
 * arguments pass through a small table of the context (a few KB per 32 frames), whose reuse is ordered on the caller's stream.
 * zj_crop_tensor_out_len: C * w * h * the element's bytes; 0: not a valid window / dtype for d, or d has no tensor. */
ZJ_API size_t zj_crop_tensor_out_len(const zj_frame_desc *d, unsigned w, unsigned h, int dtype);
ZJ_API int zj_decode_crops_tensor_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes, const int16_t *const *d_y,
                                         const int16_t *const *d_cb, const int16_t *const *d_cr, const unsigned *origins,
                                         unsigned crop_w, unsigned crop_h, int dtype, int out_layout, const float *scale,
                                         const float *bias, const uint8_t *flip, void *d_out, void *stream);
/* ... of frames of MIXED geometry: descs[f] is frame f's own descriptor (size, sampling, tables, flags, in_components);
 * out_colorspace and out_layout must be the same in all (ZJ_ERR_ARG otherwise); every window crop_w x crop_h.  Image f is
 * byte for byte zj_decode_crops_tensor_device's for frame f alone.  Every frame is checked before anything is launched: the
 * status is that call's for the first failing frame, and then nothing is written.  One launch per sampling mode. */
ZJ_API int zj_decode_crops_tensor_mixed_device(zj_ctx *ctx, const zj_frame_desc *descs, size_t nframes,
                                               const int16_t *const *d_y, const int16_t *const *d_cb,
                                               const int16_t *const *d_cr, const unsigned *origins, unsigned crop_w,
                                               unsigned crop_h, int dtype, int out_layout, const float *scale,
                                               const float *bias, const uint8_t *flip, void *d_out, void *stream);
/* u8 images in device memory into one normalised tensor, NOT resized: the last stage of the crop-tensor file
 * calls for the files whose u8 image is made by stages of its own (gray shown as RGB, CMYK, another sampling, a turned
 * file), and a call of its own.  n images of ONE size w x h (1..65535 each; no 8192 limit), interleaved, in_channels 1 or
 * 3; image f starts at d_in[f], in_pitch[f] bytes between its rows (NULL or 0: tight; below w * in_channels: ZJ_ERR_ARG).
 * channels: of the tensor, 1 or 3; in_channels 1 with channels 3 replicates the byte into the three channels, each with its
 * own scale[c], bias[c]; in_channels 3 with channels 1 is ZJ_ERR_ARG.  With p the byte of image f, row r, column i, channel
 * c, the element (c, r, flip[f] ? w - 1 - i : i) of image f is the conversion of v = p << 16 defined at zj_resize_device: for
 * w, h <= 8192 and in_channels == channels the output is byte for byte zj_resize_device's with out_w = w, out_h = h and
 * ZJ_LAYOUT_HWC input.  Image f lies at d_out + f * channels * w * h * the element's bytes; d_out aligned to the element.
 * dtype, out_layout, scale, bias, flip and their checks as zj_resize_device; n == 0 or a NULL pointer is ZJ_ERR_ARG.  ONE
 * kernel, up to 128 images per launch; no byte outside an image's own h rows of w * in_channels bytes is read.
 * Asynchronous on `stream` (NULL: the context's); nothing is launched after an error. */
ZJ_API int zj_to_tensor_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_in, unsigned w, unsigned h,
                               const unsigned *in_pitch, int in_channels, int channels, int dtype, int out_layout,
                               const float *scale, const float *bias, const uint8_t *flip, void *d_out, void *stream);
/* Affine-warped images into one normalised tensor: rotation, shear, scale, translation, the letterbox, any
 * crop whose window leaves the image.  A matrix m = (a, b, c, d, e, f) of doubles maps an output pixel CENTRE to continuous
 * source coordinates, pixel i covering [i, i + 1): sx = a (X + 1/2) + b (Y + 1/2) + c, sy = d (X + 1/2) + e (Y + 1/2) + f.
 * zj_warp_fixed gives its six integers, Q = 24: A = floor(a 2^24 + 1/2), B, D, E likewise, C0 = floor((a / 2 + b / 2 + c -
 * 1/2) 2^24 + 1/2), F0 likewise from d, e, f (the sums formed in doubles, from left to right); ZJ_ERR_ARG: a non-finite
 * entry, |a|, |b|, |d|, |e| >= 128 or |c|, |f| >= 2^31.  In 64-bit integers Ux = A X + B Y + C0, ux = Ux >> 16 (a floor: 1/256
 * pixel), x0 = ux >> 8, fx = ux & 255, and Uy, y0, fy likewise.  The four taps are (y0, x0), (y0, x0 + 1), (y0 + 1, x0),
 * (y0 + 1, x0 + 1).  edge ZJ_WARP_FILL: a tap with x outside [0, w) or y outside [0, h) reads fill[c], a byte per output
 * channel (NULL: 0); ZJ_WARP_REPLICATE: the tap's indices are clamped to the image.  The value is zj_resize_device's
 * v = top (256 - fy) + bot fy over those taps, the element its conversion of v.  There is no flip: a mirror is a matrix.
 * The identity gives zj_to_tensor_device byte for byte, the integer matrix of an EXIF orientation the displayed image's, a
 * scale by 2, 4, 1/2 or 1/4 per axis with ZJ_WARP_REPLICATE zj_resize_device's.  Nothing is antialiased.
 * zj_warp_source_window: the window x, y, w, h of a frame of frame_w x frame_h that an out_w x out_h output under `fixed`
 * can read -- U is affine, so the box of the taps is spanned by the output's four corner pixels -- and `shifted`, the
 * integers relative to it (C0 - x 2^24, F0 - y 2^24).  ZJ_WARP_FILL: the box cut to the frame; an empty cut gives w = h = 0
 * and the output is all fill.  ZJ_WARP_REPLICATE: both ends of the box clamped into the frame.  In both modes warping the
 * window's crop under `shifted` equals warping the whole frame under `fixed`.  ZJ_ERR_ARG: a NULL pointer, integers no
 * matrix gives, a size outside 1..65535 (frame) or 1..8192 (output), another edge.  Both functions run without a device. */
#define ZJ_WARP_FILL 0
#define ZJ_WARP_REPLICATE 1
ZJ_API int zj_warp_fixed(const double matrix[6], int64_t fixed[6]);
ZJ_API int zj_warp_source_window(const int64_t fixed[6], unsigned frame_w, unsigned frame_h, unsigned out_w, unsigned out_h,
                                 int edge, unsigned window[4], int64_t shifted[6]);
/* n u8 images in device memory, interleaved, channels 1 or 3, each under its own matrix (matrices: 6 doubles per image): d_in,
 * in_wh, in_pitch as in zj_resize_device (ZJ_LAYOUT_HWC alone); out_w, out_h, dtype, out_layout, scale, bias and their
 * checks as there too, d_out aligned to the element; image f lies at d_out + f * channels * out_w * out_h * the element's
 * bytes (zj_resized_out_len).  ZJ_ERR_ARG as well: a matrix zj_warp_fixed refuses, another edge.  One kernel per channel
 * count, up to 48 images per launch; a tap outside an image is never loaded and no byte outside an image's own h rows of
 * w * channels bytes is read.  Asynchronous on `stream` (NULL: the context's); nothing is launched after an error. */
ZJ_API int zj_warp_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_in, const unsigned *in_wh, const unsigned *in_pitch,
                          int channels, const double *matrices, unsigned out_w, unsigned out_h, int dtype, int out_layout,
                          const float *scale, const float *bias, const uint8_t *fill, int edge, void *d_out, void *stream);
/* nframes frames of ONE geometry, frame f warped under matrices[6f .. 6f + 5], given in FRAME pixels: the output is by
 * definition zj_warp_device applied to EXACTLY the bytes zj_decode_crops_device writes for the whole frame (its zeros and
 * ZJ_FLAG_CORRECTED included).  Only each frame's source window (zj_warp_source_window) is decoded, by the crop stage into
 * the context's buffer in the launch groups of zj_decode_crops_resized_device and under its ordering; a frame whose output
 * sees nothing of the frame decodes nothing.  d and its refusals as in zj_decode_crops_resized_device (ZJ_FLAG_GRAY_TO_RGB
 * included), out_layout ZJ_LAYOUT_HWC; the tail as zj_warp_device.  Asynchronous on `stream`; nothing is launched after an
 * error. */
ZJ_API int zj_decode_crops_warped_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes, const int16_t *const *d_y,
                                         const int16_t *const *d_cb, const int16_t *const *d_cr, const double *matrices,
                                         unsigned out_w, unsigned out_h, int dtype, int out_layout, const float *scale,
                                         const float *bias, const uint8_t *fill, int edge, void *d_out, void *stream);
/* Resize filters of the *_filtered_device entry points:
 *   ZJ_RESIZE_BILINEAR     the bilinear definition above: the entry points without a filter, byte for byte
 *   ZJ_RESIZE_BILINEAR_AA  antialiased: the triangle filter of Pillow's bilinear / F.interpolate(antialias=True), in exact
 *                          integers.  Every source pixel under an output's support contributes, with weights in units of
 *                          2^-14 that sum to exactly 2^14 per output; the vertical pass runs first and rounds its sums to
 *                          1/256, the horizontal pass gives the same v (0 .. 255 x 65536) the conversions above take.  A
 *                          window of exactly out_w x out_h gives the crop itself, as the bilinear filter does.
 *   ZJ_RESIZE_BICUBIC_AA   antialiased bicubic: Keys' cubic with a = -1/2 over a support of 2 max(1, n / m) source pixels
 *                          each side, the filter of Pillow's BICUBIC / F.interpolate(mode="bicubic", antialias=True), in
 *                          exact integers.  The weights (units of 2^-14, some negative) sum to exactly 2^14 per output; the
 *                          vertical pass runs first and keeps its signed sums in 1/256 unclamped, the horizontal pass's v is
 *                          clamped to 0 .. 255 x 65536 and goes through the conversions above.  A window of exactly
 *                          out_w x out_h gives the crop itself.  No limit on the downscale ratio.  The same argument checks,
 *                          in the same order, as ZJ_RESIZE_BILINEAR_AA.  (The values 2 and 3 are not filters.)
 * Any other filter is ZJ_ERR_ARG and nothing is launched.  The other arguments are those of the entry point without a
 * filter. */
#define ZJ_RESIZE_BILINEAR 0
#define ZJ_RESIZE_BILINEAR_AA 1
#define ZJ_RESIZE_BICUBIC_AA 4
ZJ_API int zj_resize_filtered_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_in, const unsigned *in_wh,
                                     const unsigned *in_pitch, int channels, int in_layout, unsigned out_w, unsigned out_h,
                                     int dtype, int out_layout, const float *scale, const float *bias, const uint8_t *flip,
                                     int filter, void *d_out, void *stream);
ZJ_API int zj_decode_crops_resized_filtered_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes,
                                                   const int16_t *const *d_y, const int16_t *const *d_cb,
                                                   const int16_t *const *d_cr, const unsigned *windows, unsigned out_w,
                                                   unsigned out_h, int dtype, int out_layout, const float *scale,
                                                   const float *bias, const uint8_t *flip, int filter, void *d_out,
                                                   void *stream);
/* Reduced-size decode: the frame at 1/2, 1/4 or 1/8 of its size per axis (scale_log2 = 1, 2, 3; anything else
 * is ZJ_ERR_ARG), straight from the coefficient planes -- libjpeg's scale_num / scale_denom, Pillow's Image.draft.  The
 * reduced frame is ceil(width / s) x ceil(height / s).  Per component and axis a block yields N = min(8, (8 / s) x (f_max /
 * f_c)) samples, each the mean of 8 / N consecutive outputs of the exact 8-point IDCT, taken before rounding, then rounded to
 * nearest and clamped to 0..255 (tests/scaled_model.py is the definition, bit for bit).  Every component lands on the reduced
 * grid, so chroma is never up-sampled; a component with N = 8 on both axes (chroma of 4:2:0 at 1/2) takes the full decode's
 * block transform as it is.  Colour is the full decode's per-pixel arithmetic; every pixel of the reduced frame is written at
 * its place (no early tail, no zero columns or rows).  Of zj_frame_desc.flags only ZJ_FLAG_CLAMP_DC has an effect, and only
 * on the components that take the full transform; the other flags have none.  Outputs: RGB, GRAYSCALE, YCbCr, HWC or CHW;
 * RGBA / RGBX are ZJ_ERR_UNSUPPORTED.  A single-component d with a colour output is zeros of that output's size, as for
 * zj_crop_out_len.  d->out_pitch must be 0.
 * zj_scaled_size: the reduced frame.  zj_scaled_crop_out_len: bytes of a w x h window of it whose rows lie out_pitch bytes
 * apart (0 = tight; x 3 planes for CHW); 0 = not a valid size for d. */
ZJ_API int zj_scaled_size(const zj_frame_desc *d, int scale_log2, unsigned *w, unsigned *h);
ZJ_API size_t zj_scaled_crop_out_len(const zj_frame_desc *d, int scale_log2, unsigned w, unsigned h, unsigned out_pitch);
/* nframes frames of ONE geometry, frame f cut to the window windows[4f .. 4f + 3] = x, y, w, h in REDUCED pixels (windows ==
 * NULL: the whole reduced frame); only the blocks a window touches are read.  Each crop is tight (out_pitch 0) or has its
 * rows out_pitch bytes apart; what lies outside a window's rows, the pitch padding included, is never written.  Pointers as
 * in zj_decode_crops_device; batches larger than ZJ_SCATTER_MAX are split into several launches.  A scale outside 1..3, an
 * empty window, one that leaves the reduced frame, a pitch below a row or d->out_pitch != 0 is ZJ_ERR_ARG and nothing is
 * launched.  Asynchronous on `stream`. */
ZJ_API int zj_decode_crops_scaled_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes, const int16_t *const *d_y,
                                         const int16_t *const *d_cb, const int16_t *const *d_cr, int scale_log2,
                                         const unsigned *windows, uint8_t *const *d_out, unsigned out_pitch, void *stream);
/* zj_decode_crops_resized_filtered_device with a reduced-size decode under the resize: windows stay in FULL-resolution
 * pixels; max_prescale_log2 = 0..3 (else ZJ_ERR_ARG).  Per image, s is the largest power of two <= 2^max_prescale_log2 with
 * floor(w / s) >= out_w and floor(h / s) >= out_h, so the resize never enlarges.  An image with s = 1 is decoded and resized
 * exactly as before.  Otherwise the output is the resize (`filter`) of the reduced crop (zj_decode_crops_scaled_device at
 * log2 s) at the window [floor(x / s), ceil((x + w) / s)) x [floor(y / s), ceil((y + h) / s)), clipped to the reduced
 * frame.  This is the one place where prescaling changes geometry: that window covers the requested one and exceeds it by
 * less than s source pixels per side, which -- because w >= s x out_w -- is less than one output pixel's footprint.
 * max_prescale_log2 = 0 is zj_decode_crops_resized_filtered_device byte for byte. */
ZJ_API int zj_decode_crops_resized_prescaled_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes,
                                                    const int16_t *const *d_y, const int16_t *const *d_cb,
                                                    const int16_t *const *d_cr, const unsigned *windows, unsigned out_w,
                                                    unsigned out_h, int dtype, int out_layout, const float *scale,
                                                    const float *bias, const uint8_t *flip, int filter,
                                                    int max_prescale_log2, void *d_out, void *stream);
/* EXIF orientation.  o = 1..8 is the Orientation tag; S the stored image, h rows of w pixels -- what the decode
 * writes, quirks included -- and D the displayed one:
 *   o  size of D   D[r][c]               o  size of D   D[r][c]
 *   1  h x w       S[r][c]               5  w x h       S[c][r]
 *   2  h x w       S[r][w-1-c]           6  w x h       S[h-1-c][r]
 *   3  h x w       S[h-1-r][w-1-c]       7  w x h       S[h-1-c][w-1-r]
 *   4  h x w       S[h-1-r][c]           8  w x h       S[c][w-1-r]
 * (Pillow's FLIP_LEFT_RIGHT, ROTATE_180, FLIP_TOP_BOTTOM, TRANSPOSE, ROTATE_270, TRANSVERSE, ROTATE_90 for 2..8:
 * ImageOps.exif_transpose.)  A pixel moves as a whole, its bytes keep their order;
 * ZJ_LAYOUT_CHW: every plane is turned on its own.
 * zj_oriented_size: the size of D.  zj_orient_window: the window x, y, w, h of D, given for a stored frame of frame_w x
 * frame_h, as the window of S whose displayed form is exactly D[y : y + h, x : x + w].  ZJ_ERR_ARG: an orientation outside
 * 1..8; zj_orient_window also: an empty window or one that leaves D. */
ZJ_API int zj_oriented_size(int orientation, unsigned w, unsigned h, unsigned *ow, unsigned *oh);
ZJ_API int zj_orient_window(int orientation, unsigned frame_w, unsigned frame_h, const unsigned window[4], unsigned stored[4]);
/* n u8 images in device memory -> their displayed form: d_in, in_wh (STORED width and height, 1..65535), in_pitch, channels and
 * in_layout as in zj_resize_device; orientation[i] = 1..8 (NULL: all 1, a plain copy); d_out[i] the first byte of image i's
 * output, in the same layout, its rows out_pitch[i] bytes apart (NULL or 0: tight; the padding is never written; CHW: the
 * planes lie out_pitch x displayed height apart).  An image's input and output must not overlap.  One launch per 128 images,
 * whatever their sizes.  Asynchronous on `stream` (NULL: the context's); nothing is launched after an argument error. */
ZJ_API int zj_orient_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_in, const unsigned *in_wh, const unsigned *in_pitch,
                            int channels, int in_layout, const uint8_t *orientation, uint8_t *const *d_out,
                            const unsigned *out_pitch, void *stream);
/* n u8 planes in device memory -> 3-channel u8 images with every channel equal to the plane: d_in, in_wh
 * (width and height, 1..65535) and in_pitch as in zj_orient_device; out_layout ZJ_LAYOUT_HWC (pixels g g g) or ZJ_LAYOUT_CHW
 * (three planes, out_pitch x height apart); d_out[i] the first byte of image i's output, its rows out_pitch[i] bytes apart
 * (NULL or 0: tight, 3 x width bytes for HWC and width bytes for CHW; the padding is never written).  Any addresses and
 * pitches; an image's input and output must not overlap.  One launch per 128 images, whatever their sizes.  Asynchronous on
 * `stream` (NULL: the context's); nothing is launched after an argument error. */
ZJ_API int zj_gray_to_rgb_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_in, const unsigned *in_wh, const unsigned *in_pitch,
                                 int out_layout, uint8_t *const *d_out, const unsigned *out_pitch, void *stream);
/* n 3-channel u8 images a and n u8 planes k of the same sizes, in device memory -> 3-channel u8 images with
 * out[c] = (a[c] * k + 127) / 255 (integer division): Pillow's CMYK -> RGB on complemented samples.
 * inverted[i] (NULL: all 0) non-zero: image i's samples are used as stored (an Adobe file, whose samples are complemented
 * already); 0: a and k are complemented (x ^ 255) first.  in_wh (width and height, 1..65535); `layout` of a and of the output,
 * ZJ_LAYOUT_HWC or ZJ_LAYOUT_CHW (three planes, pitch x height apart); a_pitch, k_pitch, out_pitch bytes between rows (NULL or
 * 0: tight; the padding is never read or written).  Any addresses and pitches.  d_out[i] == d_a[i] with equal pitches is
 * allowed (a lane reads its run before it writes it); any other overlap of an output with an input is the caller's error.
 * One launch per 96 images (40 bytes of kernel arguments each), whatever their sizes.  Asynchronous on `stream` (NULL: the
 * context's); nothing is launched after an argument error. */
ZJ_API int zj_cmyk_to_rgb_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_a, const uint8_t *const *d_k, const unsigned *in_wh,
                                 const unsigned *a_pitch, const unsigned *k_pitch, int layout, const uint8_t *inverted,
                                 uint8_t *const *d_out, const unsigned *out_pitch, void *stream);
/* n images from three u8 component planes each, in device memory, every plane at its own resolution:
 * out[r][c] = colour(p0[r / ry0][c / rx0], p1[r / ry1][c / rx1], p2[r / ry2][c / rx2]), integer divisions (box replication);
 * colour is the full decode's per-pixel YCbCr -> RGB, or with stored_rgb != 0 the identity (the planes are R, G, B).
 * in_wh: width and height of each OUTPUT (1..65535); ratios: six bytes per image, rx0 ry0 rx1 ry1 rx2 ry2, each 1, 2 or 4
 * (anything else: ZJ_ERR_ARG); plane k of an image is ceil(w / rx_k) x ceil(h / ry_k) samples; pitches: three per image, bytes
 * between a plane's rows (NULL or 0: tight); `layout` of the output, ZJ_LAYOUT_HWC or ZJ_LAYOUT_CHW (three planes, pitch x
 * height apart); out_pitch (NULL or 0: tight).  Any addresses and pitches; no byte outside a plane's samples is read, no padding
 * is written.  An output must not overlap a plane.  One launch per 72 images (56 bytes of kernel arguments each), whatever
 * their sizes.  Asynchronous on `stream` (NULL: the context's); nothing is launched after an argument error. */
ZJ_API int zj_planes_to_rgb_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_p0, const uint8_t *const *d_p1,
                                   const uint8_t *const *d_p2, const unsigned *in_wh, const uint8_t *ratios, const unsigned *pitches,
                                   int stored_rgb, int layout, uint8_t *const *d_out, const unsigned *out_pitch, void *stream);
/* zj_decode_crops_resized_prescaled_device for frames that are to be shown turned: orientation[f] = 1..8 per frame (NULL: all
 * 1, and the call IS the prescaled one), windows in DISPLAYED pixels of each frame.  The output is zj_resize_filtered_device
 * applied to EXACTLY the displayed form of the u8 crop zj_decode_crops_device writes for the stored window (zj_orient_window)
 * -- the reference's quirks turn with the image; with prescaling, of the reduced crop of that stored window, the scale picked
 * from the displayed window's sides.  Orientation comes first: `flip` still mirrors the output's columns after everything
 * else.  Frames with orientation 1 skip the orient stage; the others pass through a second region of the context's buffer.
 * An orientation outside 1..8 or a window that leaves the displayed frame is ZJ_ERR_ARG and nothing is launched. */
ZJ_API int zj_decode_crops_resized_oriented_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes,
                                                   const int16_t *const *d_y, const int16_t *const *d_cb,
                                                   const int16_t *const *d_cr, const unsigned *windows, unsigned out_w,
                                                   unsigned out_h, int dtype, int out_layout, const float *scale,
                                                   const float *bias, const uint8_t *flip, int filter,
                                                   int max_prescale_log2, const uint8_t *orientation, void *d_out,
                                                   void *stream);
/* ---- frames of MIXED geometry into one resized-crop tensor ---------------------------------------------
 * zj_decode_crops_resized_oriented_device for frames that each bring their own descriptor: frame f is described by descs[f].
 * Width and height, h_max and v_max, the quantisation tables, flags and in_components may differ per frame; out_colorspace
 * and out_layout must be the same in all descriptors (ZJ_ERR_ARG otherwise) and out_pitch 0.
 * DEFINITION: image f of the output equals, byte for byte, what zj_decode_crops_resized_oriented_device(ctx, &descs[f], 1, ...)
 * writes for that frame alone, with the same window, filter, prescale, orientation and flip.
 * All frames are checked before anything is launched; on a failed check the call returns the status the single-frame call
 * would return for the first failing frame and launches nothing.  The crops pass through the context's buffer in groups, as
 * in the one-geometry call; per group the crop stage is at most one launch per sampling mode present, one reduced-decode
 * launch per (sampling mode, scale) present and one launch for the rows below the frames' last complete strips -- the
 * frames' geometry travels in a table in device memory that the call uploads on `stream` -- then the orient and resize
 * launches, one per 128 images.  Not limited to ZJ_SCATTER_MAX frames per launch.  Asynchronous on `stream` (NULL: the
 * context's). */
ZJ_API int zj_decode_crops_resized_mixed_device(zj_ctx *ctx, const zj_frame_desc *descs /* [nframes] */, size_t nframes,
                                                const int16_t *const *d_y, const int16_t *const *d_cb,
                                                const int16_t *const *d_cr, const unsigned *windows, unsigned out_w,
                                                unsigned out_h, int dtype, int out_layout, const float *scale,
                                                const float *bias, const uint8_t *flip, int filter, int max_prescale_log2,
                                                const uint8_t *orientation, void *d_out, void *stream);
/* ---- colour matrices: brightness, contrast, saturation, hue, grayscale, a channel order -----------------
 * A colour matrix is 12 doubles, m[4c + k]: m[c][0..2] multiply R, G, B in output channel c, m[c][3] is an offset in grey
 * levels.  zj_color_fixed gives its 12 integers, q = floor(m 65536 + 1/2) evaluated in doubles, and refuses (ZJ_ERR_ARG) a NULL
 * pointer, an entry that is not finite, |m[c][0..2]| > 16 and |m[c][3]| > 4096.  Runs without a device.
 * DEFINITION, for a pixel of bytes (R, G, B):  v = q[c][0] R + q[c][1] G + q[c][2] B + q[c][3],
 * out[c] = clamp((v + 32768) >> 16, 0, 255) with an arithmetic shift; |v| < 2^31 under the limits above.  The identity gives
 * the input bytes, a permutation matrix the permuted bytes, three rows (0.299, 0.587, 0.114, 0) Pillow's convert("L"). */
ZJ_API int zj_color_fixed(const double matrix[12], int32_t fixed[12]);
/* n 3-channel u8 images in device memory, each of its own size and under its own matrix (matrices: 12 doubles per image) ->
 * 3-channel u8 images of the same sizes by the definition above.  in_wh (width and height, 1..65535); `layout` of the input
 * and of the output, ZJ_LAYOUT_HWC or ZJ_LAYOUT_CHW (three planes, pitch x height apart); in_pitch, out_pitch bytes between
 * rows (NULL or 0: tight; the padding is never read or written).  Any addresses and pitches.  d_out[i] == d_in[i] with equal
 * pitches is allowed (a lane reads its run before it writes it); any other overlap of an output with an input is the
 * caller's error.  One launch per 48 images (76 bytes of kernel arguments each), whatever their sizes.  Asynchronous on
 * `stream` (NULL: the context's); every argument, the matrices included, is checked first and nothing is launched after an
 * error. */
ZJ_API int zj_color_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_in, const unsigned *in_wh, const unsigned *in_pitch,
                           int layout, const double *matrices /* 12 per image */, uint8_t *const *d_out,
                           const unsigned *out_pitch, void *stream);
/* zj_decode_crops_resized_mixed_device with frame f's image under the matrix color[12f .. 12f + 11] in front of the resize.
 * DEFINITION: image f equals zj_resize_filtered_device applied to zj_color_device of EXACTLY the u8 image the call without
 * `color` resizes -- after the crop or reduced decode, the turn and the gray expand, in place in the context's buffer.  The
 * flip, the filter and the normalisation are untouched.  color NULL: the call IS zj_decode_crops_resized_mixed_device, byte
 * for byte and launch for launch; frames whose integers are the identity's are left out of the colour launch (one per 48
 * frames of a group).  All matrices are checked before anything is launched (ZJ_ERR_ARG: one zj_color_fixed refuses).  The
 * output colour space must have three components: ZJ_CS_GRAYSCALE with a non-NULL color is ZJ_ERR_UNSUPPORTED. */
ZJ_API int zj_decode_crops_resized_mixed_colored_device(zj_ctx *ctx, const zj_frame_desc *descs /* [nframes] */, size_t nframes,
                                                        const int16_t *const *d_y, const int16_t *const *d_cb,
                                                        const int16_t *const *d_cr, const unsigned *windows, unsigned out_w,
                                                        unsigned out_h, int dtype, int out_layout, const float *scale,
                                                        const float *bias, const uint8_t *flip, int filter,
                                                        int max_prescale_log2, const uint8_t *orientation,
                                                        const double *color /* 12 per frame, or NULL */, void *d_out,
                                                        void *stream);
/* ---- tone curves: invert, posterize, solarize, autocontrast, equalize, a caller's own table -------------
 * A tone op is two int32, `op` and `param`, applied per channel to 1-channel or 3-channel u8 images.  Every table is byte for
 * byte Pillow's ImageOps (invert, posterize, solarize, autocontrast with cutoff 0 and no ignore / mask / preserve_tone,
 * equalize without a mask).  The table t[0..255] of a channel with bins h[0..255]:
 *   ZJ_TONE_IDENTITY      param 0               t[i] = i
 *   ZJ_TONE_INVERT        param 0               t[i] = 255 - i
 *   ZJ_TONE_POSTERIZE     param bits 1..8       t[i] = i & ~(2^(8 - bits) - 1)
 *   ZJ_TONE_SOLARIZE      param threshold 0..256   t[i] = i < threshold ? i : 255 - i
 *   ZJ_TONE_AUTOCONTRAST  param 0   lo, hi = the first and the last non-empty bin; hi <= lo: the identity; else
 *                         scale = 255.0 / (hi - lo), offset = -lo * scale, t[i] = clamp((int)(i * scale + offset), 0, 255) in IEEE
 *                         doubles, the product and the sum rounded separately, the conversion toward zero
 *   ZJ_TONE_EQUALIZE      param 0   at most one non-empty bin: the identity; step = (sum of h - h[hi]) / 255 (integers); step 0:
 *                         the identity; else n = step / 2, and for i = 0..255: t[i] = min(n / step, 255), n += h[i] (n in 64 bits)
 * Any other (op, param) is ZJ_ERR_ARG, checked for all images before anything is launched. */
#define ZJ_TONE_IDENTITY 0
#define ZJ_TONE_INVERT 1
#define ZJ_TONE_POSTERIZE 2
#define ZJ_TONE_SOLARIZE 3
#define ZJ_TONE_AUTOCONTRAST 4
#define ZJ_TONE_EQUALIZE 5
/* The histograms of n u8 images in device memory, each of its own size: d_hist[i][c][v] (unsigned [n][channels][256]: 32-bit
 * counters in device memory, 4-byte aligned) = the pixels of image i whose channel c is v.  The table is overwritten: zeroed on the stream in
 * front of the kernel.  channels 1 or 3; `layout` ZJ_LAYOUT_HWC or ZJ_LAYOUT_CHW (three planes, pitch x height apart; one
 * channel: either); in_wh (width and height, 1..65535); in_pitch bytes between rows (NULL or 0: tight, up to 2^24; the padding
 * is never read and never counted).  Any addresses and pitches.  Integer sums through atomics: the result does not depend on
 * the order of arrival.  One launch per 128 images.  Asynchronous on `stream` (NULL: the context's). */
ZJ_API int zj_histogram_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_in, const unsigned *in_wh, const unsigned *in_pitch,
                               int channels, int layout, unsigned *d_hist, void *stream);
/* The tables of n ops (host memory, op and param per image): d_luts[i][c][.] (uint8 [n][channels][256], device memory) from
 * ops[2i], ops[2i + 1] and, for ZJ_TONE_AUTOCONTRAST and ZJ_TONE_EQUALIZE, the bins d_hist[i][c][.] (as zj_histogram_device
 * leaves them; NULL when no op needs them, ZJ_ERR_ARG when one does).  The ops travel in the kernel arguments, 256 images per
 * launch; nothing comes back to the host.  Asynchronous on `stream`. */
ZJ_API int zj_tone_luts_device(zj_ctx *ctx, size_t n, int channels, const int32_t *ops /* 2 per image */, const unsigned *d_hist,
                               uint8_t *d_luts, void *stream);
/* n u8 images through their own tables: out[c] = d_luts[i][c][in[c]] (uint8 [n][channels][256], device memory: what
 * zj_tone_luts_device wrote, or the caller's own -- gamma, any tone curve).  Sizes, layout and pitches as zj_histogram_device;
 * d_out[i] == d_in[i] with equal pitches is allowed (a lane reads its run before it writes it); any other overlap of an
 * output with an input is the caller's error.  One launch per 128 images.  Asynchronous on `stream`. */
ZJ_API int zj_lut_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_in, const unsigned *in_wh, const unsigned *in_pitch,
                         int channels, int layout, const uint8_t *d_luts, uint8_t *const *d_out, const unsigned *out_pitch,
                         void *stream);
/* n u8 images each under its own op: zj_histogram_device of the images whose op needs one, zj_tone_luts_device,
 * zj_lut_device, all on `stream` with the histograms and tables in the context's own buffer -- the kernel boundaries are the
 * only ordering, nothing is synchronised.  A ZJ_TONE_IDENTITY image that is its own output (same address, same pitch) is left
 * out of every launch, and a call of such images alone launches nothing; with a separate output it is copied (the lookup
 * under the identity table).  The context's buffer holds channels x 1280 bytes for EVERY image of the launches (bins and
 * table, also where the op needs no bins): 3840 bytes an RGB image, about 4 GB at the 2^20 images a call may have. */
ZJ_API int zj_tone_device(zj_ctx *ctx, size_t n, const uint8_t *const *d_in, const unsigned *in_wh, const unsigned *in_pitch,
                          int channels, int layout, const int32_t *ops /* 2 per image */, uint8_t *const *d_out,
                          const unsigned *out_pitch, void *stream);
/* zj_decode_crops_resized_mixed_colored_device with frame f's image under the tone op tone[2f], tone[2f + 1] behind the
 * colour matrix and in front of the resize.  DEFINITION: image f equals zj_resize_filtered_device applied to zj_tone_device
 * of EXACTLY the u8 image the call without `tone` resizes -- after the crop or reduced decode, the turn, the gray expand and,
 * if `color` is given, the colour matrix -- in place in the context's buffer.  The order is fixed, colour first, then tone;
 * another order is the stages' to build.  The histogram is that of the CROP the resize reads, not of the whole file: Pillow
 * on the crop is the reference.  tone NULL: the call IS zj_decode_crops_resized_mixed_colored_device, byte for byte and launch
 * for launch; ZJ_TONE_IDENTITY frames are left out of the tone launches.  All ops are checked before anything is launched
 * (ZJ_ERR_ARG).  A ZJ_CS_GRAYSCALE output takes a tone op as its one channel; only a non-NULL color stays
 * ZJ_ERR_UNSUPPORTED there. */
ZJ_API int zj_decode_crops_resized_mixed_toned_device(zj_ctx *ctx, const zj_frame_desc *descs /* [nframes] */, size_t nframes,
                                                      const int16_t *const *d_y, const int16_t *const *d_cb,
                                                      const int16_t *const *d_cr, const unsigned *windows, unsigned out_w,
                                                      unsigned out_h, int dtype, int out_layout, const float *scale,
                                                      const float *bias, const uint8_t *flip, int filter, int max_prescale_log2,
                                                      const uint8_t *orientation, const double *color /* 12 per frame, or NULL */,
                                                      const int32_t *tone /* 2 per frame, or NULL */, void *d_out, void *stream);
/* Times zj_decode_planes_device with HIP events recorded on the launch stream: *ms_total = `iters`
 * back-to-back launches between one event pair; *ms_each (optional) = mean over `iters` launches
 * each bracketed by its own event pair; *kernel_name = the dominant kernel. */
ZJ_API int zj_time_decode_device(zj_ctx *ctx, const zj_frame_desc *d, size_t nframes, const int16_t *d_y,
                          const int16_t *d_cb, const int16_t *d_cr, uint8_t *d_out, void *stream,
                          int iters, float *ms_total, float *ms_each, const char **kernel_name);

/* ---- ONE frame whose planes are still being written (round 6): strips go to the GPU as they become final ----------------
 * The reference runs post_process on strip N while its Huffman decoder is in strip N + 1 (src/mcu.rs:356-368: the strip is
 * handed to a pool thread).  zj_frame_begin names the frame's planes and output; zj_frame_rows_ready(ctx, n) says that the
 * coefficients of MCU rows [0, n) are final (n only grows; call it as often as convenient); the strips that became complete
 * go through the three-stream pipeline in units of an eighth of the frame (at least 4 MB of coefficients, ZJ_STREAM_UNIT_MB)
 * while the caller fills later rows; zj_frame_end submits what is left and waits for the pixels.  All calls but
 * zj_frame_end return at once when the planes are pinned (zj_alloc_pinned).  Output: a device pointer (out_on_device), pinned
 * host memory (downloads overlap as well), or pageable host memory (decoded into a device buffer, copied once at the end).
 * One such frame at a time per context, and no other call on the context in between.  Same bytes as zj_decode_planes.
 * ZJ_ERR_UNSUPPORTED: ZJ_LAYOUT_CHW, a padded out_pitch with a host output.  zj_decoder_decode_buffer uses this for baseline
 * files when the decoder's planes are pinned (zj_options.pinned_planes); ZJ_STREAM=off keeps the two stages apart. */
ZJ_API int zj_frame_begin(zj_ctx *ctx, const zj_frame_desc *d, const int16_t *y, const int16_t *cb, const int16_t *cr,
                          uint8_t *out, int out_on_device);
ZJ_API int zj_frame_rows_ready(zj_ctx *ctx, size_t mcu_rows);
ZJ_API int zj_frame_end(zj_ctx *ctx);
ZJ_API int zj_frame_abort(zj_ctx *ctx);   /* drains what is in flight; the output's content is undefined */
/* Host planes -> pixels that stay in HBM (d_out: device pointer, 16-byte aligned). Synchronous. */
ZJ_API int zj_decode_planes_to_device(zj_ctx *ctx, const zj_frame_desc *d, const int16_t *y, const int16_t *cb,
                               const int16_t *cr, uint8_t *d_out);
/* A prepared baseline scan (zj_decoder_prepare / zj_decoder_scan_blob; host memory, pinned for an asynchronous upload)
 * -> pixels: upload, Huffman decoding on the device into whole-frame planes in HBM, pixel kernel, and -- unless
 * out_on_device -- the download.  Replaces the MCU walk of src/mcu.rs:231-351.  Synchronous.  ZJ_RETRY_CPU with
 * *status_bits (optional) when the device hands the scan back. */
ZJ_API int zj_decode_scan(zj_ctx *ctx, const zj_frame_desc *d, const void *blob, size_t blob_bytes, uint8_t *out,
                   int out_on_device, unsigned *status_bits);
/* The same for up to ZJ_SCAN_BATCH_MAX prepared scans of any geometry at once: every phase of the entropy stage is ONE
 * launch over all of them (a single file leaves most of the GPU idle); the scans of one geometry and one set of tables
 * also share ONE pixel-kernel launch, wherever their outputs lie (zj_decode_frames_device's scattered form).  rcs[k] = ZJ_OK, ZJ_RETRY_CPU
 * or a zj_status of scan k; status_bits[k] optional.  The return value reports failures of the call itself. */
#define ZJ_SCAN_BATCH_MAX 16
ZJ_API int zj_decode_scans(zj_ctx *ctx, size_t n, const zj_frame_desc *descs, const void *const *blobs, const size_t *blob_bytes,
                    uint8_t *const *outs, int outs_on_device, int *rcs, unsigned *status_bits);
/* diagnostics: the coefficient planes the last zj_decode_scan on ctx left in HBM, copied to host buffers of zj_plane_len
 * elements each (NULL: skipped); len[3] (optional) receives the lengths */
ZJ_API int zj_scan_planes(zj_ctx *ctx, int16_t *y, int16_t *cb, int16_t *cr, size_t len[3]);
/* of the last zj_decode_scan on ctx: synchronisation rounds; ms[3] = host milliseconds spent submitting (everything in
 * front of the final synchronisation); with ZJ_HUFF_TIME set in the environment, ms[0..2] = device milliseconds of
 * upload + rounds | prefix sums + write pass | pixel kernel (+ download) */
ZJ_API int zj_scan_stats(const zj_ctx *ctx, int *rounds, float ms[4]);

/* ---- whole decoder: the CPU front-end the path is fed by (container + Huffman on the host) ------
 * Mirrors Decoder / ZuneJpegOptions / ImageInfo (src/decoder.rs:60,178,452,652; src/options.rs:6-40):
 * SOF0 baseline and SOF2 progressive Huffman, 8-bit, 1 or 3 components, DRI/RST.  The entropy decode
 * runs on the CPU into whole-image coefficient planes; zj_decoder_decode_buffer then runs the pixel
 * path on the GPU through zj_decode_planes. */
typedef struct zj_options {      /* zero = reference default */
    int32_t out_colorspace;      /* ZJ_CS_RGB (default 0), ZJ_CS_GRAYSCALE, ZJ_CS_YCBCR */
    int32_t strict_mode;         /* options.rs:38 */
    int32_t max_width, max_height; /* options.rs:34-35, default 16384 */
    int32_t max_scans;           /* options.rs:36, default 64 */
    int32_t num_threads;         /* options.rs:33, default 4.  The reference spends them on post_process strips; here
                                    the pixel path is one GPU launch, so they decode restart segments (DRI/RSTn,
                                    baseline) concurrently, enter a baseline scan WITHOUT restart markers at one point
                                    per thread (at most 16; zj_decoder_parallel_mcus) and clear the planes; the
                                    decoder keeps its helper threads until zj_decoder_free; 1 = strictly serial */
    int32_t pinned_planes;       /* non-zero: coefficient planes live in pinned host memory (DMA without staging) */
    uint32_t flags;              /* ZJ_FLAG_* for the pixel path (0 = the reference's bytes), see zj_frame_desc;
                                    + ZJ_FLAG_FULL_AC_VALUES, ZJ_FLAG_CMYK_TO_RGB and ZJ_FLAG_ANY_SAMPLING for the front-end
                                    itself */
    uint32_t out_layout;         /* ZJ_LAYOUT_HWC (0) or ZJ_LAYOUT_CHW */
    int32_t entropy;             /* where baseline Huffman scans are decoded: ZJ_ENTROPY_CPU (0), ZJ_ENTROPY_GPU (scans of
                                    32 KB and more and 16 bits per block and more on the device, the rest and everything
                                    the device hands back on the CPU), ZJ_ENTROPY_GPU_ALWAYS (every eligible scan: for
                                    tests).  Progressive files: always CPU.  The output bytes do not depend on it */
} zj_options;
#define ZJ_ENTROPY_CPU 0
#define ZJ_ENTROPY_GPU 1
#define ZJ_ENTROPY_GPU_ALWAYS 2
typedef struct zj_image_info {   /* ImageInfo, src/decoder.rs:652-668 (+ what the GPU path needs) */
    uint16_t width, height;
    uint8_t components, progressive, h_max, v_max;
    uint16_t scans, restart_interval;
} zj_image_info;
typedef struct zj_decoder zj_decoder;
ZJ_API zj_decoder *zj_decoder_new(const zj_options *opt);            /* Decoder::new_with_options */
ZJ_API void zj_decoder_free(zj_decoder *d);
ZJ_API const char *zj_decoder_error(const zj_decoder *d);            /* Display text of the last DecodeErrors */
ZJ_API int zj_decoder_read_headers(zj_decoder *d, const uint8_t *buf, size_t len, zj_image_info *info); /* decoder.rs:452 */
/* CPU half only: planes stay owned by the decoder until the next call (mcu_prog.rs:73-79 layout) */
ZJ_API int zj_decoder_decode_coefficients(zj_decoder *d, const uint8_t *buf, size_t len, zj_frame_desc *desc,
                                   const int16_t **planes /*[3]*/, size_t *plane_len /*[3]*/, zj_image_info *info);
/* Stage 1 on the CPU, whatever the options say it is: with entropy == ZJ_ENTROPY_CPU the same as
 * zj_decoder_decode_coefficients; with a GPU setting, headers + the byte-level preparation of a baseline scan
 * (stuffing removed, restart segments located, sub-sequence grid: csrc/zj_huff.h), leaving the Huffman decoding itself
 * (src/mcu.rs:231-351, src/bitstream.rs:314-373) to zj_decoder_finish_pixels.  `buf` must then stay valid until the
 * pixels are finished (a scan the device hands back is decoded from it on the CPU). */
ZJ_API int zj_decoder_prepare(zj_decoder *d, const uint8_t *buf, size_t len, zj_frame_desc *desc, zj_image_info *info);
/* GPU half: the pixel path over the planes the last zj_decoder_decode_coefficients / zj_decoder_prepare left in the
 * decoder; after a zj_decoder_prepare that left a scan for the device: entropy stage + pixel path on the GPU */
ZJ_API int zj_decoder_finish_pixels(zj_decoder *d, zj_ctx *ctx, uint8_t *out, size_t out_cap, size_t *out_len);
/* the same with the pixels left in HBM (d_out: device pointer on ctx's device, 16-byte aligned) for consumers on the GPU.
 * Stream ordering (also zj_decode_planes_device with stream = NULL, zj_decoder_finish_pixels_batch with device outputs and
 * zj_pool_decode_files_device): the library writes d_out on ITS OWN non-blocking stream and returns once that is complete;
 * it does NOT order itself after work the caller still has in flight on other streams.  A caller whose allocator recycles
 * device memory stream-ordered (a caching tensor allocator) must synchronise the stream that last used d_out before the call. */
ZJ_API int zj_decoder_finish_pixels_device(zj_decoder *d, zj_ctx *ctx, uint8_t *d_out, size_t out_cap, size_t *out_len);
/* the decoder's last prepared file cut to a window (zj_decode_crops_device's contract), pixels left in HBM; stream ordering
 * as zj_decoder_finish_pixels_device.  Planes decoded on the CPU: only the window's strips are uploaded; a scan left for
 * the device (zj_options.entropy): the entropy stage runs on the device, the crop kernel over its planes in HBM.
 * *out_len = zj_crop_out_len(); out_cap below it is ZJ_ERR_ARG. */
ZJ_API int zj_decoder_finish_pixels_crop_device(zj_decoder *d, zj_ctx *ctx, unsigned x, unsigned y, unsigned w, unsigned h,
                                                uint8_t *d_out, size_t out_cap, unsigned out_pitch, size_t *out_len);
/* the decoder's last prepared file: the w x h window at (x, y) resized (zj_decode_crops_resized_device's contract; the crop
 * is zj_decoder_finish_pixels_crop_device's), pixels left in HBM; stream ordering as zj_decoder_finish_pixels_device.
 * *out_len = zj_resized_out_len(); out_cap below it is ZJ_ERR_ARG. */
ZJ_API int zj_decoder_finish_pixels_resized_crop_device(zj_decoder *d, zj_ctx *ctx, unsigned x, unsigned y, unsigned w,
                                                        unsigned h, unsigned out_w, unsigned out_h, int dtype, int out_layout,
                                                        const float *scale, const float *bias, int flip, void *d_out,
                                                        size_t out_cap, size_t *out_len);
/* the decoder's last prepared file: the w x h window at (x, y) converted into one image of a normalised tensor, NOT resized
 * (zj_decode_crops_tensor_device's contract; flip: non-zero mirrors the columns), left in HBM; the file path, its uploads
 * and the stream ordering are zj_decoder_finish_pixels_crop_device's.  It takes the files that call takes, with an
 * out_colorspace of RGB / YCBCR / GRAYSCALE, out_layout ZJ_LAYOUT_HWC and no out_pitch.  With the decoder's flags set it
 * also takes a one-component file shown as RGB (ZJ_FLAG_GRAY_TO_RGB, out_colorspace RGB: the GRAYSCALE u8
 * crop, every channel that byte's conversion), a four-component file (ZJ_FLAG_CMYK_TO_RGB) and a file of another sampling or
 * stored RGB (ZJ_FLAG_ANY_SAMPLING): the u8 image the resized-crop call makes of the window in the context's buffer, then
 * zj_to_tensor_device -- byte for byte that call at out_w = w, out_h = h, bilinear.  ZJ_ERR_UNSUPPORTED, with a
 * zj_decoder_error text that says so: a one-component file of a decoder that asks for a colour output without
 * ZJ_FLAG_GRAY_TO_RGB, or for YCbCr with it (with out_colorspace GRAYSCALE it has its one-channel tensor).  A prescale is
 * the resized-crop calls'.  *out_len = C * w * h * the element's bytes; out_cap below it is ZJ_ERR_ARG. */
ZJ_API int zj_decoder_finish_pixels_crop_tensor_device(zj_decoder *d, zj_ctx *ctx, unsigned x, unsigned y, unsigned w,
                                                       unsigned h, int dtype, int out_layout, const float *scale,
                                                       const float *bias, int flip, void *d_out, size_t out_cap,
                                                       size_t *out_len);
/* ... with x, y, w, h in DISPLAYED pixels of the file's own orientation (zj_decoder_orientation): the stored window is
 * zj_orient_window's (orientations 5..8: h x w), the tensor always w x h, flip mirrors the displayed image's columns.  A file
 * with orientation 1, or with no or an invalid tag, takes the call above as it is.  A turned file: the u8 crop of the stored
 * window, the orient stage (CMYK and other samplings: in finish order of the resized oriented call), zj_to_tensor_device --
 * byte for byte zj_decoder_finish_pixels_resized_crop_oriented_device at out_w = w, out_h = h, bilinear, no prescale. */
ZJ_API int zj_decoder_finish_pixels_crop_tensor_oriented_device(zj_decoder *d, zj_ctx *ctx, unsigned x, unsigned y, unsigned w,
                                                                unsigned h, int dtype, int out_layout, const float *scale,
                                                                const float *bias, int flip, void *d_out, size_t out_cap,
                                                                size_t *out_len);
/* n decoders' last prepared files, of any sizes, into ONE crop tensor: file k's window is w x h at origins[2k],
 * origins[2k + 1], its image at d_out + k * zj_crop_tensor_out_len's bytes, image k what the single-file call above writes
 * for file k.  The decoders must agree in out_colorspace and out_layout (ZJ_ERR_ARG).  Consecutive files the CPU walker
 * decoded go through one mixed-geometry launch group; files prepared for device entropy, the files that call finishes
 * through zj_to_tensor_device (a one-component file shown as RGB, four components, another sampling) and every file it
 * refuses (a one-component file among colour ones without ZJ_FLAG_GRAY_TO_RGB, a damaged file, a window that leaves the
 * image) go through that call, which sets the decoder's error text.  rcs[k]: file k's status; a failed file leaves its
 * image untouched and stops no other.  out_cap below n images is ZJ_ERR_ARG.  Synchronous. */
ZJ_API int zj_decoder_finish_pixels_crop_tensor_batch_device(zj_decoder *const *ds, size_t n, zj_ctx *ctx,
                                                             const unsigned *origins, unsigned w, unsigned h, int dtype,
                                                             int out_layout, const float *scale, const float *bias,
                                                             const uint8_t *flip, void *d_out, size_t out_cap, int *rcs);
/* ... with the origins in DISPLAYED pixels of each file's own orientation: image k and rcs[k] are
 * zj_decoder_finish_pixels_crop_tensor_oriented_device's for file k; the turned files go through that call */
ZJ_API int zj_decoder_finish_pixels_crop_tensor_batch_oriented_device(zj_decoder *const *ds, size_t n, zj_ctx *ctx,
                                                                      const unsigned *origins, unsigned w, unsigned h,
                                                                      int dtype, int out_layout, const float *scale,
                                                                      const float *bias, const uint8_t *flip, void *d_out,
                                                                      size_t out_cap, int *rcs);
/* The decoder's last prepared file warped into one image of a normalised tensor: `matrix` as in zj_warp_device,
 * in pixels of the stored frame, or, with apply_orientation != 0, of the DISPLAYED frame of the file's EXIF orientation -- the
 * definition is orient first, then warp.  The image is zj_warp_device's of the u8 image the file decodes to (what
 * zj_decoder_finish_pixels_resized_crop_oriented_device resizes: a one-component file of an RGB decoder with
 * ZJ_FLAG_GRAY_TO_RGB as R = G = B, a four-component file with ZJ_FLAG_CMYK_TO_RGB, another sampling or stored RGB with
 * ZJ_FLAG_ANY_SAMPLING), but only the part of the frame the output can see (zj_warp_source_window) is decoded and, under the
 * CPU walker, uploaded; an output that sees nothing of the frame is all fill and decodes nothing.  The decoder's out_layout
 * must be ZJ_LAYOUT_HWC (ZJ_ERR_UNSUPPORTED otherwise); the other refusals are that call's and zj_warp_device's.  *out_len:
 * zj_resized_out_len's bytes.  Synchronous. */
ZJ_API int zj_decoder_finish_pixels_warped_device(zj_decoder *d, zj_ctx *ctx, const double matrix[6], int apply_orientation,
                                                  unsigned out_w, unsigned out_h, int dtype, int out_layout,
                                                  const float *scale, const float *bias, const uint8_t *fill, int edge,
                                                  void *d_out, size_t out_cap, size_t *out_len);
/* n decoders' last prepared files, of any sizes, each under its own matrix (matrices: 6 doubles per file), into ONE warped
 * tensor: file k's image lies at d_out + k * zj_resized_out_len's bytes and is what the single-file call above writes for
 * file k.  The decoders must agree in out_colorspace and out_layout (ZJ_ERR_ARG).  Consecutive files the CPU walker decoded
 * whose output sees some of their frame share the mixed-geometry crop launches of
 * zj_decoder_finish_pixels_resized_crop_batch_device, each cut to its own source window, and the warp launches over each
 * group's crops (48 files a launch); files prepared for device entropy, four-component files, files of another sampling or
 * stored RGB, an output that sees nothing of its frame and every file the single-file call refuses (a damaged file, a matrix
 * the warp does not take) go through that call, which sets the decoder's error text.  rcs[k]: file k's status; a failed file
 * leaves its image untouched and stops no other.  out_cap below n images is ZJ_ERR_ARG.  Synchronous. */
ZJ_API int zj_decoder_finish_pixels_warped_batch_device(zj_decoder *const *ds, size_t n, zj_ctx *ctx, const double *matrices,
                                                        int apply_orientation, unsigned out_w, unsigned out_h, int dtype,
                                                        int out_layout, const float *scale, const float *bias,
                                                        const uint8_t *fill, int edge, void *d_out, size_t out_cap, int *rcs);
/* ... with a resize filter (ZJ_RESIZE_*; any other is ZJ_ERR_ARG) */
ZJ_API int zj_decoder_finish_pixels_resized_crop_filtered_device(zj_decoder *d, zj_ctx *ctx, unsigned x, unsigned y,
                                                                 unsigned w, unsigned h, unsigned out_w, unsigned out_h,
                                                                 int dtype, int out_layout, const float *scale,
                                                                 const float *bias, int flip, int filter, void *d_out,
                                                                 size_t out_cap, size_t *out_len);
/* the decoder's last prepared file at 1 / 2^scale_log2, cut to the window x, y, w, h of the REDUCED frame (all four 0: the
 * whole reduced frame), pixels left in HBM: zj_decode_crops_scaled_device's contract.  With the CPU walker only the plane
 * rows the window's blocks lie in are uploaded; with device entropy the planes in HBM are used.
 * *out_len = zj_scaled_crop_out_len(); out_cap below it is ZJ_ERR_ARG.  Synchronous on the context's stream. */
ZJ_API int zj_decoder_finish_pixels_scaled_device(zj_decoder *d, zj_ctx *ctx, int scale_log2, unsigned x, unsigned y,
                                                  unsigned w, unsigned h, uint8_t *d_out, size_t out_cap,
                                                  unsigned out_pitch, size_t *out_len);
/* zj_decoder_finish_pixels_resized_crop_filtered_device with a reduced-size decode under the resize
 * (zj_decode_crops_resized_prescaled_device's contract for one image: x, y, w, h in full-resolution pixels,
 * max_prescale_log2 = 0..3, 0 = the call without it byte for byte) */
ZJ_API int zj_decoder_finish_pixels_resized_crop_prescaled_device(zj_decoder *d, zj_ctx *ctx, unsigned x, unsigned y,
                                                                  unsigned w, unsigned h, unsigned out_w, unsigned out_h,
                                                                  int dtype, int out_layout, const float *scale,
                                                                  const float *bias, int flip, int filter,
                                                                  int max_prescale_log2, void *d_out, size_t out_cap,
                                                                  size_t *out_len);
/* EXIF Orientation of the file whose headers were read last (zj_decoder_read_headers / _prepare / _decode_coefficients /
 * _decode_buffer): 1..8, 1 when the file says nothing usable; 0 before any file.  The first APP1 segment in front of SOS whose
 * payload begins "Exif\0\0" decides: TIFF header (II or MM), IFD0, the entry with tag 0x0112, type SHORT, count 1.  Anything
 * else (a bad header, an offset or entry past the segment or the buffer, another type or count, a value outside 1..8) is 1. */
ZJ_API int zj_decoder_orientation(const zj_decoder *d);
/* the Adobe APP14 segment of the file whose headers were read last: -1 when none was seen (or before any file), else its
 * transform byte (0: CMYK / RGB as stored, 1: YCbCr, 2: YCCK).  Read for every file; it decides something for four-component
 * files only (ZJ_FLAG_CMYK_TO_RGB). */
ZJ_API int zj_decoder_adobe_transform(const zj_decoder *d);
/* 1 when the last file whose headers were read is STORED RGB: three components and an Adobe APP14 segment with transform 0
 * (the samples are R, G, B, not Y, Cb, Cr); else 0.  The rule does not look at component ids: 'R','G','B' without the segment
 * stays YCbCr, as in libjpeg.  It decides something with ZJ_FLAG_ANY_SAMPLING only. */
ZJ_API int zj_decoder_stored_rgb(const zj_decoder *d);
/* the sampling factors (h, v) of component `comp` (0 .. components - 1) of the last file whose headers were read, as its
 * frame header states them (a one-component file: 1, 1).  Either output may be NULL.  ZJ_ERR_ARG: no such component. */
ZJ_API int zj_decoder_component_sampling(const zj_decoder *d, int comp, unsigned *h, unsigned *v);
/* plane `comp` (0 .. components - 1) of the last file, after a successful CPU decode (zj_decoder_decode_coefficients, or
 * zj_decoder_prepare that left no scan for the device): the plane, its length in int16 elements and its size in blocks.
 * Any output pointer may be NULL.  ZJ_ERR_ARG: no such component, or no decoded coefficients. */
ZJ_API int zj_decoder_plane(const zj_decoder *d, int comp, const int16_t **plane, size_t *len, unsigned *blocks_w,
                            unsigned *blocks_h);
/* zj_decoder_finish_pixels_device with the file's orientation applied (what an EXIF-aware image loader returns): the whole
 * DISPLAYED image, tight, in the decoder's colour space and layout; *out_w x *out_h (optional) its size.  Orientation 1
 * decodes straight into d_out; the others decode into a buffer of the context and are turned from there.  RGBA / RGBX are
 * ZJ_ERR_UNSUPPORTED.  *out_len = zj_out_len(); out_cap below it is ZJ_ERR_ARG. */
ZJ_API int zj_decoder_finish_pixels_oriented_device(zj_decoder *d, zj_ctx *ctx, uint8_t *d_out, size_t out_cap, size_t *out_len,
                                                    unsigned *out_w, unsigned *out_h);
/* zj_decoder_finish_pixels_resized_crop_prescaled_device with x, y, w, h in DISPLAYED pixels of the file's own orientation
 * (zj_decode_crops_resized_oriented_device's contract for one image).  With the CPU walker still only the stored window's
 * strips / MCU rows are uploaded. */
ZJ_API int zj_decoder_finish_pixels_resized_crop_oriented_device(zj_decoder *d, zj_ctx *ctx, unsigned x, unsigned y,
                                                                 unsigned w, unsigned h, unsigned out_w, unsigned out_h,
                                                                 int dtype, int out_layout, const float *scale,
                                                                 const float *bias, int flip, int filter,
                                                                 int max_prescale_log2, void *d_out, size_t out_cap,
                                                                 size_t *out_len);
/* n decoders after zj_decoder_prepare or zj_decoder_decode_coefficients, each with its own file of any size, into one
 * resized-crop tensor: image k lands at d_out + k * zj_resized_out_len().  windows[4k .. 4k + 3] = x, y, w, h in DISPLAYED
 * pixels of file k's own orientation when apply_orientation is set, else in stored pixels.
 * DEFINITION: image k equals what zj_decoder_finish_pixels_resized_crop_oriented_device gives for decoder k alone (without
 * apply_orientation: the _prescaled_ call), and rcs[k] is that call's status.  A file that fails leaves its image's bytes
 * untouched and does not stop the others.  The call itself returns non-zero only for null arguments, out_cap below n images,
 * or decoders whose output colour space or layout differ.
 * Files the CPU walker decoded: only the plane rows each window needs are uploaded, all files of a launch group into one
 * arena of the context, all uploads queued before the group's mixed-geometry launches
 * (zj_decode_crops_resized_mixed_device).  Decoders with a scan left for the device (zj_options.entropy), and all-zero
 * outputs, are finished one by one through the single-file call.  Stream ordering as zj_decoder_finish_pixels_device. */
ZJ_API int zj_decoder_finish_pixels_resized_crop_batch_device(zj_decoder *const *ds, size_t n, zj_ctx *ctx,
                                                              const unsigned *windows, unsigned out_w, unsigned out_h,
                                                              int dtype, int out_layout, const float *scale,
                                                              const float *bias, const uint8_t *flip, int filter,
                                                              int max_prescale_log2, int apply_orientation, void *d_out,
                                                              size_t out_cap, int *rcs);
/* zj_decoder_finish_pixels_resized_crop_batch_device with file k's image under the colour matrix color[12k .. 12k + 11]
 * (zj_color_fixed's definition) in front of the resize: the matrix acts on exactly the u8 image the call
 * without it resizes -- after the crop or reduced decode, the turn, the gray expand (ZJ_FLAG_GRAY_TO_RGB), the CMYK combine
 * (ZJ_FLAG_CMYK_TO_RGB) and the plane combine (ZJ_FLAG_ANY_SAMPLING) -- in place.  color NULL: the call above.  A matrix
 * zj_color_fixed refuses gives rcs[k] = ZJ_ERR_ARG and the decoder's error text; that file's image is untouched and the
 * others are decoded.  A decoder whose output has one channel: ZJ_ERR_UNSUPPORTED for that file.  n = 1 is the single-file
 * call. */
ZJ_API int zj_decoder_finish_pixels_resized_crop_batch_colored_device(zj_decoder *const *ds, size_t n, zj_ctx *ctx,
                                                                      const unsigned *windows, unsigned out_w, unsigned out_h,
                                                                      int dtype, int out_layout, const float *scale,
                                                                      const float *bias, const uint8_t *flip, int filter,
                                                                      int max_prescale_log2, int apply_orientation,
                                                                      const double *color /* 12 per file, or NULL */,
                                                                      void *d_out, size_t out_cap, int *rcs);
/* zj_decoder_finish_pixels_resized_crop_batch_colored_device with file k's image under the tone op tone[2k], tone[2k + 1]
 * (the ops above) behind the colour matrix and in front of the resize: the op acts on exactly the u8 image the
 * call without it resizes -- after the crop or reduced decode, the turn, the gray expand, the CMYK combine, the plane combine
 * and the colour matrix -- in place; its histogram is that of this crop, not of the whole file.  tone NULL: the call above.
 * An op the stage refuses gives rcs[k] = ZJ_ERR_ARG and the decoder's error text; that file's image is untouched and the
 * others are decoded.  A decoder whose output has one channel takes its op as one channel (a non-NULL color stays
 * ZJ_ERR_UNSUPPORTED for that file). */
ZJ_API int zj_decoder_finish_pixels_resized_crop_batch_toned_device(zj_decoder *const *ds, size_t n, zj_ctx *ctx,
                                                                    const unsigned *windows, unsigned out_w, unsigned out_h,
                                                                    int dtype, int out_layout, const float *scale,
                                                                    const float *bias, const uint8_t *flip, int filter,
                                                                    int max_prescale_log2, int apply_orientation,
                                                                    const double *color /* 12 per file, or NULL */,
                                                                    const int32_t *tone /* 2 per file, or NULL */, void *d_out,
                                                                    size_t out_cap, int *rcs);
/* stage 2 of n decoders on one context: the scans left for the device are decoded together (zj_decode_scans), the rest
 * one by one; rcs[k] is what zj_decoder_finish_pixels[_device] would have returned for decoder k */
ZJ_API int zj_decoder_finish_pixels_batch(zj_decoder *const *ds, size_t n, zj_ctx *ctx, uint8_t *const *outs,
                                   const size_t *out_caps, size_t *out_lens /*[n] or NULL*/, int outs_on_device, int *rcs);
/* diagnostics: the prepared scan of the last zj_decoder_prepare (ZJ_ERR_ARG: none); the status bits (csrc/zj_huff.h
 * HUFF_ST_*) with which the device handed the last scan back to the CPU (0: it did not) */
ZJ_API int zj_decoder_scan_blob(const zj_decoder *d, const void **blob, size_t *len);
ZJ_API unsigned zj_decoder_gpu_status(const zj_decoder *d);
/* Decoder::decode_buffer (decoder.rs:178): width*height*ncomp bytes into `out` */
ZJ_API int zj_decoder_decode_buffer(zj_decoder *d, zj_ctx *ctx, const uint8_t *buf, size_t len, uint8_t *out,
                             size_t out_cap, size_t *out_len, zj_image_info *info);
/* restart segments the last baseline scan decoded concurrently (0 = the serial walk was used) */
ZJ_API int zj_decoder_parallel_segments(const zj_decoder *d);
/* MCUs of the last baseline scan WITHOUT restart markers that several threads decoded (zj_options.num_threads > 1: the scan is
 * entered at one point per thread, the threads fall into step with the true symbol sequence; zj_jpeg.cpp); 0 = the serial walk */
ZJ_API int64_t zj_decoder_parallel_mcus(const zj_decoder *d);
/* Decoder::set_num_threads (src/decoder.rs:591-603, deprecated there in favour of the options): the thread count from the next
 * file on; 0 -> ZJ_ERR_FORMAT "Cannot set zero threads to decode image".  zj_pool uses it to lend the workers a short batch
 * leaves idle to the files it has (below). */
ZJ_API int zj_decoder_set_num_threads(zj_decoder *d, int threads);

/* ---- batches of files: `threads` persistent host workers, each with its own entropy
 * decoder, pinned coefficient planes and GPU context on `device`; file i is decoded by whichever worker is
 * free, so the CPU Huffman stage of one file overlaps the PCIe copies and kernels of the others.  Replaces a
 * caller-side loop over Decoder::decode_buffer (src/decoder.rs:178; the reference's own pool is per decode,
 * src/mcu.rs:135).  outs[i] must hold out_caps[i] >= width*height*ncomp bytes; statuses[i] (optional) gets
 * the zj_status of file i; the return value is the first error seen (ZJ_OK if none), text via zj_pool_error.
 * A batch of at most half as many files as workers gets the idle workers' share of the CPUs inside its files
 * (threads / files threads per file, at most 16: zj_decoder_set_num_threads), so two large files on a pool of sixteen do
 * not take what one file takes on one thread; opt->num_threads is the floor (default here: 1). */
typedef struct zj_pool zj_pool;
ZJ_API zj_pool *zj_pool_create(int device, int threads, const zj_options *opt, int *status);
/* Image-level sharding across the GPUs of one node, inside the library (north_star): one pool over `ndev`
 * device slots (devices[k] = HIP device of slot k; a device may fill several slots), threads_per_device entropy workers
 * per slot.  Every slot has its own submitters and contexts; workers and pinned plane sets are shared.  Files whose
 * pixels go to host memory are taken by whichever slot is free (dealt by readiness, so a slow GPU does not hold up a
 * fixed share); with zj_pool_decode_files_device each file goes to the slot(s) of the device that owns its output pointer
 * (zj_pointer_device), so a caller shards by allocating output i on device i * ndev / nfiles.  Results are in the caller's
 * order either way.  The 8-GPU node: devices = {0,...,7}. */
ZJ_API zj_pool *zj_pool_create_multi(const int *devices, int ndev, int threads_per_device, const zj_options *opt, int *status);
ZJ_API int zj_pool_devices(const zj_pool *pool);              /* device slots */
/* of one slot, accumulated since creation: its HIP device, seconds inside its GPU stage, files it finished */
ZJ_API int zj_pool_device_stats(zj_pool *pool, int slot, int *device, double *gpu_seconds, size_t *files);
/* of one slot: NUMA node of its device (-1 unknown), how many of its threads (entropy workers + submitters) were bound to
 * that node, how many it has.  Each slot has its own workers and plane sets; a file's planes are filled, pinned and DMA'd
 * on the socket of the GPU that decodes it (a slot with nothing to do may take over a file of another slot). */
ZJ_API int zj_pool_slot_numa(zj_pool *pool, int slot, int *device_node, int *threads_bound, int *threads);
ZJ_API void zj_pool_destroy(zj_pool *pool);
ZJ_API int zj_pool_threads(const zj_pool *pool);
ZJ_API const char *zj_pool_error(const zj_pool *pool);
/* accumulated since creation: seconds spent inside the entropy stage and inside the GPU stage (summed over the
 * threads of each stage) and files that reached the GPU stage */
ZJ_API int zj_pool_stats(zj_pool *pool, double *entropy_seconds, double *gpu_seconds, size_t *files);
ZJ_API int zj_pool_decode_files(zj_pool *pool, size_t nfiles, const uint8_t *const *bufs, const size_t *lens,
                         uint8_t *const *outs, const size_t *out_caps, size_t *out_lens /*[nfiles] or NULL*/,
                         zj_image_info *infos /*[nfiles] or NULL*/, int *statuses /*[nfiles] or NULL*/);

/* the same with device pointers (on the pool's device, 16-byte aligned) as outputs: the pixels stay in HBM for a
 * consumer on the GPU, nothing crosses PCIe but the compressed files (with a GPU entropy setting) or the planes */
ZJ_API int zj_pool_decode_files_device(zj_pool *pool, size_t nfiles, const uint8_t *const *bufs, const size_t *lens,
                                uint8_t *const *d_outs, const size_t *out_caps, size_t *out_lens /*[nfiles] or NULL*/,
                                zj_image_info *infos /*[nfiles] or NULL*/, int *statuses /*[nfiles] or NULL*/);

/* ---- image-level sharding of plane batches across the GPUs of one node ------------------------------
 * Frames are independent, so N frames over D device slots are D contiguous shards (zj_shard_range: sizes differ by at
 * most one; the same rule as bench.py's ranks) and no collective.  A zj_multi owns one context and one persistent host
 * thread per slot ("one host thread per GPU"); a call runs every slot's shard at once through that slot's three-stream
 * pipeline and returns when all are done.  statuses[slot] (optional) = that shard's zj_status; the return value is the
 * first error.  devices[k] may repeat (two slots on one GPU).  The 8-GPU node: devices = {0,...,7}. */
typedef struct zj_multi zj_multi;
ZJ_API void zj_shard_range(size_t nframes, int slot, int nslots, size_t *lo, size_t *hi); /* [lo, hi) of slot */
ZJ_API zj_multi *zj_multi_create(const int *devices, int ndev, int *status);
ZJ_API void zj_multi_destroy(zj_multi *m);
ZJ_API int zj_multi_devices(const zj_multi *m);
ZJ_API zj_ctx *zj_multi_ctx(zj_multi *m, int slot);            /* slot's context (owned by m), e.g. for zj_device_alloc */
ZJ_API int zj_multi_slot_stats(zj_multi *m, int slot, int *device, size_t *frames); /* frames decoded since creation */
/* where slot's device and its host thread live: NUMA node of the device (-1 unknown), node the thread runs on (-1 unknown),
 * whether the thread was bound (0 with ZJ_NUMA=off, an unknown node, or an affinity that excludes the node) */
ZJ_API int zj_multi_slot_numa(zj_multi *m, int slot, int *device_node, int *thread_node, int *bound);
/* zj_decode_planes_batch / zj_decode_frames, sharded: host planes (pinned: zj_alloc_pinned) -> host pixels */
ZJ_API int zj_multi_decode_planes_batch(zj_multi *m, const zj_frame_desc *d, size_t nframes, const int16_t *y,
                                 const int16_t *cb, const int16_t *cr, uint8_t *out, int *statuses /*[slots] or NULL*/);
ZJ_API int zj_multi_decode_frames(zj_multi *m, const zj_frame_desc *d, size_t nframes, const int16_t *const *y,
                           const int16_t *const *cb, const int16_t *const *cr, uint8_t *const *out, int *statuses);
/* zj_decode_frames_device, sharded: frame f's pointers must live on the device of the slot whose shard holds f;
 * returns once every shard is complete */
ZJ_API int zj_multi_decode_frames_device(zj_multi *m, const zj_frame_desc *d, size_t nframes, const int16_t *const *d_y,
                                  const int16_t *const *d_cb, const int16_t *const *d_cr, uint8_t *const *d_out,
                                  int *statuses);

/* ---- memory helpers ------------------------------------------------------------------------- */
/* hipHostMalloc, portable (usable as a DMA source/target from every device); NULL on failure.  zj_free_pinned keeps up to
 * ZJ_PINNED_CACHE_MB (default 512, 0 = none) of freed blocks for later requests of at least half their size from a thread on the
 * same device: pinning costs milliseconds per 10 MB, and a decoder made per file (zj_options.pinned_planes) would pay it per file */
ZJ_API void *zj_alloc_pinned(size_t bytes);
/* binds the CALLING thread to `device` (hipSetDevice): host threads that only allocate pinned memory or fill planes for a
 * context on device N call this first, so they neither initialise nor pin against device 0 */
ZJ_API int zj_set_thread_device(int device);
/* ---- NUMA placement of a device's host side (round 6).  On a two-socket node a GPU's feeder threads and the
 * pinned planes they fill belong on the GPU's socket.  hipHostMalloc already puts pinned memory on the node of the thread's
 * CURRENT device (so call zj_set_thread_device before zj_alloc_pinned); these bind the threads.  zj_pool and zj_multi bind
 * their own slot threads; a process-per-GPU caller (bench.py's ranks) calls zj_bind_thread_near_device first thing, so every
 * thread it starts later inherits the placement.  ZJ_NUMA=off turns all binding off.  A CPU affinity the process was
 * started with (taskset, cpuset) is respected: threads are bound to its intersection with the node, or left alone. */
ZJ_API int zj_device_pci_bus_id(int device, char *buf, size_t cap);  /* "0000:5a:00.0" */
ZJ_API int zj_device_numa_node(int device);          /* >= 0, or -1: unknown / single node */
ZJ_API int zj_bind_thread_to_numa_node(int node);    /* CPUs the calling thread may now run on, or -1: not bound */
ZJ_API int zj_bind_thread_near_device(int device);   /* the node the calling thread is now bound to, or -1: not bound */
ZJ_API int zj_thread_numa_node(void);                /* node of the CPU the calling thread is running on, or -1 */
/* the HIP device that owns device pointer p (>= 0), ZJ_ERR_ARG for host memory or an unknown pointer */
ZJ_API int zj_pointer_device(const void *p);
ZJ_API void zj_free_pinned(void *p);
ZJ_API void *zj_device_alloc(zj_ctx *ctx, size_t bytes);
ZJ_API void zj_device_free(zj_ctx *ctx, void *p);
ZJ_API int zj_memcpy_h2d(zj_ctx *ctx, void *dst, const void *src, size_t bytes);
ZJ_API int zj_memcpy_d2h(zj_ctx *ctx, void *dst, const void *src, size_t bytes);
ZJ_API int zj_device_memset(zj_ctx *ctx, void *d_ptr, int value, size_t bytes);
ZJ_API int zj_sync(zj_ctx *ctx);

/* ---- tuning knobs (every setting produces the same bytes) ------------------------------------ */
/* generation of the fused kernel: 0 = packed IDCT + staged stores (default), 1 = wide (24-bit multiplies, per-lane
 * stores; only in a `make VARIANTS=all` build), 2 = packed with direct stores.  Also settable per process with ZJ_VARIANT. */
ZJ_API int zj_set_variant(zj_ctx *ctx, int variant);
/* 1 if this build of the library carries the variant.  The default build is the product: 0 and 2.  Variant 1 (round 1's
 * generation, the A/B baseline and the parity suite's N-version cross-check) comes with `make VARIANTS=all`; without it
 * zj_set_variant(ctx, 1) returns ZJ_ERR_UNSUPPORTED. */
ZJ_API int zj_variant_available(int variant);
/* 0 = zj_decode_planes_batch runs upload / kernel / download back to back instead of overlapped on three streams */
ZJ_API int zj_set_pipeline(zj_ctx *ctx, int on);

#ifdef __cplusplus
}
#endif
#endif

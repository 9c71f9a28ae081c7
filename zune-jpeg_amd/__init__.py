"""
zune-jpeg_amd -- MI355X-native implementation of zune-jpeg's post-entropy pixel path
(dequantize + 8x8 integer IDCT, chroma up-sampling, YCbCr->RGB), behind the C ABI of
include/zjhip.h.  This Python package is only the thin ctypes binding used by tests/ and bench.py;
the product is libzjhip.so (zune-jpeg_amd/csrc).

There is NO CPU fallback: if libzjhip.so is missing, or no HIP device is usable, the calls raise.
Import with importlib.import_module("zune-jpeg_amd") (the directory name carries a hyphen).
"""
from .host import (  # noqa: F401
    BACKEND_AVX2, BACKEND_HIP, BACKEND_SCALAR, FLAG_CLAMP_DC, FLAG_CORRECTED, FLAG_EDGE_REPLICATE, FLAG_ANY_SAMPLING, FLAG_CMYK_TO_RGB, FLAG_FULL_AC_VALUES, FLAG_GRAY_TO_RGB, FLAG_PLAIN_TAIL, LAYOUT_CHW, LAYOUT_HWC, ColorSpace, Component, Context, DecodeError, Decoder, FrameDesc,
    ENTROPY_CPU, ENTROPY_GPU, ENTROPY_GPU_ALWAYS, HUFF_ST, RETRY_CPU, FileBatchDecoder, ImageInfo, Pool, ZjError,
    ZuneJpegOptions, abi_symbols, choose_idct_func, choose_upsample_func,
    choose_ycbcr_to_rgb_convert_func, device_count, finish_pixels_batch, finish_pixels_resized_crop_batch, finish_pixels_crop_tensor_batch, lib, lib_path, num_components,
    SCATTER_MAX, Multi, pointer_device, shard_range, device_numa_node, bind_thread_near_device, thread_numa_node, variants_available,
    crop_out_len, resized_out_len, crop_tensor_out_len, scaled_size, scaled_crop_out_len, oriented_size, orient_window, DTYPE_F32, DTYPE_F16, DTYPE_BF16, DTYPE_U8, TENSOR_NCHW, TENSOR_NHWC,
    RESIZE_BILINEAR, RESIZE_BILINEAR_AA, RESIZE_BICUBIC_AA, resize_filter,
    WARP_FILL, WARP_REPLICATE, warp_edge, warp_fixed, warp_source_window, finish_pixels_warped_batch,
    color_fixed,
    TONE_IDENTITY, TONE_INVERT, TONE_POSTERIZE, TONE_SOLARIZE, TONE_AUTOCONTRAST, TONE_EQUALIZE, TONE_OPS,
)

"""
host.py -- ctypes binding of libzjhip.so mirroring the reference's interface for the pixel path.

Names follow the reference (paths relative to the zune-jpeg tree):
  ColorSpace                         src/misc.rs:88-121
  ZuneJpegOptions                    src/options.rs:6-160 (+ a `backend` knob: scalar / avx2 / hip)
  choose_idct_func                   src/idct.rs:40
  choose_upsample_func               Decoder::set_upsampling, src/decoder.rs:468-523
  choose_ycbcr_to_rgb_convert_func   src/color_convert.rs:61
  Context.post_process               src/worker.rs:32
  Context.decode_planes              strip loop of src/mcu_prog.rs:132-246 over whole-image planes

Only the HIP arm exists here; asking for scalar/avx2 raises ZjError(ZJ_ERR_BACKEND) because those
arms live in the host application (the Rust crate), not in this library.
"""
import ctypes as C
import enum
import os
import sys

import numpy as np

BACKEND_SCALAR, BACKEND_AVX2, BACKEND_HIP = 0, 1, 2

OK, ERR_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_NOMEM, ERR_PANIC, ERR_NO_DEVICE, ERR_BACKEND = 0, -1, -2, -3, -4, -5, -6, -7


class ColorSpace(enum.IntEnum):  # src/misc.rs:88-106
    RGB = 0
    GRAYSCALE = 1
    YCbCr = 2
    CMYK = 3
    YCCK = 4
    RGBA = 5
    RGBX = 6

    def num_components(self):  # src/misc.rs:113-121
        return {0: 3, 2: 3, 1: 1}.get(int(self), 4)


def num_components(cs):
    return ColorSpace(cs).num_components()


class ZjError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = what
        try:
            msg = f"{what}: {lib().zj_strerror(status).decode()}"
        except Exception:
            pass
        super().__init__(f"[zj status {status}] {msg}")


class Component(C.Structure):  # zj_component  <->  Components, src/components.rs:18-43
    _fields_ = [("horizontal_sample", C.c_size_t), ("vertical_sample", C.c_size_t),
                ("width_stride", C.c_size_t), ("quantization_table", C.c_int32 * 64)]


FLAG_PLAIN_TAIL = 1   # zj_frame_desc.flags: extension, every pixel at its own position (no Q5/Q6)
FLAG_CLAMP_DC = 2     # extension: DC-only shortcut value clamped to 0..255 (Q1 corrected)
FLAG_EDGE_REPLICATE = 4  # extension: horizontal chroma filter per row with replicated edges (Q4 corrected)
FLAG_CORRECTED = 7
FLAG_FULL_AC_VALUES = 8  # zj_options.flags only: the front-end yields AC values as coded (the reference cuts some to six bits)
FLAG_GRAY_TO_RGB = 16    # resized crops and the crop-tensor file calls only: a one-component frame / file asked for RGB gives R = G = B
FLAG_CMYK_TO_RGB = 32    # decoder options only: four-component (Adobe CMYK / YCCK) files are accepted and the resized-crop
                         # calls show them as RGB
FLAG_ANY_SAMPLING = 64   # decoder options only: three-component files of any sampling with factors 1, 2, 4 (4:1:1, 4:1:0,
                         # chroma that is not (1,1)), any ids, and stored-RGB files are accepted and the resized-crop calls
                         # show them as RGB
LAYOUT_HWC, LAYOUT_CHW = 0, 1
DTYPE_F32, DTYPE_F16, DTYPE_BF16, DTYPE_U8 = 0, 1, 2, 3  # zj_resize_device and the resized crops: the output's dtype
TENSOR_NCHW, TENSOR_NHWC = 0, 1                          # ... and its layout
RESIZE_BILINEAR, RESIZE_BILINEAR_AA = 0, 1               # ... and its filter (the *_filtered_device entry points)
RESIZE_BICUBIC_AA = 4                                    # (2 and 3 are not filters)


def resize_filter(antialias=False, interpolation="bilinear"):
    """The RESIZE_* filter of the Python keywords: "bilinear" plain or antialiased (the triangle filter), "bicubic" only
    antialiased (Keys' cubic, a = -1/2, over the scaled support: Pillow's BICUBIC, F.interpolate(mode="bicubic",
    antialias=True))."""
    if interpolation == "bilinear":
        return RESIZE_BILINEAR_AA if antialias else RESIZE_BILINEAR
    if interpolation == "bicubic":
        if not antialias:
            raise ValueError('interpolation="bicubic" needs antialias=True: supported are "bilinear" (antialias False or '
                             'True) and "bicubic" with antialias=True; the plain 4-tap bicubic is another filter')
        return RESIZE_BICUBIC_AA
    raise ValueError(f'interpolation must be "bilinear" or "bicubic", not {interpolation!r}')


class FrameDesc(C.Structure):  # zj_frame_desc
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("h_max", C.c_uint32),
                ("v_max", C.c_uint32), ("in_components", C.c_uint32), ("out_colorspace", C.c_int32),
                ("qt", (C.c_int32 * 64) * 3), ("flags", C.c_uint32), ("out_layout", C.c_uint32),
                ("out_pitch", C.c_uint32)]

    @classmethod
    def make(cls, width, height, h_max, v_max, in_components, out_colorspace, qts, flags=0, out_layout=0, out_pitch=0):
        d = cls()
        d.width, d.height, d.h_max, d.v_max = width, height, h_max, v_max
        d.in_components, d.out_colorspace = in_components, int(out_colorspace)
        d.flags, d.out_layout, d.out_pitch = int(flags), int(out_layout), int(out_pitch)
        for c in range(3):
            q = np.asarray(qts[min(c, len(qts) - 1)], np.int32).reshape(64)
            C.memmove(d.qt[c], q.ctypes.data, 256)
        return d


ENTROPY_CPU, ENTROPY_GPU, ENTROPY_GPU_ALWAYS = 0, 1, 2
ZJ_SCAN_BATCH_MAX = 16
RETRY_CPU = 1  # zj_decode_scan: the device hands the scan back
# csrc/zj_huff.h HUFF_ST_*
HUFF_ST = {1: "bad code", 2: "run past 63", 4: "bits exhausted", 8: "EOI cut before the last row loop", 16: "phase",
           32: "no synchronisation", 64: "a DC symbol the reference may read short"}


class Options(C.Structure):  # zj_options
    _fields_ = [("out_colorspace", C.c_int32), ("strict_mode", C.c_int32), ("max_width", C.c_int32),
                ("max_height", C.c_int32), ("max_scans", C.c_int32), ("num_threads", C.c_int32),
                ("pinned_planes", C.c_int32), ("flags", C.c_uint32), ("out_layout", C.c_uint32),
                ("entropy", C.c_int32)]


class ImageInfo(C.Structure):  # zj_image_info  <->  ImageInfo, src/decoder.rs:652-668
    _fields_ = [("width", C.c_uint16), ("height", C.c_uint16), ("components", C.c_uint8),
                ("progressive", C.c_uint8), ("h_max", C.c_uint8), ("v_max", C.c_uint8),
                ("scans", C.c_uint16), ("restart_interval", C.c_uint16)]


class ZuneJpegOptions:
    """Mirror of src/options.rs:6-40 (defaults :26-40) plus the dispatch knob."""

    def __init__(self):
        self.use_unsafe = True
        self.out_colorspace = ColorSpace.RGB
        self.num_threads = 4
        self.max_width = 16384
        self.max_height = 16384
        self.max_scans = 64
        self.strict_mode = False
        self.backend = BACKEND_HIP
        self.device = 0
        self.pinned_planes = False
        self.flags = 0          # FLAG_* extensions of the pixel path (0 = the reference's bytes)
        self.out_layout = LAYOUT_HWC
        self.entropy = ENTROPY_CPU  # ENTROPY_GPU / ENTROPY_GPU_ALWAYS: baseline Huffman scans on the device

    def to_c(self):
        o = Options()
        o.out_colorspace = int(self.out_colorspace)
        o.strict_mode = int(self.strict_mode)
        o.max_width, o.max_height, o.max_scans = self.max_width, self.max_height, self.max_scans
        o.num_threads = int(self.num_threads)
        o.pinned_planes = int(bool(self.pinned_planes))
        o.flags, o.out_layout = int(self.flags), int(self.out_layout)
        o.entropy = int(self.entropy)
        return o


_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

ABI = [  # every symbol include/zjhip.h declares
    "zj_abi_version", "zj_device_count", "zj_ctx_create", "zj_ctx_destroy", "zj_default_ctx",
    "zj_strerror", "zj_last_error", "zj_idct_strip", "zj_upsample_h", "zj_upsample_v",
    "zj_upsample_hv", "zj_ycbcr_to_rgb16", "zj_post_process_strip", "zj_choose_idct_func",
    "zj_choose_upsample_func", "zj_choose_ycbcr_to_rgb_convert_func", "zj_plane_len", "zj_out_len",
    "zj_num_components", "zj_decode_planes", "zj_decode_planes_batch", "zj_decode_planes_device",
    "zj_time_decode_device", "zj_alloc_pinned", "zj_free_pinned", "zj_set_thread_device", "zj_device_alloc",
    "zj_device_free", "zj_memcpy_h2d", "zj_memcpy_d2h", "zj_sync", "zj_device_memset",
    "zj_decode_planes_to_device", "zj_decode_scan", "zj_decode_scans", "zj_decoder_finish_pixels_batch", "zj_scan_stats", "zj_scan_planes", "zj_decoder_prepare",
    "zj_decoder_finish_pixels_device", "zj_decoder_scan_blob", "zj_decoder_gpu_status", "zj_pool_decode_files_device",
    "zj_decoder_new", "zj_decoder_free", "zj_decoder_error", "zj_decoder_read_headers",
    "zj_decoder_decode_coefficients", "zj_decoder_finish_pixels", "zj_decoder_decode_buffer",
    "zj_decoder_parallel_segments", "zj_decoder_parallel_mcus", "zj_decoder_set_num_threads",
    "zj_pool_create", "zj_pool_destroy", "zj_pool_threads", "zj_pool_error", "zj_pool_stats",
    "zj_pool_decode_files", "zj_set_variant", "zj_variant_available", "zj_set_pipeline",
    "zj_decode_frames", "zj_decode_planes_device_strided", "zj_decode_frames_device", "zj_pointer_device",
    "zj_pool_create_multi", "zj_pool_devices", "zj_pool_device_stats",
    "zj_shard_range", "zj_multi_create", "zj_multi_destroy", "zj_multi_devices", "zj_multi_ctx", "zj_multi_slot_stats",
    "zj_frame_begin", "zj_frame_rows_ready", "zj_frame_end", "zj_frame_abort",
    "zj_device_pci_bus_id", "zj_device_numa_node", "zj_bind_thread_to_numa_node", "zj_bind_thread_near_device",
    "zj_thread_numa_node", "zj_pool_slot_numa", "zj_multi_slot_numa",
    "zj_multi_decode_planes_batch", "zj_multi_decode_frames", "zj_multi_decode_frames_device",
    "zj_crop_out_len", "zj_decode_crops_device", "zj_decoder_finish_pixels_crop_device",
    "zj_resized_out_len", "zj_resize_device", "zj_decode_crops_resized_device", "zj_decoder_finish_pixels_resized_crop_device",
    "zj_resize_filtered_device", "zj_decode_crops_resized_filtered_device",
    "zj_decoder_finish_pixels_resized_crop_filtered_device",
    "zj_scaled_size", "zj_scaled_crop_out_len", "zj_decode_crops_scaled_device", "zj_decode_crops_resized_prescaled_device",
    "zj_decoder_finish_pixels_scaled_device", "zj_decoder_finish_pixels_resized_crop_prescaled_device",
    "zj_oriented_size", "zj_orient_window", "zj_orient_device", "zj_decode_crops_resized_oriented_device",
    "zj_decoder_orientation", "zj_decoder_finish_pixels_oriented_device",
    "zj_decoder_finish_pixels_resized_crop_oriented_device",
    "zj_decode_crops_resized_mixed_device", "zj_decoder_finish_pixels_resized_crop_batch_device",
    "zj_gray_to_rgb_device", "zj_cmyk_to_rgb_device", "zj_decoder_adobe_transform", "zj_decoder_plane",
    "zj_planes_to_rgb_device", "zj_decoder_stored_rgb", "zj_decoder_component_sampling",
    "zj_crop_tensor_out_len", "zj_decode_crops_tensor_device", "zj_decoder_finish_pixels_crop_tensor_device",
    "zj_decode_crops_tensor_mixed_device", "zj_decoder_finish_pixels_crop_tensor_batch_device",
    "zj_to_tensor_device", "zj_decoder_finish_pixels_crop_tensor_oriented_device",
    "zj_decoder_finish_pixels_crop_tensor_batch_oriented_device",
    "zj_warp_fixed", "zj_warp_source_window", "zj_warp_device", "zj_decode_crops_warped_device",
    "zj_decoder_finish_pixels_warped_device", "zj_decoder_finish_pixels_warped_batch_device",
    "zj_color_fixed", "zj_color_device", "zj_decode_crops_resized_mixed_colored_device",
    "zj_decoder_finish_pixels_resized_crop_batch_colored_device",
    "zj_histogram_device", "zj_tone_luts_device", "zj_lut_device", "zj_tone_device",
    "zj_decode_crops_resized_mixed_toned_device", "zj_decoder_finish_pixels_resized_crop_batch_toned_device",
]
SCATTER_MAX = 32  # ZJ_SCATTER_MAX: frames per launch of the scattered form


def abi_symbols():
    return list(ABI)


def lib_path():
    return os.path.join(_HERE, os.environ.get("ZJ_LIB", "libzjhip.so"))  # ZJ_LIB: A/B builds (tools/ab_lib.sh)


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (soname libamdhip64.so.7, asked for as `libamdhip64.so`);
    libzjhip.so asks for `libamdhip64.so.7` and otherwise brings in /opt/rocm's copy.  Two HIP runtimes in one process
    do not coexist: whichever initialises second reports "No HIP GPUs are available".  A process that uses both must
    therefore `import torch` BEFORE the first call into this module (bench.py and tests/conftest.py do), or set
    ZJ_TORCH_HIP=1, which opens the wheel's copy here (without importing torch) so that libzjhip.so binds to it by
    soname.  It is not the default: the runtime bundled with torch 2.10+rocm7.0 runs the three-stream host pipeline of
    zj_decode_planes at half the rate of ROCm 7.2's (5.9 k against 11.9 k megapixels/s for one 4096x4096 frame,
    tools/e2e.py), so torch-free processes keep the system runtime."""
    if not os.environ.get("ZJ_TORCH_HIP") or "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:  # noqa: BLE001 -- best effort; the plain load below still works without torch in the process
        pass


def lib():
    """Loads libzjhip.so; raises (never falls back) when it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise ImportError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C zune-jpeg_amd/csrc` (there is no CPU fallback)")
    _share_torch_hip_runtime()
    L = C.CDLL(p)
    vp, sz, i16p, i32p, u8p = C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p
    L.zj_strerror.restype = C.c_char_p
    L.zj_strerror.argtypes = [C.c_int]
    L.zj_last_error.restype = C.c_char_p
    L.zj_last_error.argtypes = [vp]
    L.zj_ctx_create.restype = vp
    L.zj_ctx_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.zj_ctx_destroy.argtypes = [vp]
    L.zj_default_ctx.restype = vp
    L.zj_plane_len.restype = sz
    L.zj_plane_len.argtypes = [C.POINTER(FrameDesc), C.c_int]
    L.zj_out_len.restype = sz
    L.zj_out_len.argtypes = [C.POINTER(FrameDesc)]
    L.zj_idct_strip.argtypes = [vp, i16p, sz, i32p, sz, sz, sz, i16p]
    for f in (L.zj_upsample_h, L.zj_upsample_v, L.zj_upsample_hv):
        f.argtypes = [vp, i16p, sz, i16p, sz]
    L.zj_ycbcr_to_rgb16.argtypes = [vp, i16p, i16p, i16p, u8p, sz, C.POINTER(sz)]
    L.zj_post_process_strip.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(sz), C.POINTER(Component),
                                        C.c_int, C.c_int, u8p, sz, sz]
    L.zj_decode_planes.argtypes = [vp, C.POINTER(FrameDesc), i16p, i16p, i16p, u8p]
    L.zj_decode_planes_batch.argtypes = [vp, C.POINTER(FrameDesc), sz, i16p, i16p, i16p, u8p]
    L.zj_decode_planes_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, vp]
    L.zj_time_decode_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, vp, C.c_int,
                                        C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_char_p)]
    L.zj_alloc_pinned.restype = vp
    L.zj_alloc_pinned.argtypes = [sz]
    L.zj_free_pinned.argtypes = [vp]
    L.zj_set_thread_device.argtypes = [C.c_int]
    L.zj_device_alloc.restype = vp
    L.zj_device_alloc.argtypes = [vp, sz]
    L.zj_device_free.argtypes = [vp, vp]
    L.zj_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    L.zj_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    L.zj_sync.argtypes = [vp]
    L.zj_choose_idct_func.restype = vp
    L.zj_choose_idct_func.argtypes = [C.c_int]
    L.zj_choose_upsample_func.restype = vp
    L.zj_choose_upsample_func.argtypes = [C.c_int, C.c_int, C.c_int]
    L.zj_choose_ycbcr_to_rgb_convert_func.restype = vp
    L.zj_choose_ycbcr_to_rgb_convert_func.argtypes = [C.c_int, C.c_int]
    L.zj_decoder_new.restype = vp
    L.zj_decoder_new.argtypes = [C.POINTER(Options)]
    L.zj_decoder_free.argtypes = [vp]
    L.zj_decoder_error.restype = C.c_char_p
    L.zj_decoder_error.argtypes = [vp]
    L.zj_decoder_read_headers.argtypes = [vp, vp, sz, C.POINTER(ImageInfo)]
    L.zj_decoder_decode_coefficients.argtypes = [vp, vp, sz, C.POINTER(FrameDesc), C.POINTER(C.c_void_p), C.POINTER(sz), C.POINTER(ImageInfo)]
    L.zj_decoder_decode_buffer.argtypes = [vp, vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(ImageInfo)]
    L.zj_decoder_parallel_segments.argtypes = [vp]
    L.zj_decoder_parallel_mcus.restype = C.c_longlong
    L.zj_decoder_parallel_mcus.argtypes = [vp]
    L.zj_decoder_set_num_threads.argtypes = [vp, C.c_int]
    L.zj_decoder_prepare.argtypes = [vp, vp, sz, C.POINTER(FrameDesc), C.POINTER(ImageInfo)]
    L.zj_decoder_finish_pixels.argtypes = [vp, vp, vp, sz, C.POINTER(sz)]
    L.zj_decoder_finish_pixels_device.argtypes = [vp, vp, vp, sz, C.POINTER(sz)]
    L.zj_decoder_scan_blob.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(sz)]
    L.zj_decoder_gpu_status.restype = C.c_uint
    L.zj_decoder_gpu_status.argtypes = [vp]
    L.zj_decode_scan.argtypes = [vp, C.POINTER(FrameDesc), vp, sz, vp, C.c_int, C.POINTER(C.c_uint)]
    L.zj_decode_planes_to_device.argtypes = [vp, C.POINTER(FrameDesc), i16p, i16p, i16p, vp]
    L.zj_scan_stats.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.zj_scan_planes.argtypes = [vp, vp, vp, vp, C.POINTER(sz)]
    L.zj_decode_scans.argtypes = [vp, sz, vp, vp, vp, vp, C.c_int, vp, vp]
    L.zj_decoder_finish_pixels_batch.argtypes = [vp, sz, vp, vp, vp, vp, C.c_int, vp]
    L.zj_device_memset.argtypes = [vp, vp, C.c_int, sz]
    L.zj_pool_create.restype = vp
    L.zj_pool_create.argtypes = [C.c_int, C.c_int, C.POINTER(Options), C.POINTER(C.c_int)]
    L.zj_pool_destroy.argtypes = [vp]
    L.zj_pool_threads.argtypes = [vp]
    L.zj_pool_error.restype = C.c_char_p
    L.zj_pool_error.argtypes = [vp]
    L.zj_pool_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(sz)]
    L.zj_pool_decode_files.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.zj_pool_decode_files_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.zj_set_pipeline.argtypes = [vp, C.c_int]
    L.zj_set_variant.argtypes = [vp, C.c_int]
    L.zj_variant_available.argtypes = [C.c_int]
    L.zj_decode_frames.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp]
    L.zj_decode_planes_device_strided.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, sz, sz, sz, vp]
    L.zj_decode_frames_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, vp]
    L.zj_pointer_device.argtypes = [vp]
    L.zj_crop_out_len.restype = sz
    L.zj_crop_out_len.argtypes = [C.POINTER(FrameDesc), C.c_uint, C.c_uint, C.c_uint]
    L.zj_decode_crops_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.c_uint, C.c_uint, vp, C.c_uint, vp]
    L.zj_decoder_finish_pixels_crop_device.argtypes = [vp, vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, vp, sz, C.c_uint,
                                                       C.POINTER(sz)]
    L.zj_resized_out_len.restype = sz
    L.zj_resized_out_len.argtypes = [C.POINTER(FrameDesc), C.c_uint, C.c_uint, C.c_int]
    L.zj_resize_device.argtypes = [vp, sz, vp, vp, vp, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.zj_decode_crops_resized_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.c_uint, C.c_uint, C.c_int,
                                                 C.c_int, vp, vp, vp, vp, vp]
    L.zj_decoder_finish_pixels_resized_crop_device.argtypes = [vp, vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                                               C.c_uint, C.c_int, C.c_int, vp, vp, C.c_int, vp, sz,
                                                               C.POINTER(sz)]
    L.zj_crop_tensor_out_len.restype = sz
    L.zj_crop_tensor_out_len.argtypes = [C.POINTER(FrameDesc), C.c_uint, C.c_uint, C.c_int]
    L.zj_decode_crops_tensor_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.c_uint, C.c_uint, C.c_int,
                                                C.c_int, vp, vp, vp, vp, vp]
    L.zj_decoder_finish_pixels_crop_tensor_device.argtypes = [vp, vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                              vp, vp, C.c_int, vp, sz, C.POINTER(sz)]
    L.zj_decode_crops_tensor_mixed_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, C.c_uint, C.c_uint, C.c_int, C.c_int, vp, vp, vp,
                                                      vp, vp]
    L.zj_decoder_finish_pixels_crop_tensor_batch_device.argtypes = [vp, sz, vp, vp, C.c_uint, C.c_uint, C.c_int, C.c_int, vp, vp,
                                                                    vp, vp, sz, vp]
    L.zj_decoder_finish_pixels_crop_tensor_oriented_device.argtypes = L.zj_decoder_finish_pixels_crop_tensor_device.argtypes
    L.zj_decoder_finish_pixels_crop_tensor_batch_oriented_device.argtypes = L.zj_decoder_finish_pixels_crop_tensor_batch_device.argtypes
    L.zj_to_tensor_device.argtypes = [vp, sz, vp, C.c_uint, C.c_uint, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.zj_warp_fixed.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.zj_warp_source_window.argtypes = [C.POINTER(C.c_int64), C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_uint),
                                        C.POINTER(C.c_int64)]
    L.zj_warp_device.argtypes = [vp, sz, vp, vp, vp, C.c_int, vp, C.c_uint, C.c_uint, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp]
    L.zj_decode_crops_warped_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                vp, vp, vp, C.c_int, vp, vp]
    L.zj_decoder_finish_pixels_warped_device.argtypes = [vp, vp, C.POINTER(C.c_double), C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                         vp, vp, vp, C.c_int, vp, sz, C.POINTER(sz)]
    L.zj_decoder_finish_pixels_warped_batch_device.argtypes = [vp, sz, vp, vp, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_int, vp, vp, vp,
                                                               C.c_int, vp, sz, vp]
    L.zj_resize_filtered_device.argtypes = [vp, sz, vp, vp, vp, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_int, vp, vp,
                                            vp, C.c_int, vp, vp]
    L.zj_decode_crops_resized_filtered_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.c_uint, C.c_uint,
                                                          C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp]
    L.zj_decoder_finish_pixels_resized_crop_filtered_device.argtypes = [vp, vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                                                        C.c_uint, C.c_uint, C.c_int, C.c_int, vp, vp, C.c_int,
                                                                        C.c_int, vp, sz, C.POINTER(sz)]
    L.zj_scaled_size.argtypes = [C.POINTER(FrameDesc), C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.zj_scaled_crop_out_len.restype = sz
    L.zj_scaled_crop_out_len.argtypes = [C.POINTER(FrameDesc), C.c_int, C.c_uint, C.c_uint, C.c_uint]
    L.zj_decode_crops_scaled_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, C.c_int, vp, vp, C.c_uint, vp]
    L.zj_decode_crops_resized_prescaled_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.c_uint, C.c_uint,
                                                           C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.zj_decoder_finish_pixels_scaled_device.argtypes = [vp, vp, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, vp, sz, C.c_uint,
                                                         C.POINTER(sz)]
    L.zj_decoder_finish_pixels_resized_crop_prescaled_device.argtypes = [vp, vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                                                         C.c_uint, C.c_uint, C.c_int, C.c_int, vp, vp, C.c_int,
                                                                         C.c_int, C.c_int, vp, sz, C.POINTER(sz)]
    L.zj_oriented_size.argtypes = [C.c_int, C.c_uint, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.zj_orient_window.argtypes = [C.c_int, C.c_uint, C.c_uint, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.zj_orient_device.argtypes = [vp, sz, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.zj_gray_to_rgb_device.argtypes = [vp, sz, vp, vp, vp, C.c_int, vp, vp, vp]
    L.zj_cmyk_to_rgb_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.zj_decoder_adobe_transform.argtypes = [vp]
    L.zj_planes_to_rgb_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.zj_decoder_stored_rgb.argtypes = [vp]
    L.zj_decoder_component_sampling.argtypes = [vp, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.zj_decoder_plane.argtypes = [vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(sz), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.zj_decode_crops_resized_oriented_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.c_uint, C.c_uint,
                                                          C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.zj_decoder_orientation.argtypes = [vp]
    L.zj_decoder_finish_pixels_oriented_device.argtypes = [vp, vp, vp, sz, C.POINTER(sz), C.POINTER(C.c_uint),
                                                           C.POINTER(C.c_uint)]
    L.zj_decoder_finish_pixels_resized_crop_oriented_device.argtypes = [vp, vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                                                        C.c_uint, C.c_uint, C.c_int, C.c_int, vp, vp, C.c_int,
                                                                        C.c_int, C.c_int, vp, sz, C.POINTER(sz)]
    L.zj_decode_crops_resized_mixed_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.c_uint, C.c_uint,
                                                       C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.zj_decoder_finish_pixels_resized_crop_batch_device.argtypes = [vp, sz, vp, vp, C.c_uint, C.c_uint, C.c_int, C.c_int, vp,
                                                                     vp, vp, C.c_int, C.c_int, C.c_int, vp, sz,
                                                                     C.POINTER(C.c_int)]
    L.zj_color_fixed.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.zj_color_device.argtypes = [vp, sz, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.zj_decode_crops_resized_mixed_colored_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.c_uint, C.c_uint,
                                                               C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.zj_decoder_finish_pixels_resized_crop_batch_colored_device.argtypes = [vp, sz, vp, vp, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                                             vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, sz,
                                                                             C.POINTER(C.c_int)]
    L.zj_histogram_device.argtypes = [vp, sz, vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.zj_tone_luts_device.argtypes = [vp, sz, C.c_int, vp, vp, vp, vp]
    L.zj_lut_device.argtypes = [vp, sz, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.zj_tone_device.argtypes = [vp, sz, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.zj_decode_crops_resized_mixed_toned_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.c_uint, C.c_uint,
                                                             C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.zj_decoder_finish_pixels_resized_crop_batch_toned_device.argtypes = [vp, sz, vp, vp, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                                                           vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, sz,
                                                                           C.POINTER(C.c_int)]
    L.zj_pool_create_multi.restype = vp
    L.zj_pool_create_multi.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(Options), C.POINTER(C.c_int)]
    L.zj_pool_devices.argtypes = [vp]
    L.zj_pool_device_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(sz)]
    L.zj_shard_range.restype = None
    L.zj_shard_range.argtypes = [sz, C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz)]
    L.zj_multi_create.restype = vp
    L.zj_multi_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    L.zj_multi_destroy.argtypes = [vp]
    L.zj_multi_devices.argtypes = [vp]
    L.zj_multi_ctx.restype = vp
    L.zj_multi_ctx.argtypes = [vp, C.c_int]
    L.zj_multi_slot_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(sz)]
    L.zj_multi_decode_planes_batch.argtypes = [vp, C.POINTER(FrameDesc), sz, i16p, i16p, i16p, u8p, C.POINTER(C.c_int)]
    L.zj_multi_decode_frames.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.zj_multi_decode_frames_device.argtypes = [vp, C.POINTER(FrameDesc), sz, vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.zj_frame_begin.argtypes = [vp, C.POINTER(FrameDesc), i16p, i16p, i16p, vp, C.c_int]
    L.zj_frame_rows_ready.argtypes = [vp, sz]
    L.zj_frame_end.argtypes = [vp]
    L.zj_frame_abort.argtypes = [vp]
    ip = C.POINTER(C.c_int)
    L.zj_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, sz]
    L.zj_device_numa_node.argtypes = [C.c_int]
    L.zj_bind_thread_to_numa_node.argtypes = [C.c_int]
    L.zj_bind_thread_near_device.argtypes = [C.c_int]
    L.zj_thread_numa_node.argtypes = []
    L.zj_pool_slot_numa.argtypes = [vp, C.c_int, ip, ip, ip]
    L.zj_multi_slot_numa.argtypes = [vp, C.c_int, ip, ip, ip]
    if hasattr(L, "zj_set_ablation"):  # diagnostic build only (tools/build_variant.sh ablate "-DZJ_ABLATION")
        L.zj_set_ablation.argtypes = [vp, C.c_int]
    _LIB = L
    return L


def crop_out_len(desc, w, h, out_pitch=0):
    """bytes of one w x h crop of frames of `desc` (zj_crop_out_len); 0: not a valid window"""
    return lib().zj_crop_out_len(C.byref(desc), w, h, out_pitch)


def resized_out_len(desc, out_w, out_h, dtype):
    """bytes of one out_w x out_h resized output of frames of `desc` (zj_resized_out_len); 0: not supported"""
    return lib().zj_resized_out_len(C.byref(desc), out_w, out_h, dtype)


def crop_tensor_out_len(desc, w, h, dtype):
    """bytes of one image of the tensor of w x h crops of frames of `desc` (zj_crop_tensor_out_len); 0: not supported"""
    return lib().zj_crop_tensor_out_len(C.byref(desc), w, h, dtype)


def scale_log2(scale):
    """1, 2, 4, 8 -> 0, 1, 2, 3 (a reduced decode's scale, a resize's max_prescale); anything else is a ValueError"""
    if scale not in (1, 2, 4, 8) or isinstance(scale, bool):
        raise ValueError(f"scale must be 1, 2, 4 or 8, not {scale!r}")
    return {1: 0, 2: 1, 4: 2, 8: 3}[scale]


def scaled_size(desc, scale):
    """(w, h) of frames of `desc` decoded at 1/scale (zj_scaled_size): ceil(width / scale) x ceil(height / scale)"""
    w, h = C.c_uint(0), C.c_uint(0)
    _check(lib().zj_scaled_size(C.byref(desc), scale_log2(scale), C.byref(w), C.byref(h)), "zj_scaled_size")
    return w.value, h.value


def scaled_crop_out_len(desc, scale, w, h, out_pitch=0):
    """bytes of a w x h window of the frame decoded at 1/scale (zj_scaled_crop_out_len); 0: not a valid size"""
    return lib().zj_scaled_crop_out_len(C.byref(desc), scale_log2(scale), w, h, out_pitch)


def oriented_size(orientation, w, h):
    """(w, h) of the displayed form of a stored w x h image under EXIF orientation 1..8 (zj_oriented_size)"""
    ow, oh = C.c_uint(0), C.c_uint(0)
    _check(lib().zj_oriented_size(int(orientation), w, h, C.byref(ow), C.byref(oh)), "zj_oriented_size")
    return ow.value, oh.value


def orient_window(orientation, frame_w, frame_h, window):
    """The window (x, y, w, h) of the DISPLAYED image of a stored frame_w x frame_h frame as a window of the stored one
    (zj_orient_window)"""
    win = (C.c_uint * 4)(*[int(v) for v in window])
    st = (C.c_uint * 4)()
    _check(lib().zj_orient_window(int(orientation), frame_w, frame_h, win, st), "zj_orient_window")
    return tuple(st)


WARP_FILL, WARP_REPLICATE = 0, 1  # ZJ_WARP_*


def warp_edge(edge):
    """"fill" / "replicate" (or the codes) -> ZJ_WARP_FILL / ZJ_WARP_REPLICATE"""
    try:
        return {"fill": WARP_FILL, "replicate": WARP_REPLICATE, WARP_FILL: WARP_FILL, WARP_REPLICATE: WARP_REPLICATE}[edge]
    except (KeyError, TypeError):
        raise ValueError(f'edge must be "fill" or "replicate", not {edge!r}') from None


def warp_fixed(matrix):
    """The six Q24 integers (A, B, C0, D, E, F0) of an affine matrix (a, b, c, d, e, f) that maps an output pixel centre to
    source coordinates (zj_warp_fixed); ZjError: an entry the warp refuses"""
    m = (C.c_double * 6)(*[float(v) for v in matrix])
    q = (C.c_int64 * 6)()
    _check(lib().zj_warp_fixed(m, q), "zj_warp_fixed")
    return [int(v) for v in q]


def warp_source_window(fixed, frame_w, frame_h, out_w, out_h, edge="fill"):
    """((x, y, w, h), shifted integers): the part of a frame_w x frame_h frame an out_w x out_h output under the integers
    `fixed` can read, and the integers relative to it (zj_warp_source_window); w = h = 0: the output is all fill"""
    q = (C.c_int64 * 6)(*[int(v) for v in fixed])
    win = (C.c_uint * 4)()
    sh = (C.c_int64 * 6)()
    _check(lib().zj_warp_source_window(q, frame_w, frame_h, out_w, out_h, warp_edge(edge), win, sh), "zj_warp_source_window")
    return tuple(int(v) for v in win), [int(v) for v in sh]


IDENTITY_COLOR = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def color_fixed(matrix):
    """The 12 integers floor(m * 65536 + 1/2) of a colour matrix, [3, 4] or 12 numbers (zj_color_fixed);
    ZjError: an entry the colour stage refuses"""
    m = (C.c_double * 12)(*_color_flat(matrix))
    q = (C.c_int32 * 12)()
    _check(lib().zj_color_fixed(m, q), "zj_color_fixed")
    return [int(v) for v in q]


def _color_flat(matrix):
    flat = [float(v) for row in matrix for v in (row if hasattr(row, "__len__") else (row,))]
    if len(flat) != 12:
        raise ValueError("a colour matrix is [3, 4]: 12 numbers")
    return flat


def _colors(matrices, n):
    """one colour matrix per image (None entries: the identity) as 12 n doubles; None: no colour"""
    if matrices is None:
        return None
    if len(matrices) != n:
        raise ValueError("one colour matrix per image")
    return (C.c_double * (12 * n))(*[v for m in matrices for v in (IDENTITY_COLOR if m is None else _color_flat(m))])


# ZJ_TONE_*: the ops of the tone stage
TONE_IDENTITY, TONE_INVERT, TONE_POSTERIZE, TONE_SOLARIZE, TONE_AUTOCONTRAST, TONE_EQUALIZE = 0, 1, 2, 3, 4, 5
TONE_OPS = {"identity": TONE_IDENTITY, "invert": TONE_INVERT, "posterize": TONE_POSTERIZE, "solarize": TONE_SOLARIZE,
            "autocontrast": TONE_AUTOCONTRAST, "equalize": TONE_EQUALIZE}


def _tones(ops, n):
    """one tone op per image, (op, param) pairs or None (the identity), as 2 n int32; None: no tone stage"""
    if ops is None:
        return None
    if len(ops) != n:
        raise ValueError("one tone op per image")
    return (C.c_int32 * (2 * n))(*[int(v) for op in ops for v in ((TONE_IDENTITY, 0) if op is None else tuple(op))])


def _matrices(matrices, n):
    if len(matrices) != n or any(len(m) != 6 for m in matrices):
        raise ValueError("one matrix of six numbers per image")
    return (C.c_double * (6 * n))(*[float(v) for m in matrices for v in m])


def _fill(fill):
    if fill is None:
        return None
    f = [int(v) for v in fill]
    if not 1 <= len(f) <= 3 or any(not 0 <= v <= 255 for v in f):
        raise ValueError("fill: one byte per channel")
    return (C.c_uint8 * 3)(*(f + [0] * (3 - len(f))))


def _floats(v):
    return (C.c_float * len(v))(*[float(x) for x in v]) if v is not None else None


def _wh(sizes):
    """(w, h) pairs as the unsigned array of a stage call"""
    return (C.c_uint * (2 * len(sizes)))(*[int(v) for s in sizes for v in s])


def _pit(v, n):
    """one pitch for each of n images (None: all tight)"""
    return (C.c_uint * n)(*[int(x) for x in v]) if v is not None else None


def _flips(v, n):
    if v is None:
        return None
    if len(v) != n:
        raise ValueError("one flip flag per image")
    return (C.c_uint8 * n)(*[1 if f else 0 for f in v])


def device_count():
    return lib().zj_device_count()


def _check(rc, what, ctx=None):
    if rc != OK:
        detail = what
        if rc == ERR_HIP and ctx is not None:
            detail = f"{what} ({lib().zj_last_error(ctx).decode()})"
        raise ZjError(rc, detail)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _i16(a):
    return np.ascontiguousarray(a, dtype=np.int16)


IDCT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                      C.c_size_t, C.c_void_p)
UPSAMPLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t)
CC16_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                      C.POINTER(C.c_size_t))


def _fn_or_raise(addr, proto, what):
    if not addr:
        raise ZjError(ERR_BACKEND, what)
    return proto(addr)


def choose_idct_func(backend=BACKEND_HIP):
    """src/idct.rs:40 -- returns the C function pointer of the chosen arm (HIP only)."""
    return _fn_or_raise(lib().zj_choose_idct_func(backend), IDCT_FN, "choose_idct_func")


def choose_upsample_func(backend, h_max, v_max):
    """Decoder::set_upsampling, src/decoder.rs:468-523."""
    return _fn_or_raise(lib().zj_choose_upsample_func(backend, h_max, v_max), UPSAMPLE_FN, "choose_upsample_func")


def choose_ycbcr_to_rgb_convert_func(backend, out_cs=ColorSpace.RGB):
    """src/color_convert.rs:61"""
    return _fn_or_raise(lib().zj_choose_ycbcr_to_rgb_convert_func(backend, int(out_cs)), CC16_FN,
                        "choose_ycbcr_to_rgb_convert_func")


class Context:
    """zj_ctx: one HIP stream + scratch buffers on one device."""

    def __init__(self, backend=BACKEND_HIP, device=0):
        st = C.c_int(0)
        self._h = lib().zj_ctx_create(backend, device, C.byref(st))
        if not self._h:
            raise ZjError(st.value, "zj_ctx_create")
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().zj_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # ---- strip level (fn-pointer compatible) -------------------------------------------------
    def idct_strip(self, coeff, qt, stride, samp_factors, v_samp):
        """IDCTPtr: dequantize_and_idct_int(vector, qt_table, stride, samp_factors, v_samp)."""
        coeff = _i16(coeff)
        qt = np.ascontiguousarray(qt, dtype=np.int32)
        out = np.empty(coeff.size, np.int16)
        _check(lib().zj_idct_strip(self._h, _ptr(coeff), coeff.size, _ptr(qt), stride, samp_factors, v_samp,
                                   _ptr(out)), "zj_idct_strip", self._h)
        return out

    def _ups(self, fn, inp, out_len, what):
        inp = _i16(inp)
        out = np.empty(out_len, np.int16)
        _check(fn(self._h, _ptr(inp), inp.size, _ptr(out), out_len), what, self._h)
        return out

    def upsample_horizontal(self, inp, output_len):
        return self._ups(lib().zj_upsample_h, inp, output_len, "zj_upsample_h")

    def upsample_vertical(self, inp, output_len):
        return self._ups(lib().zj_upsample_v, inp, output_len, "zj_upsample_v")

    def upsample_hv(self, inp, output_len):
        return self._ups(lib().zj_upsample_hv, inp, output_len, "zj_upsample_hv")

    def ycbcr_to_rgb_16(self, y, cb, cr, output, pos):
        """ColorConvert16Ptr; returns the new pos."""
        y, cb, cr = _i16(y), _i16(cb), _i16(cr)
        p = C.c_size_t(pos)
        _check(lib().zj_ycbcr_to_rgb16(self._h, _ptr(y), _ptr(cb), _ptr(cr), _ptr(output), output.size,
                                       C.byref(p)), "zj_ycbcr_to_rgb16", self._h)
        return p.value

    def post_process(self, coeff, comps, in_cs, out_cs, output, width):
        """post_process(coeff, component_data, .., input_colorspace, output_colorspace, output, width)"""
        arrs = [_i16(c) for c in coeff]
        while len(arrs) < 3:
            arrs.append(np.zeros(0, np.int16))
        ptrs = (C.c_void_p * 3)(*[a.ctypes.data if a.size else None for a in arrs])
        lens = (C.c_size_t * 3)(*[a.size for a in arrs])
        _check(lib().zj_post_process_strip(self._h, ptrs, lens, comps, int(in_cs), int(out_cs), _ptr(output),
                                           output.size, width), "zj_post_process_strip", self._h)

    # ---- frame level ---------------------------------------------------------------------------
    def decode_planes(self, desc, planes, nframes=1):
        arrs = [_i16(p) for p in planes]
        while len(arrs) < 3:
            arrs.append(np.zeros(8, np.int16))
        out = np.empty(nframes * lib().zj_out_len(C.byref(desc)), np.uint8)
        _check(lib().zj_decode_planes_batch(self._h, C.byref(desc), nframes, _ptr(arrs[0]), _ptr(arrs[1]),
                                            _ptr(arrs[2]), _ptr(out)), "zj_decode_planes_batch", self._h)
        return out

    def decode_planes_device(self, desc, nframes, d_y, d_cb, d_cr, d_out, stream=None):
        """Device pointers (ints), asynchronous on `stream` (int handle or None = ctx stream)."""
        _check(lib().zj_decode_planes_device(self._h, C.byref(desc), nframes, d_y, d_cb, d_cr, d_out, stream),
               "zj_decode_planes_device", self._h)

    def decode_planes_device_strided(self, desc, nframes, d_y, d_cb, d_cr, d_out, y_stride=0, c_stride=0, out_stride=0, stream=None):
        """Frames at a uniform distance (int16 elements for the planes, bytes for the pixels; 0 = packed): ONE launch."""
        _check(lib().zj_decode_planes_device_strided(self._h, C.byref(desc), nframes, d_y, d_cb, d_cr, d_out, y_stride, c_stride,
                                                     out_stride, stream), "zj_decode_planes_device_strided", self._h)

    def decode_frames_device(self, desc, d_y, d_cb, d_cr, d_out, stream=None):
        """Scattered batch: lists of device pointers (ints), one entry per frame, any order, independent allocations.
        d_cb / d_cr may be None for GRAYSCALE output.  Asynchronous on `stream`."""
        n = len(d_y)
        arr = lambda v: (C.c_void_p * n)(*v) if v is not None else None
        _check(lib().zj_decode_frames_device(self._h, C.byref(desc), n, arr(d_y), arr(d_cb), arr(d_cr), arr(d_out), stream),
               "zj_decode_frames_device", self._h)

    def decode_crops_device(self, desc, d_y, d_cb, d_cr, origins, crop_w, crop_h, d_out, out_pitch=0, stream=None):
        """Crop windows (zj_decode_crops_device): lists of device pointers as in decode_frames_device, origins = one (x, y)
        per frame, every window crop_w x crop_h; each output gets crop_out_len(desc, crop_w, crop_h, out_pitch) bytes.
        Asynchronous on `stream`."""
        n = len(d_y)
        if len(origins) != n or len(d_out) != n:
            raise ValueError("one origin and one output per frame")
        arr = lambda v: (C.c_void_p * n)(*v) if v is not None else None
        org = (C.c_uint * (2 * n))(*[int(v) for xy in origins for v in xy])
        _check(lib().zj_decode_crops_device(self._h, C.byref(desc), n, arr(d_y), arr(d_cb), arr(d_cr), org, crop_w, crop_h,
                                            arr(d_out), out_pitch, stream), "zj_decode_crops_device", self._h)

    def resize_device(self, d_in, sizes, channels, in_layout, out_w, out_h, dtype, out_layout, d_out, scale=None, bias=None,
                      flips=None, pitches=None, stream=None, antialias=False, interpolation="bilinear"):
        """Resize + normalise (zj_resize_device): d_in = device pointers of u8 images, sizes = one (w, h) each, pitches =
        bytes between rows (None: tight); the dense output at d_out.  antialias: the triangle filter
        (zj_resize_filtered_device, RESIZE_BILINEAR_AA); with interpolation="bicubic" the bicubic one (RESIZE_BICUBIC_AA,
        see resize_filter).  Asynchronous on `stream`."""
        filt = resize_filter(antialias, interpolation)
        n = len(d_in)
        if len(sizes) != n or (pitches is not None and len(pitches) != n):
            raise ValueError("one size (and pitch) per image")
        args = (self._h, n, (C.c_void_p * n)(*d_in), _wh(sizes), _pit(pitches, n), channels, in_layout, out_w, out_h, dtype,
                out_layout, _floats(scale), _floats(bias), _flips(flips, n))
        if filt != RESIZE_BILINEAR:
            _check(lib().zj_resize_filtered_device(*args, filt, d_out, stream), "zj_resize_filtered_device", self._h)
        else:
            _check(lib().zj_resize_device(*args, d_out, stream), "zj_resize_device", self._h)

    def to_tensor_device(self, d_in, w, h, in_channels, channels, dtype, out_layout, d_out, scale=None, bias=None, flips=None,
                         pitches=None, stream=None):
        """u8 images of ONE size into a normalised tensor, not resized (zj_to_tensor_device): d_in = device
        pointers of interleaved u8 images of w x h with in_channels (1 or 3), pitches = bytes between rows (None: tight);
        channels = the tensor's (1 or 3; 3 from 1 replicates); the dense output at d_out.  Asynchronous on `stream`."""
        n = len(d_in)
        if pitches is not None and len(pitches) != n:
            raise ValueError("one pitch per image")
        _check(lib().zj_to_tensor_device(self._h, n, (C.c_void_p * n)(*d_in), w, h, _pit(pitches, n), in_channels, channels, dtype,
                                         out_layout, _floats(scale), _floats(bias), _flips(flips, n), d_out, stream),
               "zj_to_tensor_device", self._h)

    def warp_device(self, d_in, sizes, channels, matrices, out_w, out_h, dtype, out_layout, d_out, scale=None, bias=None,
                    fill=None, edge="fill", pitches=None, stream=None):
        """Affine-warped images into a normalised tensor (zj_warp_device): d_in = device pointers of
        interleaved u8 images, sizes = one (w, h) each, matrices = one (a, b, c, d, e, f) each, output pixel centre -> source
        coordinates; fill = one byte per channel (None: 0), edge "fill" or "replicate"; pitches = bytes between rows
        (None: tight); the dense output at d_out.  Asynchronous on `stream`."""
        n = len(d_in)
        if len(sizes) != n or (pitches is not None and len(pitches) != n):
            raise ValueError("one size (and pitch) per image")
        _check(lib().zj_warp_device(self._h, n, (C.c_void_p * n)(*d_in), _wh(sizes), _pit(pitches, n), channels, _matrices(matrices, n),
                                    out_w, out_h, dtype, out_layout, _floats(scale), _floats(bias), _fill(fill), warp_edge(edge),
                                    d_out, stream),
               "zj_warp_device", self._h)

    def decode_crops_warped_device(self, desc, d_y, d_cb, d_cr, matrices, out_w, out_h, dtype, out_layout, d_out, scale=None,
                                   bias=None, fill=None, edge="fill", stream=None):
        """Frames of one geometry warped into a normalised tensor (zj_decode_crops_warped_device): pointers as in
        decode_crops_device, matrices = one per frame, in frame pixels; only the part of each frame its output can see is
        decoded.  The other arguments as warp_device.  Asynchronous on `stream`."""
        n = len(d_y)
        arr = lambda v: (C.c_void_p * n)(*v) if v is not None else None
        _check(lib().zj_decode_crops_warped_device(self._h, C.byref(desc), n, arr(d_y), arr(d_cb), arr(d_cr), _matrices(matrices, n),
                                                   out_w, out_h, dtype, out_layout, _floats(scale), _floats(bias), _fill(fill),
                                                   warp_edge(edge), d_out, stream),
               "zj_decode_crops_warped_device", self._h)

    def orient_device(self, d_in, sizes, channels, in_layout, orientations, d_out, in_pitches=None, out_pitches=None,
                      stream=None):
        """EXIF orientation (zj_orient_device): d_in = device pointers of u8 images, sizes = one STORED (w, h) each,
        orientations = one of 1..8 each (None: all 1, a copy), d_out = one device pointer each for the displayed image
        (oriented_size); pitches = bytes between rows (None: tight).  Input and output must not overlap.  Asynchronous
        on `stream`."""
        n = len(d_in)
        if len(sizes) != n or len(d_out) != n or (orientations is not None and len(orientations) != n):
            raise ValueError("one size, orientation and output per image")
        ori = (C.c_uint8 * n)(*[int(o) for o in orientations]) if orientations is not None else None
        _check(lib().zj_orient_device(self._h, n, (C.c_void_p * n)(*d_in), _wh(sizes), _pit(in_pitches, n), channels, in_layout, ori,
                                      (C.c_void_p * n)(*d_out), _pit(out_pitches, n), stream), "zj_orient_device", self._h)

    def gray_to_rgb_device(self, d_in, sizes, out_layout, d_out, in_pitches=None, out_pitches=None, stream=None):
        """One u8 plane each -> a 3-channel u8 image with R = G = B (zj_gray_to_rgb_device): d_in = device
        pointers of the planes, sizes = one (w, h) each, out_layout LAYOUT_HWC (pixels g g g) or LAYOUT_CHW (three planes),
        d_out = one device pointer each; pitches = bytes between rows (None: tight).  Input and output must not overlap.
        Asynchronous on `stream`."""
        n = len(d_in)
        if len(sizes) != n or len(d_out) != n:
            raise ValueError("one size and output per image")
        _check(lib().zj_gray_to_rgb_device(self._h, n, (C.c_void_p * n)(*d_in), _wh(sizes), _pit(in_pitches, n), out_layout,
                                           (C.c_void_p * n)(*d_out), _pit(out_pitches, n), stream), "zj_gray_to_rgb_device", self._h)

    def cmyk_to_rgb_device(self, d_a, d_k, sizes, layout, d_out, inverted=None, a_pitches=None, k_pitches=None, out_pitches=None,
                           stream=None):
        """One 3-channel u8 image a and one u8 plane k each -> the 3-channel u8 image (a * k + 127) // 255
        (zj_cmyk_to_rgb_device): d_a, d_k = device pointers, sizes = one (w, h) each, layout LAYOUT_HWC or
        LAYOUT_CHW of a and of the output, d_out = one device pointer each (d_a[i] itself with the same pitch: in place);
        inverted = one flag each (None: all 0): non-zero uses the samples as stored, 0 complements a and k first; pitches =
        bytes between rows (None: tight).  Asynchronous on `stream`."""
        n = len(d_a)
        if len(d_k) != n or len(sizes) != n or len(d_out) != n or (inverted is not None and len(inverted) != n):
            raise ValueError("one plane, size, inverted flag and output per image")
        inv = (C.c_uint8 * n)(*[1 if v else 0 for v in inverted]) if inverted is not None else None
        _check(lib().zj_cmyk_to_rgb_device(self._h, n, (C.c_void_p * n)(*d_a), (C.c_void_p * n)(*d_k), _wh(sizes), _pit(a_pitches, n),
                                           _pit(k_pitches, n), layout, inv, (C.c_void_p * n)(*d_out), _pit(out_pitches, n), stream),
               "zj_cmyk_to_rgb_device", self._h)

    def color_device(self, d_in, sizes, layout, matrices, d_out, in_pitches=None, out_pitches=None, stream=None):
        """One 3-channel u8 image each under its own colour matrix (zj_color_device): d_in = device pointers,
        sizes = one (w, h) each, layout LAYOUT_HWC or LAYOUT_CHW of the input and of the output, matrices = one [3, 4] each
        (None: the identity), d_out = one device pointer each (d_in[i] itself with the same pitch: in place); pitches = bytes
        between rows (None: tight).  Asynchronous on `stream`."""
        n = len(d_in)
        if len(sizes) != n or len(d_out) != n or matrices is None:
            raise ValueError("one size, matrix and output per image")
        _check(lib().zj_color_device(self._h, n, (C.c_void_p * n)(*d_in), _wh(sizes), _pit(in_pitches, n), layout,
                                     _colors(matrices, n), (C.c_void_p * n)(*d_out), _pit(out_pitches, n), stream),
               "zj_color_device", self._h)

    def histogram_device(self, d_in, sizes, channels, layout, d_hist, in_pitches=None, stream=None):
        """The histograms of u8 images (zj_histogram_device): d_in = device pointers, sizes = one (w, h) each,
        channels 1 or 3, layout LAYOUT_HWC or LAYOUT_CHW, d_hist = device pointer of uint32 [n][channels][256] (overwritten).
        Asynchronous on `stream`."""
        n = len(d_in)
        if len(sizes) != n:
            raise ValueError("one size per image")
        wh = (C.c_uint * (2 * n))(*[int(v) for s in sizes for v in s])
        pit = (C.c_uint * n)(*[int(x) for x in in_pitches]) if in_pitches is not None else None
        _check(lib().zj_histogram_device(self._h, n, (C.c_void_p * n)(*d_in), wh, pit, channels, layout, d_hist, stream),
               "zj_histogram_device", self._h)

    def tone_luts_device(self, ops, channels, d_hist, d_luts, stream=None):
        """The tables of tone ops (zj_tone_luts_device): ops = one (op, param) each, d_hist = device pointer of uint32
        [n][channels][256] (None when no op is autocontrast or equalize), d_luts = device pointer of uint8 [n][channels][256]."""
        n = len(ops)
        _check(lib().zj_tone_luts_device(self._h, n, channels, _tones(ops, n), d_hist, d_luts, stream), "zj_tone_luts_device", self._h)

    def lut_device(self, d_in, sizes, channels, layout, d_luts, d_out, in_pitches=None, out_pitches=None, stream=None):
        """u8 images through their own tables, out[c] = luts[i][c][in[c]] (zj_lut_device): d_luts = device pointer of uint8
        [n][channels][256]; d_out[i] may be d_in[i] with the same pitch.  Asynchronous on `stream`."""
        n = len(d_in)
        if len(sizes) != n or len(d_out) != n:
            raise ValueError("one size and output per image")
        wh = (C.c_uint * (2 * n))(*[int(v) for s in sizes for v in s])
        pit = lambda v: (C.c_uint * n)(*[int(x) for x in v]) if v is not None else None
        _check(lib().zj_lut_device(self._h, n, (C.c_void_p * n)(*d_in), wh, pit(in_pitches), channels, layout, d_luts,
                                   (C.c_void_p * n)(*d_out), pit(out_pitches), stream), "zj_lut_device", self._h)

    def tone_device(self, d_in, sizes, channels, layout, ops, d_out, in_pitches=None, out_pitches=None, stream=None):
        """u8 images each under its own tone op (zj_tone_device): ops = one (op, param) each (None: the
        identity); histogram, table build and lookup on `stream`, nothing synchronised.  d_out[i] may be d_in[i] with the same
        pitch; an identity image that is its own output costs no launch."""
        n = len(d_in)
        if len(sizes) != n or len(d_out) != n or ops is None:
            raise ValueError("one size, op and output per image")
        wh = (C.c_uint * (2 * n))(*[int(v) for s in sizes for v in s])
        pit = lambda v: (C.c_uint * n)(*[int(x) for x in v]) if v is not None else None
        _check(lib().zj_tone_device(self._h, n, (C.c_void_p * n)(*d_in), wh, pit(in_pitches), channels, layout, _tones(ops, n),
                                    (C.c_void_p * n)(*d_out), pit(out_pitches), stream), "zj_tone_device", self._h)

    def planes_to_rgb_device(self, d_p0, d_p1, d_p2, sizes, ratios, layout, d_out, stored_rgb=False, pitches=None,
                             out_pitches=None, stream=None):
        """Three u8 component planes per image, each at its own resolution -> the 3-channel u8 image whose pixel (r, c) is
        colour(p0[r // ry0][c // rx0], p1[...], p2[...]) (zj_planes_to_rgb_device): d_p0, d_p1, d_p2 =
        device pointers, sizes = one (w, h) of the OUTPUT each, ratios = ((rx0, ry0), (rx1, ry1), (rx2, ry2)) each, every
        ratio 1, 2 or 4 (plane k holds ceil(w / rx_k) x ceil(h / ry_k) samples), layout LAYOUT_HWC or LAYOUT_CHW of the
        output, d_out = one device pointer each; stored_rgb: the planes are R, G, B as they are, not Y, Cb, Cr; pitches =
        three per image, out_pitches = one per image, bytes between rows (None: tight).  Asynchronous on `stream`."""
        n = len(d_p0)
        if len(d_p1) != n or len(d_p2) != n or len(sizes) != n or len(ratios) != n or len(d_out) != n:
            raise ValueError("three planes, a size, three ratio pairs and an output per image")
        flat = [int(v) for r in ratios for pair in r for v in pair]
        if len(flat) != 6 * n or any(v < 0 or v > 255 for v in flat):
            raise ValueError("ratios: three (rx, ry) pairs per image")
        rt = (C.c_uint8 * (6 * n))(*flat)
        pit = (C.c_uint * (3 * n))(*[int(v) for p in pitches for v in p]) if pitches is not None else None
        _check(lib().zj_planes_to_rgb_device(self._h, n, (C.c_void_p * n)(*d_p0), (C.c_void_p * n)(*d_p1), (C.c_void_p * n)(*d_p2),
                                             _wh(sizes), rt, pit, 1 if stored_rgb else 0, layout, (C.c_void_p * n)(*d_out),
                                             _pit(out_pitches, n), stream),
               "zj_planes_to_rgb_device", self._h)

    def decode_crops_resized_device(self, desc, d_y, d_cb, d_cr, windows, out_w, out_h, dtype, out_layout, d_out, scale=None,
                                    bias=None, flips=None, stream=None, antialias=False, max_prescale=1, orientations=None,
                                    interpolation="bilinear"):
        """Resized crop windows (zj_decode_crops_resized_device): pointers as in decode_crops_device, windows = one
        (x, y, w, h) per frame; the dense output at d_out.  antialias: the triangle filter
        (zj_decode_crops_resized_filtered_device, RESIZE_BILINEAR_AA).  max_prescale = 2, 4, 8: a reduced-size decode of
        up to that scale under the resize wherever it does not enlarge (zj_decode_crops_resized_prescaled_device); 1: none,
        today's bytes.  orientations: one EXIF orientation 1..8 per frame, the windows then in DISPLAYED pixels
        (zj_decode_crops_resized_oriented_device); None: today's call.  interpolation="bicubic" (with antialias=True):
        RESIZE_BICUBIC_AA in the same calls (see resize_filter).  Asynchronous on `stream`."""
        filt = resize_filter(antialias, interpolation)
        n = len(d_y)
        scale_log2(max_prescale)
        if len(windows) != n:
            raise ValueError("one window per frame")
        arr = lambda v: (C.c_void_p * n)(*v) if v is not None else None
        win = (C.c_uint * (4 * n))(*[int(v) for w in windows for v in w])
        args = (self._h, C.byref(desc), n, arr(d_y), arr(d_cb), arr(d_cr), win, out_w, out_h, dtype, out_layout,
                _floats(scale), _floats(bias), _flips(flips, n))
        if orientations is not None:
            if len(orientations) != n:
                raise ValueError("one orientation per frame")
            ori = (C.c_uint8 * n)(*[int(o) for o in orientations])
            _check(lib().zj_decode_crops_resized_oriented_device(*args, filt, scale_log2(max_prescale), ori, d_out, stream),
                   "zj_decode_crops_resized_oriented_device", self._h)
        elif max_prescale != 1:
            _check(lib().zj_decode_crops_resized_prescaled_device(*args, filt, scale_log2(max_prescale), d_out, stream),
                   "zj_decode_crops_resized_prescaled_device", self._h)
        elif filt != RESIZE_BILINEAR:
            _check(lib().zj_decode_crops_resized_filtered_device(*args, filt, d_out, stream),
                   "zj_decode_crops_resized_filtered_device", self._h)
        else:
            _check(lib().zj_decode_crops_resized_device(*args, d_out, stream), "zj_decode_crops_resized_device", self._h)

    def decode_crops_tensor_device(self, desc, d_y, d_cb, d_cr, origins, w, h, dtype, out_layout, d_out, scale=None, bias=None,
                                   flips=None, stream=None):
        """Crop windows straight into a normalised tensor, not resized (zj_decode_crops_tensor_device): pointers and
        origins as in decode_crops_device, every window w x h; the dense output at d_out, image f of crop_tensor_out_len
        bytes.  dtype, out_layout, scale, bias, flips as decode_crops_resized_device.  Asynchronous on `stream`."""
        n = len(d_y)
        if len(origins) != n:
            raise ValueError("one origin per frame")
        arr = lambda v: (C.c_void_p * n)(*v) if v is not None else None
        org = (C.c_uint * (2 * n))(*[int(v) for xy in origins for v in xy])
        _check(lib().zj_decode_crops_tensor_device(self._h, C.byref(desc), n, arr(d_y), arr(d_cb), arr(d_cr), org, w, h, dtype,
                                                   out_layout, _floats(scale), _floats(bias), _flips(flips, n), d_out, stream),
               "zj_decode_crops_tensor_device", self._h)

    def decode_crops_tensor_mixed_device(self, descs, d_y, d_cb, d_cr, origins, w, h, dtype, out_layout, d_out, scale=None,
                                         bias=None, flips=None, stream=None):
        """Crop windows of frames of MIXED geometry straight into a normalised tensor (zj_decode_crops_tensor_mixed_device):
        descs = one FrameDesc per frame (out_colorspace and out_layout the same in all), every window w x h; the other
        arguments as decode_crops_tensor_device.  Image f equals that call's for frame f alone.  Asynchronous on `stream`."""
        n = len(d_y)
        if len(descs) != n or len(origins) != n:
            raise ValueError("one descriptor and origin per frame")
        arr = lambda v: (C.c_void_p * n)(*v) if v is not None else None
        org = (C.c_uint * (2 * n))(*[int(v) for xy in origins for v in xy])
        darr = (FrameDesc * n)(*descs)
        _check(lib().zj_decode_crops_tensor_mixed_device(self._h, darr, n, arr(d_y), arr(d_cb), arr(d_cr), org, w, h, dtype,
                                                         out_layout, _floats(scale), _floats(bias), _flips(flips, n), d_out,
                                                         stream),
               "zj_decode_crops_tensor_mixed_device", self._h)

    def decode_crops_resized_mixed_device(self, descs, d_y, d_cb, d_cr, windows, out_w, out_h, dtype, out_layout, d_out,
                                          scale=None, bias=None, flips=None, stream=None, antialias=False, max_prescale=1,
                                          orientations=None, interpolation="bilinear", colors=None, tones=None):
        """Resized crop windows of frames of MIXED geometry (zj_decode_crops_resized_mixed_device): descs = one FrameDesc
        per frame (sizes, sampling, tables, flags and in_components their own; out_colorspace and out_layout the same in
        all); the other arguments as decode_crops_resized_device.  Image f equals that call's for frame f alone.
        colors: one [3, 4] colour matrix per frame (None entries: the identity), the u8 image under it in front of the
        resize (zj_decode_crops_resized_mixed_colored_device); None: today's call.
        tones: one (op, param) tone op per frame (None entries: the identity), the same image under it behind the colour
        matrix (zj_decode_crops_resized_mixed_toned_device); None: no tone stage.
        Asynchronous on `stream`."""
        filt = resize_filter(antialias, interpolation)
        n = len(d_y)
        if len(descs) != n or len(windows) != n or (orientations is not None and len(orientations) != n):
            raise ValueError("one descriptor, window (and orientation) per frame")
        arr = lambda v: (C.c_void_p * n)(*v) if v is not None else None
        win = (C.c_uint * (4 * n))(*[int(v) for w in windows for v in w])
        ori = (C.c_uint8 * n)(*[int(o) for o in orientations]) if orientations is not None else None
        if tones is not None:
            _check(lib().zj_decode_crops_resized_mixed_toned_device(
                self._h, (FrameDesc * n)(*descs), n, arr(d_y), arr(d_cb), arr(d_cr), win, out_w, out_h, dtype, out_layout,
                _floats(scale), _floats(bias), _flips(flips, n), filt, scale_log2(max_prescale), ori, _colors(colors, n),
                _tones(tones, n), d_out, stream), "zj_decode_crops_resized_mixed_toned_device", self._h)
            return
        if colors is not None:
            _check(lib().zj_decode_crops_resized_mixed_colored_device(
                self._h, (FrameDesc * n)(*descs), n, arr(d_y), arr(d_cb), arr(d_cr), win, out_w, out_h, dtype, out_layout,
                _floats(scale), _floats(bias), _flips(flips, n), filt, scale_log2(max_prescale), ori, _colors(colors, n), d_out,
                stream), "zj_decode_crops_resized_mixed_colored_device", self._h)
            return
        _check(lib().zj_decode_crops_resized_mixed_device(self._h, (FrameDesc * n)(*descs), n, arr(d_y), arr(d_cb), arr(d_cr), win,
                                                          out_w, out_h, dtype, out_layout, _floats(scale), _floats(bias),
                                                          _flips(flips, n), filt, scale_log2(max_prescale), ori, d_out, stream),
               "zj_decode_crops_resized_mixed_device", self._h)

    def decode_crops_scaled_device(self, desc, d_y, d_cb, d_cr, scale, d_out, windows=None, out_pitch=0, stream=None):
        """Reduced-size decode (zj_decode_crops_scaled_device): the frames at 1/scale (2, 4 or 8), pointers as in
        decode_crops_device, windows = one (x, y, w, h) per frame in reduced pixels (None: the whole reduced frame); each
        output gets scaled_crop_out_len(desc, scale, w, h, out_pitch) bytes.  Asynchronous on `stream`."""
        n = len(d_y)
        k = scale_log2(scale)
        if len(d_out) != n or (windows is not None and len(windows) != n):
            raise ValueError("one output (and window) per frame")
        arr = lambda v: (C.c_void_p * n)(*v) if v is not None else None
        win = (C.c_uint * (4 * n))(*[int(v) for w in windows for v in w]) if windows is not None else None
        _check(lib().zj_decode_crops_scaled_device(self._h, C.byref(desc), n, arr(d_y), arr(d_cb), arr(d_cr), k, win, arr(d_out),
                                                   out_pitch, stream), "zj_decode_crops_scaled_device", self._h)

    def decode_frames(self, desc, frames_planes, outs=None):
        """Host frames that are independent allocations (zj_decode_frames): frames_planes[f] = [y, cb, cr] arrays of frame
        f.  Returns the list of per-frame uint8 arrays."""
        n = len(frames_planes)
        arrs = [[_i16(p) for p in pl] for pl in frames_planes]
        nc = max(len(a) for a in arrs)
        if outs is None:
            outs = [np.empty(lib().zj_out_len(C.byref(desc)), np.uint8) for _ in range(n)]
        tab = [(C.c_void_p * n)(*[a[c].ctypes.data for a in arrs]) if c < nc else None for c in range(3)]
        otab = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        _check(lib().zj_decode_frames(self._h, C.byref(desc), n, tab[0], tab[1], tab[2], otab), "zj_decode_frames", self._h)
        return outs

    def decode_to_tensor(self, desc, y, cb=None, cr=None, out=None):
        """Device-resident in, device-resident out, for PyTorch-ROCm consumers: y / cb / cr are int16
        CUDA tensors holding N frames of coefficient planes back to back; returns a uint8 CUDA tensor shaped
        [N, C, H, W] when desc.out_layout is LAYOUT_CHW, else [N, H, W, C].  Runs on torch's current stream."""
        import torch
        ylen = lib().zj_plane_len(C.byref(desc), 0)
        n = y.numel() // ylen
        assert n >= 1 and y.numel() == n * ylen and y.dtype == torch.int16 and y.is_cuda
        nc = ColorSpace(desc.out_colorspace).num_components()
        shape = (n, nc, desc.height, desc.width) if desc.out_layout == LAYOUT_CHW else (n, desc.height, desc.width, nc)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=y.device)
        assert out.is_contiguous() and out.numel() == n * lib().zj_out_len(C.byref(desc))
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.decode_planes_device(desc, n, ptr(y), ptr(cb), ptr(cr), out.data_ptr(), torch.cuda.current_stream(y.device).cuda_stream)
        return out

    # ---- one frame whose planes are still being written (zj_frame_*): pointers are raw addresses, the caller keeps them alive
    def frame_begin(self, desc, y, cb, cr, out, out_on_device=False):
        _check(lib().zj_frame_begin(self._h, C.byref(desc), y, cb, cr, out, 1 if out_on_device else 0), "zj_frame_begin", self._h)

    def frame_rows_ready(self, mcu_rows):
        _check(lib().zj_frame_rows_ready(self._h, int(mcu_rows)), "zj_frame_rows_ready", self._h)

    def frame_end(self):
        _check(lib().zj_frame_end(self._h), "zj_frame_end", self._h)

    def frame_abort(self):
        _check(lib().zj_frame_abort(self._h), "zj_frame_abort", self._h)

    def time_decode_device(self, desc, nframes, d_y, d_cb, d_cr, d_out, iters, stream=None):
        """HIP-event timing on the launch stream.  Returns (ms per launch from `iters` back-to-back
        launches, mean ms of individually bracketed launches, kernel name)."""
        ms, each = C.c_float(0), C.c_float(0)
        name = C.c_char_p()
        _check(lib().zj_time_decode_device(self._h, C.byref(desc), nframes, d_y, d_cb, d_cr, d_out, stream,
                                           iters, C.byref(ms), C.byref(each), C.byref(name)),
               "zj_time_decode_device", self._h)
        return ms.value / iters, each.value, (name.value or b"").decode()

    def set_variant(self, variant):
        """Kernel variant: 0 = packed generation (dot2 IDCT under an exact guard, byte luma staging, staged stores;
        the default), 1 = wide generation (round 1's kernel), 2 = packed with direct stores.  All are bit-exact."""
        _check(lib().zj_set_variant(self._h, int(variant)), "zj_set_variant", self._h)

    def set_pipeline(self, on):
        """zj_decode_planes_batch: 1 (default) = units of ~8 MB overlapped over three streams, 0 = one unit."""
        _check(lib().zj_set_pipeline(self._h, int(bool(on))), "zj_set_pipeline", self._h)

    def set_ablation(self, mask):
        """Diagnostic build only (ZJ_LIB=libzjhip_ablate.so): bit 0 skips the IDCT, bit 1 the colour math (output is
        wrong when set).  The product library has no such switch."""
        if not hasattr(lib(), "zj_set_ablation"):
            raise ZjError(ERR_ARG, "zj_set_ablation: not in this build (tools/build_variant.sh ablate \"-DZJ_ABLATION\")")
        _check(lib().zj_set_ablation(self._h, int(mask)), "zj_set_ablation", self._h)

    def device_alloc(self, nbytes):
        p = lib().zj_device_alloc(self._h, nbytes)
        if not p:
            raise ZjError(ERR_NOMEM, "zj_device_alloc")
        return p

    def device_free(self, p):
        lib().zj_device_free(self._h, p)

    def h2d(self, dst, arr):
        arr = np.ascontiguousarray(arr)
        _check(lib().zj_memcpy_h2d(self._h, dst, _ptr(arr), arr.nbytes), "zj_memcpy_h2d", self._h)

    def d2h(self, arr, src):
        _check(lib().zj_memcpy_d2h(self._h, _ptr(arr), src, arr.nbytes), "zj_memcpy_d2h", self._h)

    def sync(self):
        _check(lib().zj_sync(self._h), "zj_sync", self._h)

    def scan_stats(self):
        """(synchronisation rounds, [ms upload + rounds, ms prefix sums + write pass, ms pixel kernel + download, host ms
        spent submitting]) of the last scan the GPU entropy stage decoded on this context; the device times need
        ZJ_HUFF_TIME in the environment."""
        r = C.c_int(0)
        ms = (C.c_float * 4)()
        _check(lib().zj_scan_stats(self._h, C.byref(r), ms), "zj_scan_stats", self._h)
        return r.value, [float(x) for x in ms]

    def scan_planes(self):
        """The coefficient planes the last decode_scan / device-entropy decode on this context left in HBM (copies)."""
        lens = (C.c_size_t * 3)()
        _check(lib().zj_scan_planes(self._h, None, None, None, lens), "zj_scan_planes", self._h)
        planes = [np.zeros(max(int(n), 1), np.int16) for n in lens]
        _check(lib().zj_scan_planes(self._h, _ptr(planes[0]), _ptr(planes[1]) if lens[1] else None,
                                    _ptr(planes[2]) if lens[2] else None, lens), "zj_scan_planes", self._h)
        return [p[: int(n)] for p, n in zip(planes, lens) if n]

    def decode_scan(self, desc, blob, out=None, device_out=None):
        """zj_decode_scan: a prepared scan -> pixels (host array, or a device pointer with device_out).  Returns
        (pixels or None, return code, status bits)."""
        blob = np.ascontiguousarray(blob, np.uint8)
        st = C.c_uint(0)
        if device_out is not None:
            rc = lib().zj_decode_scan(self._h, C.byref(desc), _ptr(blob), blob.size, device_out, 1, C.byref(st))
            return None, rc, st.value
        if out is None:
            out = np.zeros(lib().zj_out_len(C.byref(desc)), np.uint8)
        rc = lib().zj_decode_scan(self._h, C.byref(desc), _ptr(blob), blob.size, _ptr(out), 0, C.byref(st))
        if rc < 0:
            _check(rc, "zj_decode_scan", self._h)
        return out, rc, st.value


class DecodeError(ZjError):
    """Mirrors DecodeErrors (src/errors.rs:16-43): .status is the variant, str() carries the text."""

    def __init__(self, status, text):
        RuntimeError.__init__(self, f"[zj status {status}] {text}")
        self.status = status
        self.text = text


class Decoder:
    """Mirror of zune_jpeg::Decoder (src/decoder.rs:60): CPU entropy decode + GPU pixel path."""

    def __init__(self, options=None, ctx=None):
        o = options.to_c() if options is not None else Options()
        self._d = lib().zj_decoder_new(C.byref(o))
        self._out_cs = int(o.out_colorspace)
        self._ctx = ctx
        self._info = None

    def close(self):
        if getattr(self, "_d", None):
            lib().zj_decoder_free(self._d)
            self._d = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc):
        raise DecodeError(rc, lib().zj_decoder_error(self._d).decode(errors="replace"))

    def parallel_segments(self):
        """Restart segments the last baseline scan decoded concurrently (0 = serial walk)."""
        return lib().zj_decoder_parallel_segments(self._d)

    def parallel_mcus(self):
        """MCUs of the last baseline scan without restart markers that several threads decoded (0 = serial walk)."""
        return int(lib().zj_decoder_parallel_mcus(self._d))

    def set_num_threads(self, threads):  # decoder.rs:591-603 (deprecated there: options are the way)
        rc = lib().zj_decoder_set_num_threads(self._d, int(threads))
        if rc:
            self._raise(rc)

    def read_headers(self, buf):  # decoder.rs:452
        b = np.frombuffer(bytes(buf), np.uint8)
        info = ImageInfo()
        rc = lib().zj_decoder_read_headers(self._d, _ptr(b), b.size, C.byref(info))
        if rc:
            self._raise(rc)
        self._info = info
        return info

    def info(self):  # decoder.rs:210
        return self._info

    def decode_coefficients(self, buf, copy=True):
        """CPU half only: (FrameDesc, [planes], ImageInfo).  The planes are copies (copy=False: views of the decoder's own
        planes, valid until its next call or its end).  NOT for timing the walker: the copy of the planes -- 199 MB for a
        7680 x 4320 4:4:4 file -- costs more than the Huffman stage; prepare() leaves the planes where they are
        (tools/walker_bench.py)."""
        b = np.frombuffer(bytes(buf), np.uint8)
        desc, info = FrameDesc(), ImageInfo()
        ptrs = (C.c_void_p * 3)()
        lens = (C.c_size_t * 3)()
        rc = lib().zj_decoder_decode_coefficients(self._d, _ptr(b), b.size, C.byref(desc), ptrs, lens, C.byref(info))
        if rc:
            self._raise(rc)
        planes = [np.ctypeslib.as_array(C.cast(ptrs[c], C.POINTER(C.c_int16)), shape=(lens[c],))
                  for c in range(min(3, info.components))]  # (a four-component file: components 1-3; plane(3) gives the fourth)
        if copy:
            planes = [p.copy() for p in planes]
        self._info = info
        return desc, planes, info

    def prepare(self, buf):
        """Stage 1 (CPU) as the options ask: (FrameDesc, ImageInfo).  With a GPU entropy setting a baseline scan is
        only prepared (scan_blob() then returns it); `buf` is kept alive by this object until the next call."""
        self._src = np.frombuffer(bytes(buf), np.uint8)
        desc, info = FrameDesc(), ImageInfo()
        rc = lib().zj_decoder_prepare(self._d, _ptr(self._src), self._src.size, C.byref(desc), C.byref(info))
        if rc:
            self._raise(rc)
        self._info = info
        return desc, info

    def scan_blob(self):
        """The prepared scan (csrc/zj_huff.h) of the last prepare() as a uint8 array, or None."""
        p, n = C.c_void_p(), C.c_size_t(0)
        if lib().zj_decoder_scan_blob(self._d, C.byref(p), C.byref(n)):
            return None
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).copy()

    def gpu_status(self):
        """HUFF_ST bits with which the device handed the last scan back to the CPU walker (0: it kept it)."""
        return int(lib().zj_decoder_gpu_status(self._d))

    def finish_pixels(self, out=None):
        """Stage 2 after prepare() / decode_coefficients(): the pixels as a uint8 array."""
        if self._ctx is None:
            self._ctx = Context()
        info = self._info
        ncomp = 1 if info.components == 1 else ColorSpace(self._out_cs).num_components()
        if out is None:
            out = np.zeros(int(info.width) * int(info.height) * ncomp, np.uint8)
        n = C.c_size_t(0)
        rc = lib().zj_decoder_finish_pixels(self._d, self._ctx.handle, _ptr(out), out.size, C.byref(n))
        if rc:
            self._raise(rc)
        return out[: n.value]

    def finish_pixels_crop_device(self, x, y, w, h, d_out, cap, out_pitch=0):
        """Stage 2 cut to the w x h window at (x, y), pixels left in HBM at device pointer d_out (the contract of
        zj_decode_crops_device); returns the crop's length in bytes."""
        if self._ctx is None:
            self._ctx = Context()
        n = C.c_size_t(0)
        rc = lib().zj_decoder_finish_pixels_crop_device(self._d, self._ctx.handle, x, y, w, h, d_out, cap, out_pitch, C.byref(n))
        if rc:
            self._raise(rc)
        return n.value

    def finish_pixels_crop_tensor_device(self, x, y, w, h, dtype, out_layout, d_out, cap, scale=None, bias=None, flip=False,
                                         apply_orientation=False):
        """Stage 2 cut to the w x h window at (x, y) and converted into one image of a normalised tensor, not resized (the
        contract of zj_decode_crops_tensor_device), left in HBM at device pointer d_out; returns the image's length in
        bytes.  apply_orientation: the window is in DISPLAYED pixels of the file's EXIF orientation
        (zj_decoder_finish_pixels_crop_tensor_oriented_device)."""
        if self._ctx is None:
            self._ctx = Context()
        n = C.c_size_t(0)
        fn = (lib().zj_decoder_finish_pixels_crop_tensor_oriented_device if apply_orientation
              else lib().zj_decoder_finish_pixels_crop_tensor_device)
        rc = fn(self._d, self._ctx.handle, x, y, w, h, dtype, out_layout, _floats(scale), _floats(bias), 1 if flip else 0, d_out, cap,
                C.byref(n))
        if rc:
            self._raise(rc)
        return n.value

    def finish_pixels_warped_device(self, matrix, out_w, out_h, dtype, out_layout, d_out, cap, scale=None, bias=None, fill=None,
                                    edge="fill", apply_orientation=False):
        """Stage 2 warped under the affine `matrix` (a, b, c, d, e, f: output pixel centre -> frame coordinates) into one image
        of a normalised tensor (zj_decoder_finish_pixels_warped_device), left in HBM at device pointer d_out;
        returns the image's length in bytes.  Only the part of the frame the output sees is decoded.  apply_orientation: the
        matrix is in DISPLAYED pixels of the file's EXIF orientation."""
        if self._ctx is None:
            self._ctx = Context()
        n = C.c_size_t(0)
        m = (C.c_double * 6)(*[float(v) for v in matrix])
        rc = lib().zj_decoder_finish_pixels_warped_device(self._d, self._ctx.handle, m, 1 if apply_orientation else 0, out_w, out_h,
                                                          dtype, out_layout, _floats(scale), _floats(bias), _fill(fill),
                                                          warp_edge(edge), d_out, cap, C.byref(n))
        if rc:
            self._raise(rc)
        return n.value

    def finish_pixels_scaled_device(self, scale, d_out, cap, window=None, out_pitch=0):
        """Stage 2 at 1/scale (2, 4 or 8), cut to window = (x, y, w, h) of the reduced frame (None: all of it), pixels left
        in HBM at device pointer d_out (the contract of zj_decode_crops_scaled_device); returns the length in bytes."""
        if self._ctx is None:
            self._ctx = Context()
        k = scale_log2(scale)
        if k == 0:
            raise ValueError("scale must be 2, 4 or 8")
        x, y, w, h = window if window is not None else (0, 0, 0, 0)
        if window is not None and (w == 0 or h == 0):
            raise ValueError("an empty window")
        n = C.c_size_t(0)
        rc = lib().zj_decoder_finish_pixels_scaled_device(self._d, self._ctx.handle, k, x, y, w, h, d_out, cap, out_pitch, C.byref(n))
        if rc:
            self._raise(rc)
        return n.value

    @property
    def orientation(self):
        """EXIF Orientation (1..8; 1: the file says nothing usable) of the file whose headers were read last; 0: none yet."""
        return int(lib().zj_decoder_orientation(self._d))

    @property
    def adobe_transform(self):
        """The transform byte of the last file's Adobe APP14 segment (0: CMYK / as stored, 1: YCbCr, 2: YCCK); -1: none seen."""
        return int(lib().zj_decoder_adobe_transform(self._d))

    @property
    def stored_rgb(self):
        """True when the last file is stored RGB: three components and an Adobe APP14 segment with transform 0
        (zj_decoder_stored_rgb; Pillow's save(keep_rgb=True) writes such files)."""
        return bool(lib().zj_decoder_stored_rgb(self._d))

    def component_sampling(self, comp):
        """(h, v) of component `comp` (0 .. components - 1) of the last file whose headers were read, as its frame header
        states them (zj_decoder_component_sampling)."""
        h, v = C.c_uint(0), C.c_uint(0)
        rc = lib().zj_decoder_component_sampling(self._d, int(comp), C.byref(h), C.byref(v))
        if rc:
            raise DecodeError(rc, "no such component")
        return h.value, v.value

    def plane(self, comp, copy=True):
        """Coefficient plane `comp` (0 .. components - 1) of the last file after a CPU decode (zj_decoder_plane): an int16
        array [blocks_h, blocks_w, 64], natural order (copy=False: a view, valid until the decoder's next call or its end)."""
        p, n, bw, bh = C.c_void_p(), C.c_size_t(0), C.c_uint(0), C.c_uint(0)
        rc = lib().zj_decoder_plane(self._d, int(comp), C.byref(p), C.byref(n), C.byref(bw), C.byref(bh))
        if rc:
            raise DecodeError(rc, "no such plane, or no decoded coefficients")
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), shape=(n.value,)).reshape(bh.value, bw.value, 64)
        return a.copy() if copy else a

    def finish_pixels_resized_crop_device(self, x, y, w, h, out_w, out_h, dtype, out_layout, d_out, cap, scale=None, bias=None,
                                          flip=False, antialias=False, max_prescale=1, apply_orientation=False,
                                          interpolation="bilinear"):
        """Stage 2 cut to the w x h window at (x, y) and resized (the contract of zj_decode_crops_resized_device), left in
        HBM at device pointer d_out; returns the output's length in bytes.  antialias: the triangle filter
        (zj_decoder_finish_pixels_resized_crop_filtered_device, RESIZE_BILINEAR_AA).  max_prescale = 2, 4, 8: a
        reduced-size decode under the resize (zj_decoder_finish_pixels_resized_crop_prescaled_device); 1: none.
        apply_orientation: the window is in DISPLAYED pixels of the file's EXIF orientation and so is the output
        (zj_decoder_finish_pixels_resized_crop_oriented_device); False: today's call.  interpolation="bicubic" (with
        antialias=True): RESIZE_BICUBIC_AA in the same calls (see resize_filter)."""
        filt = resize_filter(antialias, interpolation)
        if self._ctx is None:
            self._ctx = Context()
        n = C.c_size_t(0)
        k = scale_log2(max_prescale)
        args = (self._d, self._ctx.handle, x, y, w, h, out_w, out_h, dtype, out_layout, _floats(scale), _floats(bias),
                1 if flip else 0)
        if apply_orientation:
            rc = lib().zj_decoder_finish_pixels_resized_crop_oriented_device(*args, filt, k, d_out, cap, C.byref(n))
        elif k:
            rc = lib().zj_decoder_finish_pixels_resized_crop_prescaled_device(*args, filt, k, d_out, cap, C.byref(n))
        elif filt != RESIZE_BILINEAR:
            rc = lib().zj_decoder_finish_pixels_resized_crop_filtered_device(*args, filt, d_out, cap, C.byref(n))
        else:
            rc = lib().zj_decoder_finish_pixels_resized_crop_device(*args, d_out, cap, C.byref(n))
        if rc:
            self._raise(rc)
        return n.value

    def finish_pixels_device(self, d_out, cap, apply_orientation=False):
        """Stage 2 with the pixels left in HBM at device pointer d_out; returns their length in bytes.
        apply_orientation: the DISPLAYED image of the file's EXIF orientation
        (zj_decoder_finish_pixels_oriented_device); returns (length, width, height) of it."""
        if self._ctx is None:
            self._ctx = Context()
        n = C.c_size_t(0)
        if apply_orientation:
            w, h = C.c_uint(0), C.c_uint(0)
            rc = lib().zj_decoder_finish_pixels_oriented_device(self._d, self._ctx.handle, d_out, cap, C.byref(n), C.byref(w),
                                                                C.byref(h))
            if rc:
                self._raise(rc)
            return n.value, w.value, h.value
        rc = lib().zj_decoder_finish_pixels_device(self._d, self._ctx.handle, d_out, cap, C.byref(n))
        if rc:
            self._raise(rc)
        return n.value

    def decode_buffer(self, buf, out=None):  # decoder.rs:178
        """out: a uint8 array to decode into (e.g. a view of pinned memory, so that the downloads of a streamed baseline
        decode overlap as well); allocated when None."""
        if self._ctx is None:
            self._ctx = Context()
        b = np.frombuffer(bytes(buf), np.uint8)
        info = self.read_headers(buf)
        ncomp = 1 if info.components == 1 else ColorSpace(self._out_cs).num_components()
        if out is None:
            out = np.zeros(int(info.width) * int(info.height) * ncomp, np.uint8)
        n = C.c_size_t(0)
        rc = lib().zj_decoder_decode_buffer(self._d, self._ctx.handle, _ptr(b), b.size, _ptr(out), out.size,
                                            C.byref(n), C.byref(info))
        if rc:
            self._raise(rc)
        self._info = info
        return out[: n.value]


def finish_pixels_batch(decoders, ctx, outs=None, device_ptrs=None):
    """zj_decoder_finish_pixels_batch over Decoder objects that went through prepare(): the scans left for the device are
    decoded together.  outs: list of uint8 arrays (allocated when None and no device_ptrs); device_ptrs: list of
    (pointer, capacity) to leave the pixels in HBM.  Returns (outs or lengths, list of return codes)."""
    n = len(decoders)
    dptr = (C.c_void_p * n)(*[d._d for d in decoders])
    if device_ptrs is None and outs is None:
        outs = []
        for d in decoders:
            i = d._info
            nc = 1 if i.components == 1 else ColorSpace(d._out_cs).num_components()
            outs.append(np.zeros(int(i.width) * int(i.height) * nc, np.uint8))
    if device_ptrs is not None:
        optr = (C.c_void_p * n)(*[p for p, _ in device_ptrs])
        caps = (C.c_size_t * n)(*[cap for _, cap in device_ptrs])
    else:
        optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        caps = (C.c_size_t * n)(*[o.size for o in outs])
    lens = (C.c_size_t * n)()
    rcs = (C.c_int * n)()
    _check(lib().zj_decoder_finish_pixels_batch(dptr, n, ctx.handle, optr, caps, lens, 1 if device_ptrs is not None else 0, rcs),
           "zj_decoder_finish_pixels_batch", ctx.handle)
    if device_ptrs is not None:
        return list(lens), list(rcs)
    return [o[: lens[k]] for k, o in enumerate(outs)], list(rcs)


def finish_pixels_resized_crop_batch(decoders, ctx, windows, out_w, out_h, dtype, out_layout, d_out, cap, scale=None, bias=None,
                                     flips=None, antialias=False, max_prescale=1, apply_orientation=False,
                                     interpolation="bilinear", colors=None, tones=None):
    """zj_decoder_finish_pixels_resized_crop_batch_device over Decoder objects that went through prepare() or
    decode_coefficients(), each with a file of its own size: windows = one (x, y, w, h) per decoder (displayed pixels with
    apply_orientation), image k left at device pointer d_out + k * resized_out_len.  Returns the list of statuses: image k
    is Decoder.finish_pixels_resized_crop_device's for decoder k alone, a failed file's slot is untouched.
    colors: one [3, 4] colour matrix per decoder (None entries: the identity), each file's u8 image under its matrix in
    front of the resize (zj_decoder_finish_pixels_resized_crop_batch_colored_device); None: no colour stage.
    tones: one (op, param) tone op per decoder (None entries: the identity), the same image under it behind the colour matrix
    (zj_decoder_finish_pixels_resized_crop_batch_toned_device); None: no tone stage."""
    filt = resize_filter(antialias, interpolation)
    n = len(decoders)
    if len(windows) != n:
        raise ValueError("one window per decoder")
    dptr = (C.c_void_p * n)(*[d._d for d in decoders])
    win = (C.c_uint * (4 * n))(*[int(v) for w in windows for v in w])
    rcs = (C.c_int * n)()
    if tones is not None:
        _check(lib().zj_decoder_finish_pixels_resized_crop_batch_toned_device(
            dptr, n, ctx.handle, win, out_w, out_h, dtype, out_layout, _floats(scale), _floats(bias), _flips(flips, n), filt,
            scale_log2(max_prescale), 1 if apply_orientation else 0, _colors(colors, n), _tones(tones, n), d_out, cap, rcs),
            "zj_decoder_finish_pixels_resized_crop_batch_toned_device", ctx.handle)
        return list(rcs)
    if colors is not None:
        _check(lib().zj_decoder_finish_pixels_resized_crop_batch_colored_device(
            dptr, n, ctx.handle, win, out_w, out_h, dtype, out_layout, _floats(scale), _floats(bias), _flips(flips, n), filt,
            scale_log2(max_prescale), 1 if apply_orientation else 0, _colors(colors, n), d_out, cap, rcs),
            "zj_decoder_finish_pixels_resized_crop_batch_colored_device", ctx.handle)
        return list(rcs)
    _check(lib().zj_decoder_finish_pixels_resized_crop_batch_device(dptr, n, ctx.handle, win, out_w, out_h, dtype, out_layout,
                                                                    _floats(scale), _floats(bias), _flips(flips, n), filt,
                                                                    scale_log2(max_prescale), 1 if apply_orientation else 0,
                                                                    d_out, cap, rcs),
           "zj_decoder_finish_pixels_resized_crop_batch_device", ctx.handle)
    return list(rcs)


def finish_pixels_crop_tensor_batch(decoders, ctx, origins, w, h, dtype, out_layout, d_out, cap, scale=None, bias=None,
                                    flips=None, apply_orientation=False):
    """zj_decoder_finish_pixels_crop_tensor_batch_device over Decoder objects that went through prepare() or
    decode_coefficients(), each with a file of its own size: origins = one (x, y) per decoder, every window w x h, image k
    left at device pointer d_out + k * crop_tensor_out_len.  Returns the list of statuses: image k is
    Decoder.finish_pixels_crop_tensor_device's for decoder k alone, a failed file's slot is untouched.  apply_orientation:
    the origins are in DISPLAYED pixels of each file's own orientation (the _batch_oriented_ entry point)."""
    n = len(decoders)
    if len(origins) != n:
        raise ValueError("one origin per decoder")
    dptr = (C.c_void_p * n)(*[d._d for d in decoders])
    org = (C.c_uint * (2 * n))(*[int(v) for xy in origins for v in xy])
    rcs = (C.c_int * n)()
    name = "zj_decoder_finish_pixels_crop_tensor_batch_oriented_device" if apply_orientation else "zj_decoder_finish_pixels_crop_tensor_batch_device"
    _check(getattr(lib(), name)(dptr, n, ctx.handle, org, w, h, dtype, out_layout, _floats(scale), _floats(bias), _flips(flips, n),
                                d_out, cap, rcs), name, ctx.handle)
    return list(rcs)


def finish_pixels_warped_batch(decoders, ctx, matrices, out_w, out_h, dtype, out_layout, d_out, cap, scale=None, bias=None,
                               fill=None, edge="fill", apply_orientation=False):
    """zj_decoder_finish_pixels_warped_batch_device over Decoder objects that went through prepare() or decode_coefficients(),
    each with a file of its own size: matrices = one (a, b, c, d, e, f) per decoder, in pixels of its frame (of its DISPLAYED
    frame with apply_orientation); image k left at device pointer d_out + k * resized_out_len.  Returns the list of
    statuses: image k is Decoder.finish_pixels_warped_device's for decoder k alone, a failed file's slot is untouched."""
    n = len(decoders)
    dptr = (C.c_void_p * n)(*[d._d for d in decoders])
    rcs = (C.c_int * n)()
    _check(lib().zj_decoder_finish_pixels_warped_batch_device(dptr, n, ctx.handle, _matrices(matrices, n), 1 if apply_orientation else 0,
                                                              out_w, out_h, dtype, out_layout, _floats(scale), _floats(bias),
                                                              _fill(fill), warp_edge(edge), d_out, cap, rcs),
           "zj_decoder_finish_pixels_warped_batch_device", ctx.handle)
    return list(rcs)


class FileBatchDecoder:
    """JPEG files -> pixels left in HBM, e.g. a uint8 CUDA tensor [N, H, W, C] for PyTorch-ROCm consumers.
    Keeps `capacity` decoders (their prepared scans live in pinned memory) and one context; every call prepares the files
    on the CPU (headers + byte-level preparation) and finishes them in batches through zj_decoder_finish_pixels_batch:
    the entropy stage of a batch is one launch per phase, and images of one size that land equally spaced -- the rows of
    a tensor do -- share one pixel-kernel launch.  Progressive files and whatever the device hands back take the CPU
    walker; the bytes are the same."""

    def __init__(self, ctx=None, options=None, capacity=ZJ_SCAN_BATCH_MAX):
        if options is None:
            options = ZuneJpegOptions()
            options.entropy = ENTROPY_GPU
            options.pinned_planes = True
        self._ctx = ctx if ctx is not None else Context()
        self._out_cs = int(options.out_colorspace)
        self._layout = int(options.out_layout)
        self._decs = [Decoder(options, self._ctx) for _ in range(max(1, min(int(capacity), ZJ_SCAN_BATCH_MAX)))]

    def close(self):
        for d in self._decs:
            d.close()
        self._decs = []

    def decode(self, files, device_ptrs):
        """files[k] -> device_ptrs[k] = (pointer, capacity).  Returns (lengths, infos); raises DecodeError on the first failure."""
        lens, infos = [], []
        for base in range(0, len(files), len(self._decs)):
            chunk = files[base:base + len(self._decs)]
            for d, f in zip(self._decs, chunk):
                infos.append(d.prepare(f)[1])
            ln, rcs = finish_pixels_batch(self._decs[:len(chunk)], self._ctx, device_ptrs=device_ptrs[base:base + len(chunk)])
            for d, rc in zip(self._decs, rcs):
                if rc:
                    d._raise(rc)
            lens += ln
        return lens, infos

    def to_tensor(self, files, device="cuda:0"):
        """Files of ONE size -> uint8 tensor [N, H, W, C] ([N, C, H, W] with LAYOUT_CHW) on `device`."""
        import torch
        info = self._decs[0].read_headers(files[0])
        nc = 1 if info.components == 1 else ColorSpace(self._out_cs).num_components()
        h, w = int(info.height), int(info.width)
        shape = (len(files), nc, h, w) if self._layout == LAYOUT_CHW else (len(files), h, w, nc)
        t = torch.empty(shape, dtype=torch.uint8, device=device)
        # torch's caching allocator may hand back a block that work queued on torch's current stream still reads; the
        # library writes it on ITS OWN stream, so that work has to be over first (completion is the library's business)
        torch.cuda.current_stream(t.device).synchronize()
        step = h * w * nc
        if step % 16:
            raise ZjError(ERR_ARG, "to_tensor: width * height * components must be a multiple of 16 (rows of the tensor are the outputs)")
        lens, infos = self.decode(files, [(t.data_ptr() + k * step, step) for k in range(len(files))])
        for i in infos:
            if (int(i.width), int(i.height)) != (w, h):
                raise ZjError(ERR_ARG, "to_tensor: files of different sizes")
        return t


def device_numa_node(device=0):
    """NUMA node of a HIP device (PCI bus id -> sysfs), -1 unknown"""
    return lib().zj_device_numa_node(int(device))


def bind_thread_near_device(device=0):
    """Bind the calling thread (and the threads it starts from now on) to the CPUs of the device's NUMA node; returns the
    node, or -1 if nothing was bound (unknown node, ZJ_NUMA=off, an affinity that excludes the node)."""
    return lib().zj_bind_thread_near_device(int(device))


def thread_numa_node():
    return lib().zj_thread_numa_node()


def variants_available():
    """Kernel variants this build of libzjhip.so carries: [0, 2], plus 1 when it was built with `make VARIANTS=all`."""
    return [v for v in (0, 1, 2) if lib().zj_variant_available(v)]


def pointer_device(p):
    """HIP device that owns device pointer p, or a negative zj_status (host memory, unknown pointer)."""
    return lib().zj_pointer_device(p)


def shard_range(nframes, slot, nslots):
    """zj_shard_range: contiguous shard [lo, hi) of `slot` (the rule of shard.shard_range, in the library)."""
    lo, hi = C.c_size_t(0), C.c_size_t(0)
    lib().zj_shard_range(nframes, slot, nslots, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class Multi:
    """zj_multi: image-level sharding of plane batches over device slots (one context + one host thread per slot)."""

    def __init__(self, devices):
        devs = (C.c_int * len(devices))(*devices)
        st = C.c_int(0)
        self._m = lib().zj_multi_create(devs, len(devices), C.byref(st))
        if not self._m:
            raise ZjError(st.value, "zj_multi_create")
        self.nslots = len(devices)

    def close(self):
        if getattr(self, "_m", None):
            lib().zj_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def slot_stats(self):
        """[(device, frames decoded)] per slot"""
        res = []
        for k in range(self.nslots):
            d, n = C.c_int(0), C.c_size_t(0)
            lib().zj_multi_slot_stats(self._m, k, C.byref(d), C.byref(n))
            res.append((d.value, n.value))
        return res

    def slot_numa(self):
        """[(NUMA node of the slot's device, node its host thread runs on, bound?)] per slot; -1 = unknown"""
        res = []
        for k in range(self.nslots):
            a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(0)
            lib().zj_multi_slot_numa(self._m, k, C.byref(a), C.byref(b), C.byref(c))
            res.append((a.value, b.value, bool(c.value)))
        return res

    def decode_planes(self, desc, planes, nframes):
        """Packed host frames -> packed host pixels, sharded over the slots."""
        arrs = [_i16(p) for p in planes]
        while len(arrs) < 3:
            arrs.append(np.zeros(8, np.int16))
        out = np.empty(nframes * lib().zj_out_len(C.byref(desc)), np.uint8)
        sts = (C.c_int * self.nslots)()
        rc = lib().zj_multi_decode_planes_batch(self._m, C.byref(desc), nframes, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]),
                                                _ptr(out), sts)
        if rc:
            raise ZjError(rc, f"zj_multi_decode_planes_batch (per slot: {list(sts)})")
        return out

    def decode_frames(self, desc, frames_planes):
        """Host frames that are independent allocations, sharded over the slots; returns the per-frame arrays."""
        n = len(frames_planes)
        arrs = [[_i16(p) for p in pl] for pl in frames_planes]
        nc = max(len(a) for a in arrs)
        outs = [np.empty(lib().zj_out_len(C.byref(desc)), np.uint8) for _ in range(n)]
        tab = [(C.c_void_p * n)(*[a[c].ctypes.data for a in arrs]) if c < nc else None for c in range(3)]
        otab = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        sts = (C.c_int * self.nslots)()
        rc = lib().zj_multi_decode_frames(self._m, C.byref(desc), n, tab[0], tab[1], tab[2], otab, sts)
        if rc:
            raise ZjError(rc, f"zj_multi_decode_frames (per slot: {list(sts)})")
        return outs

    def decode_frames_device(self, desc, d_y, d_cb, d_cr, d_out):
        """Device pointers per frame (frame f on the device of the slot whose shard holds f); returns when all are done."""
        n = len(d_y)
        arr = lambda v: (C.c_void_p * n)(*v) if v is not None else None
        sts = (C.c_int * self.nslots)()
        rc = lib().zj_multi_decode_frames_device(self._m, C.byref(desc), n, arr(d_y), arr(d_cb), arr(d_cr), arr(d_out), sts)
        if rc:
            raise ZjError(rc, f"zj_multi_decode_frames_device (per slot: {list(sts)})")


class Pool:
    """zj_pool: persistent host workers (entropy decoder + GPU context each) for batches of JPEG files.  `devices` (a
    list) makes it a multi-device pool (zj_pool_create_multi): `threads` entropy workers per device slot."""

    def __init__(self, threads=4, options=None, device=0, devices=None):
        o = options.to_c() if options is not None else Options()
        st = C.c_int(0)
        if devices is not None:
            devs = (C.c_int * len(devices))(*devices)
            self._p = lib().zj_pool_create_multi(devs, len(devices), int(threads), C.byref(o), C.byref(st))
        else:
            self._p = lib().zj_pool_create(int(device), int(threads), C.byref(o), C.byref(st))
        if not self._p:
            raise ZjError(st.value, "zj_pool_create")
        self._out_cs = int(o.out_colorspace)

    def device_stats(self):
        """[(device, GPU-stage seconds, files)] per device slot"""
        res = []
        for k in range(lib().zj_pool_devices(self._p)):
            d, s_, n = C.c_int(0), C.c_double(0), C.c_size_t(0)
            lib().zj_pool_device_stats(self._p, k, C.byref(d), C.byref(s_), C.byref(n))
            res.append((d.value, s_.value, n.value))
        return res

    def slot_numa(self):
        """[(NUMA node of the slot's device, threads bound there, threads)] per device slot; node -1 = unknown"""
        res = []
        for k in range(lib().zj_pool_devices(self._p)):
            a, b, c = C.c_int(-1), C.c_int(0), C.c_int(0)
            lib().zj_pool_slot_numa(self._p, k, C.byref(a), C.byref(b), C.byref(c))
            res.append((a.value, b.value, c.value))
        return res

    def close(self):
        if getattr(self, "_p", None):
            lib().zj_pool_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def threads(self):
        return lib().zj_pool_threads(self._p)

    def stats(self):
        """(entropy-stage seconds, GPU-stage seconds, files) accumulated since creation."""
        e, g, n = C.c_double(0), C.c_double(0), C.c_size_t(0)
        lib().zj_pool_stats(self._p, C.byref(e), C.byref(g), C.byref(n))
        return e.value, g.value, n.value

    def decode_files_device(self, blobs, d_outs, caps, raise_on_error=True):
        """blobs -> pixels left in HBM at the device pointers d_outs (capacities caps).  Returns (lengths, infos, statuses)."""
        n = len(blobs)
        arrs = [np.frombuffer(bytes(b), np.uint8) for b in blobs]
        bufs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * n)(*[a.size for a in arrs])
        optr = (C.c_void_p * n)(*d_outs)
        capv = (C.c_size_t * n)(*caps)
        olen = (C.c_size_t * n)()
        infos = (ImageInfo * n)()
        sts = (C.c_int * n)()
        rc = lib().zj_pool_decode_files_device(self._p, n, bufs, lens, optr, capv, olen, infos, sts)
        if rc and raise_on_error:
            raise DecodeError(rc, lib().zj_pool_error(self._p).decode(errors="replace"))
        return list(olen), list(infos), list(sts)

    def to_tensor(self, blobs, device="cuda:0", layout=LAYOUT_HWC):
        """Files of ONE size -> uint8 tensor [N, H, W, C] on `device` (the pool's): the workers prepare, the submitters
        finish in batches into the rows of the tensor (with a GPU entropy setting nothing but the files crosses PCIe)."""
        import torch
        dec = Decoder()
        info = dec.read_headers(blobs[0])
        dec.close()
        nc = 1 if info.components == 1 else ColorSpace(self._out_cs).num_components()
        h, w = int(info.height), int(info.width)
        t = torch.empty((len(blobs), nc, h, w) if layout == LAYOUT_CHW else (len(blobs), h, w, nc), dtype=torch.uint8, device=device)
        torch.cuda.current_stream(t.device).synchronize()   # see FileBatchDecoder.to_tensor: the pool writes on its own streams
        step = h * w * nc
        if step % 16:
            raise ZjError(ERR_ARG, "to_tensor: width * height * components must be a multiple of 16")
        lens, infos, sts = self.decode_files_device(blobs, [t.data_ptr() + k * step for k in range(len(blobs))], [step] * len(blobs))
        if any(int(i.width) != w or int(i.height) != h for i in infos):
            raise ZjError(ERR_ARG, "to_tensor: files of different sizes")
        return t

    def decode_files(self, blobs, outs=None, raise_on_error=True):
        """blobs: list of bytes-like JPEG files.  Returns (list of uint8 arrays, list of ImageInfo, statuses).
        `outs` may supply preallocated uint8 arrays (e.g. views of pinned memory)."""
        n = len(blobs)
        arrs = [np.frombuffer(bytes(b), np.uint8) for b in blobs]
        if outs is None:
            dec = Decoder()
            outs = []
            for a in arrs:
                try:
                    info = dec.read_headers(a)
                    nc = 1 if info.components == 1 else ColorSpace(self._out_cs).num_components()
                    outs.append(np.zeros(int(info.width) * int(info.height) * nc, np.uint8))
                except DecodeError:
                    outs.append(np.zeros(16, np.uint8))
            dec.close()
        bufs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * n)(*[a.size for a in arrs])
        optr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        caps = (C.c_size_t * n)(*[o.size for o in outs])
        olen = (C.c_size_t * n)()
        infos = (ImageInfo * n)()
        sts = (C.c_int * n)()
        rc = lib().zj_pool_decode_files(self._p, n, bufs, lens, optr, caps, olen, infos, sts)
        if rc and raise_on_error:
            raise DecodeError(rc, lib().zj_pool_error(self._p).decode(errors="replace"))
        return [o[: olen[i]] for i, o in enumerate(outs)], list(infos), list(sts)

"""Decoded frames as PyTorch-ROCm tensors (the consumer-side layouts).  Plumbing over the C ABI, nothing
computes here: the tensors are views of the bytes zj_decode_planes_device writes.

  layout                      desc                                   view (uint8)                 strides (bytes)
  interleaved (the reference)  out_layout = LAYOUT_HWC                [N, H, W, C]                 out_len, pitch, C, 1
  planar                       out_layout = LAYOUT_CHW, RGB           [N, 3, H, W]                 out_len, pitch*H, pitch, 1
  grayscale                    out_colorspace = GRAYSCALE             [N, H, W]                    out_len, pitch, 1

pitch = desc.out_pitch, or the row's own length when that is 0 (the reference's tight rows, /root/reference/src/mcu.rs:375-379).
With a padded pitch (padded_desc: the next multiple of 128 bytes, which keeps every tile's row segment on whole cache
lines -- DESIGN.md 4.0) the view is simply strided over the padding; `.contiguous()` gives the tight tensor.
"""
import copy
import ctypes as C

from .host import DTYPE_BF16, DTYPE_F16, DTYPE_F32, DTYPE_U8, LAYOUT_CHW, LAYOUT_HWC, TENSOR_NCHW, TENSOR_NHWC, ColorSpace, lib


def row_bytes(desc):
    """bytes of one output row (CHW: of one plane's row)"""
    ncomp = ColorSpace(desc.out_colorspace).num_components()
    planar = desc.out_layout == LAYOUT_CHW and ncomp == 3
    return desc.width if planar else desc.width * ncomp


def padded_desc(desc, align=128):
    """a copy of `desc` whose rows lie at the next multiple of `align` bytes (zj_frame_desc.out_pitch; device outputs only)"""
    d = copy.copy(desc)
    d.out_pitch = (row_bytes(desc) + align - 1) // align * align
    return d


def output_tensor(desc, nframes, device, fill=None):
    """(storage, view): a flat uint8 tensor of nframes * zj_out_len(desc) bytes on `device` to hand to
    Context.decode_planes_device(..., storage.data_ptr()), and its view in the layout the descriptor names."""
    import torch
    out_len = lib().zj_out_len(C.byref(desc))
    if out_len == 0:
        raise ValueError("zj_out_len(desc) == 0: not a decodable frame descriptor")
    storage = torch.empty(nframes * out_len, dtype=torch.uint8, device=device) if fill is None else \
        torch.full((nframes * out_len,), fill, dtype=torch.uint8, device=device)
    return storage, view_of(desc, storage, nframes)


def view_of(desc, storage, nframes):
    """the [N, H, W, C] / [N, 3, H, W] / [N, H, W] view of a flat output buffer (see the module docstring)"""
    out_len = lib().zj_out_len(C.byref(desc))
    ncomp = ColorSpace(desc.out_colorspace).num_components()
    pitch = desc.out_pitch or row_bytes(desc)
    h, w = desc.height, desc.width
    if desc.out_layout == LAYOUT_CHW and ncomp == 3:
        return storage.as_strided((nframes, 3, h, w), (out_len, pitch * h, pitch, 1))
    if ncomp == 1:
        return storage.as_strided((nframes, h, w), (out_len, pitch, 1))
    return storage.as_strided((nframes, h, w, ncomp), (out_len, pitch, ncomp, 1))


def decode_to_tensor(ctx, desc, planes, nframes=1, stream=None):
    """planes: three int16 CUDA tensors (Y, Cb, Cr; `nframes` frames back to back, include/zjhip.h "whole-frame layout").
    Launches on `stream` (a torch.cuda.Stream, or None = torch's current stream) and returns the view; the caller
    synchronises as with any other kernel on that stream."""
    import torch
    dev = planes[0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    # The output is allocated (and, with a fill, written) under `s`, so that the caching allocator ties the block to the
    # stream the kernel writes it on: allocated under another stream it could be handed out again while the launch is
    # still pending.  The planes were produced on the caller's current stream: `s` waits for it before the launch.
    with torch.cuda.stream(s):
        storage, view = output_tensor(desc, nframes, dev)
    if s != cur:
        s.wait_stream(cur)
        for p in planes:
            p.record_stream(s)
    ctx.decode_planes_device(desc, nframes, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), storage.data_ptr(), s.cuda_stream)
    return view


def crop_view_of(desc, storage, nframes, w, h):
    """the dense [N, h, w, C] / [N, 3, h, w] / [N, h, w] view of nframes tight w x h crops back to back"""
    ncomp = ColorSpace(desc.out_colorspace).num_components()
    if desc.out_layout == LAYOUT_CHW and ncomp == 3:
        return storage.view(nframes, 3, h, w)
    if ncomp == 1:
        return storage.view(nframes, h, w)
    return storage.view(nframes, h, w, ncomp)


def decode_crops_to_tensor(ctx, desc, frames, origins, size, stream=None):
    """Crop windows as one dense uint8 tensor (zj_decode_crops_device): frames = a list of (Y, Cb, Cr) int16 CUDA tensors,
    one frame each (Cb / Cr may be None for GRAYSCALE output), origins = one (x, y) per frame, size = (w, h) of every
    window.  Returns [N, h, w, C], [N, 3, h, w] or [N, h, w]; crop n equals view[n, ..., y:y+h, x:x+w] of the full decode.
    Stream and allocator rules as decode_to_tensor."""
    import torch
    w, h = size
    n = len(frames)
    if n == 0 or len(origins) != n:
        raise ValueError("one origin per frame, at least one frame")
    crop_len = lib().zj_crop_out_len(C.byref(desc), w, h, 0)
    if crop_len == 0:
        raise ValueError(f"{w}x{h} is not a valid crop of this frame descriptor")
    dev = frames[0][0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    with torch.cuda.stream(s):
        storage = torch.empty(n * crop_len, dtype=torch.uint8, device=dev)
    if s != cur:
        s.wait_stream(cur)
        for fr in frames:
            for p in fr:
                if p is not None:
                    p.record_stream(s)
    ptr = lambda t: t.data_ptr() if t is not None else None
    base = storage.data_ptr()
    ctx.decode_crops_device(desc, [ptr(fr[0]) for fr in frames], [ptr(fr[1]) for fr in frames], [ptr(fr[2]) for fr in frames],
                            origins, w, h, [base + i * crop_len for i in range(n)], 0, s.cuda_stream)
    return crop_view_of(desc, storage, n, w, h)


def _resize_dtype(dtype):
    import torch
    codes = {torch.float32: DTYPE_F32, torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16, torch.uint8: DTYPE_U8}
    if dtype not in codes:
        raise ValueError(f"resized outputs are float32, float16, bfloat16 or uint8, not {dtype}")
    return codes[dtype]


def normalize_factors(channels, mean=None, std=None):
    """torchvision-style mean / std (of the [0, 1] image) -> the float32 scale and bias of zj_resize_device:
    y = x * scale + bias for x in [0, 255] units, scale = 1 / (255 std), bias = -mean / std (None: 0 and 1)"""
    import numpy as np
    m = np.broadcast_to(np.asarray(0.0 if mean is None else mean, np.float64), (channels,))
    sd = np.broadcast_to(np.asarray(1.0 if std is None else std, np.float64), (channels,))
    return [float(v) for v in np.float32(1.0 / (255.0 * sd))], [float(v) for v in np.float32(-m / sd)]


def _resized_out(n, channels, size, dtype, layout, dev, s):
    import torch
    ow, oh = size
    if layout not in ("NCHW", "NHWC"):
        raise ValueError("layout is 'NCHW' or 'NHWC'")
    shape = (n, channels, oh, ow) if layout == "NCHW" else (n, oh, ow, channels)
    with torch.cuda.stream(s):
        return torch.empty(shape, dtype=dtype, device=dev)


def _on_stream(s, cur, tensors):
    if s != cur:
        s.wait_stream(cur)
        for t in tensors:
            if t is not None:
                t.record_stream(s)


def decode_resized_crops_to_tensor(ctx, desc, frames, windows, size, dtype=None, layout="NCHW", mean=None, std=None,
                                   flips=None, stream=None, antialias=False, max_prescale=1, orientations=None,
                                   interpolation="bilinear", color=None, tone=None):
    """Crop windows resized and normalised into ONE dense tensor (zj_decode_crops_resized_device): frames = a list of
    (Y, Cb, Cr) int16 CUDA tensors, one frame each (Cb / Cr may be None for GRAYSCALE output), windows = one (x, y, w, h)
    per frame (each its own size), size = (out_w, out_h).  Returns [N, C, out_h, out_w] ("NCHW") or [N, out_h, out_w, C]
    ("NHWC") of `dtype` (default bfloat16); C = 3 for RGB / YCbCr, 1 for GRAYSCALE.  mean / std: torchvision's Normalize
    of the [0, 1] image (None: the [0, 1] image itself); unused for uint8.  flips: one bool per frame (horizontal).
    antialias: the triangle filter of F.interpolate(antialias=True) instead of plain bilinear.
    interpolation: "bilinear" (default) or, with antialias=True only, "bicubic": the filter of F.interpolate(mode="bicubic",
    antialias=True) and Pillow's BICUBIC; anything else is a ValueError.
    max_prescale = 2, 4 or 8: every window is decoded at the largest reduced size (1/2, 1/4, 1/8, up to 1/max_prescale)
    that still is at least the output's, and resized from there; 1 (default): none.  Anything else is a
    ValueError.  orientations: one EXIF orientation 1..8 per frame; the windows are then in DISPLAYED pixels of the frames
    and the crops are turned before the resize; None (default): none.
    One-component frames: desc.flags | FLAG_GRAY_TO_RGB with ColorSpace.RGB gives the image a viewer shows, R = G = B
    (DESIGN.md 3.11): the GRAYSCALE crop, turned, copied into three channels, then resized.  Without the flag a
    one-component descriptor that asks for RGB is refused (ZjError: not supported); ask for GRAYSCALE and get C = 1.  The
    flag does nothing for three-component frames.
    color: one [3, 4] colour matrix per frame (color_matrix; None in a frame's place: the identity), applied to the u8 image
    in front of the resize, clamped as an 8-bit image is; the call then goes through
    zj_decode_crops_resized_mixed_colored_device with the descriptor repeated.  None (default): none.  Needs a
    three-channel output.
    tone: one tone op per frame (tone_op; None in a frame's place: the identity) -- invert, posterize, solarize, autocontrast,
    equalize, byte for byte Pillow's ImageOps on the u8 CROP the resize reads -- behind the colour matrix and
    in front of the resize (zj_decode_crops_resized_mixed_toned_device).  None (default): none.  One-channel outputs take it
    too.  Stream and allocator rules as decode_to_tensor."""
    import torch
    from .host import resize_filter, scale_log2
    scale_log2(max_prescale)
    resize_filter(antialias, interpolation)
    dtype = torch.bfloat16 if dtype is None else dtype
    code = _resize_dtype(dtype)
    n = len(frames)
    if n == 0 or len(windows) != n:
        raise ValueError("one window per frame, at least one frame")
    ow, oh = size
    if lib().zj_resized_out_len(C.byref(desc), ow, oh, code) == 0:
        raise ValueError(f"{ow}x{oh} {dtype} is not a supported resized output of this frame descriptor")
    channels = ColorSpace(desc.out_colorspace).num_components()
    scale, bias = normalize_factors(channels, mean, std)
    dev = frames[0][0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    out = _resized_out(n, channels, size, dtype, layout, dev, s)
    _on_stream(s, cur, [p for fr in frames for p in fr])
    ptr = lambda t: t.data_ptr() if t is not None else None
    if color is not None or tone is not None:
        if (color is not None and len(color) != n) or (tone is not None and len(tone) != n):
            raise ValueError("one colour matrix / tone op per frame")
        cbs = [ptr(fr[1]) for fr in frames]
        ctx.decode_crops_resized_mixed_device([desc] * n, [ptr(fr[0]) for fr in frames], cbs if any(cbs) else None,
                                              [ptr(fr[2]) for fr in frames] if any(cbs) else None, windows, ow, oh, code,
                                              TENSOR_NCHW if layout == "NCHW" else TENSOR_NHWC, out.data_ptr(), scale, bias, flips,
                                              s.cuda_stream, antialias, max_prescale, orientations, interpolation, colors=color,
                                              tones=tone)
        return out
    ctx.decode_crops_resized_device(desc, [ptr(fr[0]) for fr in frames], [ptr(fr[1]) for fr in frames],
                                    [ptr(fr[2]) for fr in frames], windows, ow, oh, code,
                                    TENSOR_NCHW if layout == "NCHW" else TENSOR_NHWC, out.data_ptr(), scale, bias, flips,
                                    s.cuda_stream, antialias, max_prescale, orientations, interpolation)
    return out


def decode_crops_to_normalized_tensor(ctx, desc, frames, origins, size, dtype=None, layout="NCHW", mean=None, std=None,
                                      flips=None, stream=None):
    """Crop windows converted and normalised into ONE dense tensor WITHOUT a resize (zj_decode_crops_tensor_device,
    DESIGN.md 3.14): frames = a list of (Y, Cb, Cr) int16 CUDA tensors, one frame each (Cb / Cr may be None for GRAYSCALE
    output), origins = one (x, y) per frame, size = (w, h) of every window (any size inside the frame: no 8192 limit).
    Returns [N, C, h, w] ("NCHW") or [N, h, w, C] ("NHWC") of `dtype` (default bfloat16), element for element what
    decode_resized_crops_to_tensor gives for windows of exactly `size`, written once by one launch per 32 frames.  dtype,
    mean / std and flips as there.  Stream and allocator rules as decode_to_tensor."""
    import torch
    dtype = torch.bfloat16 if dtype is None else dtype
    code = _resize_dtype(dtype)
    n = len(frames)
    if n == 0 or len(origins) != n:
        raise ValueError("one origin per frame, at least one frame")
    w, h = size
    if lib().zj_crop_tensor_out_len(C.byref(desc), w, h, code) == 0:
        raise ValueError(f"{w}x{h} {dtype} is not a supported crop tensor of this frame descriptor")
    channels = ColorSpace(desc.out_colorspace).num_components()
    scale, bias = normalize_factors(channels, mean, std)
    dev = frames[0][0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    out = _resized_out(n, channels, size, dtype, layout, dev, s)
    _on_stream(s, cur, [p for fr in frames for p in fr])
    ptr = lambda t: t.data_ptr() if t is not None else None
    ctx.decode_crops_tensor_device(desc, [ptr(fr[0]) for fr in frames], [ptr(fr[1]) for fr in frames],
                                   [ptr(fr[2]) for fr in frames], origins, w, h, code,
                                   TENSOR_NCHW if layout == "NCHW" else TENSOR_NHWC, out.data_ptr(), scale, bias, flips,
                                   s.cuda_stream)
    return out


def _prepare_files(ctx, blobs, options, workers, decoders):
    """(decs, prepared) of the decode_files_* calls: one Decoder per blob, made as needed and kept in `decoders`, each
    prepared on a pool of at most 16 threads; the first file that fails raises DecodeError naming its index."""
    from concurrent.futures import ThreadPoolExecutor
    from .host import DecodeError, Decoder
    n = len(blobs)
    decs = decoders if decoders is not None else []
    while len(decs) < n:
        decs.append(Decoder(options, ctx))
    decs = decs[:n]

    def prep(k):
        try:
            return decs[k].prepare(blobs[k])
        except DecodeError as e:
            return e

    nw = max(1, min(int(workers), 16, n))
    if nw > 1:
        with ThreadPoolExecutor(nw) as ex:
            prepared = list(ex.map(prep, range(n)))
    else:
        prepared = [prep(k) for k in range(n)]
    for k, r in enumerate(prepared):
        if isinstance(r, DecodeError):
            raise DecodeError(r.status, f"file {k}: {r.text}")
    return decs, prepared


def _files_out(ctx, decs, what, size, dtype, layout, mean, std, stream):
    """(out, scale, bias) of the decode_files_* calls: the dense output of len(decs) images allocated under `stream` (None:
    torch's current) and that stream synchronised -- the allocator may hand out a block that work queued on it still uses,
    and the batch calls run on the context's stream."""
    import torch
    channels = ColorSpace(decs[0]._out_cs).num_components()
    if channels not in (1, 3):
        raise ValueError(f"{what} have 1 or 3 channels")
    scale, bias = normalize_factors(channels, mean, std)
    dev = torch.device("cuda", ctx.device) if hasattr(ctx, "device") else torch.device("cuda")
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    out = _resized_out(len(decs), channels, size, dtype, layout, dev, s)
    s.synchronize()
    return out, scale, bias


def _raise_first_failed(decs, rcs):
    from .host import DecodeError
    for k, rc in enumerate(rcs):
        if rc:
            raise DecodeError(rc, f"file {k}: " + lib().zj_decoder_error(decs[k]._d).decode(errors="replace"))


def decode_files_resized_to_tensor(ctx, blobs, windows, size, dtype=None, layout="NCHW", mean=None, std=None, flips=None,
                                   antialias=False, interpolation="bilinear", max_prescale=1, apply_orientation=False,
                                   options=None, workers=1, stream=None, decoders=None, color=None, tone=None):
    """JPEG files of ANY sizes -> ONE dense resized-crop tensor (zj_decoder_finish_pixels_resized_crop_batch_device,
    DESIGN.md 3.10): blobs = a list of bytes-like JPEG files, windows = one (x, y, w, h) per file (displayed pixels with
    apply_orientation; None, or None in a file's place: the whole displayed image), size = (out_w, out_h).  Returns
    [N, C, out_h, out_w] ("NCHW") or [N, out_h, out_w, C] ("NHWC") of `dtype` (default bfloat16); image k is
    Decoder.finish_pixels_resized_crop_device's for file k alone.  The other keywords as decode_resized_crops_to_tensor.
    options: ZuneJpegOptions of the decoders (None: the defaults).  workers: threads that prepare the files (headers and
    the CPU entropy stage; the library calls release the GIL), at most 16.  decoders: a list to keep between calls --
    Decoder objects are made as needed, appended to it and reused.  A file that fails raises DecodeError naming its index.
    Grayscale (one-component) files among colour ones: give options.flags | FLAG_GRAY_TO_RGB with out_colorspace RGB, and
    their images are R = G = B like torchvision's decode_jpeg(mode=RGB), decoded in the same launch groups
    as the colour files.  WITHOUT the flag a one-component file is decoded as GRAYSCALE whatever the options ask for: its
    one channel lands in the first third of its 3-channel slot, the rest of the slot is not written, no error is raised,
    and the files around it are decoded one by one.  The flag does nothing for three-component files.
    Four-component files (Adobe CMYK / YCCK): with options.flags | FLAG_CMYK_TO_RGB and out_colorspace RGB their images are
    what Pillow's convert("RGB") shows, each finished through its single-file call; WITHOUT the flag such a
    file is refused when it is prepared (DecodeError naming its index), as the reference refuses it.
    Three-component files the reference refuses -- 4:1:1, 4:1:0, chroma that is not (1,1), ids outside 1..3 -- and stored-RGB
    files (Adobe transform 0, Pillow's keep_rgb=True): with options.flags | FLAG_ANY_SAMPLING and out_colorspace RGB their
    images are the resize of the box-replicated, colour-converted component planes, never prescaled, each
    finished through its single-file call; WITHOUT the flag the first kind is refused when it is prepared (DecodeError
    naming its index) and a stored-RGB file with ids 1..3 is shown through YCbCr -> RGB, with wrong colours.
    color: one [3, 4] colour matrix per file (color_matrix; None in a file's place: the identity): each file's finished u8
    image -- gray, CMYK, odd-sampled and turned files included -- under its matrix in front of the resize, clamped as an
    8-bit image is (zj_decoder_finish_pixels_resized_crop_batch_colored_device).  None (default): none.
    tone: one tone op per file (tone_op; None in a file's place: the identity): the same u8 image under it behind the colour
    matrix -- invert, posterize, solarize, autocontrast and equalize as Pillow's ImageOps on the CROP the resize reads, not on
    the whole file (zj_decoder_finish_pixels_resized_crop_batch_toned_device).  With color= and the warp this
    reaches RandAugment's op set inside the call, Sharpness excepted.  None (default): none.
    The batch call runs on the context's stream and has finished when it returns; `stream` (None: torch's current) is
    the stream the output is allocated under, synchronised before the call writes it."""
    import torch
    from .host import finish_pixels_resized_crop_batch, oriented_size, resize_filter, scale_log2
    scale_log2(max_prescale)
    resize_filter(antialias, interpolation)
    dtype = torch.bfloat16 if dtype is None else dtype
    code = _resize_dtype(dtype)
    n = len(blobs)
    if n == 0 or (windows is not None and len(windows) != n):
        raise ValueError("one window per file, at least one file")
    decs, prepared = _prepare_files(ctx, blobs, options, workers, decoders)
    wins = []
    for k in range(n):
        w = windows[k] if windows is not None else None
        if w is None:
            info = prepared[k][1]
            iw, ih = int(info.width), int(info.height)
            if apply_orientation:
                iw, ih = oriented_size(decs[k].orientation, iw, ih)
            w = (0, 0, iw, ih)
        wins.append(w)
    out, scale, bias = _files_out(ctx, decs, "resized outputs", size, dtype, layout, mean, std, stream)
    rcs = finish_pixels_resized_crop_batch(decs, ctx, wins, size[0], size[1], code,
                                           TENSOR_NCHW if layout == "NCHW" else TENSOR_NHWC, out.data_ptr(),
                                           out.numel() * out.element_size(), scale, bias, flips, antialias, max_prescale,
                                           apply_orientation, interpolation, colors=color, tones=tone)
    _raise_first_failed(decs, rcs)
    return out


def decode_files_cropped_to_tensor(ctx, blobs, origins, size, dtype=None, layout="NCHW", mean=None, std=None, flips=None,
                                   options=None, workers=1, stream=None, decoders=None, apply_orientation=False):
    """JPEG files -> ONE dense tensor of their size = (w, h) windows, converted and normalised but NOT resized
    (zj_decoder_finish_pixels_crop_tensor_batch_device): blobs = a list of bytes-like JPEG files, origins = one
    (x, y) per file, or None: the whole image, and then every file must measure exactly `size` (ValueError naming the
    first that does not).  Returns [N, C, h, w] ("NCHW") or [N, h, w, C] ("NHWC") of `dtype` (default bfloat16); image k
    is Decoder.finish_pixels_crop_tensor_device's for file k.  dtype, mean / std, flips, options, workers, decoders and
    stream as decode_files_resized_to_tensor.  The batch call runs on the context's stream and has finished when it
    returns; a file that fails raises DecodeError naming its index (its image is untouched, the others are decoded).
    apply_orientation: origins and size are in DISPLAYED pixels of each file's own EXIF orientation; with
    origins=None the displayed size must equal `size`.  With FLAG_GRAY_TO_RGB, FLAG_CMYK_TO_RGB or FLAG_ANY_SAMPLING in the
    options' flags, gray files shown as RGB, CMYK / YCCK files and files of another sampling or stored RGB are decoded here
    as well, through their u8 image and to_normalized_tensor's stage; a prescale is decode_files_resized_to_tensor's."""
    import torch
    from .host import finish_pixels_crop_tensor_batch, oriented_size
    dtype = torch.bfloat16 if dtype is None else dtype
    code = _resize_dtype(dtype)
    n = len(blobs)
    if n == 0 or (origins is not None and len(origins) != n) or (flips is not None and len(flips) != n):
        raise ValueError("one origin (and flip) per file, at least one file")
    decs, prepared = _prepare_files(ctx, blobs, options, workers, decoders)
    w, h = size
    if origins is None:
        for k in range(n):
            info = prepared[k][1]
            shown = (int(info.width), int(info.height))
            if apply_orientation:
                shown = tuple(oriented_size(decs[k].orientation, *shown))
            if shown != (w, h):
                raise ValueError(f"file {k} is {shown[0]}x{shown[1]}, not {w}x{h}: give origins")
        origins = [(0, 0)] * n
    out, scale, bias = _files_out(ctx, decs, "crop tensors", size, dtype, layout, mean, std, stream)
    rcs = finish_pixels_crop_tensor_batch(decs, ctx, origins, w, h, code, TENSOR_NCHW if layout == "NCHW" else TENSOR_NHWC,
                                          out.data_ptr(), out.numel() * out.element_size(), scale, bias, flips,
                                          apply_orientation=bool(apply_orientation))
    _raise_first_failed(decs, rcs)
    return out


def decode_scaled_to_tensor(ctx, desc, frames, scale, windows=None, stream=None):
    """Frames decoded at 1/scale (2, 4 or 8) as one dense uint8 tensor (zj_decode_crops_scaled_device): frames = a list of
    (Y, Cb, Cr) int16 CUDA tensors, one frame each (Cb / Cr may be None for GRAYSCALE output); windows = None (the whole
    reduced frame, ceil(width / scale) x ceil(height / scale)) or one (x, y, w, h) per frame in reduced pixels, all of one
    size (windows of different sizes are a ValueError).  Returns [N, h, w, C], [N, 3, h, w] or [N, h, w].  Stream and
    allocator rules as decode_to_tensor."""
    import torch
    from .host import scaled_size, scale_log2
    scale_log2(scale)
    if scale == 1:
        raise ValueError("scale must be 2, 4 or 8")
    n = len(frames)
    if n == 0 or (windows is not None and len(windows) != n):
        raise ValueError("one window per frame, at least one frame")
    if windows is None:
        w, h = scaled_size(desc, scale)
    else:
        sizes = {(int(wd[2]), int(wd[3])) for wd in windows}
        if len(sizes) != 1:
            raise ValueError("the windows of one call have one size")
        w, h = sizes.pop()
    crop_len = lib().zj_scaled_crop_out_len(C.byref(desc), scale_log2(scale), w, h, 0)
    if crop_len == 0:
        raise ValueError(f"{w}x{h} is not a valid window of this frame descriptor at 1/{scale}")
    dev = frames[0][0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    with torch.cuda.stream(s):
        storage = torch.empty(n * crop_len, dtype=torch.uint8, device=dev)
    _on_stream(s, cur, [p for fr in frames for p in fr])
    ptr = lambda t: t.data_ptr() if t is not None else None
    base = storage.data_ptr()
    ctx.decode_crops_scaled_device(desc, [ptr(fr[0]) for fr in frames], [ptr(fr[1]) for fr in frames],
                                   [ptr(fr[2]) for fr in frames], scale, [base + i * crop_len for i in range(n)], windows, 0,
                                   s.cuda_stream)
    return crop_view_of(desc, storage, n, w, h)


def _u8_images(images, in_layout):
    """images as the u8 entry points take them: (tensors, (w, h) each, row pitch each, channels)"""
    import torch
    if len(images) == 0:
        raise ValueError("at least one image")
    imgs, sizes, pitches = [], [], []
    for im in images:
        if im.dtype != torch.uint8 or not im.is_cuda:
            raise ValueError("images are uint8 CUDA tensors")
        if in_layout == "CHW":
            if im.dim() != 3 or im.shape[0] != 3:
                raise ValueError("CHW images are [3, H, W]")
            if im.stride(2) != 1 or im.stride(0) != im.stride(1) * im.shape[1]:
                im = im.contiguous()
            h, w, pitch = im.shape[1], im.shape[2], im.stride(1)
        else:
            im3 = im if im.dim() == 3 else im.unsqueeze(-1)
            if im3.dim() != 3 or im3.shape[2] not in (1, 3):
                raise ValueError("HWC images are [H, W, 3], [H, W, 1] or [H, W]")
            if im3.stride(2) != 1 or im3.stride(1) != im3.shape[2]:
                im3 = im3.contiguous()
            im = im3
            h, w, pitch = im.shape[0], im.shape[1], im.stride(0)
        imgs.append(im)
        sizes.append((w, h))
        pitches.append(pitch)
    channels = 3 if in_layout == "CHW" else imgs[0].shape[2]
    if any((3 if in_layout == "CHW" else im.shape[2]) != channels for im in imgs):
        raise ValueError("every image has the same channels")
    return imgs, sizes, pitches, channels


def orient_to_tensor(ctx, images, orientations, in_layout="HWC", stream=None):
    """u8 CUDA images turned to their displayed form (zj_orient_device): images as resize_to_tensor takes
    them, orientations = one EXIF orientation 1..8 each.  Returns a list of new contiguous tensors, [H', W', C] ([H', W'] for
    a two-dimensional input) or [3, H', W'], H' x W' the displayed size.  Streams as decode_to_tensor."""
    import torch
    from .host import oriented_size
    imgs, sizes, pitches, channels = _u8_images(images, in_layout)
    if len(orientations) != len(imgs):
        raise ValueError("one orientation per image")
    dev = imgs[0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    outs = []
    with torch.cuda.stream(s):
        for (w, h), o in zip(sizes, orientations):
            dw, dh = oriented_size(o, w, h)
            outs.append(torch.empty((3, dh, dw) if in_layout == "CHW" else (dh, dw, channels), dtype=torch.uint8, device=dev))
    _on_stream(s, cur, imgs)
    ctx.orient_device([im.data_ptr() for im in imgs], sizes, channels, LAYOUT_CHW if in_layout == "CHW" else LAYOUT_HWC,
                      orientations, [o.data_ptr() for o in outs], pitches, None, s.cuda_stream)
    return [o.squeeze(-1) if in_layout != "CHW" and im.dim() == 2 else o for o, im in zip(outs, images)]


def gray_to_rgb_tensor(ctx, images, out_layout="HWC", stream=None):
    """u8 CUDA planes -> 3-channel images with R = G = B (zj_gray_to_rgb_device): images = [H, W] (or
    [H, W, 1]) uint8 tensors of their own sizes; rows may be strided.  Returns a list of new contiguous tensors, [H, W, 3]
    ("HWC") or [3, H, W] ("CHW").  Streams as decode_to_tensor."""
    import torch
    if out_layout not in ("HWC", "CHW"):
        raise ValueError("out_layout is 'HWC' or 'CHW'")
    imgs, sizes, pitches, channels = _u8_images(images, "HWC")
    if channels != 1:
        raise ValueError("images are single planes: [H, W] or [H, W, 1]")
    dev = imgs[0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    with torch.cuda.stream(s):
        outs = [torch.empty((3, h, w) if out_layout == "CHW" else (h, w, 3), dtype=torch.uint8, device=dev) for w, h in sizes]
    _on_stream(s, cur, imgs)
    ctx.gray_to_rgb_device([im.data_ptr() for im in imgs], sizes, LAYOUT_CHW if out_layout == "CHW" else LAYOUT_HWC,
                           [o.data_ptr() for o in outs], pitches, None, s.cuda_stream)
    return outs


def cmyk_to_rgb_tensor(ctx, images, planes, layout="HWC", inverted=None, stream=None):
    """u8 CUDA images a ([H, W, 3] "HWC" or [3, H, W] "CHW") and planes k ([H, W]) of the same sizes -> new contiguous tensors
    (a * k + 127) // 255 in the same layout (zj_cmyk_to_rgb_device): Pillow's CMYK -> RGB.  inverted = one
    flag per image (None: all False): True uses the samples as stored (Adobe files), False complements them first.  Rows may
    be strided.  Streams as decode_to_tensor."""
    import torch
    if layout not in ("HWC", "CHW"):
        raise ValueError("layout is 'HWC' or 'CHW'")
    imgs, sizes, pitches, channels = _u8_images(images, layout)
    ks, ksizes, kpitches, kch = _u8_images(planes, "HWC")
    if channels != 3 or kch != 1 or sizes != ksizes:
        raise ValueError("one 3-channel image and one plane of the same size per pair")
    dev = imgs[0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    with torch.cuda.stream(s):
        outs = [torch.empty((3, h, w) if layout == "CHW" else (h, w, 3), dtype=torch.uint8, device=dev) for w, h in sizes]
    _on_stream(s, cur, imgs + ks)
    ctx.cmyk_to_rgb_device([im.data_ptr() for im in imgs], [k.data_ptr() for k in ks], sizes,
                           LAYOUT_CHW if layout == "CHW" else LAYOUT_HWC, [o.data_ptr() for o in outs], inverted, pitches,
                           kpitches, None, s.cuda_stream)
    return outs


_LUMA = (0.299, 0.587, 0.114)
# RGB -> YIQ (NTSC): the rows of I and Q sum to 0, so the inverse's first column is ones and a gray pixel keeps its value
_RGB_TO_YIQ = ((0.299, 0.587, 0.114), (0.595716, -0.274453, -0.321263), (0.211456, -0.522591, 0.311135))


def color_matrix(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, contrast_center=128.0, grayscale=False, bgr=False):
    """The float64 [3, 4] colour matrix of the colour stage: out[c] = m[c][0] R + m[c][1] G + m[c][2] B +
    m[c][3], in grey levels 0..255.  The steps are affine maps composed WITHOUT clamps between them, in this order:
    brightness b (b I), contrast c about contrast_center (c I, offset (1 - c) centre; Pillow's ImageEnhance.Contrast uses
    int(mean of L + 0.5) of the image, which the caller passes: the stage makes no reduction), saturation s
    (s I + (1 - s) W, every row of W the luma weights 0.299, 0.587, 0.114: ImageEnhance.Color, torchvision's
    adjust_saturation), hue: a rotation by `hue` TURNS (1.0 = 360 degrees) of the I, Q plane of YIQ, I' = cos I - sin Q,
    Q' = sin I + cos Q.  That is DALI's linear hue (hsv / color_twist), NOT torchvision's adjust_hue, which shifts H of HSV and
    is not linear.  grayscale: saturation 0 (RandomGrayscale, Pillow's convert("L") in all three channels).  bgr: rows 0 and 2
    swapped last (the output is B, G, R)."""
    import math
    import numpy as np
    eye = np.eye(3)
    lin, off = float(brightness) * eye, np.zeros(3)
    lin, off = float(contrast) * lin, float(contrast) * off + (1.0 - float(contrast)) * float(contrast_center)
    s = 0.0 if grayscale else float(saturation)
    sat = s * eye + (1.0 - s) * np.tile(np.asarray(_LUMA, np.float64), (3, 1))
    lin, off = sat @ lin, sat @ off
    if hue != 0.0:
        a = 2.0 * math.pi * float(hue)
        t = np.asarray(_RGB_TO_YIQ, np.float64)
        rot = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(a), -math.sin(a)], [0.0, math.sin(a), math.cos(a)]])
        h = np.linalg.inv(t) @ rot @ t
        lin, off = h @ lin, h @ off
    m = np.concatenate([lin, off[:, None]], axis=1)
    if bgr:
        m = m[::-1].copy()
    return np.ascontiguousarray(m, np.float64)


def color_twist_tensor(ctx, images, matrices, in_layout="HWC", inplace=False, stream=None):
    """u8 CUDA images under one [3, 4] colour matrix each (zj_color_device): images = [H, W, 3] ("HWC") or
    [3, H, W] ("CHW") uint8 tensors of their own sizes, rows may be strided; matrices = one per image (color_matrix; None: the
    identity).  out[c] = clamp((q[c] . (R, G, B, 1) + 32768) >> 16, 0, 255) with q = floor(m 65536 + 1/2), exact integers.
    Returns a list of new contiguous tensors in the same layout; inplace=True: the images themselves are written (each must
    be usable as it is: unit stride inside a row, CHW planes H rows apart) and returned.  Streams as decode_to_tensor."""
    import torch
    if in_layout not in ("HWC", "CHW"):
        raise ValueError("in_layout is 'HWC' or 'CHW'")
    imgs, sizes, pitches, channels = _u8_images(images, in_layout)
    if channels != 3:
        raise ValueError("colour matrices map 3-channel images")
    if len(matrices) != len(imgs):
        raise ValueError("one colour matrix per image")
    if inplace and any(a is not b for a, b in zip(imgs, images)):
        raise ValueError("inplace needs images that are used as they are (3 dimensions, unit stride inside a row)")
    dev = imgs[0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    if inplace:
        outs, opitches = imgs, pitches
    else:
        with torch.cuda.stream(s):
            outs = [torch.empty((3, h, w) if in_layout == "CHW" else (h, w, 3), dtype=torch.uint8, device=dev) for w, h in sizes]
        opitches = None
    _on_stream(s, cur, imgs)
    ctx.color_device([im.data_ptr() for im in imgs], sizes, LAYOUT_CHW if in_layout == "CHW" else LAYOUT_HWC, matrices,
                     [o.data_ptr() for o in outs], pitches, opitches, s.cuda_stream)
    return outs


def tone_op(kind, param=0):
    """The (op, param) pair of a tone op: kind = "identity", "invert", "posterize" (param: bits 1..8),
    "solarize" (param: threshold 0..256), "autocontrast" or "equalize" (or the TONE_* code).  Each is Pillow's ImageOps
    function of that name, byte for byte; autocontrast with cutoff 0, equalize without a mask."""
    from .host import TONE_OPS, TONE_POSTERIZE, TONE_SOLARIZE
    op = TONE_OPS[kind] if isinstance(kind, str) else int(kind)
    param = int(param)
    if op not in TONE_OPS.values():
        raise ValueError("not a tone op")
    lo, hi = {TONE_POSTERIZE: (1, 8), TONE_SOLARIZE: (0, 256)}.get(op, (0, 0))
    if not lo <= param <= hi:
        raise ValueError(f"this op's param is {lo}..{hi}")
    return (op, param)


def gamma_lut(gamma, gain=1.0):
    """A uint8 [3, 256] table for lut_tensor: min(255, int(255 * gain * (i / 255) ** gamma + 0.5)) in every channel.  A
    helper: the stage applies whatever table it is given."""
    import numpy as np
    i = np.arange(256, dtype=np.float64) / 255.0
    t = np.minimum(255, (255.0 * float(gain) * i ** float(gamma) + 0.5).astype(np.int64))
    return np.ascontiguousarray(np.tile(np.maximum(t, 0).astype(np.uint8), (3, 1)))


def _tone_images(images, in_layout):
    if in_layout not in ("HWC", "CHW"):
        raise ValueError("in_layout is 'HWC' or 'CHW'")
    return _u8_images(images, in_layout)


def histogram_tensor(ctx, images, in_layout="HWC", stream=None):
    """The histograms of u8 CUDA images (zj_histogram_device): images = [H, W, 3], [H, W, 1], [H, W] ("HWC")
    or [3, H, W] ("CHW") uint8 tensors of their own sizes, rows may be strided.  Returns an int32 CUDA tensor
    [N, channels, 256] (the counts are below 2^32; a count of 2^31 or more reads as negative).  Streams as decode_to_tensor."""
    import torch
    imgs, sizes, pitches, channels = _tone_images(images, in_layout)
    dev = imgs[0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    with torch.cuda.stream(s):
        hist = torch.empty((len(imgs), channels, 256), dtype=torch.int32, device=dev)
    _on_stream(s, cur, imgs)
    ctx.histogram_device([im.data_ptr() for im in imgs], sizes, channels, LAYOUT_CHW if in_layout == "CHW" else LAYOUT_HWC,
                         hist.data_ptr(), pitches, s.cuda_stream)
    return hist


def _tone_outputs(torch, imgs, images, sizes, pitches, channels, in_layout, inplace, s):
    if inplace:
        if any(a is not b and a.data_ptr() != b.data_ptr() for a, b in zip(imgs, images)):
            raise ValueError("inplace needs images that are used as they are (unit stride inside a row)")
        return imgs, pitches
    dev = imgs[0].device
    with torch.cuda.stream(s):
        outs = [torch.empty((3, h, w) if in_layout == "CHW" else (h, w, channels), dtype=torch.uint8, device=dev) for w, h in sizes]
    return outs, None


def lut_tensor(ctx, images, luts, in_layout="HWC", inplace=False, stream=None):
    """u8 CUDA images through tables, out[c] = luts[i][c][in[c]] (zj_lut_device): luts = a uint8
    [N, channels, 256] CUDA tensor or array, or one [channels, 256] table for every image (gamma_lut, any tone curve).
    Returns new contiguous tensors in the same layout; inplace=True writes the images themselves.  Streams as
    decode_to_tensor."""
    import torch
    imgs, sizes, pitches, channels = _tone_images(images, in_layout)
    dev = imgs[0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    with torch.cuda.stream(s):
        t = torch.as_tensor(luts, dtype=torch.uint8).to(dev)
        if t.dim() == 2:
            t = t.unsqueeze(0).expand(len(imgs), -1, -1)
        if tuple(t.shape) != (len(imgs), channels, 256):
            raise ValueError("luts are [N, channels, 256] or [channels, 256]")
        t = t.contiguous()
    outs, opitches = _tone_outputs(torch, imgs, images, sizes, pitches, channels, in_layout, inplace, s)
    _on_stream(s, cur, imgs)
    ctx.lut_device([im.data_ptr() for im in imgs], sizes, channels, LAYOUT_CHW if in_layout == "CHW" else LAYOUT_HWC, t.data_ptr(),
                   [o.data_ptr() for o in outs], pitches, opitches, s.cuda_stream)
    t.record_stream(s)
    return outs


def tone_tensor(ctx, images, ops, in_layout="HWC", inplace=False, stream=None):
    """u8 CUDA images each under its own tone op (zj_tone_device): ops = one tone_op each (None: the
    identity).  Autocontrast and equalize use each image's own histogram, computed on the device; nothing is synchronised.
    Returns new contiguous tensors in the same layout; inplace=True writes the images themselves (an identity image then
    costs no launch).  Streams as decode_to_tensor."""
    import torch
    imgs, sizes, pitches, channels = _tone_images(images, in_layout)
    if len(ops) != len(imgs):
        raise ValueError("one tone op per image")
    cur = torch.cuda.current_stream(imgs[0].device)
    s = stream if stream is not None else cur
    outs, opitches = _tone_outputs(torch, imgs, images, sizes, pitches, channels, in_layout, inplace, s)
    _on_stream(s, cur, imgs)
    ctx.tone_device([im.data_ptr() for im in imgs], sizes, channels, LAYOUT_CHW if in_layout == "CHW" else LAYOUT_HWC, ops,
                    [o.data_ptr() for o in outs], pitches, opitches, s.cuda_stream)
    return outs


def planes_to_rgb_tensor(ctx, planes, sizes, ratios, layout="HWC", stored_rgb=False, stream=None):
    """Three u8 CUDA planes ([h_k, w_k] each) per image -> new contiguous RGB tensors ([H, W, 3] "HWC" or [3, H, W] "CHW"),
    pixel (r, c) = colour(p0[r // ry0][c // rx0], p1[...], p2[...]) (zj_planes_to_rgb_device): planes = one
    (p0, p1, p2) per image, sizes = one (W, H) of the output each, ratios = ((rx0, ry0), (rx1, ry1), (rx2, ry2)) each, every
    ratio 1, 2 or 4; plane k must hold ceil(W / rx_k) x ceil(H / ry_k) samples.  colour is the full decode's YCbCr -> RGB,
    with stored_rgb the identity.  Rows may be strided.  Streams as decode_to_tensor."""
    import torch
    if layout not in ("HWC", "CHW"):
        raise ValueError("layout is 'HWC' or 'CHW'")
    n = len(planes)
    if n == 0 or len(sizes) != n or len(ratios) != n:
        raise ValueError("three planes, a size and three ratio pairs per image")
    ps, pitches = [[], [], []], []
    for trio, (w, h), rs in zip(planes, sizes, ratios):
        if len(trio) != 3 or len(rs) != 3:
            raise ValueError("three planes and three ratio pairs per image")
        ims, szs, pit, ch = _u8_images(list(trio), "HWC")
        if ch != 1 or any(r not in (1, 2, 4) for pair in rs for r in pair):
            raise ValueError("one-channel planes and ratios 1, 2 or 4")
        for k in range(3):
            if szs[k] != (-(-int(w) // rs[k][0]), -(-int(h) // rs[k][1])):
                raise ValueError("plane %d is not ceil(W / rx) x ceil(H / ry)" % k)
            ps[k].append(ims[k])
        pitches.append(pit)
    dev = ps[0][0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    with torch.cuda.stream(s):
        outs = [torch.empty((3, int(h), int(w)) if layout == "CHW" else (int(h), int(w), 3), dtype=torch.uint8, device=dev)
                for w, h in sizes]
    _on_stream(s, cur, ps[0] + ps[1] + ps[2])
    ctx.planes_to_rgb_device([t.data_ptr() for t in ps[0]], [t.data_ptr() for t in ps[1]], [t.data_ptr() for t in ps[2]],
                             [(int(w), int(h)) for w, h in sizes], ratios, LAYOUT_CHW if layout == "CHW" else LAYOUT_HWC,
                             [o.data_ptr() for o in outs], stored_rgb, pitches, None, s.cuda_stream)
    return outs


def resize_to_tensor(ctx, images, size, dtype=None, layout="NCHW", in_layout="HWC", mean=None, std=None, flips=None,
                     stream=None, antialias=False, orientations=None, interpolation="bilinear"):
    """u8 CUDA images of their own sizes resized and normalised into ONE dense tensor (zj_resize_device): images =
    [H, W, C] or [H, W] tensors (in_layout "HWC"), or [3, H, W] ("CHW"); rows may be strided, pixels not.  Output,
    mean / std, flips, streams, antialias and interpolation as decode_resized_crops_to_tensor.  orientations: one EXIF
    orientation 1..8 per image, applied first (orient_to_tensor); None: none."""
    import torch
    from .host import resize_filter
    resize_filter(antialias, interpolation)
    dtype = torch.bfloat16 if dtype is None else dtype
    code = _resize_dtype(dtype)
    if orientations is not None:
        images = orient_to_tensor(ctx, images, orientations, in_layout, stream)
    imgs, sizes, pitches, channels = _u8_images(images, in_layout)
    n = len(imgs)
    scale, bias = normalize_factors(channels, mean, std)
    dev = imgs[0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    out = _resized_out(n, channels, size, dtype, layout, dev, s)
    _on_stream(s, cur, imgs)
    ctx.resize_device([im.data_ptr() for im in imgs], sizes, channels, LAYOUT_CHW if in_layout == "CHW" else LAYOUT_HWC,
                      size[0], size[1], code, TENSOR_NCHW if layout == "NCHW" else TENSOR_NHWC, out.data_ptr(), scale, bias,
                      flips, pitches, s.cuda_stream, antialias, interpolation)
    return out


def to_normalized_tensor(ctx, images, dtype=None, layout="NCHW", mean=None, std=None, flips=None, channels=None, stream=None):
    """u8 CUDA images of ONE size converted and normalised into one dense tensor, NOT resized (zj_to_tensor_device, DESIGN.md
    3.15): images = [h, w, 3], [h, w, 1] or [h, w] tensors, all of one size, contiguous or row-strided.  channels: of the
    output (None: the images'); 3 from one-channel images puts the byte into all three channels, each with its own mean /
    std.  Returns [N, C, h, w] ("NCHW") or [N, h, w, C] ("NHWC") of `dtype` (default bfloat16).  mean / std, flips and
    streams as resize_to_tensor.  No size limit but 65535 a side."""
    import torch
    dtype = torch.bfloat16 if dtype is None else dtype
    code = _resize_dtype(dtype)
    imgs, sizes, pitches, cin = _u8_images(images, "HWC")
    if any(sz != sizes[0] for sz in sizes):
        raise ValueError("every image has the same size")
    channels = cin if channels is None else int(channels)
    if channels not in (1, 3) or (cin == 3 and channels == 1):
        raise ValueError("channels is 1 or 3, and 3 for 3-channel images")
    n = len(imgs)
    scale, bias = normalize_factors(channels, mean, std)
    dev = imgs[0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    out = _resized_out(n, channels, sizes[0], dtype, layout, dev, s)
    _on_stream(s, cur, imgs)
    ctx.to_tensor_device([im.data_ptr() for im in imgs], sizes[0][0], sizes[0][1], cin, channels, code,
                         TENSOR_NCHW if layout == "NCHW" else TENSOR_NHWC, out.data_ptr(), scale, bias, flips, pitches, s.cuda_stream)
    return out


def warp_matrix(out_size, center, angle=0.0, scale=1.0, shear=(0.0, 0.0), translate=(0.0, 0.0), hflip=False):
    """The matrix (a, b, c, d, e, f) of float64 that warp_to_tensor and its kin take -- output pixel centre -> continuous
    source coordinates, x to the right, y DOWN, pixel i covering [i, i + 1) -- for an augmentation given the forward way.
    With out_size = (out_w, out_h) and homogeneous 3 x 3 matrices acting on source coordinates,

        M = T(out_w / 2 + tx, out_h / 2 + ty) . R(angle) . Sh(shear) . S(scale) . [F] . T(-cx, -cy)

    takes a source point to its place in the output, and the result is the first two rows of M^-1:
        T(x, y)    the translation by (x, y); center = (cx, cy) is the source point that lands on the output's centre,
                   moved by translate = (tx, ty) output pixels
        F          diag(-1, 1): the source mirrored left to right about `center` first (hflip)
        S(scale)   diag(sx, sy), scale a number or (sx, sy): > 1 enlarges
        Sh(shear)  [[1, tan shx], [tan shy, 1]], shear = (shx, shy) in degrees
        R(angle)   [[cos t, sin t], [-sin t, cos t]], t = angle in degrees: with y down, a positive angle turns the image
                   COUNTER-clockwise as displayed (90 is numpy's rot90)
    A letterbox of a w x h image into S x S is warp_matrix((S, S), (w / 2, h / 2), scale=min(S / w, S / h)) with edge
    "fill"; ValueError: a singular M."""
    import math
    import numpy as np
    ow, oh = out_size
    sx, sy = (scale, scale) if np.isscalar(scale) else scale
    t = math.radians(angle)

    def T(x, y):
        return np.array([[1.0, 0.0, x], [0.0, 1.0, y], [0.0, 0.0, 1.0]])

    def L(m00, m01, m10, m11):
        return np.array([[m00, m01, 0.0], [m10, m11, 0.0], [0.0, 0.0, 1.0]])

    M = T(ow / 2.0 + translate[0], oh / 2.0 + translate[1]) @ L(math.cos(t), math.sin(t), -math.sin(t), math.cos(t)) \
        @ L(1.0, math.tan(math.radians(shear[0])), math.tan(math.radians(shear[1])), 1.0) @ L(float(sx), 0.0, 0.0, float(sy)) \
        @ L(-1.0 if hflip else 1.0, 0.0, 0.0, 1.0) @ T(-float(center[0]), -float(center[1]))
    det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    if not math.isfinite(det) or det == 0.0:
        raise ValueError("warp_matrix: the map is singular")
    inv = np.linalg.inv(M)
    return tuple(float(v) for v in inv[:2].reshape(-1))


def warp_to_tensor(ctx, images, matrices, size, dtype=None, layout="NCHW", mean=None, std=None, fill=None, edge="fill",
                   stream=None):
    """u8 CUDA images of their own sizes, each under its own affine map, into ONE dense normalised tensor (zj_warp_device,
    DESIGN.md 3.16): images = [H, W, 3], [H, W, 1] or [H, W] tensors, rows may be strided; matrices = one (a, b, c, d, e, f)
    per image, output pixel centre -> source coordinates (warp_matrix builds them); size = (out_w, out_h).  Bilinear taps,
    not antialiased.  edge "fill": outside the image the taps read fill, one byte 0..255 per channel (None: 0), which
    becomes (fill / 255 - mean) / std; "replicate": the image's edge pixels.  Output, dtype, mean / std and streams as
    resize_to_tensor."""
    import torch
    from .host import warp_edge
    warp_edge(edge)
    dtype = torch.bfloat16 if dtype is None else dtype
    code = _resize_dtype(dtype)
    imgs, sizes, pitches, channels = _u8_images(images, "HWC")
    n = len(imgs)
    if len(matrices) != n:
        raise ValueError("one matrix per image")
    scale, bias = normalize_factors(channels, mean, std)
    dev = imgs[0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    out = _resized_out(n, channels, size, dtype, layout, dev, s)
    _on_stream(s, cur, imgs)
    ctx.warp_device([im.data_ptr() for im in imgs], sizes, channels, matrices, size[0], size[1], code,
                    TENSOR_NCHW if layout == "NCHW" else TENSOR_NHWC, out.data_ptr(), scale, bias, fill, edge, pitches,
                    s.cuda_stream)
    return out


def decode_warped_to_tensor(ctx, desc, frames, matrices, size, dtype=None, layout="NCHW", mean=None, std=None, fill=None,
                            edge="fill", stream=None):
    """Frames of one geometry decoded and warped into ONE dense normalised tensor (zj_decode_crops_warped_device, DESIGN.md
    3.16): frames as decode_resized_crops_to_tensor takes them, matrices = one per frame in FRAME pixels (warp_matrix).  Only
    the part of each frame its output can see is decoded; the result is warp_to_tensor's of the whole decoded frame.
    desc.flags | FLAG_GRAY_TO_RGB as decode_resized_crops_to_tensor.  The other arguments as warp_to_tensor."""
    import torch
    from .host import warp_edge
    warp_edge(edge)
    dtype = torch.bfloat16 if dtype is None else dtype
    code = _resize_dtype(dtype)
    n = len(frames)
    if n == 0 or len(matrices) != n:
        raise ValueError("one matrix per frame, at least one frame")
    ow, oh = size
    if lib().zj_resized_out_len(C.byref(desc), ow, oh, code) == 0:
        raise ValueError(f"{ow}x{oh} {dtype} is not a supported warped output of this frame descriptor")
    channels = ColorSpace(desc.out_colorspace).num_components()
    scale, bias = normalize_factors(channels, mean, std)
    dev = frames[0][0].device
    cur = torch.cuda.current_stream(dev)
    s = stream if stream is not None else cur
    out = _resized_out(n, channels, size, dtype, layout, dev, s)
    _on_stream(s, cur, [p for fr in frames for p in fr])
    ptr = lambda t: t.data_ptr() if t is not None else None
    ctx.decode_crops_warped_device(desc, [ptr(fr[0]) for fr in frames], [ptr(fr[1]) for fr in frames],
                                   [ptr(fr[2]) for fr in frames], matrices, ow, oh, code,
                                   TENSOR_NCHW if layout == "NCHW" else TENSOR_NHWC, out.data_ptr(), scale, bias, fill, edge,
                                   s.cuda_stream)
    return out


def decode_files_warped_to_tensor(ctx, blobs, matrices, size, dtype=None, layout="NCHW", mean=None, std=None, fill=None,
                                  edge="fill", apply_orientation=False, options=None, workers=1, stream=None, decoders=None):
    """JPEG files of ANY sizes, each under its own affine map, -> ONE dense normalised tensor: blobs = a list of
    bytes-like JPEG files, matrices = one (a, b, c, d, e, f) per file, output pixel centre -> coordinates of the file's frame
    (of its DISPLAYED frame with apply_orientation; warp_matrix builds them), size = (out_w, out_h).  Image k is
    Decoder.finish_pixels_warped_device's for file k (zj_decoder_finish_pixels_warped_batch_device): only the part of each
    frame its output sees is decoded, ordinary files in shared launches.  fill and edge as warp_to_tensor; dtype, mean / std,
    options (FLAG_GRAY_TO_RGB, FLAG_CMYK_TO_RGB, FLAG_ANY_SAMPLING included), workers, decoders and stream as
    decode_files_resized_to_tensor.  The batch call runs on the context's stream and has finished when it returns; a file
    that fails raises DecodeError naming its index (its image is untouched, the others are decoded)."""
    import torch
    from .host import finish_pixels_warped_batch, warp_edge
    warp_edge(edge)
    dtype = torch.bfloat16 if dtype is None else dtype
    code = _resize_dtype(dtype)
    n = len(blobs)
    if n == 0 or len(matrices) != n:
        raise ValueError("one matrix per file, at least one file")
    decs, prepared = _prepare_files(ctx, blobs, options, workers, decoders)
    out, scale, bias = _files_out(ctx, decs, "warped outputs", size, dtype, layout, mean, std, stream)
    rcs = finish_pixels_warped_batch(decs, ctx, matrices, size[0], size[1], code, TENSOR_NCHW if layout == "NCHW" else TENSOR_NHWC,
                                     out.data_ptr(), out.numel() * out.element_size(), scale, bias, fill, edge,
                                     bool(apply_orientation))
    _raise_first_failed(decs, rcs)
    return out

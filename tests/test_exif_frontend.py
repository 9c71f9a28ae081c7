"""CPU: the EXIF Orientation tag as the front-end reads it (zj_decoder_orientation) -- real files, APP1
segments built here and spliced in behind SOI, against Pillow's reader and tests/orient_model.py's; and damaged segments
(cut at every byte, lengths that lie, offsets and counts past the end), which must read as 1 or as the value, change nothing
of what the decoder does with the file, and never read outside it."""
import importlib
import io
import os
import struct
import zlib

import pytest

import orient_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
OTHER = (0x010F, 2, 4, b"zj\0\0")   # Make, ASCII
OTHER2 = (0x0128, 3, 1, struct.pack("<HH", 2, 0))  # ResolutionUnit (its bytes suit either order: the value is not read)


@pytest.fixture(scope="module")
def zj():
    return importlib.import_module("zune-jpeg_amd")


@pytest.fixture(scope="module")
def base():
    return open(os.path.join(GOLD, "test-baseline.jpg"), "rb").read()


def read(zj, data):
    """the orientation after read_headers, whether or not the file parses"""
    d = zj.Decoder()
    assert d.orientation == 0
    try:
        d.read_headers(data)
    except zj.DecodeError:
        pass
    return d.orientation


def pillow(data):
    from PIL import Image
    return Image.open(io.BytesIO(data)).getexif().get(0x0112)


def plane_hash(zj, data):
    d = zj.Decoder()
    _, planes, info = d.decode_coefficients(data, copy=False)
    return [zlib.crc32(p.tobytes()) for p in planes], (info.width, info.height), d.orientation


def test_real_files(zj, base):
    real = open(os.path.join(GOLD, "ref", "medium_horiz_samp_2500x1786.jpg"), "rb").read()
    assert b"Exif\0\0" in real[:4096] and pillow(real) == 1 and om.exif_orientation(real) == 1
    assert read(zj, real) == 1
    assert b"Exif\0\0" not in base and read(zj, base) == 1 and pillow(base) is None
    d = zj.Decoder()
    d.read_headers(om.splice(base, om.exif_segment(6)))
    assert d.orientation == 6
    d.read_headers(base)  # (the next file starts from 1 again)
    assert d.orientation == 1


@pytest.mark.parametrize("order", ["<", ">"])
def test_built_segments(zj, base, order):
    cases = []
    for v in range(10):
        cases.append((om.exif_segment(v, order), v if 1 <= v <= 8 else 1, v))
    cases.append((om.exif_segment(5, order, after=[OTHER, OTHER2]), 5, 5))                   # first of several
    cases.append((om.exif_segment(7, order, before=[OTHER], after=[OTHER2]), 7, 7))          # in the middle
    cases.append((om.exif_segment(8, order, before=[OTHER, OTHER2]), 8, 8))                  # last
    cases.append((om.exif_segment(3, order, before=[OTHER], ifd_offset=26), 3, 3))           # IFD0 not at 8
    cases.append((om.exif_segment(None, order, before=[OTHER]), 1, None))                    # no such entry
    for seg, want, raw in cases:
        data = om.splice(base, seg)
        assert read(zj, data) == want and om.exif_orientation(data) == want
        assert pillow(data) == raw
    two = om.splice(base, om.exif_segment(6, order), om.exif_segment(3, order))
    assert read(zj, two) == 6 and om.exif_orientation(two) == 6                              # the first decides
    none_then = om.splice(base, om.exif_segment(None, order), om.exif_segment(3, order))
    assert read(zj, none_then) == 1                                                          # ... even when it says nothing
    xmp = b"\xff\xe1" + struct.pack(">H", 2 + 34) + b"http://ns.adobe.com/xap/1.0/\0" + b"<x/>\0\0"
    front = om.splice(base, xmp, om.exif_segment(4, order))
    assert read(zj, front) == 4 and om.exif_orientation(front) == 4 and pillow(front) == 4   # a non-Exif APP1 is skipped
    for typ, cnt in ((4, 1), (3, 2), (1, 1)):
        assert read(zj, om.splice(base, om.exif_segment(6, order, typ=typ, count=cnt))) == 1


@pytest.mark.parametrize("order", ["<", ">"])
def test_damaged_segments_read_as_1_or_the_value_and_change_nothing(zj, base, order):
    V = 6
    seg = om.exif_segment(V, order, before=[OTHER], after=[OTHER2])
    want_planes, want_size, _ = plane_hash(zj, base)
    assert base[2:4] == b"\xff\xe0"
    app0 = 2 + struct.unpack(">H", base[4:6])[0]
    payload = seg[4:]

    def same_decode(data, allowed):
        planes, size, o = plane_hash(zj, data)
        assert planes == want_planes and size == want_size
        assert o in allowed and read(zj, data) == o
        return o

    assert same_decode(om.splice(base, seg), {V}) == V
    seen = set()
    for k in range(len(payload) + 1):
        # the payload cut to k bytes inside a segment that says so: the file parses as ever
        cut = b"\xff\xe1" + struct.pack(">H", k + 2) + payload[:k]
        seen.add(same_decode(om.splice(base, cut), {1, V}))
        # the FILE cut there: nothing behind the k bytes, the declared length past the buffer's end
        assert read(zj, b"\xff\xd8" + seg[:4 + k]) in (1, V)
        # a declared length of k + 2 in front of the whole payload: the rest lies between the markers, where the loop skips it
        if 0xFF not in payload[k:]:
            lied = b"\xff\xe1" + struct.pack(">H", k + 2) + payload
            seen.add(same_decode(om.splice(base, lied), {1, V}))
    assert seen == {1, V}
    # a declared length that takes the JFIF segment behind it along: still the same image
    longer = b"\xff\xe1" + struct.pack(">H", len(payload) + 2 + app0) + payload
    assert same_decode(om.splice(base, longer), {V}) == V
    # IFD0 offsets and entry counts that point past the end
    tiff = bytearray(payload[6:])
    for off in (len(tiff) - 1, len(tiff), len(tiff) + 1, 0xFFFFFFFF, 0x7FFFFFFF, 0xFFFFFFF6):
        t = bytearray(tiff)
        t[4:8] = struct.pack(order + "I", off)
        bad = b"\xff\xe1" + struct.pack(">H", len(t) + 8) + b"Exif\0\0" + bytes(t)
        assert same_decode(om.splice(base, bad), {1}) == 1
    for cnt in (4, 100, 0xFFFF):
        t = bytearray(tiff)
        t[8:10] = struct.pack(order + "H", cnt)
        bad = b"\xff\xe1" + struct.pack(">H", len(t) + 8) + b"Exif\0\0" + bytes(t)
        assert same_decode(om.splice(base, bad), {1, V}) == V  # (the tag lies in front of where the entries run out)
    t = bytearray(tiff)
    t[8:10] = struct.pack(order + "H", 0xFFFF)
    t[10 + 12:10 + 14] = struct.pack(order + "H", 0x0113)      # no Orientation among the entries that exist
    bad = b"\xff\xe1" + struct.pack(">H", len(t) + 8) + b"Exif\0\0" + bytes(t)
    assert same_decode(om.splice(base, bad), {1}) == 1


def test_strict_mode_and_error_strings_are_as_before(zj, base):
    """the parse only looks: a segment length below 2 is the same error with and without the Exif signature"""
    o = zj.ZuneJpegOptions()
    o.strict_mode = True
    d = zj.Decoder(o)
    d.read_headers(om.splice(base, om.exif_segment(3)))
    assert d.orientation == 3
    for body in (b"Exif\0\0II*\0", b"Abcd\0\0II*\0"):
        with pytest.raises(zj.DecodeError) as e:
            zj.Decoder().read_headers(b"\xff\xd8\xff\xe1\x00\x01" + body + base[2:])
        assert "Found a marker with invalid length:1" in str(e.value)

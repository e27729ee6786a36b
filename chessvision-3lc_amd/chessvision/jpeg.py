"""JPEG decode: the host half (ctypes over ``csrc/jpeg.cpp``) and the numpy host form of the device half.

``jpeg_info`` and ``entropy_decode`` call the library's host-only entry points (no engine, no GPU): the marker parser and the
Huffman stage, which turn a baseline JPEG stream into quantised coefficients.  ``reconstruct`` restates, in vectorised integer
numpy, what ``csrc/jpeg.hip`` does with those coefficients on the device: dequantise, libjpeg's "islow" integer inverse DCT, its
fancy chroma up-sampling and its fixed-point YCbCr -> RGB conversion.  As everywhere in this package the numpy form is the readable
checker: it shares no code with the kernel, and both are held to the bytes libjpeg itself produces (Pillow and ``cv2.imdecode``
decode with libjpeg's defaults).  All arithmetic wraps in 32 bits, so the two forms agree on any coefficients.
``apply_orientation`` is the numpy form of the EXIF orientation the oriented colour kernel applies in its store
(``orientation="exif"`` on the JPEG entries; the default ``"ignore"`` leaves the tag reported and unused).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

ORDERS = {"bgr": 0, "rgb": 1, "gray": 2}


class UnsupportedJpeg(ValueError):
    """A stream this library does not decode (progressive, arithmetic, 12-bit, CMYK, other sampling factors, several scans) or one
    that is truncated or corrupt.  ``reasons`` maps the index of each refused blob to the parser's reason."""

    def __init__(self, reasons):
        self.reasons = dict(reasons)
        super().__init__("unsupported JPEG stream(s): " + "; ".join(f"[{i}] {r}" for i, r in sorted(self.reasons.items())))


class _Info(ctypes.Structure):                    # mirrors cv_jpeg_info_t (include/chessvision_hip.h)
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("components", ctypes.c_int32), ("luma_h", ctypes.c_int32),
                ("luma_v", ctypes.c_int32), ("restart_interval", ctypes.c_int32), ("orientation", ctypes.c_int32),
                ("supported", ctypes.c_int32), ("reason", ctypes.c_char * 160)]


class JpegInfo(NamedTuple):
    width: int
    height: int
    components: int
    luma_h: int
    luma_v: int
    restart_interval: int
    orientation: int          # EXIF tag 0x0112 as found (1..8), 0 when absent; applied only under orientation="exif"
    supported: bool
    reason: str

    @property
    def geometry(self):
        """What one device launch needs its images to share."""
        return (self.width, self.height, self.components, self.luma_h, self.luma_v)

    @property
    def plane_blocks(self):
        """((block_rows, block_cols), ...) of each component plane, padded to whole MCUs."""
        if self.components == 1:
            return (((self.height + 7) // 8, (self.width + 7) // 8),)
        my, mx = -(-self.height // (8 * self.luma_v)), -(-self.width // (8 * self.luma_h))
        return ((my * self.luma_v, mx * self.luma_h), (my, mx), (my, mx))

    @property
    def blocks(self):
        return sum(r * c for r, c in self.plane_blocks)

    def to_c(self) -> _Info:
        return _Info(self.width, self.height, self.components, self.luma_h, self.luma_v, self.restart_interval, self.orientation,
                     int(self.supported), self.reason.encode()[:159])


def _lib():
    from .hip_backend import load_library
    return load_library()


def _buffer(blob):
    blob = bytes(blob) if not isinstance(blob, (bytes, np.ndarray)) else blob
    if isinstance(blob, np.ndarray):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        return blob, blob.ctypes.data, blob.size
    return blob, ctypes.cast(ctypes.c_char_p(blob), ctypes.c_void_p).value, len(blob)


def jpeg_info(blob) -> JpegInfo:
    """The header of a JPEG stream.  Never raises for a bad stream: ``supported`` is False and ``reason`` says why."""
    keep, addr, n = _buffer(blob)
    if n == 0:
        return JpegInfo(0, 0, 0, 0, 0, 0, 0, False, "empty buffer at byte 0")
    c = _Info()
    from .hip_backend import _check
    _check(_lib().cv_jpeg_info(addr, n, ctypes.byref(c)))
    return JpegInfo(c.width, c.height, c.components, c.luma_h, c.luma_v, c.restart_interval, c.orientation, bool(c.supported),
                    c.reason.decode(errors="replace"))


def entropy_decode(blob, info: JpegInfo | None = None, coeffs: np.ndarray | None = None, qtables: np.ndarray | None = None):
    """The Huffman stage: ``(coeffs, qtables, info)``.  ``coeffs`` is a flat int16 array of ``64 * info.blocks`` quantised
    coefficients, ``[component][block_row][block_col][64]`` in natural order, ``qtables`` uint16 ``(components, 64)``.  Both may be
    given (views of a page-locked staging buffer, say) and are then written in place.  The call releases the GIL: the copy threads of
    ``process_encoded`` run one image each.  Raises ``UnsupportedJpeg`` for a refused, truncated or corrupt stream."""
    keep, addr, n = _buffer(blob)
    if info is None:
        info = jpeg_info(keep)
    if not info.supported:
        raise UnsupportedJpeg({0: info.reason})
    count = 64 * info.blocks
    if coeffs is None:
        coeffs = np.empty(count, np.int16)
    if qtables is None:
        qtables = np.empty((info.components, 64), np.uint16)
    if coeffs.dtype != np.int16 or coeffs.size < count or not coeffs.flags.c_contiguous or not coeffs.flags.writeable:
        raise ValueError("coeffs must be a writable contiguous int16 array of at least 64 * info.blocks elements")
    if qtables.dtype != np.uint16 or qtables.size < 64 * info.components or not qtables.flags.c_contiguous or not qtables.flags.writeable:
        raise ValueError("qtables must be a writable contiguous uint16 array of components * 64 elements")
    lib = _lib()
    if lib.cv_jpeg_entropy_decode(addr, n, coeffs.ctypes.data, coeffs.size, qtables.ctypes.data) != 0:
        msg = lib.cv_last_error()
        raise UnsupportedJpeg({0: msg.decode(errors="replace") if msg else "unknown error"})
    return coeffs, qtables, info


def parse_all(blobs) -> list[JpegInfo]:
    """The headers of all blobs; raises ``UnsupportedJpeg`` listing every refused index with its reason."""
    infos = [jpeg_info(b) for b in blobs]
    bad = {i: f.reason for i, f in enumerate(infos) if not f.supported}
    if bad:
        raise UnsupportedJpeg(bad)
    return infos


def entropy_decode_many(blobs, infos, coeffs: np.ndarray, qtables: np.ndarray, pool=None, threads: int = 8) -> None:
    """Image k of ``blobs`` into row k of ``coeffs`` (n, 64 * blocks) int16 and ``qtables`` (n, components, 64) uint16, one image per
    thread of ``pool`` (a ``ThreadPoolExecutor``; a temporary one of ``threads`` threads when None).  The rows may be page-locked."""
    def one(k):
        try:
            entropy_decode(blobs[k], infos[k], coeffs[k], qtables[k])
        except UnsupportedJpeg as exc:
            raise UnsupportedJpeg({k: exc.reasons[0]}) from None

    n = len(blobs)
    if n == 1:
        one(0)
    elif pool is not None:
        list(pool.map(one, range(n)))
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=max(1, min(threads, n))) as own:
            list(own.map(one, range(n)))


# ---- the numpy host form of csrc/jpeg.hip ----------------------------------------------------------------------------------
def _i32(x):
    return np.asarray(x).astype(np.int32)


def _idct_pass(v, shift):
    """jidctint.c's 8-point pass along axis 0 of an int32 array (8, ...); every operation wraps in 32 bits."""
    c = lambda k: np.int32(k)                                               # noqa: E731
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * c(4433)
    tmp2 = z1 + z3 * c(-15137)
    tmp3 = z1 + z2 * c(6270)
    tmp0 = (v[0] + v[4]) << 13
    tmp1 = (v[0] - v[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * c(9633)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * c(2446), tmp1 * c(16819), tmp2 * c(25172), tmp3 * c(12299)
    z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = c(1 << (shift - 1))
    rows = (tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3)
    return np.stack([(r + half) >> shift for r in rows])


def _planes(coeffs, qtables, info: JpegInfo):
    """Dequantise + inverse DCT: one uint8 plane per component, padded to whole MCUs."""
    coeffs = np.asarray(coeffs, np.int16).reshape(-1)
    qtables = np.asarray(qtables, np.uint16).reshape(info.components, 64)
    planes, at = [], 0
    with np.errstate(over="ignore"):
        for comp, (rows, cols) in enumerate(info.plane_blocks):
            blk = _i32(coeffs[at:at + rows * cols * 64]).reshape(rows * cols, 8, 8) * _i32(qtables[comp]).reshape(1, 8, 8)
            at += rows * cols * 64
            ws = _idct_pass(np.moveaxis(blk, 1, 0), 11)                    # columns: the 8-point pass runs down the rows' index
            out = _idct_pass(np.moveaxis(ws, 2, 0), 18)                    # rows: out[k, r, block]
            pix = np.clip(out + np.int32(128), 0, 255).astype(np.uint8)
            pix = np.transpose(pix, (2, 1, 0)).reshape(rows, cols, 8, 8)   # [block, r, k]
            planes.append(np.transpose(pix, (0, 2, 1, 3)).reshape(rows * 8, cols * 8))
    return planes


def _fancy_h(s, bias_even, bias_odd, shift, edge_scale):
    """libjpeg's triangle filter along the last axis of the int32 array ``s`` (true down-sampled width > 2): output 2i mixes
    3 : 1 with column i - 1, output 2i + 1 with column i + 1; the first and the last output take their own column alone."""
    left = np.concatenate([s[..., :1], s[..., :-1]], axis=-1)
    right = np.concatenate([s[..., 1:], s[..., -1:]], axis=-1)
    even = (3 * s + left + bias_even) >> shift
    odd = (3 * s + right + bias_odd) >> shift
    even[..., 0] = (s[..., 0] * edge_scale + (bias_even if edge_scale > 1 else 0)) >> (shift if edge_scale > 1 else 0)
    odd[..., -1] = (s[..., -1] * edge_scale + (bias_odd if edge_scale > 1 else 0)) >> (shift if edge_scale > 1 else 0)
    out = np.empty(s.shape[:-1] + (2 * s.shape[-1],), np.int32)
    out[..., 0::2], out[..., 1::2] = even, odd
    return out


def _upsample(plane, info: JpegInfo):
    """A chroma plane at luma resolution (height x width), by libjpeg's rules on the component's true down-sampled size."""
    h, w = info.height, info.width
    if info.luma_h == 1:
        return plane[:h, :w]
    dw = (w + 1) // 2
    dh = (h + 1) // 2 if info.luma_v == 2 else h
    p = _i32(plane[:dh, :dw])
    if dw <= 2:                                                            # so narrow a plane libjpeg up-samples by replication
        up = np.repeat(p, 2, axis=1)
        if info.luma_v == 2:
            up = np.repeat(up, 2, axis=0)
        return up[:h, :w].astype(np.uint8)
    if info.luma_v == 1:
        return _fancy_h(p, 1, 2, 2, 1)[:h, :w].astype(np.uint8)
    above = np.concatenate([p[:1], p[:-1]], axis=0)                        # the row above the first is the first, below the last the last
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    sums = np.empty((2 * dh, dw), np.int32)
    sums[0::2], sums[1::2] = 3 * p + above, 3 * p + below
    return _fancy_h(sums, 8, 7, 4, 4)[:h, :w].astype(np.uint8)


def reconstruct(coeffs, qtables, info: JpegInfo, channel_order: str = "bgr") -> np.ndarray:
    """Coefficients of one image -> ``(h, w, 3)`` uint8 in BGR or RGB order, or ``(h, w)`` for ``"gray"`` (1-component streams
    only; a 1-component stream asked for in colour is replicated into the three channels)."""
    if channel_order not in ORDERS:
        raise ValueError(f"channel_order must be one of {sorted(ORDERS)}")
    planes = _planes(coeffs, qtables, info)
    h, w = info.height, info.width
    luma = planes[0][:h, :w]
    if info.components == 1:
        return luma.copy() if channel_order == "gray" else np.repeat(luma[:, :, None], 3, axis=2)
    if channel_order == "gray":
        raise ValueError("gray output is for 1-component streams only")
    y = _i32(luma)
    cb = _i32(_upsample(planes[1], info)) - 128
    cr = _i32(_upsample(planes[2], info)) - 128
    red = y + ((91881 * cr + 32768) >> 16)
    green = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    blue = y + ((116130 * cb + 32768) >> 16)
    chans = (blue, green, red) if channel_order == "bgr" else (red, green, blue)
    return np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8)


def decode(blob, channel_order: str = "bgr") -> np.ndarray:
    """Host-only decode of one stream: ``entropy_decode`` + ``reconstruct`` (the checker's path; the product path is
    ``HipEngine.jpeg_decode``)."""
    coeffs, qtables, info = entropy_decode(blob)
    return reconstruct(coeffs, qtables, info, channel_order)


# ---- EXIF orientation: the numpy form of jpeg_colour_oriented_kernel's store -------------------------------------------------
# ``orientation="exif"`` on the JPEG entries applies tag 0x0112 as ``PIL.ImageOps.exif_transpose`` does (the fixture's reference) and,
# as read in OpenCV's source but not run here, as the ExifTransform behind ``cv2.imdecode`` / ``cv2.imread`` with their default
# flags does.  With the source ``(H, W)``, ``out[y, x]`` is
#     1: src[y, x]         2: src[y, W-1-x]       3: src[H-1-y, W-1-x]     4: src[H-1-y, x]           -- out is H x W
#     5: src[x, y]         6: src[H-1-x, y]       7: src[H-1-x, W-1-y]     8: src[x, W-1-y]           -- out is W x H
# 6 is the quarter turn clockwise (a phone held upright), 8 counter-clockwise.  The default everywhere is "ignore".
ORIENTATIONS = ("ignore", "exif")


def check_orientation(orientation) -> bool:
    """True for ``"exif"``, False for ``"ignore"``; any other value raises ``ValueError``."""
    if not isinstance(orientation, str) or orientation not in ORIENTATIONS:
        raise ValueError(f"orientation must be one of {ORIENTATIONS}, got {orientation!r}")
    return orientation == "exif"


def check_tag(tag) -> int:
    """An integer orientation tag 0..8 (0: absent) as an int; anything else raises ``ValueError``."""
    if isinstance(tag, bool) or not isinstance(tag, (int, np.integer)) or not 0 <= int(tag) <= 8:
        raise ValueError(f"an orientation tag is an int 0..8, got {tag!r}")
    return int(tag)


def effective_tag(info: JpegInfo, orientation: str) -> int:
    """The tag a launch applies to this stream: 0 under ``"ignore"`` and for tags 0 (absent) and 1, which change nothing; else 2..8."""
    return info.orientation if check_orientation(orientation) and info.orientation >= 2 else 0


def job_key(info: JpegInfo, orientation: str) -> tuple:
    """What the streams of one launch share: ``(geometry, effective tag)``.  Under ``"ignore"`` the tag is 0 for every stream, so the
    groups are the geometry's."""
    return (info.geometry, effective_tag(info, orientation))


def apply_orientation(array, tag):
    """``array`` ``(h, w)`` or ``(h, w, c)`` as EXIF orientation ``tag`` turns it (the table above); tags 0 and 1 return it unchanged.
    The definition the kernel is held to: a view, no copy."""
    tag = check_tag(tag)
    a = np.asarray(array)
    if a.ndim not in (2, 3):
        raise ValueError("apply_orientation expects an (h, w) or (h, w, c) array")
    if tag >= 5:                                                           # out[y, x] = src[x, y], then the mirrors in OUTPUT axes
        a = np.swapaxes(a, 0, 1)
        rows, cols = tag in (7, 8), tag in (6, 7)                          # 8: src[x, W-1-y]; 6: src[H-1-x, y]; 7: both
    else:
        rows, cols = tag in (3, 4), tag in (2, 3)
    if rows:
        a = a[::-1]
    if cols:
        a = a[:, ::-1]
    return a


def oriented_shape(info: JpegInfo, tag) -> tuple[int, int]:
    """``(height, width)`` of the stream's picture after ``apply_orientation(..., tag)``."""
    return (info.width, info.height) if check_tag(tag) >= 5 else (info.height, info.width)


# ---- JPEG encode: the numpy host form of csrc/jpeg_enc.hip -----------------------------------------------------------------
# What libjpeg writes for a one-component image with its defaults (``PIL.Image.fromarray(a, "L").save(f, "JPEG", quality=q)``):
# baseline, the Annex K luminance table scaled by jpeg_set_quality(q, force_baseline), the "islow" integer forward DCT, the Annex K
# DC0 / AC0 Huffman tables, a JFIF 1.1 header.  The tables below are those of ITU-T T.81 Annex K.
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
LUMA_QUANT = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                       87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                       72, 92, 95, 98, 112, 100, 103, 99])
DC_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC_VALS = tuple(range(12))
AC_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d)
AC_VALS = (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
           0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
           0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
           0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
           0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
           0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
           0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
           0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)
GRAY_HEADER_BYTES = 328


def encode_quant_table(quality: int) -> np.ndarray:
    """``jpeg_set_quality(quality, force_baseline=TRUE)`` on the Annex K luminance table: (64,) int64 in natural order."""
    q = min(100, max(1, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((LUMA_QUANT.astype(np.int64) * scale + 50) // 100, 1, 255)


def _huffman_codes(bits, vals):
    """Annex C: ``{symbol: (code, length)}`` of a table given as its sixteen counts and its symbols."""
    out, code, at = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[at]] = (code, length)
            code, at = code + 1, at + 1
        code <<= 1
    return out


def gray_header(width: int, height: int, quality: int) -> bytes:
    """The 328 bytes in front of the entropy-coded segment: SOI, APP0 (JFIF 1.1, no units, density 1 x 1), DQT, SOF0, DHT DC0, DHT AC0,
    SOS."""
    qt = encode_quant_table(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += b"\xff\xdb\x00\x43\x00" + bytes(int(qt[k]) for k in ZIGZAG)
    out += b"\xff\xc0\x00\x0b\x08" + int(height).to_bytes(2, "big") + int(width).to_bytes(2, "big") + b"\x01\x01\x11\x00"
    out += b"\xff\xc4\x00\x1f\x00" + bytes(DC_BITS) + bytes(DC_VALS)
    out += b"\xff\xc4\x00\xb5\x10" + bytes(AC_BITS) + bytes(AC_VALS)
    out += b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    assert len(out) == GRAY_HEADER_BYTES
    return bytes(out)


def _fdct_pass(d, first):
    """jfdctint.c's 8-point pass along axis 0 of an int64 array (8, ...): the row pass (``first``) leaves two extra bits, the column
    pass takes them out again together with the three of the 8 x 8 scaling it keeps."""
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    shift = 11 if first else 15
    desc = lambda x, n: (x + (1 << (n - 1))) >> n                          # noqa: E731
    o0 = (tmp10 + tmp11) << 2 if first else desc(tmp10 + tmp11, 2)
    o4 = (tmp10 - tmp11) << 2 if first else desc(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * 4433
    o2, o6 = desc(z1 + tmp13 * 6270, shift), desc(z1 - tmp12 * 15137, shift)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o7, o5, o3, o1 = desc(tmp4 + z1 + z3, shift), desc(tmp5 + z2 + z4, shift), desc(tmp6 + z2 + z3, shift), desc(tmp7 + z1 + z4, shift)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7])


def encode_coefficients(image, quality: int = 95) -> np.ndarray:
    """(h, w) uint8 -> (blocks, 64) int64 quantised coefficients in zigzag order, blocks in raster order: edge replication to whole
    blocks, level shift, the islow forward DCT, division with rounding by ``q << 3``."""
    a = np.ascontiguousarray(image, dtype=np.uint8)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("encode_gray expects a non-empty (h, w) uint8 image")
    h, w = a.shape
    rows, cols = (h + 7) // 8, (w + 7) // 8
    a = np.pad(a, ((0, rows * 8 - h), (0, cols * 8 - w)), mode="edge").astype(np.int64) - 128
    blk = a.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3).reshape(rows * cols, 8, 8)            # [block, row, col]
    ws = _fdct_pass(np.moveaxis(blk, 2, 0), True)                                                 # rows: ws[u, block, row]
    out = _fdct_pass(np.moveaxis(ws, 2, 0), False)                                                # columns: out[v, u, block]
    nat = np.transpose(out, (2, 0, 1)).reshape(rows * cols, 64)
    d = encode_quant_table(quality) << 3
    mag = (np.abs(nat) + (d >> 1)) // d
    return np.where(nat < 0, -mag, mag)[:, ZIGZAG]


def _code_arrays(bits_vals_dc, bits_vals_ac):
    """(dc_code, dc_len, ac_code, ac_len) arrays of one DC / AC table pair; absent AC symbols have length 0."""
    dc, ac = _huffman_codes(*bits_vals_dc), _huffman_codes(*bits_vals_ac)
    dc_code, dc_len = np.array([dc[s][0] for s in range(12)], np.uint64), np.array([dc[s][1] for s in range(12)], np.int64)
    ac_code, ac_len = np.zeros(256, np.uint64), np.zeros(256, np.int64)
    for sym, (code, length) in ac.items():
        ac_code[sym], ac_len[sym] = code, length
    return dc_code, dc_len, ac_code, ac_len


def _entropy_segment(zz, diff, sel, tables) -> bytes:
    """The entropy-coded segment of blocks ``zz`` (nb, 64) in coded order: block b has DC difference ``diff[b]`` and uses the table
    set ``tables[sel[b]]`` (``_code_arrays``).  Bits most significant first, the last byte filled with 1-bits, FF followed by 00."""
    nb = zz.shape[0]
    dc_code, dc_len = np.stack([t[0] for t in tables]), np.stack([t[1] for t in tables])
    ac_code, ac_len = np.stack([t[2] for t in tables]), np.stack([t[3] for t in tables])

    def size_and_extra(v):                                                  # category and the bits that follow its code
        mag = np.abs(v)
        size = np.where(mag > 0, np.floor(np.log2(np.maximum(mag, 1))).astype(np.int64) + 1, 0)
        extra = np.where(v < 0, v - 1, v) & ((1 << size) - 1)
        return size, extra.astype(np.uint64)

    # one item per block for the DC difference, one per non-zero AC coefficient (its ZRLs in front), one per end-of-block
    s, e = size_and_extra(diff)
    items = [(np.arange(nb) * 65, (dc_code[sel, s] << s.astype(np.uint64)) | e, dc_len[sel, s] + s)]
    pos = np.where(zz != 0, np.arange(64), -1)
    pos[:, 0] = 0
    prev = np.maximum.accumulate(pos, axis=1)
    b, k = np.nonzero(zz[:, 1:])
    k = k + 1
    run = k - 1 - prev[b, k - 1]
    s, e = size_and_extra(zz[b, k])
    sym = ((run & 15) << 4) | s
    zrl = run >> 4
    t = sel[b]
    val = (ac_code[t, sym] << s.astype(np.uint64)) | e
    length = ac_len[t, sym] + s
    zc, zl = ac_code[t, 0xF0], ac_len[t, 0xF0]
    for r in (1, 2, 3):
        pre = np.zeros(b.size, np.uint64)
        for _ in range(r):
            pre = (pre << zl.astype(np.uint64)) | zc
        val = np.where(zrl == r, (pre << length.astype(np.uint64)) | val, val)
    length = length + zrl * zl
    items.append((b * 65 + k, val, length))
    eob = np.nonzero(zz[:, 63] == 0)[0]
    items.append((eob * 65 + 64, ac_code[sel[eob], 0], ac_len[sel[eob], 0]))
    key = np.concatenate([i[0] for i in items])
    order = np.argsort(key, kind="stable")
    val, length = np.concatenate([i[1] for i in items])[order], np.concatenate([i[2] for i in items])[order]
    start = np.cumsum(length) - length
    total = int(length.sum())
    bits = np.ones((total + 7) // 8 * 8, np.uint8)                          # the last byte is filled with 1-bits
    for j in range(int(length.max())):
        m = length > j
        bits[start[m] + j] = ((val[m] >> (length[m] - 1 - j).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    payload = np.packbits(bits)
    ff = np.nonzero(payload == 0xFF)[0]
    payload = np.insert(payload, ff + 1, 0)                                 # FF is followed by a stuffed 00
    return payload.tobytes()


def encode_gray(image, quality: int = 95) -> bytes:
    """One gray image (h, w) uint8 -> the complete baseline JPEG file libjpeg writes for it at ``quality`` (clamped to 1..100), byte
    for byte ``PIL.Image.fromarray(image, "L").save(f, "JPEG", quality=quality)``.  The numpy form of ``HipEngine.jpeg_encode_gray``
    and its checker; it shares no code with the kernels."""
    zz = encode_coefficients(image, quality)
    h, w = np.asarray(image).shape
    diff = zz[:, 0] - np.concatenate([[0], zz[:-1, 0]])
    tables = [_code_arrays((DC_BITS, DC_VALS), (AC_BITS, AC_VALS))]
    return gray_header(w, h, quality) + _entropy_segment(zz, diff, np.zeros(zz.shape[0], np.int64), tables) + b"\xff\xd9"


# ---- JPEG encode, colour: the numpy host form of the colour front end of csrc/jpeg_enc.hip -------------------------------------
# What libjpeg writes for an RGB image with its defaults (``PIL.Image.fromarray(rgb).save(f, "JPEG", quality=q, subsampling=s)``):
# three components, YCbCr by jccolor.c's 16-bit fixed point, chroma reduced by jcsample.c's plain box (no smoothing), one
# interleaved scan, luma with table set 0 and chroma with set 1 (Annex K.2 quantiser, K.3.3.2 / K.3.3.4 codes), a 623-byte header.
CHROMA_QUANT = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                         99, 99, 99, 99] + [99] * 32)
DC1_BITS = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
DC1_VALS = tuple(range(12))
AC1_BITS = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)
AC1_VALS = (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
            0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
            0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
            0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
            0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
            0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
            0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
            0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)
COLOUR_HEADER_BYTES = 623
SUBSAMPLINGS = {"4:2:0": (2, 2), "4:2:2": (2, 1), "4:4:4": (1, 1)}          # luma sampling (horizontal, vertical); chroma is 1 x 1
ENCODE_MAX_SIDE = 4096


def check_subsampling(subsampling) -> tuple[int, int]:
    """Luma's ``(horizontal, vertical)`` sampling factors of ``"4:2:0"`` / ``"4:2:2"`` / ``"4:4:4"``; anything else raises."""
    if not isinstance(subsampling, str) or subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLINGS)}, got {subsampling!r}")
    return SUBSAMPLINGS[subsampling]


def check_colour_image(image, what: str = "encode_colour") -> np.ndarray:
    """``image`` as an ``(h, w, 3)`` uint8 array, h and w 1..4096; anything else raises ``ValueError``."""
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{what} expects (h, w, 3) uint8 arrays, got {a.dtype} {a.shape}")
    if not (1 <= a.shape[0] <= ENCODE_MAX_SIDE and 1 <= a.shape[1] <= ENCODE_MAX_SIDE):
        raise ValueError(f"{what}: height and width must be 1..{ENCODE_MAX_SIDE}, got {a.shape[0]} x {a.shape[1]}")
    return a


def check_colour_order(channel_order) -> bool:
    """True when byte 0 of a pixel is R (``"rgb"``), False for ``"bgr"``; anything else raises."""
    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    return channel_order == "rgb"


def encode_chroma_quant_table(quality: int) -> np.ndarray:
    """``encode_quant_table``'s scaling on the Annex K.2 chrominance table."""
    q = min(100, max(1, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((CHROMA_QUANT.astype(np.int64) * scale + 50) // 100, 1, 255)


def colour_header(width: int, height: int, quality: int, subsampling: str = "4:2:0") -> bytes:
    """The 623 bytes in front of the entropy-coded segment: SOI, APP0, DQT 0, DQT 1, SOF0 (three components), DHT DC0, AC0, DC1, AC1,
    SOS."""
    hs, vs = check_subsampling(subsampling)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for k, qt in enumerate((encode_quant_table(quality), encode_chroma_quant_table(quality))):
        out += b"\xff\xdb\x00\x43" + bytes([k]) + bytes(int(qt[z]) for z in ZIGZAG)
    out += b"\xff\xc0\x00\x11\x08" + int(height).to_bytes(2, "big") + int(width).to_bytes(2, "big") + b"\x03"
    out += bytes([1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    out += b"\xff\xc4\x00\x1f\x00" + bytes(DC_BITS) + bytes(DC_VALS)
    out += b"\xff\xc4\x00\xb5\x10" + bytes(AC_BITS) + bytes(AC_VALS)
    out += b"\xff\xc4\x00\x1f\x01" + bytes(DC1_BITS) + bytes(DC1_VALS)
    out += b"\xff\xc4\x00\xb5\x11" + bytes(AC1_BITS) + bytes(AC1_VALS)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == COLOUR_HEADER_BYTES
    return bytes(out)


def colour_planes(image, subsampling: str = "4:2:0", channel_order: str = "bgr"):
    """``(Y, Cb, Cr)`` int64 planes as the forward DCT sees them, before the level shift: Y padded to whole MCUs by replicating its
    last column and row; chroma converted at full resolution, its last column replicated out to the MCU width, its last row only to
    a whole row group, then reduced by the box filter, then its last REDUCED row replicated down to whole blocks."""
    a = check_colour_image(image).astype(np.int64)
    hs, vs = check_subsampling(subsampling)
    r, g, b = (a[..., 0], a[..., 1], a[..., 2]) if check_colour_order(channel_order) else (a[..., 2], a[..., 1], a[..., 0])
    h, w = r.shape
    mh, mw = -(-h // (8 * vs)) * 8 * vs, -(-w // (8 * hs)) * 8 * hs
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    planes = [np.pad(y, ((0, mh - h), (0, mw - w)), mode="edge")]
    for c in (cb, cr):
        c = np.pad(c, ((0, -(-h // vs) * vs - h), (0, mw - w)), mode="edge")
        if hs == 2:
            pairs = c[:, 0::2] + c[:, 1::2]
            odd = np.arange(pairs.shape[1]) & 1
            c = (pairs[0::2] + pairs[1::2] + 1 + odd) >> 2 if vs == 2 else (pairs + odd) >> 1
        planes.append(np.pad(c, ((0, mh // vs - c.shape[0]), (0, 0)), mode="edge"))
    return tuple(planes)


def _plane_coefficients(plane, table) -> np.ndarray:
    """A padded int64 plane -> (block_rows, block_cols, 64) quantised coefficients in zigzag order (``encode_coefficients``'s steps)."""
    rows, cols = plane.shape[0] // 8, plane.shape[1] // 8
    blk = (plane - 128).reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3).reshape(rows * cols, 8, 8)
    ws = _fdct_pass(np.moveaxis(blk, 2, 0), True)
    out = _fdct_pass(np.moveaxis(ws, 2, 0), False)
    nat = np.transpose(out, (2, 0, 1)).reshape(rows * cols, 64)
    d = table << 3
    mag = (np.abs(nat) + (d >> 1)) // d
    return np.where(nat < 0, -mag, mag)[:, ZIGZAG].reshape(rows, cols, 64)


def encode_colour_coefficients(image, quality: int = 95, subsampling: str = "4:2:0", channel_order: str = "bgr"):
    """``(zz, comp, real)``: the quantised blocks of the scan in CODED order, ``(blocks, 64)`` int64 in zigzag order, MCU by MCU
    (luma blocks row-major, then Cb, then Cr); ``comp`` (blocks,) is each block's component 0 / 1 / 2 and ``real`` (blocks,) is False
    for the dummy luma blocks: those of an MCU that lie beyond the component's own ceil(h / 8) x ceil(w / 8) blocks.  A dummy holds the
    DC of the block coded before it in its component and no AC."""
    hs, vs = check_subsampling(subsampling)
    yp, cbp, crp = colour_planes(image, subsampling, channel_order)
    h, w = np.asarray(image).shape[:2]
    my, mx = yp.shape[0] // (8 * vs), yp.shape[1] // (8 * hs)
    yz = _plane_coefficients(yp, encode_quant_table(quality))
    cq = encode_chroma_quant_table(quality)
    cbz, crz = _plane_coefficients(cbp, cq), _plane_coefficients(crp, cq)
    per = hs * vs + 2
    zz = np.zeros((my, mx, per, 64), np.int64)
    real = np.ones((my, mx, per), bool)
    for v in range(vs):
        for u in range(hs):
            k = v * hs + u
            zz[:, :, k] = yz[v::vs, u::hs]
            by, bx = np.arange(my) * vs + v, np.arange(mx) * hs + u
            real[:, :, k] = (by < -(-h // 8))[:, None] & (bx < -(-w // 8))[None, :]
            if k:                                                           # block 0 of an MCU is always real
                dummy = ~real[:, :, k]
                zz[:, :, k][dummy] = 0
                zz[:, :, k, 0][dummy] = zz[:, :, k - 1, 0][dummy]
    zz[:, :, per - 2], zz[:, :, per - 1] = cbz, crz
    comp = np.tile(np.array([0] * (hs * vs) + [1, 2]), my * mx)
    return zz.reshape(-1, 64), comp, real.reshape(-1)


def encode_colour(image, quality: int = 95, subsampling: str = "4:2:0", channel_order: str = "bgr") -> bytes:
    """One colour image (h, w, 3) uint8, BGR by default -> the complete baseline JPEG file libjpeg writes for it at ``quality``
    (clamped to 1..100): byte for byte ``PIL.Image.fromarray(rgb).save(f, "JPEG", quality=quality, subsampling=subsampling)``.
    ``channel_order`` only says which byte of a pixel is R.  The numpy form of ``HipEngine.jpeg_encode_colour`` and its checker; it
    shares no code with the kernels."""
    zz, comp, _ = encode_colour_coefficients(image, quality, subsampling, channel_order)
    h, w = np.asarray(image).shape[:2]
    diff = np.zeros(zz.shape[0], np.int64)
    for c in range(3):                                                      # DC prediction runs per component, from 0
        dcs = zz[comp == c, 0]
        diff[comp == c] = dcs - np.concatenate([[0], dcs[:-1]])
    tables = [_code_arrays((DC_BITS, DC_VALS), (AC_BITS, AC_VALS)), _code_arrays((DC1_BITS, DC1_VALS), (AC1_BITS, AC1_VALS))]
    return colour_header(w, h, quality, subsampling) + _entropy_segment(zz, diff, np.minimum(comp, 1), tables) + b"\xff\xd9"

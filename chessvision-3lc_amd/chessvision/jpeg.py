"""JPEG decode: the host half (ctypes over ``csrc/jpeg.cpp``) and the numpy host form of the device half.

``jpeg_info`` and ``entropy_decode`` call the library's host-only entry points (no engine, no GPU): the marker parser and the
Huffman stage, which turn a baseline JPEG stream into quantised coefficients.  ``reconstruct`` restates, in vectorised integer
numpy, what ``csrc/jpeg.hip`` does with those coefficients on the device: dequantise, libjpeg's "islow" integer inverse DCT, its
fancy chroma up-sampling and its fixed-point YCbCr -> RGB conversion.  As everywhere in this package the numpy form is the readable
checker: it shares no code with the kernel, and both are held to the bytes libjpeg itself produces (Pillow and ``cv2.imdecode``
decode with libjpeg's defaults).  All arithmetic wraps in 32 bits, so the two forms agree on any coefficients.
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
    orientation: int          # EXIF tag 0x0112 as found (1..8), 0 when absent: reported, never applied
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

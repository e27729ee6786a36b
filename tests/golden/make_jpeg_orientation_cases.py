#!/usr/bin/env python3
"""Write the fixture of the EXIF orientation tests (Pillow only):

    python tests/golden/make_jpeg_orientation_cases.py

jpeg_orientation_cases.npz -- noise pictures WRITTEN by Pillow (libjpeg-turbo) with an EXIF orientation tag, and for each
``np.asarray(ImageOps.exif_transpose(Image.open(blob)))``: Pillow's decode, which the decoder matches byte for byte, turned by Pillow's
own transpose.

    names            (N,) str     "<sampling>_<h>x<w>_t<tag>" (+ "_II" for the hand-built little-endian blocks), in order
    sampling         (N,) str     "420" | "422" | "444" | "gray"
    tag              (N,) int     the EXIF orientation the stream carries, 0: no EXIF at all
    blobs            uint8        every stream, one after the other; stream k is blobs[blob_at[k] : blob_at[k + 1]]
    blob_at          (N + 1,) int
    pixels           uint8        every upright picture likewise: picture k is pixels[pixel_at[k] : pixel_at[k + 1]] in the shape
    pixel_at         (N + 1,) int shape[k] = (h', w', 3) RGB, or (h', w', 0) -- that is (h', w') -- for the 1-component streams
    shape            (N, 3) int
    pillow_version, libjpeg_turbo_version   str

  (Two flat arrays instead of one entry per case: the nine streams of a picture share their scan and its turned pictures share their
  rows, which the compressor only sees inside one entry.  tests/jpeg_orientation_cases.py reads the file.)

  sizes (h, w): 1x1, 1x17, 17x1, 3x5, 15x33, 33x15, 16x16, and two chosen from the oriented colour kernel's 32 x 32 tile (TILE below,
  kTile in csrc/jpeg.hip): 32x33 (a whole tile one way, one pixel into the next tile the other) and 67x31 (two tiles and three pixels
  by one short tile).  Every size with every sampling and every tag 0..8.  One picture per (sampling, size): the nine tags wrap the
  same scan, so a tag's result is the plain decode turned and nothing else.
  Pillow writes big-endian ("MM") TIFF headers; for tags 6 and 8 every (sampling, 15x33) picture is also given a little-endian ("II")
  EXIF block built by hand below.
"""
from __future__ import annotations

import io
from pathlib import Path

import numpy as np
import PIL
from PIL import Image, ImageOps, features

HERE = Path(__file__).resolve().parent
TILE = 32
SIZES = [(1, 1), (1, 17), (17, 1), (3, 5), (15, 33), (33, 15), (16, 16), (TILE, TILE + 1), (2 * TILE + 3, TILE - 1)]
SAMPLINGS = ("420", "422", "444", "gray")
QUALITY = 60                      # noise at a moderate quality: every coefficient position live, streams of a few hundred bytes


def encode(arr, sampling, exif=None):
    im = Image.fromarray(arr, "RGB")
    kw = {"quality": QUALITY}
    if sampling == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = {"420": "4:2:0", "422": "4:2:2", "444": "4:4:4"}[sampling]
    if exif is not None:
        kw["exif"] = exif
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def little_endian_exif(tag: int) -> bytes:
    """An APP1 payload with a little-endian TIFF header and one IFD0 entry: Orientation (0x0112), SHORT, count 1."""
    tiff = b"II" + (42).to_bytes(2, "little") + (8).to_bytes(4, "little")
    ifd = (1).to_bytes(2, "little") + (0x0112).to_bytes(2, "little") + (3).to_bytes(2, "little") + (1).to_bytes(4, "little") \
        + int(tag).to_bytes(2, "little") + b"\x00\x00" + (0).to_bytes(4, "little")
    return b"Exif\x00\x00" + tiff + ifd


def upright(blob: bytes):
    return np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(blob))))


def main():
    rng = np.random.default_rng(20261)
    names, samplings, tags, blobs, pictures = [], [], [], [], []

    def add(name, sampling, tag, blob):
        names.append(name); samplings.append(sampling); tags.append(tag)
        blobs.append(np.frombuffer(blob, np.uint8))
        pictures.append(upright(blob))

    for sampling in SAMPLINGS:
        for h, w in SIZES:
            arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            for tag in range(9):
                exif = None
                if tag:
                    exif = Image.Exif()
                    exif[0x0112] = tag
                add(f"{sampling}_{h}x{w}_t{tag}", sampling, tag, encode(arr, sampling, exif))
            if (h, w) == (15, 33):
                for tag in (6, 8):
                    add(f"{sampling}_{h}x{w}_t{tag}_II", sampling, tag, encode(arr, sampling, little_endian_exif(tag)))

    out = HERE / "jpeg_orientation_cases.npz"
    np.savez_compressed(out, names=np.array(names), sampling=np.array(samplings), tag=np.array(tags, np.int32),
                        blobs=np.concatenate(blobs), blob_at=np.cumsum([0] + [b.size for b in blobs]).astype(np.int32),
                        pixels=np.concatenate([p.reshape(-1) for p in pictures]),
                        pixel_at=np.cumsum([0] + [p.size for p in pictures]).astype(np.int32),
                        shape=np.array([p.shape if p.ndim == 3 else p.shape + (0,) for p in pictures], np.int32),
                        pillow_version=np.array(PIL.__version__), libjpeg_turbo_version=np.array(str(features.version("libjpeg_turbo"))))
    print(out.name + ":", len(names), "cases,", out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()

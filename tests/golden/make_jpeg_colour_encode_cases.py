#!/usr/bin/env python3
"""Write tests/golden/jpeg_colour_encode_cases.npz: colour images and the files Pillow (libjpeg-turbo) writes for them.

    python tests/golden/make_jpeg_colour_encode_cases.py

Inputs are made by tests/jpeg_colour_encode_cases.py (seeded generators, one crop of a committed photo, six streams of the decoder's
committed cases); every output is ``PIL.Image.fromarray(rgb).save(f, "JPEG", quality=q, subsampling=s)``, nothing of this package.  A
transcoded stream is ``ImageOps.exif_transpose(Image.open(blob)).convert("RGB")`` saved the same way.  The full 512 x 512 photo is
recorded by length and SHA-256 only.  Asserts (with this package's numpy form, which writes nothing) that the cases hold a stuffed
FF 00, a ZRL in a chroma block and a dummy block behind a block with a non-zero DC, and that the file stays under 700 KB.

    image/<h>x<w>/<kind>   (h, w, 3) uint8, BGR          files, file_at   all files back to back (three per group in the order of
    photo_length, photo_sha256, pillow                                    cases.group_list(), the cropped photo's, six transcodes)
"""
from __future__ import annotations

import hashlib
import io
import sys
from pathlib import Path

import numpy as np
import PIL
from PIL import Image, ImageOps

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent / "chessvision-3lc_amd"))

import jpeg_colour_encode_cases as cases  # noqa: E402


def pillow(rgb, q, sub):
    buf = io.BytesIO()
    (rgb if isinstance(rgb, Image.Image) else Image.fromarray(np.ascontiguousarray(rgb))).save(buf, "JPEG", quality=q, subsampling=sub)
    return buf.getvalue()


def findings(a, q, sub, order):
    """(a chroma block has a ZRL, a dummy block follows a block with a non-zero DC) by the numpy form's coefficients."""
    from chessvision import jpeg

    zz, comp, real = jpeg.encode_colour_coefficients(a, q, sub, order)
    pos = np.where(zz != 0, np.arange(64), -1)
    pos[:, 0] = 0
    prev = np.maximum.accumulate(pos, axis=1)
    b, k = np.nonzero(zz[:, 1:])
    zrl = (k + 1 - 1 - prev[b, k] >= 16) & (comp[b] > 0)
    dummy = np.nonzero(~real)[0]
    return bool(zrl.any()), bool(np.any(zz[dummy - 1, 0] != 0))


def main():
    out, files, stuffed, zrl, dummy = {}, [], 0, 0, 0
    for gi, (h, w) in enumerate(cases.GEOMETRIES):
        for kind in cases.KINDS:
            out[f"image/{h}x{w}/{kind}"] = cases.make_image(kind, h, w, cases.image_seed(gi, kind))
    for name, (h, w), sub, q, order, kinds in cases.group_list():
        for kind in kinds:
            a = out[f"image/{h}x{w}/{kind}"]
            files.append(pillow(a if order == "rgb" else a[..., ::-1], q, sub))
            stuffed += files[-1][623:-2].count(b"\xff\x00")
            z, d = findings(a, q, sub, order)
            zrl, dummy = zrl + z, dummy + d
    files.append(pillow(cases.photo_crop()[..., ::-1], cases.PHOTO_QUALITY, cases.PHOTO_SUBSAMPLING))
    for blob, (_, _, q, sub) in zip(cases.transcode_blobs(), cases.TRANSCODES):
        files.append(pillow(ImageOps.exif_transpose(Image.open(io.BytesIO(blob))).convert("RGB"), q, sub))
    whole = pillow(cases.photo()[..., ::-1], cases.PHOTO_QUALITY, cases.PHOTO_SUBSAMPLING)
    out["files"] = np.frombuffer(b"".join(files), np.uint8)
    out["file_at"] = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
    out["photo_length"] = np.int64(len(whole))
    out["photo_sha256"] = np.frombuffer(hashlib.sha256(whole).digest(), np.uint8)
    out["pillow"] = np.array(PIL.__version__)
    assert stuffed >= 1 and zrl >= 1 and dummy >= 1, (stuffed, zrl, dummy)
    path = HERE / "jpeg_colour_encode_cases.npz"
    np.savez_compressed(path, **out)
    size = path.stat().st_size
    assert size < 700 * 1024, size
    print(f"{path.name}: {size} bytes, {len(files)} files ({3 * len(cases.group_list())} in groups + 1 crop + {len(cases.TRANSCODES)} "
          f"transcodes) + 1 photo hash; {stuffed} stuffed bytes, {zrl} images with a chroma ZRL, {dummy} with a dummy behind a non-zero "
          f"DC; photo {len(whole)} bytes; Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()

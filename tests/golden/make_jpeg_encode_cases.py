#!/usr/bin/env python3
"""Write tests/golden/jpeg_encode_cases.npz: gray images and the files Pillow (libjpeg-turbo) writes for them.

    python tests/golden/make_jpeg_encode_cases.py

Inputs are made by tests/jpeg_encode_cases.py (seeded generators, twelve squares of squares_val.npz, one board warped from a committed
photo); every output is ``PIL.Image.fromarray(a, "L").save(f, "JPEG", quality=q)``, nothing of this package.  The 512 x 512 board is
recorded by length and SHA-256 only.  Asserts that the cases contain a stuffed FF 00 and a block with a ZRL, and that the file stays
under 700 KB.

    image/<h>x<w>/<kind>       (h, w) uint8            file/<h>x<w>/q<q>/<kind>   the file, uint8
    squares (12, 64, 64)       square_file/<i>         board_length, board_sha256, pillow (version string)
"""
from __future__ import annotations

import hashlib
import io
import sys
from pathlib import Path

import numpy as np
import PIL
from PIL import Image

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent / "chessvision-3lc_amd"))

import jpeg_encode_cases as cases  # noqa: E402


def pillow(a, q):
    buf = io.BytesIO()
    Image.fromarray(a, "L").save(buf, "JPEG", quality=q)
    return buf.getvalue()


def has_zrl(a, q):
    from chessvision import jpeg

    zz = jpeg.encode_coefficients(a, q)
    pos = np.where(zz != 0, np.arange(64), -1)
    pos[:, 0] = 0
    prev = np.maximum.accumulate(pos, axis=1)
    b, k = np.nonzero(zz[:, 1:])
    return bool(np.any(k + 1 - 1 - prev[b, k] >= 16))


def main():
    out, stuffed, zrl = {}, 0, 0
    for gi, (h, w) in enumerate(cases.GEOMETRIES):
        kinds = sorted({k for qi in range(len(cases.QUALITIES)) for k in cases.group_kinds(gi, qi)})
        for kind in kinds:
            out[f"image/{h}x{w}/{kind}"] = cases.make_image(kind, h, w, seed=1000 * gi + sum(map(ord, kind)))
        for qi, q in enumerate(cases.QUALITIES):
            for kind in cases.group_kinds(gi, qi):
                a = out[f"image/{h}x{w}/{kind}"]
                blob = pillow(a, q)
                out[f"file/{h}x{w}/q{q}/{kind}"] = np.frombuffer(blob, np.uint8)
                stuffed += blob[328:-2].count(b"\xff\x00")
                zrl += has_zrl(a, q)
    squares = np.load(HERE / "squares_val.npz")["squares"][cases.SQUARES]
    out["squares"] = squares
    for i, a in enumerate(squares):
        out[f"square_file/{i}"] = np.frombuffer(pillow(np.ascontiguousarray(a), 95), np.uint8)
    blob = pillow(cases.board_image(), 95)
    out["board_length"] = np.int64(len(blob))
    out["board_sha256"] = np.frombuffer(hashlib.sha256(blob).digest(), np.uint8)
    out["pillow"] = np.array(PIL.__version__)
    assert stuffed >= 1 and zrl >= 1, (stuffed, zrl)
    path = HERE / "jpeg_encode_cases.npz"
    np.savez_compressed(path, **out)
    size = path.stat().st_size
    assert size < 700 * 1024, size
    print(f"{path.name}: {size} bytes, {sum(k.startswith('file/') for k in out)} files + {len(squares)} squares + 1 board hash; "
          f"{stuffed} stuffed bytes, {zrl} images with a ZRL; board {len(blob)} bytes; Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()

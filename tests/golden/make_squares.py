#!/usr/bin/env python3
"""Commit 130 of the reference's labelled validation squares as DATA.  Run in the build container only (the one place the reference's
data and a JPEG decoder exist):

    python tests/golden/make_squares.py <reference checkout>/data/squares/validation

Source: data/squares/validation of the reference (2 134 squares in 13 class folders, the table scripts/train/train_classifier.py
validates on).  The first 10 files of every class folder by sorted name are decoded with PIL.  The files are already 64 x 64, mode "L",
so the Resize((64, 64)) and Grayscale() of the reference's val_transforms are identities on them and the bytes stored here are what
ToTensor() sees.  Folder names map to label names by dropping the leading underscore ("_b" -> "b"); "f" is the empty class; class
indices follow constants.LABEL_NAMES = "BKNPQRbknpqrf".

    squares_val.npz   squares (130,64,64) uint8 | labels (130,) int8

These are inputs and labels, not outputs of anything.  The statistics printed at the end are asserted by
tests/test_evaluate_squares_cpu.py.
"""
from __future__ import annotations

import sys
import zlib
from pathlib import Path

import numpy as np
from PIL import Image

HERE = Path(__file__).resolve().parent
LABEL_NAMES = list("BKNPQRbknpqr") + ["f"]
PER_CLASS = 10


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = Path(sys.argv[1])
    squares, labels = [], []
    for folder in sorted(p for p in src.iterdir() if p.is_dir()):
        label = folder.name[1:] if folder.name.startswith("_") else folder.name
        files = sorted(p for p in folder.iterdir() if p.is_file())[:PER_CLASS]
        assert len(files) == PER_CLASS, (folder, len(files))
        for path in files:
            img = Image.open(path)
            assert img.mode == "L" and img.size == (64, 64), (path, img.mode, img.size)
            squares.append(np.asarray(img, dtype=np.uint8))
            labels.append(LABEL_NAMES.index(label))
    order = np.argsort(np.asarray(labels), kind="stable")            # class index order, files in sorted order within a class
    sq = np.stack(squares)[order]
    lab = np.asarray(labels, dtype=np.int8)[order]
    assert sq.shape == (13 * PER_CLASS, 64, 64) and sq.dtype == np.uint8
    out = HERE / "squares_val.npz"
    np.savez_compressed(out, squares=sq, labels=lab)
    print(f"{out.name}: {out.stat().st_size} bytes, squares {sq.shape} {sq.dtype}, labels {np.bincount(lab).tolist()}")
    print(f"  sum {int(sq.sum(dtype=np.int64))}  min {int(sq.min())}  max {int(sq.max())}  crc32 {zlib.crc32(sq.tobytes())}")
    print(f"  mean/255 {float(sq.mean() / 255):.6f}  std/255 {float(sq.std() / 255):.6f}")
    print("  per-class byte sums", [int(sq[lab == c].sum(dtype=np.int64)) for c in range(13)])


if __name__ == "__main__":
    main()

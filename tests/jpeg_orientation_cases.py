"""The cases of the EXIF orientation tests (tests/golden/jpeg_orientation_cases.npz, written by
tests/golden/make_jpeg_orientation_cases.py): how the file is read, and the sizes it must hold."""
from __future__ import annotations

import functools
from pathlib import Path
from typing import NamedTuple

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
TILE = 32                                                    # kTile of csrc/jpeg.hip: the square of source pixels one workgroup turns
SIZES = [(1, 1), (1, 17), (17, 1), (3, 5), (15, 33), (33, 15), (16, 16), (TILE, TILE + 1), (2 * TILE + 3, TILE - 1)]      # (h, w)
SAMPLINGS = ("420", "422", "444", "gray")


class Case(NamedTuple):
    name: str
    sampling: str             # "420" | "422" | "444" | "gray"
    tag: int                  # the EXIF orientation the stream carries, 0: none
    blob: bytes
    upright: np.ndarray       # Pillow's decode turned by Pillow: (h', w', 3) RGB, or (h', w') for the 1-component streams

    @property
    def gray(self) -> bool:
        return self.sampling == "gray"


@functools.lru_cache(maxsize=None)
def load() -> tuple:
    z = np.load(GOLDEN / "jpeg_orientation_cases.npz")
    blobs, blob_at, pixels, pixel_at = z["blobs"], z["blob_at"], z["pixels"], z["pixel_at"]
    out = []
    for k, (name, sampling, tag, shape) in enumerate(zip(z["names"], z["sampling"], z["tag"], z["shape"])):
        picture = pixels[pixel_at[k]:pixel_at[k + 1]].reshape([int(v) for v in shape if v])
        picture.setflags(write=False)
        out.append(Case(str(name), str(sampling), int(tag), blobs[blob_at[k]:blob_at[k + 1]].tobytes(), picture))
    return tuple(out)


def by_picture() -> dict:
    """(sampling, (h, w)) -> the cases that wrap that one picture, in tag order (the little-endian extras last)."""
    out: dict = {}
    for case in load():
        h, w = (int(v) for v in case.name.split("_")[1].split("x"))
        out.setdefault((case.sampling, (h, w)), []).append(case)
    return out

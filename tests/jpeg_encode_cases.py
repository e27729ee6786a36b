"""The cases of the gray JPEG encoder's tests (tests/golden/jpeg_encode_cases.npz, written by tests/golden/make_jpeg_encode_cases.py):
how the inputs are made, how the file is read, and the one real board, which is recomputed from a committed photo instead of stored."""
from __future__ import annotations

from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
GEOMETRIES = [(1, 1), (7, 9), (8, 8), (16, 8), (17, 15), (33, 40), (64, 64), (128, 128)]       # (h, w)
QUALITIES = [1, 50, 95, 100]
THIRD = ["step", "const0", "binary", "const255"]        # the third image of a group rotates through these
SQUARES = [0, 11, 22, 33, 44, 55, 66, 77, 88, 99, 110, 121]     # rows of squares_val.npz: one of (nearly) every class
BOARD_QUAD = np.array([[140, 90], [930, 120], [980, 700], [100, 680]], np.float32)   # corners in the photo, clockwise from top left


def make_image(kind: str, h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    if kind == "smooth":
        return np.clip(128 + 90 * np.sin(yy / 9.0 + 0.3) * np.cos(xx / 13.0) + 20 * (xx / max(1, w - 1)), 0, 255).astype(np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    if kind == "const0":
        return np.zeros((h, w), np.uint8)
    if kind == "const255":
        return np.full((h, w), 255, np.uint8)
    if kind == "step":
        return np.where(xx * 2 + yy > w, 255, 0).astype(np.uint8)
    raise ValueError(kind)


def group_kinds(gi: int, qi: int) -> list[str]:
    """The three images that go into ONE launch for geometry gi at quality qi: different content in one batch."""
    return ["noise", "smooth", THIRD[(gi + qi) % 4]]


def board_image() -> np.ndarray:
    """A real 512 x 512 board by the numpy pipeline: the first committed photo, to gray, warped from BOARD_QUAD."""
    from chessvision import classical

    photo = np.ascontiguousarray(np.load(GOLDEN / "photos8_0.npz")["bgr"][0])
    dst = np.array([[0, 0], [511, 0], [511, 511], [0, 511]], np.float32)
    m = classical.get_perspective_transform(BOARD_QUAD, dst)
    return np.ascontiguousarray(classical.warp_perspective(classical.bgr_to_gray(photo), m, (512, 512)))


def load():
    return np.load(GOLDEN / "jpeg_encode_cases.npz")


def groups(z):
    """(name, quality, images (3, h, w), [file bytes] * 3) per launch group, then the twelve real squares as one group."""
    for gi, (h, w) in enumerate(GEOMETRIES):
        for qi, q in enumerate(QUALITIES):
            kinds = group_kinds(gi, qi)
            yield (f"{h}x{w}-q{q}", q, np.stack([z[f"image/{h}x{w}/{k}"] for k in kinds]),
                   [z[f"file/{h}x{w}/q{q}/{k}"].tobytes() for k in kinds])
    yield "squares-q95", 95, z["squares"], [z[f"square_file/{i}"].tobytes() for i in range(len(SQUARES))]

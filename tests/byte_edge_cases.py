"""Shared by tests/test_byte_edge_cases_cpu.py, tests/test_gpu_warp_edges.py and tests/test_gpu_resize_area_edges.py: the edge cases
of the two byte kernels that take the caller's photo as it comes -- the board warp (``extract_squares_u8_kernel`` and its
``CV_WARP=float`` twin) and INTER_AREA (the three ``resize_area`` kernels) -- and their reference chains.

Two references per case, which share no code: the product's host restatement (``chessvision/classical.py``, ``chessvision/utils.py``)
and the independent oracle (``oracle/classical_ref.py``).  The CPU file requires the two to agree on every case (the table is sound
before a GPU sees it); the GPU files require the device to equal both, byte for byte.  There is no tolerance anywhere.

Photos are ``(h, w)``; quadrangles are (x, y) corners in the reference's TR, TL, BL, BR order; every board is 512 x 512."""
from __future__ import annotations

import functools

import numpy as np

from chessvision import classical, utils
from oracle import classical_ref as cref

BOARD = (512, 512)
DEST = np.array(((0, 0), (512, 0), (512, 512), (0, 512)), np.float32)
BANDS = (range(0, 4), range(254, 258), range(508, 512))         # rows the scalar float oracle computes (~15 s for a whole board)


def _frame(h: int, w: int):
    return [[w, 0], [0, 0], [0, h], [w, h]]


_CONVEX = [[45, 4], [6, 3], [4, 30], [48, 33]]
# (id, (h, w) of the photo, quadrangle)
WARP_CASES = [
    ("convex", (37, 53), _CONVEX),
    ("frame", (37, 53), _frame(37, 53)),
    ("frame-minus-one", (37, 53), [[52, 0], [0, 0], [0, 36], [52, 36]]),
    ("beyond-frame", (37, 53), [[62, -7], [-8, -6], [-5, 43], [60, 45]]),                       # zero border on all four sides
    ("self-crossing", (37, 53), [_CONVEX[0], _CONVEX[1], _CONVEX[3], _CONVEX[2]]),
    ("concave", (37, 53), [[45, 4], [6, 3], [30, 12], [48, 33]]),
    ("collinear", (37, 53), [[40, 5], [5, 5], [22.5, 5], [40, 30]]),
    ("two-equal", (37, 53), [[45, 4], [45, 4], [4, 30], [48, 33]]),
    ("four-equal", (37, 53), [[20, 15]] * 4),               # singular: fixed reading reads pixel (0,0) everywhere, float reading the border
    ("far-outside", (37, 53), [[5000, 4000], [4000, 4000], [4000, 5000], [5000, 5000]]),
    ("half-pixel", (37, 53), [[10.5, 10], [10, 10], [10, 10.5], [10.5, 10.5]]),                 # 1000x magnification
    ("9x1", (9, 1), _frame(9, 1)),                          # one pixel wide: no pixel has a right neighbour
    ("9x2", (9, 2), _frame(9, 2)),
    ("1x9", (1, 9), _frame(1, 9)),
    ("1x1", (1, 1), _frame(1, 1)),
    ("2x3-self-crossing", (2, 3), [[3, 0], [0, 0], [3, 2], [0, 2]]),
    ("4x40000", (4, 40000), [[39990, 0], [33000, 0], [33000, 4], [39990, 4]]),                  # int16 saturation of the map in x ...
    ("40000x4", (40000, 4), [[0, 39990], [0, 33000], [4, 33000], [4, 39990]]),                  # ... and, transposed, in y
]
WARP_IDS = [c[0] for c in WARP_CASES]
# every route into the warp kernel must give the same bytes on these
ROUTE_IDS = ["convex", "self-crossing", "9x1", "1x1", "far-outside", "4x40000"]

# ((h, w, c), (oh, ow))
AREA_CASES = [
    ((48, 64, 3), (16, 16)),         # integer factors 3 x 4
    ((64, 64, 3), (16, 16)),         # 4 x 4
    ((32, 48, 1), (16, 16)),         # 2 x 3, one channel
    ((32, 32, 2), (16, 16)),         # 2 x 2, not three channels: no fast path
    ((32, 32, 4), (16, 16)),
    ((32, 40, 3), (16, 10)),         # 2 x 2, three channels, ow % 4 != 0: no fast path
    ((16, 32, 3), (16, 16)),         # 1 x 2
    ((16, 16, 3), (16, 16)),         # identity
    ((37, 53, 1), (16, 24)),         # fractional in both axes, every channel count up to 5
    ((37, 53, 2), (16, 24)),
    ((37, 53, 4), (16, 24)),
    ((37, 53, 5), (16, 24)),         # more channels than one register group of the table kernel
    ((32, 53, 3), (16, 24)),         # integer in y, fractional in x
    ((17, 16, 3), (16, 16)),         # fractional in y, identity in x
    ((1, 1, 3), (4, 4)),             # enlarging a single pixel
    ((1, 7, 3), (3, 3)),             # enlarging in y, shrinking in x
    ((5, 1, 3), (2, 1)),             # one-pixel axis, fractional shrink on the other
    ((3, 3, 3), (1, 1)),
    ((2, 2, 3), (1, 1)),
    ((12, 40, 3), (16, 16)),
    ((12, 32, 3), (24, 16)),
    ((8, 8, 1), (16, 16)),
    ((9, 7, 4), (16, 20)),
]
AREA_BATCH = 3                       # images per geometry: the per-image offset is part of every case
AREA_MISALIGNED = ((32, 32, 3), (16, 16))    # the 2x2c3 geometry from a source 3 bytes into its allocation: the guard picks the generic kernel
AREA_MISALIGNED_OFFSET = 3


def area_id(case) -> str:
    (h, w, c), (oh, ow) = case
    return f"{h}x{w}x{c}-{oh}x{ow}"


def warp_case(case_id: str):
    """(photo (h,w,3) uint8, quadrangle (4,2) float32) of a warp case; the photo's seed is the case's place in the table."""
    k = WARP_IDS.index(case_id)
    _, (h, w), quad = WARP_CASES[k]
    photo = np.random.default_rng(1000 + k).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return photo, np.array(quad, np.float32)


def warp_groups():
    """Case ids by photo shape, in table order: the cases of one shape go to the device in one call."""
    groups: dict[tuple[int, int], list[str]] = {}
    for case_id, shape, _ in WARP_CASES:
        groups.setdefault(shape, []).append(case_id)
    return groups


def gray_flip_host(board_bgr: np.ndarray) -> np.ndarray:
    return classical.flip_horizontal(classical.bgr_to_gray(board_bgr))


def gray_flip_oracle(board_bgr: np.ndarray) -> np.ndarray:
    return cref.flip_lr(cref.bgr_to_gray(board_bgr))


@functools.lru_cache(maxsize=None)
def host_board_bgr(case_id: str) -> np.ndarray:
    """Fixed reading, host restatement: ``utils.extract_perspective`` (512,512,3).  Computed once per process; do not write to it."""
    photo, quad = warp_case(case_id)
    return utils.extract_perspective(photo, quad, BOARD)


@functools.lru_cache(maxsize=None)
def oracle_board_bgr(case_id: str) -> np.ndarray:
    """Fixed reading, independent oracle: ``cref.extract_board`` (512,512,3).  Computed once per process; do not write to it."""
    photo, quad = warp_case(case_id)
    return cref.extract_board(photo, quad, BOARD)


def host_board_float_bgr(case_id: str) -> np.ndarray:
    """Float reading, host restatement, whole board."""
    photo, quad = warp_case(case_id)
    return classical.warp_perspective(photo, classical.get_perspective_transform(quad, DEST), BOARD, mode="float")


def oracle_bands_float_bgr(case_id: str):
    """Float reading, scalar oracle: [(rows, (len(rows),512,3))] for the three row bands."""
    photo, quad = warp_case(case_id)
    m = cref.perspective_matrix(quad, DEST.astype(np.float64))
    return [(rows, cref.warp_perspective_float(photo, m, BOARD, rows=rows)[rows.start:rows.stop]) for rows in BANDS]


def area_images(case, seed: int = 0) -> np.ndarray:
    """(AREA_BATCH,h,w,c) random uint8 of an INTER_AREA case."""
    (h, w, c), (oh, ow) = case
    return np.random.default_rng(seed * 7919 + h * 4099 + w * 131 + c * 17 + oh * 5 + ow).integers(0, 256, (AREA_BATCH, h, w, c), dtype=np.uint8)


def area_host(image: np.ndarray, out_hw) -> np.ndarray:
    return classical.resize_area(image, (out_hw[1], out_hw[0]))            # the host form takes (width, height)


def area_oracle(image: np.ndarray, out_hw) -> np.ndarray:
    h, w, _ = image.shape
    shrink = out_hw[0] <= h and out_hw[1] <= w
    return cref.resize_area(image, out_hw) if shrink else cref.resize_area_enlarge(image, out_hw)

"""Independent oracle for the board-extraction quality scores (TEST INFRASTRUCTURE ONLY).

The four scores written literally in numpy from their published behaviour (reference ``scripts/process_new_raw/process_pipeline.py:357-467``:
``np.histogram`` over ten bins of [0, 1] and its entropy; ``np.sort`` and the mean distance from 0.5 of the top quarter; the ratio
of mask pixels to the filled largest outer contour; the spread of a quadrangle's sides and angles).  Completeness has no OpenCV to
lean on here: the outer borders and their areas come from the plain-C Suzuki-Abe oracle (``oracle.contours_c``), and ``filled`` --
what ``cv2.drawContours(thickness=-1)`` of the chosen border sets -- is restated as the 8-connected component under that border with
its holes filled (``scipy.ndimage``).  Shares no code with ``chessvision/quality.py`` or ``csrc/``."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

from oracle import contours_c


def probability_distribution(mask: np.ndarray) -> float:
    hist, _ = np.histogram(mask.flatten(), bins=10, range=(0, 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        hist = hist / np.sum(hist)
        entropy = -np.sum(hist * np.log2(hist + 1e-10))
    max_entropy = -np.log2(1 / 10)
    return float(1.0 - (entropy / max_entropy))


def histogram10(values: np.ndarray) -> np.ndarray:
    return np.histogram(np.asarray(values).flatten(), bins=10, range=(0, 1))[0]


def probability_confidence(probabilities: np.ndarray) -> float:
    """The float32 literal (numpy's mean: pairwise float32 summation for a float32 array)."""
    flat = probabilities.flatten()
    k = int(flat.size * 0.25)
    top = np.sort(flat)[-k:]
    return float(np.mean(np.abs(top - 0.5)) * 2)


def probability_confidence_f64(values: np.ndarray) -> float:
    """The same selection, |v - 0.5| in the dtype of ``values`` (float32: numpy's ``sorted - 0.5``), the mean in float64."""
    flat = np.asarray(values).flatten()
    k = int(flat.size * 0.25)
    top = np.sort(flat)[-k:]
    return float(np.mean(np.abs(top - flat.dtype.type(0.5)).astype(np.float64)) * 2)


def sigmoid64(logits: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(logits, dtype=np.float64)))


def outer_contours(binary: np.ndarray):
    """Outer borders of the 8-connected components (cv2.findContours RETR_EXTERNAL) in the oracle's OpenCV order, and their areas."""
    contours, holes = contours_c.find_contours((binary != 0).astype(np.uint8), contours_c.NONE)
    outer = [c for c, hole in zip(contours, holes) if not hole]
    return outer, [contours_c.contour_area(c) for c in outer]


def mask_completeness_binary(binary: np.ndarray):
    """(score, tie): score for a 0 / non-0 mask; tie = the two largest outer-contour areas are equal (the choice is not pinned)."""
    binary = np.asarray(binary) != 0
    outer, areas = outer_contours(binary)
    if not outer:
        return 0.0, False
    best = int(np.argmax(areas))                               # first of the largest, as Python's max(contours, key=contourArea)
    tie = sorted(areas)[-2] == areas[best] if len(areas) > 1 else False
    labels, _ = ndimage.label(binary, structure=np.ones((3, 3), dtype=bool))
    x, y = outer[best][0, 0]
    filled = ndimage.binary_fill_holes(labels == labels[y, x])     # 4-connected background, as the fill of an 8-connected border
    filled_area = float(np.count_nonzero(filled))
    if filled_area == 0:
        return 0.0, tie
    return float(np.count_nonzero(binary)) / filled_area, tie


def mask_completeness(mask: np.ndarray) -> float:
    return mask_completeness_binary(np.asarray(mask) > 0.5)[0]


def quadrangle_regularity(quadrangle) -> float:
    """In the dtype of the input, as the reference computes it (float32 for a float32 quadrangle)."""
    if quadrangle is None:
        return 0.0
    q = np.asarray(quadrangle).copy().squeeze(1)
    sides = [np.sqrt(((q[i] - q[(i + 1) % 4]) ** 2).sum()) for i in range(4)]
    angles = []
    for i in range(4):
        v1, v2 = q[(i - 1) % 4] - q[i], q[(i + 1) % 4] - q[i]
        norm = np.linalg.norm(v1) * np.linalg.norm(v2)
        angles.append(np.arccos(np.dot(v1, v2) / norm) if norm > 0 else 0)
    side_term = np.std(sides) / np.mean(sides) if np.mean(sides) > 0 else 1.0
    angle_term = np.std(angles) / (np.pi / 2)
    return float(1.0 - (side_term * 0.5 + angle_term * 0.5))

"""Board-extraction quality scores: the four floats the reference's enrichment job writes per image into its 3LC table beside the
FEN (``scripts/process_new_raw/process_pipeline.py:287-311``, the functions at ``357-467`` there) -- ``confidence``, ``distribution``,
``completeness`` and ``quad_score``, the columns new uploads are sorted and filtered by.

The four functions below keep the reference's names, signatures and semantics and work on host arrays.  The two geometric ones call
the native host code (``csrc/contour.cpp``); the two reductions are numpy, written so that they return the same float as the
reference's ``np.histogram`` / ``np.sort`` formulation.  The batched pipeline does not come through here: with
``ChessVision.process_images(quality=...)`` the reductions run on the device, on the logits where the UNet left them
(``HipEngine.extraction_scores``).  ``extraction_quality`` builds the same record for a single ``BoardExtractionResult`` on the host.

Two readings of "the probabilities" exist and both are offered (``of=`` here, ``quality=`` on ``process_images``):

``"logits"``   the reference's letter: it passes ``BoardExtractionResult.probabilities``, which holds the RAW LOGITS, to all three
               array scores, so its histogram sees only the logits that happen to fall in [0, 1] and its mask is ``logit > 0.5``.
``"sigmoid"``  what the column names promise: the scores of ``sigmoid(logits)``.
"""
from __future__ import annotations

import numpy as np

from . import hip_backend
from .cv_types import BoardExtractionResult, ExtractionQuality

# np.histogram(a, bins=10, range=(0, 1)) builds its edges in the dtype of `a`: for float32 input these are the float32 nearest i / 10,
# and values are compared with them in float32 (float64 edges put float32(0.7) and float32(0.9) one bin lower)
_EDGES64 = np.arange(11, dtype=np.float64) / 10.0


def _histogram10(values: np.ndarray) -> np.ndarray:
    """``np.histogram(values, bins=10, range=(0, 1))[0]`` by the rule the device kernel uses: bin i holds e[i] <= v < e[i+1], v == 1
    joins the last bin, everything else (NaN, inf, outside [0, 1]) is dropped."""
    a = np.asarray(values).reshape(-1)
    if a.dtype != np.float32:
        a = a.astype(np.float64)
    edges = _EDGES64.astype(a.dtype)
    with np.errstate(invalid="ignore"):
        inside = a[(a >= 0) & (a <= 1)]
    return np.bincount(np.searchsorted(edges[1:10], inside, side="right"), minlength=10)


def probability_distribution(mask: np.ndarray) -> float:
    """1 - (entropy of the ten-bin histogram of ``mask`` over [0, 1]) / log2(10): 1 when every counted value shares one bin, 0 when
    the bins are evenly filled; NaN when nothing lies in [0, 1] (the reference's 0 / 0)."""
    hist = _histogram10(mask)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = hist / np.sum(hist)
        entropy = -np.sum(p * np.log2(p + 1e-10))
    return float(1.0 - entropy / -np.log2(1 / 10))


def probability_confidence(probabilities: np.ndarray) -> float:
    """``np.mean(np.abs(np.sort(flat)[-k:] - 0.5)) * 2`` with k = flat.size // 4: twice the mean distance from 0.5 of the largest
    quarter.  Selects with ``np.partition`` and sorts the quarter only; NaN when the array holds a NaN."""
    flat = np.asarray(probabilities).reshape(-1)
    k = int(flat.size * 0.25)
    if k == 0:
        top = np.sort(flat)                                   # numpy's [-0:] is the whole array
    else:
        top = np.sort(np.partition(flat, flat.size - k)[flat.size - k:])
    return float(np.mean(np.abs(top - 0.5)) * 2)


def mask_completeness(mask: np.ndarray) -> float:
    """``mask > 0.5`` pixels divided by the pixels of the filled outline of the largest connected part of that binary mask (native:
    ``hip_backend.mask_completeness``); 0.0 when the binary mask is empty, above 1 when parts lie outside the largest outline."""
    return hip_backend.mask_completeness((np.asarray(mask) > 0.5).astype(np.uint8))


def quadrangle_regularity(quadrangle: np.ndarray | None) -> float:
    """(4,1,2) corners (or None: 0.0) -> 1 - 0.5 std(sides) / mean(sides) - 0.5 std(angles) / (pi / 2); 1.0 for a square."""
    if quadrangle is None:
        return 0.0
    return hip_backend.quadrangle_regularity(np.asarray(quadrangle))


def extraction_quality(extraction: BoardExtractionResult, of: str = "logits") -> ExtractionQuality:
    """The record ``process_images(quality=of)`` attaches, for ONE result, on the host.  ``quad_score`` is taken from the quadrangle
    the result's own mask yields (mask pixels; scoring the stored, image-scaled quadrangle would also score a fallback quadrangle),
    and is 0 when it yields none."""
    if of not in ("logits", "sigmoid"):
        raise ValueError(f"of must be 'logits' or 'sigmoid', got {of!r}")
    values = np.asarray(extraction.probabilities, dtype=np.float32)
    if of == "sigmoid":
        with np.errstate(over="ignore"):
            values = (np.float32(1) / (np.float32(1) + np.exp(-values))).astype(np.float32)
    return ExtractionQuality(confidence=probability_confidence(values),
                             quad_score=quadrangle_regularity(hip_backend.find_quadrangle(extraction.binary_mask)),
                             completeness=mask_completeness(values), distribution=probability_distribution(values))

"""CPU, OPTIONAL: mask completeness against the REAL OpenCV, for whoever has `cv2` installed (the build container and the GPU boxes of
this repository do not: the whole module is skipped there, and nothing in the repository may depend on it).  ``filled`` -- what
``cv2.drawContours(thickness=-1)`` sets for the largest outer contour -- is restated in csrc/contour.cpp as "the component plus what
it encloses"; only this test can turn that restatement into a measured match:
`pip install opencv-python-headless==4.11.0.86 && python -m pytest tests/test_quality_against_cv2_if_installed.py -q`.

Reference call site: scripts/process_new_raw/process_pipeline.py:380-414."""
from __future__ import annotations

import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

from chessvision import hip_backend  # noqa: E402

from ragged import label_masks, ragged_set  # noqa: E402


def _cv2_completeness(mask):
    binary = (mask > 0).astype(np.uint8)
    contours, _ = cv2.findContours(binary, cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)
    if not contours:
        return 0.0, False
    areas = [cv2.contourArea(c) for c in contours]
    filled = np.zeros_like(binary)
    cv2.drawContours(filled, [contours[int(np.argmax(areas))]], 0, 1, -1)
    tie = len(areas) > 1 and sorted(areas)[-2] == max(areas)
    return (float(binary.sum()) / float(filled.sum()) if filled.sum() else 0.0), tie


def test_mask_completeness_on_label_and_ragged_masks():
    masks = list(label_masks()) + [m for m, _, _ in ragged_set(400)]
    for k, mask in enumerate(masks):
        want, tie = _cv2_completeness(mask)
        got = hip_backend.mask_completeness(mask)
        assert got == pytest.approx(want, rel=1e-12) or tie, k

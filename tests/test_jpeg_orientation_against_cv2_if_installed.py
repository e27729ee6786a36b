"""``cv2.imdecode(blob, cv2.IMREAD_COLOR)`` against the host decode turned by ``jpeg.apply_orientation``, where OpenCV is installed:
the reference's callers decode uploads that way, and OpenCV's source reads as if it applied the EXIF orientation with these flags.
Where this test runs, that reading has been run; elsewhere it is skipped and stays a reading."""
from __future__ import annotations

import numpy as np
import pytest

import jpeg_orientation_cases as cases
from chessvision import jpeg

cv2 = pytest.importorskip("cv2")


def test_imdecode_equals_the_turned_host_decode_on_the_colour_cases():
    seen = 0
    for c in cases.load():
        if c.gray:
            continue
        theirs = cv2.imdecode(np.frombuffer(c.blob, np.uint8), cv2.IMREAD_COLOR)
        ours = jpeg.apply_orientation(jpeg.decode(c.blob, "bgr"), c.tag)
        assert theirs is not None and theirs.shape == ours.shape and np.array_equal(theirs, ours), c.name
        seen += 1
    assert seen == 3 * (9 * 9 + 2)

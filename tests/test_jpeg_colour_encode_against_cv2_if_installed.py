"""``cv2.imencode(".jpg", bgr, [IMWRITE_JPEG_QUALITY, q])`` against the numpy form of the colour encoder, where OpenCV is installed (the
production endpoint writes the uploaded photo with ``cv2.imwrite``, whose sampling is libjpeg's default, 4:2:0).  OpenCV's header may
differ from Pillow's (its APP0 density, for one), so the comparison is of what decides the pixels: the quantisation tables, the Huffman
tables, the frame header and the entropy-coded segment.  OpenCV has not been run where this file was written: it is skipped there."""
from __future__ import annotations

import numpy as np
import pytest

import jpeg_colour_encode_cases as cases
from chessvision import jpeg

cv2 = pytest.importorskip("cv2")


def _segments(blob: bytes) -> dict:
    """marker -> list of payloads, plus "scan": everything from behind the SOS header up to EOI."""
    out, at = {}, 2
    while at < len(blob):
        assert blob[at] == 0xFF
        marker, size = blob[at + 1], int.from_bytes(blob[at + 2:at + 4], "big")
        out.setdefault(marker, []).append(blob[at + 4:at + 2 + size])
        at += 2 + size
        if marker == 0xDA:
            out["scan"] = blob[at:-2]
            break
    return out


@pytest.mark.parametrize("quality", [1, 50, 95, 100])
def test_tables_and_scan_equal_opencv(quality):
    z = cases.load()
    images = [z["image/17x33/noise"], z["image/64x64/smooth"], z["image/2x9/primaries"], z["image/24x40/binary"], cases.photo_crop()]
    for a in images:
        ok, buf = cv2.imencode(".jpg", np.ascontiguousarray(a), [cv2.IMWRITE_JPEG_QUALITY, quality])
        assert ok
        theirs, ours = _segments(buf.tobytes()), _segments(jpeg.encode_colour(a, quality, "4:2:0", "bgr"))
        assert b"".join(theirs[0xDB]) == b"".join(ours[0xDB])           # DQT, both tables (one segment or two)
        assert b"".join(theirs[0xC4]) == b"".join(ours[0xC4])           # DHT, all four tables
        assert theirs[0xC0] == ours[0xC0] and theirs[0xDA] == ours[0xDA] and theirs["scan"] == ours["scan"]

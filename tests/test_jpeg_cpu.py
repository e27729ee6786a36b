"""CPU: the host half of the JPEG decoder (csrc/jpeg.cpp through ctypes) and the numpy form of the device half (chessvision/jpeg.py:
reconstruct) against bytes a real libjpeg produced.  tests/golden/jpeg_cases.npz holds streams Pillow wrote with Pillow's own decode of
each; photos8_jpeg_{a,b}.npz hold the original bytes of the eight reference photos whose Pillow decode photos8_{i}.npz has held all
along.  Every comparison is equality of bytes."""
from __future__ import annotations

import io
import threading
import time
from pathlib import Path

import numpy as np
import pytest

from chessvision import jpeg

GOLDEN = Path(__file__).resolve().parent / "golden"
# Only the live comparison below looks there, on the build machine; anywhere else the directory is absent and that test skips.
REFERENCE_DATA = "/root/reference/data"


@pytest.fixture(scope="module")
def cases():
    z = np.load(GOLDEN / "jpeg_cases.npz")
    out = []
    for i, name in enumerate(z["names"]):
        name = str(name)
        out.append({"name": name, "kind": str(z["kind"][i]), "group": str(z["group"][i]), "reason": str(z["reason"][i]),
                    "orientation": int(z["orientation"][i]), "blob": z[f"blob/{name}"].tobytes(),
                    "pixels": z[f"pixels/{name}"] if f"pixels/{name}" in z.files else None})
    return out


def photo_blobs():
    blobs = []
    for tag in "ab":
        z = np.load(GOLDEN / f"photos8_jpeg_{tag}.npz")
        blobs += [(str(n), z[f"blob_{k}"].tobytes()) for k, n in enumerate(z["names"])]
    return blobs


def test_fixture_covers_what_the_issue_lists(cases):
    groups = {c["group"] for c in cases if c["kind"] == "group"}
    grid = (1, 2, 3, 15, 16, 17, 33)
    assert {f"420_{w}x{h}" for w in grid for h in grid} <= groups
    for s in ("422", "444", "gray"):
        assert {f"{s}_{v}x{v}" for v in grid} | {f"{s}_33x15", f"{s}_15x33"} <= groups
    assert all(sum(c["group"] == g for c in cases) == 3 for g in groups)
    assert {"optimize", "restart_blocks", "restart_rows", "quality1", "exif_orientation", "comment"} <= {c["name"] for c in cases}
    assert {"progressive", "sampling_411", "truncated_in_marker_code", "truncated_in_quant_table", "truncated_in_huffman_table",
            "truncated_in_scan"} <= {c["name"] for c in cases if c["kind"] == "refusal"}


def test_every_supported_case_equals_pillow_in_every_channel_order(cases):
    n = 0
    for c in cases:
        if c["kind"] == "refusal":
            continue
        coeffs, qtables, info = jpeg.entropy_decode(c["blob"])
        assert info.supported and coeffs.dtype == np.int16 and coeffs.size == 64 * info.blocks and qtables.shape == (info.components, 64)
        want = c["pixels"]
        if info.components == 1:
            assert want.shape == (info.height, info.width)
            assert np.array_equal(jpeg.reconstruct(coeffs, qtables, info, "gray"), want), c["name"]
            want = np.repeat(want[:, :, None], 3, axis=2)
        else:
            with pytest.raises(ValueError):
                jpeg.reconstruct(coeffs, qtables, info, "gray")
        assert want.shape == (info.height, info.width, 3)
        assert np.array_equal(jpeg.reconstruct(coeffs, qtables, info, "rgb"), want), c["name"]
        assert np.array_equal(jpeg.reconstruct(coeffs, qtables, info, "bgr"), want[:, :, ::-1]), c["name"]
        n += 1
    assert n >= 3 * (49 + 27) + 6


def test_the_eight_photos_equal_their_committed_pillow_decode():
    for i, (name, blob) in enumerate(photo_blobs()):
        z = np.load(GOLDEN / f"photos8_{i}.npz")
        assert str(z["names"][0]) == name
        info = jpeg.jpeg_info(blob)
        assert info.geometry == (512, 512, 3, 2, 2) and info.supported
        assert np.array_equal(jpeg.decode(blob, "bgr"), z["bgr"][0]), name
        assert np.array_equal(jpeg.decode(blob, "rgb"), z["bgr"][0][:, :, ::-1]), name


def test_refusals_name_their_reason_and_an_offset_inside_the_buffer(cases):
    seen = 0
    for c in cases:
        if c["kind"] != "refusal":
            continue
        info = jpeg.jpeg_info(c["blob"])
        with pytest.raises(jpeg.UnsupportedJpeg) as err:
            jpeg.entropy_decode(c["blob"])
        text = str(err.value)
        assert c["reason"] in text and " at byte " in text, (c["name"], text)
        offset = int(text.rsplit(" at byte ", 1)[1].split()[0].rstrip(";"))
        assert 0 <= offset < max(1, len(c["blob"])), (c["name"], text, len(c["blob"]))
        if not c["name"].startswith("truncated") or "scan" not in c["name"] and "eoi" not in c["name"]:
            assert not info.supported and c["reason"] in info.reason, (c["name"], info)    # the header alone says so
        seen += 1
    assert seen >= 10
    assert not jpeg.jpeg_info(b"").supported and not jpeg.jpeg_info(b"not a jpeg at all").supported


def test_info_fields(cases):
    by_name = {c["name"]: c for c in cases}
    for c in cases:
        if c["kind"] == "refusal":
            continue
        info = jpeg.jpeg_info(c["blob"])
        h, w = c["pixels"].shape[:2]
        assert (info.width, info.height) == (w, h) and info.supported and info.reason == "" and info.orientation == c["orientation"]
        if c["kind"] == "group":
            sampling = c["group"].split("_")[0]
            assert (info.components, info.luma_h, info.luma_v) == {"420": (3, 2, 2), "422": (3, 2, 1), "444": (3, 1, 1), "gray": (1, 1, 1)}[sampling]
    assert by_name["exif_orientation"]["orientation"] == 6 and jpeg.jpeg_info(by_name["exif_orientation"]["blob"]).orientation == 6
    assert jpeg.jpeg_info(by_name["restart_blocks"]["blob"]).restart_interval == 1
    assert jpeg.jpeg_info(by_name["restart_rows"]["blob"]).restart_interval == 3           # one row of 48 / 16 MCUs
    assert jpeg.jpeg_info(by_name["optimize"]["blob"]).restart_interval == 0
    info = jpeg.jpeg_info(by_name["420_17x33_0"]["blob"])
    assert info.plane_blocks == ((6, 4), (3, 2), (3, 2)) and info.blocks == 36


def test_entropy_decode_writes_in_place_and_checks_capacity(cases):
    blob = next(c for c in cases if c["name"] == "420_33x17_0")["blob"]
    info = jpeg.jpeg_info(blob)
    staging = np.full(64 * info.blocks + 64, 12345, np.int16)
    tables = np.zeros((3, 64), np.uint16)
    coeffs, qtables, _ = jpeg.entropy_decode(blob, info, staging[:64 * info.blocks], tables)
    fresh, fresh_q, _ = jpeg.entropy_decode(blob)
    assert np.array_equal(staging[:64 * info.blocks], fresh) and np.array_equal(tables, fresh_q) and (staging[64 * info.blocks:] == 12345).all()
    with pytest.raises(ValueError):
        jpeg.entropy_decode(blob, info, staging[:64 * info.blocks - 64], tables)


def test_entropy_decode_releases_the_gil():
    """ctypes drops the GIL around a call unless the library was loaded as a PyDLL (FUNCFLAG_PYTHONAPI); and another Python thread
    does make progress while this one decodes."""
    import ctypes

    from chessvision.hip_backend import load_library

    lib = load_library()
    assert isinstance(lib, ctypes.CDLL) and not isinstance(lib, ctypes.PyDLL)
    assert not lib.cv_jpeg_entropy_decode._flags_ & ctypes._FUNCFLAG_PYTHONAPI
    blob = photo_blobs()[0][1]
    info = jpeg.jpeg_info(blob)
    coeffs, tables = np.empty(64 * info.blocks, np.int16), np.empty((3, 64), np.uint16)
    ticks, stop = [0], threading.Event()

    def spin():
        while not stop.is_set():
            ticks[0] += 1

    t = threading.Thread(target=spin)
    t.start()
    try:
        time.sleep(0.02)
        before, inside = ticks[0], 0.0
        for _ in range(40):
            t0 = time.perf_counter()
            jpeg.entropy_decode(blob, info, coeffs, tables)
            inside += time.perf_counter() - t0
        gained = ticks[0] - before
    finally:
        stop.set()
        t.join()
    assert inside > 0.005 and gained > 1000, (inside, gained)


def test_live_pillow_over_the_reference_data():
    """All colour files and every tenth 1-component file of the reference's data decode natively and equal Pillow's pixels."""
    Image = pytest.importorskip("PIL.Image")
    root = Path(REFERENCE_DATA)
    if not root.is_dir():
        pytest.skip("the reference's data is not on this machine")
    files = sorted(p for p in root.rglob("*") if p.suffix.lower() in (".jpg", ".jpeg"))
    colour, single = [], []
    for p in files:
        blob = p.read_bytes()
        info = jpeg.jpeg_info(blob)
        assert info.supported, (p, info.reason)
        (colour if info.components == 3 else single).append((p, blob, info))
    assert len(colour) >= 600 and len(single) >= 10000
    for p, blob, info in colour + single[::10]:
        want = np.asarray(Image.open(io.BytesIO(blob)))
        assert np.array_equal(jpeg.decode(blob, "rgb" if info.components == 3 else "gray"), want), p

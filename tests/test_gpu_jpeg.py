"""GPU: the device half of the JPEG decoder (csrc/jpeg.hip through ``HipEngine.jpeg_decode``) against the numpy form
(``jpeg.reconstruct``) and against the pixels Pillow (libjpeg-turbo) recorded in tests/golden/jpeg_cases.npz.  Every geometry group is
one launch of three images with three different quantisation tables; every comparison is equality of bytes."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

from chessvision import jpeg

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def engine():
    from chessvision.hip_backend import HipEngine

    eng = HipEngine(precision="f32")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def groups():
    z = np.load(GOLDEN / "jpeg_cases.npz")
    out: dict[str, list] = {}
    for name, kind, group in zip(z["names"], z["kind"], z["group"]):
        if str(kind) == "group":
            out.setdefault(str(group), []).append((z[f"blob/{name}"].tobytes(), z[f"pixels/{name}"]))
    features = [(str(n), z[f"blob/{n}"].tobytes(), z[f"pixels/{n}"]) for n, k in zip(z["names"], z["kind"]) if str(k) == "feature"]
    return out, features


def test_every_geometry_group_equals_numpy_and_pillow(engine, groups):
    from chessvision.hip_backend import HipBackendError

    by_group, _ = groups
    assert len(by_group) == 49 + 3 * 9
    for name, members in by_group.items():
        blobs, want = [b for b, _ in members], np.stack([p for _, p in members])
        assert len(blobs) == 3
        decoded = [jpeg.entropy_decode(b) for b in blobs]
        gray = name.startswith("gray")
        orders = ("bgr", "rgb", "gray") if gray else ("bgr", "rgb")
        for order in orders:
            got = engine.jpeg_decode(blobs, order).cpu().numpy()
            host = np.stack([jpeg.reconstruct(c, q, f, order) for c, q, f in decoded])
            assert got.shape == host.shape and np.array_equal(got, host), (name, order)
            pillow = want if order == "gray" else np.repeat(want[..., None], 3, axis=3) if gray else want if order == "rgb" else want[..., ::-1]
            assert np.array_equal(got, pillow), (name, order)
        if not gray:
            with pytest.raises(HipBackendError, match="1-component"):
                engine.jpeg_decode(blobs, "gray")


def test_stream_features_decode_to_pillows_pixels(engine, groups):
    _, features = groups
    assert len(features) == 6
    for name, blob, want in features:
        assert np.array_equal(engine.jpeg_decode([blob], "rgb").cpu().numpy()[0], want), name
    # restart intervals, custom Huffman tables, a comment and EXIF change nothing about the geometry: one launch takes them together
    same = [b for n, b, _ in features if n != "quality1"]
    got = engine.jpeg_decode(same, "rgb").cpu().numpy()
    assert np.array_equal(got, np.stack([w for n, _, w in features if n != "quality1"]))


def test_the_eight_photos_equal_their_committed_decode(engine):
    blobs = []
    for tag in "ab":
        z = np.load(GOLDEN / f"photos8_jpeg_{tag}.npz")
        blobs += [z[f"blob_{k}"].tobytes() for k in range(len(z["names"]))]
    want = np.concatenate([np.load(GOLDEN / f"photos8_{i}.npz")["bgr"] for i in range(8)])
    got = engine.jpeg_decode(blobs)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (8, 512, 512, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(engine.jpeg_decode(blobs, "rgb").cpu().numpy(), want[..., ::-1])


def test_coefficients_must_be_16_byte_aligned_and_a_misaligned_view_is_refused(engine, groups):
    """The kernel loads a row of a block (8 int16) with one 16-byte load: the ABI asks for 16-byte aligned coefficients and tables
    (include/chessvision_hip.h) and refuses anything else instead of faulting."""
    from chessvision.hip_backend import HipBackendError

    members = groups[0]["420_33x17"]
    decoded = [jpeg.entropy_decode(b) for b, _ in members]
    info = decoded[0][2]
    count = 64 * info.blocks
    flat = torch.zeros(3 * count + 8, dtype=torch.int16)
    for k, (c, _, _) in enumerate(decoded):
        flat[1 + k * count:1 + (k + 1) * count] = torch.from_numpy(c)
    qt = torch.from_numpy(np.stack([q for _, q, _ in decoded]).view(np.int16)).to(engine.device)
    dev = flat.to(engine.device)
    shifted = dev[1:1 + 3 * count].view(3, count)                     # the same coefficients, two bytes off
    assert shifted.data_ptr() % 16 == 2
    with pytest.raises(HipBackendError, match="16-byte aligned"):
        engine.jpeg_reconstruct_dev(shifted, qt, info, "rgb")
    aligned = shifted.clone()
    got = engine.jpeg_reconstruct_dev(aligned, qt, info, "rgb").cpu().numpy()
    assert np.array_equal(got, np.stack([p for _, p in members]))


def test_mixed_geometries_in_one_engine_call_are_refused(engine, groups):
    from chessvision.hip_backend import HipBackendError

    by_group, _ = groups
    a, b = by_group["420_16x16"][0][0], by_group["gray_33x33"][0][0]
    with pytest.raises(HipBackendError, match="one geometry"):
        engine.jpeg_decode([a, b])

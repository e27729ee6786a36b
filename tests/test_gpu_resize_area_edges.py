"""GPU: INTER_AREA on the device (``resize_area_2x2c3_kernel``, ``resize_area_tab_kernel``, ``resize_area_u8_kernel``) at its edges --
the geometries of tests/byte_edge_cases.py: every channel count from 1 to 5, integer factors other than 2 x 2, an integer factor in one
axis and a fraction in the other, one-pixel axes, enlarging in one or both axes, and every fall-back of the 2 x 2 x 3-channel fast path
(width not a multiple of 4, other channel counts, a source off its 8-byte boundary).  device == host == oracle, byte for byte, on
every image of a batch of three; no tolerance."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import byte_edge_cases as bec

pytestmark = pytest.mark.gpu


def _device(eng, images: np.ndarray, out_hw) -> np.ndarray:
    return eng.resize_area_u8(torch.from_numpy(images), out_hw).cpu().numpy()


def _check(got: np.ndarray, images: np.ndarray, out_hw, what) -> None:
    assert got.shape == (len(images), out_hw[0], out_hw[1], images.shape[3]), what
    for k, image in enumerate(images):
        host = bec.area_host(image, out_hw)
        assert np.array_equal(got[k], host), (what, k, int(np.abs(got[k].astype(int) - host.astype(int)).max()), float((got[k] != host).mean()))
        assert np.array_equal(got[k], bec.area_oracle(image, out_hw)), (what, k)


@pytest.mark.parametrize("case", bec.AREA_CASES, ids=[bec.area_id(c) for c in bec.AREA_CASES])
def test_device_equals_host_and_oracle(engines, case):
    images = bec.area_images(case)
    _check(_device(engines["f32"], images, case[1]), images, case[1], bec.area_id(case))


def test_source_off_its_eight_byte_boundary(engines):
    """The 2 x 2, 3-channel geometry from a source that starts 3 bytes into its allocation (a contiguous view of a flat buffer): the fast
    path's 8-byte loads are not available, the alignment guard picks the generic kernel, and the bytes are those of the aligned call."""
    eng = engines["f32"]
    (h, w, c), out_hw = bec.AREA_MISALIGNED
    images = bec.area_images(bec.AREA_MISALIGNED)
    flat = torch.zeros(bec.AREA_MISALIGNED_OFFSET + images.size, dtype=torch.uint8, device=eng.device)
    flat[bec.AREA_MISALIGNED_OFFSET:] = torch.from_numpy(images).reshape(-1).to(eng.device)
    view = flat[bec.AREA_MISALIGNED_OFFSET:].view(images.shape)
    assert view.is_contiguous() and view.data_ptr() % 8 == bec.AREA_MISALIGNED_OFFSET
    got = eng.resize_area_u8(view, out_hw).cpu().numpy()
    _check(got, images, out_hw, "misaligned")
    assert np.array_equal(got, _device(eng, images, out_hw))               # the aligned call: the fast path


def test_interleaved_geometries_rebuild_the_cached_tables(engines):
    """The engine keeps the tables of ONE fractional geometry.  Two geometries that share (h, w) and differ in channels, two that differ
    only in (oh, ow), alternating, with new pixels every time."""
    eng = engines["f32"]
    order = [((37, 53, 1), (16, 24)), ((37, 53, 5), (16, 24)), ((37, 53, 1), (16, 24)),          # same tables, another channel count
             ((37, 53, 3), (16, 24)), ((37, 53, 3), (24, 16)), ((37, 53, 3), (16, 24)), ((37, 53, 3), (24, 16))]
    for seed, case in enumerate(order, start=1):
        images = bec.area_images(case, seed)
        _check(_device(eng, images, case[1]), images, case[1], (seed, bec.area_id(case)))

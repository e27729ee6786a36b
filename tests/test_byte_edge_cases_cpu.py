"""CPU: the case table of tests/byte_edge_cases.py is sound before a GPU sees it -- on every case the product's host restatement and
the independent oracle give the same bytes (fixed reading of the warp on the whole board, float reading on three row bands,
INTER_AREA on every image of the batch), and the native homographies equal the host's bit for bit.  A disagreement here is a finding
about the restatements, to be resolved against the OpenCV operation order both cite -- never by dropping the case."""
from __future__ import annotations

import numpy as np
import pytest

import byte_edge_cases as bec
from chessvision import classical


def test_the_table_holds_every_listed_case():
    shapes = {case_id: shape for case_id, shape, _ in bec.WARP_CASES}
    assert len(set(bec.WARP_IDS)) == len(bec.WARP_IDS) >= 18
    assert sum(shape == (37, 53) for shape in shapes.values()) == 11
    assert {shapes[k] for k in ("9x1", "9x2", "1x9", "1x1", "2x3-self-crossing", "4x40000", "40000x4")} == \
        {(9, 1), (9, 2), (1, 9), (1, 1), (2, 3), (4, 40000), (40000, 4)}
    assert set(bec.ROUTE_IDS) >= {"convex", "self-crossing", "9x1", "1x1", "far-outside"} and set(bec.ROUTE_IDS) <= set(bec.WARP_IDS)
    assert len(bec.AREA_CASES) == 23 and len({bec.area_id(c) for c in bec.AREA_CASES}) == 23
    assert {c[0][2] for c in bec.AREA_CASES} == {1, 2, 3, 4, 5} and bec.AREA_BATCH == 3
    assert bec.AREA_MISALIGNED[0][2] == 3 and bec.AREA_MISALIGNED_OFFSET % 8 != 0


@pytest.mark.parametrize("case_id", bec.WARP_IDS)
def test_warp_fixed_reading_host_equals_oracle_on_the_whole_board(case_id):
    a, b = bec.host_board_bgr(case_id), bec.oracle_board_bgr(case_id)
    assert a.shape == (512, 512, 3)
    assert np.array_equal(a, b), (int(np.abs(a.astype(int) - b.astype(int)).max()), float((a != b).mean()))
    assert np.array_equal(bec.gray_flip_host(a), bec.gray_flip_oracle(b))
    if case_id == "four-equal":                             # singular matrix -> zeros -> every board pixel reads source pixel (0,0)
        assert (a == bec.warp_case(case_id)[0][0, 0]).all()
    if case_id == "far-outside":
        assert not a.any()


@pytest.mark.parametrize("case_id", bec.WARP_IDS)
def test_warp_float_reading_host_equals_oracle_on_row_bands(case_id):
    host = bec.host_board_float_bgr(case_id)
    for rows, band in bec.oracle_bands_float_bgr(case_id):
        assert np.array_equal(host[rows.start:rows.stop], band), rows
    if case_id == "four-equal":                             # 0 / 0 maps nowhere: the border value
        assert not host.any()


@pytest.mark.parametrize("case_id", ["4x40000", "40000x4"])
def test_the_wide_photos_do_reach_the_int16_saturation(case_id):
    """What these two cases are for: every board pixel's source column (row) lies beyond 32767, so the fixed reading reads the
    saturated pixel -- the board is not what an unsaturated map would give."""
    photo, quad = bec.warp_case(case_id)
    axis = 1 if case_id == "4x40000" else 0
    cut = np.take(photo, range(32769), axis=axis)           # a photo that ends where the map saturates: same taps, hence same board
    assert np.array_equal(bec.host_board_bgr(case_id), classical.warp_perspective(
        cut, classical.get_perspective_transform(quad, bec.DEST), bec.BOARD, mode="fixed"))
    assert quad[:, 1 - axis].min() > 32768                  # quadrangles are (x, y); the photo's axis 1 is x


def test_native_homographies_equal_the_host_form_bit_for_bit():
    from chessvision.hip_backend import board_homographies

    quads = np.stack([bec.warp_case(case_id)[1] for case_id in bec.WARP_IDS])
    inv = board_homographies(quads, bec.BOARD)
    for k, case_id in enumerate(bec.WARP_IDS):
        want = classical.invert3(classical.get_perspective_transform(quads[k], bec.DEST))
        assert np.array_equal(inv[k], want), case_id
        assert np.array_equal(inv[k].view(np.uint64), want.view(np.uint64)), case_id      # signed zeros and all
    assert not inv[bec.WARP_IDS.index("four-equal")].any()


@pytest.mark.parametrize("case", bec.AREA_CASES + [bec.AREA_MISALIGNED], ids=[bec.area_id(c) for c in bec.AREA_CASES] + ["misaligned"])
def test_inter_area_host_equals_oracle(case):
    (h, w, c), out_hw = case
    for image in bec.area_images(case):
        a, b = bec.area_host(image, out_hw), bec.area_oracle(image, out_hw)
        assert a.shape == (out_hw[0], out_hw[1], c)
        assert np.array_equal(a, b), (int(np.abs(a.astype(int) - b.astype(int)).max()), float((a != b).mean()))

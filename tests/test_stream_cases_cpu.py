"""CPU: the preconditions of the two-stream table cases of tests/test_gpu_stream_contract.py, from the numpy forms of the tables
(``classical._area_tab``, ``classical.antialias_taps``).  Those cases let one stream rebuild the engine's cached resize tables while a
launch of another geometry is still queued; the pair of geometries is chosen so that even a library that swaps the tables under the
running kernel can only produce wrong pixels.  The GPU module asserts the same gate in front of its first launch."""
from __future__ import annotations

import pytest

import stream_probe as sp


def test_both_area_tables_have_one_layout_and_stay_inside_the_larger_image():
    a, b = (sp.area_table_facts(side, sp.TABLE_OUT) for side in sp.TABLE_PAIR)
    assert a["lengths"] == b["lengths"] == (17, 56, 56)
    assert (a["max_index"], b["max_index"]) == (41, 40)
    sp.assert_table_swap_cannot_leave_the_buffers(sp.area_table_facts)


def test_both_antialias_tables_have_one_layout_and_stay_inside_the_larger_image():
    a, b = (sp.antialias_table_facts(side, sp.TABLE_OUT) for side in sp.TABLE_PAIR)
    assert a["lengths"] == b["lengths"] == (16, 16, 16 * 6)
    assert a["widest"] == b["widest"] == 6
    assert (a["max_index"], b["max_index"]) == (41, 40)
    sp.assert_table_swap_cannot_leave_the_buffers(sp.antialias_table_facts)


@pytest.mark.parametrize("pair", [(42, 40), (53, 41)])
def test_the_gate_refuses_a_pair_whose_tables_differ_in_layout(pair):
    """42 -> 16 and 40 -> 16 differ in entry count (56 / 48 area entries, strides 6 / 5); so do 53 and 41: the gate must say so."""
    for facts in (sp.area_table_facts, sp.antialias_table_facts):
        with pytest.raises(AssertionError):
            sp.assert_table_swap_cannot_leave_the_buffers(facts, pair=pair)


def test_the_farthest_byte_of_the_smaller_batch_is_inside_the_shared_backing():
    n, c = sp.TABLE_BATCH, sp.TABLE_CHANNELS
    assert sp.backing_bytes() == n * 42 * 42 * c
    farthest = (((n - 1) * 41 + 41) * 41 + 41) * c + c - 1                        # row 41, column 41 of the last 41 x 41 image
    assert farthest < sp.backing_bytes()
    assert farthest >= n * 41 * 41 * c                                           # an allocation of the batch's own size would not do

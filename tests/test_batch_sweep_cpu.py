"""The batch-sweep helpers (tests/batch_sweep.py) without a GPU: the row-to-input map, the census classes and their representatives, the
figures against the whole-model bars, the replacement cap of the f16 pools and the report."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import batch_sweep as bs

A, B, C = (("l1", "k<64>"), ("l2", "k<64>")), (("l1", "k<64,splitK3>"), ("l2", "k<64>")), (("l1", "k<256>"), ("l2", "k<256>"), ("l1", "k<64>"))


# ---- pool_index -------------------------------------------------------------------------------------------------------------------------
def _reached(batches, pool, modulus):
    hit = np.zeros((pool, modulus), dtype=bool)
    for n in batches:
        i = np.arange(n)
        hit[bs.pool_rows(n, pool), i % modulus] = True
    return hit


@pytest.mark.parametrize("modulus", [2, 4, 8, 16, 64])
def test_every_square_of_the_pool_reaches_every_residue_of_the_tile_sizes(modulus):
    for every_kth in (1, 4):
        assert _reached(bs.resnet_batches(every_kth), bs.RESNET_POOL, modulus).all()


@pytest.mark.parametrize("modulus", [2, 4, 8, 16])
def test_every_image_of_the_pool_reaches_every_residue_of_the_tile_sizes(modulus):
    assert _reached(bs.UNET_BATCHES, bs.UNET_POOL, modulus).all()


def test_every_row_position_of_the_unet_chunk_meets_as_many_images_as_there_are_batches_that_have_it():
    """Residues of 64 for the UNet are row positions: row i exists in the 65 - i batches N > i, which move the pool by 3 each -- coprime to
    11, so those batches put min(11, 65 - i) distinct images there (all 11 up to row 54; rows 63 and 64 exist in two batches and one)."""
    hit = np.zeros((65, bs.UNET_POOL), dtype=bool)
    for n in bs.UNET_BATCHES:
        hit[np.arange(n), bs.pool_rows(n, bs.UNET_POOL)] = True
    assert [int(h.sum()) for h in hit] == [min(bs.UNET_POOL, 65 - i) for i in range(65)]


@pytest.mark.parametrize("pool, batches", [(bs.UNET_POOL, bs.UNET_BATCHES), (bs.RESNET_POOL, (1, 7, 64, 257, 258, 1000, 16385))])
def test_no_two_rows_less_than_a_pool_length_apart_share_an_input(pool, batches):
    for n in batches:
        rows = bs.pool_rows(n, pool)
        assert rows.min() >= 0 and rows.max() < pool and rows[0] == (3 * n) % pool
        for d in range(1, min(pool, n)):
            assert not (rows[d:] == rows[:-d]).any(), (n, d)


def test_the_pools_are_coprime_to_every_tile_group_and_chunk_size():
    for pool in (bs.UNET_POOL, bs.RESNET_POOL):
        assert all(math.gcd(pool, m) == 1 for m in (2, 3, 8, 16, 64, 128, 192, 256, 384, 512, 1024, 2048, 16384))
    assert bs.pool_index(5, 7, 11) == 4 and int(bs.pool_index(np.int64(256), 1, 257)) == 2


def test_the_swept_sizes():
    assert bs.UNET_BATCHES[0] == 65 and bs.UNET_BATCHES[-1] == 1 and len(bs.UNET_BATCHES) == 65
    r18, r34 = bs.resnet_batches(), bs.resnet_batches(4)
    assert list(r18) == sorted(r18, reverse=True) and r18[0] == 16385
    assert {64 * k for k in range(1, 65)} | set(bs.RESNET_RAGGED) | {8192, 16384, 16385} == set(r18)
    assert {256 * k for k in range(1, 17)} | set(bs.RESNET_RAGGED) | {8192, 16384, 16385} == set(r34) and 64 not in r34


def test_the_pools_hold_what_they_say():
    sq = bs.resnet_pool_u8()
    assert sq.shape == (257, 64, 64) and sq.dtype == np.uint8
    at = bs.RESNET_SPECIALS_AT
    assert not sq[at].any() and (sq[at + 1] == 255).all() and sq[at + 3].sum() == 255          # zero, full, corner_tl
    assert len({s.tobytes() for s in sq}) == 257
    again = bs.resnet_pool_u8({at: 1, 5: 2})
    assert again[at].any() and not np.array_equal(again[5], sq[5]) and np.array_equal(again[6], sq[6])
    assert [bs.unet_slot(j)[0] for j in range(11)].count("border") == 1 and len({bs.unet_slot(j)[1] for j in range(11)}) == 11
    assert bs.unet_slot(2) == ("border", bs.UNET_SEED + 14) and bs.unet_slot(2, 1) == ("random", bs.UNET_SEED + 14 + 1000)


# ---- classes ----------------------------------------------------------------------------------------------------------------------------
def test_classes_contiguous():
    cls = bs.classes({1: B, 2: A, 3: A, 4: A, 5: C})
    assert [(c["smallest"], c["largest"], c["members"]) for c in cls] == [(1, 1, [1]), (2, 4, [2, 3, 4]), (5, 5, [5])]
    assert [c["signature"] for c in cls] == [B, A, C]


def test_classes_non_contiguous_and_their_representatives():
    cen = {64: B, 128: A, 192: B, 256: A, 1024: C, 63: B, 7: A}
    cls = bs.classes(cen)
    assert [(c["smallest"], c["largest"]) for c in cls] == [(7, 256), (63, 192), (1024, 1024)]
    assert cls[0]["members"] == [7, 128, 256] and cls[1]["members"] == [63, 64, 192]
    assert bs.class_of(cls, 192) is cls[1]
    assert bs.ranges(cls[0]["members"]) == "7, 128, 256" and bs.ranges([1, 2, 3, 7, 9, 10]) == "1-3, 7, 9-10"
    assert bs.ranges([64, 128, 192, 1000], swept=[63, 64, 128, 192, 256, 1000]) == "64..192, 1000"
    assert bs.ranges([63, 64, 65, 100, 128, 1000], swept=[1, 63, 64, 65, 100, 128, 192, 1000]) == "63..128, 1000"
    assert bs.ranges([1, 7, 63, 64], swept=[1, 7, 63, 64, 65]) == "1..64" and bs.ranges([1, 7], swept=[1, 7, 63]) == "1, 7"
    assert bs.tripwire(cls, [7], 256) == [63] and bs.tripwire(cls, [7, 63], 256) == [] and bs.tripwire(cls, [], 8) == [7]
    assert bs.tripwire(cls, [64, 128], 256) == [7, 63]                  # a member that is not the smallest does not count


def test_signature_diff_and_the_failure_text():
    assert bs.signature_diff(A, A) == []
    assert bs.signature_diff(B, A) == [("l1", "k<64,splitK3>", "k<64>")]
    assert bs.signature_diff(A, C) == [("l1", "k<64>", "k<256>"), ("l2", "k<64>", "k<256>"), ("l1 #2", "-", "k<64>")]
    assert bs.signature_diff((("pool", ""),), (("pool", "p<2>"),)) == [("pool", "(no kernel string)", "p<2>")]
    cls = bs.classes({1: B, 2: A, 3: A, 5: C})
    text = bs.describe_class(cls, 1, passing=[2, 3, 5])
    assert "n in {1}" in text and "nearest passing n = 2" in text and "l1: k<64,splitK3>   (n = 2: k<64>)" in text
    assert "no n outside this class passed" in bs.describe_class(cls, 1, passing=[1])
    assert "nearest passing n = 5" in bs.describe_class(cls, 3, passing=[3, 5])


def test_thinning_keeps_the_class_edges_and_their_neighbours():
    cen = {n: (A if n <= 7 else B if n <= 40 else C) for n in range(1, 66)}
    assert bs.thin(bs.classes(cen), range(1, 66)) == [65, 64, 42, 41, 40, 39, 9, 8, 7, 6, 2, 1]


# ---- the figures ------------------------------------------------------------------------------------------------------------------------
def test_row_figures_name_the_row_the_metric_and_hold_the_stated_bars():
    ref = torch.linspace(-3, 3, 5 * 13).reshape(5, 13).flip(1)
    ok = bs.row_figures("resnet", "f16x3", ref + 9e-4, ref)
    assert ok["ok"] and ok["metric"] == "logit" and ok["bar"] == 1e-3 and set(ok["figures"]) == {"logit", "agree"}
    got = ref.clone()
    got[4, 3] += 2e-3
    bad = bs.row_figures("resnet", "f32", got, ref)
    assert not bad["ok"] and bad["row"] == 4 and bad["metric"] == "logit" and bad["ratio"] == pytest.approx(2.0, rel=1e-3)
    f16 = bs.row_figures("resnet", "f16r", got, ref)                       # 2e-3 is inside 5e-3 max(1, max|ref row|)
    assert f16["ok"] and f16["figures"]["logit"][1] == pytest.approx(5e-3 * float(ref[4].abs().max())) and "prob" in f16["figures"]
    got = ref.clone()
    got[2] = ref[2].roll(1)                                                # another arg-max in one row of five
    assert not bs.row_figures("resnet", "f16", got, ref)["ok"] and bs.row_figures("resnet", "f16", got, ref)["figures"]["agree"] == (0.8, 0.99)
    got = ref.clone()
    got[1, 0] = float("nan")
    nan = bs.row_figures("resnet", "f16x3", got, ref)
    assert not nan["ok"] and nan["row"] == 1 and nan["err"] == float("inf")


def test_row_figures_of_masks():
    ref = torch.linspace(-2, 2, 3 * 64 * 64).reshape(3, 1, 64, 64)
    assert bs.row_figures("unet", "f32", ref + 5e-5, ref)["figures"]["iou"] == (1.0, 0.9999)
    got = ref.clone()
    got[2, 0, :2] = -got[2, 0, :2]                                         # 128 pixels of the last image change side
    bad = bs.row_figures("unet", "f16", got, ref)
    assert not bad["ok"] and bad["row"] == 2 and bad["figures"]["iou"][0] < 0.995 and set(bad["figures"]) == {"logit", "prob", "iou"}
    empty = -torch.ones(1, 1, 8, 8)
    assert bs.row_figures("unet", "f32", empty, empty)["figures"]["iou"] == (1.0, 0.9999)      # two empty masks are identical


def test_u8_figures():
    logits = torch.linspace(-1, 1, 26).reshape(2, 13)
    assert bs.u8_figures(torch.softmax(logits, 1), logits)["ok"]
    bad = bs.u8_figures(torch.softmax(logits, 1) + torch.tensor([[0.0], [3e-6]]), logits)
    assert not bad["ok"] and bad["row"] == 1 and bad["bar"] == 1e-6


# ---- the replacement cap ----------------------------------------------------------------------------------------------------------------
def test_replacement_cap():
    assert bs.screen_pool(lambda rep: [], 2) == {}
    assert bs.screen_pool(lambda rep: [j for j in (3, 9) if rep.get(j, 0) < 1], 2) == {3: 1, 9: 1}
    assert bs.screen_pool(lambda rep: [4] if rep.get(4, 0) < 2 else [], 2) == {4: 2}              # one slot, two seeds: one replacement
    with pytest.raises(AssertionError, match="at most 2 may be replaced"):
        bs.screen_pool(lambda rep: [j for j in (1, 2, 3) if j not in rep], 2)
    with pytest.raises(AssertionError, match="at most 8 may be replaced"):
        bs.screen_pool(lambda rep: [j for j in range(9) if j not in rep], 8)
    with pytest.raises(AssertionError, match="still over the bar"):
        bs.screen_pool(lambda rep: [0], 2)
    assert (bs.UNET_MAX_REPLACED, bs.RESNET_MAX_REPLACED) == (2, 8)


# ---- the report -------------------------------------------------------------------------------------------------------------------------
def test_render(tmp_path):
    def res(n, stage, ratio, ok=True, last=False):
        return {"n": n, "stage": stage, "ok": ok, "ratio": ratio, "metric": "logit", "row": 0, "pool": 3, "last_row": last, "err": ratio * 1e-3, "bar": 1e-3}
    rec = {"model": "unet", "prec": "f16x3", "variant": "convT", "census": {"1": [list(p) for p in B], "2": [list(p) for p in A], "3": [list(p) for p in A]},
           "results": [res(1, "three forwards", 0.05), res(2, "three forwards", 0.04), res(3, "profiled forward", 0.07, last=True)],
           "replaced": {}, "seconds": {"three forwards": 2.5, "profiled forward": 1.25}, "thinned": False}
    rec2 = dict(rec, model="resnet18", prec="f16", variant="", replaced={"120": 1}, results=[res(1, "u8 entry", 1.5, ok=False)])
    text = bs.render([rec, rec2])
    assert "## unet f16x3 convT" in text and "## resnet18 f16\n" in text
    assert "| 0 | 1 | 0.050 | logit | 1 | three forwards | no | yes |" in text
    assert "| 1 | 2-3 | 0.070 | logit | 3 | profiled forward | yes | yes |" in text
    assert "* `l1`: `k<64,splitK3>` -> `k<64>`" in text
    assert "three forwards 2.5 s, profiled forward 1.2 s" in text or "profiled forward 1.3 s" in text
    assert "Replaced pool inputs: none." in text and "Replaced pool inputs: slot 120 (1x)." in text
    assert "| 0 | 1 | 1.500 | logit | 1 | u8 entry | no | NO |" in text and "| 1 | 2-3 | - | - | - | - | - | not run |" in text
    path = tmp_path / "r.jsonl"
    import json
    path.write_text(json.dumps(dict(rec, seconds={})) + "\n" + json.dumps(rec2) + "\n" + json.dumps(rec) + "\n")
    assert bs.render(bs.load_records(path)) == bs.render([rec, rec2])       # the last record of a parameter wins, first-seen order

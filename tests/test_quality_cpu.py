"""Board-extraction quality scores, the parts that need no GPU: the native host functions (mask completeness, quadrangle regularity,
the record -> score formulas), the ``chessvision.quality`` module and the API surface, against the independent oracle
``tests/quality_ref.py``."""
from __future__ import annotations

import inspect
import math

import numpy as np
import pytest

import quality_ref
import ragged
from chessvision import ChessVision, hip_backend, quality
from chessvision.cv_types import BoardExtractionResult, ChessVisionResult, ExtractionQuality


def _check_completeness(masks, max_tie_share):
    """C++ against the oracle; both sides divide the same two integers.  Which of two outer contours with EQUAL largest area is
    chosen is not pinned, so a mask with such a tie may disagree -- and only such a mask, and only a small share of the set."""
    masks = list(masks)
    left_out, lo, hi = 0, math.inf, -math.inf
    for m in masks:
        want, tie = quality_ref.mask_completeness_binary(m)
        got = hip_backend.mask_completeness(m)
        if tie and got != pytest.approx(want, rel=1e-12, abs=0):
            left_out += 1
            continue
        assert got == pytest.approx(want, rel=1e-12, abs=0), (got, want)
        lo, hi = min(lo, want), max(hi, want)
    assert left_out <= max_tie_share * len(masks), (left_out, len(masks))
    return lo, hi


def test_completeness_matches_the_oracle_on_label_masks():
    lo, hi = _check_completeness(ragged.label_masks(), 0.01)
    assert 0.9 < lo <= hi < 1.1


def test_completeness_matches_the_oracle_on_ragged_masks():
    _check_completeness((m for m, _, _ in ragged.ragged_set(400)), 0.01)


def test_completeness_matches_the_oracle_on_random_masks():
    rng = np.random.default_rng(7)
    masks = []
    for t in range(200):
        h, w = (int(v) for v in rng.integers(5, 41, 2))
        masks.append(((rng.random((h, w)) < 0.1 + 0.8 * (t % 9) / 8) * 255).astype(np.uint8))
    _check_completeness(masks, 0.05)


def test_completeness_edge_masks():
    assert hip_backend.mask_completeness(np.zeros((12, 9), np.uint8)) == 0.0
    assert hip_backend.mask_completeness(np.full((12, 9), 255, np.uint8)) == 1.0
    one = np.zeros((12, 9), np.uint8)
    one[5, 3] = 1
    assert hip_backend.mask_completeness(one) == quality_ref.mask_completeness_binary(one)[0] == 1.0
    ring = np.zeros((70, 70), np.uint8)                      # a ring across a 64-bit word boundary with a speck inside and one outside
    ring[3:68, 2:69] = 255
    ring[10:60, 9:66] = 0
    ring[30, 30] = ring[0, 0] = 255
    want = (65 * 67 - 50 * 57 + 2) / (65 * 67)
    assert quality_ref.mask_completeness_binary(ring)[0] == want
    assert hip_backend.mask_completeness(ring) == want


def test_completeness_batch_equals_single():
    masks = np.stack([m for m, _, _ in ragged.ragged_set(40)])
    single = np.array([hip_backend.mask_completeness(m) for m in masks])
    assert np.array_equal(hip_backend.mask_completenesses(masks, n_threads=4), single)
    assert np.array_equal(hip_backend.mask_completenesses(masks, n_threads=1), single)
    assert hip_backend.mask_completenesses(masks[:0]).shape == (0,)


def test_regularity_of_squares_and_missing_quadrangle():
    assert hip_backend.quadrangle_regularity(None) == 0.0
    assert quality.quadrangle_regularity(None) == 0.0
    square = np.array([[[200, 10]], [[10, 10]], [[10, 200]], [[200, 200]]], dtype=np.float32)
    diamond = np.array([[[100, 0]], [[0, 100]], [[100, 200]], [[200, 100]]], dtype=np.int32)
    assert quality.quadrangle_regularity(square) == pytest.approx(1.0, abs=1e-6)
    assert quality.quadrangle_regularity(diamond) == pytest.approx(1.0, abs=1e-6)
    assert hip_backend.quadrangle_regularity(square.reshape(4, 2)) == pytest.approx(1.0, abs=1e-6)


def test_regularity_matches_the_float32_literal_on_random_convex_quadrangles():
    """Bar 1e-5 absolute: the literal computes in float32 (a few 1e-7 relative per operation, acos well conditioned for angles in
    30..150 degrees), the product in double."""
    rng = np.random.default_rng(11)
    done = 0
    while done < 200:
        # a vertex in each quadrant around a centre: convex when every interior angle stays below 180 degrees
        r = rng.uniform(30, 120, 4)
        phi = np.deg2rad(np.array([45, 135, 225, 315]) + rng.uniform(-35, 35, 4))
        q = (np.stack([128 + r * np.cos(phi), 128 + r * np.sin(phi)], axis=1)).astype(np.float32).reshape(4, 1, 2)
        p = q.reshape(4, 2).astype(np.float64)
        ang = []
        cross = []
        for i in range(4):
            a, b = p[i - 1] - p[i], p[(i + 1) % 4] - p[i]
            ang.append(np.degrees(np.arccos(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))))
            cross.append(a[0] * b[1] - a[1] * b[0])
        if not (all(30 <= v <= 150 for v in ang) and (all(c > 0 for c in cross) or all(c < 0 for c in cross))):
            continue
        done += 1
        assert quality.quadrangle_regularity(q) == pytest.approx(quality_ref.quadrangle_regularity(q), abs=1e-5)


def test_regularity_with_a_repeated_vertex_takes_the_zero_norm_branch():
    q = np.array([[[10, 10]], [[10, 10]], [[90, 20]], [[40, 80]]], dtype=np.float32)
    want = quality_ref.quadrangle_regularity(q)
    assert math.isfinite(want)
    assert quality.quadrangle_regularity(q) == pytest.approx(want, abs=1e-5)
    point = np.zeros((4, 1, 2), np.float32) + 7                 # all four coincide: side term 1, angle term 0
    assert quality.quadrangle_regularity(point) == quality_ref.quadrangle_regularity(point) == 0.5


def _arrays():
    rng = np.random.default_rng(3)
    edges = np.arange(11, dtype=np.float64) / 10
    near = []
    for e in list(edges) + [0.5]:
        v = np.float32(e)
        lo = hi = v
        near.append(v)
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
            near += [lo, hi]
    yield "normal", rng.normal(0, 6, (64, 64)).astype(np.float32)
    yield "uniform+edges", np.concatenate([rng.random(5000).astype(np.float32), np.array(near, np.float32)])
    yield "constant", np.full(1000, 0.7, np.float32)
    yield "negative", -rng.random(777).astype(np.float32) - 1
    yield "zeros+inf", np.array([0.0, -0.0, np.inf, -np.inf, 0.3, 1.0, 0.5, -0.0, 0.0, 2.0, 0.9, 0.1], np.float32)
    yield "float64", rng.random((50, 50))
    yield "tiny", np.array([0.25, 0.75, 0.5, 1.0], np.float32)


@pytest.mark.parametrize("name,a", list(_arrays()), ids=[n for n, _ in _arrays()])
def test_array_scores_equal_the_literals(name, a):
    assert np.array_equal(quality._histogram10(a), quality_ref.histogram10(a))
    got_d, want_d = quality.probability_distribution(a), quality_ref.probability_distribution(a)
    assert got_d == want_d or (math.isnan(got_d) and math.isnan(want_d))
    assert quality.probability_confidence(a) == quality_ref.probability_confidence(a)
    m = a.reshape(-1, 1) if a.ndim == 1 else a
    assert quality.mask_completeness(m) == pytest.approx(quality_ref.mask_completeness(m), rel=1e-12)


def test_scores_of_special_arrays():
    nothing = np.array([-1.0, 2.0, np.nan, np.inf, 7.0], np.float32)
    assert math.isnan(quality.probability_distribution(nothing)) and math.isnan(quality_ref.probability_distribution(nothing))
    with_nan = np.array([0.1, 0.9, np.nan, 0.3, 0.2, 0.8, 0.6, 0.4], np.float32)
    assert math.isnan(quality.probability_confidence(with_nan)) and math.isnan(quality_ref.probability_confidence(with_nan))


def test_finish_formulas_from_hand_made_records():
    """distribution = 1 - H / log2(10), H = -sum p log2(p + 1e-10).  The 1e-10 inside the logarithm is part of the formula, so a one-bin
    histogram scores 1 + log2(1 + 1e-10) / log2(10) (4.3e-11 above 1) and a uniform one 1 + log2(0.1 + 1e-10) / log2(10) (4.3e-10):
    the exact values are asserted to 1e-12, and that they are 1 and 0 to 1e-9."""
    rec = np.zeros(5, dtype=hip_backend.SCORE_RECORD)
    rec["hist"][0, 6] = 65536
    rec["hist"][1] = 4096
    rec["hist"][2, :2] = (100, 300)
    rec["top_count"] = (16384, 10240, 100, 7, 3)
    rec["top_sum"] = (16384 * 0.25, 1.0, 12.5, 0.0, 1.5)
    rec["n_nan"][4] = 1
    conf, dist = hip_backend.scores_finish(rec)
    assert dist[0] == pytest.approx(1.0 + math.log2(1 + 1e-10) / math.log2(10), abs=1e-12) and abs(dist[0] - 1.0) < 1e-9
    assert dist[1] == pytest.approx(1.0 + math.log2(0.1 + 1e-10) / math.log2(10), abs=1e-12) and abs(dist[1]) < 1e-9
    p = np.array([0.25, 0.75])
    assert dist[2] == pytest.approx(1.0 + float(np.sum(p * np.log2(p + 1e-10))) / math.log2(10), abs=1e-12)
    assert math.isnan(dist[3]) and math.isnan(dist[4])                   # empty histograms: 0 / 0
    assert conf[0] == 0.5 and conf[1] == 2.0 / 10240 and conf[2] == 0.25 and conf[3] == 0.0
    assert math.isnan(conf[4])                                           # a NaN in the image


def test_finish_matches_the_literal_for_a_real_histogram():
    a = np.random.default_rng(5).random(65536).astype(np.float32) ** 3
    rec = np.zeros(1, dtype=hip_backend.SCORE_RECORD)
    rec["hist"][0] = quality_ref.histogram10(a)
    k = a.size // 4
    rec["top_count"] = k
    rec["top_sum"] = np.abs(np.sort(a)[-k:] - np.float32(0.5)).astype(np.float64).sum()
    conf, dist = hip_backend.scores_finish(rec)
    assert dist[0] == pytest.approx(quality_ref.probability_distribution(a), abs=1e-12)
    assert conf[0] == pytest.approx(quality_ref.probability_confidence_f64(a), rel=1e-12)


def test_extraction_quality_on_the_host():
    yy, xx = np.mgrid[:256, :256]
    depth = np.minimum(80 - np.abs(yy - 128), 85 - np.abs(xx - 120))          # pixels inside (+) / outside (-) a rectangle
    logits = (6.5 * np.tanh(depth / 3.0) + np.random.default_rng(2).normal(0, 0.3, (256, 256))).astype(np.float32)
    mask = ((logits > 0) * 255).astype(np.uint8)
    ext = BoardExtractionResult(probabilities=logits, binary_mask=mask, quadrangle=None, board_image=None)
    for of in ("logits", "sigmoid"):
        v = logits if of == "logits" else quality_ref.sigmoid64(logits).astype(np.float32)
        q = quality.extraction_quality(ext, of=of)
        assert isinstance(q, ExtractionQuality)
        assert q.completeness == pytest.approx(quality_ref.mask_completeness(v), rel=1e-12)
        assert q.quad_score == pytest.approx(quality_ref.quadrangle_regularity(
            np.asarray(hip_backend.find_quadrangle(mask), dtype=np.float32)), abs=1e-5)
        assert 0.9 < q.quad_score <= 1.0
        if of == "logits":
            assert q.confidence == quality_ref.probability_confidence(v) and q.distribution == quality_ref.probability_distribution(v)
        else:
            assert q.confidence == pytest.approx(quality_ref.probability_confidence(v), abs=1e-5)
    with pytest.raises(ValueError):
        quality.extraction_quality(ext, of="probabilities")
    blank = BoardExtractionResult(probabilities=logits, binary_mask=np.zeros((256, 256), np.uint8), quadrangle=None, board_image=None)
    assert quality.extraction_quality(blank).quad_score == 0.0


def test_api_surface():
    ext = BoardExtractionResult(probabilities=np.zeros((256, 256), np.float32), binary_mask=np.zeros((256, 256), np.uint8),
                                quadrangle=None, board_image=None)
    res = ChessVisionResult(ext, None, 0.25)
    assert res.quality is None and res.processing_time == 0.25
    assert [f for f in ChessVisionResult.__dataclass_fields__][-1] == "quality"
    assert list(ExtractionQuality.__dataclass_fields__) == ["confidence", "quad_score", "completeness", "distribution"]
    param = inspect.signature(ChessVision.process_images).parameters["quality"]
    assert param.default is None
    names = {name for name, _, _ in hip_backend.SYMBOLS}
    assert {"cv_extraction_scores", "cv_extraction_scores_finish", "cv_mask_completeness", "cv_mask_completenesses",
            "cv_quadrangle_regularity"} <= names
    assert hip_backend.SCORE_RECORD.itemsize == 64

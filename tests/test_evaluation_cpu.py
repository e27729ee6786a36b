"""Ground-truth scores without a GPU: the reference's known answers for labels and top-k, the native per-square scores against the
Python form and the loop oracle (``tests/evaluation_ref.py``), FEN parsing, the finish step of the segmentation records, the numpy
segmentation scores against the torch expression of the reference's LossCollector, the aggregate record and the API surface."""
from __future__ import annotations

import ctypes
import inspect
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import evaluation_ref as ref
from chessvision import ChessVision, constants, evaluation, hip_backend
from chessvision.cv_types import ChessVisionResult

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR"
EMPTY = "8/8/8/8/8/8/8/8"
IDX = constants.LABEL_INDICES
PHOTOS = [Path(__file__).resolve().parent / "golden" / f"photos8_{i}.npz" for i in range(8)]
MALFORMED = ["", "8/8/8/8/8/8/8", "8/8/8/8/8/8/8/8/8", "9/8/8/8/8/8/8/8", "7/8/8/8/8/8/8/8", "rnbqkbnr/ppppppppp/8/8/8/8/8/8",
             "8/8/8/8/8/8/8/7x", "8/8/8/8/8/8/8/7f", "8/8/8/8/8/8/8/44P", "8/8/8/8/8/8/8/80", "8/8/8/8/8/8/8/"]


# ---- the reference's own known answers (its tests/test_metrics.py), inputs rebuilt from their description -----------------------------
def test_board_to_labels_known_answers():
    labels = evaluation.board_to_labels(START + " w KQkq - 0 1")
    assert labels[:8] == list("rnbqkbnr") and labels[8:16] == ["p"] * 8 and labels[16:48] == ["f"] * 32
    assert labels[48:56] == ["P"] * 8 and labels[56:] == list("RNBQKBNR")
    assert evaluation.board_to_labels(EMPTY) == ["f"] * 64
    lone = evaluation.board_to_labels("8/8/8/8/4Q3/8/8/8")
    assert lone[36] == "Q" and sum(1 for s in lone if s != "f") == 1          # e4: fifth rank from the top, fifth file


def test_topk_known_answers():
    p = np.zeros((64, 13), np.float32)
    p[:32, IDX["f"]] = 1.0
    p[32:48, IDX["p"]], p[32:48, IDX["f"]] = 1.0, 0.9
    p[48:, IDX["P"]], p[48:, IDX["p"]], p[48:, IDX["f"]] = 1.0, 0.9, 0.8
    res = evaluation.compute_model_topk_accuracy(p, EMPTY, k=3)
    assert isinstance(res, evaluation.TopKAccuracyResult) and res.k == 3 and len(res.accuracies) == 3
    assert (res.top_1, res.top_2, res.top_3) == (0.5, 0.75, 1.0)


def test_topk_variable_k_known_answers():
    fen = "8/8/8/8/8/8/PPPPPPPP/8"
    p = np.zeros((64, 13), np.float32)
    p[:, IDX["f"]] = 1.0
    p[48:56, IDX["f"]], p[48:56, IDX["P"]] = 0.0, 1.0
    k1 = evaluation.compute_model_topk_accuracy(p, fen, k=1)
    assert k1.k == 1 and len(k1.accuracies) == 1 and k1.top_1 == 1.0 and k1.top_2 == 0.0
    k5 = evaluation.compute_model_topk_accuracy(p, fen, k=5)
    assert k5.k == 5 and len(k5.accuracies) == 5 and all(a == 1.0 for a in k5.accuracies)


def test_topk_with_overwritten_triples_known_answer():
    """0.9 / 0.8 / 0.7 triples written in the reference's order, so a later write of the same class overwrites an earlier one
    (e.g. the true queen on d8: q = 0.8 becomes 0.7): 40, 57 and 64 squares of 64."""
    labels = evaluation.board_to_labels(START)
    p = np.zeros((64, 13), np.float32)
    for sq, label in enumerate(labels):
        if sq < 8:
            order = [("p", 0.9), ("q", 0.8), (label, 0.7)]
        elif sq >= 56:
            order = [("P", 0.9), (label, 0.8), ("Q", 0.7)]
        else:
            order = [(label, 0.9), ("f", 0.8), ("p", 0.7)]
        for sym, v in order:
            p[sq, IDX[sym]] = v
    res = evaluation.compute_model_topk_accuracy(p, START, k=3)
    assert abs(res.top_1 - 40 / 64) < 1e-6 and abs(res.top_2 - 57 / 64) < 1e-6 and abs(res.top_3 - 64 / 64) < 1e-6


# ---- native per-square scores == Python form == loop oracle ------------------------------------------------------------------------
def _check_boards(probs, labels, fens=None):
    per_square, per_board = hip_backend.classification_scores(probs, labels)
    assert per_square.shape == (len(probs), 64) and per_board.shape == (len(probs),)
    for b in range(len(probs)):
        want = ref.board_scores(probs[b], labels[b])
        sq = per_square[b]
        assert sq["rank"].tolist() == want["rank"] and sq["predicted"].tolist() == want["predicted"]
        assert per_board["hits"][b].tolist() == want["hits"] and per_board["n_nan"][b] == want["n_nan"]
        np.testing.assert_array_equal(sq["confidence"], np.array(want["confidence"], np.float32))
        np.testing.assert_allclose(sq["loss"], np.array(want["loss"]), rtol=0, atol=1e-12)
        if math.isnan(want["mean_loss"]) or math.isinf(want["mean_loss"]):
            assert np.array_equal(per_board["mean_loss"][b], want["mean_loss"], equal_nan=True)
        else:
            assert abs(per_board["mean_loss"][b] - want["mean_loss"]) <= 1e-12
        # the Python form
        assert evaluation.true_class_ranks(probs[b], labels[b]).tolist() == want["rank"]
        if fens is not None:
            py = evaluation.position_scores(probs[b], fens[b], fens[b], fens[b])
            assert py.rank.tolist() == want["rank"] and py.predicted_labels.tolist() == want["predicted"]
            assert py.top_k == tuple(h / 64 for h in want["hits"][:3])
            np.testing.assert_allclose(py.loss, np.array(want["loss"]), rtol=0, atol=1e-12)
            np.testing.assert_array_equal(py.confidence, np.array(want["confidence"], np.float32))
            assert np.array_equal(py.mean_loss, want["mean_loss"], equal_nan=True) or abs(py.mean_loss - want["mean_loss"]) <= 1e-12
            topk = evaluation.compute_model_topk_accuracy(probs[b], fens[b], k=13)
            assert list(topk.accuracies) == [h / 64 for h in want["hits"]]
    return per_square, per_board


def _random_fen(rng):
    rows = []
    for _ in range(8):
        row, empty = "", 0
        for _ in range(8):
            c = int(rng.integers(0, 13)) if rng.random() < 0.5 else 12
            if c == 12:
                empty += 1
                continue
            row += (str(empty) if empty else "") + constants.LABEL_NAMES[c]
            empty = 0
        rows.append(row + (str(empty) if empty else ""))
    return "/".join(rows)


def test_classification_scores_on_random_boards_without_ties():
    rng = np.random.default_rng(5)
    fens = [_random_fen(rng) for _ in range(200)]
    labels = np.array([ref.fen_indices(f) for f in fens], np.int8)
    logits = rng.normal(0, 3, (200, 64, 13))
    probs = torch.softmax(torch.from_numpy(logits).float(), dim=-1).numpy()
    assert all(len(set(row.tolist())) == 13 for row in probs.reshape(-1, 13))                  # no ties
    _check_boards(probs, labels, fens)


def test_classification_scores_with_planted_ties_follow_the_stable_argsort():
    rng = np.random.default_rng(6)
    probs = rng.choice(np.array([0.0, 0.125, 0.25, 0.5], np.float32), (12, 64, 13))            # most rows tie at several levels
    probs[0] = 0.0                                                                             # all equal: rank = 12 - t
    probs[1] = 1.0 / 13
    labels = rng.integers(0, 13, (12, 64)).astype(np.int8)
    per_square, _ = _check_boards(probs, labels)
    for b in range(12):
        for i in range(64):
            assert per_square["rank"][b, i] == ref.rank_by_stable_argsort(probs[b, i], int(labels[b, i]))
    assert per_square["rank"][0].tolist() == [12 - int(t) for t in labels[0]]
    assert np.isinf(per_square["loss"][0]).all() and (per_square["loss"][0] > 0).all()         # -log(0) = +inf


def test_classification_scores_with_nan_squares():
    rng = np.random.default_rng(7)
    probs = torch.softmax(torch.from_numpy(rng.normal(0, 3, (3, 64, 13))).float(), dim=-1).numpy()
    labels = rng.integers(0, 13, (3, 64)).astype(np.int8)
    probs[0, 5, int(labels[0, 5])] = np.nan              # the true class itself
    probs[0, 9, (int(labels[0, 9]) + 1) % 13] = np.nan   # another class
    probs[2, 63] = np.nan                                # a whole row
    per_square, per_board = _check_boards(probs, labels)
    assert per_board["n_nan"].tolist() == [2, 0, 1]
    assert per_square["rank"][0, 5] == per_square["rank"][0, 9] == per_square["rank"][2, 63] == 13
    assert math.isnan(per_board["mean_loss"][0]) and math.isfinite(per_board["mean_loss"][1])
    assert math.isfinite(per_square["loss"][0, 9]) and math.isnan(per_square["confidence"][0, 9])
    assert per_board["hits"][0, 12] == 62                # a NaN square misses at every k


def test_classification_scores_argument_errors():
    lib = hip_backend.load_library()
    probs, labels = np.zeros((1, 64, 13), np.float32), np.zeros((1, 64), np.int8)
    labels[0, 3] = 13
    with pytest.raises(hip_backend.HipBackendError, match="label 3"):
        hip_backend.classification_scores(probs, labels)
    with pytest.raises(hip_backend.HipBackendError):
        hip_backend.classification_scores(probs[:, :63], labels[:, :63])
    assert lib.cv_classification_scores(None, None, 1, None, None) == 1
    assert hip_backend.classification_scores(probs[:0], labels[:0])[1].shape == (0,)


# ---- FEN labels and position accuracy ------------------------------------------------------------------------------------------------
def test_fen_labels_on_the_ground_truth_fens_and_on_malformed_ones():
    fens = [str(np.load(p)["fen"][0]) for p in PHOTOS]
    assert len(set(fens)) >= 2
    for fen in fens + [START, EMPTY, START + " w KQkq - 0 1", "8/8/8/8/4Q3/8/8/8 b - - 3 9"]:
        got = hip_backend.fen_labels(fen)
        assert got.dtype == np.int8 and got.tolist() == ref.fen_indices(fen)
        assert [constants.LABEL_NAMES[k] for k in got] == evaluation.board_to_labels(fen)
        assert evaluation.label_indices(fen).tolist() == got.tolist()
    lib = hip_backend.load_library()
    for bad in MALFORMED:
        out = np.full(64, -7, np.int8)
        assert lib.cv_fen_labels(bad.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int8))) == 1, bad
        assert b"cv_fen_labels" in lib.cv_last_error() and (out == -7).all(), bad             # nothing is written on failure
        with pytest.raises(ValueError):
            evaluation.board_to_labels(bad)
        with pytest.raises(ValueError):
            ref.fen_symbols(bad)
    assert lib.cv_fen_labels(None, None) == 1


def test_compute_position_accuracy_hand_cases():
    acc = evaluation.compute_position_accuracy
    assert acc(START, START) == evaluation.PositionAccuracy(accuracy=1.0, num_correct=64, total_squares=64)
    assert acc(EMPTY, START).num_correct == 32 and acc(EMPTY, START).accuracy == 0.5
    one_off = "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR"
    assert acc(one_off, START).num_correct == 62
    assert acc(START.swapcase(), START).num_correct == 32                     # colours swapped: only the empty squares agree
    for a, b in [(one_off, START), (EMPTY, one_off), (START + " w - - 0 1", one_off)]:
        assert acc(a, b).accuracy == ref.position_accuracy(a, b)
    with pytest.raises(ValueError):
        acc("8/8", START)


# ---- finish step ---------------------------------------------------------------------------------------------------------------------
def _record(**kw):
    r = np.zeros(1, hip_backend.SEG_RECORD)
    for k, v in kw.items():
        r[k] = v
    return r


def test_segmentation_finish_on_hand_made_records():
    cases = [
        dict(n_label=3, n_pred=4, n_both=2, bce_sum=5.5, sig_sum=4.25, sig_label_sum=2.5, count=10),
        dict(n_label=0, n_pred=0, n_both=0, bce_sum=0.125, sig_sum=0.75, sig_label_sum=0.0, count=16),        # both empty
        dict(n_label=0, n_pred=0, n_both=0, bce_sum=0.0, sig_sum=0.0, sig_label_sum=0.0, count=4),            # S == 0
        dict(n_label=65536, n_pred=65536, n_both=65536, bce_sum=1e-3, sig_sum=65535.5, sig_label_sum=65535.5, count=65536),
        dict(n_label=7, n_pred=5, n_both=0, bce_sum=812.0, sig_sum=5.0, sig_label_sum=1e-9, count=100),
        dict(n_label=2, n_pred=1, n_both=1, n_nan=1, bce_sum=math.nan, sig_sum=math.nan, sig_label_sum=math.nan, count=9),
    ]
    records = np.concatenate([_record(**c) for c in cases])
    got = hip_backend.segmentation_scores_finish(records)
    assert set(got) == {"bce", "dice_loss", "loss", "dice", "iou", "pixel_accuracy"}
    for i, c in enumerate(cases):
        want = ref.seg_finish({**c})
        for key, w in want.items():
            g = float(got[key][i])
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-15 * max(1.0, abs(w)), (i, key, g, w)
    assert got["dice"][1] == 1.0 and got["iou"][1] == 1.0 and got["pixel_accuracy"][1] == 1.0
    assert got["dice_loss"][2] == 0.0 and got["loss"][2] == 0.0                                 # S == 0: soft Dice is 1
    assert got["iou"][4] == 0.0 and math.isnan(got["loss"][5]) and got["dice"][5] == ref.dice(1, 3)
    lib = hip_backend.load_library()
    assert lib.cv_segmentation_scores_finish(None, 1, None, None, None, None, None, None) == 1
    bad = _record(count=0)
    with pytest.raises(hip_backend.HipBackendError, match="no pixels"):
        hip_backend.segmentation_scores_finish(bad)


# ---- numpy scores against the LossCollector's torch expression -----------------------------------------------------------------------
def test_numpy_segmentation_scores_match_the_torch_expression():
    """BCEWithLogitsLoss(reduction="none").mean((-1,-2)) + 1 - dice_coeff(sigmoid(x), t) on CPU in float32; 1e-6 relative (the
    float32-to-float64 gap measured on 4 x 65536 normal(0,6) logits is 1.2e-7)."""
    rng = np.random.default_rng(11)
    logits = rng.normal(0, 6, (4, 256, 256)).astype(np.float32)
    masks = np.where(rng.random((4, 256, 256)) < 0.4, 255, 0).astype(np.uint8)
    masks[3] = 0
    x, t = torch.from_numpy(logits), torch.from_numpy(masks / 255.0).float()
    bce = torch.nn.BCEWithLogitsLoss(reduction="none")(x, t).mean((-1, -2))
    s = torch.sigmoid(x)
    inter, sets_sum = 2 * (s * t).sum((-1, -2)), s.sum((-1, -2)) + t.sum((-1, -2))
    sets_sum = torch.where(sets_sum == 0, inter, sets_sum)
    want = (1 - (inter + 1e-6) / (sets_sum + 1e-6)) + bce
    for i in range(4):
        got = evaluation.segmentation_scores(logits[i], masks[i])
        assert abs(got.loss - float(want[i])) <= 1e-6 * abs(float(want[i])), (i, got.loss, float(want[i]))
        assert abs(got.bce - float(bce[i])) <= 1e-6 * float(bce[i])
        oracle = ref.seg_scores(logits[i], masks[i])
        for key, w in oracle.items():
            assert abs(getattr(got, key) - w) <= 1e-12 * max(1.0, abs(w)), (i, key)
        hard = (s[i] > 0.5).numpy()
        assert got.pixel_accuracy == float(np.mean(hard == (masks[i] != 0)))
    empty = evaluation.segmentation_scores(np.full((256, 256), -40.0, np.float32), np.zeros((256, 256), np.uint8))
    assert empty.dice == 1.0 and empty.iou == 1.0 and empty.pixel_accuracy == 1.0
    with_nan = logits[0].copy()
    with_nan[3, 3] = np.nan
    got = evaluation.segmentation_scores(with_nan, masks[0])
    assert math.isnan(got.loss) and math.isnan(got.bce) and math.isnan(got.dice_loss) and math.isfinite(got.dice)


# ---- aggregate -------------------------------------------------------------------------------------------------------------------------
def _pos(orig, valid, top2, top3, fixes):
    z = np.zeros(64)
    return evaluation.PositionScores(top_k=(orig, top2, top3), accuracy_original=orig, accuracy_validated=valid, mean_loss=1.0,
                                     num_fixes=fixes, true_labels=z, predicted_labels=z, validated_labels=z, rank=z, confidence=z, loss=z)


def _seg(loss, dice, iou):
    return evaluation.SegmentationScores(bce=0.0, dice_loss=loss, loss=loss, dice=dice, iou=iou, pixel_accuracy=1.0)


def test_aggregate_from_hand_made_records():
    E = evaluation.ImageEvaluation
    evs = [E(_seg(0.5, 0.75, 0.5), _pos(0.5, 0.75, 0.875, 1.0, 3), False),
           E(None, _pos(1.0, 1.0, 1.0, 1.0, 0), False),
           E(_seg(0.25, 0.25, 1.0), None, True),                       # FEN given, no board found
           E(None, _pos(0.25, 0.125, 0.5, 0.75, 2), False),            # the rule made it worse: no improvement
           E(_seg(0.75, 0.5, 0.0), None, False)]                       # no FEN given: neither scored nor a failure
    agg = evaluation.aggregate(evs, [0.1, 0.2, 0.3, 0.4, 0.5])
    assert set(evaluation.AGGREGATE_KEYS) <= set(agg) and {"mean_loss", "mean_dice", "mean_iou"} <= set(agg)
    assert agg["top_1_accuracy_validated"] == (0.75 + 1.0 + 0.125) / 3 and agg["top_1_accuracy"] == (0.5 + 1.0 + 0.25) / 3
    assert agg["top_2_accuracy"] == (0.875 + 1.0 + 0.5) / 3 and agg["top_3_accuracy"] == (1.0 + 1.0 + 0.75) / 3
    assert agg["validation_fixes"] == 5 and agg["validation_improvements"] == 1 and agg["extraction_failures"] == 1
    assert agg["avg_time_per_prediction"] == sum([0.1, 0.2, 0.3, 0.4, 0.5]) / 5
    assert agg["mean_loss"] == 0.5 and agg["mean_dice"] == 0.5 and agg["mean_iou"] == 0.5
    none = evaluation.aggregate([E(None, None, True), E(None, None, True)], [1.0, 3.0])           # zero successful extractions
    assert all(math.isnan(none[k]) for k in ("top_1_accuracy_validated", "top_1_accuracy", "top_2_accuracy", "top_3_accuracy",
                                            "mean_loss", "mean_dice", "mean_iou"))
    assert none["extraction_failures"] == 2 and none["validation_fixes"] == 0 and none["validation_improvements"] == 0
    assert none["avg_time_per_prediction"] == 2.0


# ---- evaluate_images: the argument errors that need no device ------------------------------------------------------------------------
def test_evaluate_images_argument_errors():
    cv = ChessVision()
    images = [np.zeros((64, 64, 3), np.uint8)] * 3
    good = np.zeros((256, 256), np.uint8)
    with pytest.raises(ValueError, match="ground truth"):
        cv.evaluate_images(images)
    with pytest.raises(ValueError, match="true_fens has 2"):
        cv.evaluate_images(images, true_fens=[START, None])
    with pytest.raises(ValueError, match="label_masks has 4"):
        cv.evaluate_images(images, label_masks=[good] * 4)
    with pytest.raises(ValueError, match="image 1"):
        cv.evaluate_images(images, true_fens=[START, "8/8/8/8", None])
    with pytest.raises(ValueError, match="image 2"):
        cv.evaluate_images(images, true_fens=[None, None, 17])
    with pytest.raises(ValueError, match="image 2"):
        cv.evaluate_images(images, label_masks=[good, None, np.zeros((128, 128), np.uint8)])
    with pytest.raises(ValueError, match="image 0"):
        cv.evaluate_images(images, label_masks=[good.astype(np.float32), None, None])
    with pytest.raises(ValueError, match="image 1"):
        cv.evaluate_images(images, true_fens=[START] * 3, label_masks=[good, [[0]], good])
    assert not cv._engines                                     # nothing was created, let alone queued


def test_api_surface():
    names = {name for name, _, _ in hip_backend.SYMBOLS}
    assert {"cv_segmentation_scores", "cv_segmentation_scores_finish", "cv_fen_labels", "cv_classification_scores"} <= names
    assert hip_backend.SEG_RECORD.itemsize == 64 and hip_backend.SQUARE_SCORE.itemsize == 24 and hip_backend.BOARD_SCORE.itemsize == 64
    assert hip_backend.ABI_VERSION == 6 and hip_backend.load_library().cv_abi_version() == 6
    assert list(ChessVisionResult.__dataclass_fields__) == ["board_extraction", "position", "processing_time", "quality"]
    sig = inspect.signature(ChessVision.evaluate_images)
    assert list(sig.parameters) == ["self", "images", "true_fens", "label_masks", "threshold", "flip", "fallback_quad", "pipeline_chunk",
                                    "timings"]
    assert sig.parameters["true_fens"].default is None and sig.parameters["pipeline_chunk"].default == 64
    assert list(inspect.signature(ChessVision.process_images).parameters)[-1] == "quality"
    assert list(evaluation.SegmentationScores.__dataclass_fields__) == ["bce", "dice_loss", "loss", "dice", "iou", "pixel_accuracy"]
    assert list(evaluation.ImageEvaluation.__dataclass_fields__) == ["segmentation", "position", "extraction_failed"]
    assert list(evaluation.EvaluationReport.__dataclass_fields__) == ["results", "evaluations", "aggregate"]
    assert hasattr(hip_backend.HipEngine, "segmentation_scores_dev") and hasattr(hip_backend.HipEngine, "segmentation_scores")

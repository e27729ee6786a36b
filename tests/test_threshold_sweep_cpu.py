"""CPU: the host side of ``ChessVision.evaluate_thresholds`` -- the numpy form of the levels kernel against brute force, the board
planner, argument validation before any engine is touched, the curve arithmetic, and the record layout against the header."""
from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np
import pytest

from chessvision import ChessVision, evaluation, hip_backend

ROOT = Path(__file__).resolve().parent.parent
GRID = [0.0, 0.25, 0.5, 0.5000001, 0.75, 1.0]                 # both ends of the range and two float32 neighbours


def _sigmoid32(x):
    with np.errstate(over="ignore"):
        return np.float32(1) / (np.float32(1) + np.exp(-np.asarray(x, np.float32)))


# ---- threshold_levels ------------------------------------------------------------------------------------------------------------------
def test_numpy_levels_against_brute_force():
    rng = np.random.default_rng(5)
    thr = np.asarray(GRID, np.float32)
    assert thr[2] < thr[3]                                    # the neighbours are distinct as float32
    x = rng.normal(0, 3, (3, 37, 41)).astype(np.float32)
    x[0, 0, :6] = [0.0, np.inf, -np.inf, np.nan, 1e-7, -1e-7]  # sigmoid exactly 0.5, 1, 0; NaN; the two sides of 0.5
    lab = np.array([0, 1, 7, 255], np.uint8)[rng.integers(0, 4, x.shape)]
    levels, hist, n_nan = evaluation.threshold_levels(x, thr, lab)
    assert levels.shape == x.shape and levels.dtype == np.uint8 and hist.shape == (3, 2, 33) and n_nan.tolist() == [1, 0, 0]
    assert levels[0, 0, 3] == 0                               # the NaN
    v = _sigmoid32(x)
    for k, t in enumerate(thr):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(levels > k, v > t), k
    n_label, n_pred, n_both = evaluation.level_counts(hist, len(thr))
    for i in range(3):
        assert hist[i].sum() == x[i].size and not hist[i, :, len(thr) + 1:].any()
        assert n_label[i] == np.count_nonzero(lab[i])
        for k, t in enumerate(thr):
            with np.errstate(invalid="ignore"):
                pred = v[i] > t
            assert n_pred[i, k] == pred.sum() and n_both[i, k] == (pred & (lab[i] != 0)).sum()
    # without labels every pixel counts under b = 0
    levels2, hist2, _ = evaluation.threshold_levels(x, thr)
    assert np.array_equal(levels2, levels) and not hist2[:, 1].any() and np.array_equal(hist2[:, 0], hist.sum(axis=1))


def test_level_counts_give_the_scores_of_segmentation_scores_exactly():
    """Dice / IoU / pixel accuracy from the histogram's suffix sums, through the native finish, equal the single-threshold host form."""
    rng = np.random.default_rng(6)
    thr = np.asarray(GRID, np.float32)
    x = rng.normal(0, 2, (2, 50, 30)).astype(np.float32)
    x[1] -= 9                                                 # an almost empty prediction
    lab = np.where(rng.random(x.shape) < 0.4, 255, 0).astype(np.uint8)
    _, hist, n_nan = evaluation.threshold_levels(x, thr, lab)
    rec = np.zeros(2, hip_backend.LEVEL_RECORD)
    rec["count"], rec["n_thresholds"], rec["n_nan"], rec["hist"] = 1500, len(thr), n_nan, hist
    fin = hip_backend.threshold_levels_finish(rec)
    assert fin["dice"].shape == (2, len(thr))
    for i in range(2):
        for k, t in enumerate(thr):
            want = evaluation.segmentation_scores(x[i], lab[i], float(t))
            assert (fin["dice"][i, k], fin["iou"][i, k], fin["pixel_accuracy"][i, k]) == (want.dice, want.iou, want.pixel_accuracy), (i, k)
    none = hip_backend.threshold_levels_finish(rec, labels_present=False)
    empty = evaluation.segmentation_scores(x[0], np.zeros_like(lab[0]), 0.5)
    assert (none["dice"][0, 2], none["iou"][0, 2], none["pixel_accuracy"][0, 2]) == (empty.dice, empty.iou, empty.pixel_accuracy)
    bad = rec.copy()
    bad["n_thresholds"][1] = 3
    with pytest.raises(hip_backend.HipBackendError, match="cv_threshold_levels_finish"):
        hip_backend.threshold_levels_finish(bad)


def test_numpy_levels_refuse_a_bad_grid():
    x = np.zeros((1, 8), np.float32)
    for thr in ([], [0.5, 0.5], [0.7, 0.3], [-0.1], [1.5], [math.nan], list(np.linspace(0, 1, 33))):
        with pytest.raises(ValueError):
            evaluation.threshold_levels(x, thr)
    with pytest.raises(ValueError):
        evaluation.threshold_levels(x, [0.5], np.zeros((1, 7), np.uint8))


# ---- plan_threshold_groups -------------------------------------------------------------------------------------------------------------
def _quad(seed):
    return (np.arange(8, dtype=np.int32).reshape(4, 1, 2) + seed).astype(np.int32)


def test_plan_all_thresholds_agree():
    quads = [[_quad(10), _quad(20), _quad(30)] for _ in range(3)]          # equal bytes, different objects
    distinct, use, groups = evaluation.plan_threshold_groups(quads)
    assert [len(d) for d in distinct] == [1, 1, 1] and use == [[0, 0, 0]] * 3
    assert len(groups) == 1 and [i for i, _ in groups[0]] == [0, 1, 2]
    assert sum(len(d) for d in distinct) == 3                              # boards_classified == n
    assert np.array_equal(groups[0][1][1], _quad(20))


def test_plan_all_distinct_and_order_of_first_appearance():
    quads = [[_quad(1), _quad(5)], [_quad(2), _quad(6)], [_quad(1), _quad(7)]]
    distinct, use, groups = evaluation.plan_threshold_groups(quads)
    assert [[int(q[0, 0, 0]) for q in d] for d in distinct] == [[1, 2], [5, 6, 7]]
    assert use == [[0, 0], [1, 1], [0, 2]]
    assert [[i for i, _ in g] for g in groups] == [[0, 1], [0, 1], [1]]
    assert int(groups[2][0][1][0, 0, 0]) == 7


def test_plan_none_at_some_thresholds_and_an_image_never_found():
    quads = [[None, None, _quad(3)], [_quad(1), None, _quad(3)], [None, None, _quad(4)]]
    distinct, use, groups = evaluation.plan_threshold_groups(quads)
    assert [len(d) for d in distinct] == [1, 0, 2]
    assert use == [[None, None, 0], [0, None, 0], [None, None, 1]]
    assert [[i for i, _ in g] for g in groups] == [[0, 2], [2]]            # image 1 is in no group
    assert evaluation.plan_threshold_groups([[None, None]]) == ([[], []], [[None, None]], [])
    assert evaluation.plan_threshold_groups([]) == ([], [], [])
    with pytest.raises(ValueError):
        evaluation.plan_threshold_groups([[None], [None, None]])


def test_plan_after_the_fallback_substitution():
    from chessvision import constants

    whole = constants.WHOLE_MASK_QUADRANGLE
    found = [[None, _quad(2)], [None, _quad(2)], [_quad(9), None]]
    quads = [[whole if q is None else q for q in row] for row in found]
    distinct, use, groups = evaluation.plan_threshold_groups(quads)
    assert use == [[0, 0], [0, 0], [1, 1]] and [len(g) for g in groups] == [2, 2]
    assert distinct[0][0] is whole and np.array_equal(distinct[1][1], whole)
    # equality is of bytes: the same numbers in another dtype are another quadrangle
    _, use2, _ = evaluation.plan_threshold_groups([[_quad(1)], [_quad(1).astype(np.int64)]])
    assert use2 == [[0], [1]]


# ---- argument validation: before any engine is touched --------------------------------------------------------------------------------
class _NoEngine(ChessVision):
    """An instance whose models, engines and library must never be asked for."""

    def __init__(self):
        pass

    def __getattr__(self, name):
        raise AssertionError(f"evaluate_thresholds touched {name!r} before its arguments were checked")


def test_arguments_are_checked_before_anything_is_touched():
    cv = _NoEngine()
    image = np.zeros((64, 64, 3), np.uint8)
    fen = "8/8/8/8/8/8/8/8"
    for thr in ([], (), list(np.linspace(0, 1, 33)), [0.5, math.nan], [-0.01], [1.01], [0.5, 0.5], [0.5, 0.5 + 1e-9], 0.5, None):
        with pytest.raises(ValueError):
            ChessVision.evaluate_thresholds(cv, [image], thr, true_fens=[fen])
    with pytest.raises(AssertionError, match="touched"):                  # a good grid gets past the check (and meets the stub)
        ChessVision.evaluate_thresholds(cv, [image], [0.5, 0.5000001], true_fens=[fen])
    assert np.float32(0.5) != np.float32(0.5000001) and np.float32(0.5) == np.float32(0.5 + 1e-9)


def test_ground_truth_rules_are_those_of_targets():
    cv = ChessVision.__new__(ChessVision)                    # class attributes only: evaluation_resize = "area"
    image = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="ground truth"):
        cv.evaluate_thresholds([image], [0.5])
    with pytest.raises(ValueError, match="image 0"):
        cv.evaluate_thresholds([image], [0.5], true_fens=["not a fen"])
    with pytest.raises(ValueError, match="label mask"):
        cv.evaluate_thresholds([image], [0.5], label_masks=[np.zeros((8, 8), np.uint8)])
    with pytest.raises(ValueError, match="entries"):
        cv.evaluate_thresholds([image], [0.5], true_fens=[])
    empty = cv.evaluate_thresholds([], [0.7, 0.3], true_fens=[])
    assert empty.thresholds == [0.7, 0.3] and len(empty.reports) == 2 and empty.boards_classified == 0


# ---- curve / best ---------------------------------------------------------------------------------------------------------------------
def _report(top1, pixel_accuracies):
    seg = [evaluation.SegmentationScores(bce=0.1, dice_loss=0.2, loss=0.3, dice=0.5, iou=0.4, pixel_accuracy=p) for p in pixel_accuracies]
    evs = [evaluation.ImageEvaluation(segmentation=s, position=None, extraction_failed=False) for s in seg]
    agg = evaluation.aggregate(evs, [0.01] * len(evs))
    agg["top_1_accuracy"] = top1
    return evaluation.EvaluationReport(results=[], evaluations=evs, aggregate=agg)


def test_curve_and_best_on_hand_made_reports():
    reports = [_report(0.5, [0.5, 1.0]), _report(math.nan, []), _report(0.75, [0.25]), _report(0.75, [1.0])]
    sweep = evaluation.ThresholdSweepReport.from_reports([0.7, 0.1, 0.3, 0.5], reports, boards_found=9, boards_classified=4)
    assert set(sweep.curve) == (set(reports[0].aggregate) - {"avg_time_per_prediction"}) | {"mean_pixel_accuracy"}
    assert all(len(v) == 4 for v in sweep.curve.values())
    assert sweep.curve["top_1_accuracy"][0] == 0.5 and math.isnan(sweep.curve["top_1_accuracy"][1])
    assert sweep.curve["mean_pixel_accuracy"][0] == 0.75 and math.isnan(sweep.curve["mean_pixel_accuracy"][1])
    assert sweep.curve["mean_dice"][2] == reports[2].aggregate["mean_dice"] == 0.5
    assert sweep.best() == 0.3                                # the first of the two 0.75s; the NaN is ignored
    assert sweep.best("mean_pixel_accuracy") == 0.5
    assert sweep.at(0.3) is reports[2] and sweep.at(np.float32(0.7)) is reports[0]
    with pytest.raises(KeyError):
        sweep.at(0.4)
    with pytest.raises(ValueError):
        evaluation.ThresholdSweepReport.from_reports([0.1], [reports[1]]).best()
    assert (sweep.boards_found, sweep.boards_classified) == (9, 4)


# ---- the record layout ----------------------------------------------------------------------------------------------------------------
def test_level_record_mirrors_the_header():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "chessvision_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct cv_level_record \{(.*?)\} cv_level_record_t;", header, flags=re.S).group(1)
    cap = int(re.search(r"#define CV_MAX_THRESHOLDS (\d+)", header).group(1))
    assert cap == hip_backend.MAX_THRESHOLDS == evaluation.MAX_THRESHOLDS == 32
    words, names = 0, []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"int32_t\s+(\w+)((?:\[[^\]]+\])*)", decl)
        assert m, decl
        dims = [int(eval(d, {"CV_MAX_THRESHOLDS": cap})) for d in re.findall(r"\[([^\]]+)\]", m.group(2))]   # noqa: S307 - the header's own arithmetic
        names.append(m.group(1))
        assert hip_backend.LEVEL_RECORD.fields[m.group(1)][1] == 4 * words, m.group(1)
        words += int(np.prod(dims)) if dims else 1
    assert tuple(names) == hip_backend.LEVEL_RECORD.names
    assert 4 * words == hip_backend.LEVEL_RECORD.itemsize == 320 and hip_backend.LEVEL_RECORD.itemsize % 64 == 0
    assert hip_backend.LEVEL_RECORD["hist"].shape == (2, 33)
    declared = set(re.findall(r"\b(cv_[a-z0-9_]+)\s*\(", header))
    assert {"cv_threshold_levels", "cv_threshold_levels_finish"} <= declared
    assert {"cv_threshold_levels", "cv_threshold_levels_finish"} <= {name for name, _, _ in hip_backend.SYMBOLS}
    assert hasattr(hip_backend.HipEngine, "threshold_levels_dev") and hasattr(hip_backend.HipEngine, "threshold_levels")


# ---- one threshold's report from explicit lists ------------------------------------------------------------------------------------
def test_build_report_reads_its_lists_and_leaves_the_targets_alone():
    from chessvision.cv_types import BoardExtractionResult, ChessVisionResult

    fen = "8/8/8/8/8/8/8/8"
    targets = evaluation.Targets(3, true_fens=[fen, fen, None], label_masks=[np.zeros((256, 256), np.uint8), None, None])
    own_seg, own_pos = targets.segmentation, targets.position
    blank = BoardExtractionResult(board_image=None, binary_mask=None, quadrangle=None, probabilities=None)
    results = [ChessVisionResult(board_extraction=blank, position=None, processing_time=0.5) for _ in range(3)]
    seg = [evaluation.SegmentationScores(bce=0.1, dice_loss=0.2, loss=0.3, dice=0.5, iou=0.4, pixel_accuracy=0.9), None, None]
    rep = evaluation.build_report(results, targets.labels, seg, [None] * 3)
    assert rep.results is results and [e.segmentation for e in rep.evaluations] == seg
    assert [e.extraction_failed for e in rep.evaluations] == [True, True, False]      # a FEN but no board; no FEN: not a failure
    assert rep.aggregate["extraction_failures"] == 2 and rep.aggregate["mean_dice"] == 0.5
    assert targets.segmentation is own_seg and targets.position is own_pos
    assert own_seg == [None] * 3 and own_pos == [None] * 3
    same = targets.report(results)                            # Targets.report is the same function on the instance's own lists
    assert [e.segmentation for e in same.evaluations] == [None] * 3 and same.aggregate["extraction_failures"] == 2

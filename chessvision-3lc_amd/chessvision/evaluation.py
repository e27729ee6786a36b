"""Scores against ground truth: what the reference's evaluation side computes from the two networks' outputs and the labels.

``scripts/eval/evaluate.py:264-360`` compares every ``process_image`` result with the true piece placement (square accuracy of
``original_fen`` and ``fen``, top-1/2/3 accuracy of ``model_probabilities``, fixes, improvements, extraction failures) and averages
them into its ``test_results`` record; ``scripts/train/unet_loss_collector.py:19-48`` writes a per-image ``loss`` = soft Dice loss +
mean ``BCEWithLogitsLoss`` of the UNet's logits against the label mask; ``train_unet.py:333-338`` selects checkpoints by ``val_dice``.

The functions below keep the reference's names and signatures and work on host arrays, without ``python-chess``: they are the
readable forms and the test checkers.  ``ChessVision.evaluate_images`` does not come through them: there the per-pixel reductions
run on the device, on the logits where the UNet left them (``HipEngine.segmentation_scores_dev``), and the per-square scores of a
whole job come from one native call (``hip_backend.classification_scores``).

The classifier's own batched caller, ``scripts/train/train_classifier.py`` (``validate()`` :90-111 and the ``tlc.collect_metrics`` pass
:274-292 over a table of labelled 64 x 64 squares), is ``ChessVision.evaluate_squares``: ``square_records`` below is its host form and
checker, ``SquareScores`` / ``SquaresReport`` are what it returns.  3LC's ``ClassificationMetricsCollector`` is not in the reference
tree; loss / predicted / confidence / accuracy per sample is this library's reading of it.

Two readings are stated here because the reference leaves them open:

* Dice.  The reference calls ``dice_loss(..., reduction="none")`` of a vendored Pytorch-UNet whose directory is empty in its tree.
  Used here: upstream Pytorch-UNet's ``dice_coeff`` per image, ``(2 * inter + 1e-6) / (sets_sum + 1e-6)`` with ``sets_sum`` replaced
  by ``2 * inter`` where it is 0.
* Ties.  The reference ranks classes with ``np.argsort`` of the default kind, which numpy 2.2 does not keep stable for 13 float32
  columns, so its order among EQUAL probabilities is undefined.  Used here: the stable order, rank of the true class t =
  ``#{j: p_j > p_t} + #{j > t: p_j == p_t}``.  A square holding a NaN has rank 13: a miss at every k.
"""
from __future__ import annotations

import math
from collections.abc import Sequence
from dataclasses import dataclass, field

import numpy as np
from numpy.typing import NDArray

from . import constants
from .cv_types import ChessVisionResult

_EPS = 1e-6
AGGREGATE_KEYS = ("top_1_accuracy_validated", "top_1_accuracy", "top_2_accuracy", "top_3_accuracy", "validation_fixes",
                  "validation_improvements", "extraction_failures", "avg_time_per_prediction")


# ---- the reference's host functions (evaluate.py:28-140) ---------------------------------------------------------------------------
@dataclass
class PositionAccuracy:
    accuracy: float
    num_correct: int
    total_squares: int = 64


@dataclass
class TopKAccuracyResult:
    k: int
    accuracies: Sequence[float]

    @property
    def top_1(self) -> float:
        return self.accuracies[0]

    @property
    def top_2(self) -> float:
        return self.accuracies[1] if len(self.accuracies) > 1 else 0.0

    @property
    def top_3(self) -> float:
        return self.accuracies[2] if len(self.accuracies) > 2 else 0.0


def board_to_labels(fen: str) -> list[str]:
    """Piece-placement field of a FEN (anything after the first space is ignored) -> 64 symbols in a8..h1 order, "f" for an empty
    square.  ``ValueError`` for a malformed placement.  (The reference takes a ``chess.BaseBoard``; this form takes its FEN.)"""
    ranks = str(fen).split(" ", 1)[0].split("/")
    if len(ranks) != 8:
        raise ValueError(f"malformed piece placement {fen!r}: {len(ranks)} ranks instead of 8")
    labels: list[str] = []
    for rank in ranks:
        row: list[str] = []
        for ch in rank:
            if ch in "12345678":
                row += ["f"] * int(ch)
            elif ch != "f" and ch in constants.LABEL_INDICES:
                row.append(ch)
            else:
                raise ValueError(f"malformed piece placement {fen!r}: unknown symbol {ch!r}")
        if len(row) != 8:
            raise ValueError(f"malformed piece placement {fen!r}: rank {rank!r} does not sum to 8 squares")
        labels += row
    return labels


def label_indices(fen: str) -> NDArray[np.int8]:
    """``board_to_labels`` as class indices (order of ``constants.LABEL_NAMES``): evaluate.py's ``get_validated_indices``."""
    return np.array([constants.LABEL_INDICES[s] for s in board_to_labels(fen)], dtype=np.int8)


def compute_position_accuracy(predicted_fen: str, true_fen: str) -> PositionAccuracy:
    pred, true = board_to_labels(predicted_fen), board_to_labels(true_fen)
    correct = sum(1 for p, t in zip(pred, true) if p == t)
    return PositionAccuracy(accuracy=correct / 64, num_correct=correct)


def true_class_ranks(model_probabilities: NDArray[np.float32], labels) -> NDArray[np.int32]:
    """(64,13) probabilities, 64 true class indices given per row -> per row the number of classes ranked above the true one
    (0 = the arg-max), ties in numpy's stable order; 13 for a row holding a NaN."""
    p = np.asarray(model_probabilities, dtype=np.float32)
    t = np.asarray(labels, dtype=np.int64)
    pt = p[np.arange(p.shape[0]), t][:, None]
    with np.errstate(invalid="ignore"):
        rank = (p > pt).sum(axis=1) + ((p == pt) & (np.arange(p.shape[1])[None, :] > t[:, None])).sum(axis=1)
    return np.where(np.isnan(p).any(axis=1), p.shape[1], rank).astype(np.int32)


def compute_model_topk_accuracy(model_probabilities: NDArray[np.float32], true_fen: str, k: int = 3) -> TopKAccuracyResult:
    """Fraction of squares whose true class is among the k most probable, for 1..k (evaluate.py:112-140).  Row i of the
    probabilities is compared with square i of the FEN in a8..h1 order, as in the reference."""
    rank = true_class_ranks(model_probabilities, label_indices(true_fen))
    return TopKAccuracyResult(k=k, accuracies=[int((rank < j).sum()) / 64 for j in range(1, k + 1)])


# ---- the records ---------------------------------------------------------------------------------------------------------------------
@dataclass
class SegmentationScores:
    """One image's UNet output against its label mask."""
    bce: float                 # mean over pixels of BCEWithLogitsLoss
    dice_loss: float           # 1 - soft Dice of sigmoid(logits) and the mask
    loss: float                # dice_loss + bce: the LossCollector's column
    dice: float                # Dice of the thresholded mask and the label: the per-image val_dice (1 when both are empty)
    iou: float                 # intersection over union of the two (1 when the union is empty)
    pixel_accuracy: float


@dataclass
class PositionScores:
    """One board's classifier output against its true placement.  The arrays have one entry per row of ``model_probabilities``
    (``PositionResult.square_names`` order): the per-square columns of evaluate.py:327-343."""
    top_k: tuple               # (top-1, top-2, top-3) accuracy of the raw probabilities
    accuracy_original: float   # square accuracy of original_fen: the reference's top_1_accuracy
    accuracy_validated: float  # square accuracy of fen: its top_1_accuracy_validated
    mean_loss: float           # mean of -log(p_true)
    num_fixes: int
    true_labels: NDArray[np.int8]
    predicted_labels: NDArray[np.int8]
    validated_labels: NDArray[np.int8]
    rank: NDArray[np.int32]
    confidence: NDArray[np.float32]
    loss: NDArray[np.float64]

    @property
    def top_1(self) -> float:
        return self.top_k[0]

    @property
    def top_2(self) -> float:
        return self.top_k[1]

    @property
    def top_3(self) -> float:
        return self.top_k[2]


@dataclass
class ImageEvaluation:
    segmentation: SegmentationScores | None      # None: no label mask was given for the image
    position: PositionScores | None              # None: no FEN was given, or no board was found
    extraction_failed: bool                      # no board was found (counted only among the images that have a FEN)


@dataclass
class EvaluationReport:
    results: list[ChessVisionResult]
    evaluations: list[ImageEvaluation]
    aggregate: dict = field(default_factory=dict)


@dataclass
class SquareScores:
    """The per-square columns of a squares table, one entry per square: the fields of ``cv_square_record_t``
    (include/chessvision_hip.h)."""
    predicted: NDArray[np.int32]     # first maximum of the 13 logits
    rank: NDArray[np.int32]          # classes ranked above the true one (stable reading); 13 for a NaN row, -1 when unlabelled
    label: NDArray[np.int32]         # true class index, -1 = unlabelled
    flags: NDArray[np.int32]         # bit 0: the row holds a NaN
    confidence: NDArray[np.float32]  # the largest soft-max probability
    loss: NDArray[np.float32]        # CrossEntropyLoss(reduction="none"); NaN when unlabelled or NaN row
    max_logit: NDArray[np.float32]
    logsumexp: NDArray[np.float32]

    @property
    def correct(self) -> NDArray[np.bool_]:
        """predicted == label: the reference's ``predicted.eq(target)``; False for unlabelled squares and NaN rows."""
        return (self.label >= 0) & (self.predicted == self.label) & ((self.flags & 1) == 0)

    @classmethod
    def from_records(cls, records) -> "SquareScores":
        """From the structured array of ``HipEngine.square_records`` (``hip_backend.SQUARE_RECORD``)."""
        return cls(**{k: np.ascontiguousarray(records[k]) for k in ("predicted", "rank", "label", "flags", "confidence", "loss",
                                                                     "max_logit", "logsumexp")})


@dataclass
class SquaresReport:
    """What ``ChessVision.evaluate_squares`` returns: the per-square columns (also reachable as attributes of the report),
    optionally the (N,512) classifier embeddings, and ``aggregate`` = the record of ``cv_square_records_finish`` as a dict
    (n, n_labelled, n_correct, n_nan, hits, confusion, loss_sum, val_loss, val_acc, n_batches)."""
    scores: SquareScores
    embeddings: NDArray[np.float32] | None = None
    aggregate: dict = field(default_factory=dict)

    predicted = property(lambda self: self.scores.predicted)
    confidence = property(lambda self: self.scores.confidence)
    loss = property(lambda self: self.scores.loss)
    correct = property(lambda self: self.scores.correct)
    rank = property(lambda self: self.scores.rank)


# ---- host forms of the scores ------------------------------------------------------------------------------------------------------
def square_label_indices(labels, n: int) -> NDArray[np.int8]:
    """Labels of a squares table -> (n,) int8 class indices, -1 = unlabelled.  Accepted: None (all unlabelled), integers -1..12,
    label names in ``constants.LABEL_NAMES`` order ("B" .. "r", "f" = empty) and the reference's folder names (``data/squares``:
    the black pieces' folders carry a leading underscore, "_b" .. "_r")."""
    if labels is None:
        return np.full(n, -1, dtype=np.int8)
    items = list(labels.tolist() if isinstance(labels, np.ndarray) else labels)
    if len(items) != n:
        raise ValueError(f"labels has {len(items)} entries for {n} squares")
    out = np.empty(n, dtype=np.int8)
    for i, v in enumerate(items):
        if v is None:
            out[i] = -1
        elif isinstance(v, str):
            name = v[1:] if len(v) == 2 and v[0] == "_" else v
            if name not in constants.LABEL_INDICES:
                raise ValueError(f"square {i}: unknown label {v!r}")
            out[i] = constants.LABEL_INDICES[name]
        else:
            if int(v) != v or not -1 <= int(v) < constants.NUM_CLASSES:
                raise ValueError(f"square {i}: a label must be a class index 0..{constants.NUM_CLASSES - 1} or -1, got {v!r}")
            out[i] = int(v)
    return out


def square_records(logits, labels=None) -> SquareScores:
    """The records of ``cv_square_records`` for host arrays, in numpy and in the kernel's float32 arithmetic: (N,13) logits and N
    labels (see ``square_label_indices``) -> ``SquareScores``.  m = first maximum by ``>``; s = sum of ``exp(x_j - m)`` added in
    ascending j; confidence = 1 / s; loss = log(s) - (x_t - m); logsumexp = m + log(s).  The integer fields are comparisons of the
    float32 logits and agree with the device exactly; the floats agree to the rounding of ``exp`` / ``log`` (numpy's and the
    device's are each within an ulp).  A row holding a NaN has rank 13, flag bit 0 and NaN in all four floats."""
    x = np.ascontiguousarray(np.asarray(logits, dtype=np.float32))
    if x.ndim != 2 or x.shape[1] != constants.NUM_CLASSES:
        raise ValueError(f"square_records expects (N,{constants.NUM_CLASSES}) logits")
    n = x.shape[0]
    t = square_label_indices(labels, n).astype(np.int32)
    nan = np.isnan(x).any(axis=1)
    predicted = np.zeros(n, dtype=np.int32)
    m = x[:, 0].copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(1, x.shape[1]):
            up = x[:, j] > m
            predicted[up] = j
            m[up] = x[up, j]
        s = np.zeros(n, dtype=np.float32)
        for j in range(x.shape[1]):
            s = s + np.exp(x[:, j] - m)                     # float32 throughout, ascending j
        ls = np.log(s)
        xt = x[np.arange(n), np.maximum(t, 0)]
        cols = np.arange(x.shape[1])[None, :]
        rank = ((x > xt[:, None]).sum(axis=1) + ((x == xt[:, None]) & (cols > t[:, None])).sum(axis=1)).astype(np.int32)
        loss = (ls - (xt - m)).astype(np.float32)
        confidence = (np.float32(1) / s).astype(np.float32)
        logsumexp = (m + ls).astype(np.float32)
    rank = np.where(t < 0, -1, np.where(nan, x.shape[1], rank)).astype(np.int32)
    qnan = np.float32(np.nan)
    return SquareScores(predicted=predicted, rank=rank, label=t, flags=nan.astype(np.int32),
                        confidence=np.where(nan, qnan, confidence), loss=np.where(nan | (t < 0), qnan, loss),
                        max_logit=np.where(nan, qnan, m), logsumexp=np.where(nan, qnan, logsumexp))


def _dice(inter: float, sets_sum: float) -> float:
    if sets_sum == 0:
        sets_sum = 2 * inter
    return (2 * inter + _EPS) / (sets_sum + _EPS)


def segmentation_scores(logits: NDArray[np.float32], label_mask: NDArray[np.uint8], threshold: float = 0.5) -> SegmentationScores:
    """The six scores of ONE image in numpy: float64 sums of the float32 logits; the hard mask is ``sigmoid(x) > threshold`` with the
    float32 sigmoid, as ``utils.create_binary_mask`` thresholds it.  A pixel is labelled "board" iff its mask value is non-zero."""
    x32 = np.asarray(logits, dtype=np.float32).reshape(-1)
    t = np.asarray(label_mask).reshape(-1) != 0
    if x32.size != t.size or x32.size == 0:
        raise ValueError("segmentation_scores expects one label per logit")
    x = x32.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        bce = float(np.mean(np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))))
        v = 1.0 / (1.0 + np.exp(-x))
        pred = (np.float32(1) / (np.float32(1) + np.exp(-x32))) > np.float32(threshold)
        dice_loss = 1.0 - _dice(float((v * t).sum()), float(v.sum()) + int(t.sum()))     # v * t: a NaN pixel spoils the sum, labelled or not
    n_label, n_pred, n_both = int(t.sum()), int(pred.sum()), int((pred & t).sum())
    union = n_pred + n_label - n_both
    return SegmentationScores(bce=bce, dice_loss=dice_loss, loss=dice_loss + bce, dice=_dice(n_both, n_pred + n_label),
                              iou=1.0 if union == 0 else n_both / union,
                              pixel_accuracy=(x.size - n_pred - n_label + 2 * n_both) / x.size)


MAX_THRESHOLDS = 32
CURVE_KEYS = tuple(k for k in AGGREGATE_KEYS if k != "avg_time_per_prediction") + ("mean_loss", "mean_dice", "mean_iou",
                                                                                   "mean_pixel_accuracy")


def check_thresholds(thresholds) -> NDArray[np.float32]:
    """The thresholds of a sweep as float32, in the caller's order.  ``ValueError`` for an empty grid, more than ``MAX_THRESHOLDS``
    values, a value that is NaN or outside [0, 1], or two values equal as float32."""
    try:
        t = np.asarray(list(thresholds), dtype=np.float32).reshape(-1)
    except TypeError:
        raise ValueError(f"thresholds must be a sequence of numbers, got {thresholds!r}") from None
    if t.size == 0:
        raise ValueError("thresholds is empty")
    if t.size > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds per sweep, got {t.size}")
    if not bool(np.all((t >= 0) & (t <= 1))):                # a NaN fails both comparisons
        raise ValueError(f"every threshold must be in [0, 1], got {[float(v) for v in t]}")
    if np.unique(t).size != t.size:
        raise ValueError(f"two thresholds are equal as float32: {[float(v) for v in t]}")
    return t


def threshold_levels(logits, thresholds, label_mask=None):
    """The numpy form of ``cv_threshold_levels`` and its checker: (N, ...) float32 logits (the first axis counts images, as on the
    device; a 1-D array is one image), strictly ascending thresholds in [0, 1], optional labels of the same shape ("board" iff
    non-zero) -> (levels uint8 of the logits' shape, hist (N,2,33) int64, n_nan (N,)).  ``level = #{k: v > thresholds[k]}`` with the float32 sigmoid ``segmentation_scores`` thresholds, so
    ``levels > k`` is its hard mask at ``thresholds[k]``; ``hist[i, b, l]`` counts image i's pixels at level l whose label is zero
    (b = 0; every pixel without labels) or non-zero (b = 1).  A single image is treated as N = 1."""
    x = np.asarray(logits, dtype=np.float32)
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    if not 1 <= thr.size <= MAX_THRESHOLDS or not bool(np.all((thr >= 0) & (thr <= 1))) or not bool(np.all(thr[1:] > thr[:-1])):
        raise ValueError(f"threshold_levels expects 1..{MAX_THRESHOLDS} strictly ascending thresholds in [0, 1]")
    if x.size == 0:
        raise ValueError("threshold_levels expects at least one logit")
    flat = x.reshape(1, -1) if x.ndim < 2 else x.reshape(x.shape[0], -1)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.float32(1) / (np.float32(1) + np.exp(-flat))
        levels = np.zeros(flat.shape, dtype=np.uint8)
        for t in thr:
            levels += v > t                                   # NaN compares false: level 0
    if label_mask is None:
        on = np.zeros(flat.shape, dtype=bool)
    else:
        on = np.asarray(label_mask).reshape(flat.shape[0], -1) != 0
        if on.shape != flat.shape:
            raise ValueError("threshold_levels expects one label per logit")
    hist = np.zeros((flat.shape[0], 2, MAX_THRESHOLDS + 1), dtype=np.int64)
    for i in range(flat.shape[0]):
        for b in (0, 1):
            hist[i, b] = np.bincount(levels[i][on[i] == bool(b)], minlength=MAX_THRESHOLDS + 1)
    return levels.reshape(x.shape), hist, np.isnan(flat).sum(axis=1)


def level_counts(hist, n_thresholds: int):
    """``hist`` (..., 2, 33) of ``threshold_levels`` -> (n_label (...,), n_pred (..., T), n_both (..., T)): the suffix sums that give
    every threshold's counts, ``n_pred[k] = sum_{l > k} hist[0][l] + hist[1][l]``, ``n_both[k] = sum_{l > k} hist[1][l]``."""
    h = np.asarray(hist, dtype=np.int64)
    above = np.flip(np.cumsum(np.flip(h, axis=-1), axis=-1), axis=-1)[..., 1:n_thresholds + 1]   # [..., b, k] = sum_{l > k}
    return h[..., 1, :].sum(axis=-1), above[..., 0, :] + above[..., 1, :], above[..., 1, :]


def plan_threshold_groups(quads):
    """Which boards a threshold sweep has to warp and classify.  ``quads[k][i]``: image i's quadrangle at threshold k ((4,1,2) int32
    or None), after the ``fallback_quad`` substitution.  Two quadrangles are the same iff their bytes are equal.  Returns
    ``(distinct, use, groups)``: ``distinct[i]`` = image i's distinct quadrangles in order of first appearance (over k ascending);
    ``use[k][i]`` = the index into ``distinct[i]`` that threshold k uses, or None; ``groups[g]`` = [(i, distinct[i][g]) for every image
    that has a g-th distinct quadrangle, in image order] -- at most one board per image, so a group goes through the warp +
    classifier stage as one ``found`` subset, and there are at most ``len(quads)`` groups."""
    n = len(quads[0]) if quads else 0
    distinct: list[list] = [[] for _ in range(n)]
    keys: list[dict] = [{} for _ in range(n)]
    use: list[list] = []
    for row in quads:
        if len(row) != n:
            raise ValueError("plan_threshold_groups expects one quadrangle (or None) per image at every threshold")
        used = []
        for i, q in enumerate(row):
            if q is None:
                used.append(None)
                continue
            a = np.ascontiguousarray(q)
            key = (a.dtype.str, a.shape, a.tobytes())
            if key not in keys[i]:
                keys[i][key] = len(distinct[i])
                distinct[i].append(q)
            used.append(keys[i][key])
        use.append(used)
    depth = max((len(d) for d in distinct), default=0)
    groups = [[(i, distinct[i][g]) for i in range(n) if len(distinct[i]) > g] for g in range(depth)]
    return distinct, use, groups


@dataclass
class ThresholdSweepReport:
    """What ``ChessVision.evaluate_thresholds`` returns.  ``thresholds`` are the caller's values in the caller's order;
    ``reports[j]`` is what ``evaluate_images(..., threshold=thresholds[j])`` returns; ``curve[key][j]`` is ``reports[j].aggregate[key]``
    for every key but ``avg_time_per_prediction``, plus ``mean_pixel_accuracy``.  The reports share arrays (logits always, board,
    crops and probabilities where the quadrangle is the same): they are views, copy before writing."""
    thresholds: list
    reports: list
    curve: dict = field(default_factory=dict)
    boards_found: int = 0          # sum over the thresholds of the boards found at each
    boards_classified: int = 0     # distinct boards actually warped and classified

    def at(self, threshold: float) -> EvaluationReport:
        """The report of a threshold that was asked for (compared as float32)."""
        t = np.float32(threshold)
        for j, v in enumerate(self.thresholds):
            if np.float32(v) == t:
                return self.reports[j]
        raise KeyError(f"threshold {threshold!r} is not one of {self.thresholds}")

    def best(self, key: str = "top_1_accuracy") -> float:
        """The threshold with the largest ``curve[key]``: the first one on ties, NaN ignored (``ValueError`` when all are NaN)."""
        values = self.curve[key]
        best = None
        for j, v in enumerate(values):
            if v == v and (best is None or v > values[best]):
                best = j
        if best is None:
            raise ValueError(f"curve[{key!r}] holds no number")
        return self.thresholds[best]

    @classmethod
    def from_reports(cls, thresholds, reports, boards_found: int = 0, boards_classified: int = 0) -> "ThresholdSweepReport":
        curve = {key: [r.aggregate[key] for r in reports] for key in CURVE_KEYS if key != "mean_pixel_accuracy"}
        curve["mean_pixel_accuracy"] = [_mean_pixel_accuracy(r.evaluations) for r in reports]
        return cls(thresholds=list(thresholds), reports=list(reports), curve=curve, boards_found=int(boards_found),
                   boards_classified=int(boards_classified))


def _mean_pixel_accuracy(evaluations) -> float:
    values = [e.segmentation.pixel_accuracy for e in evaluations if e.segmentation is not None]
    return sum(values) / len(values) if values else math.nan


def row_labels(true_labels, flip: bool) -> NDArray[np.int8]:
    """True class indices in a8..h1 order -> the order of the classifier's rows (``square_names``): reversed for a flipped board."""
    t = np.asarray(true_labels, dtype=np.int8)
    return t[::-1].copy() if flip else t


def position_scores(model_probabilities: NDArray[np.float32], fen: str, original_fen: str, true_fen: str, num_fixes: int = 0,
                    flip: bool = False) -> PositionScores:
    """The record of ONE board on the host, in plain numpy (``evaluate_images`` gets the same from the native call).  Row i of the
    probabilities is compared with the true piece on ``square_names[i]``: a8..h1, or h1..a8 with ``flip``."""
    p = np.asarray(model_probabilities, dtype=np.float32)
    true_rows = row_labels(label_indices(true_fen), flip)
    rank = true_class_ranks(p, true_rows)
    predicted = np.empty(64, dtype=np.int8)
    for i in range(64):                                      # first maximum by ">" (cv_decode_positions); np.argmax but for NaN rows
        best = 0
        for k in range(1, 13):
            if p[i, k] > p[i, best]:
                best = k
        predicted[i] = best
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = -np.log(p[np.arange(64), true_rows.astype(np.int64)].astype(np.float64))
    return PositionScores(top_k=tuple(int((rank < j).sum()) / 64 for j in (1, 2, 3)),
                          accuracy_original=compute_position_accuracy(original_fen, true_fen).accuracy,
                          accuracy_validated=compute_position_accuracy(fen, true_fen).accuracy,
                          mean_loss=float(loss.sum() / 64.0), num_fixes=int(num_fixes), true_labels=true_rows,
                          predicted_labels=predicted, validated_labels=row_labels(label_indices(fen), flip), rank=rank,
                          confidence=np.max(p, axis=1), loss=loss)


def aggregate(evaluations: Sequence[ImageEvaluation], processing_times: Sequence[float]) -> dict:
    """evaluate.py:347-356's ``aggregate_data`` from the per-image records, with its arithmetic: the four accuracies are sums over the
    successful extractions divided by their number (NaN when there are none), over the images that have a FEN; ``mean_loss``,
    ``mean_dice`` and ``mean_iou`` are means over the images that had a label mask (NaN when there are none)."""
    scored = [e for e in evaluations if e.position is not None]
    failures = sum(1 for e in evaluations if e.extraction_failed)

    def mean(values):
        values = list(values)
        return sum(values) / len(values) if values else math.nan

    seg = [e.segmentation for e in evaluations if e.segmentation is not None]
    times = list(processing_times)
    return {
        "top_1_accuracy_validated": mean(e.position.accuracy_validated for e in scored),
        "top_1_accuracy": mean(e.position.accuracy_original for e in scored),
        "top_2_accuracy": mean(e.position.top_k[1] for e in scored),
        "top_3_accuracy": mean(e.position.top_k[2] for e in scored),
        "validation_fixes": sum(e.position.num_fixes for e in scored),
        "validation_improvements": sum(1 for e in scored if e.position.accuracy_validated > e.position.accuracy_original),
        "extraction_failures": failures,
        "avg_time_per_prediction": mean(times),
        "mean_loss": mean(s.loss for s in seg),
        "mean_dice": mean(s.dice for s in seg),
        "mean_iou": mean(s.iou for s in seg),
    }


# ---- ground truth of one evaluate_images call --------------------------------------------------------------------------------------
class Targets:
    """Checked ground truth of a call, in the form the batched pipeline uses: per image the true class indices in a8..h1 order (or
    None) and the (256,256) uint8 label mask (or None)."""

    def __init__(self, n_images: int, true_fens=None, label_masks=None):
        if true_fens is None and label_masks is None:
            raise ValueError("evaluate_images needs ground truth: true_fens, label_masks or both")
        self.fens: list = [None] * n_images if true_fens is None else list(true_fens)
        self.masks: list = [None] * n_images if label_masks is None else list(label_masks)
        if len(self.fens) != n_images:
            raise ValueError(f"true_fens has {len(self.fens)} entries for {n_images} images")
        if len(self.masks) != n_images:
            raise ValueError(f"label_masks has {len(self.masks)} entries for {n_images} images")
        self.labels: list = [None] * n_images
        for i, fen in enumerate(self.fens):
            if fen is None:
                continue
            try:
                self.labels[i] = label_indices(fen)
            except (ValueError, AttributeError, TypeError) as exc:
                raise ValueError(f"image {i}: {exc}") from None
        size = (constants.INPUT_SIZE[1], constants.INPUT_SIZE[0])
        for i, m in enumerate(self.masks):
            if m is None:
                continue
            if not isinstance(m, np.ndarray) or m.dtype != np.uint8 or m.shape != size:
                what = f"{m.dtype} {m.shape}" if isinstance(m, np.ndarray) else type(m).__name__
                raise ValueError(f"image {i}: a label mask must be a {size} uint8 array, got {what}")
        self.segmentation: list = [None] * n_images      # filled by the pipeline: SegmentationScores / PositionScores per image
        self.position: list = [None] * n_images

    def report(self, results: list[ChessVisionResult]) -> EvaluationReport:
        return build_report(results, self.labels, self.segmentation, self.position)


def build_report(results: list[ChessVisionResult], labels, segmentation, position) -> EvaluationReport:
    """The report of one call (one threshold of a sweep) from its results and, per image, the true class indices (or None), the
    ``SegmentationScores`` (or None) and the ``PositionScores`` (or None)."""
    evaluations = [ImageEvaluation(segmentation=segmentation[i], position=position[i],
                                   extraction_failed=labels[i] is not None and r.position is None)
                   for i, r in enumerate(results)]
    return EvaluationReport(results=results, evaluations=evaluations,
                            aggregate=aggregate(evaluations, [r.processing_time for r in results]))

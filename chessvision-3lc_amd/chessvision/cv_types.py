"""Result records handed back by ``ChessVision``.

The attribute names and their order are the public contract of the reference's result objects
(``chessvision/cv_types.py:9-62`` there; read by ``app/computeroot/cv_endpoint.py:165-171`` and
``scripts/eval/evaluate.py:280-330``), so they are kept; everything else about this module is local.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
from numpy.typing import NDArray

from . import constants

U8 = NDArray[np.uint8]
F32 = NDArray[np.float32]


def _doc(text: str):
    return field(metadata={"doc": text})


@dataclass
class ValidationFix:
    square_name: str = _doc('board coordinate, "a1".."h8"')
    original_piece: str = _doc("symbol the classifier chose")
    corrected_piece: str = _doc("symbol after the rule fired")
    rule_name: str = _doc('rule identifier, e.g. "no_pawns_on_ends"')


def pawn_rule_fix(square_names: list[str], square: int, old: int, new: int) -> ValidationFix:
    """One correction of the pawn rule as the native decoders report it: square index, class index before and after."""
    return ValidationFix(square_name=square_names[square], original_piece=constants.LABEL_NAMES[old],
                         corrected_piece=constants.LABEL_NAMES[new], rule_name="no_pawns_on_ends")


@dataclass
class BoardExtractionResult:
    probabilities: F32 = _doc("raw UNet LOGITS, (256,256) -- the reference stores logits under this name (core.py:287,306)")
    binary_mask: U8 = _doc("0 / 255 segmentation mask, (256,256)")
    quadrangle: F32 | None = _doc("(4,1,2) corners in input-image pixels; None when no board was found")
    board_image: U8 | None = _doc("(512,512) rectified gray board; None when no board was found")


@dataclass
class PositionResult:
    fen: str = _doc("piece placement after rule validation")
    original_fen: str = _doc("piece placement straight from the per-square argmax")
    model_probabilities: F32 = _doc("(64,13) class probabilities")
    squares: U8 | None = _doc("(64,64,64,1) square crops, a8..h1 order (None from process_images unless return_crops=True)")
    square_names: list[str] = _doc("coordinate of each row of the two arrays above")
    validation_fixes: list[ValidationFix] = _doc("rule corrections that were applied")

    @property
    def confidence_scores(self) -> list[float]:
        """Top class probability per square.  NOT a reference field: ``cv_endpoint.py:169,227`` reads it although the
        reference result lacks it (HTTP 500 there); provided so the Flask app works against this package."""
        return [float(v) for v in np.max(self.model_probabilities, axis=1)]


@dataclass
class ExtractionQuality:
    """The four board-extraction scores the reference's enrichment job writes into its 3LC table per image
    (``scripts/process_new_raw/process_pipeline.py:287-311``); the attribute names are that table's column names."""
    confidence: float = _doc("2 * mean |v - 0.5| over the largest quarter of the scored values")
    quad_score: float = _doc("quadrangle regularity, 1 = a square; 0 when the mask gave no quadrangle")
    completeness: float = _doc("mask pixels / pixels of the filled outline of the largest mask component")
    distribution: float = _doc("1 - normalised entropy of the ten-bin histogram of the scored values over [0, 1]")


@dataclass
class Embeddings:
    """The activations the reference hands to 3LC's ``EmbeddingsMetricsCollector`` (``scripts/process_new_raw/process_pipeline.py:
    328-351``, ``scripts/train/train_unet.py:219``, ``scripts/train/train_classifier.py:32,212``), reduced to one vector per sample by
    the mean over the spatial dimensions (``chessvision/embeddings.py``)."""
    board_extractor: F32 = _doc("(C,) channel means of the UNet bottleneck, named_modules()[52]; C = 1024 (512 for the bilinear UNet)")
    classifier: F32 | None = _doc("(64,512) pooled layer4 output per square (named_modules()[90], global_pool), rows in "
                                  "square_names order; None when no board was found")


@dataclass
class ChessVisionResult:
    board_extraction: BoardExtractionResult = _doc("always present")
    position: PositionResult | None = _doc("None when board extraction failed")
    processing_time: float = _doc("seconds spent in process_image (per image for process_images)")
    quality: ExtractionQuality | None = field(default=None, metadata={"doc": "process_images(quality=...) only; NOT a reference field"})
    # process_images(embeddings=True) only; NOT a reference field.  A plain attribute with the class-level default None, set by the
    # batched pipeline after construction: the dataclass fields (the constructor's arguments and their order) end with ``quality``, as
    # tests/test_quality_cpu.py and tests/test_evaluation_cpu.py pin them.
    embeddings = None
    # process_images(board_jpeg=q) / process_encoded(board_jpeg=q) only; NOT a reference field: the rectified board as the complete
    # baseline JPEG file libjpeg writes for ``board_extraction.board_image`` at that quality (``bytes``; None where no board was found).
    # An attribute set after construction, like ``embeddings``.
    board_jpeg = None


@dataclass
class ValidationMetrics:
    accuracy_before: float = _doc("square accuracy of original_fen")
    accuracy_after: float = _doc("square accuracy of fen")
    num_fixes: int = _doc("len(fixes)")
    fixes: list[ValidationFix] = _doc("the corrections")

    @property
    def accuracy_delta(self) -> float:
        return self.accuracy_after - self.accuracy_before

"""No GPU: the host side of square-set evaluation -- the three new symbols, the numpy form of the per-square records
(``evaluation.square_records``, the checker of the device kernel) against torch in float64, ``cv_square_records_finish`` against a
restatement of the reference's ``validate()``, the label forms ``evaluate_squares`` accepts, and the fixture of real squares."""
from __future__ import annotations

import ctypes
import inspect
import re
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from chessvision import ChessVision, constants, evaluation, hip_backend
from squares_ref import FIXTURE, check_against_torch, crafted_rows, validate_restated

ROOT = Path(__file__).resolve().parent.parent


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "chessvision_hip.h").read_text(), flags=re.S)
    bound_syms = {name: args for name, _, args in hip_backend.SYMBOLS}
    lib = hip_backend.load_library()
    for sym, n_args in (("cv_resnet_forward_u8_norm", 9), ("cv_square_records", 6), ("cv_square_records_finish", 4)):
        assert re.search(rf"\bint {sym}\s*\(", header), sym
        assert len(bound_syms[sym]) == n_args and hasattr(lib, sym), sym
    assert lib.cv_abi_version() == hip_backend.ABI_VERSION == 6
    assert hip_backend.SQUARE_RECORD.itemsize == 32
    assert hip_backend.SQUARES_SUMMARY.itemsize == 8 * (4 + 13 + 169 + 3 + 1)


def test_argument_errors_come_back_as_status_codes():
    lib = hip_backend.load_library()
    assert lib.cv_resnet_forward_u8_norm(None, None, 1, 0.5, 0.25, 0, None, None, None) == 1 and b"null engine" in lib.cv_last_error()
    assert lib.cv_square_records(None, None, None, 1, None, None) == 1 and b"null engine" in lib.cv_last_error()
    out = np.zeros(1, hip_backend.SQUARES_SUMMARY)
    assert lib.cv_square_records_finish(None, 1, 0, out.ctypes.data_as(ctypes.c_void_p)) == 1
    rec = np.zeros(3, hip_backend.SQUARE_RECORD)
    assert lib.cv_square_records_finish(rec.ctypes.data_as(ctypes.c_void_p), 3, 0, None) == 1
    assert lib.cv_square_records_finish(rec.ctypes.data_as(ctypes.c_void_p), -1, 0, out.ctypes.data_as(ctypes.c_void_p)) == 1
    rec["flags"][1] = 2                                       # a label byte outside -1..12, as the kernel flags it
    rec["label"][1] = 40
    assert lib.cv_square_records_finish(rec.ctypes.data_as(ctypes.c_void_p), 3, 0, out.ctypes.data_as(ctypes.c_void_p)) == 1
    assert b"record 1" in lib.cv_last_error()
    with pytest.raises(hip_backend.HipBackendError):
        hip_backend.square_records_finish(rec)
    empty = hip_backend.square_records_finish(np.zeros(0, hip_backend.SQUARE_RECORD), 64)
    assert empty["n"] == 0 and np.isnan(empty["val_loss"]) and np.isnan(empty["val_acc"])


def test_python_surface():
    assert constants.CLASSIFIER_NORMALIZATION == (0.564, 0.246)
    params = inspect.signature(ChessVision.evaluate_squares).parameters
    assert list(params) == ["self", "squares", "labels", "normalize", "batch_size", "embeddings"]
    assert params["labels"].default is None and params["normalize"].default == "train" and params["batch_size"].default == 512
    assert params["embeddings"].default is False
    assert "does NOT split the forward" in ChessVision.evaluate_squares.__doc__
    for method in ("resnet_forward_u8_norm", "square_records", "square_records_dev"):
        assert callable(getattr(hip_backend.HipEngine, method))
    assert {"scores", "embeddings", "aggregate"} <= {f for f in evaluation.SquaresReport.__dataclass_fields__}


def test_label_forms():
    idx = evaluation.square_label_indices
    assert idx(None, 3).tolist() == [-1, -1, -1]
    assert idx(["B", "_b", "f", "r", "_r", None], 6).tolist() == [0, 6, 12, 11, 11, -1]
    assert idx(np.array([0, 12, -1]), 3).tolist() == [0, 12, -1]
    assert idx(np.array(constants.LABEL_NAMES), 13).tolist() == list(range(13))
    for bad in ([13], [-2], ["x"], ["_B_"], [0.5]):
        with pytest.raises(ValueError):
            idx(bad, 1)
    with pytest.raises(ValueError):
        idx([0, 1], 3)


def test_evaluate_squares_refuses_a_model_that_is_not_hip():
    cv = ChessVision(lazy_load=True)
    cv._classifier = torch.nn.Identity()
    with pytest.raises(TypeError):
        cv.evaluate_squares(np.zeros((1, 64, 64), np.uint8))


# ---- the host form against torch in float64 -----------------------------------------------------------------------------------------
def test_host_records_on_crafted_rows():
    x, t = crafted_rows()
    s = evaluation.square_records(x, t)
    check_against_torch(s, x, t, "crafted")
    assert s.rank[0] == 12 - 4 and s.predicted[0] == 0                         # all equal
    assert s.rank[1] == 1 and s.predicted[1] == 3 and bool(s.correct[1])       # tie at the top: class 9 sorts above class 3 ...
    assert s.rank[2] == 0 and s.predicted[2] == 3 and not bool(s.correct[2])   # ... though the arg-max is the first maximum
    assert s.rank[3] == 12 and s.rank[4] == 6
    assert s.rank[5] == 13 and s.flags[5] == 1 and np.isnan(s.loss[5]) and np.isnan(s.confidence[5]) and not bool(s.correct[5])
    assert s.rank[6] == -1 and s.flags[6] == 1 and s.predicted[6] == 0         # the scan never leaves a NaN in column 0
    assert s.rank[7] == -1 and np.isnan(s.loss[7]) and np.isfinite(s.confidence[7])
    assert s.loss[8] == 80.0 and s.confidence[8] == 1.0 and s.loss[9] == 0.0 and s.rank[8] == 12 and s.rank[9] == 0
    assert all(getattr(s, k).dtype == np.float32 for k in ("confidence", "loss", "max_logit", "logsumexp"))


def test_host_records_on_random_rows():
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((1000, 13)) * rng.choice([0.5, 3.0, 12.0], (1000, 1))).astype(np.float32)
    x[::7, 4] = x[::7, 10]                                     # a tie in every seventh row
    t = rng.integers(0, 13, 1000)
    t[::13] = -1
    check_against_torch(evaluation.square_records(x, t), x, t, "random")


# ---- cv_square_records_finish against validate() ------------------------------------------------------------------------------------
def records_of(scores):
    rec = np.zeros(len(scores.loss), hip_backend.SQUARE_RECORD)
    for k in hip_backend.SQUARE_RECORD.names:
        rec[k] = getattr(scores, k)
    return rec


@pytest.mark.parametrize("batch_size", [512, 64, 1, 0])
@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "unlabelled+nan"])
def test_finish_matches_validate(batch_size, dirty):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((130, 13)) * 4).astype(np.float32)
    t = rng.integers(0, 13, 130)
    x[np.arange(0, 130, 2), t[::2]] += 6                       # about half of the rows are right
    if dirty:
        t[[3, 64, 65, 129]] = -1
        x[17, 2] = np.nan
    s = evaluation.square_records(x, t)
    got = hip_backend.square_records_finish(records_of(s), batch_size)
    nan_row = (s.flags & 1) != 0
    val_loss, val_acc, total, correct, batches = validate_restated(s.loss, s.predicted, s.label, nan_row, batch_size)
    assert got["n"] == 130 and got["n_labelled"] == total and got["n_correct"] == correct and got["n_nan"] == int(nan_row.sum())
    assert got["val_acc"] == val_acc
    labelled = s.label >= 0
    assert got["n_batches"] == batches
    if not dirty:
        assert batches == (1 if batch_size in (0, 512) else -(-130 // batch_size))
    if dirty:                                                  # a labelled NaN row: torch's mean is NaN, so is this one
        assert np.isnan(val_loss) and np.isnan(got["val_loss"]) and np.isnan(got["loss_sum"])
    else:
        assert got["val_loss"] == pytest.approx(val_loss, rel=1e-12)
        assert got["loss_sum"] == pytest.approx(float(s.loss[labelled].astype(np.float64).sum()), rel=1e-12)
    assert got["hits"].tolist() == [int((labelled & (s.rank < k)).sum()) for k in range(1, 14)]
    confusion = np.zeros((13, 13), np.int64)
    np.add.at(confusion, (s.label[labelled], s.predicted[labelled]), 1)
    assert np.array_equal(got["confusion"], confusion) and confusion.sum() == total


def test_finish_without_the_nan_row_is_finite_with_unlabelled_rows():
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((130, 13)) * 4).astype(np.float32)
    t = rng.integers(0, 13, 130)
    t[64:128] = -1                                             # a whole batch of 64 without a label: skipped, not a 0 / 0
    s = evaluation.square_records(x, t)
    got = hip_backend.square_records_finish(records_of(s), 64)
    val_loss, val_acc, total, _, _ = validate_restated(s.loss, s.predicted, s.label, (s.flags & 1) != 0, 64)
    assert got["n_batches"] == 2 and got["n_labelled"] == total == 66
    assert got["val_loss"] == pytest.approx(val_loss, rel=1e-12) and got["val_acc"] == val_acc


# ---- the fixture --------------------------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_generator_printed():
    assert FIXTURE.stat().st_size < 1 << 20
    with np.load(FIXTURE) as z:
        assert sorted(z.files) == ["labels", "squares"]
        sq, lab = z["squares"], z["labels"]
    assert sq.shape == (130, 64, 64) and sq.dtype == np.uint8 and lab.shape == (130,) and lab.dtype == np.int8
    assert np.bincount(lab).tolist() == [10] * 13 and np.array_equal(lab, np.repeat(np.arange(13), 10))
    assert int(sq.sum(dtype=np.int64)) == 70377663 and int(sq.min()) == 0 and int(sq.max()) == 255
    assert zlib.crc32(sq.tobytes()) == 2813533530
    assert f"{sq.mean() / 255:.6f}" == "0.518312" and f"{sq.std() / 255:.6f}" == "0.241550"
    assert [int(sq[lab == c].sum(dtype=np.int64)) for c in range(13)] == [
        5613319, 5702870, 6318618, 6511374, 5913675, 5234425, 5168620, 5513048, 4917168, 4951598, 4824162, 3849440, 5859346]
    # the normalised range the f16-family stems must hold: |x| <= 2.30 for the training constants
    mean, std = constants.CLASSIFIER_NORMALIZATION
    lo, hi = (0 / 255 - mean) / std, (255 / 255 - mean) / std
    assert max(abs(lo), abs(hi)) < 2.30 and max(abs(lo), abs(hi)) * 128 < 65504

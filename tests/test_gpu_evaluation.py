"""Ground-truth scores on the device: ``segmentation_scores_kernel`` through ``HipEngine.segmentation_scores`` against the float64
oracle ``tests/evaluation_ref.py``, its agreement with the UNet's own mask and with the quality kernel, its argument errors, and
``ChessVision.evaluate_images`` end to end.

Measured on MI355X, worst error / bar over every case of ``test_kernel_matches_the_oracle``: bce_sum 0.044, sig_sum 0.271,
sig_label_sum 0.271, loss 0.025 (profiles/evaluation.md)."""
from __future__ import annotations

import ctypes
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import evaluation_ref as ref
from chessvision import ChessVision, evaluation, hip_backend, synthetic

pytestmark = pytest.mark.gpu

# the smallest set that reaches an empty body, a head and a tail, per-image misalignment of the float and the byte stream (odd count:
# image 1 starts 4 bytes past a 16-byte boundary and 3 bytes past a 4-byte one), and the real shape
SHAPES = [(1, 1), (1, 4), (3, 1000), (2, 4099), (5, 65536), (2, 65536 + 4)]
SUM_REL = 1e-6             # four times the ~2.4e-7 a float32 term (a sum of non-negative parts, a few ulp each) can be off by
PHOTOS = [Path(__file__).resolve().parent / "golden" / f"photos8_{i}.npz" for i in range(8)]


def _clear_of_half(x):
    """Every logit with 0 < |x| < 1e-3 moves to +-1e-3: no pixel sits where the float32 and the float64 sigmoid can disagree about
    ``> 0.5``, and none is left out of the comparison.  (An exact 0 stays: exp(-0) is exactly 1 and v exactly 0.5 in both.)"""
    near = (np.abs(x) < 1e-3) & (x != 0)
    x[near] = np.where(x[near] < 0, np.float32(-1e-3), np.float32(1e-3))
    return x


def _with_nan(rng, n, c):
    x = rng.normal(0, 6, (n, c)).astype(np.float32)
    x[0, c // 3] = np.nan
    return x


LOGITS = {
    "normal": lambda rng, n, c: rng.normal(0, 6, (n, c)).astype(np.float32),
    "all_negative": lambda rng, n, c: (-5 * rng.random((n, c)) - 0.1).astype(np.float32),
    "large_magnitude": lambda rng, n, c: np.where(rng.random((n, c)) < 0.5, np.float32(-80), np.float32(80)).astype(np.float32),
    "constant_zero": lambda rng, n, c: np.zeros((n, c), np.float32),
    "one_nan": _with_nan,
}
LABELS = {
    "random_40_percent": lambda rng, n, c: np.where(rng.random((n, c)) < 0.4, 255, 0).astype(np.uint8),
    "all_zero": lambda rng, n, c: np.zeros((n, c), np.uint8),
    "all_255": lambda rng, n, c: np.full((n, c), 255, np.uint8),
    "bytes_0_1_7_255": lambda rng, n, c: np.array([0, 1, 7, 255], np.uint8)[rng.integers(0, 4, (n, c))],
}
WORST = {"bce_sum": 0.0, "sig_sum": 0.0, "sig_label_sum": 0.0, "loss": 0.0}


def _close(got, want, rel):
    if math.isnan(want):
        return math.isnan(got), 0.0
    err = abs(got - want)
    bar = rel * abs(want)
    return err <= bar, (err / bar if bar else (0.0 if err == 0 else math.inf))


def _check(eng, logits, labels, offset=0):
    """One launch against the oracle.  ``offset``: both device buffers start that many elements into their allocations."""
    n, count = logits.shape
    lg_base = torch.empty(n * count + offset, dtype=torch.float32, device=eng.device)
    lb_base = torch.empty(n * count + offset, dtype=torch.uint8, device=eng.device)
    lg, lb = lg_base[offset:].view(n, count), lb_base[offset:].view(n, count)
    lg.copy_(torch.from_numpy(logits))
    lb.copy_(torch.from_numpy(labels))
    rec, scores = eng.segmentation_scores(lg, lb, 0.5)
    rec2, _ = eng.segmentation_scores(lg, lb, 0.5)
    assert rec.tobytes() == rec2.tobytes()                                   # bit-identical run to run
    assert rec.shape == (n,) and not rec["reserved"].any() and (rec["count"] == count).all()
    if count >= 4:                                                           # the quality kernel's contract starts at 4 values
        q, _, _, half = eng.extraction_scores(lg, transform="sigmoid", want_mask=True)
        assert np.array_equal(rec["n_pred"], q["above_half"])
        assert np.array_equal(rec["n_both"], np.count_nonzero((half != 0) & (labels != 0), axis=1))
    for i in range(n):
        want = ref.seg_sums(logits[i], labels[i], 0.5)
        for key in ("n_label", "n_pred", "n_both", "n_nan", "count"):
            assert rec[key][i] == want[key], (i, key, rec[key][i], want[key])
        for key in ("bce_sum", "sig_sum", "sig_label_sum"):
            ok, ratio = _close(float(rec[key][i]), want[key], SUM_REL)
            WORST[key] = max(WORST[key], ratio)
            assert ok, (i, key, float(rec[key][i]), want[key], ratio)
        fin = ref.seg_finish(want)
        if math.isnan(fin["loss"]):
            assert math.isnan(scores["loss"][i]) and math.isnan(scores["bce"][i]) and math.isnan(scores["dice_loss"][i])
        else:
            bar = 2e-6 + 1e-6 * fin["bce"]
            err = abs(scores["loss"][i] - fin["loss"])
            WORST["loss"] = max(WORST["loss"], err / bar)
            assert err <= bar, (i, scores["loss"][i], fin["loss"])
        for key in ("dice", "iou", "pixel_accuracy"):                        # functions of the (exact) counts
            assert scores[key][i] == fin[key], (i, key)


@pytest.mark.parametrize("kind", list(LOGITS))
def test_kernel_matches_the_oracle(engines, kind):
    rng = np.random.default_rng(100 + sorted(LOGITS).index(kind))
    for n, count in SHAPES:
        x = _clear_of_half(LOGITS[kind](rng, n, count))
        for lab in LABELS:
            _check(engines["f32"], x, LABELS[lab](rng, n, count))
    print(f"segmentation scores [{kind}], worst error / bar so far: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


def test_kernel_on_buffers_that_start_off_a_16_byte_boundary(engines):
    rng = np.random.default_rng(7)
    for offset in (1, 2, 3):                                                 # image 0 itself has a head; the label bytes start unaligned
        for n, count in [(3, 1000), (2, 4099), (1, 2)]:
            x = _clear_of_half(LOGITS["normal"](rng, n, count))
            _check(engines["f32"], x, LABELS["bytes_0_1_7_255"](rng, n, count), offset=offset)


def test_nan_images_have_nan_sums_and_exact_counts(engines):
    rng = np.random.default_rng(8)
    x = _clear_of_half(rng.normal(0, 6, (3, 4099)).astype(np.float32))
    labels = LABELS["random_40_percent"](rng, 3, 4099)
    labels[0, 17], labels[2, 4098] = 0, 255
    x[0, 17] = np.nan                                                        # an unlabelled pixel and a labelled one (the last, in the tail)
    x[2, 4098] = np.nan
    rec, scores = engines["f32"].segmentation_scores(torch.from_numpy(x).to(engines["f32"].device),
                                                     torch.from_numpy(labels).to(engines["f32"].device))
    assert rec["n_nan"].tolist() == [1, 0, 1]
    for i in (0, 2):
        assert math.isnan(rec["bce_sum"][i]) and math.isnan(rec["sig_sum"][i]) and math.isnan(rec["sig_label_sum"][i])
        assert math.isnan(scores["loss"][i]) and math.isfinite(scores["dice"][i])
        want = ref.seg_sums(x[i], labels[i])
        assert (rec["n_label"][i], rec["n_pred"][i], rec["n_both"][i]) == (want["n_label"], want["n_pred"], want["n_both"])
    assert math.isfinite(rec["bce_sum"][1]) and math.isfinite(scores["loss"][1])


def test_argument_errors(engines):
    eng = engines["f32"]
    lib = eng._lib
    x = torch.zeros(4, 16, dtype=torch.float32, device=eng.device)
    lab = torch.zeros(4, 16, dtype=torch.uint8, device=eng.device)
    rec = torch.zeros(4, 64, dtype=torch.uint8, device=eng.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    X, L, R = x.data_ptr(), lab.data_ptr(), rec.data_ptr()
    cases = {
        "null logits": (eng._h, None, L, 4, 16, 0.5, R),
        "null labels": (eng._h, X, None, 4, 16, 0.5, R),
        "null records": (eng._h, X, L, 4, 16, 0.5, None),
        "count = 0": (eng._h, X, L, 4, 0, 0.5, R),
        "count too large": (eng._h, X, L, 1, (1 << 24) + 1, 0.5, R),
        "n = 0": (eng._h, X, L, 0, 16, 0.5, R),
        "NaN threshold": (eng._h, X, L, 4, 16, math.nan, R),
        "infinite threshold": (eng._h, X, L, 4, 16, math.inf, R),
        "misaligned logits": (eng._h, X + 2, L, 4, 15, 0.5, R),
        "misaligned records": (eng._h, X, L, 4, 16, 0.5, R + 4),
    }
    for name, args in cases.items():
        assert lib.cv_segmentation_scores(*args, stream) == 1, name                          # CV_ERR_INVALID
        assert b"cv_segmentation_scores" in lib.cv_last_error(), name
    assert lib.cv_segmentation_scores(None, X, L, 4, 16, 0.5, R, stream) == 1                # null engine
    with pytest.raises(hip_backend.HipBackendError):
        eng.segmentation_scores_dev(x, lab[:, :15])
    with pytest.raises(hip_backend.HipBackendError):
        eng.segmentation_scores_dev(x, lab.float())
    with pytest.raises(hip_backend.HipBackendError):
        eng.segmentation_scores_dev(x.cpu(), lab)
    with pytest.raises(hip_backend.HipBackendError):
        eng.segmentation_scores_dev(x.t(), lab.t())                                          # not contiguous
    with pytest.raises(hip_backend.HipBackendError):
        eng.segmentation_scores_dev(x, lab, threshold=math.nan)
    torch.cuda.synchronize(eng.device)
    assert not rec.cpu().numpy().any()                                                       # nothing was launched


# ---- the pipeline --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cv_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("weights_evaluation")
    pe, pc = synthetic.save_checkpoints(d, segmenting=True)
    return ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))


@pytest.mark.parametrize("threshold", [0.3, 0.7])
def test_n_pred_is_the_unet_masks_pixel_count(cv_model, threshold):
    _ = cv_model.board_extractor
    eng = cv_model._get_engine("unet")
    photos = torch.from_numpy(np.stack([synthetic.board_photo(40 + s) for s in range(3)])).to(eng.device)
    logits, mask = eng.unet_forward_u8(eng.resize_area_u8(photos, (256, 256)), threshold=threshold)
    labels = (torch.rand(3, 256, 256, device=eng.device) < 0.5).to(torch.uint8)
    rec, _ = eng.segmentation_scores(logits, labels, threshold)
    mask, labels = mask.cpu().numpy(), labels.cpu().numpy()
    assert rec["n_pred"].tolist() == [int(np.count_nonzero(m)) for m in mask]
    assert rec["n_both"].tolist() == [int(np.count_nonzero((m != 0) & (t != 0))) for m, t in zip(mask, labels)]
    assert 0 < rec["n_pred"].min() and rec["n_pred"].max() < 65536                           # a real mask, not an empty or full one


def _rand_fen(rng):
    rows = []
    for _ in range(8):
        row, empty = "", 0
        for c in rng.integers(0, 26, 8):
            if c >= 12:
                empty += 1
                continue
            row += (str(empty) if empty else "") + "BKNPQRbknpqr"[c]
            empty = 0
        rows.append(row + (str(empty) if empty else ""))
    return "/".join(rows)


def _same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        xe, ye = x.board_extraction, y.board_extraction
        for p, q in ((xe.probabilities, ye.probabilities), (xe.binary_mask, ye.binary_mask), (xe.quadrangle, ye.quadrangle),
                     (xe.board_image, ye.board_image)):
            assert (p is None) == (q is None) and (p is None or (p.dtype == q.dtype and np.array_equal(p, q)))
        assert (x.position is None) == (y.position is None) and x.quality is None and y.quality is None
        if x.position is not None:
            xp, yp = x.position, y.position
            assert (xp.fen, xp.original_fen, xp.square_names, xp.validation_fixes) == (yp.fen, yp.original_fen, yp.square_names, yp.validation_fixes)
            assert np.array_equal(xp.model_probabilities, yp.model_probabilities) and np.array_equal(xp.squares, yp.squares)


def _check_report(report, fens, masks, flip, threshold=0.5):
    """Every record of the report against the restatements, from the report's own results."""
    assert len(report.results) == len(report.evaluations) == len(fens)
    for i, (res, ev) in enumerate(zip(report.results, report.evaluations)):
        ext = res.board_extraction
        if masks[i] is None:
            assert ev.segmentation is None
        else:
            got, want = ev.segmentation, ref.seg_scores(ext.probabilities, masks[i], threshold)
            assert all(type(getattr(got, k)) is float for k in want)
            assert abs(got.bce - want["bce"]) <= 1e-6 * want["bce"]
            assert abs(got.dice_loss - want["dice_loss"]) <= 2e-6               # both sums of the quotient within 1e-6 relative, Dice <= 1
            assert abs(got.loss - want["loss"]) <= 2e-6 + 1e-6 * want["bce"]
            pred, lab = ext.binary_mask != 0, masks[i] != 0                     # the hard counts are those of the result's own mask
            hard = ref.seg_finish({"count": 65536, "n_label": int(lab.sum()), "n_pred": int(pred.sum()), "n_both": int((pred & lab).sum()),
                                   "bce_sum": 0.0, "sig_sum": 1.0, "sig_label_sum": 0.0})
            assert (got.dice, got.iou, got.pixel_accuracy) == (hard["dice"], hard["iou"], hard["pixel_accuracy"])
        assert ev.extraction_failed == (fens[i] is not None and res.position is None)
        if fens[i] is None or res.position is None:
            assert ev.position is None
            continue
        pos, got = res.position, ev.position
        want = evaluation.position_scores(pos.model_probabilities, pos.fen, pos.original_fen, fens[i], len(pos.validation_fixes), flip)
        assert got.top_k == want.top_k and (got.top_1, got.top_2, got.top_3) == want.top_k
        assert (got.accuracy_original, got.accuracy_validated, got.num_fixes) == (want.accuracy_original, want.accuracy_validated, want.num_fixes)
        assert got.accuracy_original == ref.position_accuracy(pos.original_fen, fens[i])
        assert got.accuracy_validated == ref.position_accuracy(pos.fen, fens[i])
        for name in ("true_labels", "predicted_labels", "validated_labels", "rank", "confidence"):
            a, b = getattr(got, name), getattr(want, name)
            assert a.dtype == b.dtype and np.array_equal(a, b), (i, name)
        np.testing.assert_allclose(got.loss, want.loss, rtol=0, atol=1e-12)
        assert abs(got.mean_loss - want.mean_loss) <= 1e-12
        # independently of the package: the true piece on square_names[row], through the loop oracle
        true_a8h1 = ref.fen_indices(fens[i])
        rows = [true_a8h1[(8 - int(nm[1])) * 8 + "abcdefgh".index(nm[0])] for nm in pos.square_names]
        assert pos.square_names[0] == ("h1" if flip else "a8") and got.true_labels.tolist() == rows
        loop = ref.board_scores(pos.model_probabilities, rows)
        assert got.rank.tolist() == loop["rank"] and got.top_k == tuple(h / 64 for h in loop["hits"][:3])
        assert got.predicted_labels.tolist() == loop["predicted"]
    agg = report.aggregate
    again = evaluation.aggregate(report.evaluations, [r.processing_time for r in report.results])
    assert set(agg) == set(again) and all(np.array_equal(agg[k], again[k], equal_nan=True) for k in agg)
    scored = [e.position for e in report.evaluations if e.position is not None]
    assert agg["extraction_failures"] == sum(1 for f, r in zip(fens, report.results) if f is not None and r.position is None)
    assert agg["validation_fixes"] == sum(p.num_fixes for p in scored)
    if scored:
        assert agg["top_1_accuracy"] == sum(p.accuracy_original for p in scored) / len(scored)
        assert agg["top_3_accuracy"] == sum(p.top_k[2] for p in scored) / len(scored)
    seg = [e.segmentation for e in report.evaluations if e.segmentation is not None]
    if seg:
        assert agg["mean_loss"] == sum(s.loss for s in seg) / len(seg) and agg["mean_dice"] == sum(s.dice for s in seg) / len(seg)
    else:
        assert math.isnan(agg["mean_loss"]) and math.isnan(agg["mean_iou"])


@pytest.fixture(scope="module")
def six_images():
    """Two shapes A A B A A B with pipeline_chunk=2: jobs [0,1] [3,4] [2,5], so results are scattered back over the caller's order."""
    rng = np.random.default_rng(21)
    images = [synthetic.board_photo(700 + s) for s in range(6)]
    for k in (2, 5):
        images[k] = np.ascontiguousarray(images[k][:384])
    fens = [_rand_fen(rng) for _ in range(6)]
    fens[4] = None
    yy, xx = np.mgrid[:256, :256]
    masks = [np.where((yy > 40 + 9 * k) & (yy < 215) & (xx > 30) & (xx < 200 + 8 * k), 255, 0).astype(np.uint8) for k in range(6)]
    masks[1] = masks[5] = None
    masks[3] = np.where(masks[3] != 0, 1, 0).astype(np.uint8)                   # "board" is any non-zero byte
    return images, fens, masks


@pytest.mark.parametrize("flip", [False, True])
def test_evaluate_images_end_to_end(cv_model, six_images, flip):
    images, fens, masks = six_images
    kw = dict(flip=flip, fallback_quad=True, pipeline_chunk=2)
    timings = {}
    report = cv_model.evaluate_images(images, true_fens=fens, label_masks=masks, timings=timings, **kw)
    assert isinstance(report, evaluation.EvaluationReport) and timings["jobs"] == 3
    assert timings["seg_ms"] > 0 and timings["evaluation"] > 0
    plain_timings = {}
    plain = cv_model.process_images(images, timings=plain_timings, **kw)
    _same_results(report.results, plain)
    assert "seg_ms" not in plain_timings and "evaluation" not in plain_timings   # without ground truth nothing new runs
    assert all(r.position is not None for r in report.results)
    assert sum(e.segmentation is not None for e in report.evaluations) == 4 and sum(e.position is not None for e in report.evaluations) == 5
    _check_report(report, fens, masks, flip)
    again = cv_model.evaluate_images(images, true_fens=fens, label_masks=masks, **kw)
    assert [e.segmentation for e in again.evaluations] == [e.segmentation for e in report.evaluations]      # bit-identical run to run


def test_only_one_kind_of_ground_truth(cv_model, six_images):
    images, fens, masks = six_images
    kw = dict(fallback_quad=True, pipeline_chunk=2)
    timings = {}
    only_fens = cv_model.evaluate_images(images, true_fens=fens, timings=timings, **kw)
    assert "seg_ms" not in timings                                              # no label mask: no kernel, no copy
    assert all(e.segmentation is None for e in only_fens.evaluations)
    _check_report(only_fens, fens, [None] * 6, False)
    only_masks = cv_model.evaluate_images(images, label_masks=masks, threshold=0.3, **kw)
    assert all(e.position is None and not e.extraction_failed for e in only_masks.evaluations)
    _check_report(only_masks, [None] * 6, masks, False, threshold=0.3)
    _same_results(only_masks.results, cv_model.process_images(images, threshold=0.3, **kw))


def test_a_blank_photo_with_a_fen_is_an_extraction_failure(cv_model):
    blank = np.random.default_rng(1003).integers(0, 60, (512, 512, 3), dtype=np.uint8)
    images = [synthetic.board_photo(300), blank, synthetic.board_photo(301)]
    fens = ["rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR"] * 3
    masks = [None, np.zeros((256, 256), np.uint8), None]
    report = cv_model.evaluate_images(images, true_fens=fens, label_masks=masks)                # no fallback quadrangle
    assert report.results[1].position is None
    ev = report.evaluations[1]
    assert ev.extraction_failed and ev.position is None and ev.segmentation is not None
    found = [e for e in report.evaluations if e.position is not None]
    assert report.aggregate["extraction_failures"] == 3 - len(found) >= 1
    if found:                                                                   # the mean runs over the boards that were found
        assert report.aggregate["top_1_accuracy"] == sum(e.position.accuracy_original for e in found) / len(found)
    else:
        assert math.isnan(report.aggregate["top_1_accuracy"])
    _check_report(report, fens, masks, False)


def test_real_photos_with_their_ground_truth(cv_model):
    """The eight fixtures with their FENs; random weights, so the values mean nothing -- the bookkeeping does."""
    photos = [np.ascontiguousarray(np.load(p)["bgr"][0]) for p in PHOTOS]
    fens = [str(np.load(p)["fen"][0]) for p in PHOTOS]
    rng = np.random.default_rng(31)
    masks = [np.where(rng.random((256, 256)) < 0.3, 255, 0).astype(np.uint8) if k % 2 else None for k in range(8)]
    report = cv_model.evaluate_images(photos, true_fens=fens, label_masks=masks, fallback_quad=True, pipeline_chunk=3)
    assert all(e.position is not None for e in report.evaluations)
    _check_report(report, fens, masks, False)
    _same_results(report.results, cv_model.process_images(photos, fallback_quad=True, pipeline_chunk=3))

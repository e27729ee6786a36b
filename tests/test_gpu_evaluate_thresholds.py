"""``ChessVision.evaluate_thresholds`` against ``evaluate_images`` at each threshold, on the same instance: the contract of DESIGN.md
section 4 field by field, the curve, the number of boards actually classified, shared arrays, the options, and no leaked state."""
from __future__ import annotations

import math

import numpy as np
import pytest

from chessvision import ChessVision, evaluation, synthetic

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.7, 0.3, 0.5)                                  # the caller's order is not the ascending one
PROB_BAR = 1e-4                                              # the cross-batch contract


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


@pytest.fixture(scope="module")
def cv_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("weights_evaluate_thresholds")
    pe, pc = synthetic.save_checkpoints(d, segmenting=True)
    return ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))


@pytest.fixture(scope="module")
def data():
    """20 photos, with ``pipeline_chunk=16`` one 16-image job and one 4-image job; a FEN for every photo, a label mask for every other one."""
    rng = np.random.default_rng(77)
    images = [synthetic.board_photo(900 + s) for s in range(20)]
    fens = [_rand_fen(rng) for _ in range(20)]
    yy, xx = np.mgrid[:256, :256]
    masks = [np.where((yy > 40 + 3 * k) & (yy < 215) & (xx > 45) & (xx < 200 + 2 * k), 255, 0).astype(np.uint8) if k % 2 == 0 else None
             for k in range(20)]
    return images, fens, masks


@pytest.fixture(scope="module")
def runs(cv_model, data):
    """The sweep and the three single calls, once for the module; nothing below changes them."""
    images, fens, masks = data
    before = cv_model.process_images(images[:4])
    timings = {}
    sweep = cv_model.evaluate_thresholds(images, THRESHOLDS, true_fens=fens, label_masks=masks, pipeline_chunk=16, timings=timings)
    after = cv_model.process_images(images[:4])
    single_timings = {}
    singles = {t: cv_model.evaluate_images(images, true_fens=fens, label_masks=masks, threshold=t, pipeline_chunk=16,
                                           timings=single_timings if t == 0.5 else None) for t in THRESHOLDS}
    return sweep, singles, timings, single_timings, before, after


def _same_array(a, b):
    return (a is None) == (b is None) and (a is None or (a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)))


def _check_contract(got, want):
    """One threshold's report of the sweep against ``evaluate_images`` at that threshold."""
    assert len(got.results) == len(want.results) == len(got.evaluations)
    for i, (g, w) in enumerate(zip(got.results, want.results)):
        ge, we = g.board_extraction, w.board_extraction
        assert _same_array(ge.probabilities, we.probabilities), i            # the logits, bit for bit
        assert _same_array(ge.binary_mask, we.binary_mask), i
        assert _same_array(ge.quadrangle, we.quadrangle), i                  # including the found / not-found pattern
        assert _same_array(ge.board_image, we.board_image), i
        assert (g.position is None) == (w.position is None), i
        assert g.quality is None and g.processing_time > 0
        if g.position is not None:
            gp, wp = g.position, w.position
            assert _same_array(gp.squares, wp.squares), i
            err = float(np.abs(gp.model_probabilities - wp.model_probabilities).max())
            assert err <= PROB_BAR, (i, err)
            assert (gp.fen, gp.original_fen, gp.square_names, gp.validation_fixes) == (wp.fen, wp.original_fen, wp.square_names, wp.validation_fixes)
        gv, wv = got.evaluations[i], want.evaluations[i]
        assert gv.segmentation == wv.segmentation, i                         # all six fields, bit for bit
        assert gv.extraction_failed == wv.extraction_failed and (gv.position is None) == (wv.position is None)
        if gv.position is not None:
            a, b = gv.position, wv.position
            assert (a.top_k, a.accuracy_original, a.accuracy_validated, a.num_fixes) == (b.top_k, b.accuracy_original, b.accuracy_validated, b.num_fixes)
            for name in ("true_labels", "predicted_labels", "validated_labels", "rank"):
                assert np.array_equal(getattr(a, name), getattr(b, name)), (i, name)
            assert abs(a.mean_loss - b.mean_loss) <= 1e-4 * abs(b.mean_loss)
    _check_aggregate(got.aggregate, want.aggregate)


def _check_aggregate(got, want):
    assert set(got) == set(want)
    for key, w in want.items():
        if key == "avg_time_per_prediction":
            continue
        g = got[key]
        if isinstance(w, int) or key.startswith("top_"):                     # counts and square accuracies: equal
            assert g == w or (math.isnan(g) and math.isnan(w)), key
        else:
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-4 * abs(w), key


def test_every_threshold_is_evaluate_images_at_that_threshold(runs):
    sweep, singles = runs[0], runs[1]
    assert isinstance(sweep, evaluation.ThresholdSweepReport) and sweep.thresholds == list(THRESHOLDS) and len(sweep.reports) == 3
    for j, t in enumerate(THRESHOLDS):
        assert sweep.at(t) is sweep.reports[j]
        _check_contract(sweep.at(t), singles[t])
    assert sum(e.segmentation is not None for e in sweep.at(0.5).evaluations) == 10
    assert any(r.position is not None for r in sweep.at(0.5).results)        # the photos are found: the comparison is not empty
    with pytest.raises(KeyError):
        sweep.at(0.4)


def test_curve_is_the_three_aggregates(runs):
    sweep, singles = runs[0], runs[1]
    assert set(sweep.curve) == (set(singles[0.5].aggregate) - {"avg_time_per_prediction"}) | {"mean_pixel_accuracy"}
    for j, t in enumerate(THRESHOLDS):
        point = {key: values[j] for key, values in sweep.curve.items() if key != "mean_pixel_accuracy"}
        for key, v in point.items():                                         # the sweep's own reports, exactly
            w = sweep.reports[j].aggregate[key]
            assert v == w or (math.isnan(v) and math.isnan(w)), key
        _check_aggregate({**point, "avg_time_per_prediction": 0.0}, singles[t].aggregate)
        pa = [e.segmentation.pixel_accuracy for e in singles[t].evaluations if e.segmentation is not None]
        assert sweep.curve["mean_pixel_accuracy"][j] == sum(pa) / len(pa)
    best = sweep.best()
    top = sweep.curve["top_1_accuracy"]
    assert best == THRESHOLDS[[v == max(top) for v in top].index(True)]


def test_boards_classified_is_the_number_of_distinct_quadrangles(runs):
    sweep, singles = runs[0], runs[1]
    quads = [[r.board_extraction.quadrangle for r in singles[t].results] for t in sorted(THRESHOLDS)]
    distinct, _, groups = evaluation.plan_threshold_groups(quads)
    assert sweep.boards_classified == sum(len(d) for d in distinct)
    assert sweep.boards_found == sum(q is not None for row in quads for q in row)
    assert sweep.boards_classified <= sweep.boards_found and len(groups) <= 3
    # thresholds that found the same quadrangle share the board, the crops and the probabilities; the logits are always shared
    for i in range(20):
        res = [sweep.at(t).results[i] for t in sorted(THRESHOLDS)]
        assert res[0].board_extraction.probabilities is res[1].board_extraction.probabilities is res[2].board_extraction.probabilities
        for a, b in ((0, 1), (1, 2), (0, 2)):
            qa, qb = quads[a][i], quads[b][i]
            if qa is not None and qb is not None and np.array_equal(qa, qb):
                assert res[a].position.model_probabilities is res[b].position.model_probabilities
                assert res[a].board_extraction.board_image is res[b].board_extraction.board_image


def test_timings_and_no_leaked_state(runs):
    _, _, timings, single_timings, before, after = runs
    assert set(single_timings) <= set(timings) and timings["jobs"] == 2 and timings["levels_ms"] > 0 and timings["seg_ms"] > 0
    for b, a in zip(before, after):
        assert _same_array(b.board_extraction.probabilities, a.board_extraction.probabilities)
        assert _same_array(b.board_extraction.binary_mask, a.board_extraction.binary_mask)
        assert _same_array(b.board_extraction.board_image, a.board_extraction.board_image)
        assert (b.position is None) == (a.position is None)
        if b.position is not None:
            assert b.position.fen == a.position.fen and np.array_equal(b.position.model_probabilities, a.position.model_probabilities)


def test_two_neighbouring_thresholds_share_every_board(cv_model, data, runs):
    images, fens, masks = data
    cuts = (0.5, 0.5000001)
    assert np.float32(cuts[0]) < np.float32(cuts[1])
    logits = [r.board_extraction.probabilities for r in runs[0].at(0.5).results]
    # no logit between the two cuts: sigmoid(x) - 0.5 ~ x / 4, the cuts are 1.2e-7 apart, so |x| > 1e-5 leaves both exps room to spare
    chosen = [i for i in range(20) if np.abs(logits[i]).min() > 1e-5][:4]
    assert len(chosen) == 4
    for i in chosen:
        assert np.abs(logits[i]).min() > 1e-5
    sub = lambda seq: [seq[i] for i in chosen]               # noqa: E731
    sweep = cv_model.evaluate_thresholds(sub(images), cuts, true_fens=sub(fens), label_masks=sub(masks))
    a, b = sweep.at(cuts[0]), sweep.at(cuts[1])
    found = sum(r.position is not None for r in a.results)
    assert found > 0 and sweep.boards_classified == found and sweep.boards_found == 2 * found
    for x, y in zip(a.results, b.results):
        assert np.array_equal(x.board_extraction.binary_mask, y.board_extraction.binary_mask)
        assert (x.position is None) == (y.position is None)
        if x.position is not None:
            assert x.position.model_probabilities is y.position.model_probabilities
    assert [e.segmentation for e in a.evaluations] == [e.segmentation for e in b.evaluations]


@pytest.mark.parametrize("option", ["flip", "fallback_quad", "antialias"])
def test_options_follow_evaluate_images(cv_model, data, option):
    images, fens, masks = data
    blank = np.random.default_rng(1003).integers(0, 60, (512, 512, 3), dtype=np.uint8)       # no board: the fallback has work to do
    images, fens, masks = images[:4] + [blank], fens[:5], masks[:5]
    kw = {"flip": True} if option == "flip" else {"fallback_quad": True} if option == "fallback_quad" else {}
    try:
        if option == "antialias":
            cv_model.evaluation_resize = "antialias"
        sweep = cv_model.evaluate_thresholds(images, (0.6, 0.4), true_fens=fens, label_masks=masks, **kw)
        want = cv_model.evaluate_images(images, true_fens=fens, label_masks=masks, threshold=0.6, **kw)
    finally:
        if option == "antialias":
            del cv_model.evaluation_resize                   # back to the class default
    assert cv_model.evaluation_resize == "area"
    _check_contract(sweep.at(0.6), want)
    if option == "fallback_quad":
        assert all(r.position is not None for r in sweep.at(0.6).results) and sweep.boards_found == 10
    if option == "flip":
        assert all(r.position.square_names[0] == "h1" for r in sweep.at(0.6).results if r.position is not None)


def test_three_jobs_with_embeddings_follow_evaluate_images(cv_model, data):
    """Five photos in jobs of two: the third upload is gated and the first job retires behind the second one's classifier, with the
    embeddings of both networks riding in the holds of the shared steps."""
    images, fens, masks = (seq[:5] for seq in data)
    timings, single_timings = {}, {}
    try:
        cv_model.evaluation_embeddings = True
        sweep = cv_model.evaluate_thresholds(images, THRESHOLDS, true_fens=fens, label_masks=masks, pipeline_chunk=2, timings=timings)
        singles = {t: cv_model.evaluate_images(images, true_fens=fens, label_masks=masks, threshold=t, pipeline_chunk=2,
                                               timings=single_timings if t == 0.5 else None) for t in THRESHOLDS}
    finally:
        del cv_model.evaluation_embeddings                   # back to the class default
    assert cv_model.evaluation_embeddings is False
    for t in THRESHOLDS:
        _check_contract(sweep.at(t), singles[t])
        for g, w in zip(sweep.at(t).results, singles[t].results):
            assert g.embeddings.board_extractor is not None
            assert _same_array(g.embeddings.board_extractor, w.embeddings.board_extractor)       # bit for bit
            assert (g.embeddings.classifier is None) == (w.embeddings.classifier is None) == (g.position is None)
    for i in range(5):                                       # one UNet embedding per image, shared by its thresholds
        a, b, c = (sweep.at(t).results[i].embeddings.board_extractor for t in THRESHOLDS)
        assert a is b is c
    assert timings["jobs"] == 3 == single_timings["jobs"]
    assert set(timings) == set(single_timings) | {"levels_ms"}

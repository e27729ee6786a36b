"""GPU: BASELINE configs[3] end to end against an oracle-side pipeline (VERDICT r01 "next round" 1).

``ChessVision.process_images`` (device resize, fused u8 UNet entry with on-device threshold, C++ contours, fused device warp +
gray + flip + split, u8 classifier entry with on-device softmax, C++ FEN/pawn rule) versus ``oracle.pipeline_ref``: the
reference's per-image ``process_image`` order of operations with the oracle's torch-CPU UNet / ResNet-18 at the model seam
and the numpy restatements of the OpenCV stages (reference core.py:152-195, 309-355).  The UNet weights are random except
for one rewired channel that makes the network segment bright quadrilaterals (chessvision/synthetic.py: make_segmenting), so
masks have real contours and most boards are found the way they would be with a trained checkpoint; the rest go through
``fallback_quad``.  Asserted per board: masks equal outside |logit - logit(thr)| < 1e-4 (a board with a flipped pixel inside that band is continued
from the product's mask, not skipped), quadrangles identical, rectified boards IDENTICAL BYTE FOR BYTE (whole-image fallback
quadrangle included), probabilities within 1e-3, FEN / original FEN / validation fixes identical (squares whose top-2 margin is
inside the probability tolerance excepted).
The 256-board run is checked through size-independent properties and a sampled oracle comparison."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from chessvision import ChessVision, constants, synthetic
from oracle import pipeline_ref
from oracle.resnet_ref import ResNet18
from oracle.unet_ref import UNet

pytestmark = pytest.mark.gpu


def _oracle_models():
    usd = {k: torch.from_numpy(v) for k, v in synthetic.unet_state_dict(1, segmenting=True).items()}
    rsd = {k: torch.from_numpy(v) for k, v in synthetic.resnet18_state_dict(2).items()}
    unet, resnet = UNet(3, 1, False), ResNet18()
    unet.load_state_dict(usd, strict=False)
    resnet.load_state_dict(rsd, strict=False)
    return unet.eval(), resnet.eval()


@pytest.fixture(scope="module")
def cv_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("weights_e2e")
    pe, pc = synthetic.save_checkpoints(d, segmenting=True)
    return ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))


def _images(n, seed0=0):
    imgs = [synthetic.board_photo(seed0 + s) for s in range(n)]
    for k in range(0, n, 7):                              # every seventh: no board at all -> fallback quadrangle
        imgs[k] = np.random.default_rng(1000 + k).integers(0, 60, (512, 512, 3), dtype=np.uint8)
    return imgs


def _compare(got, ref, stats, resnet, image, flip=False, fallback_quad=True, logit_thr=0.0):
    ge, re_ = got.board_extraction, ref.board_extraction
    assert np.abs(ge.probabilities - re_.probabilities).max() <= 1e-3          # UNet logits, north_star bar
    unsure = np.abs(re_.probabilities - logit_thr) < 1e-4
    assert np.array_equal(ge.binary_mask[~unsure], re_.binary_mask[~unsure])
    if unsure.any() and not np.array_equal(ge.binary_mask, re_.binary_mask):
        # a mask pixel whose logit is within 1e-4 of the threshold flipped: the two contours may differ, so the oracle continues
        # from the PRODUCT's mask for this board -- everything downstream of the mask is still compared
        stats["mask_flips_inside_tolerance"] += 1
        ref = pipeline_ref.process_from_mask(resnet, image, ge.binary_mask, re_.probabilities, flip, fallback_quad)
        re_ = ref.board_extraction
    assert (ge.quadrangle is None) == (re_.quadrangle is None)
    assert (got.position is None) == (ref.position is None)
    if re_.quadrangle is not None:
        assert np.array_equal(ge.quadrangle, re_.quadrangle)
    if ref.position is None:
        return
    # byte work is bit-exact: device warp + gray + flip == the independent oracle's, fallback quadrangle (dyadic ties) included
    assert np.array_equal(ge.board_image, re_.board_image), (int(np.abs(ge.board_image.astype(int) - re_.board_image.astype(int)).max()),
                                                              float((ge.board_image != re_.board_image).mean()))
    stats["boards_identical"] = stats.get("boards_identical", 0) + 1
    gp, rp = got.position, ref.position
    perr = np.abs(gp.model_probabilities - rp.model_probabilities).max()
    assert perr <= 1e-3, perr
    stats["max_prob_err"] = max(stats["max_prob_err"], float(perr))
    top2 = np.sort(rp.model_probabilities, axis=1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 2e-3                                  # argmax cannot flip inside the tolerance there
    if decided.all():
        assert gp.original_fen == rp.original_fen and gp.fen == rp.fen
        assert [(f.square_name, f.original_piece, f.corrected_piece, f.rule_name) for f in gp.validation_fixes] == \
               [(f.square_name, f.original_piece, f.corrected_piece, f.rule_name) for f in rp.validation_fixes]
        stats["fen_checked"] += 1
    else:
        got_lab = np.argmax(gp.model_probabilities, axis=1)
        ref_lab = np.argmax(rp.model_probabilities, axis=1)
        assert np.array_equal(got_lab[decided], ref_lab[decided])
    assert gp.square_names == rp.square_names


def test_process_images_matches_the_oracle_pipeline(cv_model):
    unet, resnet = _oracle_models()
    images = _images(32)
    got = cv_model.process_images(images, fallback_quad=True, return_crops=True)
    ref = pipeline_ref.process_images(unet, resnet, images, fallback_quad=True)
    stats = {"mask_flips_inside_tolerance": 0, "max_prob_err": 0.0, "fen_checked": 0}
    found = 0
    for g, r, im in zip(got, ref, images):
        _compare(g, r, stats, resnet, im)
        found += int(r.board_extraction.quadrangle is not None and not np.array_equal(
            r.board_extraction.quadrangle, cv_model._scale_quadrangle(np.array([[[255, 0]], [[0, 0]], [[0, 255]], [[255, 255]]], np.int32), (512, 512))))
        if g.position is not None:
            crops = ChessVision.extract_squares(g.board_extraction.board_image)
            assert np.array_equal(g.position.squares, crops)
    assert found >= 20, found                              # the segmenting weights really find the boards
    assert stats["fen_checked"] >= 16, stats
    assert stats["mask_flips_inside_tolerance"] <= 2, stats


def test_two_shapes_through_six_jobs_match_the_oracle_image_by_image(cv_model):
    """Eleven photos of two shapes, interleaved, in jobs of at most 3 with both ends cut to 1: six jobs -- [0] [2,4] [6,8,9] [1,3,5] [7]
    [10] (tests/test_batched_pipeline_cpu.py) -- so results are scattered back over the caller's order from a split first job, full
    jobs of either shape and a split last job.  Result i must be image i's; the quality scores change nothing else."""
    unet, resnet = _oracle_models()
    images = [synthetic.board_photo(900 + s) for s in range(11)]
    for k in (1, 3, 5, 7, 10):
        images[k] = images[k][:384]                         # (384,512,3): the board is cut, most of these take the fallback quadrangle
    kw = dict(pipeline_chunk=3, first_job=1, last_job=1, fallback_quad=True)
    timings = {}
    got = cv_model.process_images(images, timings=timings, **kw)
    assert timings["jobs"] == 6 and len(got) == 11
    ref = pipeline_ref.process_images(unet, resnet, images, fallback_quad=True)
    stats = {"mask_flips_inside_tolerance": 0, "max_prob_err": 0.0, "fen_checked": 0}
    for g, r, im in zip(got, ref, images):
        _compare(g, r, stats, resnet, im)
    assert all(g.position is not None and g.quality is None for g in got)
    scored = cv_model.process_images(images, quality="sigmoid", **kw)
    for g, s in zip(got, scored):
        assert s.quality is not None
        ge, se = g.board_extraction, s.board_extraction
        for a, b in ((ge.probabilities, se.probabilities), (ge.binary_mask, se.binary_mask), (ge.quadrangle, se.quadrangle),
                     (ge.board_image, se.board_image), (g.position.model_probabilities, s.position.model_probabilities)):
            assert np.array_equal(a, b)
        assert (g.position.fen, g.position.original_fen, g.position.validation_fixes) == \
               (s.position.fen, s.position.original_fen, s.position.validation_fixes)


def test_flip_and_threshold_variants_match_the_oracle(cv_model):
    unet, resnet = _oracle_models()
    images = _images(6, seed0=50)
    stats = {"mask_flips_inside_tolerance": 0, "max_prob_err": 0.0, "fen_checked": 0}
    for thr, flip in ((0.3, True), (0.7, False)):
        got = cv_model.process_images(images, threshold=thr, flip=flip, fallback_quad=True)
        ref = pipeline_ref.process_images(unet, resnet, images, threshold=thr, flip=flip, fallback_quad=True)
        for g, r, im in zip(got, ref, images):
            # masks are thresholded on sigmoid(logit): the uncertainty band sits at logit(thr), not at 0
            _compare(g, r, stats, resnet, im, flip, logit_thr=float(np.log(thr / (1.0 - thr))))
            if g.position is not None:
                assert g.position.square_names == (constants.SQUARE_NAMES_FLIPPED if flip else constants.SQUARE_NAMES_NORMAL)
    assert stats["fen_checked"] >= 4, stats


def test_full_size_job_properties_and_sampled_oracle(cv_model):
    """BASELINE configs[3] size: 256 boards in one call (jobs of 64, software-pipelined).  Properties that need no oracle at
    this size + a sampled comparison against the oracle pipeline."""
    unet, resnet = _oracle_models()
    images = _images(256, seed0=200)
    res = cv_model.process_images(images, fallback_quad=True)
    assert len(res) == 256 and all(r.position is not None for r in res)
    again = cv_model.process_images(images[40:104], fallback_quad=True)          # other job boundaries, same boards
    for a, b in zip(res[40:104], again):
        assert a.position.fen == b.position.fen and np.array_equal(a.board_extraction.binary_mask, b.board_extraction.binary_mask)
        assert np.array_equal(a.position.model_probabilities, b.position.model_probabilities)
    for r in res:
        p = r.position
        assert np.allclose(p.model_probabilities.sum(axis=1), 1.0, atol=1e-5)
        for fen in (p.fen, p.original_fen):
            ranks = fen.split("/")
            assert len(ranks) == 8 and all(sum(int(c) if c.isdigit() else 1 for c in rk) == 8 for rk in ranks)
        assert not any(c in "pP" for c in p.fen.split("/")[0] + p.fen.split("/")[7])
        assert (len(p.validation_fixes) > 0) == (p.fen != p.original_fen)
        assert set(np.unique(r.board_extraction.binary_mask)) <= {0, 255}
    stats = {"mask_flips_inside_tolerance": 0, "max_prob_err": 0.0, "fen_checked": 0}
    pick = [3, 64, 65, 127, 128, 200, 255]
    ref = pipeline_ref.process_images(unet, resnet, [images[i] for i in pick], fallback_quad=True)
    for i, r in zip(pick, ref):
        _compare(res[i], r, stats, resnet, images[i])


def test_mixed_precision_pipeline_matches_the_oracle(tmp_path):
    """precision "f16x3+f16r": f32-grade UNet, classifier in its fp16 mode (one engine per model).  Board extraction is
    unchanged (same masks, quadrangles, boards); probabilities stay within configs[2]'s 1e-3 of the oracle pipeline and every FEN
    whose squares are decided beyond that tolerance is identical."""
    pe, pc = synthetic.save_checkpoints(tmp_path, segmenting=True)
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision="f16x3+f16r")
    assert cv._get_engine("unet").precision == "f16x3" and cv._get_engine("resnet18").precision == "f16r"
    assert cv._get_engine("unet") is not cv._get_engine("resnet18")
    unet, resnet = _oracle_models()
    images = _images(16, seed0=300)
    got = cv.process_images(images, fallback_quad=True)
    ref = pipeline_ref.process_images(unet, resnet, images, fallback_quad=True)
    stats = {"mask_flips_inside_tolerance": 0, "max_prob_err": 0.0, "fen_checked": 0}
    for g, r, im in zip(got, ref, images):
        _compare(g, r, stats, resnet, im)
    assert stats["fen_checked"] >= 8 and 0 < stats["max_prob_err"] <= 1e-3, stats
    single = cv.process_image(images[1])                    # the per-image API takes the same two engines
    assert single.position is not None and np.abs(single.position.model_probabilities - ref[1].position.model_probabilities).max() <= 1e-3


def test_process_image_is_the_native_pipeline_and_matches_batched_api_and_oracle(cv_model):
    """VERDICT r03 'next' 1: ``process_image`` / ``predict`` / ``extract_board`` / ``classify_position`` -- the API the reference's
    callers use (cv_endpoint.py:159, evaluate.py:270) -- run the same device stages as ``process_images``:
    process_image(img) == process_images([img])[0] field by field (bit for bit: same kernels, same batch size), and both match the
    oracle pipeline (boards byte-exact, probabilities within 1e-3, FEN identical).  No numpy warp / contour code runs on this path."""
    from unittest import mock

    from chessvision import classical

    unet, resnet = _oracle_models()
    images = _images(8, seed0=700)                          # index 0 and 7: no board -> position None without the fallback
    wide = np.zeros((384, 512, 3), np.uint8)
    wide[:, :384] = synthetic.board_photo(5, 384)
    images.append(wide)                                     # non-square photo: fractional resize, height-only quadrangle scale
    stats = {"mask_flips_inside_tolerance": 0, "max_prob_err": 0.0, "fen_checked": 0}
    with mock.patch.object(classical, "warp_perspective", side_effect=AssertionError("numpy warp on the native path")), \
         mock.patch.object(classical, "find_contours", side_effect=AssertionError("numpy contours on the native path")), \
         mock.patch.object(classical, "resize_area", side_effect=AssertionError("numpy resize on the native path")):
        singles = [cv_model.process_image(im) for im in images]
        assert cv_model.predict.__func__ is cv_model.process_image.__func__
    for im, single in zip(images, singles):
        batched = cv_model.process_images([im])[0]
        a, b = single.board_extraction, batched.board_extraction
        assert np.array_equal(a.probabilities, b.probabilities) and np.array_equal(a.binary_mask, b.binary_mask)
        assert (a.quadrangle is None) == (b.quadrangle is None) and (single.position is None) == (batched.position is None)
        if a.quadrangle is not None:
            assert np.array_equal(a.quadrangle, b.quadrangle) and a.quadrangle.dtype == np.float32
            assert np.array_equal(a.board_image, b.board_image)
            p, q = single.position, batched.position
            assert np.array_equal(p.model_probabilities, q.model_probabilities)
            assert p.fen == q.fen and p.original_fen == q.original_fen and p.square_names == q.square_names
            assert np.array_equal(p.squares, q.squares) and p.validation_fixes == q.validation_fixes
        ref = pipeline_ref.process_image(unet, resnet, im)   # the oracle's independent resize covers every shrink factor (4:3 photo too)
        _compare(single, ref, stats, resnet, im, fallback_quad=False)
    assert sum(s.position is not None for s in singles) >= 6 and stats["fen_checked"] >= 4, stats
    # the two halves on their own: extract_board, then classify_position on a board that did NOT come from this instance's last call
    ext = cv_model.extract_board(images[1])
    other = cv_model.extract_board(images[2])
    pos = cv_model.classify_position(ext.board_image.copy(), flip=True)          # a copy: takes the upload branch
    want = pipeline_ref.classify_board(resnet, ext.board_image, flip=True)
    assert np.abs(pos.model_probabilities - want.model_probabilities).max() <= 1e-3 and pos.square_names == want.square_names
    assert np.array_equal(other.board_image, singles[2].board_extraction.board_image)


def test_classifier_first_under_a_mixed_precision(tmp_path):
    """with "f16x3+f16r" the classifier engine may be requested before the extractor's (``cv.classifier`` or
    ``classify_position`` on an already rectified board); the engines are created independently."""
    pe, pc = synthetic.save_checkpoints(tmp_path, segmenting=True)
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision="f16x3+f16r")
    assert cv.classifier.engine.precision == "f16r" and list(cv._engines) == ["f16r"]
    board = np.random.default_rng(4).integers(0, 256, (512, 512), dtype=np.uint8)
    res = cv.classify_position(board)
    assert res.model_probabilities.shape == (64, 13) and cv._board_extractor is None
    assert cv.board_extractor.engine.precision == "f16x3"
    with pytest.raises(ValueError):
        ChessVision(precision="f16x3+bogus")


def test_per_image_and_batched_api_agree_to_the_summation_order_not_bit_for_bit(cv_model):
    """`process_image` runs UNet B=1 / ResNet-18 B=64 (split-K launches, graph replay), a `process_images` job runs 64 boards
    per pass through other tiles -- the same photo goes through different f32 summation orders.  Documented contract
    (include/chessvision_hip.h): masks equal except where a logit sits within 1e-4 of the threshold, the same
    quadrangle, probabilities within 1e-4, identical FEN and pawn-rule fixes; NOT bit-identical."""
    imgs = [synthetic.board_photo(200 + i) for i in range(70)]               # one full 64-board job and a short one
    batched = cv_model.process_images(imgs, fallback_quad=False)
    worst = 0.0
    for i in (0, 1, 31, 63, 64, 69):
        single = cv_model.process_image(imgs[i])
        b = batched[i]
        assert (single.position is None) == (b.position is None)
        differ = single.board_extraction.binary_mask != b.board_extraction.binary_mask
        assert np.all(np.abs(single.board_extraction.probabilities[differ]) < 1e-4)          # logits: threshold 0.5 <-> logit 0
        if single.position is None:
            continue
        assert np.array_equal(single.board_extraction.quadrangle, b.board_extraction.quadrangle)
        assert single.position.fen == b.position.fen and single.position.original_fen == b.position.original_fen
        assert [(f.square_name, f.corrected_piece) for f in single.position.validation_fixes] == \
               [(f.square_name, f.corrected_piece) for f in b.position.validation_fixes]
        worst = max(worst, float(np.abs(single.position.model_probabilities - b.position.model_probabilities).max()))
    assert worst <= 1e-4, worst

"""GPU: the antialiased bilinear resize of the reference's enrichment job on the device, through every layer.

1. ``HipEngine.resize_antialias_f32`` against the real implementation on the CPU (``F.interpolate(..., antialias=True)``; cases and the
   derived bar in tests/antialias_ref.py), and against its host form ``classical.resize_antialias`` bit for bit (the same operations in
   the same order, unfused).
2. Batch independence and full coverage of the destination.
3. ``HipEngine.unet_forward_mask``: ``unet_forward``'s logits and embedding bit for bit, the u8 entry's mask rule.
4. ``process_images(resize="antialias")`` at f16x3 against a reference composed here: torch antialias resize on the CPU -> the oracle
   UNet -> ``oracle.pipeline_ref.process_from_mask``, under the rules tests/test_gpu_e2e.py applies to the INTER_AREA path."""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

import antialias_ref as aref
from chessvision import ChessVision, classical, embeddings, synthetic
from oracle import classical_ref as cref
from oracle import pipeline_ref, synth
from oracle.resnet_ref import ResNet18
from oracle.unet_ref import UNet

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


def _same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the kernel against torch on the CPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", aref.CASES, ids=aref.case_id)
def test_kernel_matches_torch_cpu_and_the_host_form(engines, case):
    h, w, n, c = case
    eng = engines["f32"]
    batch = aref.images(case)
    want = aref.torch_resize(batch)
    got = eng.resize_antialias_f32(torch.from_numpy(batch), (aref.OUT, aref.OUT))
    assert got.shape == (n, c, aref.OUT, aref.OUT) and got.dtype == torch.float32 and got.is_contiguous()
    got = got.cpu().numpy()
    err, bar = float(np.abs(got.astype(np.float64) - want).max()), aref.bar(h, w)
    print(f"AA device {aref.case_id(case)}: err {err:.3e} bar {bar:.3e} err/bar {err / bar:.3f}")
    if (h, w) == (aref.OUT, aref.OUT):                     # every byte value goes through the kernel's form of float(u8) / 255
        assert np.unique(batch).size == 256 and _same_bits(got, want) and _same_bits(got, (batch.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))
    assert np.isfinite(got).all() and err <= bar, (case, err, bar)
    assert _same_bits(got[n - 1], classical.resize_antialias(batch[n - 1], (aref.OUT, aref.OUT)))      # device == host form
    flat = np.stack([np.full((h, w, c), 255, np.uint8), np.zeros((h, w, c), np.uint8)])
    white, black = eng.resize_antialias_f32(torch.from_numpy(flat), (aref.OUT, aref.OUT)).cpu().numpy()
    assert white.max() <= 1 + bar and white.min() >= 1 - bar
    assert not black.any()


def test_other_output_sizes_and_channel_counts(engines):
    """Output tiles that are cut on both axes (64 x 16 does not divide 100 x 50 or 70 x 33), two and four channels."""
    eng = engines["f32"]
    rng = np.random.default_rng(11)
    for (h, w, c), (oh, ow) in (((120, 333, 2), (50, 100)), ((97, 64, 4), (33, 70)), ((1, 1, 3), (5, 3)), ((40, 30, 1), (1, 1))):
        batch = rng.integers(0, 256, (2, h, w, c), dtype=np.uint8)
        got = eng.resize_antialias_f32(torch.from_numpy(batch), (oh, ow)).cpu().numpy()
        for k in range(2):
            assert _same_bits(got[k], classical.resize_antialias(batch[k], (ow, oh))), (h, w, c, oh, ow)
    # the engine keeps the tables of ONE geometry: another input shape, another output size, then the first geometry again (new pixels)
    for (h, w), out in (((37, 53), 16), ((53, 37), 16), ((37, 53), 24), ((37, 53), 16)):
        batch = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        got = eng.resize_antialias_f32(torch.from_numpy(batch), (out, out)).cpu().numpy()
        err, bar = float(np.abs(got.astype(np.float64) - aref.torch_resize(batch, out)).max()), aref.bar(h, w, out)
        print(f"AA device {h}x{w} -> {out}: err {err:.3e} bar {bar:.3e}")
        assert np.isfinite(got).all() and err <= bar, (h, w, out, err, bar)
        for k in range(2):
            assert _same_bits(got[k], classical.resize_antialias(batch[k], (out, out))), (h, w, out)
    with pytest.raises(Exception, match="resize_antialias_f32"):
        eng.resize_antialias_f32(torch.zeros((1, 8, 8, 5), dtype=torch.uint8))
    with pytest.raises(Exception, match="resize_antialias_f32"):
        eng.resize_antialias_f32(torch.zeros((1, 8, 8, 3), dtype=torch.float32))


# ---- 2. batch independence, every destination element written ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [aref.CASES[2], aref.CASES[3], aref.CASES[6]], ids=aref.case_id)
def test_an_image_gives_the_same_bits_alone_and_in_a_batch_and_the_destination_is_fully_written(engines, case):
    h, w, n, c = case
    eng = engines["f32"]
    lib, stream = eng._lib, torch.cuda.current_stream().cuda_stream
    batch = torch.from_numpy(aref.images(case, seed=1)).cuda()
    dst = torch.full((n, c, aref.OUT, aref.OUT), float("nan"), device="cuda")
    assert lib.cv_resize_antialias_f32(eng._h, batch.data_ptr(), n, h, w, c, dst.data_ptr(), aref.OUT, aref.OUT, stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dst).all())
    alone = torch.full((1, c, aref.OUT, aref.OUT), float("nan"), device="cuda")
    one = batch[2:3].clone()
    assert lib.cv_resize_antialias_f32(eng._h, one.data_ptr(), 1, h, w, c, alone.data_ptr(), aref.OUT, aref.OUT, stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(alone).all()) and _same_bits(alone[0], dst[2])
    assert lib.cv_resize_antialias_f32(eng._h, one.data_ptr(), 1, h, w, 5, alone.data_ptr(), aref.OUT, aref.OUT, stream) != 0
    assert b"cv_resize_antialias_f32" in lib.cv_last_error()


# ---- 3. the float entry that returns the mask ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unet_engine():
    from chessvision.hip_backend import HipEngine

    eng = HipEngine(precision="f16x3", unet_chunk=2)
    eng.load_unet(synth.make_unet(seed=1).state_dict())
    yield eng
    try:
        eng.check_numerics()
    finally:
        eng.close()


def _logit(thr):
    return float(np.log(thr / (1.0 - thr)))


@pytest.mark.parametrize("n, thr", [(1, 0.5), (2, 0.3), (3, 0.5)])     # one board (replays as a graph), a full chunk, a chunk and a rest
def test_unet_forward_mask_is_the_plain_forward_plus_the_u8_entrys_mask(unet_engine, n, thr):
    eng = unet_engine
    lib, stream = eng._lib, torch.cuda.current_stream().cuda_stream
    u8 = torch.from_numpy(aref.images((256, 256, n, 3), seed=2))
    x = eng.resize_antialias_f32(u8)                       # 256 -> 256: u8 / 255 exactly
    plain, plain_emb = eng.unet_forward(x, want_embedding=True)
    assert _same_bits(plain, eng.unet_forward(x))
    logits = torch.empty_like(plain)
    mask = torch.empty((n, 256, 256), dtype=torch.uint8, device="cuda")
    emb = torch.empty_like(plain_emb)
    for rep in range(3):                                   # eager, capture, replay for one board
        for want_mask, want_emb in ((True, True), (True, False), (False, False)):
            logits.fill_(float("nan")), emb.fill_(float("nan")), mask.fill_(7)
            assert lib.cv_unet_forward_mask(eng._h, x.data_ptr(), n, logits.data_ptr(), mask.data_ptr() if want_mask else None,
                                            ctypes.c_float(thr), emb.data_ptr() if want_emb else None, stream) == 0
            torch.cuda.synchronize()
            assert _same_bits(logits, plain), (rep, want_mask, want_emb)
            assert _same_bits(emb, plain_emb) if want_emb else bool(torch.isnan(emb).all())
            if not want_mask:
                assert bool((mask == 7).all())
                continue
            lg, mk = logits[:, 0].cpu().numpy(), mask.cpu().numpy()
            assert set(np.unique(mk)) <= {0, 255}
            sure = np.abs(lg - _logit(thr)) >= 1e-4        # the band tests/test_gpu_e2e.py leaves to either side
            assert np.array_equal(mk[sure], cref.binary_mask(lg, thr)[sure])
        logits.fill_(float("nan"))                         # the plain forward on the same pointers: its own graph, no mask, no embedding
        mask.fill_(7), emb.fill_(float("nan"))
        assert lib.cv_unet_forward(eng._h, x.data_ptr(), n, logits.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert _same_bits(logits, plain) and bool((mask == 7).all()) and bool(torch.isnan(emb).all())
    # the Python method: the tuple shapes of unet_forward_u8; the u8 entry on the same bytes applies the same rule to the same logits
    lg, mk = eng.unet_forward_mask(x, threshold=thr)
    lg2, mk2, em2 = eng.unet_forward_mask(x, threshold=thr, want_embedding=True)
    lg3, mk3 = eng.unet_forward_mask(x, threshold=thr, want_mask=False)
    assert mk3 is None and all(_same_bits(t, plain) for t in (lg, lg2, lg3)) and _same_bits(em2, plain_emb) and _same_bits(mk, mk2)
    lg8, mk8 = eng.unet_forward_u8(u8, threshold=thr)
    assert float((lg8 - lg).abs().max()) <= 1e-4
    if _same_bits(lg8, lg):
        assert _same_bits(mk8, mk)
    with pytest.raises(Exception):
        eng.unet_forward_mask(x, threshold=1.5)
    eng.check_numerics()


# ---- 4. process_images(resize="antialias") against the composed oracle ----------------------------------------------------------------------
def _images():
    """8 synthetic boards at 512 x 512, 3 at 300 x 400 (the board in the left 300 columns), one committed real photo.  Checked on
    the CPU for these seeds: the oracle alone has no logit within 1e-4 of the threshold (the closest, on the photo, is 1.2e-4 away),
    so a board that takes the continued-from-own-mask route does so because of the product, not of the reference."""
    imgs = [synthetic.board_photo(1200 + s) for s in range(8)]
    for s in range(3):
        wide = np.random.default_rng(1300 + s).integers(0, 40, (300, 400, 3), dtype=np.uint8)
        wide[:, :300] = synthetic.board_photo(1310 + s, 300)
        imgs.append(wide)
    imgs.append(np.ascontiguousarray(np.load(GOLDEN / "photos8_0.npz")["bgr"][0]))
    order = [0, 8, 1, 2, 9, 3, 11, 4, 5, 10, 6, 7]        # shapes interleaved: results are scattered back over the caller's order
    return [imgs[i] for i in order]


KW = dict(fallback_quad=True, pipeline_chunk=3, first_job=1, last_job=1)


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    d = tmp_path_factory.mktemp("weights_antialias")
    pe, pc = synthetic.save_checkpoints(d, segmenting=True)
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision="f16x3")
    unet, resnet = UNet(3, 1, False), ResNet18()
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.unet_state_dict(1, segmenting=True).items()}, strict=False)
    resnet.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.resnet18_state_dict(2).items()}, strict=False)
    unet, resnet = unet.eval(), resnet.eval()
    images = _images()
    hooked = []
    handle = list(unet.named_modules())[embeddings.UNET_HOOK_INDEX][1].register_forward_hook(lambda m, i, o: hooked.append(o.detach().numpy()))
    try:
        with torch.no_grad():                              # the reference, once: torch antialias resize on the CPU -> the oracle UNet
            logits = [unet(torch.from_numpy(aref.torch_resize(im[None])))[0, 0].numpy().astype(np.float32) for im in images]
    finally:
        handle.remove()
    ref_emb = [embeddings.channel_mean(t)[0] for t in hooked]
    return cv, resnet, images, logits, ref_emb


def _compare(got, ref_logits, stats, resnet, image):
    """tests/test_gpu_e2e.py: _compare, restated for a reference that starts from given logits (threshold 0.5, fallback quadrangle)."""
    ge = got.board_extraction
    lerr = float(np.abs(ge.probabilities - ref_logits).max())
    stats["max_logit_err"] = max(stats["max_logit_err"], lerr)
    assert lerr <= 1e-3, lerr
    ref_mask = cref.binary_mask(ref_logits, 0.5)
    unsure = np.abs(ref_logits) < 1e-4
    assert np.array_equal(ge.binary_mask[~unsure], ref_mask[~unsure])
    if unsure.any() and not np.array_equal(ge.binary_mask, ref_mask):
        stats["mask_flips_inside_tolerance"] += 1          # the oracle continues from the product's mask for this board
        ref_mask = ge.binary_mask
    ref = pipeline_ref.process_from_mask(resnet, image, ref_mask, ref_logits, False, True)
    re_ = ref.board_extraction
    assert ge.quadrangle is not None and re_.quadrangle is not None and got.position is not None and ref.position is not None
    assert np.array_equal(ge.quadrangle, re_.quadrangle)
    assert np.array_equal(ge.board_image, re_.board_image)
    gp, rp = got.position, ref.position
    perr = float(np.abs(gp.model_probabilities - rp.model_probabilities).max())
    stats["max_prob_err"] = max(stats["max_prob_err"], perr)
    assert perr <= 1e-3, perr
    top2 = np.sort(rp.model_probabilities, axis=1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 2e-3             # argmax cannot flip inside the tolerance there
    if decided.all():
        assert gp.original_fen == rp.original_fen and gp.fen == rp.fen
        assert [(f.square_name, f.original_piece, f.corrected_piece, f.rule_name) for f in gp.validation_fixes] == \
               [(f.square_name, f.original_piece, f.corrected_piece, f.rule_name) for f in rp.validation_fixes]
        stats["fen_checked"] += 1
    else:
        assert np.array_equal(np.argmax(gp.model_probabilities, axis=1)[decided], np.argmax(rp.model_probabilities, axis=1)[decided])
    assert gp.square_names == rp.square_names
    return re_


def test_process_images_antialias_matches_the_composed_oracle(e2e):
    cv, resnet, images, ref_logits, _ = e2e
    timings = {}
    got = cv.process_images(images, resize="antialias", timings=timings, **KW)
    assert len(got) == 12 and timings["jobs"] == 6 and timings["resize_ms"] > 0 and timings["unet_ms"] > 0
    stats = {"mask_flips_inside_tolerance": 0, "max_prob_err": 0.0, "max_logit_err": 0.0, "fen_checked": 0}
    whole = cv._scale_quadrangle(np.array([[[255, 0]], [[0, 0]], [[0, 255]], [[255, 255]]], np.int32), (512, 512))
    found = 0
    for g, lg, im in zip(got, ref_logits, images):
        re_ = _compare(g, lg, stats, resnet, im)
        found += int(im.shape[0] == 512 and not np.array_equal(re_.quadrangle, whole))
    print(f"AA e2e: {stats}, boards found in the mask {found}")
    assert stats["mask_flips_inside_tolerance"] <= 2 and stats["fen_checked"] >= 6 and found >= 6, (stats, found)
    area = cv.process_images(images, **KW)                 # the other arithmetic really is another one
    assert any(not np.array_equal(a.board_extraction.probabilities, g.board_extraction.probabilities) for a, g in zip(area, got))


def _fields(res):
    e, p = res.board_extraction, res.position
    arrays = [e.probabilities, e.binary_mask, e.quadrangle, e.board_image] + ([p.model_probabilities, p.squares] if p else [])
    return ([None if a is None else (a.dtype.str, a.shape, a.tobytes()) for a in arrays],
            None if p is None else (p.fen, p.original_fen, p.square_names, p.validation_fixes), res.quality)


def test_area_is_the_call_without_the_argument_bit_for_bit(e2e):
    cv, _, images, _, _ = e2e
    plain = cv.process_images(images, **KW)
    area = cv.process_images(images, resize="area", **KW)
    assert [_fields(r) for r in area] == [_fields(r) for r in plain]


def test_antialias_with_scores_and_embeddings_and_through_evaluate_images(e2e):
    cv, _, images, ref_logits, ref_emb = e2e
    base = cv.process_images(images, resize="antialias", **KW)
    got = cv.process_images(images, resize="antialias", quality="sigmoid", embeddings=True, **KW)
    for i, (b, g) in enumerate(zip(base, got)):
        assert _fields(b)[:2] == _fields(g)[:2]            # the extras change no other field
        q = g.quality
        assert q is not None and all(np.isfinite(v) for v in (q.confidence, q.quad_score, q.completeness, q.distribution))
        emb, ref = g.embeddings.board_extractor, ref_emb[i]
        err, bar = float(np.abs(emb - ref).max()), 1e-3 * max(1.0, float(np.abs(ref).max()))        # the embeddings' parity bar
        print(f"AA embedding image {i}: err {err:.3e} bar {bar:.3e}")
        assert emb.shape == ref.shape and err <= bar, (i, err, bar)
        assert g.embeddings.classifier is not None and g.embeddings.classifier.shape == (64, 512)
    same_jobs = dict(fallback_quad=True, pipeline_chunk=64, first_job=16, last_job=0)         # how evaluate_images cuts a call
    want = cv.process_images(images, resize="antialias", **same_jobs)
    fens = [r.position.fen for r in want]
    assert cv.evaluation_resize == "area"
    cv.evaluation_resize = "antialias"
    try:
        report = cv.evaluate_images(images, true_fens=fens, fallback_quad=True)
    finally:
        del cv.evaluation_resize
    assert [_fields(r)[:2] for r in report.results] == [_fields(r)[:2] for r in want]
    area = cv.evaluate_images(images, true_fens=fens, fallback_quad=True)
    assert [_fields(r)[:2] for r in area.results] == [_fields(r)[:2] for r in cv.process_images(images, **same_jobs)]

"""GPU: the pipeline fed with JPEG streams (``ChessVision.process_encoded`` / ``process_jpeg`` / ``cv_process_jpeg``) against the same
pipeline fed with the decoded arrays (``process_images`` / ``process_image``).  The decoder reproduces the committed Pillow pixels byte
for byte (tests/test_gpu_jpeg.py), the batch shapes are equal, so every field must be equal bit for bit."""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from chessvision import ChessVision, jpeg, synthetic

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def cv(tmp_path_factory):
    pe, pc = synthetic.save_checkpoints(tmp_path_factory.mktemp("ckpt"), segmenting=True)
    inst = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))
    yield inst
    inst.close()


@pytest.fixture(scope="module")
def photos():
    blobs = []
    for tag in "ab":
        z = np.load(GOLDEN / f"photos8_jpeg_{tag}.npz")
        blobs += [z[f"blob_{k}"].tobytes() for k in range(len(z["names"]))]
    arrays = [np.ascontiguousarray(np.load(GOLDEN / f"photos8_{i}.npz")["bgr"][0]) for i in range(8)]
    return blobs, arrays


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


def assert_equal_results(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        ge, we = g.board_extraction, w.board_extraction
        assert np.array_equal(ge.probabilities, we.probabilities), i          # logits, bit for bit
        assert np.array_equal(ge.binary_mask, we.binary_mask), i
        assert _same(ge.quadrangle, we.quadrangle) and _same(ge.board_image, we.board_image), i
        assert (g.position is None) == (w.position is None), i
        if g.position is not None:
            assert np.array_equal(g.position.model_probabilities, w.position.model_probabilities), i
            assert (g.position.fen, g.position.original_fen) == (w.position.fen, w.position.original_fen), i
            assert _same(g.position.squares, w.position.squares) and g.position.square_names == w.position.square_names, i
            assert g.position.validation_fixes == w.position.validation_fixes, i
        assert g.quality == w.quality, i
        ga, wa = getattr(g, "embeddings", None), getattr(w, "embeddings", None)
        assert (ga is None) == (wa is None), i
        if ga is not None:
            assert _same(ga.board_extractor, wa.board_extractor) and _same(ga.classifier, wa.classifier), i


@pytest.mark.parametrize("kw", [{}, {"pipeline_chunk": 3}, {"quality": "sigmoid", "embeddings": True}], ids=["default", "chunk3", "quality+embeddings"])
def test_process_encoded_equals_process_images_on_the_decoded_photos(cv, photos, kw):
    blobs, arrays = photos
    timings: dict = {}
    got = cv.process_encoded(blobs, fallback_quad=True, timings=timings, **kw)
    want = cv.process_images(arrays, fallback_quad=True, **kw)
    assert sum(r.position is not None for r in want) == 8
    assert_equal_results(got, want)
    assert timings["entropy_s"] > 0 and timings["jpeg_ms"] > 0
    assert timings["jobs"] == (3 if kw.get("pipeline_chunk") == 3 else 1)


def test_a_call_of_mixed_geometries_plans_two_jobs_and_keeps_input_order(cv):
    z = np.load(GOLDEN / "jpeg_cases.npz")
    names = ["mixed_64x48_0", "gray_33x33_0", "gray_33x33_1", "mixed_64x48_1", "gray_33x33_2"]
    blobs = [z[f"blob/{n}"].tobytes() for n in names]
    arrays = []
    for n in names:
        p = z[f"pixels/{n}"]
        arrays.append(np.ascontiguousarray(p[:, :, ::-1] if p.ndim == 3 else np.repeat(p[:, :, None], 3, axis=2)))
    assert [a.shape for a in arrays] == [(48, 64, 3), (33, 33, 3), (33, 33, 3), (48, 64, 3), (33, 33, 3)]
    timings: dict = {}
    got = cv.process_encoded(blobs, fallback_quad=True, first_job=0, timings=timings)
    assert timings["jobs"] == 2
    assert_equal_results(got, cv.process_images(arrays, fallback_quad=True, first_job=0))
    for order, pixels in zip(("bgr", "rgb"), (arrays, [a[:, :, ::-1] for a in arrays])):
        decoded = cv.decode_jpegs(blobs, order)
        assert all(np.array_equal(d, p) for d, p in zip(decoded, pixels))


def test_process_jpeg_equals_process_image(cv, photos):
    blobs, arrays = photos
    for k in (0, 5):
        assert_equal_results([cv.process_jpeg(blobs[k])], [cv.process_image(arrays[k])])
        assert_equal_results([cv.process_jpeg(blobs[k], threshold=0.3, flip=True)], [cv.process_image(arrays[k], threshold=0.3, flip=True)])
    # the pixel front after the JPEG front on the same slot: its staging pieces are where they were
    assert_equal_results([cv.process_image(arrays[0])], [cv.process_jpeg(blobs[0])])


def test_unsupported_streams_raise_before_any_launch(cv, photos):
    z = np.load(GOLDEN / "jpeg_cases.npz")
    progressive = z["blob/progressive"].tobytes()
    blobs = [photos[0][0], progressive, photos[0][1], z["blob/truncated_in_quant_table"].tobytes()]
    torch.cuda.synchronize()
    launches = []
    eng = cv._get_engine("unet")
    real = eng.jpeg_reconstruct_dev
    eng.jpeg_reconstruct_dev = lambda *a, **k: launches.append(1) or real(*a, **k)
    try:
        with pytest.raises(jpeg.UnsupportedJpeg) as err:
            cv.process_encoded(blobs)
        assert isinstance(err.value, ValueError) and sorted(err.value.reasons) == [1, 3]
        assert "progressive" in err.value.reasons[1] and "truncated" in err.value.reasons[3]
        with pytest.raises(jpeg.UnsupportedJpeg):
            cv.process_jpeg(progressive)
        with pytest.raises(jpeg.UnsupportedJpeg):
            cv.decode_jpegs(blobs)
    finally:
        del eng.jpeg_reconstruct_dev
    assert not launches


def test_cv_process_jpeg_with_an_abi3_sized_struct_leaves_squares_untouched(cv, photos):
    from chessvision.hip_backend import _ImageResult, _check, _stream_ptr, load_library

    lib, blob = load_library(), photos[0][0]
    eng_u, eng_c = cv._get_engine("unet"), cv._get_engine("resnet18")
    _ = cv.board_extractor, cv.classifier
    squares = np.full((64, 64, 64), 0xA5, np.uint8)
    board = np.zeros((512, 512), np.uint8)
    res = _ImageResult()
    res.board, res.squares = board.ctypes.data, squares.ctypes.data
    _check(lib.cv_process_jpeg(eng_u._h, eng_c._h, blob, len(blob), 0.5, 0, 1, ctypes.byref(res), _ImageResult.squares.offset,
                               _stream_ptr(eng_u.device)))
    assert res.found == 1 and board.any() and (squares == 0xA5).all()
    _check(lib.cv_process_jpeg(eng_u._h, eng_c._h, blob, len(blob), 0.5, 0, 1, ctypes.byref(res), ctypes.sizeof(res), _stream_ptr(eng_u.device)))
    assert np.array_equal(squares.reshape(8, 8, 64, 64).transpose(0, 2, 1, 3).reshape(512, 512), board)
    assert lib.cv_process_jpeg(eng_u._h, eng_c._h, blob, len(blob), 0.5, 0, 1, ctypes.byref(res), 8, _stream_ptr(eng_u.device)) != 0

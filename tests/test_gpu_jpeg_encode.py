"""GPU: the gray JPEG encoder (csrc/jpeg_enc.hip) against the committed files Pillow wrote and the numpy form ``jpeg.encode_gray`` --
equality of bytes, no case left out -- at n = 1 and across the internal chunk size, twice for determinism; and ``board_jpeg`` through
``process_images`` / ``process_encoded``: the file is libjpeg's for the board that came back, every other field is what the same call
returns without the keyword."""
from __future__ import annotations

import hashlib
from pathlib import Path

import numpy as np
import pytest
import torch

import jpeg_encode_cases as cases
from chessvision import ChessVision, jpeg, synthetic
from chessvision.hip_backend import HipEngine
from test_gpu_process_encoded import assert_equal_results

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
CHUNK_IMAGES = 1024                      # csrc/jpeg_enc_device.h: kJpegEncChunkImages


@pytest.fixture(scope="module")
def eng():
    e = HipEngine("cuda:0", precision="f32")
    yield e
    e.close()


@pytest.fixture(scope="module")
def cv(tmp_path_factory):
    pe, pc = synthetic.save_checkpoints(tmp_path_factory.mktemp("ckpt"), segmenting=True)
    inst = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))
    yield inst
    inst.close()


def test_every_golden_group_byte_for_byte(eng):
    z, n = cases.load(), 0
    for name, q, images, files in cases.groups(z):
        got = eng.jpeg_encode_gray(images, q)                   # the three (twelve) images of a group in ONE launch
        assert len(got) == len(files)
        for k, (g, want) in enumerate(zip(got, files)):
            assert g == want, (name, k, len(g), len(want))
            assert g == jpeg.encode_gray(images[k], q), (name, k)
            n += 1
    assert n == 8 * 4 * 3 + 12


def test_the_real_board_and_a_device_tensor_input(eng):
    z = cases.load()
    board = cases.board_image()
    got = eng.jpeg_encode_gray(torch.from_numpy(board[None]).to(eng.device), 95)
    assert len(got) == 1 and len(got[0]) == int(z["board_length"])
    assert hashlib.sha256(got[0]).digest() == z["board_sha256"].tobytes()


def test_one_image_and_a_batch_across_the_chunk_size(eng):
    rng = np.random.default_rng(3)
    base = [rng.integers(0, 256, (8, 8)).astype(np.uint8) for _ in range(5)] + [np.full((8, 8), 255, np.uint8), np.zeros((8, 8), np.uint8)]
    want = [jpeg.encode_gray(a, 100) for a in base]
    assert eng.jpeg_encode_gray(base[0][None], 100) == want[:1]
    n = CHUNK_IMAGES + 7                                        # two passes over the scratch, the second one short
    got = eng.jpeg_encode_gray(np.stack([base[i % 7] for i in range(n)]), 100)
    assert len(got) == n
    assert all(got[i] == want[i % 7] for i in range(n))


def test_two_runs_give_identical_bytes_and_the_device_form_is_compact(eng):
    z = cases.load()
    images = torch.from_numpy(np.stack([z["image/128x128/binary"], z["image/128x128/noise"], z["image/128x128/smooth"]])).to(eng.device)
    a, b = eng.jpeg_encode_gray(images, 100), eng.jpeg_encode_gray(images, 100)
    assert a == b and a[0] == z["file/128x128/q100/binary"].tobytes()
    out, offsets, lengths = eng.jpeg_encode_gray_dev(images, 100)
    off, ln = offsets.cpu().numpy(), lengths.cpu().numpy()
    assert off[0] == 0 and np.all(off % 16 == 0) and np.array_equal(off[1:], np.cumsum((ln + 15) // 16 * 16))
    assert [bytes(out[int(o):int(o) + int(k)].cpu().numpy()) for o, k in zip(off, ln)] == a
    with pytest.raises(Exception):
        eng.jpeg_encode_gray_dev(torch.zeros((1, 4097, 8), dtype=torch.uint8, device=eng.device))


def test_encode_gray_groups_mixed_sizes_and_takes_the_square_crops(cv):
    z = cases.load()
    board = cases.board_image()
    crops = ChessVision.extract_squares(board)                 # (64, 64, 64, 1): the training-folder format
    mixed = [z["image/7x9/noise"], crops[0], z["image/33x40/smooth"], crops[63], z["image/7x9/smooth"]]
    got = cv.encode_gray(mixed, quality=90)
    assert got == [jpeg.encode_gray(np.asarray(a).reshape(a.shape[:2]), 90) for a in mixed]


@pytest.fixture(scope="module")
def photos():
    return [np.ascontiguousarray(np.load(GOLDEN / f"photos8_{i}.npz")["bgr"][0]) for i in range(8)]


def _check_board_jpegs(got, want):
    assert_equal_results(got, want)                            # every other field: bit for bit the call without the keyword
    found = 0
    for g, w in zip(got, want):
        board = g.board_extraction.board_image
        assert w.board_jpeg is None
        if board is None:
            assert g.board_jpeg is None
        else:
            assert isinstance(g.board_jpeg, bytes) and g.board_jpeg == jpeg.encode_gray(board, 95)
            found += 1
    return found


def test_process_images_board_jpeg(cv, photos):
    timings: dict = {}
    got = cv.process_images(photos, board_jpeg=95, timings=timings, pipeline_chunk=3)
    want = cv.process_images(photos, pipeline_chunk=3)
    found = _check_board_jpegs(got, want)
    assert timings["encode_ms"] > 0 and "fetch_jpeg_s" in timings
    plain: dict = {}
    cv.process_images(photos[:2], timings=plain)
    assert "encode_ms" not in plain and "fetch_jpeg_s" not in plain
    # with the fallback quadrangle every photo has a board, hence a file
    got = cv.process_images(photos, board_jpeg=95, fallback_quad=True)
    assert _check_board_jpegs(got, cv.process_images(photos, fallback_quad=True)) == 8 >= found


def test_process_encoded_board_jpeg(cv):
    blobs = []
    for tag in "ab":
        z = np.load(GOLDEN / f"photos8_jpeg_{tag}.npz")
        blobs += [z[f"blob_{k}"].tobytes() for k in range(len(z["names"]))]
    got = cv.process_encoded(blobs, board_jpeg=95, fallback_quad=True)
    assert _check_board_jpegs(got, cv.process_encoded(blobs, fallback_quad=True)) == len(blobs)

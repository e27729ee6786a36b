"""GPU: the colour JPEG encoder (the colour front end of csrc/jpeg_enc.hip and the chain it shares with the gray one) against the
committed files Pillow wrote and the numpy form ``jpeg.encode_colour`` -- equality of bytes, no case left out, BGR and RGB -- at n = 1
and across the internal chunk size, twice for determinism; ``ChessVision.encode_colour`` on mixed sizes; ``transcode_jpegs`` against
Pillow's transcodes and against decode-then-encode; and the gray encoder right behind a colour encode that grew the shared scratch."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest
import torch

import jpeg_colour_encode_cases as cases
import jpeg_encode_cases as gray_cases
from chessvision import ChessVision, jpeg
from chessvision.hip_backend import HipEngine

pytestmark = pytest.mark.gpu
CHUNK_IMAGES = 1024                      # csrc/jpeg_enc_device.h: kJpegEncChunkImages


@pytest.fixture(scope="module")
def eng():
    e = HipEngine("cuda:0", precision="f32")
    yield e
    e.close()


@pytest.fixture(scope="module")
def cv():
    inst = ChessVision()
    yield inst
    inst.close()


def test_every_golden_group_byte_for_byte_in_both_orders(eng):
    z, n = cases.load(), 0
    for name, q, sub, order, images, files in cases.groups(z):
        other = "rgb" if order == "bgr" else "bgr"
        got = eng.jpeg_encode_colour(images, q, sub, order)       # the three images of a group in ONE launch
        swapped = eng.jpeg_encode_colour(np.ascontiguousarray(images[..., ::-1]), q, sub, other)
        assert len(got) == len(swapped) == len(files) == 3
        for k, (g, s, want) in enumerate(zip(got, swapped, files)):
            assert g == want, (name, k, len(g), len(want))
            assert s == want, (name, k, other)
            n += 1
    assert n == 3 * (10 * 3 * 4 + 3)


def test_the_real_photo_its_crop_and_a_device_tensor_input(eng):
    z = cases.load()
    got = eng.jpeg_encode_colour(torch.from_numpy(cases.photo()[None]).to(eng.device), cases.PHOTO_QUALITY, cases.PHOTO_SUBSAMPLING)
    assert len(got) == 1 and len(got[0]) == int(z["photo_length"])
    assert hashlib.sha256(got[0]).digest() == z["photo_sha256"].tobytes()
    crop = cases.photo_crop()
    assert eng.jpeg_encode_colour(crop[None], cases.PHOTO_QUALITY, cases.PHOTO_SUBSAMPLING) == [cases.extra_files(z)[0]]
    # a source that is not 8-byte aligned takes the byte loads, and gives the same file
    flat = torch.zeros(crop.size + 3, dtype=torch.uint8, device=eng.device)
    flat[3:] = torch.from_numpy(crop.reshape(-1)).to(eng.device)
    assert eng.jpeg_encode_colour(flat[3:].view(1, *crop.shape), cases.PHOTO_QUALITY, cases.PHOTO_SUBSAMPLING) == [cases.extra_files(z)[0]]


def test_one_image_and_a_batch_across_the_chunk_size(eng):
    rng = np.random.default_rng(3)
    base = [rng.integers(0, 256, (8, 8, 3)).astype(np.uint8) for _ in range(5)] + [np.full((8, 8, 3), 255, np.uint8), np.zeros((8, 8, 3), np.uint8)]
    want = [jpeg.encode_colour(a, 100, "4:4:4") for a in base]
    assert eng.jpeg_encode_colour(base[0][None], 100, "4:4:4") == want[:1]
    n = CHUNK_IMAGES + 7                                        # two passes over the scratch, the second one short
    got = eng.jpeg_encode_colour(np.stack([base[i % 7] for i in range(n)]), 100, "4:4:4")
    assert len(got) == n
    assert all(got[i] == want[i % 7] for i in range(n))


def test_passes_of_more_than_65536_coded_blocks_are_byte_exact_in_every_subsampling(eng):
    """A pass of more than 256 groups of 256 blocks, where blocks of different groups meet in one cache line of the bit buffer all
    along it: as a batch of small images (96 000, 70 400 and 76 800 coded blocks) and as ONE image of 1792 x 1792 (75 264, 100 352 and
    150 528).  When whole words of the buffer were still stored plainly, exactly these sizes lost bits in 4:2:0 and 4:2:2."""
    photo = cases.photo()
    base = [np.ascontiguousarray(photo[y:y + 64, x:x + 64]) for y, x in ((0, 0), (100, 200), (300, 50), (448, 448), (17, 301), (256, 256), (77, 400), (390, 9))]
    big = np.ascontiguousarray(np.tile(cases.photo(), (4, 4, 1))[:1792, :1792])
    for sub, n in (("4:2:0", 1000), ("4:2:2", 1100), ("4:4:4", 400)):
        want = [jpeg.encode_colour(a, 95, sub) for a in base]
        for _ in range(2):
            got = eng.jpeg_encode_colour(np.stack([base[i % 8] for i in range(n)]), 95, sub)
            assert [i for i in range(n) if got[i] != want[i % 8]] == [], sub
        assert eng.jpeg_encode_colour(big[None], 95, sub) == [jpeg.encode_colour(big, 95, sub)], sub


def test_the_gray_encoder_above_65536_blocks_is_byte_exact(eng):
    """The gray chain shares the bit buffer's rules: 20 boards of 512 x 512 are 81 920 blocks in one pass."""
    boards = [np.ascontiguousarray(np.load(cases.GOLDEN / f"photos8_{i}.npz")["bgr"][0][..., 1]) for i in range(4)]
    want = [jpeg.encode_gray(b, 95) for b in boards]
    got = eng.jpeg_encode_gray(np.stack([boards[i % 4] for i in range(20)]), 95)
    assert [i for i in range(20) if got[i] != want[i % 4]] == []


def test_two_runs_give_identical_bytes_and_the_device_form_is_compact(eng):
    z = cases.load()
    images = torch.from_numpy(np.stack([z[f"image/64x64/{k}"] for k in ("binary", "noise", "smooth")])).to(eng.device)
    for sub in cases.SUBSAMPLINGS:
        a, b = eng.jpeg_encode_colour(images, 100, sub), eng.jpeg_encode_colour(images, 100, sub)
        assert a == b and a == [jpeg.encode_colour(x, 100, sub) for x in images.cpu().numpy()]
        out, offsets, lengths = eng.jpeg_encode_colour_dev(images, 100, sub)
        off, ln = offsets.cpu().numpy(), lengths.cpu().numpy()
        assert off[0] == 0 and np.all(off % 16 == 0) and np.array_equal(off[1:], np.cumsum((ln + 15) // 16 * 16))
        assert off[-1] == (off[-2] + ln[-1] + 15) // 16 * 16                # the last entry is the end
        assert [bytes(out[int(o):int(o) + int(k)].cpu().numpy()) for o, k in zip(off, ln)] == a
    for bad in (torch.zeros((1, 4097, 8, 3), dtype=torch.uint8, device=eng.device), torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=eng.device)):
        with pytest.raises(Exception):
            eng.jpeg_encode_colour_dev(bad)


def test_encode_colour_groups_mixed_sizes_and_keeps_input_order(cv):
    z = cases.load()
    mixed = [z["image/2x9/noise"], z["image/33x31/smooth"], cases.photo_crop(), z["image/2x9/primaries"], z["image/1x1/noise"],
             z["image/33x31/binary"]]
    for sub, order in (("4:2:0", "bgr"), ("4:2:2", "rgb")):
        got = cv.encode_colour(mixed, quality=90, subsampling=sub, channel_order=order)
        assert got == [jpeg.encode_colour(a, 90, sub, order) for a in mixed]


def test_transcode_equals_pillow_and_decode_then_encode(cv):
    z = cases.load()
    blobs, want = cases.transcode_blobs(), cases.extra_files(z)[1]
    infos = [jpeg.jpeg_info(b) for b in blobs]
    assert sorted({f.orientation for f in infos}) == [0, 1, 6, 8] and sum(f.components == 1 for f in infos) == 1
    for k, (_, name, q, sub) in enumerate(cases.TRANSCODES):       # each case has its own quality and subsampling: one call each
        assert cv.transcode_jpegs([blobs[k]], q, sub, orientation="exif") == [want[k]], name
    # one call over all six: groups by (geometry, effective tag), files in input order, equal to decode-then-encode
    for orientation in ("exif", "ignore"):
        got = cv.transcode_jpegs(blobs, 90, "4:2:2", orientation=orientation)
        photos = cv.decode_jpegs(blobs, "bgr", orientation)
        assert got == cv.encode_colour(photos, 90, "4:2:2") == [jpeg.encode_colour(p, 90, "4:2:2") for p in photos], orientation
    upright = cv.decode_jpegs(blobs, "bgr", "exif")
    assert [jpeg.jpeg_info(f).geometry[:3] for f in cv.transcode_jpegs(blobs, orientation="exif")] == [(p.shape[1], p.shape[0], 3) for p in upright]


def test_the_gray_encoder_right_behind_a_colour_encode_that_grew_the_scratch():
    """A fresh engine: a 64 x 64 4:4:4 colour encode sizes the scratch, the gray encodes that follow carve the same block anew (other
    offsets, the 328-byte header, one table set) and must give the gray files; then colour again."""
    z, g = cases.load(), gray_cases.load()
    e = HipEngine("cuda:0", precision="f32")
    try:
        colour = np.stack([z[f"image/64x64/{k}"] for k in ("noise", "smooth", "binary")])
        want = [jpeg.encode_colour(a, 95, "4:4:4") for a in colour]
        assert e.jpeg_encode_colour(colour, 95, "4:4:4") == want
        for h, w in ((33, 40), (7, 9), (64, 64)):
            kinds = gray_cases.group_kinds(gray_cases.GEOMETRIES.index((h, w)), gray_cases.QUALITIES.index(95))
            images = np.stack([g[f"image/{h}x{w}/{k}"] for k in kinds])
            got = e.jpeg_encode_gray(images, 95)
            assert got == [g[f"file/{h}x{w}/q95/{k}"].tobytes() for k in kinds] == [jpeg.encode_gray(a, 95) for a in images], (h, w)
        assert e.jpeg_encode_colour(colour, 95, "4:4:4") == want
    finally:
        e.close()

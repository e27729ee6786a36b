"""GPU: EXIF orientation applied in the colour stage's store (``jpeg_colour_oriented_kernel`` in csrc/jpeg.hip, through
``HipEngine.jpeg_decode(orientation="exif")``, ``jpeg_reconstruct_dev(orientation=tag)``, ``ChessVision.decode_jpegs``,
``process_encoded`` and ``process_jpeg``).  The expected pixels are tests/golden/jpeg_orientation_cases.npz: Pillow's decode turned by
``PIL.ImageOps.exif_transpose``; every comparison is equality of bytes.  The sizes straddle the kernel's 32 x 32 tile (one pixel, one
tile and a pixel, two tiles and three pixels, a short tile), and every destination is also tried off 4-byte alignment, since the
kernel chooses between dword and byte stores by the address of each output row."""
from __future__ import annotations

import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_orientation_cases as cases
from chessvision import ChessVision, jpeg, synthetic
from test_gpu_process_encoded import assert_equal_results

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def engine():
    from chessvision.hip_backend import HipEngine

    eng = HipEngine(precision="f32")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def cv(tmp_path_factory):
    pe, pc = synthetic.save_checkpoints(tmp_path_factory.mktemp("ckpt"), segmenting=True)
    inst = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))
    yield inst
    inst.close()


def _want(case, order):
    """The fixture's upright picture in a channel order: RGB as stored, BGR reversed, a 1-component stream replicated in colour."""
    if case.gray:
        return case.upright if order == "gray" else np.repeat(case.upright[:, :, None], 3, axis=2)
    return case.upright if order == "rgb" else case.upright[:, :, ::-1]


def test_jpeg_decode_exif_equals_pillows_transpose_on_every_case_in_every_channel_order(engine):
    seen = 0
    for c in cases.load():
        for order in (("bgr", "rgb", "gray") if c.gray else ("bgr", "rgb")):
            got = engine.jpeg_decode([c.blob], order, orientation="exif")
            want = _want(c, order)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (1,) + want.shape, (c.name, order)
            assert np.array_equal(got.cpu().numpy()[0], want), (c.name, order)
            seen += 1
    assert seen == 3 * (9 * 9 + 2) * 2 + (9 * 9 + 2) * 3


def test_three_images_per_launch_into_misaligned_guarded_buffers(engine):
    """n = 3 of the same stream (the image stride of planes and of dst), written into the middle of a buffer 64 bytes too large at
    each end and filled with a sentinel, at every byte alignment in turn: not one byte outside the pictures may change."""
    for k, c in enumerate(cases.load()):
        coeffs, qtables, info = jpeg.entropy_decode(c.blob)
        co = torch.from_numpy(np.stack([coeffs] * 3)).to(engine.device)
        qt = torch.from_numpy(np.stack([qtables] * 3).view(np.int16)).to(engine.device)
        for order in (("bgr", "gray") if c.gray else ("bgr",)):
            want = _want(c, order)
            shape, size = (3,) + want.shape, 3 * want.size
            off = 64 + k % 4
            flat = torch.full((size + 131,), SENTINEL, dtype=torch.uint8, device=engine.device)
            out = flat[off:off + size].view(shape)
            assert out.data_ptr() % 4 == k % 4
            got = engine.jpeg_reconstruct_dev(co, qt, info, order, out=out, orientation=c.tag)
            assert got is out
            host = flat.cpu().numpy()
            assert (host[:off] == SENTINEL).all() and (host[off + size:] == SENTINEL).all(), (c.name, order)
            assert np.array_equal(host[off:off + size].reshape(shape), np.stack([want] * 3)), (c.name, order)


def test_ignore_and_tags_0_and_1_are_the_existing_entry_bit_for_bit(engine):
    for (sampling, size), members in cases.by_picture().items():
        order = "gray" if sampling == "gray" else "bgr"
        plain = engine.jpeg_decode([members[0].blob], order).cpu().numpy()
        for c in (members[0], members[1]):
            assert np.array_equal(engine.jpeg_decode([c.blob], order, orientation="exif").cpu().numpy(), plain), c.name
        for c in (members[1], members[6], members[7]):                          # a tag that is there is not applied unless asked for
            assert np.array_equal(engine.jpeg_decode([c.blob], order).cpu().numpy(), plain), c.name
            assert np.array_equal(engine.jpeg_decode([c.blob], order, orientation="ignore").cpu().numpy(), plain), c.name
        coeffs, qtables, info = jpeg.entropy_decode(members[6].blob)
        co, qt = torch.from_numpy(coeffs[None]).to(engine.device), torch.from_numpy(qtables[None].view(np.int16)).to(engine.device)
        for tag in (0, 1):
            assert np.array_equal(engine.jpeg_reconstruct_dev(co, qt, info, order, orientation=tag).cpu().numpy(), plain), (sampling, size, tag)


def test_mixed_tags_in_one_launch_and_bad_tags_are_refused(engine):
    from chessvision.hip_backend import HipBackendError

    members = cases.by_picture()[("420", (15, 33))]
    blobs = [members[t].blob for t in (6, 6, 0, 6, 8)]
    with pytest.raises(ValueError, match=r"\[2, 4\]"):
        engine.jpeg_decode(blobs, orientation="exif")
    assert tuple(engine.jpeg_decode(blobs).shape) == (5, 15, 33, 3)                            # the tags do not matter unless asked for
    assert tuple(engine.jpeg_decode([members[0].blob, members[1].blob], orientation="exif").shape) == (2, 15, 33, 3)   # absent and 1: one key
    with pytest.raises(ValueError, match="orientation"):
        engine.jpeg_decode(blobs, orientation="auto")
    coeffs, qtables, info = jpeg.entropy_decode(members[6].blob)
    co, qt = torch.from_numpy(coeffs[None]).to(engine.device), torch.from_numpy(qtables[None].view(np.int16)).to(engine.device)
    for bad in (9, -1, "6"):
        with pytest.raises(ValueError, match="0..8"):
            engine.jpeg_reconstruct_dev(co, qt, info, orientation=bad)
    with pytest.raises(HipBackendError, match="shape"):                                          # the plain shape is not tag 6's
        engine.jpeg_reconstruct_dev(co, qt, info, out=torch.empty((1, 15, 33, 3), dtype=torch.uint8, device=engine.device), orientation=6)
    import ctypes

    from chessvision.hip_backend import _ptr, _stream_ptr
    planes = torch.empty(64 * info.blocks, dtype=torch.uint8, device=engine.device)
    out = torch.full((1, 33, 15, 3), SENTINEL, dtype=torch.uint8, device=engine.device)
    c_info = info.to_c()
    for bad in (9, -1):
        status = engine._lib.cv_jpeg_reconstruct_oriented_u8(engine._h, _ptr(co), _ptr(qt), 1, ctypes.addressof(c_info), 0, bad, _ptr(planes),
                                                             planes.numel(), _ptr(out), _stream_ptr(engine.device))
        assert status != 0 and b"orientation must be 0..8" in engine._lib.cv_last_error()
    assert bool((out == SENTINEL).all())


def test_decode_jpegs_groups_mixed_tags_and_geometries_and_keeps_input_order(cv):
    pictures = cases.by_picture()
    picks = [pictures[("420", (15, 33))][6], pictures[("444", (33, 15))][8], pictures[("420", (15, 33))][0], pictures[("gray", (3, 5))][5],
             pictures[("420", (15, 33))][6], pictures[("422", (67, 31))][7], pictures[("420", (15, 33))][3], pictures[("420", (15, 33))][1]]
    got = cv.decode_jpegs([c.blob for c in picks], "rgb", orientation="exif")
    assert [g.shape for g in got] == [(33, 15, 3), (15, 33, 3), (15, 33, 3), (5, 3, 3), (33, 15, 3), (31, 67, 3), (15, 33, 3), (15, 33, 3)]
    for g, c in zip(got, picks):
        assert np.array_equal(g, _want(c, "rgb")), c.name
    plain = cv.decode_jpegs([c.blob for c in picks], "rgb")
    assert [p.shape for p in plain] == [(15, 33, 3), (33, 15, 3), (15, 33, 3), (3, 5, 3), (15, 33, 3), (67, 31, 3), (15, 33, 3), (15, 33, 3)]


# ---- the pipeline on turned photos ---------------------------------------------------------------------------------------------------
H, W = 256, 320
TAGS = [0, 6, 8, 3, 5, 1]


@pytest.fixture(scope="module")
def uploads():
    """Six synthetic board photos of 256 x 320 (the board in the left 256 columns), each stored as the camera would have held it for
    its tag: (blobs, the upright BGR photos ``apply_orientation(decode, tag)``)."""
    rng = np.random.default_rng(77)
    blobs, upright = [], []
    for k, tag in enumerate(TAGS):
        photo = rng.integers(0, 36, (H, W, 3), dtype=np.uint8)
        photo[:, :H] = synthetic.board_photo(2100 + k, H)
        buf = io.BytesIO()
        kw = {}
        if tag:
            kw["exif"] = Image.Exif()
            kw["exif"][0x0112] = tag
        Image.fromarray(np.ascontiguousarray(photo[:, :, ::-1]), "RGB").save(buf, "JPEG", quality=90, **kw)
        blobs.append(buf.getvalue())
        info = jpeg.jpeg_info(blobs[-1])
        assert (info.height, info.width, info.orientation) == (H, W, tag)
        upright.append(np.ascontiguousarray(jpeg.apply_orientation(jpeg.decode(blobs[-1], "bgr"), tag)))
    assert [a.shape for a in upright] == [(H, W, 3), (W, H, 3), (W, H, 3), (H, W, 3), (W, H, 3), (H, W, 3)]
    return blobs, upright


def _jpegs_equal(got, want):
    assert [r.board_jpeg for r in got] == [r.board_jpeg for r in want] and all(r.board_jpeg for r in want if r.position is not None)


def test_process_encoded_exif_equals_process_images_of_the_upright_photos(cv, uploads):
    """One image per job on both sides, so that every launch has the same form on both (the launch planner chooses kernels by the
    images in a launch): ONE ``process_images`` call over the six upright arrays is the expected result."""
    blobs, upright = uploads
    kw = {"fallback_quad": True, "pipeline_chunk": 1, "board_jpeg": 90}
    timings: dict = {}
    got = cv.process_encoded(blobs, orientation="exif", timings=timings, **kw)
    want = cv.process_images(upright, **kw)
    assert timings["jobs"] == 6 and sum(r.position is not None for r in want) == 6
    assert_equal_results(got, want)
    _jpegs_equal(got, want)
    # the tag matters: the same streams without the keyword are the photos as stored
    stored = cv.process_encoded(blobs, **kw)
    assert not np.array_equal(stored[1].board_extraction.probabilities, got[1].board_extraction.probabilities)
    assert_equal_results([stored[0], stored[5]], [got[0], got[5]])


def test_process_encoded_exif_plans_jobs_by_tag_at_the_default_chunk(cv, uploads):
    """Default chunk: the six streams share a geometry and fall into the jobs [0, 5], [1], [2], [3], [4] by effective tag.  The expected
    results are ``process_images`` of the same upright arrays launch by launch, i.e. with the images per launch the jobs have."""
    blobs, upright = uploads
    timings: dict = {}
    got = cv.process_encoded(blobs, orientation="exif", fallback_quad=True, first_job=0, timings=timings)
    assert timings["jobs"] == 5
    want: list = [None] * 6
    for ids in ([0, 5], [1], [2], [3], [4]):
        for i, r in zip(ids, cv.process_images([upright[i] for i in ids], fallback_quad=True, first_job=0)):
            want[i] = r
    assert_equal_results(got, want)
    assert all(r.board_extraction.quadrangle is not None for r in got)


def test_process_jpeg_exif_equals_process_image_of_the_upright_photo(cv):
    rng = np.random.default_rng(78)
    for k, tag in enumerate((6, 7)):
        photo = rng.integers(0, 36, (H, W, 3), dtype=np.uint8)
        photo[:, :H] = synthetic.board_photo(2200 + k, H)
        exif = Image.Exif()
        exif[0x0112] = tag
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(photo[:, :, ::-1]), "RGB").save(buf, "JPEG", quality=90, exif=exif)
        blob = buf.getvalue()
        stored = jpeg.decode(blob, "bgr")
        upright = np.ascontiguousarray(jpeg.apply_orientation(stored, tag))
        assert upright.shape == (W, H, 3)
        assert_equal_results([cv.process_jpeg(blob, orientation="exif")], [cv.process_image(upright)])
        assert_equal_results([cv.process_jpeg(blob, threshold=0.3, flip=True, orientation="exif")],
                             [cv.process_image(upright, threshold=0.3, flip=True)])
        assert_equal_results([cv.process_jpeg(blob)], [cv.process_image(stored)])               # the default is the call it was
        assert_equal_results([cv.process_jpeg(blob, orientation="ignore")], [cv.process_image(stored)])

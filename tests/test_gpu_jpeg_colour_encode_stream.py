"""GPU: ``cv_jpeg_encode_colour_u8`` held to the header's stream contract with the probe of tests/stream_probe.py, exactly as each row
of tests/test_gpu_stream_contract.py is: every launch of the chain is ordered on the stream the call was handed -- it reads the pixels
a copy EARLIER on that stream wrote, behind a delay -- and the call returns to the host while the delay is still running.  One row:
the three images of the (17, 33) 4:2:0 quality-95 group (partial MCUs on both edges).  And "gray and colour encodes of one engine are
ordered on the device, whatever their streams": a colour encode waits behind a delay on one stream while a gray encode of the same
engine, which uses the same scratch, is issued on another."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jpeg_colour_encode_cases as cases
import jpeg_encode_cases as gray_cases
import stream_probe as sp
from chessvision import hip_backend as hb
from chessvision import jpeg

pytestmark = pytest.mark.gpu
H, W, SUB, Q, N = 17, 33, "4:2:0", 95, 3
U8, I32, I64 = torch.uint8, torch.int32, torch.int64


def _group():
    for name, q, sub, order, images, files in cases.groups(cases.load()):
        if name == f"{H}x{W}-{SUB}-q{Q}":
            return images, files
    raise AssertionError("the group is not in the golden file")


def _files(outs_cpu):
    """(offsets, lengths, the files): the bytes between the files and behind the last one are not part of the result."""
    out, offsets, lengths = (t.numpy() for t in outs_cpu)
    files = tuple(out[int(o):int(o) + max(0, int(k))].tobytes() if 0 <= int(o) <= out.size else b"" for o, k in zip(offsets[:-1], lengths))
    return (offsets.tobytes(), lengths.tobytes(), files)


def _inputs(true: bool) -> list:
    images = _group()[0]
    return [torch.from_numpy(np.ascontiguousarray(images if true else images[::-1]))]


def _outputs(ctx) -> list:
    return [((N * hb.jpeg_colour_max_bytes(H, W, SUB),), U8), ((N + 1,), I64), ((N,), I32)]


def _colour(lib, eng, images, out, offsets, lengths, sub, q, stream) -> None:
    n, h, w, _ = images.shape
    status = lib.cv_jpeg_encode_colour_u8(eng._h, images.data_ptr(), n, h, w, jpeg.ORDERS["bgr"], hb.JPEG_SUBSAMPLINGS[sub], q, out.data_ptr(),
                                          out.numel(), offsets.data_ptr(), lengths.data_ptr(), stream)
    assert status == 0, (status, lib.cv_last_error())


def _call(ctx, ins, outs, stream) -> None:
    _colour(ctx.lib, ctx.engine, ins[0], outs[0], outs[1], outs[2], SUB, Q, stream)


ROW = sp.Row(f"cv_jpeg_encode_colour_u8-{H}x{W}-420-q{Q}", _inputs, _outputs, _call, canon=_files, reps=3)


@pytest.fixture(scope="module")
def ctx():
    engine = hb.HipEngine(precision="f32")
    torch.cuda.synchronize()
    yield SimpleNamespace(engine=engine, lib=engine._lib)
    engine.close()


@pytest.fixture(scope="module")
def probe(ctx):
    p = sp.Probe()
    p.baselines = {ROW.name: p.baseline(ctx, ROW)}
    p.choose_delay(p.baselines)
    assert p.pick_streams() and all(p.control_result.values()), p.control_log
    yield p


def test_control_sees_a_default_stream_kernel_read_the_decoy(probe):
    assert probe.control_result == {"read_decoy": True, "delay_outlasted_kernel": True, "copy_landed": True}


def test_the_default_stream_result_is_the_committed_files(ctx, probe):
    """What the probe compares against is the right answer: libjpeg's files for the three images, in 16-byte steps."""
    offsets, lengths, files = probe.baselines[ROW.name].y_true
    assert files == tuple(_group()[1])
    ln = np.frombuffer(lengths, np.int32)
    assert np.array_equal(np.frombuffer(offsets, np.int64), np.concatenate([[0], np.cumsum((ln + 15) // 16 * 16)]))


def test_entry_is_ordered_on_its_stream_and_returns_before_the_stream_gets_there(ctx, probe):
    outcomes = probe.run(ctx, ROW, probe.baselines[ROW.name])
    print(f"{ROW.name}: default-stream call {probe.baselines[ROW.name].ms:.3f} ms; " +
          ", ".join(f"rep {o.rep}: {o.verdict}, returned {'early' if o.returned_early else 'LATE'}" for o in outcomes))
    for o in outcomes:
        assert o.verdict == "true", (
            f"{ROW.name}, call {o.rep} on the side stream: the output holds '{o.verdict}' where the default-stream result was expected "
            "('decoy': work ran before the stream's earlier copy; 'sentinel': the last kernel ran elsewhere)")
    late = [o.rep for o in outcomes[1:] if not o.returned_early]
    assert not late, f"{ROW.name}: calls {late} returned only after the {probe.delay_ms:.0f} ms delay in front of them had run out"


def _held(probe, stream):
    """The delay on ``stream`` and the event behind it."""
    after = torch.cuda.Event()
    with torch.cuda.stream(stream):
        probe.sleep_ms(probe.delay_ms)
        after.record(stream)
    return after


@pytest.mark.parametrize("gray_geometry", [(33, 40), (128, 128)], ids=["gray-fits-the-scratch", "gray-grows-the-scratch"])
def test_a_colour_and_a_gray_encode_share_the_scratch_in_device_order_whatever_their_streams(ctx, probe, gray_geometry):
    """The colour encode is queued on s1 behind a delay; the gray encode of the same engine goes to s2 straight after it.  Both carve
    the one scratch from its start, so the gray one must wait for the colour one on the device (the ``jpeg_enc_done`` event), and a
    gray geometry that needs more scratch re-allocates it only once the colour encode has left it.  Expected: the committed files."""
    z = gray_cases.load()
    eng = hb.HipEngine(precision="f32")                                     # an engine whose scratch has held nothing yet
    try:
        colour, colour_files = _group()
        colour = torch.from_numpy(np.ascontiguousarray(colour)).cuda()
        h, w = gray_geometry
        kinds = gray_cases.group_kinds(gray_cases.GEOMETRIES.index((h, w)), gray_cases.QUALITIES.index(95))
        gray = torch.from_numpy(np.stack([z[f"image/{h}x{w}/{k}"] for k in kinds])).cuda()
        gray_files = [z[f"file/{h}x{w}/q95/{k}"].tobytes() for k in kinds]

        def buffers(each):
            made = (torch.empty(N * each, dtype=U8, device="cuda"), torch.empty(N + 1, dtype=I64, device="cuda"),
                    torch.empty(N, dtype=I32, device="cuda"))
            for t in made:
                sp.fill_sentinel(t)
            return made

        outs_c, outs_g, warm = buffers(hb.jpeg_colour_max_bytes(H, W, SUB)), buffers(hb.jpeg_gray_max_bytes(h, w)), buffers(hb.jpeg_colour_max_bytes(H, W, SUB))
        torch.cuda.synchronize()
        s1, s2 = probe.side, probe.s2
        _colour(ctx.lib, eng, colour, *warm, SUB, Q, s1.cuda_stream)        # the scratch exists for the colour geometry
        torch.cuda.synchronize()
        after = _held(probe, s1)
        _colour(ctx.lib, eng, colour, *outs_c, SUB, Q, s1.cuda_stream)
        assert not after.query(), "the s1 encode waited for its stream: the case would test nothing"
        status = ctx.lib.cv_jpeg_encode_gray_u8(eng._h, gray.data_ptr(), N, h, w, 95, outs_g[0].data_ptr(), outs_g[0].numel(), outs_g[1].data_ptr(),
                                                outs_g[2].data_ptr(), s2.cuda_stream)
        assert status == 0, (status, ctx.lib.cv_last_error())
        s1.synchronize()
        s2.synchronize()
        assert _files([t.cpu() for t in outs_c])[2] == tuple(colour_files)
        assert _files([t.cpu() for t in outs_g])[2] == tuple(gray_files)
    finally:
        eng.close()

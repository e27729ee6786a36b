"""GPU: ``cv_jpeg_reconstruct_oriented_u8`` held to the header's stream contract with the probe of tests/stream_probe.py, exactly as each
row of tests/test_gpu_stream_contract.py is: both launches (inverse DCT, oriented colour stage) are ordered on the stream the call was
handed -- they read the coefficients a copy EARLIER on that stream wrote, behind a delay -- and the call returns to the host while the
delay is still running.  Tag 6 on the three streams of the 4:2:0 33 x 17 group: two tiles of the oriented kernel per image, the second
one pixel wide."""
from __future__ import annotations

import ctypes
import functools
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stream_probe as sp
from chessvision import hip_backend as hb
from chessvision import jpeg

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
TAG = 6


@functools.lru_cache(maxsize=None)
def _group():
    """The three streams of the 420_33x17 group after the host Huffman stage: [(coeffs, qtables)], info, its C form."""
    z = np.load(GOLDEN / "jpeg_cases.npz")
    blobs = [z[f"blob/{name}"].tobytes() for name, kind, group in zip(z["names"], z["kind"], z["group"])
             if str(kind) == "group" and str(group) == "420_33x17"]
    assert len(blobs) == 3
    decoded = [jpeg.entropy_decode(b) for b in blobs]
    info = decoded[0][2]
    return [(c, q) for c, q, _ in decoded], info, info.to_c()


def _inputs(true: bool) -> list:
    decoded = _group()[0]
    order = [0, 1, 2] if true else [2, 0, 1]
    return [torch.from_numpy(np.stack([decoded[k][0] for k in order])),
            torch.from_numpy(np.stack([decoded[k][1] for k in order]).view(np.int16))]


def _outputs(ctx) -> list:
    return [((3,) + jpeg.oriented_shape(_group()[1], TAG) + (3,), torch.uint8)]


def _call(ctx, ins, outs, stream) -> None:
    _, info, c_info = _group()
    status = ctx.lib.cv_jpeg_reconstruct_oriented_u8(ctx.engine._h, ins[0].data_ptr(), ins[1].data_ptr(), 3, ctypes.addressof(c_info),
                                                     jpeg.ORDERS["bgr"], TAG, ctx.planes.data_ptr(), ctx.planes.numel(), outs[0].data_ptr(), stream)
    assert status == 0, (status, ctx.lib.cv_last_error())


ROW = sp.Row("cv_jpeg_reconstruct_oriented_u8-420_33x17-tag6", _inputs, _outputs, _call, reps=3)


@pytest.fixture(scope="module")
def ctx():
    engine = hb.HipEngine(precision="f32")
    planes = torch.empty(3 * 64 * _group()[1].blocks, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    yield SimpleNamespace(engine=engine, lib=engine._lib, planes=planes)
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


def test_the_default_stream_result_is_the_turned_picture(ctx, probe):
    """What the probe compares against is the right answer: image k is the numpy reconstruction of stream k, turned by tag 6."""
    decoded, info, _ = _group()
    want = np.stack([jpeg.apply_orientation(jpeg.reconstruct(c, q, info, "bgr"), TAG) for c, q in decoded])
    assert want.shape == (3, 33, 17, 3) and probe.baselines[ROW.name].y_true == (want.tobytes(),)


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

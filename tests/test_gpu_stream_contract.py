"""GPU: every stream-taking device entry point of include/chessvision_hip.h held to its stream contract OFF the default stream.

The header promises "asynchronous with respect to the host and ordered on `stream`" for almost every device entry; every other test
passes the legacy default stream, where that holds whatever the library does, while the product runs on side streams (three per call
in batched.py / encoded.py, one per request slot in core.py).  Here each entry runs behind a measured delay on a side stream and must
(a) produce, by the time that stream reaches the end of the call, exactly what it produces on the default stream -- its inputs are
only put in place ON that stream, behind the delay, so anything the library issues elsewhere reads a decoy -- and (b) return to the
host while the delay is still running (tests/stream_probe.py has the mechanism and its control).  The table below is one row per entry
and shape.  The second half runs ONE engine from two streams: the cached resize tables, the encoder's scratch, a model's workspace.

Bars: equality of bytes with the default-stream result of the same call, which the rest of the suite already holds to float64 /
byte references.  Nothing here sets an environment variable, and the module opens three streams of its own."""
from __future__ import annotations

import ctypes
import functools
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jpeg_encode_cases as enc_cases
import layer_local as ll
import stream_probe as sp
from chessvision import hip_backend as hb
from chessvision import jpeg
from oracle import synth

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
F32, U8, I16, I32, I64, I8, F64 = torch.float32, torch.uint8, torch.int16, torch.int32, torch.int64, torch.int8, torch.float64
UNET_TAP = "down4.maxpool_conv.1.double_conv.5"          # the bottleneck, the reference's hook point
NORM = (0.564, 0.246)                                    # train_classifier.py's val_transforms


def _p(t):
    return None if t is None else int(t.data_ptr())


def _ok(status: int) -> None:
    hb._check(status)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def _unet_u8(n: int, true: bool) -> np.ndarray:
    kinds = (["random", "photo", "border"] if true else ["photo", "random", "random"])[:n]
    return ll.unet_images_u8((40 if true else 50) + n, kinds)


def _squares(n: int, true: bool) -> np.ndarray:
    specials = {i: kind for i, kind in ll.specials_from(2 if true else 0).items() if i < n}
    return ll.squares_u8((60 if true else 70) + n, n, specials)


def _unet_rows():
    def rows_of(n):                                       # a function, so that every closure below binds this n
        as_f32 = lambda true: [ll.unet_f32(_unet_u8(n, true))]
        as_u8 = lambda true: [torch.from_numpy(_unet_u8(n, true))]
        logits, mask = ((n, 1, 256, 256), F32), ((n, 256, 256), U8)
        emb = lambda ctx: ((n, ctx.unet.embedding_dim("unet")), F32)
        entries = [
            ("cv_unet_forward", as_f32, lambda ctx: [logits],
             lambda ctx, i, o, s: _ok(ctx.lib.cv_unet_forward(ctx.unet._h, _p(i[0]), n, _p(o[0]), s))),
            ("cv_unet_forward_u8", as_u8, lambda ctx: [logits, mask],
             lambda ctx, i, o, s: _ok(ctx.lib.cv_unet_forward_u8(ctx.unet._h, _p(i[0]), n, _p(o[0]), _p(o[1]), 0.5, s))),
            ("cv_unet_forward_mask", as_f32, lambda ctx: [logits, mask, emb(ctx)],
             lambda ctx, i, o, s: _ok(ctx.lib.cv_unet_forward_mask(ctx.unet._h, _p(i[0]), n, _p(o[0]), _p(o[1]), 0.5, _p(o[2]), s))),
            ("cv_unet_forward_emb", as_f32, lambda ctx: [logits, emb(ctx)],
             lambda ctx, i, o, s: _ok(ctx.lib.cv_unet_forward_emb(ctx.unet._h, _p(i[0]), n, _p(o[0]), _p(o[1]), s))),
            ("cv_unet_forward_u8_emb", as_u8, lambda ctx: [logits, mask, emb(ctx)],
             lambda ctx, i, o, s: _ok(ctx.lib.cv_unet_forward_u8_emb(ctx.unet._h, _p(i[0]), n, _p(o[0]), _p(o[1]), 0.5, _p(o[2]), s))),
        ]
        # three calls on fixed buffers: eager, capture, hipGraph replay (N = 1); N = 3 is chunks of 2 + 1 and runs eagerly every time
        return [sp.Row(f"{name}-N{n}", make, outs, call, reps=3) for name, make, outs, call in entries]

    return rows_of(1) + rows_of(3)


def _resnet_rows():
    def rows_of(n):
        as_f32 = lambda true: [ll.squares_f32(_squares(n, true))]
        as_u8 = lambda true: [torch.from_numpy(_squares(n, true))]
        out, emb = ((n, 13), F32), ((n, 512), F32)
        entries = [
            ("cv_resnet18_forward", as_f32, lambda ctx: [out],
             lambda ctx, i, o, s: _ok(ctx.lib.cv_resnet18_forward(ctx.resnet._h, _p(i[0]), n, _p(o[0]), s))),
            ("cv_resnet18_forward_u8", as_u8, lambda ctx: [out],
             lambda ctx, i, o, s: _ok(ctx.lib.cv_resnet18_forward_u8(ctx.resnet._h, _p(i[0]), n, _p(o[0]), s))),
            ("cv_resnet18_forward_emb", as_f32, lambda ctx: [out, emb],
             lambda ctx, i, o, s: _ok(ctx.lib.cv_resnet18_forward_emb(ctx.resnet._h, _p(i[0]), n, _p(o[0]), _p(o[1]), s))),
            ("cv_resnet18_forward_u8_emb", as_u8, lambda ctx: [out, emb],
             lambda ctx, i, o, s: _ok(ctx.lib.cv_resnet18_forward_u8_emb(ctx.resnet._h, _p(i[0]), n, _p(o[0]), _p(o[1]), s))),
            ("cv_resnet_forward_u8_norm", as_u8, lambda ctx: [out, emb],       # the constants never change: one graph key
             lambda ctx, i, o, s: _ok(ctx.lib.cv_resnet_forward_u8_norm(ctx.resnet._h, _p(i[0]), n, NORM[0], NORM[1], 0, _p(o[0]), _p(o[1]), s))),
        ]
        return [sp.Row(f"{name}-n{n}", make, outs, call, reps=3 if n < 200 else 2) for name, make, outs, call in entries]

    return rows_of(7) + rows_of(64) + rows_of(200)


def _channel_means_rows():
    """The forward and the pooling of its tap on the same stream: the workspace is the pooling's input, so the decoy is put there by a
    default-stream forward in front of every probe (``prepare``)."""
    scratch = {}

    def logits_scratch(key, shape):
        if key not in scratch:
            scratch[key] = torch.empty(shape, dtype=F32, device="cuda")
        return scratch[key]

    def unet_call(ctx, i, o, s):
        _ok(ctx.lib.cv_unet_forward(ctx.unet._h, _p(i[0]), 1, _p(logits_scratch(("u", i[0].data_ptr()), (1, 1, 256, 256))), s))
        dims = (ctypes.c_int64 * 2)()
        _ok(ctx.lib.cv_activation_channel_means(ctx.unet._h, b"unet", UNET_TAP.encode(), _p(o[0]), o[0].numel(), dims, s))
        assert tuple(dims) == tuple(o[0].shape)

    def resnet_call(ctx, i, o, s):
        _ok(ctx.lib.cv_resnet18_forward(ctx.resnet._h, _p(i[0]), 7, _p(logits_scratch(("r", i[0].data_ptr()), (7, 13))), s))
        dims = (ctypes.c_int64 * 2)()
        _ok(ctx.lib.cv_activation_channel_means(ctx.resnet._h, b"resnet18", b"global_pool", _p(o[0]), o[0].numel(), dims, s))
        assert tuple(dims) == tuple(o[0].shape)

    def unet_prepare(ctx, decoy):
        _ok(ctx.lib.cv_unet_forward(ctx.unet._h, _p(decoy[0]), 1, _p(logits_scratch(("u", decoy[0].data_ptr()), (1, 1, 256, 256))), 0))

    def resnet_prepare(ctx, decoy):
        _ok(ctx.lib.cv_resnet18_forward(ctx.resnet._h, _p(decoy[0]), 7, _p(logits_scratch(("r", decoy[0].data_ptr()), (7, 13))), 0))

    return [
        sp.Row("cv_activation_channel_means-unet", lambda true: [ll.unet_f32(_unet_u8(1, true))],
               lambda ctx: [((1, ctx.unet.embedding_dim("unet")), F32)], unet_call, reps=3, prepare=unet_prepare),
        sp.Row("cv_activation_channel_means-resnet", lambda true: [ll.squares_f32(_squares(7, true))],
               lambda ctx: [((7, 512), F32)], resnet_call, reps=3, prepare=resnet_prepare),
    ]


def _rng(seed: int):
    return np.random.default_rng(seed)


def _logits(seed: int, shape) -> torch.Tensor:
    return torch.from_numpy((_rng(seed).standard_normal(shape) * 3).astype(np.float32))


def _small_rows():
    thresholds = np.array([0.25, 0.5, 0.75], np.float32)
    fp = ctypes.POINTER(ctypes.c_float)

    def labels13(true):
        return torch.from_numpy(_rng(5 if true else 6).integers(-1, 13, 5).astype(np.int8))

    def seg_inputs(true):
        return [_logits(11 if true else 12, (2, 1000)), torch.from_numpy((_rng(13 if true else 14).integers(0, 2, (2, 1000)) * 255).astype(np.uint8))]

    return [
        sp.Row("cv_softmax13-n5", lambda true: [_logits(1 if true else 2, (5, 13))], lambda ctx: [((5, 13), F32)],
               lambda ctx, i, o, s: _ok(ctx.lib.cv_softmax13(ctx.unet._h, _p(i[0]), 5, _p(o[0]), s))),
        sp.Row("cv_square_records-n5", lambda true: [_logits(3 if true else 4, (5, 13)), labels13(true)],
               lambda ctx: [((5, hb.SQUARE_RECORD.itemsize), U8)],
               lambda ctx, i, o, s: _ok(ctx.lib.cv_square_records(ctx.unet._h, _p(i[0]), _p(i[1]), 5, _p(o[0]), s))),
        sp.Row("cv_extraction_scores-2x1000", lambda true: [_logits(7 if true else 8, (2, 1000))],
               lambda ctx: [((2, hb.SCORE_RECORD.itemsize), U8), ((2, 1000), U8)],
               lambda ctx, i, o, s: _ok(ctx.lib.cv_extraction_scores(ctx.unet._h, _p(i[0]), 2, 1000, 1, _p(o[0]), _p(o[1]), s))),
        sp.Row("cv_segmentation_scores-2x1000", seg_inputs, lambda ctx: [((2, hb.SEG_RECORD.itemsize), U8)],
               lambda ctx, i, o, s: _ok(ctx.lib.cv_segmentation_scores(ctx.unet._h, _p(i[0]), _p(i[1]), 2, 1000, 0.5, _p(o[0]), s))),
        sp.Row("cv_threshold_levels-2x1000x3", seg_inputs, lambda ctx: [((2, 1000), U8), ((2, hb.LEVEL_RECORD.itemsize), U8)],
               lambda ctx, i, o, s: _ok(ctx.lib.cv_threshold_levels(ctx.unet._h, _p(i[0]), _p(i[1]), 2, 1000, thresholds.ctypes.data_as(fp), 3,
                                                                    _p(o[0]), _p(o[1]), s))),
    ]


def _photo_batch(seed: int, n: int, h: int, w: int, c: int) -> torch.Tensor:
    return torch.from_numpy(_rng(seed).integers(0, 256, (n, h, w, c), dtype=np.uint8))


def _resize_rows():
    def area(h, w, c):
        return sp.Row(f"cv_resize_area_u8-{h}x{w}x{c}", lambda true: [_photo_batch((20 if true else 30) + h, 2, h, w, c)],
                      lambda ctx: [((2, 16, 16, c), U8)],
                      lambda ctx, i, o, s: _ok(ctx.lib.cv_resize_area_u8(ctx.unet._h, _p(i[0]), 2, h, w, c, _p(o[0]), 16, 16, s)))

    # 2x2 three-channel kernel; table kernel (its tables are cached from the second call on); the enlarging form of the generic kernel
    rows = [area(32, 32, 3), area(42, 42, 3), area(10, 12, 1)]
    rows.append(sp.Row("cv_resize_antialias_f32-42x42x3", lambda true: [_photo_batch(24 if true else 34, 2, 42, 42, 3)],
                       lambda ctx: [((2, 3, 16, 16), F32)],
                       lambda ctx, i, o, s: _ok(ctx.lib.cv_resize_antialias_f32(ctx.unet._h, _p(i[0]), 2, 42, 42, 3, _p(o[0]), 16, 16, s))))
    return rows


@functools.lru_cache(maxsize=None)
def _inverse_maps() -> np.ndarray:
    quad = np.array([[[44, 5], [6, 3], [4, 58], [45, 60]]], np.float32)                 # TR, TL, BL, BR inside the 64 x 48 photo
    return hb.board_homographies(quad)                                                  # (1, 3, 3) float64, cv_board_homographies


def _extract_rows():
    h, w = 64, 48
    dp = ctypes.POINTER(ctypes.c_double)
    outs = lambda ctx: [((64, 64, 64), U8), ((1, 512, 512), U8)]
    photo = lambda true: _photo_batch(41 if true else 42, 1, h, w, 3)
    return [
        sp.Row("cv_extract_squares_u8_dev", lambda true: [photo(true), torch.from_numpy(_inverse_maps().reshape(1, 9).copy())], outs,
               lambda ctx, i, o, s: _ok(ctx.lib.cv_extract_squares_u8_dev(ctx.unet._h, _p(i[0]), 1, h, w, _p(i[1]), _p(o[0]), _p(o[1]), s))),
        # host matrices: the header says it synchronises `stream` before returning -- the result is held to the contract, the return is not
        sp.Row("cv_extract_squares_u8", lambda true: [photo(true)], outs,
               lambda ctx, i, o, s: _ok(ctx.lib.cv_extract_squares_u8(ctx.unet._h, _p(i[0]), 1, h, w, _inverse_maps().ctypes.data_as(dp),
                                                                      _p(o[0]), _p(o[1]), s)),
               asynchronous=False),
    ]


@functools.lru_cache(maxsize=None)
def _jpeg_group():
    """The three streams of the 420_33x17 group after the host Huffman stage: [(coeffs, qtables)], info, its C form."""
    z = np.load(GOLDEN / "jpeg_cases.npz")
    blobs = [z[f"blob/{name}"].tobytes() for name, kind, group in zip(z["names"], z["kind"], z["group"])
             if str(kind) == "group" and str(group) == "420_33x17"]
    assert len(blobs) == 3
    decoded = [jpeg.entropy_decode(b) for b in blobs]
    info = decoded[0][2]
    return [(c, q) for c, q, _ in decoded], info, info.to_c()


def _jpeg_rows():
    planes = {}

    def inputs(true):
        decoded = _jpeg_group()[0]
        order = [0, 1, 2] if true else [2, 0, 1]
        return [torch.from_numpy(np.stack([decoded[k][0] for k in order])),
                torch.from_numpy(np.stack([decoded[k][1] for k in order]).view(np.int16))]

    def reconstruct(ctx, i, o, s):
        _, info, c_info = _jpeg_group()
        if "p" not in planes:
            planes["p"] = torch.empty(3 * 64 * info.blocks, dtype=U8, device="cuda")
        _ok(ctx.lib.cv_jpeg_reconstruct_u8(ctx.unet._h, _p(i[0]), _p(i[1]), 3, ctypes.addressof(c_info), jpeg.ORDERS["bgr"], _p(planes["p"]),
                                           planes["p"].numel(), _p(o[0]), s))

    kinds = enc_cases.group_kinds(enc_cases.GEOMETRIES.index((33, 40)), enc_cases.QUALITIES.index(95))

    def images(true):
        z = enc_cases.load()
        return [torch.from_numpy(np.stack([z[f"image/33x40/{k}"] for k in (kinds if true else kinds[::-1])]))]

    def encode(ctx, i, o, s):
        _ok(ctx.lib.cv_jpeg_encode_gray_u8(ctx.unet._h, _p(i[0]), 3, 33, 40, 95, _p(o[0]), o[0].numel(), _p(o[1]), _p(o[2]), s))

    return [
        sp.Row("cv_jpeg_reconstruct_u8-420_33x17", inputs,
               lambda ctx: [((3, _jpeg_group()[1].height, _jpeg_group()[1].width, 3), U8)], reconstruct),
        sp.Row("cv_jpeg_encode_gray_u8-33x40-q95", images,
               lambda ctx: [((3 * hb.jpeg_gray_max_bytes(33, 40),), U8), ((4,), I64), ((3,), I32)], encode, canon=_files),
    ]


def _files(outs_cpu):
    """(offsets, lengths, the files): the bytes between the files and behind the last one are not part of the result."""
    out, offsets, lengths = (t.numpy() for t in outs_cpu)
    files = tuple(out[int(o):int(o) + max(0, int(k))].tobytes() if 0 <= int(o) <= out.size else b"" for o, k in zip(offsets[:-1], lengths))
    return (offsets.tobytes(), lengths.tobytes(), files)


ROWS = _unet_rows() + _resnet_rows() + _channel_means_rows() + _small_rows() + _resize_rows() + _extract_rows() + _jpeg_rows()
ROW_IDS = [r.name for r in ROWS]
# entries that may wait for their stream before they return.  An entry belongs here only if include/chessvision_hip.h says that it
# synchronises, and why.
SYNCHRONISING = {"cv_extract_squares_u8"}


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    unet = hb.HipEngine(precision="f16x3", unet_chunk=2, resnet_chunk=128)
    unet.load_unet(synth.make_unet(seed=1).state_dict())
    resnet = hb.HipEngine(precision="f16r", unet_chunk=2, resnet_chunk=128)
    resnet.load_resnet18(synth.make_resnet(seed=2).state_dict())
    made = SimpleNamespace(unet=unet, resnet=resnet, lib=unet._lib)
    yield made
    try:
        unet.check_numerics()
        resnet.check_numerics()
    finally:
        unet.close()
        resnet.close()


@pytest.fixture(scope="module")
def probe(ctx):
    """Every row's default-stream results, the delay sized from them, the control (which also picks the side stream: a module whose
    control fails on all of its streams cannot see anything and fails here, for every test), the warm-up on the probes' stream."""
    p = sp.Probe()
    p.baselines = {row.name: p.baseline(ctx, row) for row in ROWS}
    delay = p.choose_delay(p.baselines)
    seen_something = p.pick_streams()
    print(f"\nstream probe: delay {delay:.1f} ms = clamp(20 x {p.longest[1]:.3f} ms of {p.longest[0]}, 50, 500); "
          f"_sleep {p.cycles_per_ms:.0f} ticks / ms; control {p.control_result}; second stream independent: {p.s2_independent}")
    for what, result in p.control_log:
        print(f"  control, {what}: {result}")
    assert seen_something and all(p.control_result.values()), (
        f"the probe cannot see anything on this runtime: a default-stream kernel launched while a side stream held a {delay:.0f} ms delay "
        f"waited for it or read the copy behind it, on each of {len(p.candidates)} side streams ({p.control_log}) -- torch's side streams "
        "are not non-blocking here, every one of them shares the default stream's hardware queue, or the delay is too short")
    with torch.cuda.stream(p.side):                       # order_forward's host wait and the first-use allocations are behind us
        ctx.unet.unet_forward(ll.unet_f32(_unet_u8(3, True)))
        ctx.resnet.resnet18_forward(ll.squares_f32(_squares(200, True)))
    p.side.synchronize()
    yield p


# ---- 1. the control, 2. every entry -----------------------------------------------------------------------------------------------------
def test_control_default_stream_kernel_reads_the_decoy_while_the_side_stream_is_held(probe):
    assert probe.control_result == {"read_decoy": True, "delay_outlasted_kernel": True, "copy_landed": True}
    assert sp.DELAY_MIN_MS <= probe.delay_ms <= sp.DELAY_MAX_MS
    assert probe.delay_ms == min(sp.DELAY_MAX_MS, max(sp.DELAY_MIN_MS, sp.DELAY_FACTOR * max(b.ms for b in probe.baselines.values())))


def test_the_table_names_every_entry_and_exempts_only_what_the_header_says_synchronises():
    names = {r.name.split("-")[0] for r in ROWS}
    assert names == {"cv_unet_forward", "cv_unet_forward_u8", "cv_unet_forward_mask", "cv_unet_forward_emb", "cv_unet_forward_u8_emb",
                     "cv_resnet18_forward", "cv_resnet18_forward_u8", "cv_resnet18_forward_emb", "cv_resnet18_forward_u8_emb",
                     "cv_resnet_forward_u8_norm", "cv_activation_channel_means", "cv_softmax13", "cv_square_records", "cv_extraction_scores",
                     "cv_segmentation_scores", "cv_threshold_levels", "cv_resize_area_u8", "cv_resize_antialias_f32",
                     "cv_extract_squares_u8_dev", "cv_extract_squares_u8", "cv_jpeg_reconstruct_u8", "cv_jpeg_encode_gray_u8"}
    assert {r.name.split("-")[0] for r in ROWS if not r.asynchronous} == SYNCHRONISING
    header = (Path(__file__).resolve().parent.parent / "include" / "chessvision_hip.h").read_text()
    for name in SYNCHRONISING:
        at = header.index(f"int {name}(")
        assert "Synchronises `stream` before returning" in header[header.rindex("/*", 0, at):at], name


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_entry_is_ordered_on_its_stream_and_returns_before_the_stream_gets_there(ctx, probe, row):
    outcomes = probe.run(ctx, row, probe.baselines[row.name])
    print(f"{row.name}: default-stream call {probe.baselines[row.name].ms:.3f} ms; " +
          ", ".join(f"rep {o.rep}: {o.verdict}, returned {'early' if o.returned_early else 'LATE'}" for o in outcomes))
    for o in outcomes:
        assert o.verdict == "true", (
            f"{row.name}, call {o.rep} on the side stream: the outputs hold '{o.verdict}' where the default-stream result was expected "
            "('decoy': work ran before the stream's earlier copy; 'sentinel': the last kernel ran elsewhere)")
    if row.asynchronous:
        late = [o.rep for o in outcomes[1:] if not o.returned_early]
        assert not late, f"{row.name}: calls {late} returned only after the {probe.delay_ms:.0f} ms delay in front of them had run out"
    for eng in (ctx.unet, ctx.resnet):
        _ok(ctx.lib.cv_engine_numeric_status(eng._h, probe.side.cuda_stream))


# ---- 3. shared engine state across two streams --------------------------------------------------------------------------------------
def _held(probe, stream):
    """The delay on ``stream`` and the event behind it."""
    after = torch.cuda.Event()
    with torch.cuda.stream(stream):
        probe.sleep_ms(probe.delay_ms)
        after.record(stream)
    return after


def _first_pixel(got: torch.Tensor, want: torch.Tensor) -> str:
    g, w = got.cpu().numpy(), want.cpu().numpy()
    if np.array_equal(g.view(np.uint8), w.view(np.uint8)):
        return ""
    at = tuple(int(v) for v in np.argwhere(g.view(np.uint8).reshape(g.shape[:-1] + (-1,)) != w.view(np.uint8).reshape(w.shape[:-1] + (-1,)))[0])
    return f"first difference at {at} of {tuple(g.shape)}: {g[at[:-1]].tolist()} for {w[at[:-1]].tolist()}"


def _carved(side: int, seed: int) -> torch.Tensor:
    """A (n, side, side, c) batch at the start of an allocation sized for the LARGER geometry (stream_probe.backing_bytes)."""
    n, c = sp.TABLE_BATCH, sp.TABLE_CHANNELS
    backing = torch.zeros(sp.backing_bytes(), dtype=U8, device="cuda")
    view = backing[:n * side * side * c].view(n, side, side, c)
    view.copy_(_photo_batch(seed, n, side, side, c))
    return view


TABLE_ENTRIES = {
    "area": (sp.area_table_facts, U8, lambda n, c: (n, sp.TABLE_OUT, sp.TABLE_OUT, c),
             lambda ctx, x, y, s: _ok(ctx.lib.cv_resize_area_u8(ctx.unet._h, _p(x), x.shape[0], x.shape[1], x.shape[2], x.shape[3], _p(y),
                                                                sp.TABLE_OUT, sp.TABLE_OUT, s))),
    "antialias": (sp.antialias_table_facts, F32, lambda n, c: (n, c, sp.TABLE_OUT, sp.TABLE_OUT),
                  lambda ctx, x, y, s: _ok(ctx.lib.cv_resize_antialias_f32(ctx.unet._h, _p(x), x.shape[0], x.shape[1], x.shape[2], x.shape[3], _p(y),
                                                                           sp.TABLE_OUT, sp.TABLE_OUT, s))),
}


@pytest.mark.parametrize("first", sp.TABLE_PAIR, ids=lambda v: f"{v}-then-{sum(sp.TABLE_PAIR) - v}")
@pytest.mark.parametrize("kind", ["area", "antialias"])
def test_tables_rebuilt_on_one_stream_while_a_launch_of_the_other_geometry_waits_on_another(ctx, probe, kind, first):
    """Cases 1 and 2.  The engine caches the tables of the LAST geometry.  ``s1`` holds a launch of geometry ``first`` (tables cached)
    behind the delay; the host then resizes the other geometry on ``s2``, which rebuilds the tables.  The ``s1`` launch must still read
    its own tables when it finally runs -- with either geometry in the waiting role.

    What holds this today (MI355X, all four cases pass and the ``s2`` call returns only after the ``s1`` delay has run out): not the
    ``hipStreamSynchronize(st)`` at the top of ``ResizeTables::replace`` -- ``st`` is the NEW call's stream, idle here -- but the
    device-wide wait in ``block_release`` (engine.cpp) that ``DeviceBuffer::upload`` goes through before the block is refilled.  A
    change that removes that wait (a per-table event, a release under ``ReleaseAlreadySynced``) has to keep these cases green."""
    facts, dtype, out_shape, call = TABLE_ENTRIES[kind]
    sp.assert_table_swap_cannot_leave_the_buffers(facts)                    # before the first launch: wrong pixels at worst, never a fault
    second = sum(sp.TABLE_PAIR) - first
    n, c = sp.TABLE_BATCH, sp.TABLE_CHANNELS
    x = {side: _carved(side, 90 + side) for side in sp.TABLE_PAIR}
    want = {side: torch.empty(out_shape(n, c), dtype=dtype, device="cuda") for side in sp.TABLE_PAIR}
    got = {side: torch.empty(out_shape(n, c), dtype=dtype, device="cuda") for side in sp.TABLE_PAIR}
    for side in (second, first):                                            # default stream, one after the other
        call(ctx, x[side], want[side], 0)
    torch.cuda.synchronize()
    s1, s2 = probe.side, probe.s2
    call(ctx, x[first], got[first], s1.cuda_stream)                         # the tables of `first` are the cached ones, on s1
    s1.synchronize()
    for t in got.values():
        sp.fill_sentinel(t)
    torch.cuda.synchronize()
    after = _held(probe, s1)
    call(ctx, x[first], got[first], s1.cuda_stream)
    assert not after.query(), "the s1 call waited for its stream although its tables were cached: the case would test nothing"
    call(ctx, x[second], got[second], s2.cuda_stream)                       # rebuilds the tables while the s1 launch is queued
    print(f"{kind} {first}-then-{second}: the s2 call returned {'after' if after.query() else 'before'} the s1 delay ran out")
    s1.synchronize()
    s2.synchronize()
    for side, role in ((first, "waiting on s1 across the rebuild"), (second, "rebuilt and run on s2")):
        assert not (diff := _first_pixel(got[side], want[side])), f"{kind} {side}x{side} ({role}): {diff}"


def _encode(lib, eng, images: torch.Tensor, quality: int, stream_ptr: int):
    n, h, w = images.shape
    out = torch.empty(n * hb.jpeg_gray_max_bytes(h, w), dtype=U8, device="cuda")
    offsets, lengths = torch.empty(n + 1, dtype=I64, device="cuda"), torch.empty(n, dtype=I32, device="cuda")
    for t in (out, offsets, lengths):
        sp.fill_sentinel(t)
    return (out, offsets, lengths), lambda: _ok(lib.cv_jpeg_encode_gray_u8(eng._h, _p(images), n, h, w, quality, _p(out), out.numel(), _p(offsets),
                                                                           _p(lengths), stream_ptr))


@pytest.mark.parametrize("second_geometry", [(33, 40), (128, 128)], ids=["same-geometry", "scratch-grows"])
def test_two_encodes_share_the_scratch_in_device_order_whatever_their_streams(ctx, probe, second_geometry):
    """Case 3: "Two encodes on one engine are ordered on the device, whatever their streams" (the ``jpeg_enc_done`` event), and a larger
    second geometry re-allocates the scratch only once the first encode has left it.  Expected: the committed libjpeg files."""
    z = enc_cases.load()
    eng = hb.HipEngine(precision="f32")                                     # an engine whose scratch has never held 128 x 128
    try:
        jobs = []
        for (h, w), order in (((33, 40), 1), (second_geometry, -1)):
            kinds = enc_cases.group_kinds(enc_cases.GEOMETRIES.index((h, w)), enc_cases.QUALITIES.index(95))[::order]
            images = torch.from_numpy(np.stack([z[f"image/{h}x{w}/{k}"] for k in kinds])).cuda()
            jobs.append((images, [z[f"file/{h}x{w}/q95/{k}"].tobytes() for k in kinds]))
        torch.cuda.synchronize()
        s1, s2 = probe.side, probe.s2
        outs1, call1 = _encode(ctx.lib, eng, jobs[0][0], 95, s1.cuda_stream)
        outs2, call2 = _encode(ctx.lib, eng, jobs[1][0], 95, s2.cuda_stream)
        warm, call0 = _encode(ctx.lib, eng, jobs[0][0], 95, s1.cuda_stream)   # the scratch exists for the first geometry
        call0()
        torch.cuda.synchronize()
        after = _held(probe, s1)
        call1()
        assert not after.query(), "the s1 encode waited for its stream: the case would test nothing"
        call2()
        s1.synchronize()
        s2.synchronize()
        for outs, (_, files) in ((outs1, jobs[0]), (outs2, jobs[1])):
            assert _files([t.cpu() for t in outs])[2] == tuple(files)
    finally:
        eng.close()


def _forward_pair(ctx, probe, calls):
    """``calls`` = two (call(x, y, stream_ptr), x_true, out shape): default-stream results, then the first behind the delay on s1 and the
    second on s2 straight after it."""
    want, got = [], []
    for call, x, shape in calls:
        want.append(torch.empty(shape, dtype=F32, device="cuda"))
        got.append(torch.empty(shape, dtype=F32, device="cuda"))
        sp.fill_sentinel(got[-1])
        call(x, want[-1], 0)
    torch.cuda.synchronize()
    s1, s2 = probe.side, probe.s2
    after = _held(probe, s1)
    calls[0][0](calls[0][1], got[0], s1.cuda_stream)
    assert not after.query(), "the s1 forward waited for its stream: the case would test nothing"
    calls[1][0](calls[1][1], got[1], s2.cuda_stream)
    second_returned_early = not after.query()
    s2.synchronize()
    second_finished_early = not after.query()
    s1.synchronize()
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g.view(U8), w.view(U8)), f"forward {k + 1} of the pair: {_first_pixel(g, w)}"
    return second_returned_early, second_finished_early


def test_forwards_of_the_same_model_on_two_streams_never_overlap_on_the_workspace(ctx, probe):
    """Case 4: "Forwards of the SAME model may be enqueued on different streams ... the two never overlap on the shared workspace."  The
    second call may wait on the host; only the results are asserted."""
    xa, xb = (ll.unet_f32(_unet_u8(1, flag)).cuda() for flag in (True, False))
    unet = lambda x, y, s: _ok(ctx.lib.cv_unet_forward(ctx.unet._h, _p(x), 1, _p(y), s))
    _forward_pair(ctx, probe, [(unet, xa, (1, 1, 256, 256)), (unet, xb, (1, 1, 256, 256))])
    qa, qb = (ll.squares_f32(_squares(64, flag)).cuda() for flag in (True, False))
    resnet = lambda x, y, s: _ok(ctx.lib.cv_resnet18_forward(ctx.resnet._h, _p(x), 64, _p(y), s))
    _forward_pair(ctx, probe, [(resnet, qa, (64, 13)), (resnet, qb, (64, 13))])
    _ok(ctx.lib.cv_engine_numeric_status(ctx.unet._h, probe.s2.cuda_stream))
    _ok(ctx.lib.cv_engine_numeric_status(ctx.resnet._h, probe.s2.cuda_stream))


def test_unet_and_resnet_of_one_engine_on_two_streams(ctx, probe):
    """Case 5: "A UNet forward and a ResNet-18 forward of one engine may run on two streams at once (separate workspaces and scratch)."
    Both models in ONE engine; the UNet forward waits behind the delay on s1 while the ResNet forward runs on s2."""
    both = hb.HipEngine(precision="f16r", unet_chunk=2, resnet_chunk=128)
    try:
        both.load_unet(synth.make_unet(seed=1).state_dict())
        both.load_resnet18(synth.make_resnet(seed=2).state_dict())
        x, q = ll.unet_f32(_unet_u8(1, True)).cuda(), ll.squares_f32(_squares(64, True)).cuda()
        unet = lambda x_, y, s: _ok(ctx.lib.cv_unet_forward(both._h, _p(x_), 1, _p(y), s))
        resnet = lambda x_, y, s: _ok(ctx.lib.cv_resnet18_forward(both._h, _p(x_), 64, _p(y), s))
        returned_early, finished_early = _forward_pair(ctx, probe, [(unet, x, (1, 1, 256, 256)), (resnet, q, (64, 13))])
        print(f"two models, one engine: the ResNet call on s2 returned {'before' if returned_early else 'after'} and finished "
              f"{'before' if finished_early else 'after'} the delay in front of the UNet on s1 ran out")
        _ok(ctx.lib.cv_engine_numeric_status(both._h, probe.s2.cuda_stream))
        _ok(ctx.lib.cv_engine_numeric_status(both._h, probe.side.cuda_stream))
    finally:
        both.close()

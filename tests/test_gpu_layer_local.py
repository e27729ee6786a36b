"""GPU: every tapped layer of the networks against float64, one layer at a time, in the launch forms the networks really use.

tests/test_gpu_ops.py reaches the kernels through ``cv_op_*`` -- one stand-alone launch, channel offset 0, the launch form the planner
picks for that lone shape.  Here each case is ONE forward of a whole network; then for every tensor the engine exposes by module name
(``HipEngine.activation``) the device's own input tap(s) of that layer go through a float64 restatement of just that layer
(tests/layer_local.py) and the result is compared with the device's output tap at the op-level bar.  That covers the split-K forms at one
board, the position-major / packed-image forms of the small ResNet maps, the LDS-resident 1x1 GEMM (shortcuts, up3.up / up4.up), pools
fused into a producer's epilogue, pixel-shuffle and bilinear stores into the second half of a concatenated buffer, the fused ``inc`` pair,
the fused last-conv + OutConv, the chained layer1 of f16r, and the kernels without an op entry (both stems, inc0, the head).

Every exposed tap is either checked or in the stated absent set of its engine (layer_local.expected_absent); a tap missing outside that
set, or exposed inside it, fails the case.  The bars are layer_local.BARS (none is new); max-pools and aliases are bit-exact.
The cases at ``unet_chunk=2`` / ``resnet_chunk=128`` are followed by the small-batch forms of the DEFAULT chunk sizes
(``LAYER_LOCAL_AT_DEFAULT_CHUNK``, frozen from the census of tests/test_gpu_batch_sweep.py, whose tripwire keeps the list complete).
Each case appends its per-edge figures to the parity report of test_gpu_models.py (``_record``); profiles/layer_local_parity.md is made
from them.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import layer_local as ll
import resnet34_ref
from chessvision import synthetic
from oracle import synth
from test_gpu_models import _record as models_report

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CHAIN_FORM = 1 if os.environ.get("CV_CHAIN_WG", "")[:1] == "1" else 2           # as resnet.cpp: chain_form() reads it


def _record(payload):
    models_report("layer_local", payload)             # one more line in the parity report the whole-model tests write


def _check(tag, taps, inputs, sd, prec, images, absent, entry="float", only=None):
    """check_edges + one report line, written whether the case passes or not."""
    try:
        res = ll.check_edges(taps, inputs, sd, ll.BARS[prec], images, absent=absent, entry=entry, only=only)
    except AssertionError as exc:
        res = getattr(exc, "results", [])
        _record({**tag, "passed": False, "worst": ll.worst_edge(res) if res else None, "edges": res, "message": str(exc)[:4000]})
        raise
    _record({**tag, "passed": True, "worst": ll.worst_edge(res), "edges": res})
    for r in res:
        print(f"{tag} {r['edge']:40s} {r['kind']:8s} err {r['max_abs_err']:.3e} bar {r['bar']:.3e} ring {r['on_ring']}")
    return res


def _repeat_on_fixed_buffers(eng, entry, x_dev, n, out_dev, reps=3):
    """The same pointers every time: eager call, capture call, hipGraph replay (engine.cpp: run_graphed)."""
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(reps):
        assert getattr(eng._lib, entry)(eng._h, x_dev.data_ptr(), n, out_dev.data_ptr(), stream) == 0
    eng.check_numerics()


# ---- UNet ---------------------------------------------------------------------------------------------------------------------
UNET_ENGINES = [(prec, bilinear) for prec in ("f32", "f16x3", "f16") for bilinear in (False, True)]


@pytest.fixture(scope="module", params=UNET_ENGINES, ids=[f"{p}-{'bilinear' if b else 'convT'}" for p, b in UNET_ENGINES])
def unet_engine(request):
    from chessvision.hip_backend import HipEngine

    prec, bilinear = request.param
    net = synth.make_unet(seed=1, bilinear=bilinear)
    eng = HipEngine(precision=prec, unet_chunk=2)
    eng.load_unet(net.state_dict())
    yield eng, net.state_dict(), prec, bilinear
    try:
        eng.check_numerics()
    finally:
        eng.close()


def _unet_taps(eng, logits):
    return lambda name: logits if name == "logits" else eng.activation("unet", name)


@pytest.mark.parametrize("case", ["one_board_graph_replay", "three_boards_last_chunk", "u8_entry"])
def test_unet_every_tapped_layer_matches_float64(unet_engine, case):
    eng, sd, prec, bilinear = unet_engine
    tag = {"model": "unet", "variant": "bilinear" if bilinear else "convT", "prec": prec, "case": case}
    absent = ll.expected_absent(sd, prec)
    if case == "one_board_graph_replay":               # (a) the single-board forms, split-K; checked after the replay
        x = ll.unet_f32(ll.unet_images_u8(3, ["random"]))
        x_dev, out = x.cuda(), torch.empty((1, 1, 256, 256), device="cuda")
        _repeat_on_fixed_buffers(eng, "cv_unet_forward", x_dev, 1, out)
        inputs, logits, images = x, out.cpu().numpy(), [0]
    elif case == "three_boards_last_chunk":            # (b) chunks of 2 + 1: the taps hold the last chunk, the border-saturated image
        x = ll.unet_f32(ll.unet_images_u8(5, ["random", "photo", "border"]))
        out = eng.unet_forward(x).cpu().numpy()
        inputs, logits, images = x[2:3], out[2:3], [0]
    else:                                              # (c) the uint8 instantiations of the first-layer kernels; the board photo
        u8 = ll.unet_images_u8(7, ["random", "photo"])
        out, _ = eng.unet_forward_u8(torch.from_numpy(u8))
        eng.check_numerics()
        inputs, logits, images = ll.unet_f32(u8), out.cpu().numpy(), [1]
    _check(tag, _unet_taps(eng, logits), inputs, sd, prec, images, absent)
    eng.check_numerics()


# ---- ResNet -------------------------------------------------------------------------------------------------------------------
RESNET_ENGINES = [("resnet18", p) for p in ("f32", "f16x3", "f16", "f16r")] + [("resnet34", p) for p in ("f16x3", "f16r")]


def _resnet(arch):
    return synth.make_resnet(seed=2) if arch == "resnet18" else resnet34_ref.make_resnet34(synthetic.resnet34_state_dict(2))


def _resnet_engine(request, chunk):
    from chessvision.hip_backend import HipEngine

    arch, prec = request.param
    sd = _resnet(arch).state_dict()
    eng = HipEngine(precision=prec, resnet_chunk=chunk)
    eng.load_resnet({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}, arch)
    yield eng, sd, arch, prec
    try:
        eng.check_numerics()
    finally:
        eng.close()


@pytest.fixture(scope="module", params=RESNET_ENGINES, ids=[f"{a}-{p}" for a, p in RESNET_ENGINES])
def resnet_engine(request):
    yield from _resnet_engine(request, 128)


@pytest.fixture(scope="module", params=RESNET_ENGINES, ids=[f"{a}-{p}" for a, p in RESNET_ENGINES])
def resnet_engine_4096(request):
    yield from _resnet_engine(request, 4096)


def _resnet_taps(eng, arch, out, name_of_out):
    return lambda name: out if name == name_of_out else eng.activation(arch, name)


@pytest.mark.parametrize("case", ["ragged_tail_of_200", "one_board_64_graph_replay", "u8_entry"])
def test_resnet_every_tapped_layer_matches_float64(resnet_engine, case):
    eng, sd, arch, prec = resnet_engine
    tag = {"model": arch, "variant": "", "prec": prec, "case": case}
    entry = "u8" if case == "u8_entry" else "float"
    absent = ll.expected_absent(sd, prec, entry=entry, chain_form=CHAIN_FORM)
    if case == "ragged_tail_of_200":                   # (a) chunks of 128 + 72: the taps hold rows 128..199, all 72 checked
        x = ll.squares_f32(ll.squares_u8(11, 200, ll.specials_from(131)))
        out = eng.resnet18_forward(x).cpu().numpy()
        assert eng.activation(arch, "maxpool").shape[0] == 72
        inputs, result, images = x[128:], out[128:], range(72)
    elif case == "one_board_64_graph_replay":          # (b) the process_image shape: paired launches, split-K; checked after the replay
        x = ll.squares_f32(ll.squares_u8(12, 64, ll.specials_from(3)))
        x_dev, out = x.cuda(), torch.empty((64, 13), device="cuda")
        _repeat_on_fixed_buffers(eng, "cv_resnet18_forward", x_dev, 64, out)
        inputs, result, images = x, out.cpu().numpy(), range(64)
    else:                                              # (c) uint8 squares in, soft-max out
        u8 = ll.squares_u8(13, 80, ll.specials_from(40))
        out = eng.resnet18_forward_u8(torch.from_numpy(u8))
        eng.check_numerics()
        inputs, result, images = ll.squares_f32(u8), out.cpu().numpy(), range(80)
    _check(tag, _resnet_taps(eng, arch, result, "probs" if entry == "u8" else "logits"), inputs, sd, prec, images, absent, entry=entry)
    eng.check_numerics()


def test_resnet_stem_and_head_past_2048_squares_in_one_chunk(resnet_engine_4096):
    """(d) 2050 squares in one chunk: the persistent stem loop wraps past its 2048 workgroups.  Only the stem edge(s) and the head edge,
    on the first squares, the last of the first round and the wrapped ones."""
    eng, sd, arch, prec = resnet_engine_4096
    picks = [0, 1, 2047, 2048, 2049]
    x = ll.squares_f32(ll.squares_u8(14, 2050, {1: "frame", 2047: "full", 2048: "corner_br", 2049: "ramp_v"}))
    out = eng.resnet18_forward(x).cpu().numpy()
    assert eng.activation(arch, "layer4").shape[0] == 2050
    tag = {"model": arch, "variant": "", "prec": prec, "case": "2050_squares_one_chunk"}
    res = _check(tag, _resnet_taps(eng, arch, out, "logits"), x, sd, prec, picks, ll.expected_absent(sd, prec, chain_form=CHAIN_FORM),
                 only={"act1", "maxpool", "logits"})
    assert [r["edge"] for r in res] == (["act1"] if prec == "f32" else []) + ["maxpool", "logits"]
    eng.check_numerics()


# ---- the launch forms of the DEFAULT chunk sizes ------------------------------------------------------------------------------------
# The cases above run engines packed for chunks of 2 images / 128 (4096) squares.  The production engines pack for 64 / 16384: wide
# layers carry 256-row weights and fall back per launch, so a small batch takes other forms there.  This list is frozen from the census of
# tests/test_gpu_batch_sweep.py: per (model, precision, variant) N = 1 / n = 64 and the smallest member of every other census class that
# begins at a size small enough to download every tap (UNet N <= 4, ResNet n <= 256).  The sweep's tripwire fails when the planner grows
# a small-batch form that is not here.
LAYER_LOCAL_AT_DEFAULT_CHUNK = tuple(
    # every N up to 8 is a launch form of its own (split-K factors, 8 x 16 / 16 x 16 patches, the transposed convs' tiles)
    [("unet", prec, variant, n) for prec, variant in (("f32", "convT"), ("f32", "bilinear"), ("f16x3", "convT"), ("f16x3", "bilinear"),
                                                      ("f16", "convT")) for n in (1, 2, 3, 4)]
    # 64 = one board; 63 shares its class under f16r only; every other swept size up to 256 begins a class
    + [("resnet18", prec, "", n) for prec in ("f32", "f16x3", "f16", "f16r") for n in (1, 7, 63, 64, 100, 128, 192, 256)]
    + [("resnet34", "f16x3", "", n) for n in (1, 7, 63, 64, 65, 100, 256)]
    + [("resnet34", "f16r", "", n) for n in (1, 7, 63, 64, 100, 256)])


class _OneEngineAtATime:
    """The default-chunk engine of (model, precision, variant), built on first use and closed when another is asked for."""

    def __init__(self):
        self.key, self.eng, self.sd = None, None, None

    def get(self, model, prec, variant):
        from chessvision.hip_backend import HipEngine

        if self.key != (model, prec, variant):
            self.close()
            for var in ("CHESSVISION_HIP_UNET_CHUNK", "CHESSVISION_HIP_RESNET_CHUNK"):
                assert var not in os.environ, f"{var} is set: this case is about the library's own chunk sizes"
            eng = HipEngine(precision=prec)
            if model == "unet":
                sd = synth.make_unet(seed=1, bilinear=variant == "bilinear").state_dict()
                eng.load_unet(sd)
            else:
                sd = _resnet(model).state_dict()
                eng.load_resnet({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}, model)
            self.key, self.eng, self.sd = (model, prec, variant), eng, sd
        return self.eng, self.sd

    def close(self):
        if self.eng is not None:
            eng, self.eng, self.key = self.eng, None, None
            try:
                eng.check_numerics()
            finally:
                eng.close()


@pytest.fixture(scope="module")
def default_chunk_engines():
    holder = _OneEngineAtATime()
    yield holder
    holder.close()


@pytest.mark.parametrize("model, prec, variant, n", LAYER_LOCAL_AT_DEFAULT_CHUNK,
                         ids=[f"{m}-{p}{'-' + v if v else ''}-{n}" for m, p, v, n in LAYER_LOCAL_AT_DEFAULT_CHUNK])
def test_default_chunk_small_batch_forms_every_tapped_layer_matches_float64(default_chunk_engines, monkeypatch, model, prec, variant, n):
    """One forward of ``n`` at the default chunk size, three times on fixed buffers (every listed size is one the engine replays as a
    hipGraph); then every tap as in the cases above: the last image of the batch, or its last 72 squares."""
    monkeypatch.delenv("CHESSVISION_HIP_UNET_CHUNK", raising=False)
    monkeypatch.delenv("CHESSVISION_HIP_RESNET_CHUNK", raising=False)
    eng, sd = default_chunk_engines.get(model, prec, variant)
    tag = {"model": model, "variant": variant, "prec": prec, "case": f"default_chunk_{n}"}
    if model == "unet":
        x = ll.unet_f32(ll.unet_images_u8(20 + n, ["photo", "border", "photo", "random"][4 - n:]))       # the checked (last) image: random bytes
        x_dev, out = x.cuda(), torch.empty((n, 1, 256, 256), device="cuda")
        _repeat_on_fixed_buffers(eng, "cv_unet_forward", x_dev, n, out)
        assert eng.activation("unet", "inc").shape[0] == n
        _check(tag, _unet_taps(eng, out.cpu().numpy()), x, sd, prec, [n - 1], ll.expected_absent(sd, prec))
    else:
        first = max(0, n - 72)
        specials = {i: kind for i, kind in ll.specials_from(max(0, n - 40)).items() if i < n}
        x = ll.squares_f32(ll.squares_u8(30 + n, n, specials))
        x_dev, out = x.cuda(), torch.empty((n, 13), device="cuda")
        _repeat_on_fixed_buffers(eng, "cv_resnet18_forward", x_dev, n, out)
        assert eng.activation(model, "maxpool").shape[0] == n
        _check(tag, _resnet_taps(eng, model, out.cpu().numpy(), "logits"), x, sd, prec, range(first, n),
               ll.expected_absent(sd, prec, chain_form=CHAIN_FORM))
    eng.check_numerics()


# ---- the stand-alone OutConv: CV_FUSE_HEAD is read once per process ---------------------------------------------------------------
_UNFUSED_HEAD_SCRIPT = r"""
import json, sys
sys.path.insert(0, r"{root}"); sys.path.insert(0, r"{root}/chessvision-3lc_amd"); sys.path.insert(0, r"{root}/tests")
import layer_local as ll
from oracle import synth
from chessvision.hip_backend import HipEngine
net = synth.make_unet(seed=1)
sd = net.state_dict()
x = ll.unet_f32(ll.unet_images_u8(5, ["random", "photo", "border"]))
code = 0
for prec in ("f16x3", "f32"):
    eng = HipEngine(precision=prec, unet_chunk=2)
    eng.load_unet(sd)
    out = eng.unet_forward(x).cpu().numpy()
    taps = lambda name: out[2:3] if name == "logits" else eng.activation("unet", name)
    try:
        res, msg = ll.check_edges(taps, x[2:3], sd, ll.BARS[prec], [0], absent=ll.expected_absent(sd, prec, fused_head=False)), ""
    except AssertionError as exc:
        res, msg, code = getattr(exc, "results", []), str(exc), 1
    eng.check_numerics()
    eng.close()
    print("LAYER_LOCAL " + json.dumps({{"prec": prec, "edges": res, "message": msg}}))
sys.exit(code)
"""


def test_unfused_head_up4_output_and_standalone_outconv_each_get_their_edge(tmp_path):
    script = tmp_path / "unfused_head.py"
    script.write_text(_UNFUSED_HEAD_SCRIPT.format(root=str(ROOT)))
    run = subprocess.run([sys.executable, str(script)], env=dict(os.environ, CV_FUSE_HEAD="0"), capture_output=True, text=True, timeout=600)
    rows = [json.loads(ln[len("LAYER_LOCAL "):]) for ln in run.stdout.splitlines() if ln.startswith("LAYER_LOCAL ")]
    for row in rows:
        _record({"model": "unet", "variant": "convT, CV_FUSE_HEAD=0", "prec": row["prec"], "case": "three_boards_last_chunk",
                 "passed": not row["message"], "worst": ll.worst_edge(row["edges"]) if row["edges"] else None, "edges": row["edges"],
                 "message": row["message"][:4000]})
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert [row["prec"] for row in rows] == ["f16x3", "f32"]
    for row in rows:
        edges = {r["edge"]: r for r in row["edges"]}
        assert edges["up4.conv.double_conv.5"]["kind"] == "conv" and edges["up4.conv.double_conv.5"]["spans"] == []
        assert edges["logits"]["kind"] == "outconv" and edges["logits"]["spans"] == [] and edges["logits"]["ok"]
        assert edges["up4"]["kind"] == "alias"
        assert len(edges) == (37 if row["prec"] == "f32" else 35)     # f32: + the packed input copy and inc.double_conv.2

"""GPU: every tapped layer of YOLOv8-cls, all five scales (n / s / m / l / x), against float64, one layer at a time.

tests/test_gpu_yolov8_cls.py holds the n and m models at the logits and at five taps against a float32 helper fed its own upstream
values; tests/test_gpu_ops_silu.py reaches the SiLU epilogue through lone launches at channel offset 0 of n's and m's slice widths.  Here
each case is ONE forward of the whole network; then every tensor ``Engine::YoloCls::build_taps`` exposes is checked from the device's own
stored input(s) to the device's own stored output through the float64 edge table of tests/layer_local.py (``yolo_cls_ops``): 27 edges
for n and s, 39 for m, 51 for l and x.  That sees a wrong slice offset in a plan, a wrong shortcut source, the fused-checkpoint loader,
the stem at 32 / 64 / 80 channels, x's 80-channel slices (a 64-row slab and a quarter) and whatever launch form the planner picks for
the real layers at the batch size of the case.

  * small chunk: ``resnet_chunk=128``, 300 squares = 128 + 128 + 44, the nine special squares inside the last chunk, all 44 rows of every
    edge, for 5 scales x (f32, f16x3, f16); on f16x3 also the u8 entry and the fused checkpoint (s, x) and n = 1 / n = 64 after a hipGraph
    replay on fixed buffers (m, x);
  * the default chunk: the census of ``HipEngine.profile`` over ``CENSUS_SIZES`` groups the batch sizes by identical (layer, kernel)
    lists; the smallest member of every class is frozen in ``YOLO_AT_DEFAULT_CHUNK`` and gets the layer-local check (three forwards on
    fixed buffers, then the last min(n, 72) rows and rows 0, 63, 64).  The census case is the tripwire: it fails when the planner grows
    a form whose smallest size is not listed, when a YOLO convolution leaves the implicit-GEMM family (SiLU exists nowhere else), and
    when an f16x3 scale no longer reaches a split-K form, a position-major form or a tile family of profiles/yolov8_cls.md (the
    families of that profile belong to 16384 squares, so for n and m the census profiles that size too; it is too large to tap).

Bars: layer_local.BARS, unchanged.  The cases are ordered so that consecutive ones share an engine; one engine exists at a time (x's
weights are large).  Figures join the parity report through test_gpu_layer_local._record; profiles/yolov8_cls_parity.md is made from it.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "chessvision-3lc_amd"), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import batch_sweep as bs  # noqa: E402
import layer_local as ll  # noqa: E402
import yolov8_cls_ref  # noqa: E402
from chessvision import synthetic  # noqa: E402
from test_gpu_layer_local import _check, _repeat_on_fixed_buffers  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = ("n", "s", "m", "l", "x")
PRECS = ("f32", "f16x3", "f16")
EDGES = {"n": 27, "s": 27, "m": 39, "l": 51, "x": 51}


def _arch(scale):
    return f"yolov8{scale}-cls"


class _States:
    """scale -> state dict (as trained / fused), one scale at a time: x's dict is 225 MB."""

    def __init__(self):
        self.key, self.sd = None, None

    def get(self, scale, fused=False):
        if self.key != (scale, fused):
            self.key, self.sd = None, None
            sd = synthetic.yolov8_cls_state_dict(2, _arch(scale))
            self.sd = yolov8_cls_ref.fuse_state(sd) if fused else sd
            self.key = (scale, fused)
        return self.sd


class _OneEngineAtATime:
    """The engine of (scale, precision, chunk, fused), built on first use and closed when another is asked for."""

    def __init__(self):
        self.key, self.eng, self.states = None, None, _States()

    def get(self, scale, prec, chunk=None, fused=False):
        from chessvision.hip_backend import HipEngine

        sd = self.states.get(scale, fused)
        if self.key != (scale, prec, chunk, fused):
            self.close()
            if chunk is None:
                assert "CHESSVISION_HIP_RESNET_CHUNK" not in os.environ, "this case is about the library's own chunk size"
                eng = HipEngine(precision=prec)
            else:
                eng = HipEngine(precision=prec, resnet_chunk=chunk)
            try:
                eng.load_yolo_cls(sd, _arch(scale))
            except BaseException:
                eng.close()
                raise
            self.key, self.eng = (scale, prec, chunk, fused), eng
        return self.eng, sd

    def close(self):
        if self.eng is not None:
            eng, self.eng, self.key = self.eng, None, None
            try:
                eng.check_numerics()
            finally:
                eng.close()


@pytest.fixture(scope="module")
def engines():
    holder = _OneEngineAtATime()
    yield holder
    holder.close()


def _taps(eng, arch, out, name_of_out):
    return lambda name: out if name == name_of_out else eng.activation(arch, name)


# ---- a. b. c.: resnet_chunk = 128 -------------------------------------------------------------------------------------------------------
def _small_chunk_cases():
    cases = []
    for scale in SCALES:
        for prec in PRECS:
            cases.append((scale, prec, "ragged_tail_of_300"))
            if prec == "f16x3" and scale in ("s", "x"):
                cases.append((scale, prec, "u8_entry"))
            if prec == "f16x3" and scale in ("m", "x"):
                cases += [(scale, prec, "graph_replay_1"), (scale, prec, "graph_replay_64")]
            if prec == "f16x3" and scale in ("s", "x"):
                cases.append((scale, prec, "fused_checkpoint"))
    return cases


SMALL_CHUNK_CASES = _small_chunk_cases()


@pytest.mark.parametrize("scale, prec, case", SMALL_CHUNK_CASES, ids=[f"{s}-{p}-{c}" for s, p, c in SMALL_CHUNK_CASES])
def test_small_chunk_every_tapped_layer_matches_float64(engines, scale, prec, case):
    arch = _arch(scale)
    eng, sd = engines.get(scale, prec, chunk=128, fused=case == "fused_checkpoint")
    assert eng.classifier_arch == arch and ("model.0.conv.bias" in sd) == (case == "fused_checkpoint")
    tag = {"model": arch, "variant": "fused checkpoint" if case == "fused_checkpoint" else "", "prec": prec, "case": case}
    entry = "u8" if case == "u8_entry" else "float"
    if case.startswith("graph_replay_"):               # c. fixed buffers: eager, capture, hipGraph replay; the taps after the replay
        n = int(case.rsplit("_", 1)[1])
        x = ll.squares_f32(ll.squares_u8(42 + n, n, {i: k for i, k in ll.specials_from(3).items() if i < n}))
        x_dev, out = x.cuda(), torch.empty((n, 13), device="cuda")
        _repeat_on_fixed_buffers(eng, "cv_resnet18_forward", x_dev, n, out)
        inputs, result, images = x, out.cpu().numpy(), range(n)
    else:                                              # a. b. chunks of 128 + 128 + 44: the taps hold rows 256..299, all 44 checked
        u8 = ll.squares_u8(41, 300, ll.specials_from(270))
        if entry == "u8":
            out = eng.resnet18_forward_u8(torch.from_numpy(u8))
            eng.check_numerics()
        else:
            out = eng.resnet18_forward(ll.squares_f32(u8))
        inputs, result, images = ll.squares_f32(u8)[256:], out.cpu().numpy()[256:], range(44)
    assert eng.activation(arch, "model.0").shape[0] == len(images)
    res = _check(tag, _taps(eng, arch, result, "probs" if entry == "u8" else "logits"), inputs, sd, prec, images,
                 ll.expected_absent(sd, prec, entry=entry), entry=entry)
    assert len(res) == EDGES[scale]                    # the u8 entry: no logits edge, the probs edge spans the head
    if entry == "u8":
        assert res[-1]["edge"] == "probs" and res[-1]["kind"] == "softmax" and res[-1]["spans"] == ["logits"] and res[-1]["bar"] == 1e-6
    eng.check_numerics()


# ---- d. the launch forms of the default chunk -------------------------------------------------------------------------------------------------
CENSUS_SIZES = (1, 2, 3, 4, 7, 8, 16, 32, 63, 64, 65, 100, 128, 129, 192, 256)
# Frozen from the census: per (scale, precision) the smallest member of every class of CENSUS_SIZES (profiles/yolov8_cls_parity.md has
# the classes; 63-65 is one class everywhere, 128-129 everywhere but l).  The census case below fails when the planner grows a form that
# is not here.
_SMALL_NETS = (1, 16, 32, 63, 100, 128, 192)
_S = (1, 4, 7, 16, 32, 63, 100, 128, 192, 256)
_M = (1, 2, 3, 4, 7, 16, 32, 63, 100, 128, 192, 256)
_L = (1, 2, 3, 4, 7, 8, 16, 32, 63, 100, 128, 129, 192, 256)
_X = (1, 2, 3, 4, 7, 8, 16, 32, 63, 100, 128, 192, 256)
YOLO_AT_DEFAULT_CHUNK = {
    ("n", "f32"): _SMALL_NETS, ("n", "f16x3"): _SMALL_NETS, ("n", "f16"): (1, 128),
    ("s", "f32"): _S, ("s", "f16x3"): _S, ("s", "f16"): (1, 7, 16, 32, 63, 100, 128, 192),
    ("m", "f32"): _M, ("m", "f16x3"): _M, ("m", "f16"): (1, 3, 4, 7, 8, 16, 32, 63, 100, 128, 192, 256),
    ("l", "f32"): _L, ("l", "f16x3"): _L, ("l", "f16"): (1, 2, 3, 4, 7, 16, 32, 63, 100, 128, 129, 192, 256),
    ("x", "f32"): _X, ("x", "f16x3"): _X, ("x", "f16"): _X,
}
# The tile families of the generic kernel that profiles/yolov8_cls.md lists per scale (its per-launch tables: n and m, at 16384 squares).
# Up to 256 squares the planner stays on 64x128 / 128x128 / 64x256 tiles, so for these two the census also profiles one forward of
# FAMILY_SIZE squares -- too many to download every tap of; that size is held row by row by tests/test_gpu_yolov8_batch_sweep.py.
TILE_FAMILIES = {"n": ("64x128", "64x256", "128x256", "256x256"), "m": ("64x128", "64x256", "128x256", "256x256")}
FAMILY_SIZE = 16384


def _default_chunk_cases():
    cases = []
    for scale in SCALES:
        for prec in PRECS:
            cases.append((scale, prec, "census"))
            cases += [(scale, prec, n) for n in YOLO_AT_DEFAULT_CHUNK[scale, prec]]
    return cases


DEFAULT_CHUNK_CASES = _default_chunk_cases()


def census_problems(scale, prec, cen, listed):
    """What the census of one (scale, precision) must show; every problem names its layer or its class."""
    problems = []
    depth = sum(yolov8_cls_ref.depths(scale))
    for n, sig in cen.items():
        convs = [(name, kern) for name, kern in sig if name.startswith("model.") and name.endswith(".conv")]
        if len(convs) != 13 + 2 * depth or len(sig) != len(convs) + 2:
            problems.append(f"n = {n}: {len(convs)} convolution entries of {len(sig)}, expected {13 + 2 * depth} of {15 + 2 * depth}")
        for name, kern in convs:
            if not kern.startswith("conv_igemm_kernel<"):
                problems.append(f"n = {n}: {name} ran '{kern}': SiLU exists in the implicit-GEMM kernel only")
    cls = bs.classes(cen)
    for smallest in bs.tripwire(cls, listed, max(CENSUS_SIZES)):
        k = next(i for i, c in enumerate(cls) if c["smallest"] == smallest)
        diff = bs.signature_diff(cls[k]["signature"], cls[k - 1]["signature"]) if k else []
        problems.append(f"({scale!r}, {prec!r}): n = {smallest} begins a launch form of its own (n in {{{bs.ranges(cls[k]['members'], cen)}}}) "
                        "without a layer-local case -- add it to YOLO_AT_DEFAULT_CHUNK:"
                        + "".join(f"\n      {layer}: {ka}   (class before: {kb})" for layer, ka, kb in diff))
    if prec == "f16x3":
        kernels = {(name, kern) for sig in cen.values() for name, kern in sig}
        for mark, what in ((",splitK", "split-K"), (",POS", "position-major (POS)")) + tuple(
                (f",{fam},", f"{fam} tile") for fam in TILE_FAMILIES.get(scale, ())):
            if not any(mark in kern for _, kern in kernels):
                problems.append(f"({scale!r}, f16x3): no layer runs a {what} form at any n of {sorted(cen)}: a planner threshold moved "
                                "and took this form's layer-local case away")
    return cls, problems


@pytest.mark.parametrize("scale, prec, n", DEFAULT_CHUNK_CASES, ids=[f"{s}-{p}-{n}" for s, p, n in DEFAULT_CHUNK_CASES])
def test_default_chunk_forms_every_tapped_layer_matches_float64(engines, monkeypatch, scale, prec, n):
    """``census``: the tripwire.  A size: three forwards of ``n`` on fixed buffers at the library's own chunk size (every listed size is one
    the engine replays as a hipGraph), then every tap on the last min(n, 72) rows and rows 0, 63 and 64."""
    monkeypatch.delenv("CHESSVISION_HIP_RESNET_CHUNK", raising=False)
    arch = _arch(scale)
    eng, sd = engines.get(scale, prec)
    if n == "census":
        sizes = CENSUS_SIZES + ((FAMILY_SIZE,) if prec == "f16x3" and scale in TILE_FAMILIES else ())
        x = ll.squares_f32(ll.squares_u8(29, max(CENSUS_SIZES), {}))
        if len(sizes) > len(CENSUS_SIZES):
            x = x.repeat(FAMILY_SIZE // x.shape[0], 1, 1, 1)
        cen = bs.census(eng, arch, sizes, x)
        eng.check_numerics()
        cls, problems = census_problems(scale, prec, cen, YOLO_AT_DEFAULT_CHUNK[scale, prec])
        for c in cls:
            print(f"census {arch} {prec}: class n in {{{bs.ranges(c['members'], sizes)}}}")
        assert not problems, f"{len(problems)} census problem(s):\n  " + "\n  ".join(problems)
        return
    tag = {"model": arch, "variant": "", "prec": prec, "case": f"default_chunk_{n}"}
    images = sorted(set(range(max(0, n - 72), n)) | {r for r in (0, 63, 64) if r < n})
    specials = {i: kind for i, kind in ll.specials_from(max(0, n - 40)).items() if i < n}
    x = ll.squares_f32(ll.squares_u8(30 + n, n, specials))
    x_dev, out = x.cuda(), torch.empty((n, 13), device="cuda")
    _repeat_on_fixed_buffers(eng, "cv_resnet18_forward", x_dev, n, out)
    assert eng.activation(arch, "model.0").shape[0] == n
    res = _check(tag, _taps(eng, arch, out.cpu().numpy(), "logits"), x, sd, prec, images, ll.expected_absent(sd, prec))
    assert len(res) == EDGES[scale]
    eng.check_numerics()

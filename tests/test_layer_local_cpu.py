"""The layer-local harness (tests/layer_local.py) on the CPU: taps from forward hooks of the float32 torch oracle networks.

  * every edge of both UNet variants, ResNet-18 and ResNet-34 is inside the f32 bars on the inputs the GPU tests use -- the float64
    reference and the float32 oracle agree layer by layer, so a GPU failure at these bars is the kernel's;
  * four planted defects (as forward hooks, so that everything downstream consumes the defective tensor, the way a defective kernel's
    consumers would): the harness names exactly the planted edge and no other;
  * a tap missing outside the stated absent set fails the run;
  * YOLOv8-cls, all five scales, in both checkpoint forms: every edge of the float32 helper (tests/yolov8_cls_ref.py) uses at most 0.05
    of its f32 bar, five planted defects of the kinds a C2f plan can have are each named alone, and a dropped tap is named.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_local as ll
import resnet34_ref
import yolov8_cls_ref
from chessvision import synthetic
from oracle import synth

BARS = ll.BARS["f32"]
UNET_ABSENT = frozenset({"input"})                  # the packed 8-channel input copy is a tensor of the f32 engine, not a module


def hooked_forward(net, x, names, plant=None, plant_full=None):
    """name -> float32 output of every module in ``names`` (+ "logits"); ``plant`` = {module name: fn(output) -> replacement output},
    ``plant_full`` = {module name: fn(module, inputs, output) -> replacement output, or None to leave it}."""
    got, hs = {}, []
    mods = dict(net.named_modules())
    for n, fn in (plant or {}).items():
        hs.append(mods[n].register_forward_hook(lambda m, i, o, fn=fn: fn(o)))
    for n, fn in (plant_full or {}).items():
        hs.append(mods[n].register_forward_hook(fn))
    for n in names:
        if n in mods:
            hs.append(mods[n].register_forward_hook(lambda m, i, o, n=n: got.__setitem__(n, o.detach().clone())))
    try:
        with torch.no_grad():
            got["logits"] = net(x)
    finally:
        for h in hs:
            h.remove()
    return got


def run(net, x, images, plant=None, absent=frozenset(), ops=None, drop=(), plant_full=None, sd=None):
    sd = net.state_dict() if sd is None else sd
    ops = ll.ops_for(sd) if ops is None else ops
    got = hooked_forward(net, x, [op.out for op in ops] + [i for op in ops for i in op.ins], plant, plant_full)
    for name in drop:
        got.pop(name)
    return ll.check_edges(got.__getitem__, x, sd, BARS, images, absent=absent, ops=ops)


def squares():
    return ll.squares_f32(ll.squares_u8(4, 12, ll.specials_from(2)))         # 0, 1, 11 random; 2..10 the nine special squares


@pytest.fixture(scope="module")
def unets():
    return {bilinear: synth.make_unet(seed=1, bilinear=bilinear) for bilinear in (False, True)}


@pytest.mark.parametrize("bilinear", [False, True], ids=["convT", "bilinear"])
def test_unet_reference_alone_is_inside_the_f32_bars(unets, bilinear):
    x = ll.unet_f32(ll.unet_images_u8(3, ["random", "photo", "border"]))
    res = run(unets[bilinear], x, [0, 1, 2], absent=UNET_ABSENT)
    names = {r["edge"] for r in res}
    assert len(res) == 36 and {"logits", "up3.up", "down4.maxpool_conv.0", "up4.conv.double_conv.5", "inc"} <= names
    assert all(r["max_abs_err"] == 0.0 for r in res if r["kind"] in ll.EXACT)
    assert {r["kind"] for r in res if r["edge"].endswith(".up")} == ({"bilinear"} if bilinear else {"conv"})


@pytest.mark.parametrize("arch", ["resnet18", "resnet34"])
def test_resnet_reference_alone_is_inside_the_f32_bars(arch):
    net = synth.make_resnet(seed=2) if arch == "resnet18" else resnet34_ref.make_resnet34(synthetic.resnet34_state_dict(2))
    x = squares()
    res = run(net, x, range(12))
    blocks = 8 if arch == "resnet18" else 16
    assert len(res) == 2 + 2 * blocks + 3 + 4 + 1                             # stem, pool, act1 + block, shortcuts, aliases, logits
    assert [r["edge"] for r in res if r["kind"] == "head"] == ["logits"]
    # the u8 classifier entry: no logits, the soft-max edge spans the head and keeps its absolute bar
    sd = net.state_dict()
    ops = ll.resnet_ops(sd, entry="u8")
    got = hooked_forward(net, x, [op.out for op in ops])
    got["probs"] = torch.softmax(got.pop("logits"), 1)
    res = ll.check_edges(got.__getitem__, x, sd, BARS, range(12), absent=ll.expected_absent(sd, "f32", entry="u8"), entry="u8")
    last = res[-1]
    assert last["edge"] == "probs" and last["kind"] == "softmax" and last["spans"] == ["logits"] and last["bar"] == 1e-6


def _only_failing(excinfo):
    return ll.failing_edges(excinfo.value), str(excinfo.value)


def test_planted_corner_pixel_two_bars_off_is_named(unets):
    edge = "down2.maxpool_conv.1.double_conv.2"
    x = ll.unet_f32(ll.unet_images_u8(3, ["random"]))
    clean = {r["edge"]: r for r in run(unets[False], x, [0], absent=UNET_ABSENT)}

    def plant(o):
        o = o.clone()
        o[0, 37, 0, 63] += 2.0 * clean[edge]["bar"]                          # top-right corner pixel of channel 37
        return o

    with pytest.raises(AssertionError) as ei:
        run(unets[False], x, [0], plant={edge: plant}, absent=UNET_ABSENT)
    failing, text = _only_failing(ei)
    assert failing == [edge], text
    bad = next(r for r in ei.value.results if r["edge"] == edge)
    assert bad["worst"] == [0, 37, 0, 63] and bad["on_ring"]


def test_planted_swap_of_two_channel_groups_is_named(unets):
    x = ll.unet_f32(ll.unet_images_u8(3, ["random"]))

    def plant(o):
        o = o.clone()
        o[:, 16:24], o[:, 24:32] = o[:, 24:32].clone(), o[:, 16:24].clone()
        return o

    with pytest.raises(AssertionError) as ei:
        run(unets[False], x, [0], plant={"up3.up": plant}, absent=UNET_ABSENT)
    failing, text = _only_failing(ei)
    assert failing == ["up3.up"], text


class _ZeroPaddedPool(torch.nn.Module):
    def forward(self, x):
        return F.max_pool2d(F.pad(x, (1, 1, 1, 1), value=0.0), 3, stride=2)


def test_planted_zero_padding_in_the_3x3_pool_is_named_on_an_all_negative_map():
    net = synth.make_resnet(seed=2)
    net.maxpool = _ZeroPaddedPool()
    sd = net.state_dict()
    ops = [op for op in ll.resnet_ops(sd) if op.out != "act1"]                # act1 is a source here: the map below is no ReLU output
    with pytest.raises(AssertionError) as ei:
        run(net, squares(), range(12), plant={"act1": lambda o: -o - 0.125}, ops=ops)
    failing, text = _only_failing(ei)
    assert failing == ["maxpool"], text
    bad = next(r for r in ei.value.results if r["edge"] == "maxpool")
    assert bad["on_ring"] and bad["bar"] == 0.0
    # the same map through the correct pool passes: it is the padding that is caught, not the negative values
    run(synth.make_resnet(seed=2), squares(), range(12), plant={"act1": lambda o: -o - 0.125}, ops=ops)


def test_planted_logit_column_shifted_by_one_class_is_named():
    net = synth.make_resnet(seed=2)

    def plant(o):
        o = o.clone()
        o[:, 7] = o[:, 6]                                                    # class 6's logit also lands in column 7
        return o

    with pytest.raises(AssertionError) as ei:
        run(net, squares(), range(12), plant={"fc": plant})
    failing, text = _only_failing(ei)
    assert failing == ["logits"], text
    assert next(r for r in ei.value.results if r["edge"] == "logits")["worst"][1] == 7


def test_an_unexpected_missing_tap_fails_the_run():
    net = synth.make_resnet(seed=2)
    with pytest.raises(AssertionError, match="tap 'layer3.0.act1' is missing and not in the stated absent set"):
        run(net, squares(), [0, 2], drop=["layer3.0.act1"])
    # ... a tap stated absent that the engine exposes fails it as well (it would go unchecked) ...
    with pytest.raises(AssertionError, match="tap 'layer1.0.act1' is stated absent but the engine exposes it"):
        run(net, squares(), [0, 2], absent=frozenset({"layer1.0.act1"}))
    # ... and a stated-absent tap that really is absent shortens nothing: its consumer spans it from the nearest upstream tap
    res = run(net, squares(), [0, 2], drop=["layer1.0.act1"], absent=frozenset({"layer1.0.act1"}))
    assert next(r for r in res if r["edge"] == "layer1.0")["spans"] == ["layer1.0.act1"]
    assert "layer1.0.act1" not in {r["edge"] for r in res}


def test_the_stated_absent_sets():
    u, r18 = synth.make_unet(1).state_dict(), synth.make_resnet(2).state_dict()
    r34 = synthetic.resnet34_state_dict(2)
    assert ll.expected_absent(u, "f32") == {"up4.conv.double_conv.5", "up4"}
    assert ll.expected_absent(u, "f16") == {"input", "up4.conv.double_conv.5", "up4"}
    assert ll.expected_absent(u, "f16x3", fused_head=False) == {"input", "inc.double_conv.2"}
    assert ll.expected_absent(r18, "f32") == frozenset() and ll.expected_absent(r18, "f16x3") == {"act1"}
    assert ll.expected_absent(r18, "f16r") == {"act1", "layer1.0.act1", "layer1.1.act1"}
    assert ll.expected_absent(r18, "f16r", chain_form=1) == {"act1", "layer1.0.act1", "layer1.1.act1", "layer1.0"}
    assert ll.expected_absent(r34, "f16r") == {"act1", "layer1.0.act1", "layer1.1.act1", "layer1.2.act1"}
    assert ll.resnet_depths(r18) == (2, 2, 2, 2) and ll.resnet_depths(r34) == (3, 4, 6, 3)
    assert np.array_equal(ll.special_square("corner_br")[-1, -1:], [255]) and ll.special_square("corner_br").sum() == 255


# ---- YOLOv8-cls: all five scales, both checkpoint forms ---------------------------------------------------------------------------------
YOLO_SCALES = ("n", "s", "m", "l", "x")
YOLO_EDGES = {"n": 27, "s": 27, "m": 39, "l": 51, "x": 51}              # 15 + 2 x (Bottlenecks of the four C2f)
REFERENCE_CEILING = 0.05         # of the f32 bar; the float32 helper against float64 of each layer measured 0.0060 (n), 0.0085 (s), 0.0059 (m),
                                 # 0.0060 (l), 0.0062 (x): a reference that drifts fails here before it loosens a GPU test


@pytest.fixture(scope="module")
def yolos():
    """scale -> (state dict as trained, the float32 helper on it); built on first use, never modified"""
    made = {}

    def get(scale):
        if scale not in made:
            sd = synthetic.yolov8_cls_state_dict(2, scale)
            made[scale] = (sd, yolov8_cls_ref.make(scale, sd))
        return made[scale]
    return get


def _inside_the_ceiling(res, what):
    over = [(r["edge"], r["max_abs_err"] / r["bar"]) for r in res if r["max_abs_err"] > REFERENCE_CEILING * r["bar"]]
    worst = max(res, key=lambda r: r["max_abs_err"] / r["bar"])
    print(f"{what}: worst edge {worst['edge']} at {worst['max_abs_err'] / worst['bar']:.4f} of its bar")
    assert not over, f"{what}: edges over {REFERENCE_CEILING} of the f32 bar: {over}"


@pytest.mark.parametrize("scale", YOLO_SCALES)
def test_yolo_reference_alone_is_inside_the_f32_bars_in_both_checkpoint_forms(yolos, scale):
    sd, net = yolos(scale)
    x = squares()
    res = run(net, x, range(12), sd=sd)
    assert len(res) == YOLO_EDGES[scale] == 15 + 2 * sum(ll.yolo_cls_depths(sd)) and ll.yolo_cls_scale(sd) == scale
    assert [r["edge"] for r in res if r["kind"] == "head"] == ["logits"] and {r["kind"] for r in res} == {"conv", "head"}
    assert all(r["spans"] == [] for r in res)                                # nothing is fused away: every edge is one layer
    assert {"model.0", "model.2.cv1", "model.4.m.1.cv1", "model.4.m.1", "model.8", "model.9.conv"} <= {r["edge"] for r in res}
    _inside_the_ceiling(res, f"yolov8{scale}-cls as trained")
    # the form model.fuse() leaves: the helper built from it against the table read from it ...
    fused = yolov8_cls_ref.fuse_state(sd)
    assert "model.0.conv.bias" in fused and not any(".bn." in k for k in fused)
    res_fused = run(yolov8_cls_ref.make(scale, fused), x, range(12), sd=fused)
    assert [r["edge"] for r in res_fused] == [r["edge"] for r in res]
    _inside_the_ceiling(res_fused, f"yolov8{scale}-cls fused")
    # ... and the table read from the fused dict restates the layers of the UNFUSED network: the two forms give the same results
    _inside_the_ceiling(run(net, x, range(12), sd=fused), f"yolov8{scale}-cls as trained against the fused table")
    # the u8 entry: no logits, the soft-max edge spans the head and keeps its absolute bar
    ops = ll.yolo_cls_ops(sd, scale, entry="u8")
    got = hooked_forward(net, x, [op.out for op in ops])
    got["probs"] = torch.softmax(got.pop("logits"), 1)
    last = ll.check_edges(got.__getitem__, x, sd, BARS, range(12), absent=ll.expected_absent(sd, "f32", entry="u8"), entry="u8")[-1]
    assert last["edge"] == "probs" and last["kind"] == "softmax" and last["spans"] == ["logits"] and last["bar"] == 1e-6


def _planted(yolos, scale, edge, plant_full, images=range(12)):
    sd, net = yolos(scale)
    with pytest.raises(AssertionError) as ei:
        run(net, squares(), images, plant_full=plant_full, sd=sd)
    failing, text = _only_failing(ei)
    assert failing == [edge], text
    assert "missing" not in text and "stated absent" not in text, text
    return next(r for r in ei.value.results if r["edge"] == edge)


def test_yolo_planted_shortcut_added_before_the_silu_is_named(yolos):
    def plant(m, i, o):                                                       # Bottleneck: silu(bn(conv(cv1(x))) + x) instead of x + silu(...)
        return F.silu(m.cv2.bn(m.cv2.conv(m.cv1(i[0]))) + i[0])
    _planted(yolos, "m", "model.6.m.2", {"model.6.m.2": plant})


def test_yolo_planted_wrong_slice_into_a_second_bottleneck_is_named(yolos):
    stash = {}

    def keep(m, i, o):
        stash["cv1"] = o

    def plant(m, i, o):                                                       # channels [0, c) of model.4.cv1 instead of model.4.m.0
        c = o.shape[1]
        with torch.no_grad():
            return m.act(m.bn(m.conv(stash["cv1"][:, :c])))
    _planted(yolos, "n", "model.4.m.1.cv1", {"model.4.cv1": keep, "model.4.m.1.cv1": plant})


def test_yolo_planted_relu_instead_of_silu_in_one_cv2_is_named(yolos):
    def plant(m, i, o):
        return F.relu(m.bn(m.conv(i[0])))
    _planted(yolos, "s", "model.6.m.0", {"model.6.m.0.cv2": plant})          # cv2 has no tap of its own: its Bottleneck's output fails


def test_yolo_planted_stale_second_slab_group_of_an_80_channel_slice_is_named(yolos):
    def plant(m, i, o):                                                       # x: c = 80 = one 64-row slab + a quarter; channels 64..71 are
        o = o.clone()                                                         # the first group of the second slab, left at what was there
        o[:, 64:72] = o.roll(1, 0)[:, 64:72]                                  # (here: the neighbouring square's values)
        return o
    bad = _planted(yolos, "x", "model.2.m.1", {"model.2.m.1": plant}, images=range(4))
    assert 64 <= bad["worst"][1] < 72


def test_yolo_planted_last_column_of_a_2x2_map_without_its_left_neighbour_is_named(yolos):
    def plant(m, i, o):
        x = i[0].clone()
        x[5, :, :, 0] = 0.0                                                   # square 5: column 1 computed as if column 0 were padding
        o = o.clone()
        o[5, :, :, 1] = m.act(m.bn(m.conv(x)))[5, :, :, 1]
        return o
    bad = _planted(yolos, "l", "model.8.m.0.cv1", {"model.8.m.0.cv1": plant}, images=range(4, 8))
    assert bad["worst"][0] == 5 and bad["worst"][3] == 1 and bad["on_ring"]


def test_yolo_a_dropped_tap_fails_the_run_and_is_named(yolos):
    sd, net = yolos("n")
    with pytest.raises(AssertionError, match=r"tap 'model\.6\.m\.1\.cv1' is missing and not in the stated absent set"):
        run(net, squares(), [0, 2], drop=["model.6.m.1.cv1"], sd=sd)
    with pytest.raises(AssertionError, match=r"tap 'model\.2\.cv1' is missing and not in the stated absent set"):
        run(net, squares(), [0, 2], drop=["model.2.cv1"], sd=sd)
    for prec in ("f32", "f16x3", "f16"):
        assert ll.expected_absent(sd, prec) == frozenset() and ll.expected_absent(sd, prec, entry="u8") == {"logits"}
    assert ll.yolo_cls_depths(synthetic.yolov8_cls_state_dict(2, "m")) == (2, 4, 4, 2)
    with pytest.raises(AssertionError, match="the state dict is yolov8n-cls"):
        ll.yolo_cls_ops(sd, "yolov8s-cls")

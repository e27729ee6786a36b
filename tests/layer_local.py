"""Layer-local parity: every tapped layer of the UNet, the ResNet and the YOLOv8-cls classifiers against float64, one layer at a time.

TEST INFRASTRUCTURE -- a plain module (no conftest), imports nothing from ``chessvision.hip_backend``, so the CPU tests drive it with
forward hooks of the torch oracle and the GPU tests with ``HipEngine.activation``.

The idea: a whole-forward test asserts the logits only, and ten to thirty layers behind a kernel that is wrong on one border row, one
channel group or one slice parity wash the defect out.  Here each layer is evaluated on its own: the DEVICE's input tap(s) of the layer
go through a float64 restatement of just that layer on the CPU, and the result is compared with the DEVICE's output tap at the op-level
bar.  Nothing upstream of the input tap and nothing downstream of the output tap takes part.

Three parts:
  * float64 reference ops on ``torch.nn.functional`` over ``double`` tensors, straight from a reference-format state dict (they share no
    code with oracle/unet_ref.py / oracle/resnet_ref.py / tests/yolov8_cls_ref.py beyond torch itself; BatchNorm eps = 1e-5 -- 1e-3 for
    YOLOv8-cls -- folded in float64);
  * the edge tables: one ``Op`` per module output, (output tap, input taps, reference function, kind).  Where an engine fuses a tensor
    away (the stated ``expected_absent`` set) the edge spans the ops from the nearest upstream tap; any OTHER missing tap fails the run;
  * ``check_edges``: evaluates the edges for the chosen images, returns the figures and raises ONE AssertionError naming every failing edge.

Bars (``BARS``; none is new -- tests/test_gpu_ops.py TOL, the bilinear / OutConv op bars of pointwise.hip and
test_outconv_golden_vector_and_edge_logits, test_softmax13): relative kinds are ``factor * max(1, max|ref|)``, soft-max is absolute,
max-pools / copies / aliases are bit-exact (both sides are stored values, rounding is monotone, a power-of-two exponent change is exact).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
YOLO_BN_EPS = 1e-3                 # ultralytics sets it in initialize_weights; a state dict does not carry it
INPUT = "@x"                       # the caller's input tensor (float32 as the engine receives it, or u8 / 255 done in float32)

# ---- bars ---------------------------------------------------------------------------------------------------------------------
EXACT = ("pool", "copy", "alias")
_F32 = {"conv": 1e-4, "bilinear": 1e-5, "outconv": 1e-5, "head": 1e-4, "softmax": 1e-6}
_F16 = {"conv": 4e-3, "bilinear": 4e-3, "head": 1e-4, "softmax": 1e-6}
BARS = {"f32": _F32, "f16x3": _F32, "f16": _F16, "f16r": _F16}
# a spanning edge (fused ops) takes the kind of highest rank among the ops it spans, its own on a tie: a pool or an OutConv fused into a
# convolution is held to the convolution's bar, the soft-max of the u8 classifier entry keeps its absolute 1e-6
_RANK = {"alias": 0, "copy": 0, "pool": 0, "bilinear": 1, "outconv": 1, "conv": 2, "head": 2, "softmax": 3}


def bar_of(bars: dict, kind: str, max_ref: float) -> float:
    if kind in EXACT:
        return 0.0
    if kind == "softmax":
        return bars[kind]
    return bars[kind] * max(1.0, max_ref)


# ---- float64 reference ops ----------------------------------------------------------------------------------------------------
def _p(sd, key) -> torch.Tensor:
    return torch.as_tensor(np.asarray(sd[key])).to(torch.float64)


def conv_bn(sd, conv, bn, x, stride=1, residual=None, relu=True):
    """conv k x k / stride / pad (k-1)/2 with the eval-mode BatchNorm folded into weight and bias in float64 (+ residual) (+ ReLU)."""
    w = _p(sd, conv + ".weight")
    scale = _p(sd, bn + ".weight") / torch.sqrt(_p(sd, bn + ".running_var") + BN_EPS)
    shift = _p(sd, bn + ".bias") - _p(sd, bn + ".running_mean") * scale
    y = F.conv2d(x, w * scale.view(-1, 1, 1, 1), shift, stride=stride, padding=(w.shape[-1] - 1) // 2)
    if residual is not None:
        y = y + residual
    return F.relu(y) if relu else y


def conv_act(sd, p, x, stride=1, act="silu", shortcut=None, eps=YOLO_BN_EPS):
    """ultralytics ``Conv`` ``p``: conv k x k / stride / pad k // 2, then the eval-mode BatchNorm (``p.bn.*``, folded in float64) or -- a
    checkpoint as ``model.fuse()`` leaves it -- the bias ``p.conv.bias`` with scale 1, then the activation, then (+ shortcut): the add
    comes AFTER the activation.  A filter with more input channels than ``x`` has is summed over them (the grey square repeated)."""
    w = _p(sd, p + ".conv.weight")
    if w.shape[1] != x.shape[1]:
        assert x.shape[1] == 1, (p, tuple(w.shape), tuple(x.shape))
        w = w.sum(1, keepdim=True)
    if p + ".conv.bias" in sd:
        shift = _p(sd, p + ".conv.bias")
    else:
        scale = _p(sd, p + ".bn.weight") / torch.sqrt(_p(sd, p + ".bn.running_var") + eps)
        shift = _p(sd, p + ".bn.bias") - _p(sd, p + ".bn.running_mean") * scale
        w = w * scale.view(-1, 1, 1, 1)
    y = F.conv2d(x, w, shift, stride=stride, padding=w.shape[-1] // 2)
    y = {"silu": lambda t: t * torch.sigmoid(t), "relu": F.relu, "none": lambda t: t}[act](y)
    return y if shortcut is None else y + shortcut


def yolo_head(sd, x):
    return F.linear(x.mean((2, 3)), _p(sd, "model.9.linear.weight"), _p(sd, "model.9.linear.bias"))


def maxpool2(x):
    return F.max_pool2d(x, 2)


def maxpool3s2(x):
    return F.max_pool2d(x, 3, stride=2, padding=1)           # pads with -inf


def conv_transpose_k2s2(sd, prefix, x):
    return F.conv_transpose2d(x, _p(sd, prefix + ".weight"), _p(sd, prefix + ".bias"), stride=2)


def bilinear2x(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


def outconv(sd, x):
    return F.conv2d(x, _p(sd, "outc.conv.weight"), _p(sd, "outc.conv.bias"))


def head(sd, x):
    return F.linear(F.adaptive_avg_pool2d(x, 1).flatten(1), _p(sd, "fc.weight"), _p(sd, "fc.bias"))


def softmax(x):
    return torch.softmax(x, 1)


# ---- edge tables --------------------------------------------------------------------------------------------------------------
Op = namedtuple("Op", "out ins fn kind")            # fn(state_dict, *inputs as float64 (n, C, H, W)) -> float64


def is_unet(sd) -> bool:
    return "outc.conv.weight" in sd


def unet_ops(sd) -> list:
    """Every module output of UNet(3, 1[, bilinear]) by its tap name (cv_get_activation; unet.cpp: Engine::UNet::build_taps) + "logits"."""
    bilinear = "up1.up.weight" not in sd
    ops = [Op("input", [INPUT], lambda sd, x: F.pad(x, (0, 0, 0, 0, 0, 5)), "copy")]      # the 8-channel packed copy (f32 engine)

    def double_conv(p, first_ins):
        ops.append(Op(p + ".2", first_ins, lambda sd, *xs, p=p: conv_bn(sd, p + ".0", p + ".1", torch.cat(xs, 1)), "conv"))
        ops.append(Op(p + ".5", [p + ".2"], lambda sd, x, p=p: conv_bn(sd, p + ".3", p + ".4", x), "conv"))
        return p + ".5"

    skips = [double_conv("inc.double_conv", [INPUT])]
    ops.append(Op("inc", [skips[0]], lambda sd, x: x, "alias"))
    for i in range(1, 5):
        p = f"down{i}.maxpool_conv"
        ops.append(Op(p + ".0", [skips[-1]], lambda sd, x: maxpool2(x), "pool"))
        skips.append(double_conv(p + ".1.double_conv", [p + ".0"]))
        ops.append(Op(f"down{i}", [skips[-1]], lambda sd, x: x, "alias"))
    deep = skips[4]
    for i in range(1, 5):
        up = f"up{i}.up"
        if bilinear:
            ops.append(Op(up, [deep], lambda sd, x: bilinear2x(x), "bilinear"))
        else:
            ops.append(Op(up, [deep], lambda sd, x, up=up: conv_transpose_k2s2(sd, up, x), "conv"))
        deep = double_conv(f"up{i}.conv.double_conv", [skips[4 - i], up])      # torch.cat([skip, upsampled], 1)
        ops.append(Op(f"up{i}", [deep], lambda sd, x: x, "alias"))
    ops.append(Op("logits", [deep], lambda sd, x: outconv(sd, x), "outconv"))
    return ops


def resnet_depths(sd) -> tuple:
    return tuple(len({k.split(".")[1] for k in sd if k.startswith(f"layer{l}.")}) for l in range(1, 5))


def resnet_ops(sd, entry: str = "float") -> list:
    """Every module output of the timm ResNet (18 or 34, by the keys of ``sd``) by its tap name (resnet.cpp: Engine::ResNet::build_taps) + "logits";
    ``entry="u8"`` adds "probs", the soft-max the u8 classifier entry returns."""
    ops = [Op("act1", [INPUT], lambda sd, x: conv_bn(sd, "conv1", "bn1", x, stride=2), "conv"),
           Op("maxpool", ["act1"], lambda sd, x: maxpool3s2(x), "pool")]
    cur = "maxpool"
    for l, depth in enumerate(resnet_depths(sd), start=1):
        for b in range(depth):
            p = f"layer{l}.{b}"
            stride = 2 if (b == 0 and l > 1) else 1
            ops.append(Op(p + ".act1", [cur], lambda sd, x, p=p, s=stride: conv_bn(sd, p + ".conv1", p + ".bn1", x, stride=s), "conv"))
            shortcut = cur
            if p + ".downsample.0.weight" in sd:
                shortcut = p + ".downsample"
                ops.append(Op(shortcut, [cur], lambda sd, x, p=p, s=stride: conv_bn(sd, p + ".downsample.0", p + ".downsample.1", x,
                                                                                    stride=s, relu=False), "conv"))
            ops.append(Op(p, [p + ".act1", shortcut], lambda sd, y, r, p=p: conv_bn(sd, p + ".conv2", p + ".bn2", y, residual=r), "conv"))
            cur = p
        ops.append(Op(f"layer{l}", [cur], lambda sd, x: x, "alias"))
    ops.append(Op("logits", [cur], lambda sd, x: head(sd, x), "head"))
    if entry == "u8":
        ops.append(Op("probs", ["logits"], lambda sd, x: softmax(x), "softmax"))
    return ops


YOLO_STEM_WIDTHS = {16: "n", 32: "s", 48: "m", 64: "l", 80: "x"}


def is_yolo_cls(sd) -> bool:
    return "model.0.conv.weight" in sd


def yolo_cls_scale(sd) -> str:
    """"n" | "s" | "m" | "l" | "x" by the widths in the dict: the stem's and, as a cross-check, model.9.conv's input (16 x the stem's)."""
    w0, w4 = int(sd["model.0.conv.weight"].shape[0]), int(sd["model.9.conv.conv.weight"].shape[1])
    assert w0 in YOLO_STEM_WIDTHS and w4 == 16 * w0, f"not a YOLOv8-cls state dict: stem width {w0}, model.9.conv input {w4}"
    return YOLO_STEM_WIDTHS[w0]


def yolo_cls_depths(sd) -> tuple:
    return tuple(len({k.split(".")[3] for k in sd if k.startswith(f"model.{P}.m.")}) for P in (2, 4, 6, 8))


def yolo_cls_ops(sd, arch=None, entry: str = "float") -> list:
    """Every module output of the ultralytics YOLOv8-cls in ``sd`` (as trained, or as ``model.fuse()`` leaves it) by its tap name
    (yolo_cls.cpp: Engine::YoloCls::build_taps) + "logits"; ``entry="u8"`` adds "probs".  ``arch`` ("yolov8x-cls" or "x"), when given,
    must be the scale the widths of ``sd`` say.  A C2f's chunk / cat move nothing: its Bottlenecks read and write channel slices of
    tensors that are themselves taps, so every edge goes from stored inputs to one stored output."""
    scale = yolo_cls_scale(sd)
    if arch is not None:
        assert (arch[6] if arch.startswith("yolov8") else arch) == scale, f"{arch!r} asked for, the state dict is yolov8{scale}-cls"
    ops = [Op("model.0", [INPUT], lambda sd, x: conv_act(sd, "model.0", x, stride=2), "conv")]
    cur = "model.0"
    for s, n in enumerate(yolo_cls_depths(sd)):
        down, P = f"model.{2 * s + 1}", f"model.{2 * s + 2}"
        c = int(sd[P + ".cv1.conv.weight"].shape[0]) // 2
        ops.append(Op(down, [cur], lambda sd, x, p=down: conv_act(sd, p, x, stride=2), "conv"))
        ops.append(Op(P + ".cv1", [down], lambda sd, x, p=P + ".cv1": conv_act(sd, p, x), "conv"))
        for i in range(n):
            b = f"{P}.m.{i}"
            if i == 0:                               # the second half of cv1's output: torch.chunk(2, 1)[1]
                src, cut = P + ".cv1", (lambda t, c=c: t[:, c:2 * c])
            else:
                src, cut = f"{P}.m.{i - 1}", (lambda t: t)
            ops.append(Op(b + ".cv1", [src], lambda sd, x, p=b + ".cv1", cut=cut: conv_act(sd, p, cut(x)), "conv"))
            ops.append(Op(b, [b + ".cv1", src], lambda sd, y, r, p=b + ".cv2", cut=cut: conv_act(sd, p, y, shortcut=cut(r)), "conv"))
        ops.append(Op(P, [P + ".cv1"] + [f"{P}.m.{i}" for i in range(n)],
                      lambda sd, *xs, p=P + ".cv2": conv_act(sd, p, torch.cat(xs, 1)), "conv"))
        cur = P
    ops.append(Op("model.9.conv", [cur], lambda sd, x: conv_act(sd, "model.9.conv", x), "conv"))
    ops.append(Op("logits", ["model.9.conv"], lambda sd, x: yolo_head(sd, x), "head"))
    if entry == "u8":
        ops.append(Op("probs", ["logits"], lambda sd, x: softmax(x), "softmax"))
    return ops


def ops_for(sd, entry: str = "float") -> list:
    if is_unet(sd):
        return unet_ops(sd)
    return yolo_cls_ops(sd, entry=entry) if is_yolo_cls(sd) else resnet_ops(sd, entry)


def expected_absent(sd, precision: str, entry: str = "float", fused_head: bool = True, chain_form: int = 2) -> frozenset:
    """The taps an engine of ``precision`` does NOT materialise for the model of ``sd`` -- the complete, stated list.  A tap missing
    outside this set fails ``check_edges``; a tap of this set that IS exposed fails it too (it would go unchecked)."""
    absent = set()
    if is_unet(sd):
        if precision != "f32":
            absent.add("input")                     # the first layer reads the caller's image, no packed copy
        if precision == "f16x3":
            absent.add("inc.double_conv.2")         # fused inc pair: exists only inside inc.double_conv.3's kernel
        if fused_head:
            absent |= {"up4.conv.double_conv.5", "up4"}
        return frozenset(absent)
    if is_yolo_cls(sd):                             # every layer is one launch and every output is stored, in every precision
        return frozenset({"logits"} if entry == "u8" else ())
    if precision != "f32":
        absent.add("act1")                          # stem + max-pool in one kernel
    if precision == "f16r":                         # layer1 (up to three blocks) as one chained launch
        nb = min(resnet_depths(sd)[0], 3)
        absent |= {f"layer1.{b}.act1" for b in range(nb)}
        if chain_form == 1:
            absent |= {f"layer1.{b}" for b in range(nb - 1)}
    if entry == "u8":
        absent.add("logits")                        # the u8 entry returns the soft-max
    return frozenset(absent)


# ---- the check ----------------------------------------------------------------------------------------------------------------
def check_edges(taps, inputs, state_dict, bars, images, absent=frozenset(), entry="float", only=None, ops=None):
    """Evaluate every edge of the model of ``state_dict`` on images ``images`` (indices into the tapped batch).

    ``taps``: callable name -> ndarray / tensor (N, C, H, W) or (N, classes) of the tapped batch, raising when the tensor is not exposed;
    ``inputs``: the caller's input of that batch, (N, C, H, W) float32; ``bars``: one entry of ``BARS``; ``absent``: the stated set of
    taps the engine fuses away (``expected_absent``); ``only``: restrict the checked outputs to these names.
    Returns [{"edge", "kind", "max_abs_err", "max_ref", "bar", "worst", "on_ring", "ok"}]; raises ONE AssertionError naming every
    failing edge, every unexpectedly missing tap and every tap stated absent but exposed."""
    ops = ops_for(state_dict, entry) if ops is None else ops
    by_out = {op.out: op for op in ops}
    idx = torch.as_tensor(list(images), dtype=torch.long)
    problems, cache = [], {}

    def fetch(name):                                 # device side: the stored tensor, float64, chosen images; None when not exposed
        if name not in cache:
            if name == INPUT:
                cache[name] = torch.as_tensor(np.asarray(inputs))[idx].to(torch.float64)
            else:
                try:
                    got = taps(name)
                except Exception as exc:            # noqa: BLE001 -- whatever the tap source raises for "not exposed"
                    cache[name] = None
                    if name not in absent:
                        problems.append(f"tap '{name}' is missing and not in the stated absent set ({type(exc).__name__}: {exc})")
                else:
                    cache[name] = torch.as_tensor(np.asarray(got))[idx].to(torch.float64)
                    if name in absent:
                        problems.append(f"tap '{name}' is stated absent but the engine exposes it: it would go unchecked")
        return cache[name]

    def source(name):                                # reference side input: the device tap, or -- fused away -- the ops behind it
        got = fetch(name)
        if got is not None:
            return got, "alias", []
        op = by_out[name]
        xs, kind, spanned = [], op.kind, [name]
        for i in op.ins:
            x, k, s = source(i)
            xs.append(x); spanned += s
            kind = k if _RANK[k] > _RANK[kind] else kind
        return op.fn(state_dict, *xs), kind, spanned

    results = []
    for op in ops:
        if only is not None and op.out not in only:
            continue
        got = fetch(op.out)
        if got is None:
            continue                                 # in the absent set (or reported above): its consumers span it
        xs, kind, spanned = [], op.kind, []
        for i in op.ins:
            x, k, s = source(i)
            xs.append(x); spanned += s
            kind = k if _RANK[k] > _RANK[kind] else kind
        with torch.no_grad():
            ref = op.fn(state_dict, *xs)
        if tuple(ref.shape) != tuple(got.shape):
            problems.append(f"edge '{op.out}': tap shape {tuple(got.shape)} != reference shape {tuple(ref.shape)}")
            continue
        d = (got - ref).abs()
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))       # a NaN on either side is a failure, not a pass
        flat = int(d.argmax())
        worst = tuple(int(v) for v in np.unravel_index(flat, tuple(d.shape)))
        err, max_ref = float(d.max()), float(ref.abs().max())
        on_ring = err > 0.0 and d.dim() == 4 and (worst[2] in (0, d.shape[2] - 1) or worst[3] in (0, d.shape[3] - 1))
        bar = bar_of(bars, kind, max_ref)
        ok = err <= bar
        results.append({"edge": op.out, "kind": kind, "spans": spanned, "max_abs_err": err, "max_ref": max_ref, "bar": bar,
                        "worst": [int(idx[worst[0]])] + list(worst[1:]), "on_ring": bool(on_ring), "ok": bool(ok)})
        if not ok:
            problems.append(f"edge '{op.out}' [{kind}{' spanning ' + '+'.join(spanned) if spanned else ''}]: max-abs err {err:.3e} > bar "
                            f"{bar:.3e} (max|ref| {max_ref:.3f}) at (image, ...) = {results[-1]['worst']}"
                            f"{', on the border ring' if on_ring else ''}; {int((d > bar).sum())} of {d.numel()} elements over the bar")
    for name in absent:                              # a stated-absent tap nobody consumed is still probed
        if name in by_out:
            fetch(name)
    if problems:
        err = AssertionError(f"{len(problems)} layer-local problem(s):\n  " + "\n  ".join(problems))
        err.results = results
        raise err
    return results


def failing_edges(exc: AssertionError) -> list:
    return [r["edge"] for r in getattr(exc, "results", []) if not r["ok"]]


def worst_edge(results: list) -> dict:
    """The edge closest to (or furthest past) its bar; bit-exact edges count as 0 when exact and infinite otherwise."""
    def ratio(r):
        if r["bar"] == 0.0:
            return 0.0 if r["max_abs_err"] == 0.0 else float("inf")
        return r["max_abs_err"] / r["bar"]
    w = max(results, key=ratio)
    return {"edge": w["edge"], "err_over_bar": ratio(w), "on_ring": w["on_ring"], "max_abs_err": w["max_abs_err"], "bar": w["bar"]}


# ---- inputs that put weight where kernels go wrong (section "inputs": deterministic from oracle.prng / chessvision.synthetic) ------------
SPECIAL_SQUARES = ("zero", "full", "frame", "corner_tl", "corner_tr", "corner_bl", "corner_br", "ramp_h", "ramp_v")


def special_square(kind: str, seed: int = 0) -> np.ndarray:
    from oracle import prng

    sq = np.zeros((64, 64), dtype=np.uint8)
    if kind == "full":
        sq[:] = 255
    elif kind == "frame":                            # zero except a random 3-pixel frame along the edge
        rnd = prng.bytes_u8(seed, "frame", (64, 64))
        sq[:3], sq[-3:], sq[:, :3], sq[:, -3:] = rnd[:3], rnd[-3:], rnd[:, :3], rnd[:, -3:]
    elif kind.startswith("corner_"):
        sq[0 if kind[7] == "t" else 63, 0 if kind[8] == "l" else 63] = 255
    elif kind == "ramp_h":
        sq[:] = (np.arange(64) * 4 + 1).astype(np.uint8)[None, :]
    elif kind == "ramp_v":
        sq[:] = (np.arange(64) * 4 + 1).astype(np.uint8)[:, None]
    elif kind != "zero":
        raise KeyError(kind)
    return sq


def squares_u8(seed: int, n: int, special_at: dict) -> np.ndarray:
    """(n, 64, 64) uint8: random bytes, with the squares at ``special_at`` = {index: kind of SPECIAL_SQUARES} replaced."""
    from oracle import prng

    sq = prng.bytes_u8(seed, "layer_local_squares", (n, 64, 64))
    for i, kind in special_at.items():
        sq[i] = special_square(kind, seed + i)
    return sq


def specials_from(first: int) -> dict:
    """All nine special squares in a row from index ``first`` (the rows around them stay random)."""
    return {first + j: kind for j, kind in enumerate(SPECIAL_SQUARES)}


def squares_f32(u8: np.ndarray) -> torch.Tensor:
    """(N, 1, 64, 64) float32: ``/= 255.0`` in float32, as core.py does before the classifier."""
    t = torch.from_numpy(u8).to(torch.float32).unsqueeze(1)
    t /= 255.0
    return t


def unet_images_u8(seed: int, kinds) -> np.ndarray:
    """(B, 256, 256, 3) uint8 HWC; kinds of "random" (bytes), "photo" (synthetic.board_photo), "border" (the outermost two rows and
    columns saturated, the rest zero)."""
    from chessvision import synthetic
    from oracle import prng

    out = np.zeros((len(kinds), 256, 256, 3), dtype=np.uint8)
    for i, kind in enumerate(kinds):
        if kind == "random":
            out[i] = prng.bytes_u8(seed + i, "layer_local_unet", (256, 256, 3))
        elif kind == "photo":
            out[i] = synthetic.board_photo(seed + i, 256)
        elif kind == "border":
            out[i, :2], out[i, -2:], out[i, :, :2], out[i, :, -2:] = 255, 255, 255, 255
        else:
            raise KeyError(kind)
    return out


def unet_f32(u8: np.ndarray) -> torch.Tensor:
    """(B, 3, 256, 256) float32: u8 / 255 in float32, NCHW."""
    return (torch.from_numpy(u8).to(torch.float32) / 255).permute(0, 3, 1, 2).contiguous()

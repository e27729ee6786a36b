"""CPU fp32 YOLOv8-cls (ultralytics' classification models, scales n / s / m / l / x) in plain torch, for the YOLOv8-cls tests.

TEST INFRASTRUCTURE -- never imported by the product.  ultralytics is not needed: this restates ``yolov8-cls.yaml`` and the modules
``Conv``, ``Bottleneck``, ``C2f`` and ``Classify`` of ``ultralytics.nn.modules``:

    Conv(c1,c2,k,s)  = Conv2d(k, s, pad=k//2, bias=False) -> BatchNorm2d(eps=1e-3) -> SiLU
    Bottleneck(c)    = x + Conv(c,c,3,1)(Conv(c,c,3,1)(x))            (the add after the SiLU, nothing after the add)
    C2f(c1,c2,n)     : c = c2//2; y = chunk(Conv(c1,2c,1)(x), 2); y += [m_i(y[-1]) for i<n]; Conv((2+n)c, c2, 1)(cat(y))
    Classify(c1,nc)  : Linear(1280,nc)(avgpool(Conv(c1,1280,1)(x)).flatten(1))          (eval returns the softmax; here: the logits)
    model = [Conv(ch,w0,3,2), Conv(w0,w1,3,2), C2f(w1,w1,n0), Conv(w1,w2,3,2), C2f(w2,w2,n1),
             Conv(w2,w3,3,2), C2f(w3,w3,n2), Conv(w3,w4,3,2), C2f(w4,w4,n3), Classify(w4,nc)]
    widths = ceil8(min(c,1024)*width) for c in 64,128,256,512,1024;  depths = max(round(n*depth),1) for n in 3,6,6,3

The module tree gives the state-dict keys of ``YOLO(path).model.state_dict()`` (``model.0.conv.weight``, ``model.2.m.0.cv1.bn.weight``,
``model.9.linear.bias`` ...).  The structural pin is the parameter count ultralytics prints for ch=3, nc=1000 (PARAMS_3CH_1000 below).
``forward`` takes the reference's (N,1,64,64) squares in [0,1] and repeats them to the model's input channels, as the reference does.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

BN_EPS = 1e-3
NUM_CLASSES = 13
SCALES = {"n": (0.33, 0.25), "s": (0.33, 0.50), "m": (0.67, 0.75), "l": (1.0, 1.0), "x": (1.0, 1.25)}     # (depth, width)
# what ultralytics prints for yolov8{n,s,m,l,x}-cls (3 input channels, 1000 classes), and the same plan at 1 channel / 13 classes
PARAMS_3CH_1000 = {"n": 2_719_288, "s": 6_361_736, "m": 17_053_336, "l": 37_480_744, "x": 57_422_840}
PARAMS_1CH_13 = {"n": 1_454_653, "s": 5_096_813, "m": 15_788_125, "l": 36_215_245, "x": 56_157_053}
MACS_1CH_13 = {"n": 16_154_880, "s": 61_653_248, "m": 207_290_624, "l": 492_388_608, "x": 767_525_120}


def scale_of(arch: str) -> str:
    """"yolov8m-cls" -> "m" (a bare scale letter is returned as it is)."""
    return arch[6] if arch.startswith("yolov8") else arch


def widths(scale: str):
    return [int(math.ceil(min(c, 1024) * SCALES[scale][1] / 8) * 8) for c in (64, 128, 256, 512, 1024)]


def depths(scale: str):
    return [max(round(n * SCALES[scale][0]), 1) for n in (3, 6, 6, 3)]


class Conv(nn.Module):
    def __init__(self, c1, c2, k=1, s=1, fused=False):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, k // 2, bias=fused)
        self.bn = nn.Identity() if fused else nn.BatchNorm2d(c2, eps=BN_EPS)
        self.act = nn.SiLU()

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


class Bottleneck(nn.Module):
    def __init__(self, c, fused=False):
        super().__init__()
        self.cv1 = Conv(c, c, 3, 1, fused)
        self.cv2 = Conv(c, c, 3, 1, fused)

    def forward(self, x):
        return x + self.cv2(self.cv1(x))


class C2f(nn.Module):
    def __init__(self, c1, c2, n, fused=False):
        super().__init__()
        self.c = c2 // 2
        self.cv1 = Conv(c1, 2 * self.c, 1, 1, fused)
        self.cv2 = Conv((2 + n) * self.c, c2, 1, 1, fused)
        self.m = nn.ModuleList(Bottleneck(self.c, fused) for _ in range(n))

    def forward(self, x):
        y = list(self.cv1(x).chunk(2, 1))
        y.extend(m(y[-1]) for m in self.m)
        return self.cv2(torch.cat(y, 1))


class Classify(nn.Module):
    def __init__(self, c1, nc, fused=False):
        super().__init__()
        self.conv = Conv(c1, 1280, 1, 1, fused)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.linear = nn.Linear(1280, nc)

    def features(self, x):
        return self.pool(self.conv(x)).flatten(1)

    def forward(self, x):
        return self.linear(self.features(x))


class YoloV8Cls(nn.Module):
    def __init__(self, scale: str, ch: int = 3, nc: int = NUM_CLASSES, fused: bool = False):
        super().__init__()
        w, d = widths(scale), depths(scale)
        layers = [Conv(ch, w[0], 3, 2, fused)]
        for i in range(4):
            layers += [Conv(w[i], w[i + 1], 3, 2, fused), C2f(w[i + 1], w[i + 1], d[i], fused)]
        layers.append(Classify(w[4], nc, fused))
        self.model = nn.Sequential(*layers)
        self.ch = ch

    def _input(self, x):
        return x.repeat(1, self.ch, 1, 1) if x.shape[1] == 1 and self.ch != 1 else x

    def pooled(self, x):
        """(N, 1280): the input of the linear layer -- the pooled model.9.conv output."""
        return self.model[9].features(self.model[:9](self._input(x)))

    def forward(self, x):
        return self.model(self._input(x))


def make(arch: str, state: dict | None = None, ch: int = 3, nc: int = NUM_CLASSES) -> YoloV8Cls:
    """The helper in eval mode for ``arch`` ("yolov8m-cls" or "m"), with ``state`` loaded when given (numpy or torch values; as trained,
    or in the form ``model.fuse()`` leaves: conv.weight + conv.bias, no bn.*)."""
    fused = state is not None and "model.0.conv.bias" in state
    if state is not None:
        ch = int(state["model.0.conv.weight"].shape[1])
        nc = int(state["model.9.linear.weight"].shape[0])
    net = YoloV8Cls(scale_of(arch), ch, nc, fused).eval()
    if state is not None:
        sd = {k: torch.as_tensor(v) for k, v in state.items()}
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return net


def fuse_state(state: dict) -> dict:
    """``state`` as ``model.fuse()`` would leave it: every BatchNorm folded into its convolution (float64 arithmetic, rounded once)."""
    out = {}
    for k, v in state.items():
        if ".bn." in k:
            continue
        v = torch.as_tensor(v)
        if k.endswith(".conv.weight"):
            p = k[:-len(".conv.weight")]
            g, b, m, var = (torch.as_tensor(state[f"{p}.bn.{leaf}"]).double() for leaf in ("weight", "bias", "running_mean", "running_var"))
            s = g / torch.sqrt(var + BN_EPS)
            out[k] = (v.double() * s.view(-1, 1, 1, 1)).float()
            out[f"{p}.conv.bias"] = (b - m * s).float()
        else:
            out[k] = v
    return out


def params(net: nn.Module) -> int:
    return sum(p.numel() for p in net.parameters())


def macs(net: nn.Module, hw: int = 64) -> int:
    """Multiply-accumulates of one (1, ch, hw, hw) forward: every Conv2d and Linear, counted as tests/resnet34_ref.macs counts them."""
    total = 0

    def hook(mod, inp, out):
        nonlocal total
        if isinstance(mod, nn.Conv2d):
            total += out.numel() * mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1]
        else:
            total += out.numel() * mod.in_features

    hs = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
    with torch.no_grad():
        net(torch.zeros(1, net.ch, hw, hw))
    for h in hs:
        h.remove()
    return total


def taps(net: nn.Module, x: torch.Tensor, names) -> dict:
    """Outputs of the named modules ("model.1", "model.4.m.1", "model.9.conv" ...) for input ``x``, plus "logits" and "pooled"."""
    out: dict = {}
    mods = dict(net.named_modules())
    hs = [mods[n].register_forward_hook(lambda m, i, o, n=n: out.__setitem__(n, o.detach().clone())) for n in names]
    with torch.no_grad():
        out["logits"] = net(x)
        out["pooled"] = net.pooled(x)
    for h in hs:
        h.remove()
    return out

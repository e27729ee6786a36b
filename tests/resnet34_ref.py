"""CPU fp32 timm-style ResNet-34 (in_chans=1, num_classes=13) for the ResNet-34 tests.

TEST INFRASTRUCTURE -- never imported by the product.  timm builds ``resnet34`` as ``ResNet(BasicBlock, layers=[3, 4, 6, 3])``:
the stem, stage widths, stride-2 first blocks, ``downsample = [conv1x1 s2, BN]``, ``global_pool`` and ``fc`` of ResNet-18, only
deeper stages.  This stacks ``oracle.resnet_ref.BasicBlock`` / ``_GlobalPool`` (the restatement the ResNet-18 oracle is pinned by)
in that plan, so the module names are ResNet-18's with the extra blocks inserted, in order.
"""
from __future__ import annotations

import sys
from pathlib import Path

import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle.resnet_ref import BN_EPS, NUM_CLASSES, BasicBlock, _GlobalPool  # noqa: E402

DEPTHS = (3, 4, 6, 3)
WIDTHS = (64, 128, 256, 512)


class ResNet34(nn.Module):
    def __init__(self, num_classes: int = NUM_CLASSES, in_chans: int = 1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_chans, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64, eps=BN_EPS)
        self.act1 = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        cin = 64
        for i, (w, d) in enumerate(zip(WIDTHS, DEPTHS)):
            blocks = [BasicBlock(cin, w, 1 if i == 0 else 2)] + [BasicBlock(w, w, 1) for _ in range(d - 1)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
            cin = w
        self.global_pool = _GlobalPool()
        self.fc = nn.Linear(512, num_classes)

    def forward_features(self, x):
        x = self.maxpool(self.act1(self.bn1(self.conv1(x))))
        for i in range(1, 5):
            x = getattr(self, f"layer{i}")(x)
        return x

    def forward(self, x):
        return self.fc(self.global_pool(self.forward_features(x)))


def make_resnet34(state: dict | None = None) -> ResNet34:
    """The helper in eval mode, with ``state`` (numpy or torch values, no ``num_batches_tracked``) loaded when given."""
    net = ResNet34().eval()
    if state is not None:
        sd = {k: torch.as_tensor(v) for k, v in state.items()}
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return net


def macs(net: nn.Module | None = None, hw: int = 64) -> int:
    """Multiply-accumulates of one (1, 1, hw, hw) forward: every Conv2d and Linear, counted as oracle.resnet_ref.resnet18_macs counts."""
    net = (net or ResNet34()).eval()
    total = 0

    def hook(mod, inp, out):
        nonlocal total
        if isinstance(mod, nn.Conv2d):
            total += out.numel() * mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1]
        else:
            total += out.numel() * mod.in_features

    hs = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
    with torch.no_grad():
        net(torch.zeros(1, 1, hw, hw))
    for h in hs:
        h.remove()
    return total


def taps(net: nn.Module, x: torch.Tensor, names) -> dict:
    """Outputs of the named modules for input ``x`` (forward hooks), as float32 CPU tensors."""
    out: dict = {}
    mods = dict(net.named_modules())
    hs = [mods[n].register_forward_hook(lambda m, i, o, n=n: out.__setitem__(n, o.detach().clone())) for n in names]
    with torch.no_grad():
        logits = net(x)
    for h in hs:
        h.remove()
    out["logits"] = logits
    return out

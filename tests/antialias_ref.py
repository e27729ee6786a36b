"""Shared by tests/test_resize_antialias_cpu.py and tests/test_gpu_resize_antialias.py: the cases, the reference and the bar of the
antialiased bilinear resize (``classical.resize_antialias`` on the host, ``HipEngine.resize_antialias_f32`` on the device).

Reference: the real implementation, ``torch.nn.functional.interpolate(u8.float() / 255, (256, 256), mode="bilinear", antialias=True,
align_corners=False)`` on the CPU -- what ``v2.Resize((256, 256), antialias=True)`` of the reference's enrichment job runs on a float
image (scripts/process_new_raw/process_pipeline.py:340-344).

Bar (derived, not tuned): ``2**-24 * (taps_w + taps_h + 8)`` absolute, taps = the widest tap count of each axis: one float32 rounding
per tap and pass plus the weight normalisation, on values in [0, 1].  9.5e-7 at 512 -> 256 (4 + 4 taps)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from chessvision import classical

OUT = 256
# (h, w, batch, channels)
CASES = [
    (256, 256, 3, 3),        # identity: exact
    (16, 16, 3, 3),          # enlarging
    (512, 512, 3, 3),        # the workload's factor
    (300, 400, 3, 3),        # two fractional factors
    (300, 400, 3, 1),        # one channel
    (200, 180, 3, 3),        # enlarging on both axes
    (257, 511, 3, 3),        # odd sizes, a factor just above 1
    (1024, 768, 3, 3),
    (1536, 2048, 1, 3),      # 12 / 16 taps: beyond any unrolled count, beyond one LDS slab
    (255, 1000, 1, 3),       # enlarging on one axis, 8 taps on the other
]


def case_id(case) -> str:
    h, w, n, c = case
    return f"{h}x{w}-n{n}-c{c}"


def images(case, seed: int = 0) -> np.ndarray:
    """(n,h,w,c) random uint8 of a case."""
    h, w, n, c = case
    return np.random.default_rng(seed * 7919 + h * 4099 + w * 3 + c).integers(0, 256, (n, h, w, c), dtype=np.uint8)


def bar(h: int, w: int, out: int = OUT) -> float:
    taps_w = int(classical.antialias_taps(w, out)[1].max())
    taps_h = int(classical.antialias_taps(h, out)[1].max())
    return 2.0 ** -24 * (taps_w + taps_h + 8)


def torch_resize(batch_u8: np.ndarray, out: int = OUT) -> np.ndarray:
    """(n,h,w,c) uint8 -> (n,c,out,out) float32 by the real implementation on the CPU."""
    x = torch.from_numpy(batch_u8).permute(0, 3, 1, 2).float() / 255
    return F.interpolate(x, (out, out), mode="bilinear", antialias=True, align_corners=False).numpy()

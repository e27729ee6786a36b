"""GPU: the single launches the YOLOv8-cls plan adds, per element against float64 of the STORED operands (tests/quantised_ref.py).

  conv      SiLU and SiLU + residual-after in the implicit-GEMM epilogue, on channel slices narrower than a wave's 64-row slab, with
            the tensor exponents (in, out) = (0, 0) and (-3, 2) on the f16x3 engine.  Window per element:
                1.1 * W_pre + 8 * 2^-24 * |ref|
            W_pre = the window quantised_ref gives the pre-activation; 1.1 bounds |silu'| (its maximum is 1.0998); the second term
            covers the exponential (library expf, <= 1 ulp), the add (1/2 ulp), the IEEE division (1/2 ulp) and the residual add, with
            room to spare.  The store's own rounding is applied to the window's ends as quantised_ref.window does.
  slices    every channel outside the written slice of the destination is bit-equal afterwards.
  refusal   a layer the halo kernel would take with ReLU runs on the implicit-GEMM kernel with SiLU (the predicates: the CPU test).
  stem      conv 3x3 s2 + BN + SiLU from float, u8 and normalised u8 squares.
  head      average pool + Linear(1280 -> 13), logits / softmax / pooled features."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "chessvision-3lc_amd"), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import quantised_ref as q  # noqa: E402
from chessvision.hip_backend import HipBackendError, HipEngine  # noqa: E402
from oracle import prng  # noqa: E402

pytestmark = pytest.mark.gpu

U = q.U
EXPS = {"f32": ((0, 0),), "f16x3": ((0, 0), (-3, 2))}


@pytest.fixture(scope="module")
def engines():
    out = {p: HipEngine(precision=p) for p in EXPS}
    yield out
    for e in out.values():
        e.close()


def silu64(t):
    return t / (1.0 + np.exp(-t))


def grid_values(seed, name, shape):
    """N(0, 1) on a grid of 1/64: every storage holds them exactly, at exponent 0 and at exponent 2."""
    return (np.round(prng.normal(seed, name, shape) * 64.0) / 64.0 + 0.0).astype(np.float32)      # + 0.0: no negative zero (hi + lo loses its sign)


# (name, k, stride, cin, cout, x channels, x offset, y channels, y offset, residual offset in y (-1: none), map, batches)
# 16 and 48 are the Bottleneck widths of n and m: a slice of a 64- / 192-channel concat tensor, reading one slice and writing the next
CONV_CASES = [
    ("c16_16x16", 3, 1, 16, 16, 64, 16, 64, 32, 16, 16, (2,)),
    ("c16_4x4", 3, 1, 16, 16, 64, 16, 64, 32, 16, 4, (64, 300)),
    ("c16_2x2", 3, 1, 16, 16, 64, 16, 64, 32, 16, 2, (64, 520)),
    ("c48_16x16", 3, 1, 48, 48, 192, 48, 192, 96, 48, 16, (2,)),
    ("c48_4x4", 3, 1, 48, 48, 192, 48, 192, 96, 48, 4, (64, 300)),
    ("c48_2x2", 3, 1, 48, 48, 192, 48, 192, 96, 48, 2, (64, 520)),
    ("c128_4x4", 3, 1, 128, 128, 384, 128, 384, 256, 128, 4, (300,)),           # 128 rows, table-free offsets: position-major at this batch
    ("p64_32", 1, 1, 64, 32, 64, 0, 96, 16, 48, 8, (3,)),
    ("p768_1280", 1, 1, 768, 1280, 768, 0, 1280, 0, -1, 2, (8, 64)),
    ("s2_16_32", 3, 2, 16, 32, 16, 0, 64, 32, 0, 16, (2, 64)),
]


# (case, batch) -> the launch form beyond the plain one.  Position-major needs a 128-row tile and table-free offsets (Cin a multiple of
# the 128-byte line), which among the Bottleneck widths only 128 and up have; split-K is the planner's choice for launches of few tiles
# with a long K.  The 16- and 48-channel slices gather through the offset table and run the plain form at every batch.
FORMS = {("c128_4x4", 300): "POS", ("p768_1280", 8): "splitK"}


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
@pytest.mark.parametrize("prec", list(EXPS))
def test_conv_silu_per_element(engines, prec, case):
    name, k, stride, cin, cout, xc, xoff, yc, yoff, res_off, hw, batches = case
    eng = engines[prec]
    ho = hw // stride
    for n in batches:
        xs, rows, scale, shift, _ = q.exact_data(prec, name, (n, cin, hw, hw), (cout, cin, k, k))
        x_full = grid_values(3, name + "xf", (n, xc, hw, hw))
        x_full[:, xoff:xoff + cin] = xs
        y_init = grid_values(5, name + "y", (n, yc, ho, ho))
        for in_exp, out_exp in EXPS[prec]:
            # stored operands are the exact-sum integers whatever the exponent: the true input is xs * 2^in_exp
            w = q.conv_window(prec, xs, rows, np.ldexp(scale, in_exp), shift, exact=True, stride=stride)
            assert w.ratio < 2.0 ** 24, (name, w.ratio)
            for with_res in (False, True):
                if with_res and res_off < 0:
                    continue
                ref = silu64(w.pre)
                if with_res:
                    ref = ref + np.ldexp(y_init[:, res_off:res_off + cout].astype(np.float64), out_exp)
                delta = 1.1 * w.delta + 8 * U * np.abs(ref)
                lo, hi, _ = q.window(prec, np.ldexp(ref, -out_exp), np.ldexp(delta, -out_exp))      # in stored units, where the store rounds
                got = eng.op_conv2d_act(torch.from_numpy(np.ldexp(x_full, in_exp).astype(np.float32)), rows,
                                        torch.from_numpy(np.ldexp(y_init, out_exp).astype(np.float32)), x_coff=xoff, y_coff=yoff,
                                        stride=stride, scale=scale, shift=shift, act="silu", act_first=with_res,
                                        res_coff=res_off if with_res else -1, in_exp=in_exp, out_exp=out_exp).cpu().numpy()
                kern = eng.op_kernels()
                what = f"{name} {prec} n={n} exps=({in_exp},{out_exp}) res={with_res} {kern}"
                sl = np.ldexp(got[:, yoff:yoff + cout].astype(np.float64), -out_exp)
                err = np.abs(sl - np.ldexp(ref, -out_exp))
                print(f"{what}: worst |got - ref| / delta (the store's rounding not counted) = {float((err / np.maximum(np.ldexp(delta, -out_exp), 1e-300)).max()):.3f}")
                q.assert_inside(sl, lo, hi, what)
                # the padding rows of the 64-row slab are not stored: every other channel of the destination keeps its bits
                keep = np.ones(yc, bool)
                keep[yoff:yoff + cout] = False
                assert np.array_equal(got[:, keep], np.ldexp(y_init, out_exp).astype(np.float32)[:, keep]), what
                assert len(kern) == 1 and "conv_igemm_kernel" in kern[0], what                    # never the halo family
                # the form the planner takes for this shape: with it the position-major and the split-K instantiations of the
                # extended epilogue (and the split-K second pass) stay covered; a moved threshold shows up here
                form = FORMS.get((name, n), "")
                assert (",POS" in kern[0]) == (form == "POS") and (",splitK" in kern[0]) == (form == "splitK"), (what, form)


SENTINEL = {"f32": np.array([0xDEADBEEF], np.uint32).view(np.float32)[0],          # -6.26e18: nothing a SiLU layer writes
            "f16x3": np.array([0xDEAD], np.uint16).view(np.float16).astype(np.float32)[0]}     # -427.25, the f16 with those bits: hi exact, lo 0


@pytest.mark.parametrize("prec", list(EXPS))
def test_slice_stores_leave_the_neighbouring_slices_alone(engines, prec):
    eng = engines[prec]
    n, hw, c = 5, 8, 16
    xs, rows, scale, shift, _ = q.exact_data(prec, "slice", (n, c, hw, hw), (c, c, 3, 3))
    y_init = np.full((n, 64, hw, hw), SENTINEL[prec], np.float32)                              # one bit pattern everywhere
    for yoff in (0, 16, 48):
        got = eng.op_conv2d_act(torch.from_numpy(xs), rows, torch.from_numpy(y_init), y_coff=yoff, scale=scale, shift=shift, act="silu").cpu().numpy()
        keep = np.ones(64, bool)
        keep[yoff:yoff + c] = False
        assert np.array_equal(got[:, keep].view(np.uint32), y_init[:, keep].view(np.uint32)), yoff
        assert not (got[:, ~keep].view(np.uint32) == y_init[:, ~keep].view(np.uint32)).any(), yoff   # ... and every element of the slice was written


def test_silu_never_reaches_a_launch_form_without_it(engines):
    """A 3x3 / s1 layer of 64 channels on 16 x 16 maps is the halo kernel's with ReLU; asked for SiLU, or for the activation ahead of
    the residual, the planner runs it on the implicit-GEMM kernel instead -- and the result is SiLU's, not ReLU's.  (What each
    launcher and the planner refuse is a pure predicate, checked combination by combination in tests/test_yolov8_cls_cpu.py.)"""
    eng = engines["f16x3"]
    n, c, hw = 256, 64, 16                                   # enough 16 x 16 patches for the planner to pick the halo tile
    xs, rows, scale, shift, _ = q.exact_data("f16x3", "halo_shape", (n, c, hw, hw), (c, c, 3, 3))
    zeros = torch.zeros(n, c, hw, hw)
    relu = eng.op_conv2d_act(torch.from_numpy(xs), rows, zeros, scale=scale, shift=shift, act="relu").cpu().numpy()
    assert any("conv3x3_halo_kernel" in s for s in eng.op_kernels()), eng.op_kernels()
    w = q.conv_window("f16x3", xs, rows, scale, shift, exact=True)
    for act, first in (("silu", False), ("silu", True), ("relu", True)):
        got = eng.op_conv2d_act(torch.from_numpy(xs), rows, zeros, scale=scale, shift=shift, act=act, act_first=first).cpu().numpy()
        assert all("conv_igemm_kernel" in s for s in eng.op_kernels()), (act, first, eng.op_kernels())
        ref = silu64(w.pre) if act == "silu" else np.maximum(w.pre, 0.0)
        lo, hi, _ = q.window("f16x3", ref, 1.1 * w.delta + 8 * U * np.abs(ref))
        q.assert_inside(got, lo, hi, f"{act} first={first}")
    assert float(np.abs(relu - np.maximum(w.pre, 0.0)).max()) < 1e-3 < float(np.abs(relu - silu64(w.pre)).max())      # the two differ visibly
    # an activation nobody knows is an error of the planner, not ReLU
    with pytest.raises(HipBackendError, match="unknown epilogue activation"):
        eng.ACTS["gelu"] = 3
        try:
            eng.op_conv2d_act(torch.from_numpy(xs), rows, zeros, act="gelu")
        finally:
            del eng.ACTS["gelu"]


@pytest.mark.parametrize("c0", (16, 48))
@pytest.mark.parametrize("prec", list(EXPS))
def test_stem_against_float64(engines, prec, c0):
    eng = engines[prec]
    w = prng.normal(61, f"stem_w{c0}", (c0, 9), 0.0, (2.0 / 9) ** 0.5).astype(np.float32)
    scale = prng.uniform(62, f"stem_s{c0}", (c0,), 0.5, 1.5).astype(np.float32)
    shift = prng.normal(63, f"stem_b{c0}", (c0,), 0.0, 0.1).astype(np.float32)
    mean, std = np.float32(0.445), np.float32(0.269)
    for n in (1, 65):
        u8 = (prng.bits64(64, f"stem_x{n}", n * 4096) >> np.uint64(40)).astype(np.uint8).reshape(n, 64, 64)
        as_float = (u8.astype(np.float32) / np.float32(255)).astype(np.float32)
        inputs = {"float": (torch.from_numpy(as_float), None, as_float),
                  "u8": (torch.from_numpy(u8), None, as_float),
                  "u8_norm": (torch.from_numpy(u8), (float(mean), float(std)), ((as_float - mean) / std).astype(np.float32))}
        for kind, (x, norm, plane) in inputs.items():
            p64 = torch.from_numpy(plane.astype(np.float64)).unsqueeze(1)
            w64 = torch.from_numpy(w.astype(np.float64)).reshape(c0, 1, 3, 3)
            acc = F.conv2d(p64, w64, stride=2, padding=1).numpy()
            absacc = F.conv2d(p64.abs(), w64.abs(), stride=2, padding=1).numpy()
            sc, sh = scale.astype(np.float64).reshape(1, -1, 1, 1), shift.astype(np.float64).reshape(1, -1, 1, 1)
            pre = acc * sc + sh
            # nine FMAs and the affine in float32: (9 + 3) roundings, each below sum|x w| |scale| + |shift|
            w_pre = 12 * U * (absacc * np.abs(sc) + np.abs(sh))
            ref = silu64(pre)
            delta = 1.1 * w_pre + 8 * U * np.abs(ref)
            lo, hi, _ = q.window(prec, ref, delta)
            got = eng.op_stem3x3s2(x, w, scale, shift, normalize=norm).cpu().numpy()
            assert got.shape == (n, c0, 32, 32)
            q.assert_inside(got, lo, hi, f"stem {prec} c0={c0} n={n} {kind}")


@pytest.mark.parametrize("prec", list(EXPS))
def test_head_against_float64(engines, prec):
    eng = engines[prec]
    c = 1280
    w = prng.normal(71, "head_w", (13, c), 0.0, c ** -0.5).astype(np.float32)
    b = prng.normal(72, "head_b", (13,), 0.0, 0.1).astype(np.float32)
    for n in (1, 63, 300):
        x = prng.normal(73, f"head_x{n}", (n, c, 2, 2)).astype(np.float32)
        xs = q.stored_value(q.store(prec, x))                                 # what the engine holds
        pooled_ref = xs.reshape(n, c, 4).mean(axis=2)
        sum_abs = np.abs(xs).reshape(n, c, 4).sum(axis=2)
        logits, pooled = eng.op_head_pool_fc(torch.from_numpy(x), w, b)
        probs, _ = eng.op_head_pool_fc(torch.from_numpy(x), w, b, softmax=True)
        logits, pooled, probs = logits.cpu().numpy().astype(np.float64), pooled.cpu().numpy().astype(np.float64), probs.cpu().numpy().astype(np.float64)
        # a 4-term float32 sum (3 adds), the scale by 1/4 (exact) and, for split-f16 storage, hi + lo per term: 8 roundings at most
        assert (np.abs(pooled - pooled_ref) <= 8 * U * sum_abs / 4 + 1e-300).all(), (prec, n)
        ref = pooled_ref @ w.astype(np.float64).T + b.astype(np.float64)
        bound = c * U * (np.abs(pooled_ref) @ np.abs(w.astype(np.float64)).T + np.abs(b.astype(np.float64)))     # the usual dot-product bound
        assert (np.abs(logits - ref) <= bound).all(), (prec, n, float((np.abs(logits - ref) / bound).max()))
        e = np.exp(ref - ref.max(axis=1, keepdims=True))
        p_ref = e / e.sum(axis=1, keepdims=True)
        # |dp| <= 2 max|dlogit| p, plus the fast exponential of the soft-max (a few 2^-24 relative) and its division
        assert (np.abs(probs - p_ref) <= 2 * bound.max(axis=1, keepdims=True) + 16 * U).all(), (prec, n)
        assert np.abs(probs.sum(axis=1) - 1.0).max() <= 1e-6

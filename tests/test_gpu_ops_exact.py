"""GPU parity per element: every kernel form of the single-layer entry points inside the windows of tests/quantised_ref.py.

tests/test_gpu_ops.py holds the ops to a bar scaled by the global maximum of a float32 reference on unrounded operands.  Here the
reference is float64 on what the engine stores, each output element has its own window (a few float32 ulps of the epilogue plus the
store's own rounding), and the operands come in two kinds: exact-sum data (any K, split-K included: the accumulation is exact in every
order) and the rounded-normal operands of test_gpu_ops.py (K <= 576, where the order-free accumulation bound is still tight).

The cases are the smallest shapes that reach each launch form, derived from the launch planner (engine.cpp: choose_ct, choose_cfg, the
halo and split-K conditions of Engine::run_conv, the Knobs defaults), not from the networks.  Every test reads the form string of its
own launch (HipEngine.op_kernels) and the last test fails if a required family of forms was reached by no case: a planner threshold
that moves cannot silently take a form's op-level case away.

Each test prints one ``OPX|`` line (case, precision, kind, form, undecided share, worst |got - act(pre)| / delta); the figures of the run
that introduced the file are in profiles/op_exact_parity.md.
"""
from __future__ import annotations

import re

import numpy as np
import pytest
import torch

import quantised_ref as q
from oracle import prng

pytestmark = pytest.mark.gpu

PRECS = list(q.PRECS)

# name, n, cin, h, w, cout, k, stride, relu, residual -- and why the planner sends it where the name says (M = output pixels,
# tiles = ceil(M / 256) * ceil(cout / 64) for the halo kernel)
CONV_CASES = [
    # halo_ok (3x3, stride 1, square map, extent % 16 == 0, Cin a whole 128-byte line): 64 tiles reach the halo threshold of 64; under
    # 384 workgroups the patch is 8 x 16
    ("halo_8x16", 16, 64, 32, 32, 64, 3, 1, True, False),
    # 384 tiles: the 16 x 16 patch, two channel tiles per patch
    ("halo_16x16_residual", 48, 64, 32, 32, 128, 3, 1, True, True),
    # 8 x 8 maps with Cout % 128 == 0 pack four images per patch; 258 images leave a ragged last group; 130 tiles >= 128
    ("halo_img8_ragged_residual", 258, 128, 8, 8, 128, 3, 1, True, True),
    # one board, 4 tiles, 72 (f16) / 144 stages: the K loop is dealt by channel blocks inside the halo kernel
    ("halo_splitk", 1, 512, 16, 16, 256, 3, 1, True, False),
    # one board, one 64-channel tile, 45 (f32, f16x3) stages of 32 channels: too few pixels for the halo kernel, so the generic kernel deals
    # the stages out, 23 splits of two with a last split of one; f16 (23 stages of 64) is cheaper unsplit
    ("splitk_cin160_uneven_stages", 1, 160, 16, 16, 64, 3, 1, False, False),
    # Cin padded to 8: no whole line, so the generic kernel with its offset table; Cout 16 / 64 -> the 64-row tile, short K -> 64x128
    ("igemm_64x128_cin8_cout16", 1, 8, 16, 16, 16, 3, 1, False, False),
    ("igemm_64x128_cin3", 2, 3, 32, 32, 64, 3, 1, True, False),
    # a non-square map is never halo_ok; Cout 128 -> 128-row tile, 480 pixels leave a ragged pixel tile
    ("igemm_128x128_ragged", 1, 64, 24, 20, 128, 3, 1, True, False),
    # Cout 64 packs 64-row tiles, which the halo kernel takes whenever both extents divide by 16 (square or not): a 40 x 40 map keeps the
    # generic kernel; more than 4 stages and 512 tiles of 64x256 (M = 82 * 1600: 513 tiles, the last one ragged) select its 64x256 tile
    ("igemm_64x256_40x40", 82, 64, 40, 40, 64, 3, 1, True, False),
    # Cout 128 and 256 tiles of 128x256: M = 256 * 256
    ("igemm_128x256_nonsquare_residual", 32, 64, 32, 64, 128, 3, 1, True, True),
    # Cout 256 and 256 tiles of 256x256 (CV_CT256_MIN_BLOCKS), not halo_ok because 1x1
    ("igemm_256x256_1x1", 16, 128, 64, 64, 256, 1, 1, True, False),
    # few tiles and long K on small or strided maps: the generic kernel dealt by K stages
    ("igemm_splitk_4x4_residual", 64, 256, 4, 4, 256, 3, 1, True, True),
    ("igemm_splitk_stride2", 16, 256, 8, 8, 512, 3, 2, True, False),
    # 4 x 4 maps with a pixel tile (128) of images per position and too short a K loop for a split to win: position-major rows
    ("igemm_pos_4x4", 256, 128, 4, 4, 128, 3, 1, True, False),
    ("igemm_1x1_stride2", 4, 64, 16, 16, 128, 1, 2, False, False),
]
# n, cin, h, w, cout: rows = 4 * cout
CONVT_CASES = [
    ("convT_small", 2, 64, 8, 8, 32),
    ("convT_unet_up1", 1, 1024, 16, 16, 512),        # one board of the UNet's first up-convolution: 16 / 32 stages, cheaper unsplit
    # 32 / 64 stages on 64 pixels: the cost model of run_conv deals the K stages out (twice the depth of any up-convolution of the UNet)
    ("convT_splitk", 1, 2048, 8, 8, 64),
]

# families of forms every precision must reach (ring depth and split count are not part of a family's name)
FAMILIES = ["halo 16x16", "halo 8x16", "halo IMG8", "halo splitK", "igemm 64x128", "igemm 64x256", "igemm 128x128", "igemm 128x256",
            "igemm 256x256", "igemm splitK", "igemm POS", "igemm shuffle", "igemm shuffle+splitK"]
REQUIRED = {p: set(FAMILIES) for p in PRECS}
_reached = {p: {} for p in PRECS}                    # family -> cases that ran it
_ran = {p: set() for p in PRECS}


def family_of(form: str) -> str:
    m = re.fullmatch(r"(conv3x3_halo_kernel|conv_igemm_kernel)<([^>]*)>", form)
    assert m, f"unknown form string {form!r}"
    parts = m.group(2).split(",")[1:]
    split = any(p.startswith("splitK") for p in parts)
    if m.group(1) == "conv3x3_halo_kernel":
        return "halo " + ("splitK" if split else "IMG8" if "IMG8" in parts else parts[1])
    if "shuffle" in parts:
        return "igemm shuffle" + ("+splitK" if split else "")
    return "igemm " + ("splitK" if split else "POS" if "POS" in parts else parts[0])


def test_family_of():
    assert family_of("conv3x3_halo_kernel<split_t,64,8x16,splitK4>") == "halo splitK"
    assert family_of("conv3x3_halo_kernel<half_t,64,16x16,IMG8>") == "halo IMG8"
    assert family_of("conv3x3_halo_kernel<float,64,8x16>") == "halo 8x16"
    assert family_of("conv_igemm_kernel<half_t,128x128,ring3,POS>") == "igemm POS"
    assert family_of("conv_igemm_kernel<half_t,128x128,ring3,shuffle,splitK8>") == "igemm shuffle+splitK"
    assert family_of("conv_igemm_kernel<float,256x256,ring3>") == "igemm 256x256"


def _note(name, prec, kind, form, win, got, relu):
    fam = family_of(form)
    _reached[prec].setdefault(fam, []).append(name)
    m = q.margin(got, win, prec, relu)
    print(f"OPX|{name}|{prec}|{kind}|{form}|{float(win.undecided.mean()):.5f}|{'-' if m is None else f'{m:.3f}'}")
    return fam


def _check(engines, prec, name, kind, ops, win, got, relu):
    eng = engines[prec]
    forms = eng.op_kernels()
    assert len(forms) == 1 and forms[0], forms
    _note(name, prec, kind, forms[0], win, got, relu)
    if kind == "exact":
        assert win.ratio < 2.0 ** 24, f"{name} [{prec}]: sum|x||w| reaches 2^{np.log2(win.ratio):.1f} granules: the case is not exactly summable"
        share = float(win.undecided.mean())
        assert share <= 0.01, f"{name} [{prec}]: {share:.4f} of the elements undecided: change the case"
    q.assert_inside(got, win.lo, win.hi, f"{name} [{prec}, {kind}] {forms[0]}")
    eng.check_numerics()


def _conv(engines, prec, case, kind):
    name, n, cin, h, w, cout, k, stride, relu, use_res = case
    pad = (k - 1) // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    rs = (n, cout, ho, wo) if use_res else None
    if kind == "exact":
        ops = q.exact_data(prec, name, (n, cin, h, w), (cout, cin, k, k), rs)
    else:
        ops = q.normal_data(name, (n, cin, h, w), (cout, cin, k, k), rs)
    x, wt, scale, shift, res = ops
    win = q.conv_window(prec, *ops, relu=relu, stride=stride, exact=kind == "exact")
    got = engines[prec].op_conv2d(torch.from_numpy(x), wt, stride=stride, scale=scale, shift=shift,
                                  residual=None if res is None else torch.from_numpy(res), relu=relu).cpu().numpy()
    _check(engines, prec, name, kind, ops, win, got, relu)


def _convT(engines, prec, case, kind):
    name, n, cin, h, w, cout = case
    if kind == "exact":
        x, rows, _, bias4, _ = q.exact_data(prec, name, (n, cin, h, w), (4 * cout, cin, 1, 1))
        rows = rows * np.float32(2.0 ** q.exact_scale_exponent(cin))         # the entry point has no scale: a power of two in the weights
        wt = np.ascontiguousarray(np.transpose(rows.reshape(4, cout, cin), (2, 1, 0))).reshape(cin, cout, 2, 2)   # inverse of convT_rows
        bias = bias4[:cout]
    else:
        x = prng.normal(21, name + "x", (n, cin, h, w))
        wt = prng.normal(22, name + "w", (cin, cout, 2, 2), 0.0, (1.0 / cin) ** 0.5)
        bias = prng.normal(23, name + "b", (cout,), 0.0, 0.1)
    rows, sc, sh = q.convT_rows(wt, bias)
    win = q.conv_window(prec, x, rows, sc, sh, exact=kind == "exact", shuffle_cout=cout)
    got = engines[prec].op_conv_transpose2x2(torch.from_numpy(x), wt, bias).cpu().numpy()
    _check(engines, prec, name, kind, None, win, got, False)


def _short_k(case):
    return case[2] * case[6] * case[6] <= 576


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_exact_sum(engines, prec, case):
    _ran[prec].add(case[0])
    _conv(engines, prec, case, "exact")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", CONVT_CASES, ids=[c[0] for c in CONVT_CASES])
def test_conv_transpose_exact_sum(engines, prec, case):
    _ran[prec].add(case[0])
    _convT(engines, prec, case, "exact")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", [c for c in CONV_CASES if _short_k(c)], ids=[c[0] for c in CONV_CASES if _short_k(c)])
def test_conv_rounded_normal(engines, prec, case):
    _conv(engines, prec, case, "normal")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", [c for c in CONVT_CASES if c[2] <= 576], ids=[c[0] for c in CONVT_CASES if c[2] <= 576])
def test_conv_transpose_rounded_normal(engines, prec, case):
    _convT(engines, prec, case, "normal")


@pytest.mark.parametrize("prec", PRECS)
def test_outc_exact_sum(engines, prec):
    """The stand-alone OutConv on exact-sum data: the logit inside its window; the mask where that window lies clear of the threshold."""
    x, w, bias = q.outc_data(prec, "outc", (2, 64, 16, 24))
    assert q.outc_exactness(prec, x, w) < 2.0 ** 24
    lo, hi, pre, delta, mask, decided = q.outc_window(prec, x, w, bias, 0.5)
    logits, got_mask = engines[prec].op_outc_1x1(torch.from_numpy(x), w, bias, 0.5)
    q.assert_inside(logits.cpu().numpy(), lo, hi, f"outc [{prec}]")
    assert decided.mean() > 0.99
    assert np.array_equal((got_mask.cpu().numpy() != 0)[decided], mask[decided])
    engines[prec].check_numerics()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(2, 32, 16, 16), (1, 16, 5, 9)], ids=["16x16", "5x9"])
def test_bilinear_rounded_normal(engines, prec, shape):
    """Bilinear x2, align_corners: a square size and an odd, non-square one, so that the first and last row and column blocks of the
    2 x 2-block kernel are not all the same case."""
    v = prng.normal(33, "up", shape)
    lo, hi, und, pre, delta = q.bilinear_window(prec, v)
    got = engines[prec].op_upsample_bilinear2x(torch.from_numpy(v)).cpu().numpy()
    print(f"OPX|bilinear_{shape[2]}x{shape[3]}|{prec}|normal|upsample_bilinear2x|{float(und.mean()):.5f}|-")
    q.assert_inside(got, lo, hi, f"bilinear {shape} [{prec}]")
    engines[prec].check_numerics()


def test_census_every_form_family_was_reached():
    """Runs last in this file.  Every family of REQUIRED must have been reached by at least one case of each precision whose exact-sum
    tests all ran (a selection with -k that left some of them out checks nothing)."""
    missing = {}
    for prec in PRECS:
        if _ran[prec] != {c[0] for c in CONV_CASES + CONVT_CASES}:
            continue
        for fam, cases in sorted(_reached[prec].items()):
            print(f"OPX-census|{prec}|{fam}|{','.join(sorted(set(cases)))}")
        gone = REQUIRED[prec] - set(_reached[prec])
        if gone:
            missing[prec] = sorted(gone)
    assert not missing, f"form families that no case reached: {missing}"

"""CPU: the per-element windows of tests/quantised_ref.py, against a float32 torch restatement of the device arithmetic.

Three statements:
  * the restatement (stored operands, float32 accumulation, float32 epilogue, the engine's store) lies inside every window, for the
    three precisions and both data kinds, and on exact-sum data its float32 accumulator IS the float64 one;
  * on exact-sum data the f16 window leaves at most 1 % of the elements undecided (a condition on the inputs, not on the device);
  * the gap this module closes: four mutants of the restatement fall outside the windows and pass the global-maximum bar of
    tests/test_gpu_ops.py (``TOL``).  Both halves are asserted.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import quantised_ref as q

# name, n, cin, h, w, cout, k, stride, relu, residual -- K = 27, 72, 64 (1x1 stride 2), 576, 2304, 4608
CASES = [
    ("k27", 2, 3, 12, 12, 32, 3, 1, True, False),
    ("k72", 2, 8, 12, 12, 32, 3, 1, True, False),
    ("k64_1x1_s2", 2, 64, 8, 8, 32, 1, 2, False, False),
    ("k576", 2, 64, 10, 10, 64, 3, 1, True, True),
    ("k2304", 1, 256, 8, 8, 32, 3, 1, True, False),
    ("k4608", 1, 512, 6, 6, 32, 3, 1, False, False),
]
BY_NAME = {c[0]: c for c in CASES}
_cache: dict = {}


def _case(name, prec, kind):
    """(operands, window, restatement, its accumulator, relu, stride), computed once per (case, precision, kind)."""
    key = (name, prec, kind)
    if key not in _cache:
        _, n, cin, h, w, cout, k, stride, relu, use_res = BY_NAME[name]
        pad = (k - 1) // 2
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        rs = (n, cout, ho, wo) if use_res else None
        if kind == "exact":
            ops = q.exact_data(prec, name, (n, cin, h, w), (cout, cin, k, k), rs)
        else:
            ops = q.normal_data(name, (n, cin, h, w), (cout, cin, k, k), rs)
        win = q.conv_window(prec, *ops, relu=relu, stride=stride, exact=kind == "exact")
        got, acc = q.device32(prec, *ops, relu=relu, stride=stride)
        _cache[key] = (ops, win, got, acc, relu, stride)
    return _cache[key]


def _kinds(name):
    cin, k = BY_NAME[name][2], BY_NAME[name][6]
    return ("exact", "normal") if cin * k * k <= 576 else ("exact",)


PARAMS = [(c[0], p, kind) for c in CASES for p in q.PRECS for kind in _kinds(c[0])]


@pytest.mark.parametrize("name,prec,kind", PARAMS)
def test_restatement_lies_inside_every_window(name, prec, kind):
    ops, win, got, acc, relu, _ = _case(name, prec, kind)
    q.assert_inside(got, win.lo, win.hi, f"{name} [{prec}, {kind}]")
    if kind == "exact":
        assert win.ratio < 2.0 ** 24, f"{name} [{prec}]: sum|x||w| reaches 2^{np.log2(win.ratio):.1f} granules: the case is not exactly summable"
        assert np.array_equal(acc.astype(np.float64), win.acc), "float32 accumulation of exact-sum data must equal the float64 one"
        m = q.margin(got, win, prec, relu)
        assert m is None or m <= 1.0


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_f16_window_leaves_at_most_one_percent_undecided(name):
    _, win, _, _, _, _ = _case(name, "f16", "exact")
    share = float(win.undecided.mean())
    assert share <= 0.01, f"{name}: {share:.4f} of the elements undecided"


def test_second_level_reaches_the_lo_halves_and_the_cross_terms():
    """f16x3, K <= 576: lo halves of inputs and weights are non-zero on a sizeable share, and the reference differs from hi*hi alone."""
    ops, win, _, _, _, _ = _case("k576", "f16x3", "exact")
    xh = q.store("f16x3", ops[0])
    wh, _, e = q.pack_rows("f16x3", ops[1], ops[2])
    assert (xh[1] != 0).mean() > 0.3 and (wh[1] != 0).mean() > 0.3
    assert len(set(e.tolist())) >= 3                               # rows normalise to different exponents
    hihi = F.conv2d(torch.from_numpy(xh[0]), torch.from_numpy(wh[0]), padding=1).numpy()
    assert (hihi != win.acc).mean() > 0.9


def test_transposed_rows_are_the_transposed_convolution():
    """convT_rows + pixel_shuffle_rows restate ConvLayer::build_convT: the float64 reference equals torch's conv_transpose2d."""
    from oracle import prng

    x = prng.normal(5, "ctx", (2, 16, 3, 5))
    w = prng.normal(6, "ctw", (16, 8, 2, 2))
    b = prng.normal(7, "ctb", (8,))
    rows, sc, sh = q.convT_rows(w, b)
    win = q.conv_window("f32", x, rows, sc, sh, exact=False, shuffle_cout=8)
    ref = F.conv_transpose2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=2).numpy()
    assert np.abs(win.pre - ref).max() < 1e-12
    got, _ = q.device32("f32", x, rows, sc, sh, shuffle_cout=8)
    q.assert_inside(got, win.lo, win.hi, "convT restatement")


@pytest.mark.parametrize("prec", q.PRECS)
def test_outc_and_bilinear_windows_hold_the_restatement(prec):
    from oracle import prng

    x, w, bias = q.outc_data(prec, "outc", (2, 64, 6, 7))
    lo, hi, pre, delta, mask, decided = q.outc_window(prec, x, w, bias)
    assert q.outc_exactness(prec, x, w) < 2.0 ** 24
    xs = q.stored_value(q.store(prec, x)).astype(np.float32)
    logit = (xs * w.reshape(1, -1, 1, 1)).sum(axis=1, keepdims=True, dtype=np.float32) + bias[0]
    q.assert_inside(logit, lo, hi, f"outc [{prec}]")
    assert decided.mean() > 0.99 and np.array_equal((logit[:, 0] > 0)[decided], mask[decided])
    for shape in ((2, 8, 16, 16), (1, 8, 5, 9)):
        v = prng.normal(33, "up", shape)
        lo, hi, und, pre, delta = q.bilinear_window(prec, v)
        # the nested float32 form of upsample_bilinear2x_kernel on the kernel's own weights (torch's CPU kernel forms its weights
        # differently in the last bits, which is why the op bar of test_gpu_ops.py cannot be tight)
        s = q.stored_value(q.store(prec, v)).astype(np.float32)
        (y0, y1, ly0, ly1), (x0, x1, lx0, lx1) = q._bilinear_axis(shape[2], 2 * shape[2]), q._bilinear_axis(shape[3], 2 * shape[3])
        ly0, ly1 = (a.astype(np.float32).reshape(-1, 1) for a in (ly0, ly1))
        lx0, lx1 = (a.astype(np.float32) for a in (lx0, lx1))
        top, bot = s[:, :, y0], s[:, :, y1]
        got = ly0 * (lx0 * top[..., x0] + lx1 * top[..., x1]) + ly1 * (lx0 * bot[..., x0] + lx1 * bot[..., x1])
        assert got.dtype == np.float32
        assert np.abs(got - F.interpolate(torch.from_numpy(s), scale_factor=2, mode="bilinear", align_corners=True).numpy()).max() <= 1e-5
        if prec != "f32":
            got = q.stored_value(q.store(prec, got))
        q.assert_inside(got, lo, hi, f"bilinear {shape} [{prec}]")


# ---- the mutant pairs ---------------------------------------------------------------------------------------------------------------
def _tol_err(prec, got, ops, relu, stride):
    """tests/test_gpu_ops.py: max|got - ref| and TOL * max(1, max|ref|), ref = torch float32 on the unrounded operands."""
    x, rows, scale, shift, res = ops
    k = rows.shape[-1]
    ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(rows), stride=stride, padding=(k - 1) // 2)
    ref = ref * torch.from_numpy(scale).view(1, -1, 1, 1) + torch.from_numpy(shift).view(1, -1, 1, 1)
    if res is not None:
        ref = ref + torch.from_numpy(res)
    if relu:
        ref = F.relu(ref)
    ref = ref.numpy()
    return float(np.abs(got - ref).max()), q.TOL[prec] * max(1.0, float(np.abs(ref).max()))


def _pair(name, prec, kind, **mutation):
    ops, win, _, _, relu, stride = _case(name, prec, kind)
    got, _ = q.device32(prec, *ops, relu=relu, stride=stride, **mutation)
    share = float(q.outside(got, win.lo, win.hi).mean())
    err, bar = _tol_err(prec, got, ops, relu, stride)
    return share, err, bar


@pytest.mark.parametrize("name,kind", [("k27", "exact"), ("k576", "exact"), ("k2304", "exact"), ("k4608", "exact"), ("k27", "normal"), ("k72", "normal")])
def test_mutant_truncating_f16_store(name, kind):
    """A store that rounds toward zero: about a quarter of the elements leave their window at every K; the global bar passes it."""
    share, err, bar = _pair(name, "f16", kind, truncate=True)
    assert share >= 0.05, share
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("name,which", [("k72", "all"), ("k576", "odd")])
def test_mutant_f16x3_without_the_input_lo_chain(name, which):
    """hi*hi + hi*lo only: the lo halves of the inputs never reach the MFMA -- everywhere (K = 72), or in the odd 8-channel K-groups,
    the ones stored [lo, hi] (K = 576).  Exact-sum data with the second level; the global bar passes both."""
    cin = BY_NAME[name][2]
    keep = np.zeros(cin, bool) if which == "all" else (np.arange(cin) // 8) % 2 == 0
    share, err, bar = _pair(name, "f16x3", "exact", x_lo_keep=keep)
    assert share >= 0.05, share
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("name,which", [("k72", "all"), ("k576", "odd")])
def test_mutant_f16x3_weight_lo_halves_zeroed(name, which):
    """The packer leaves the weights' lo halves zero (hi*hi + lo*hi only), everywhere or in the odd K-groups."""
    cin = BY_NAME[name][2]
    keep = np.zeros(cin, bool) if which == "all" else (np.arange(cin) // 8) % 2 == 0
    share, err, bar = _pair(name, "f16x3", "exact", w_lo_keep=keep)
    assert share >= 0.05, share
    assert err <= bar, (err, bar)


def test_mutant_tap_dropped_on_the_top_border_row():
    """f16x3, K = 576: on the top output row of image 0 the lo chunk of the centre tap is not read (its lo*hi products are missing).  A
    whole tap of hi values moves the output by a third of its spread and today's bar catches that; the lo chunk of a tap moves it by
    ~1e-4 and the bar does not.  Every element the mutation moves by more than the width of its window must leave it, and those
    are nearly all the elements the mutation touches."""
    ops, win, _, _, relu, stride = _case("k576", "f16x3", "exact")
    moved = {}

    def drop(acc, xh, wh):
        centre = np.zeros_like(wh[0])
        centre[:, :, 1, 1] = wh[0][:, :, 1, 1]
        d = F.conv2d(torch.from_numpy(xh[1]), torch.from_numpy(centre), padding=1).numpy()
        moved["d"] = d[0, :, 0, :].copy()
        acc[0, :, 0, :] -= moved["d"]

    got, _ = q.device32("f16x3", *ops, relu=relu, stride=stride, acc_edit=drop)
    bad = q.outside(got, win.lo, win.hi)
    rest = np.ones(bad.shape, bool)
    rest[0, :, 0, :] = False
    assert not bad[rest].any()                                                     # nothing else moved
    d = np.abs(moved["d"].astype(np.float64) * win.scale_eff.astype(np.float64).reshape(-1, 1))
    live = (win.pre[0, :, 0, :] - win.delta[0, :, 0, :] > 0) if relu else np.ones(d.shape, bool)   # a ReLU hides what stays negative
    touched = (d > 0) & live
    beyond = (d > (win.hi - win.lo)[0, :, 0, :]) & live
    assert touched.sum() >= 100 and beyond.sum() >= 0.9 * touched.sum(), (int(touched.sum()), int(beyond.sum()))
    assert bad[0, :, 0, :][beyond].all()
    err, bar = _tol_err("f16x3", got, ops, relu, stride)
    assert err <= bar, (err, bar)

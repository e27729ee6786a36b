"""Per-element windows for the single-layer entry points: a float64 reference computed from what the engine STORES.

TEST INFRASTRUCTURE -- a plain module (no conftest), imports nothing from ``chessvision.hip_backend``.  The CPU tests drive it with a
float32 torch restatement of the device arithmetic, the GPU tests with ``HipEngine.op_*``.

tests/test_gpu_ops.py compares with torch float32 on the caller's unrounded operands under a bar scaled by the global maximum.  That
bar has to cover the operands' f16 rounding and the order of summation, so it is tens to thousands of times wider than what a kernel
itself may add: a store that truncates instead of rounding, or a split-f16 product that loses a cross term, passes it.  Here the
reference starts from the stored operands, so the only freedom left to the device is the float32 epilogue and the store (and, for
operands that are not exactly summable, the order of the accumulation), and every output element gets its own window.

What is restated, and from where (chessvision-3lc_amd/csrc):
  storage      f16: round to nearest even (pointwise.hip: pack_nchw_f32_kernel -> Grp<half_t>::store, conv_device.h: OutVec<half_t>)
               split-f16 ("f16x3"): hi = f16(v), lo = f16(v - hi) (models.h: f16_half; cv_kernels.h: split_pair)
               f32: identity
  weights      engine.cpp: finish_layer -- per output row e = frexp exponent of the row's largest magnitude, the stored row is
               w * 2^-e in the engine's type, the epilogue scale is ldexp(scale, e) in float32; f32 rows are not normalised.
               The transposed convolution uses the rows ConvLayer::build_convT forms: row (dy*2 + dx) * cout + co, K = cin,
               scale 1, shift = bias[co].
  product      cv_kernels.h (kSplit): hi*hi + hi*lo + lo*hi -- the lo*lo products are not formed
  epilogue     conv_igemm_body.h / conv_igemm.hip (split-K second pass) / conv_halo.hip: v = acc * scale' + shift in float32,
               + residual (one float32 add for f32, one FMA on the stored residual otherwise), ReLU, store.

THE WINDOW.  pre = conv64(x^, w^) * scale' + shift (+ res^) in float64, with x^, w^, res^ the stored values.
  delta = 4 * 2^-24 * (|acc * scale'| + |shift| + |res^|)
The epilogue has at most three float32 roundings -- multiply, add (one if the compiler contracts them), residual add -- each relative
to a magnitude that is below that sum; the fourth unit covers the second-order terms.  For operands that are not exactly summable the
accumulation term (K + 3) * 2^-24 * sum|x^ w^| * |scale'| is added: the order-free bound of a float32 sum of K products.  (For
split-f16 three MFMA chains feed the accumulator; the MFMA adds a k-block of 32 products per instruction, so the number of float32
roundings stays far below K.)  The device value before the store lies in [pre - delta, pre + delta]; ReLU and every store are
monotone, so the admissible stored values are everything between store(act(pre - delta)) and store(act(pre + delta)):
  f16    both ends rounded to nearest even, straight from float64.  Where the two ends differ the element is UNDECIDED: it still has
         to lie between them.
  f32    the ends themselves.
  f16x3  hi + lo misses v by at most 2^-22 |v| + 2^-24 (hi: 2^-11 relative; lo: 2^-11 relative to |v - hi| <= 2^-11 |v|; the
         constant covers the f16 subnormal grid), so the ends move outwards by that much.

THE TWO DATA KINDS.
  exact-sum     inputs are integers in [-3, 3], weights integers in [-2, 2] times 2^-(row % 5) (so rows normalise to different
                exponents), and for f16x3 with K <= 576 a second level of +-2^-12 on a random half of the NON-ZERO inputs and weight
                integers, which makes lo halves and cross terms non-zero (added to a zero it would become the hi half itself, and
                hi*hi products of 2^-24 would break the condition below).  Every product and every partial sum in ANY order is then
                a multiple of the row's granule and below 2^24 granules, i.e. representable in float32: MFMA chains, split-K
                partials and the reduce pass are exact, whatever K.  ``conv_window`` evaluates that condition per output element
                (``Window.ratio``) and every test asserts it: a case that misses it is an error in the case.
  rounded-normal the prng.normal operands of tests/test_gpu_ops.py, through the storage above.  The accumulation term makes the
                window useful for short K only (K <= 576): it tests what exact data cannot -- rounding of unrepresentable inputs and
                weights, lo halves with full mantissas.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import prng

U = 2.0 ** -24                          # unit roundoff of float32
PRECS = ("f32", "f16", "f16x3")
TOL = {"f32": 1e-4, "f16": 4e-3, "f16x3": 1e-4}      # tests/test_gpu_ops.py TOL, restated for the mutant pairs (not used as a bar here)
SECOND_LEVEL = 2.0 ** -12
SECOND_LEVEL_MAX_K = 576


# ---- storage ------------------------------------------------------------------------------------------------------------------
def rne_f16(v: np.ndarray) -> np.ndarray:
    """Round to nearest even to f16, in ONE rounding from the array's own type (numpy converts float64 -> float16 directly)."""
    return np.asarray(v).astype(np.float16).astype(np.float64)


def store(prec: str, v: np.ndarray) -> tuple:
    """The halves the engine holds for float32 values ``v``, as float64 arrays: (v,), (f16(v),) or (hi, lo)."""
    v = np.asarray(v, np.float32).astype(np.float64)
    if prec == "f32":
        return (v,)
    hi = rne_f16(v)
    if prec == "f16":
        return (hi,)
    return (hi, rne_f16(v - hi))                              # v - hi is exact in float64 (and in float32, as the device forms it)


def stored_value(halves: tuple) -> np.ndarray:
    return halves[0] if len(halves) == 1 else halves[0] + halves[1]


def halves_are_normal(halves: tuple) -> bool:
    """Every stored half is zero or a normal number of its type (no f16 subnormal, no overflow)."""
    for h in halves:
        a = np.abs(h[h != 0])
        if a.size and not (np.isfinite(a).all() and a.min() >= 2.0 ** -14):
            return False
    return True


def pack_rows(prec: str, rows: np.ndarray, scale: np.ndarray):
    """finish_layer: rows (R, ...) float32 -> (stored halves, epilogue scale' float32 (R,), row exponents)."""
    rows = np.asarray(rows, np.float32)
    scale = np.asarray(scale, np.float32)
    R = rows.shape[0]
    if prec == "f32":
        return store(prec, rows), scale.copy(), np.zeros(R, np.int32)
    m = np.abs(rows.reshape(R, -1)).max(axis=1)
    e = np.where(m > 0, np.frexp(m)[1], 0).astype(np.int32)
    wn = np.ldexp(rows, -e.reshape((R,) + (1,) * (rows.ndim - 1))).astype(np.float32)
    return store(prec, wn), np.ldexp(scale, e).astype(np.float32), e


def convT_rows(w_iohw: np.ndarray, bias: np.ndarray):
    """build_convT: (cin, cout, 2, 2) -> rows (4 * cout, cin, 1, 1) with row = (dy*2 + dx) * cout + co; scale 1, shift = bias[co]."""
    cin, cout = w_iohw.shape[:2]
    rows = np.ascontiguousarray(np.transpose(np.asarray(w_iohw, np.float32).reshape(cin, cout, 4), (2, 1, 0))).reshape(4 * cout, cin, 1, 1)
    return rows, np.ones(4 * cout, np.float32), np.tile(np.asarray(bias, np.float32), 4)


def pixel_shuffle_rows(y: np.ndarray, cout: int) -> np.ndarray:
    """(n, 4*cout, h, w) in build_convT's row order -> (n, cout, 2h, 2w)."""
    n, _, h, w = y.shape
    return np.ascontiguousarray(np.transpose(y.reshape(n, 2, 2, cout, h, w), (0, 3, 4, 1, 5, 2))).reshape(n, cout, 2 * h, 2 * w)


# ---- reference ----------------------------------------------------------------------------------------------------------------
def _conv64(x, w, stride, pad):
    with torch.no_grad():
        return F.conv2d(torch.from_numpy(np.ascontiguousarray(x, np.float64)), torch.from_numpy(np.ascontiguousarray(w, np.float64)),
                        stride=stride, padding=pad).numpy()


Window = namedtuple("Window", "pre delta lo hi acc absacc scale_eff undecided K ratio")


def _ends(prec, a, b):
    if prec == "f16":
        return rne_f16(a), rne_f16(b)
    if prec == "f16x3":
        return a - (2.0 ** -22 * np.abs(a) + U), b + (2.0 ** -22 * np.abs(b) + U)
    return a, b


def window(prec, pre, delta, relu=False) -> tuple:
    """(lo, hi, undecided): the admissible stored values of an element whose device value lies in [pre - delta, pre + delta]."""
    a, b = pre - delta, pre + delta
    if relu:
        a, b = np.maximum(a, 0.0), np.maximum(b, 0.0)
    lo, hi = _ends(prec, a, b)
    und = (lo != hi) if prec == "f16" else np.zeros(pre.shape, bool)       # f32 / f16x3 ends are an interval by nature
    return lo, hi, und


def conv_window(prec, x, rows, scale, shift, res=None, relu=False, stride=1, exact=True, shuffle_cout=None) -> Window:
    """Window of act(conv(x, rows) * scale + shift (+ res)).  ``rows`` (R, cin, k, k); with ``shuffle_cout`` they are build_convT's rows
    and the result is pixel-shuffled to (n, cout, 2h, 2w).  ``exact`` = the operands are exactly summable: no accumulation term, and
    ``ratio`` is the largest sum|x^||w^| / granule over the output elements (the exactness condition asks for less than 2^24)."""
    k = rows.shape[-1]
    K = int(np.prod(rows.shape[1:]))
    xh = store(prec, x)
    wh, scale_eff, _ = pack_rows(prec, rows, scale)
    pad = (k - 1) // 2
    acc = _conv64(stored_value(xh), stored_value(wh), stride, pad)
    if prec == "f16x3" and np.any(xh[1]) and np.any(wh[1]):
        acc = acc - _conv64(xh[1], wh[1], stride, pad)                     # the product is hi*hi + hi*lo + lo*hi
    absacc = _conv64(sum(np.abs(h) for h in xh), sum(np.abs(h) for h in wh), stride, pad)
    ratio = None
    if exact:
        assert halves_are_normal(xh) and halves_are_normal(wh), "exact-sum data left the normal f16 range"
        ratio = float((absacc / _product_granule(xh, wh, rows.shape[0]).reshape(1, -1, 1, 1)).max())
    sc = scale_eff.astype(np.float64).reshape(1, -1, 1, 1)
    sh = np.asarray(shift, np.float32).astype(np.float64).reshape(1, -1, 1, 1)
    scaled = acc * sc
    pre = scaled + sh
    mag = np.abs(scaled) + np.abs(sh)
    extra = 0.0 if exact else (K + 3) * U * absacc * np.abs(sc)
    if shuffle_cout is not None:
        pre, mag, acc_o, abs_o = (pixel_shuffle_rows(a, shuffle_cout) for a in (pre, mag, acc, absacc))
        if not exact:
            extra = pixel_shuffle_rows(extra, shuffle_cout)
    else:
        acc_o, abs_o = acc, absacc
    if res is not None:
        r = stored_value(store(prec, res))
        pre = pre + r
        mag = mag + np.abs(r)
    delta = 4 * U * mag + extra
    lo, hi, und = window(prec, pre, delta, relu)
    return Window(pre, delta, lo, hi, acc_o, abs_o, scale_eff, und, K, ratio)


def granule(a: np.ndarray, axis=None) -> np.ndarray:
    """Largest power of two that divides every (float32-representable) value of ``a`` along ``axis``; 1.0 where all are zero."""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)
    mi = np.round(np.ldexp(m, 53)).astype(np.int64)                        # exact: a float64 mantissa
    low = mi & -mi                                                         # lowest set bit
    ex = np.where(mi != 0, e - 53 + np.round(np.log2(np.maximum(low, 1))).astype(np.int64), 10 ** 6)
    g = ex.min(axis=axis)
    return np.where(g == 10 ** 6, 1.0, np.ldexp(1.0, np.minimum(g, 1023).astype(np.int64)))


def _product_granule(xh, wh, R):
    """Granule of the products the engine forms, per row: hi*hi, and for split-f16 hi*lo and lo*hi (lo*lo is never formed)."""
    gx = [float(granule(h)) for h in xh]
    gw = [granule(h.reshape(R, -1), axis=1) for h in wh]
    g = gx[0] * gw[0]
    if len(xh) == 2:
        g = np.minimum(g, np.minimum(gx[0] * gw[1], gx[1] * gw[0]))
    return g


# ---- data ---------------------------------------------------------------------------------------------------------------------
def _ints(seed, name, shape, lo, hi):
    n = int(np.prod(shape))
    return ((prng.bits64(seed, name, n) >> np.uint64(33)) % np.uint64(hi - lo + 1)).astype(np.int64).reshape(shape) + lo


def _second_level(seed, name, ints):
    """+-2^-12 on a random half of the non-zero integers."""
    b = prng.bits64(seed, name + "#2", ints.size).reshape(ints.shape)
    on = ((b >> np.uint64(40)) & np.uint64(1)).astype(bool) & (ints != 0)
    sign = np.where(((b >> np.uint64(41)) & np.uint64(1)).astype(bool), 1.0, -1.0)
    return ints.astype(np.float64) + np.where(on, sign * SECOND_LEVEL, 0.0)


def exact_scale_exponent(K: int) -> int:
    """Power of two that keeps max|out| near 8: a row of weights in [-2, 2] (variance 2) on inputs in [-3, 3] (mean square 4) sums to a
    standard deviation of sqrt(8 K); the maximum over a tensor sits near 4.5 of those."""
    return int(np.round(np.log2(8.0 / (4.5 * np.sqrt(8.0 * K)))))


def exact_data(prec, name, x_shape, rows_shape, res_shape=None, seed=41):
    """Exact-sum operands (float32): x, rows (R, cin, k, k), scale (R), shift (R), res or None."""
    R = rows_shape[0]
    K = int(np.prod(rows_shape[1:]))
    xi = _ints(seed, name + "x", x_shape, -3, 3)
    wi = _ints(seed + 1, name + "w", rows_shape, -2, 2)
    two = prec == "f16x3" and K <= SECOND_LEVEL_MAX_K
    x = _second_level(seed, name + "x", xi) if two else xi.astype(np.float64)
    w = _second_level(seed + 1, name + "w", wi) if two else wi.astype(np.float64)
    w = w * np.ldexp(1.0, -(np.arange(R) % 5)).reshape((R,) + (1,) * (len(rows_shape) - 1))
    scale = prng.uniform(seed + 2, name + "s", (R,), 0.5, 1.5).astype(np.float64) * 2.0 ** exact_scale_exponent(K)
    shift = prng.normal(seed + 3, name + "b", (R,), 0.0, 0.1)
    res = None
    if res_shape is not None:
        res = prng.normal(seed + 4, name + "r", res_shape).astype(np.float16).astype(np.float32)
    return x.astype(np.float32), w.astype(np.float32), scale.astype(np.float32), shift.astype(np.float32), res


def normal_data(name, x_shape, rows_shape, res_shape=None, seed=11):
    """The operands of tests/test_gpu_ops.py: test_conv_bn_relu (rounded by the engine's storage, not here)."""
    R = rows_shape[0]
    K = int(np.prod(rows_shape[1:]))
    x = prng.normal(seed, name + "x", x_shape)
    w = prng.normal(seed + 1, name + "w", rows_shape, 0.0, (2.0 / K) ** 0.5)
    scale = prng.uniform(seed + 2, name + "s", (R,), 0.5, 1.5)
    shift = prng.normal(seed + 3, name + "b", (R,), 0.0, 0.1)
    res = prng.normal(seed + 4, name + "r", res_shape) if res_shape is not None else None
    return x, w, scale, shift, res


# ---- the other two ops ----------------------------------------------------------------------------------------------------------
def outc_window(prec, x, w, bias, threshold=0.5):
    """cv_op_outc_1x1 (pointwise.hip: outc_1x1_kernel) on exactly summable data: the input is stored in the engine's type, the weights
    stay float32, logit = acc * 1 + bias in float32 -- one rounding, inside the convolution's delta.  Returns (lo, hi, pre, delta,
    mask, mask_decided): the mask sigmoid(l) > threshold is compared where the logit's window lies clear of the threshold's logit by
    2^-20 / (threshold (1 - threshold)) -- the float32 expression 1 / (1 + __expf(-l)) is good to a few 2^-24 near the threshold and
    the sigmoid's slope there is threshold (1 - threshold)."""
    xs = stored_value(store(prec, x))
    w64 = np.asarray(w, np.float32).astype(np.float64).reshape(1, -1, 1, 1)
    b = float(np.asarray(bias, np.float32).reshape(-1)[0])
    acc = (xs * w64).sum(axis=1, keepdims=True)
    pre = acc + b
    delta = 4 * U * (np.abs(acc) + abs(b))
    t = float(np.log(threshold / (1.0 - threshold)))
    margin = delta + 2.0 ** -20 / (threshold * (1.0 - threshold))
    decided = np.abs(pre - t) > margin
    return pre - delta, pre + delta, pre, delta, (pre > t)[:, 0], decided[:, 0]


def outc_data(prec, name, x_shape, seed=51):
    """Exact-sum operands of the OutConv: inputs as ``exact_data`` makes them (second level for f16x3), integer weights without one --
    the kernel keeps its weights in float32, so a second level there would form the 2^-24 products the exactness condition excludes."""
    x = exact_data(prec, name, x_shape, (1, x_shape[1], 1, 1), seed=seed)[0]
    w = exact_data("f32", name, x_shape, (1, x_shape[1], 1, 1), seed=seed)[1]
    return x, w, prng.normal(seed + 3, name + "b", (1,), 0.0, 0.1)


def outc_exactness(prec, x, w) -> float:
    xh = store(prec, x)
    assert halves_are_normal(xh)
    g = float(min(granule(h) for h in xh)) * float(granule(np.asarray(w, np.float32)))
    return float((sum(np.abs(h) for h in xh) * np.abs(np.asarray(w, np.float64)).reshape(1, -1, 1, 1)).sum(axis=1).max() / g)


def _bilinear_axis(n_in: int, n_out: int):
    """pointwise.hip: bilinear_axis, float32 with contraction off: (i0, i1, l0, l1) per output index."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    f = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = f.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (f - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def bilinear_window(prec, x):
    """cv_op_upsample_bilinear2x, align_corners=True: pre = sum over the four taps of (ly * lx) v^ in float64 with the kernel's float32
    weights.  f32 / f16 (upsample_bilinear2x_kernel): two products, an add, a product and the outer add per path, at most four
    roundings each relative to a partial sum below S = sum|w v| -- delta = 8 * 2^-24 * S covers them twice over.  f16x3
    (upsample_split_emit): the weight ly * lx is rounded once and the eight mixed FMAs (four taps, hi and lo half) round the
    accumulator once each, nine roundings below S -- one more than the two-per-tap count, so delta = 9 * 2^-24 * S for that form.
    Returns (lo, hi, undecided, pre, delta)."""
    v = stored_value(store(prec, x))
    n, c, h, w = v.shape
    y0, y1, ly0, ly1 = _bilinear_axis(h, 2 * h)
    x0, x1, lx0, lx1 = _bilinear_axis(w, 2 * w)
    pre = np.zeros((n, c, 2 * h, 2 * w))
    S = np.zeros_like(pre)
    for yi, ly in ((y0, ly0), (y1, ly1)):
        for xi, lx in ((x0, lx0), (x1, lx1)):
            t = v[:, :, yi][:, :, :, xi] * (ly.reshape(-1, 1) * lx.reshape(1, -1))
            pre += t
            S += np.abs(t)
    delta = (9 if prec == "f16x3" else 8) * U * S
    lo, hi, und = window(prec, pre, delta)
    return lo, hi, und, pre, delta


# ---- checking -----------------------------------------------------------------------------------------------------------------
def outside(got, lo, hi) -> np.ndarray:
    """Elements outside their window (a NaN is outside)."""
    g = np.asarray(got, np.float64)
    return ~((g >= lo) & (g <= hi))


def assert_inside(got, lo, hi, what: str) -> None:
    bad = outside(got, lo, hi)
    if bad.any():
        idx = np.argwhere(bad)
        ch = sorted(set(int(i[1]) for i in idx[:2000]))[:16]
        first = [(tuple(int(v) for v in i), float(np.asarray(got)[tuple(i)]), float(lo[tuple(i)]), float(hi[tuple(i)])) for i in idx[:4]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside their window; first (index, got, lo, hi) {first}; "
                             f"bad channels {ch}")


def margin(got, w: Window, prec, relu=False):
    """Worst |got - act(pre)| / delta over the elements (act is 1-Lipschitz, so the ratio stays below 1 inside the window); for f16x3
    the store term joins the denominator.  None for f16: its store rounding dwarfs delta, the figure there is the undecided share."""
    if prec == "f16":
        return None
    g = np.asarray(got, np.float64)
    pre = np.maximum(w.pre, 0.0) if relu else w.pre
    den = w.delta + (2.0 ** -22 * np.abs(pre) + U if prec == "f16x3" else 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, np.abs(g - pre) / den, 0.0)
    return float(r.max())


# ---- the float32 restatement of the device (CPU tests; the mutants hang off its switches) --------------------------------------------
def _conv32(x, w, stride, pad):
    with torch.no_grad():
        return F.conv2d(torch.from_numpy(np.ascontiguousarray(x, np.float32)), torch.from_numpy(np.ascontiguousarray(w, np.float32)),
                        stride=stride, padding=pad).numpy()


def trunc_f16(v: np.ndarray) -> np.ndarray:
    """MUTANT store: toward zero instead of to nearest even."""
    v = np.asarray(v, np.float32)
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float32)


def device32(prec, x, rows, scale, shift, res=None, relu=False, stride=1, shuffle_cout=None, truncate=False, x_lo_keep=None,
             w_lo_keep=None, acc_edit=None):
    """The device's arithmetic in torch float32: stored operands, float32 accumulation (one convolution per MFMA chain), the float32
    epilogue and the store.  Returns (stored result as float32, float32 accumulator).  The keyword switches are the mutants of
    tests/test_quantised_ref_cpu.py: ``truncate`` (f16 store toward zero), ``x_lo_keep`` / ``w_lo_keep`` (per input channel: False zeroes
    the lo halves of the inputs / weights there), ``acc_edit(acc, xh, wh)`` (edits the accumulator in place)."""
    k = rows.shape[-1]
    pad = (k - 1) // 2
    xh = [h.astype(np.float32) for h in store(prec, x)]
    whs, scale_eff, _ = pack_rows(prec, rows, scale)
    wh = [h.astype(np.float32) for h in whs]
    acc = _conv32(xh[0], wh[0], stride, pad)
    if prec == "f16x3":
        if x_lo_keep is not None:
            xh[1] = xh[1] * np.asarray(x_lo_keep, np.float32).reshape(1, -1, 1, 1)
        if w_lo_keep is not None:
            wh[1] = wh[1] * np.asarray(w_lo_keep, np.float32).reshape(1, -1, 1, 1)
        acc = acc + _conv32(xh[0], wh[1], stride, pad) + _conv32(xh[1], wh[0], stride, pad)
    if acc_edit is not None:
        acc_edit(acc, xh, wh)
    v = (acc * scale_eff.reshape(1, -1, 1, 1)).astype(np.float32) + np.asarray(shift, np.float32).reshape(1, -1, 1, 1)
    acc_o = acc
    if shuffle_cout is not None:
        v, acc_o = pixel_shuffle_rows(v, shuffle_cout), pixel_shuffle_rows(acc, shuffle_cout)
    if res is not None:
        v = v + stored_value(store(prec, res)).astype(np.float32)
    if relu:
        v = np.maximum(v, np.float32(0))
    v = v.astype(np.float32)
    if prec == "f16":
        v = trunc_f16(v) if truncate else v.astype(np.float16).astype(np.float32)
    elif prec == "f16x3":
        v = stored_value(store(prec, v)).astype(np.float32)
    return v, acc_o

"""``threshold_levels_kernel`` through ``HipEngine.threshold_levels``: exact equality with the numpy form
(``evaluation.threshold_levels``) on logits that keep a stated distance from every threshold, equality with the device's own fused
masks and with ``segmentation_scores``' counts on real UNet logits, run-to-run identity, and the argument errors of the C entry."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
import torch

from chessvision import ChessVision, evaluation, hip_backend, synthetic

pytestmark = pytest.mark.gpu

GRIDS = {1: [0.5], 2: [0.3, 0.7], 9: list(np.linspace(0.1, 0.9, 9)), 32: list(np.linspace(0.0, 1.0, 32))}
COUNTS = [1, 3, 4, 5, 63, 1021, 65536]                       # empty body, head and tail only, one piece, odd sizes, the real size
GAP = 1e-3                                                   # every sigmoid stays this far from every threshold: a condition, not a tolerance


def _logits_clear_of(rng, shape, thr):
    """logit(p) as float32, p uniform but redrawn until it is 1.1 * GAP away from every threshold and inside [1e-12, 1 - 1e-12]
    (|logit| < 28); then a few +-inf and NaN.  Returns the logits and the mask of the finite ones."""
    thr = np.asarray(thr, np.float64)
    p = rng.random(shape)
    for _ in range(64):
        bad = (np.abs(p[..., None] - thr).min(axis=-1) < 1.1 * GAP) | (p < 1e-12) | (p > 1 - 1e-12)
        if not bad.any():
            break
        p[bad] = rng.random(int(bad.sum()))
    assert not bad.any()
    x = np.log(p / (1.0 - p)).astype(np.float32)
    assert np.abs(x).max() <= 30
    flat = x.reshape(-1)
    if flat.size >= 3:
        flat[0], flat[flat.size // 2], flat[-1] = np.inf, np.nan, -np.inf
    return x, np.isfinite(x)


def _run(eng, x, thr, labels, offset):
    """One launch on buffers that start ``offset`` floats / one byte into their allocations -> (levels, records) as numpy."""
    n, count = x.shape
    base = torch.empty(n * count + offset, dtype=torch.float32, device=eng.device)
    lg = base[offset:].view(n, count)
    lg.copy_(torch.from_numpy(x))
    lb = None
    if labels is not None:
        lbase = torch.empty(n * count + 1, dtype=torch.uint8, device=eng.device)
        lb = lbase[1:].view(n, count)
        lb.copy_(torch.from_numpy(labels))
    return eng.threshold_levels(lg, thr, lb)


@pytest.mark.parametrize("count", COUNTS)
def test_kernel_equals_the_numpy_form(engines, count):
    eng = engines["f32"]
    rng = np.random.default_rng(1000 + count)
    offsets = iter([1, 2, 3] * 4)
    for n in (1, 3):
        for T, thr in GRIDS.items():
            thr32 = np.asarray(thr, np.float32)
            x, finite = _logits_clear_of(rng, (n, count), thr32)
            with np.errstate(over="ignore"):
                v = np.float32(1) / (np.float32(1) + np.exp(-x[finite]))
            assert v.size == 0 or np.abs(v[:, None].astype(np.float64) - thr32.astype(np.float64)).min() >= GAP   # no pixel to excuse
            labels = np.array([0, 1, 7, 255], np.uint8)[rng.integers(0, 4, (n, count))]
            offset = next(offsets)
            for lab in (labels, None):
                want_levels, want_hist, want_nan = evaluation.threshold_levels(x, thr32, lab)
                levels, rec = _run(eng, x, thr32, lab, offset)
                assert levels.shape == (n, count) and levels.dtype == np.uint8 and rec.shape == (n,)
                assert np.array_equal(levels, want_levels), (n, T, offset, lab is None)
                assert np.array_equal(rec["hist"], want_hist), (n, T, offset, lab is None)
                assert np.array_equal(rec["n_nan"], want_nan) and (rec["count"] == count).all() and (rec["n_thresholds"] == T).all()
                assert not rec["reserved"].any()
                assert levels.max() <= T and rec["hist"].sum() == n * count


def test_records_and_levels_are_identical_run_to_run(engines):
    eng = engines["f32"]
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.normal(0, 2, (5, 65536)).astype(np.float32)).to(eng.device)
    lab = torch.from_numpy(np.where(rng.random((5, 65536)) < 0.4, 255, 0).astype(np.uint8)).to(eng.device)
    first = eng.threshold_levels(x, GRIDS[9], lab)
    for _ in range(2):
        again = eng.threshold_levels(x, GRIDS[9], lab)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


def test_argument_errors(engines):
    eng = engines["f32"]
    lib = eng._lib
    x = torch.zeros(4, 16, dtype=torch.float32, device=eng.device)
    lab = torch.zeros(4, 16, dtype=torch.uint8, device=eng.device)
    lev = torch.zeros(4, 16, dtype=torch.uint8, device=eng.device)
    rec = torch.zeros(4, 320, dtype=torch.uint8, device=eng.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    X, L, V, R = x.data_ptr(), lab.data_ptr(), lev.data_ptr(), rec.data_ptr()

    def grid(*values):
        return (ctypes.c_float * max(1, len(values)))(*values)

    ok = grid(0.3, 0.7)
    cases = {
        "null logits": (eng._h, None, L, 4, 16, ok, 2, V, R),
        "null thresholds": (eng._h, X, L, 4, 16, None, 2, V, R),
        "null levels": (eng._h, X, L, 4, 16, ok, 2, None, R),
        "null records": (eng._h, X, L, 4, 16, ok, 2, V, None),
        "n = 0": (eng._h, X, L, 0, 16, ok, 2, V, R),
        "count = 0": (eng._h, X, L, 4, 0, ok, 2, V, R),
        "count too large": (eng._h, X, L, 1, (1 << 24) + 1, ok, 2, V, R),
        "no thresholds": (eng._h, X, L, 4, 16, ok, 0, V, R),
        "33 thresholds": (eng._h, X, L, 4, 16, grid(*np.linspace(0, 1, 33)), 33, V, R),
        "NaN threshold": (eng._h, X, L, 4, 16, grid(0.3, math.nan), 2, V, R),
        "negative threshold": (eng._h, X, L, 4, 16, grid(-0.1, 0.5), 2, V, R),
        "threshold above 1": (eng._h, X, L, 4, 16, grid(0.5, 1.5), 2, V, R),
        "equal thresholds": (eng._h, X, L, 4, 16, grid(0.5, 0.5), 2, V, R),
        "equal as float32": (eng._h, X, L, 4, 16, grid(0.5, 0.5 + 1e-9), 2, V, R),
        "descending": (eng._h, X, L, 4, 16, grid(0.7, 0.3), 2, V, R),
        "misaligned logits": (eng._h, X + 2, L, 4, 15, ok, 2, V, R),
    }
    for name, args in cases.items():
        assert lib.cv_threshold_levels(*args, stream) == 1, name                             # CV_ERR_INVALID
        assert b"cv_threshold_levels" in lib.cv_last_error(), name
    assert lib.cv_threshold_levels(None, X, L, 4, 16, ok, 2, V, R, stream) == 1              # null engine
    for bad in ([], [0.5, 0.5], [0.7, 0.3], [math.nan], [-0.1], list(np.linspace(0, 1, 33))):
        with pytest.raises(hip_backend.HipBackendError):
            eng.threshold_levels_dev(x, bad, lab)
    with pytest.raises(hip_backend.HipBackendError):
        eng.threshold_levels_dev(x, [0.5], lab[:, :15])
    with pytest.raises(hip_backend.HipBackendError):
        eng.threshold_levels_dev(x.cpu(), [0.5])
    with pytest.raises(hip_backend.HipBackendError):
        eng.threshold_levels_dev(x.t(), [0.5])                                               # not contiguous
    torch.cuda.synchronize(eng.device)
    assert not rec.cpu().numpy().any() and not lev.cpu().numpy().any()                       # nothing was launched
    assert lib.cv_threshold_levels(eng._h, X, None, 4, 16, ok, 2, V, R, stream) == 0         # labels may be null
    torch.cuda.synchronize(eng.device)
    got = rec.cpu().numpy().view(hip_backend.LEVEL_RECORD).reshape(-1)
    assert (got["hist"][:, 0, 1] == 16).all() and got["hist"].sum() == 64                    # sigmoid(0) = 0.5: above 0.3 only


# ---- against the device's own masks ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cv_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("weights_threshold_levels")
    pe, pc = synthetic.save_checkpoints(d, segmenting=True)
    return ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))


def test_levels_are_the_fused_masks_of_the_unet(cv_model):
    _ = cv_model.board_extractor
    eng = cv_model._get_engine("unet")
    grid = [0.0, 0.3, 0.5, 0.7, 1.0]
    photos = torch.from_numpy(np.stack([synthetic.board_photo(60 + s) for s in range(8)])).to(eng.device)
    small = eng.resize_area_u8(photos, (256, 256))
    labels = (torch.rand(8, 256, 256, device=eng.device) < 0.5).to(torch.uint8)
    logits, _ = eng.unet_forward_u8(small, want_mask=False)
    levels, rec = eng.threshold_levels(logits, grid, labels)
    levels = levels.reshape(8, 256, 256)
    n_label, n_pred, n_both = evaluation.level_counts(rec["hist"], len(grid))
    for k, t in enumerate(grid):
        again, mask = eng.unet_forward_u8(small, threshold=t)
        assert torch.equal(again, logits)
        assert np.array_equal(np.where(levels > k, 255, 0).astype(np.uint8), mask.cpu().numpy()), t   # byte for byte
        seg, _ = eng.segmentation_scores(logits, labels, t)
        assert np.array_equal(seg["n_pred"], n_pred[:, k]) and np.array_equal(seg["n_both"], n_both[:, k]), t
        assert np.array_equal(seg["n_label"], n_label)
    assert 0 < n_pred[:, 2].min() and n_pred[:, 2].max() < 65536                             # at 0.5: a real mask
    assert (n_pred[:, 4] == 0).all()                                                         # nothing is above 1

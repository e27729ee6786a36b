"""No GPU: the host form of the antialiased bilinear resize (``classical.resize_antialias``, the checker of the device kernel) against
the real implementation -- ``torch.nn.functional.interpolate(..., mode="bilinear", antialias=True)`` on the CPU, cases and bar in
tests/antialias_ref.py --, and the plumbing of the ``resize`` mode: symbols, signatures, validation, and which engine calls a job of
the batched pipeline issues in either mode (recorder engines, in the style of tests/test_batched_pipeline_cpu.py)."""
from __future__ import annotations

import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import antialias_ref as aref
from chessvision import ChessVision, batched, classical, constants, hip_backend

ROOT = Path(__file__).resolve().parent.parent


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", aref.CASES, ids=aref.case_id)
def test_host_form_matches_torch(case):
    h, w, n, c = case
    batch = aref.images(case)[:1]                          # the host form is per image: one of the batch is enough here
    want = aref.torch_resize(batch)[0]
    got = classical.resize_antialias(batch[0], (aref.OUT, aref.OUT))
    assert got.shape == (c, aref.OUT, aref.OUT) and got.dtype == np.float32 and got.flags.c_contiguous
    err, bar = float(np.abs(got.astype(np.float64) - want).max()), aref.bar(h, w)
    print(f"AA host {aref.case_id(case)}: err {err:.3e} bar {bar:.3e}")
    if (h, w) == (aref.OUT, aref.OUT):
        assert np.array_equal(got, want)
    assert err <= bar, (case, err, bar)


def test_bar_is_the_derived_one():
    assert aref.bar(512, 512) == pytest.approx(2.0 ** -24 * 16) and aref.bar(512, 512) == pytest.approx(9.5e-7, rel=0.01)
    assert aref.bar(1536, 2048) == 2.0 ** -24 * (16 + 12 + 8)
    assert aref.bar(16, 16) == 2.0 ** -24 * (2 + 2 + 8)


def test_equal_sizes_are_the_identity():
    img = np.random.default_rng(3).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    got = classical.resize_antialias(img, (256, 256))
    assert np.array_equal(got, (img.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))


def test_constant_images_and_gray_input():
    for h, w in ((300, 400), (16, 16), (1536, 2048)):
        bar = aref.bar(h, w)
        white = classical.resize_antialias(np.full((h, w, 3), 255, np.uint8), (256, 256))
        assert white.max() <= 1 + bar and white.min() >= 1 - bar
        assert not classical.resize_antialias(np.zeros((h, w, 3), np.uint8), (256, 256)).any()
    gray = np.random.default_rng(5).integers(0, 256, (300, 400), dtype=np.uint8)
    assert np.array_equal(classical.resize_antialias(gray, (256, 256)), classical.resize_antialias(gray[:, :, None], (256, 256)))
    wide = classical.resize_antialias(gray, (100, 50))     # size is (width, height), as for resize_area
    assert wide.shape == (1, 50, 100)


def test_taps_follow_the_formulas():
    first, count, weights = classical.antialias_taps(512, 256)
    assert count.max() == 4 and weights.shape == (256, 4) and weights.dtype == np.float32
    assert first[0] == 0 and count[0] == 3 and first[1] == 1 and count[1] == 4      # the first output is cut at the border
    assert np.allclose(weights[1], [0.125, 0.375, 0.375, 0.125]) and np.allclose(weights.sum(axis=1), 1.0, atol=1e-6)
    first, count, weights = classical.antialias_taps(2048, 256)
    assert count.max() == 16
    first, count, weights = classical.antialias_taps(16, 256)                        # enlarging: plain two-tap bilinear
    assert count.max() == 2 and (first + count <= 16).all()
    first, count, weights = classical.antialias_taps(256, 256)
    assert np.array_equal(first, np.arange(256)) and np.array_equal(weights[:, 0], np.ones(256, np.float32)) and not weights[:, 1:].any()


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "chessvision_hip.h").read_text(), flags=re.S)
    bound = {name: args for name, _, args in hip_backend.SYMBOLS}
    lib = hip_backend.load_library()
    for sym, n_args in (("cv_resize_antialias_f32", 10), ("cv_unet_forward_mask", 8)):
        assert re.search(rf"\bint {sym}\s*\(", header), sym
        assert len(bound[sym]) == n_args and hasattr(lib, sym), sym
    assert lib.cv_abi_version() == hip_backend.ABI_VERSION == 6
    assert lib.cv_resize_antialias_f32(None, None, 1, 2, 2, 3, None, 2, 2, None) != 0 and b"null engine" in lib.cv_last_error()
    assert lib.cv_unet_forward_mask(None, None, 1, None, None, 0.5, None, None) != 0 and b"null engine" in lib.cv_last_error()
    for method in ("resize_antialias_f32", "unet_forward_mask"):
        assert callable(getattr(hip_backend.HipEngine, method))
    sig = inspect.signature(hip_backend.HipEngine.unet_forward_mask)
    assert list(sig.parameters) == list(inspect.signature(hip_backend.HipEngine.unet_forward_u8).parameters)[:1] + ["x", "threshold", "want_mask", "want_embedding"]
    assert inspect.signature(hip_backend.HipEngine.resize_antialias_f32).parameters["out_hw"].default == (256, 256)


def test_process_images_signature_and_defaults():
    params = inspect.signature(ChessVision.process_images).parameters
    names = list(params)
    assert params["resize"].default == "area" and names[-1] == "quality"
    assert names.index("resize") == names.index("embeddings") - 1 == names.index("last_job") + 1
    assert ChessVision.evaluation_resize == "area"
    assert "resize" not in inspect.signature(ChessVision.evaluate_images).parameters
    assert inspect.signature(batched.process_images).parameters["resize"].default == "area"
    assert inspect.signature(batched._Call.__init__).parameters["resize"].default == "area"


def test_a_bad_mode_raises_before_anything_is_launched():
    cv = ChessVision()                                     # lazy: no engine, no model, no device work
    img = np.zeros((512, 512, 3), np.uint8)
    for bad in ("bilinear", "AREA", None, ""):
        with pytest.raises(ValueError, match="resize"):
            cv.process_images([img], resize=bad)
    cv.evaluation_resize = "lanczos"
    with pytest.raises(ValueError, match="resize"):
        cv.evaluate_images([img], true_fens=["8/8/8/8/8/8/8/8"])
    with pytest.raises(ValueError, match="resize"):
        batched.process_images(cv, [img], 0.5, False, False, 64, True, None, 16, 0, None, resize="cubic")
    assert cv._engines == {} and cv._board_extractor is None and cv._streams is None


class _Engine:
    """Notes every call and hands back what the real method would, as a label."""

    def __init__(self):
        self.log = []

    def _note(self, name, arg, *rest, **kw):
        self.log.append((name, arg, rest, kw))

    def resize_area_u8(self, images, out_hw):
        self._note("resize_area_u8", images, out_hw)
        return "bytes 256"

    def resize_antialias_f32(self, images, out_hw):
        self._note("resize_antialias_f32", images, out_hw)
        return "floats 256"

    def _unet(self, name, x, **kw):
        self._note(name, x, **kw)
        return ("logits", "mask", "embedding") if kw.get("want_embedding") else ("logits", "mask")

    def unet_forward_u8(self, x, **kw):
        return self._unet("unet_forward_u8", x, **kw)

    def unet_forward_mask(self, x, **kw):
        return self._unet("unet_forward_mask", x, **kw)


class _ForwardOnly(batched._Call):
    def __init__(self, resize, embeddings):
        self.eng, self.resize, self.embeddings, self.threshold, self.timed = _Engine(), resize, embeddings, 0.4, False


SIZE = (constants.INPUT_SIZE[1], constants.INPUT_SIZE[0])


@pytest.mark.parametrize("embeddings", [False, True])
def test_area_issues_exactly_the_call_sequence_it_always_did(embeddings):
    call = _ForwardOnly("area", embeddings)
    out = call.forward("photos")
    kw = dict(threshold=0.4, want_mask=True, **({"want_embedding": True} if embeddings else {}))
    assert call.eng.log == [("resize_area_u8", "photos", (SIZE,), {}), ("unet_forward_u8", "bytes 256", (), kw)]
    assert out == ("logits", "mask", "embedding" if embeddings else None)


@pytest.mark.parametrize("embeddings", [False, True])
def test_antialias_issues_the_float_resize_then_the_float_entry(embeddings):
    call = _ForwardOnly("antialias", embeddings)
    out = call.forward("photos")
    kw = dict(threshold=0.4, want_mask=True, **({"want_embedding": True} if embeddings else {}))
    assert call.eng.log == [("resize_antialias_f32", "photos", (SIZE,), {}), ("unet_forward_mask", "floats 256", (), kw)]
    assert out == ("logits", "mask", "embedding" if embeddings else None)


@pytest.mark.parametrize("embeddings", [False, True])
@pytest.mark.parametrize("resize, calls", [("area", ("resize_area_u8", "bytes 256", "unet_forward_u8")),
                                           ("antialias", ("resize_antialias_f32", "floats 256", "unet_forward_mask"))])
def test_a_maskless_forward_is_the_threshold_sweeps_call_sequence(resize, calls, embeddings):
    """``forward(batch, want_mask=False)``: the same two engine calls; the UNet entry is told to leave the mask out and is always
    told whether to pool the embedding."""
    call = _ForwardOnly(resize, embeddings)
    out = call.forward("photos", want_mask=False)
    kw = dict(threshold=0.4, want_mask=False, want_embedding=embeddings)
    assert call.eng.log == [(calls[0], "photos", (SIZE,), {}), (calls[2], calls[1], (), kw)]
    assert out[0] == "logits" and out[2] == ("embedding" if embeddings else None) and len(out) == 3


def test_the_mode_reaches_the_call_from_both_public_methods():
    """``process_images`` and ``evaluate_images`` hand the mode to ``_process_images_native`` as the last positional argument, where
    the repeat on the exact-f32 instance (``_recover``) finds it too: the lambda is the same for both runs."""
    seen = []

    class _Probe(ChessVision):
        def _process_images_native(self, *args):
            seen.append(args)
            return []

    cv = _Probe()
    img = np.zeros((8, 8, 3), np.uint8)
    cv.process_images([img])
    cv.process_images([img], resize="antialias", embeddings=True, quality="sigmoid")
    assert seen[0][-1] == "area" and seen[0][-2] is False and len(seen[0]) == 13
    assert seen[1][-1] == "antialias" and seen[1][-2] is True and seen[1][9] == "sigmoid"
    cv.evaluation_resize = "antialias"
    try:
        cv.evaluate_images([img], true_fens=["8/8/8/8/8/8/8/8"])
    except Exception:                                      # the probe returns no results for the report to read
        pass
    assert seen[2][-1] == "antialias"

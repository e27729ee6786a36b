"""Board-extraction quality scores on the device: the score kernel through ``HipEngine.extraction_scores`` against the numpy oracle
``tests/quality_ref.py``, its argument errors, and ``ChessVision.process_images(quality=...)`` end to end."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
import torch

import quality_ref
from chessvision import ChessVision, hip_backend, quality, synthetic
from oracle import contours_c

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4), (3, 1000), (2, 4099), (5, 65536), (2, 65536 + 4)]
F32_LITERAL_REL = 32 * 2.0 ** -24          # pairwise float32 summation of <= 16384 + a few terms: the literal's own error bound
EDGES = np.arange(1, 10) / 10.0            # the inner bin edges (0 and 1 bound the range from inside: nothing is borderline there)


def _neighbours():
    out = []
    for e in [i / 10 for i in range(11)] + [0.5]:
        lo = hi = np.float32(e)
        out.append(lo)
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
            out += [lo, hi]
    return np.array(out, dtype=np.float32)


def _two_valued(rng, n, count, inside):
    """high value on `nh` shuffled positions: 0 < nh < k puts the value change strictly inside the top quarter, nh > k strictly
    outside it (count = 4 has k = 1 and no room inside: the change then sits on the boundary)."""
    k = count // 4
    nh = max(1, k // 2) if inside else k + max(1, (count - k) // 2)
    a = np.full((n, count), 0.2, np.float32)
    for i in range(n):
        a[i, rng.permutation(count)[:nh]] = np.float32(0.9 + 0.01 * i)
    return a


def _special(rng, n, count):
    pool = np.array([0.0, -0.0, np.inf, -np.inf, 0.25, 0.75, -3.0, 1.0], np.float32)
    return pool[rng.integers(0, len(pool), (n, count))]


def _with_nan(rng, n, count):
    a = rng.normal(0, 6, (n, count)).astype(np.float32)
    a[0, count // 3] = np.nan
    return a


def _edges(rng, n, count):
    a = rng.random((n, count)).astype(np.float32)
    nb = _neighbours()
    m = min(count, len(nb))
    a[:, :m] = nb[:m]
    return a


INPUTS = {
    "normal": lambda rng, n, c: rng.normal(0, 6, (n, c)).astype(np.float32),
    "uniform_and_edge_neighbours": _edges,
    "constant": lambda rng, n, c: np.repeat(np.array([0.7, 0.5, -1.0, 0.0, 1.0], np.float32)[:n, None], c, axis=1),
    "two_valued_change_inside_top_quarter": lambda rng, n, c: _two_valued(rng, n, c, True),
    "two_valued_change_outside_top_quarter": lambda rng, n, c: _two_valued(rng, n, c, False),
    "all_negative": lambda rng, n, c: (-5 * rng.random((n, c)) - 0.1).astype(np.float32),
    "zeros_and_infinities": _special,
    "one_nan": _with_nan,
}


def _same(a: float, b: float, rel: float = 0.0, abs_: float = 0.0) -> bool:
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= max(abs_, rel * abs(b))


def _on_device(engine, host: np.ndarray, misaligned: bool) -> torch.Tensor:
    n, count = host.shape
    if not misaligned:
        return torch.from_numpy(host).to(engine.device)
    base = torch.empty(n * count + 1, dtype=torch.float32, device=engine.device)
    view = base[1:].view(n, count)                             # contiguous, image 0 starts 4 bytes past a 16-byte boundary
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 16 == 4
    return view


def _check_against_oracle(engine, host: np.ndarray, misaligned: bool = False):
    n, count = host.shape
    dev = _on_device(engine, host, misaligned)
    rec, conf, dist, mask = engine.extraction_scores(dev, transform="none", want_mask=True)
    rec2, conf2, dist2 = engine.extraction_scores(dev, transform="none")
    assert rec.tobytes() == rec2.tobytes()                       # bit-identical run to run, with and without the mask output
    assert rec.shape == (n,) and mask.shape == (n, count) and mask.dtype == np.uint8
    for i in range(n):
        v = host[i]
        with np.errstate(invalid="ignore"):
            assert np.array_equal(rec["hist"][i], quality_ref.histogram10(v)), (i, rec["hist"][i], quality_ref.histogram10(v))
            assert rec["above_half"][i] == np.count_nonzero(v > 0.5)
            assert np.array_equal(mask[i], np.where(v > 0.5, 255, 0).astype(np.uint8))
            assert rec["n_nan"][i] == np.count_nonzero(np.isnan(v))
            assert rec["above_half"][i] == np.count_nonzero(mask[i])
            assert rec["top_count"][i] == count // 4
            want64, want32 = quality_ref.probability_confidence_f64(v), quality_ref.probability_confidence(v)
            want_dist = quality_ref.probability_distribution(v)
        assert _same(conf[i], want64, rel=1e-9), (i, conf[i], want64)
        assert _same(conf[i], want32, rel=F32_LITERAL_REL), (i, conf[i], want32)
        assert _same(dist[i], want_dist, abs_=1e-12), (i, dist[i], want_dist)
        if np.isnan(v).any():
            assert math.isnan(conf[i])


@pytest.mark.parametrize("kind", list(INPUTS))
def test_kernel_matches_the_oracle(engines, kind):
    rng = np.random.default_rng(sorted(INPUTS).index(kind))
    for n, count in SHAPES:
        _check_against_oracle(engines["f32"], INPUTS[kind](rng, n, count))


def test_kernel_on_images_that_are_not_16_byte_aligned(engines):
    rng = np.random.default_rng(99)
    for n, count in [(3, 1000), (2, 4099), (2, 65536 + 4)]:
        _check_against_oracle(engines["f32"], INPUTS["uniform_and_edge_neighbours"](rng, n, count), misaligned=True)
        _check_against_oracle(engines["f32"], INPUTS["normal"](rng, n, count), misaligned=True)


def _clear_logits(rng, shape):
    """normal(0, 4) logits, none of whose float64 sigmoid lies within 1e-4 of a bin edge or of 0.5: the oracle has no borderline
    element, whatever the last bits of the device's exp."""
    x = rng.normal(0, 4, shape).astype(np.float32)
    while True:
        s = quality_ref.sigmoid64(x)
        near = (np.abs(s[..., None] - EDGES).min(axis=-1) < 1e-4)
        if not near.any():
            return x
        x[near] = rng.normal(0, 4, int(near.sum())).astype(np.float32)


def test_sigmoid_transform_matches_the_oracle_and_the_pipeline_mask(engines):
    """confidence bar 1e-5 absolute (not derived: it assumes __expf errs by well under 1e-6 on values <= 1).
    Observed on MI355X: see OBSERVED_SIGMOID_CONFIDENCE_ERROR below."""
    eng = engines["f32"]
    rng = np.random.default_rng(17)
    worst = 0.0
    for n, count in [(5, 65536), (2, 4099)]:
        x = _clear_logits(rng, (n, count))
        dev = torch.from_numpy(x).to(eng.device)
        rec, conf, dist, mask = eng.extraction_scores(dev, transform="sigmoid", want_mask=True)
        s = quality_ref.sigmoid64(x)
        for i in range(n):
            assert np.array_equal(rec["hist"][i], quality_ref.histogram10(s[i]))
            assert rec["above_half"][i] == np.count_nonzero(s[i] > 0.5) == np.count_nonzero(mask[i])
            assert rec["n_nan"][i] == 0 and rec["top_count"][i] == count // 4
            want = quality_ref.probability_confidence_f64(s[i])
            err = abs(conf[i] - want)
            print(f"sigmoid confidence error n={n} count={count} image {i}: {err:.3e}")
            worst = max(worst, err)
            assert err <= 1e-5, (conf[i], want)
            assert _same(dist[i], quality_ref.probability_distribution(s[i]), abs_=1e-12)
        if count == 65536:                                     # the mask the UNet path thresholds with, for the same logits
            _, pipeline_mask = eng.op_outc_1x1(dev.view(n, 1, 256, 256), np.ones(1, np.float32), np.zeros(1, np.float32), threshold=0.5)
            assert np.array_equal(mask.reshape(n, 256, 256), pipeline_mask.cpu().numpy())
    print(f"sigmoid confidence error, maximum: {worst:.3e}")


OBSERVED_SIGMOID_CONFIDENCE_ERROR = "not yet measured"


def test_argument_errors(engines):
    eng = engines["f32"]
    lib = eng._lib
    x = torch.zeros(4, 16, dtype=torch.float32, device=eng.device)
    rec = torch.zeros(4, 64, dtype=torch.uint8, device=eng.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    cases = {
        "count = 3": (x.data_ptr(), 4, 3, 0, rec.data_ptr()),
        "n = 0": (x.data_ptr(), 0, 16, 0, rec.data_ptr()),
        "null records": (x.data_ptr(), 4, 16, 0, None),
        "unknown transform": (x.data_ptr(), 4, 16, 2, rec.data_ptr()),
    }
    for name, (values, n, count, transform, records) in cases.items():
        status = lib.cv_extraction_scores(eng._h, values, n, count, transform, records, None, stream)
        assert status == 1, name                                 # CV_ERR_INVALID
        assert b"cv_extraction_scores" in lib.cv_last_error(), name
    with pytest.raises(hip_backend.HipBackendError):
        eng.extraction_scores(x, transform="softmax")
    with pytest.raises(hip_backend.HipBackendError):
        eng.extraction_scores(x[:, :3])                          # count = 3 through the Python layer
    torch.cuda.synchronize(eng.device)
    assert not rec.cpu().numpy().any()                           # nothing was launched


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipeline_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("weights_quality")
    pe, pc = synthetic.save_checkpoints(d, segmenting=True)
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))
    images = [synthetic.board_photo(300 + s) for s in range(6)]
    images[3] = np.random.default_rng(1003).integers(0, 60, (512, 512, 3), dtype=np.uint8)      # no board: fallback quadrangle
    runs, timings = {}, {}
    for mode in (None, "again", "logits", "sigmoid"):
        timings[mode] = {}
        res = cv.process_images(images, fallback_quad=True, pipeline_chunk=4, timings=timings[mode],     # jobs of 4 and 2 boards
                                quality=None if mode == "again" else mode)
        runs[mode] = res
    return runs, timings


def _bytes(res):
    e = res.board_extraction
    return (res.position.fen if res.position else None, e.binary_mask.tobytes(), e.probabilities.tobytes(),
            None if e.board_image is None else e.board_image.tobytes(), None if e.quadrangle is None else e.quadrangle.tobytes())


def test_pipeline_without_quality_is_unchanged(pipeline_runs):
    runs, timings = pipeline_runs
    assert all(r.quality is None for r in runs[None])
    assert [_bytes(r) for r in runs[None]] == [_bytes(r) for r in runs["again"]]
    assert "quality" not in timings[None] and "quality_ms" not in timings[None]


@pytest.mark.parametrize("mode", ["logits", "sigmoid"])
def test_pipeline_quality_matches_the_oracle(pipeline_runs, mode):
    runs, timings = pipeline_runs
    assert [_bytes(r) for r in runs[mode]] == [_bytes(r) for r in runs[None]]
    assert timings[mode]["quality"] > 0 and timings[mode]["quality_ms"] > 0
    found_from_mask = 0
    for r in runs[mode]:
        q, e = r.quality, r.board_extraction
        assert all(type(v) is float for v in (q.confidence, q.quad_score, q.completeness, q.distribution))
        logits = e.probabilities
        n_values = logits.size
        quad = contours_c.find_quadrangle(e.binary_mask)
        found_from_mask += quad is not None
        want_quad = quality_ref.quadrangle_regularity(None if quad is None else quad.astype(np.float32))
        assert _same(q.quad_score, want_quad, abs_=1e-5), (q.quad_score, want_quad)
        host = quality.extraction_quality(e, of=mode)
        assert _same(host.quad_score, q.quad_score, abs_=1e-12)
        if mode == "logits":
            assert _same(q.confidence, quality_ref.probability_confidence_f64(logits), rel=1e-9)
            assert _same(q.confidence, quality_ref.probability_confidence(logits), rel=F32_LITERAL_REL)
            assert _same(q.distribution, quality_ref.probability_distribution(logits), abs_=1e-12)
            assert _same(q.completeness, quality_ref.mask_completeness(logits), rel=1e-12)
            assert _same(host.confidence, q.confidence, rel=F32_LITERAL_REL) and _same(host.distribution, q.distribution, abs_=1e-12)
            assert _same(host.completeness, q.completeness, rel=1e-12)
        else:
            s = quality_ref.sigmoid64(logits)
            assert _same(q.confidence, quality_ref.probability_confidence_f64(s), abs_=1e-5)
            # These logits cannot be resampled.  An element whose sigmoid lies within 1e-6 of an edge (the assumed bound on the
            # device's exp) may sit in the neighbouring bin; moving ONE of N elements between two bins changes the entropy by at most
            # |log2((p_i + 1e-10) / (p_j + 1e-10))| / N <= (log2(1e10) + 1.5) / N, i.e. the score by at most 11 / N.
            borderline = int(np.count_nonzero(np.abs(s[..., None] - EDGES).min(axis=-1) < 1e-6))
            bar = 1e-12 + 11.0 * borderline / n_values
            assert _same(q.distribution, quality_ref.probability_distribution(s), abs_=bar), (q.distribution, borderline)
            # the result's own mask (threshold 0.5) is the binarisation the kernel scored: the same expression, bit for bit
            assert _same(q.completeness, quality_ref.mask_completeness_binary(e.binary_mask)[0], rel=1e-12)
            assert _same(host.confidence, q.confidence, abs_=1e-5) and _same(host.distribution, q.distribution, abs_=bar)
            if not np.count_nonzero(np.abs(s - 0.5) < 1e-6):
                assert _same(host.completeness, q.completeness, rel=1e-12)
    assert found_from_mask >= 4                                  # the synthetic boards are found; the noise image is not

"""GPU: square-set evaluation -- the normalised byte input of the two stem kernels (bit for bit ToTensor + Normalize), the graph key,
the records kernel against its host form and float64, parity of the normalised forward against the torch-CPU oracle on real squares,
and ``ChessVision.evaluate_squares`` end to end.

Bars.  Transform, graph key, existing entry: bit equality.  Records: integer fields equal with no exclusions (comparisons of the same
float32 values), floats within 2^-21 (1 + max|x|) of float64 (squares_ref.bound).  Oracle parity of the logits: the project's 1e-3 for
f32 and f16x3; f16r and f16 are measured and printed only -- nobody had measured those engines on inputs outside [0, 1]; the figures
are in profiles/evaluate_squares.md.  End to end: 2e-3 on loss and confidence (1e-3 on each of two logits); predicted and rank on the
rows whose smallest gap between sorted oracle logits is at least 2e-3 (at most 6 of 130 rows may fall out).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import squares_ref as sr
from chessvision import ChessVision, constants, evaluation, hip_backend
from oracle import synth

pytestmark = pytest.mark.gpu

TRAIN = constants.CLASSIFIER_NORMALIZATION
PAIRS = (TRAIN, (0.3, 1.7))


def _sd(seed):
    return {k: v for k, v in synth.make_resnet(seed).state_dict().items() if not k.endswith("num_batches_tracked")}


_ENGINES = {}


@pytest.fixture(scope="module")
def engine():
    """engine(precision, seed=2, chunk=0): engines of this module, loaded once each and closed at the end."""
    def get(prec, seed=2, chunk=0):
        key = (prec, seed, chunk)
        if key not in _ENGINES:
            eng = hip_backend.HipEngine(precision=prec, resnet_chunk=chunk)
            eng.load_resnet18(_sd(seed))
            _ENGINES[key] = eng
        return _ENGINES[key]

    yield get
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _norm_entry(eng, u8_dev, n, pair, out_dev, softmax=0, emb_dev=None):
    lib = eng._lib
    assert lib.cv_resnet_forward_u8_norm(eng._h, u8_dev.data_ptr(), n, pair[0], pair[1], softmax, out_dev.data_ptr(),
                                         emb_dev.data_ptr() if emb_dev is not None else None, _stream()) == 0, lib.cv_last_error()


def _float_entry(eng, x_dev, n, out_dev):
    assert eng._lib.cv_resnet18_forward(eng._h, x_dev.data_ptr(), n, out_dev.data_ptr(), _stream()) == 0, eng._lib.cv_last_error()


def _probe_squares(n, seed=3):
    """(n,64,64) uint8: random bytes; every byte value 0..255 inside the first and the last square; 0 and 255 on all four edges of
    both (the zero border of the stem's plane sits right next to them)."""
    sq = np.random.default_rng(seed).integers(0, 256, (n, 64, 64), dtype=np.uint8)
    for i in {0, n - 1}:
        sq[i, 8:12, :] = np.arange(256, dtype=np.uint8).reshape(4, 64)
        edge = np.tile(np.array([0, 255], np.uint8), 32)
        sq[i, 0, :], sq[i, -1, :], sq[i, :, 0], sq[i, :, -1] = edge, edge[::-1], edge[::-1], edge
    return sq


# ---- 1. the transform, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_normalised_bytes_equal_the_float_entry_fed_torchs_transform(engine, prec):
    cases = [(engine(prec), n) for n in (1, 64, 65, 512, 513)] + [(engine(prec, chunk=128), 129)]      # 512 | 513: the graph limit
    for eng, n in cases:
        u8 = _probe_squares(n)
        u8_dev = torch.from_numpy(u8).cuda()
        for pair in PAIRS:
            x_dev = sr.to_tensor_normalize(u8, *pair).cuda()
            want, got = torch.empty((n, 13), device="cuda"), torch.full((n, 13), float("nan"), device="cuda")
            _float_entry(eng, x_dev, n, want)
            _norm_entry(eng, u8_dev, n, pair, got)
            torch.cuda.synchronize()
            want, got = want.cpu().numpy(), got.cpu().numpy()
            same = np.array_equal(want, got)
            print(f"SQ transform {prec} n={n} norm={pair}: equal {same} max|diff| {np.abs(want - got).max():.3e} max|logit| {np.abs(want).max():.3f}")
            assert np.isfinite(want).all() and same, (prec, n, pair)
        eng.check_numerics()


def test_bad_normalisation_constants_are_refused(engine):
    eng = engine("f16x3")
    u8 = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda")
    out = torch.empty((1, 13), device="cuda")
    for mean, std in ((float("nan"), 1.0), (float("inf"), 1.0), (0.5, 0.0), (0.5, -1.0), (0.5, float("nan")), (0.5, float("inf"))):
        assert eng._lib.cv_resnet_forward_u8_norm(eng._h, u8.data_ptr(), 1, mean, std, 0, out.data_ptr(), None, _stream()) == 1, (mean, std)
    assert b"std" in eng._lib.cv_last_error()


# ---- 2. the graph key ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_graph_key_tells_plain_and_the_two_normalisations_apart(engine, prec):
    """The same device buffers every time at n = 64 (a captured graph, engine.h: run_graphed: eager, capture, replay): plain, norm(a),
    norm(b), plain -- three rounds, so the last round is replays only."""
    eng, n = engine(prec), 64
    u8 = _probe_squares(n, seed=4)
    u8_dev, out = torch.from_numpy(u8).cuda(), torch.empty((n, 13), device="cuda")
    want = {}
    for pair in PAIRS:
        ref = torch.empty((n, 13), device="cuda")
        _float_entry(eng, sr.to_tensor_normalize(u8, *pair).cuda(), n, ref)
        want[pair] = ref.cpu().numpy()
    plain = []
    for rnd in range(3):
        for step in ("plain", PAIRS[0], PAIRS[1], "plain"):
            out.fill_(float("nan"))
            if step == "plain":
                assert eng._lib.cv_resnet18_forward_u8(eng._h, u8_dev.data_ptr(), n, out.data_ptr(), _stream()) == 0
                plain.append(out.cpu().numpy())
            else:
                _norm_entry(eng, u8_dev, n, step, out)
                assert np.array_equal(out.cpu().numpy(), want[step]), (prec, rnd, step)
    assert len(plain) == 6 and all(np.array_equal(plain[0], p) for p in plain[1:])
    assert np.allclose(plain[0].sum(axis=1), 1.0, atol=1e-5)             # probabilities, not the logits of a normalised graph
    assert not np.array_equal(want[PAIRS[0]], want[PAIRS[1]])
    eng.check_numerics()


# ---- 3. the existing entry keeps its bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_existing_byte_entry_equals_the_float_entry(engine, prec):
    """cv_resnet18_forward_u8 against cv_resnet18_forward(u8 / 255) on the fixture: the stem's output and layer4 bit for bit (the byte
    entry returns probabilities, the float entry logits: the tensors in front of the head are compared, and the probabilities against
    the soft-max of the same head through the (0, 1) normalisation, whose arithmetic is the identity)."""
    eng = engine(prec)
    u8, _ = sr.fixture()
    n = len(u8)
    u8_dev = torch.from_numpy(u8).cuda()
    probs = eng.resnet18_forward_u8(u8_dev).cpu().numpy()
    taps_u8 = {t: eng.activation("resnet18", t) for t in ("maxpool", "layer4")}
    logits = eng.resnet18_forward(sr.to_tensor_normalize(u8, None, None).cuda()).cpu().numpy()
    for t, a in taps_u8.items():
        assert np.array_equal(a, eng.activation("resnet18", t)), (prec, t)
    ident_logits, ident_probs = torch.empty((n, 13), device="cuda"), torch.empty((n, 13), device="cuda")
    _norm_entry(eng, u8_dev, n, (0.0, 1.0), ident_logits)
    _norm_entry(eng, u8_dev, n, (0.0, 1.0), ident_probs, softmax=1)
    assert np.array_equal(ident_logits.cpu().numpy(), logits) and np.array_equal(ident_probs.cpu().numpy(), probs)
    assert float(np.abs(torch.softmax(torch.from_numpy(logits).double(), 1).numpy() - probs).max()) <= 1e-6


# ---- 4. parity against the oracle on real squares --------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(seed, pair):
    if (seed, pair) not in _ORACLE:
        u8, _ = sr.fixture()
        with torch.no_grad():
            _ORACLE[(seed, pair)] = synth.make_resnet(seed)(sr.to_tensor_normalize(u8, *(pair or (None, None)))).numpy()
    return _ORACLE[(seed, pair)]


@pytest.mark.parametrize("seed", [2, 3])
@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16r", "f16"])
def test_normalised_logits_match_the_oracle(engine, prec, seed):
    eng = engine(prec, seed)
    u8, _ = sr.fixture()
    u8_dev = torch.from_numpy(u8).cuda()
    for pair in (TRAIN, None):
        ref = _oracle(seed, pair)
        got = eng.resnet_forward_u8_norm(u8_dev, pair or (0.0, 1.0)).cpu().numpy()
        guard = "quiet"
        try:
            eng.check_numerics()
        except hip_backend.NumericRangeError as exc:
            guard = f"TRIPPED at {exc.layer}"
        err = float(np.abs(got - ref).max())
        p_err = float((torch.softmax(torch.from_numpy(got), 1) - torch.softmax(torch.from_numpy(ref), 1)).abs().max())
        agree = float((got.argmax(1) == ref.argmax(1)).mean())
        print(f"SQ oracle {prec} seed {seed} normalised {pair is not None}: logits err {err:.3e} (max|ref| {np.abs(ref).max():.3f}) "
              f"probabilities err {p_err:.3e} arg-max agreement {agree:.4f} guard {guard}")
        if prec in ("f32", "f16x3"):                          # f16r / f16: measured and recorded, no bar
            assert guard == "quiet" and err <= 1e-3, (prec, seed, pair, err, guard)


# ---- 5. the records kernel ---------------------------------------------------------------------------------------------------------------
def _check_records(rec, x, t, what):
    host = evaluation.square_records(x, t)
    for k in ("predicted", "rank", "label", "flags"):
        assert np.array_equal(rec[k], getattr(host, k)), (what, k)
    sr.check_against_torch(evaluation.SquareScores.from_records(rec), x, t, what)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_records_kernel_on_the_devices_own_logits(engine, n):
    eng = engine("f16x3")
    rng = np.random.default_rng(n)
    logits = eng.resnet_forward_u8_norm(torch.from_numpy(rng.integers(0, 256, (n, 64, 64), dtype=np.uint8)).cuda(), TRAIN)
    t = rng.integers(-1, 13, n)
    rec = eng.square_records(logits, t)
    assert rec.dtype == hip_backend.SQUARE_RECORD and rec.shape == (n,)
    _check_records(rec, logits.cpu().numpy(), t, f"device n={n}")
    none = eng.square_records(logits, None)
    assert (none["rank"] == -1).all() and (none["label"] == -1).all() and np.isnan(none["loss"]).all()
    assert np.array_equal(none["predicted"], rec["predicted"]) and np.array_equal(none["confidence"], rec["confidence"])


def test_records_kernel_on_the_crafted_rows_and_bad_labels(engine):
    eng = engine("f16x3")
    x, t = sr.crafted_rows()
    _check_records(eng.square_records(torch.from_numpy(x), t), x, t, "device crafted")
    with pytest.raises(hip_backend.HipBackendError):
        eng.square_records(torch.from_numpy(x), np.full(len(x), 13))
    bad = torch.tensor([13, -2, 127, -128, 5], dtype=torch.int8, device="cuda")          # past the Python check: flagged by the kernel
    rec = eng.square_records_dev(torch.from_numpy(x[:5].copy()).cuda(), bad).cpu().numpy().view(hip_backend.SQUARE_RECORD).reshape(-1)
    assert rec["flags"].tolist() == [2, 2, 2, 2, 0] and rec["label"].tolist() == [13, -2, 127, -128, 5]
    assert (rec["rank"][:4] == -1).all() and np.isnan(rec["loss"][:4]).all() and rec["rank"][4] >= 0
    with pytest.raises(hip_backend.HipBackendError):
        hip_backend.square_records_finish(rec)
    lib = eng._lib
    assert lib.cv_square_records(eng._h, None, None, 1, None, _stream()) == 1 and b"cv_square_records" in lib.cv_last_error()
    ok = torch.zeros((1, 13), device="cuda")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert lib.cv_square_records(eng._h, ok.data_ptr(), None, 0, out.data_ptr(), _stream()) == 1
    assert lib.cv_square_records(eng._h, ok.data_ptr(), None, 1, out.data_ptr() + 4, _stream()) == 1      # records 8-byte aligned


# ---- 6. evaluate_squares end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [2, 3])
def test_evaluate_squares_matches_the_oracle(engine, seed):
    from chessvision.hip_backend import HipPieceClassifier

    eng = engine("f16x3", seed)
    cv = ChessVision(precision="f16x3")
    cv._classifier = HipPieceClassifier(eng)
    u8, lab = sr.fixture()
    ref = torch.from_numpy(_oracle(seed, TRAIN))
    target = torch.from_numpy(lab.astype(np.int64))
    ref_loss = F.cross_entropy(ref, target, reduction="none").numpy()
    ref_conf = torch.softmax(ref, 1).max(1).values.numpy()
    ref_pred = ref.argmax(1).numpy()
    ref_rank = 12 - (torch.argsort(ref, dim=1, stable=True) == target[:, None]).nonzero()[:, 1].numpy()
    val_loss, val_acc, _, _, _ = sr.validate_restated(ref_loss, ref_pred, lab, np.zeros(130, bool), 64)
    gaps = np.diff(np.sort(ref.numpy(), axis=1), axis=1).min(axis=1)
    kept = gaps >= 2e-3

    report = cv.evaluate_squares(u8, [constants.LABEL_NAMES[i] for i in lab], batch_size=64, embeddings=True)
    e_loss, e_conf = float(np.abs(report.loss - ref_loss).max()), float(np.abs(report.confidence - ref_conf).max())
    e_val = abs(report.aggregate["val_loss"] - val_loss)
    print(f"SQ e2e seed {seed}: loss err {e_loss:.3e} confidence err {e_conf:.3e} val_loss {report.aggregate['val_loss']:.6f} "
          f"(oracle {val_loss:.6f}, err {e_val:.3e}) val_acc {report.aggregate['val_acc']:.4f} (oracle {val_acc:.4f}) "
          f"excluded rows {int((~kept).sum())}")
    assert int((~kept).sum()) <= 6
    assert e_loss <= 2e-3 and e_conf <= 2e-3 and e_val <= 2e-3
    assert np.array_equal(report.predicted[kept], ref_pred[kept]) and np.array_equal(report.rank[kept], ref_rank[kept])
    hits = int(report.correct[kept].sum()) + int((ref_pred == lab)[~kept].sum())
    assert 100.0 * hits / 130 == val_acc
    agg = report.aggregate
    assert agg["n"] == agg["n_labelled"] == 130 and agg["n_batches"] == 3 and agg["n_nan"] == 0
    assert agg["val_acc"] == 100.0 * int(report.correct.sum()) / 130 and agg["n_correct"] == int(report.correct.sum())
    assert agg["confusion"].sum() == 130 and agg["hits"][12] == 130 and agg["hits"][0] == int((report.rank == 0).sum())
    _, emb = eng.resnet_forward_u8_norm(torch.from_numpy(u8).cuda(), TRAIN, want_embedding=True)
    assert report.embeddings.shape == (130, 512) and np.array_equal(report.embeddings, emb.cpu().numpy())

    same = cv.evaluate_squares(u8, lab, batch_size=512)                   # batch_size shapes val_loss only: the forward is the same
    assert same.embeddings is None and np.array_equal(same.loss, report.loss) and np.array_equal(same.predicted, report.predicted)
    assert same.aggregate["n_batches"] == 1 and same.aggregate["val_loss"] == pytest.approx(float(report.loss.astype(np.float64).mean()), rel=1e-12)
    blind = cv.evaluate_squares(u8)
    assert np.isnan(blind.loss).all() and (blind.rank == -1).all() and not blind.correct.any()
    assert np.array_equal(blind.predicted, report.predicted) and np.isnan(blind.aggregate["val_loss"])
    plain = cv.evaluate_squares(u8, lab, normalize=None)                   # the /255 of classify_position
    probs = eng.resnet18_forward_u8(torch.from_numpy(u8).cuda()).cpu().numpy()
    assert np.array_equal(plain.predicted, probs.argmax(1)) and float(np.abs(plain.confidence - probs.max(1)).max()) <= 1e-6

"""GPU: timm ResNet-34 as the piece classifier, against the CPU fp32 helper (tests/resnet34_ref.py) on synthetic.resnet34_state_dict.

Forward in every precision (f32 / f16x3 logits within 1e-3; f16r soft-max within 1e-3 and arg-max agreement >= 0.9995, BASELINE
configs[2]; f16 runs with a clean numeric guard), the per-layer taps, the u8 entry, the bits of every schedule of the chained layer1,
the loader's strictness, the by-name entry points and the pipeline through ``ChessVision(classifier_model_id="resnet34")``."""
from __future__ import annotations

import os
import subprocess
import sys
import threading
import time
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "chessvision-3lc_amd"), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import resnet34_ref  # noqa: E402
from chessvision import ChessVision, hip_backend, synthetic  # noqa: E402
from chessvision.hip_backend import HipBackendError, HipEngine  # noqa: E402
from oracle import pipeline_ref, synth  # noqa: E402
from oracle.unet_ref import UNet  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = ("f32", "f16x3", "f16r", "f16")
SIZES = (1, 63, 64, 65, 1000)
TAPS = ("layer1", "layer2", "layer3", "layer4", "layer3.5", "layer2.0.downsample")
PHOTOS = [Path(__file__).resolve().parent / "golden" / f"photos8_{i}.npz" for i in range(8)]


@pytest.fixture(scope="module")
def state():
    return synthetic.resnet34_state_dict(2)


@pytest.fixture(scope="module")
def net(state):
    return resnet34_ref.make_resnet34(state)


@pytest.fixture(scope="module")
def squares():
    return synth.squares_input(34, 4096)


@pytest.fixture(scope="module")
def ref_logits(net, squares):
    with torch.no_grad():
        return net(squares)


@pytest.fixture(scope="module")
def engines(state):
    """precision -> (engine at resnet_chunk=256, engine at the default chunk)"""
    out = {}
    for prec in PRECS:
        small = HipEngine(precision=prec, resnet_chunk=256)
        small.load_resnet(state, "resnet34")
        big = HipEngine(precision=prec)
        big.load_resnet(state, "resnet34")
        out[prec] = (small, big)
    yield out
    for small, big in out.values():
        small.close()
        big.close()


@pytest.mark.parametrize("prec", PRECS)
def test_forward_matches_the_helper(engines, squares, ref_logits, prec):
    small, big = engines[prec]
    assert small.classifier_arch == big.classifier_arch == "resnet34"
    worst = {"logit": 0.0, "prob": 0.0, "squares": 0, "agree": 0, "flip_margins": []}
    runs = [(small, n) for n in SIZES] + [(big, 4096)]
    for eng, n in runs:
        out = eng.resnet18_forward(squares[:n]).cpu()
        assert out.shape == (n, 13) and bool(torch.isfinite(out).all())
        ref = ref_logits[:n]
        p_ref, p_got = torch.softmax(ref, 1), torch.softmax(out, 1)
        worst["logit"] = max(worst["logit"], float((out - ref).abs().max()))
        worst["prob"] = max(worst["prob"], float((p_ref - p_got).abs().max()))
        same = p_ref.argmax(1) == p_got.argmax(1)
        worst["squares"] += n
        worst["agree"] += int(same.sum())
        top2 = torch.sort(p_ref, 1).values[:, -2:]
        worst["flip_margins"] += [float(m) for m in (top2[:, 1] - top2[:, 0])[~same]]
        eng.check_numerics()                       # every precision: the numeric guard stays clean
    agreement = worst["agree"] / worst["squares"]
    print(f"resnet34 {prec}: worst logit err {worst['logit']:.3e}, soft-max err {worst['prob']:.3e}, arg-max agreement {agreement:.5f} "
          f"over {worst['squares']} squares, oracle top-2 margins of the flips {worst['flip_margins']}")
    if prec in ("f32", "f16x3"):
        assert worst["logit"] <= 1e-3, worst
    elif prec == "f16r":
        # configs[2]: soft-max within 1e-3, arg-max agreement >= 0.9995; a flip can only be a near-tie inside twice the soft-max bar
        assert worst["prob"] <= 1e-3 and agreement >= 0.9995, worst
        assert all(m <= 2e-3 for m in worst["flip_margins"]), worst


@pytest.mark.parametrize("prec", PRECS)
def test_layer_taps_match_the_helper(engines, net, squares, prec):
    small, _ = engines[prec]
    x = squares[:300]                                           # chunk 256: the taps hold the ragged last chunk, rows 256..299
    ref = resnet34_ref.taps(net, x, TAPS)
    small.resnet18_forward(x).cpu()
    for name in TAPS:
        got = torch.from_numpy(small.activation("resnet34", name))
        r = ref[name][256:300]
        assert got.shape == r.shape, (name, got.shape, r.shape)
        err, scale = float((got - r).abs().max()), float(r.abs().max())
        if prec in ("f32", "f16x3"):
            assert err <= 1e-3 * max(1.0, scale), (name, err, scale)
        elif prec == "f16r":
            assert err <= 5e-3 * max(1.0, scale), (name, err, scale)
    if prec == "f16r":
        assert small.activation("resnet34", "layer1.1").shape == (44, 64, 16, 16)     # an inner chained block: its f32 twin
        with pytest.raises(HipBackendError, match="layer1.0.act1, layer1.1.act1, layer1.2.act1"):
            small.activation("resnet34", "layer1.2.act1")


def test_u8_entry_gives_the_softmax_of_the_float_path(engines):
    for prec in ("f32", "f16x3", "f16r"):
        eng = engines[prec][0]
        sq = torch.from_numpy(synthetic.random_u8(5, "squares34", (130, 64, 64))).cuda()
        probs = eng.resnet18_forward_u8(sq)
        f = sq.float().unsqueeze(1) / 255.0
        ref = torch.softmax(eng.resnet18_forward(f), 1)
        # the f16 trunk rounds the two inputs (u8 * 2^7 / 255 and the f32 quotient) to f16 apart: its bar is the f16r soft-max bar
        assert float((probs - ref).abs().max()) <= (1e-3 if prec == "f16r" else 1e-6), prec


CHAIN_SCRIPT = r"""
import hashlib, sys
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/chessvision-3lc_amd")
import torch
from chessvision import synthetic
from chessvision.hip_backend import HipEngine
from oracle import synth
eng = HipEngine(precision="f16r", resnet_chunk=256)
eng.load_resnet(synthetic.resnet34_state_dict(2), "resnet34")
h = hashlib.sha256()
for n in (64, 1, 300, 1000):
    x = synth.squares_input(90 + n, n).cuda()
    outs = [eng.resnet18_forward(x).cpu() for _ in range(3)]           # eager, capture, replay at graphed sizes
    assert all(torch.equal(outs[0], o) for o in outs[1:]), ("not deterministic", n)
    h.update(outs[0].numpy().tobytes())
eng.check_numerics()
print("SHA", h.hexdigest())
"""


def test_f16r_layer1_chain_forms_give_the_bits_of_the_layer_by_layer_schedule():
    """The three-block chain (default), its one-workgroup form (CV_CHAIN_WG=1) and the two-block chain with layer1.2 as two launches
    (CV_RESNET_CHAIN_BLOCKS=2) give the bits of layer1 run layer by layer (CV_RESNET_CHAIN=0); each in a process of its own."""
    shas = {}
    for name, knobs in (("default", {}), ("one_wg", {"CV_CHAIN_WG": "1"}), ("two_blocks", {"CV_RESNET_CHAIN_BLOCKS": "2"}),
                        ("layer_by_layer", {"CV_RESNET_CHAIN": "0"})):
        env = dict(os.environ)
        env.update(knobs)
        out = subprocess.run([sys.executable, "-c", CHAIN_SCRIPT.replace("ROOT", str(ROOT))], env=env, capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0 and "SHA" in out.stdout, (name, out.returncode, out.stdout[-500:], out.stderr[-3000:])
        shas[name] = out.stdout.split("SHA", 1)[1].split()[0]
    assert shas["default"] == shas["one_wg"] == shas["two_blocks"] == shas["layer_by_layer"], shas


def test_loader_is_strict(state):
    eng = HipEngine(precision="f16x3", resnet_chunk=256)
    try:
        eng.load_resnet(dict(state), "resnet34")               # the exact key set
        bad = dict(state, **{"layer3.5.conv3.weight": state["layer3.5.conv2.weight"]})
        with pytest.raises(HipBackendError, match=r"layer3\.5\.conv3\.weight"):
            eng.load_resnet(bad, "resnet34")
        bad = dict(state)
        bad.pop("layer2.3.bn1.running_var")
        with pytest.raises(HipBackendError, match=r"layer2\.3\.bn1\.running_var"):
            eng.load_resnet(bad, "resnet34")
        bad = dict(state)
        bad["layer4.2.conv1.weigth"] = bad.pop("layer4.2.conv1.weight")
        with pytest.raises(HipBackendError, match=r"layer4\.2\.conv1\.weig"):
            eng.load_resnet(bad, "resnet34")
        bad = dict(state, **{"layer3.4.conv2.weight": np.zeros((256, 256, 3, 1), np.float32)})
        with pytest.raises(HipBackendError, match=r"layer3\.4\.conv2\.weight"):
            eng.load_resnet(bad, "resnet34")
        with pytest.raises(HipBackendError, match=r"layer1\.2\.conv1\.weight"):
            eng.load_resnet(synthetic.resnet18_state_dict(2), "resnet34")
        with pytest.raises(HipBackendError):
            eng.load_resnet18(state)
        with pytest.raises(HipBackendError, match="'resnet18' or 'resnet34'"):          # the C entry point names the two
            hip_backend._check(eng._lib.cv_load_resnet(eng._h, b"resnet50", None, 0))
        with pytest.raises(HipBackendError, match="resnet50"):
            eng.load_resnet(state, "resnet50")
    finally:
        eng.close()


def test_by_name_entry_points(engines):
    eng = engines["f16r"][0]
    assert eng.model_macs("resnet34") == resnet34_ref.macs() == 292_624_896
    exps = eng.export_calibration("resnet34")
    assert exps.size > 0 and eng.import_calibration("resnet34", exps) is False
    for call in (lambda: eng.model_macs("resnet18"), lambda: eng.export_calibration("resnet18"),
                 lambda: eng.activation("resnet18", "layer1"), lambda: eng.activation_exponent("resnet18", "layer1")):
        with pytest.raises(HipBackendError, match="holds resnet34"):
            call()


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------
def _compare(got, ref, stats, resnet, image, fallback_quad=True):
    """tests/test_gpu_e2e.py's rule: quadrangles and boards identical, probabilities within 1e-3, FEN and fixes equal where every
    square's two best oracle classes differ by more than 2e-3, else the arg-max of the decided squares."""
    ge, re_ = got.board_extraction, ref.board_extraction
    assert np.abs(ge.probabilities - re_.probabilities).max() <= 1e-3
    unsure = np.abs(re_.probabilities) < 1e-4
    assert np.array_equal(ge.binary_mask[~unsure], re_.binary_mask[~unsure])
    if unsure.any() and not np.array_equal(ge.binary_mask, re_.binary_mask):
        stats["mask_flips_inside_tolerance"] += 1
        ref = pipeline_ref.process_from_mask(resnet, image, ge.binary_mask, re_.probabilities, False, fallback_quad)
        re_ = ref.board_extraction
    assert (ge.quadrangle is None) == (re_.quadrangle is None)
    assert (got.position is None) == (ref.position is None)
    if re_.quadrangle is not None:
        assert np.array_equal(ge.quadrangle, re_.quadrangle)
    if ref.position is None:
        return
    assert np.array_equal(ge.board_image, re_.board_image)
    gp, rp = got.position, ref.position
    perr = np.abs(gp.model_probabilities - rp.model_probabilities).max()
    assert perr <= 1e-3, perr
    stats["max_prob_err"] = max(stats["max_prob_err"], float(perr))
    top2 = np.sort(rp.model_probabilities, axis=1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 2e-3
    if decided.all():
        assert gp.original_fen == rp.original_fen and gp.fen == rp.fen
        assert [(f.square_name, f.original_piece, f.corrected_piece, f.rule_name) for f in gp.validation_fixes] == \
               [(f.square_name, f.original_piece, f.corrected_piece, f.rule_name) for f in rp.validation_fixes]
        stats["fen_checked"] += 1
    else:
        assert np.array_equal(np.argmax(gp.model_probabilities, axis=1)[decided], np.argmax(rp.model_probabilities, axis=1)[decided])
    assert gp.square_names == rp.square_names


def _boards(n, seed0):
    imgs = [synthetic.board_photo(seed0 + s) for s in range(n)]
    for k in range(0, n, 7):                                  # every seventh: no board at all -> fallback quadrangle
        imgs[k] = np.random.default_rng(1000 + k).integers(0, 60, (512, 512, 3), dtype=np.uint8)
    return imgs


@pytest.fixture(scope="module")
def pipeline_oracle(net):
    unet = UNet(3, 1, False)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.unet_state_dict(1, segmenting=True).items()}, strict=False)
    unet.eval()
    boards = _boards(32, 900)
    photos = [np.ascontiguousarray(im) for im in np.concatenate([np.load(p)["bgr"] for p in PHOTOS])]
    return {"unet": unet, "boards": boards, "photos": photos,
            "boards_ref": pipeline_ref.process_images(unet, net, boards, fallback_quad=True),
            "photos_ref": [pipeline_ref.process_image(unet, net, im, fallback_quad=True) for im in photos]}


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    return synthetic.save_checkpoints(tmp_path_factory.mktemp("weights_r34"), segmenting=True, classifier_arch="resnet34")


@pytest.mark.parametrize("precision", ["f16x3", "f16x3+f16r"])
def test_pipeline_with_a_resnet34_classifier_matches_the_oracle(pipeline_oracle, checkpoints, net, precision):
    pe, pc = checkpoints
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), classifier_model_id="resnet34", precision=precision)
    try:
        assert cv.classifier.model_name == "resnet34" and cv._get_engine("resnet18").classifier_arch == "resnet34"
        stats = {"mask_flips_inside_tolerance": 0, "max_prob_err": 0.0, "fen_checked": 0}
        got = cv.process_images(pipeline_oracle["boards"], fallback_quad=True)
        for g, r, im in zip(got, pipeline_oracle["boards_ref"], pipeline_oracle["boards"]):
            _compare(g, r, stats, net, im)
        singles = []
        for im, r in zip(pipeline_oracle["photos"], pipeline_oracle["photos_ref"]):
            g = cv._process_image_native(im, 0.5, False, time.time(), fallback_quad=True)
            assert g.position is not None
            _compare(g, r, stats, net, im)
            singles.append(g)
        print(f"resnet34 pipeline {precision}: {stats}")
        assert stats["fen_checked"] >= 16 and stats["mask_flips_inside_tolerance"] <= 2, stats
        # classify_position on a rectified board is the same classifier
        board = got[1].board_extraction.board_image
        pos = cv.classify_position(board)
        assert np.abs(pos.model_probabilities - got[1].position.model_probabilities).max() <= 1e-3

        # request slots: replicas load the ResNet-34 too, and four threads return exactly the serial results
        images = pipeline_oracle["boards"][1:7]
        want = [cv.process_image(im) for im in images]
        assert cv.warm_request_slots(4) > 1
        assert all(s.classifier_engine.classifier_arch == "resnet34" for s in cv._slots)
        bad = []

        def worker(t):
            for k in range(12):
                r, w = cv.process_image(images[(t + k) % 6]), want[(t + k) % 6]
                if not (r.position.fen == w.position.fen and np.array_equal(r.position.model_probabilities, w.position.model_probabilities)
                        and np.array_equal(r.board_extraction.board_image, w.board_extraction.board_image)):
                    bad.append((t, k))

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=600)
        assert not bad, bad
    finally:
        cv.close()


def test_resnet34_checkpoint_under_the_default_id_fails_and_names_the_id(checkpoints):
    pe, pc = checkpoints
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc))
    try:
        with pytest.raises(HipBackendError, match="classifier_model_id='resnet34'"):
            _ = cv.classifier
    finally:
        cv.close()

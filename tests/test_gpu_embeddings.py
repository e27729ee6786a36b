"""GPU: embeddings at the reference's 3LC hook points -- the channel-mean kernel on every stored layout, the forward entry points that
pool inside the forward (per chunk, inside the captured graph), the oracle's hooked means, and ``process_images(embeddings=True)``.

Bars.  Pooling alone (cases 1, 2): 1e-5 * max(1, max|ref|) against the float64 mean of the device's own stored values -- the project's
bar for f32 pointwise ops (layer_local.BARS: bilinear / outconv).  Against the torch-CPU oracle (cases 4, 5): the parity contract,
1e-3 * max(1, max|ref|), asserted for f32 and f16x3; f16 and f16r are measured and printed only (their logits are outside 1e-3 by
design).  The measured figures are in profiles/embeddings.md.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import layer_local as ll
import resnet34_ref
from chessvision import ChessVision, embeddings, synthetic
from oracle import pipeline_ref, synth
from oracle.resnet_ref import ResNet18
from oracle.unet_ref import UNet

pytestmark = pytest.mark.gpu

BOTTLENECK = "down4.maxpool_conv.1.double_conv.5"
CV_ERR_INVALID = 1


def _pool_bar(ref):
    return 1e-5 * max(1.0, float(np.abs(ref).max()))


def _parity_bar(ref):
    return 1e-3 * max(1.0, float(np.abs(ref).max()))


def _mean64(nchw):
    return np.asarray(nchw, dtype=np.float64).mean(axis=(2, 3))


def _check_pool(tag, got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float32 and got.shape == ref.shape, (tag, got.shape, ref.shape)
    err, bar = float(np.abs(got - ref).max()), _pool_bar(ref)
    print(f"EMB pool {tag}: err {err:.3e} bar {bar:.3e} err/bar {err / bar:.3f}")
    assert np.isfinite(got).all() and err <= bar, (tag, err, bar)
    return err / bar


def _same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- engines: those of test_gpu_layer_local.py ------------------------------------------------------------------------------------
UNET_ENGINES = [(prec, bilinear) for prec in ("f32", "f16x3", "f16") for bilinear in (False, True)]
RESNET_ENGINES = [("resnet18", p) for p in ("f32", "f16x3", "f16", "f16r")] + [("resnet34", p) for p in ("f16x3", "f16r")]


@pytest.fixture(scope="module", params=UNET_ENGINES, ids=[f"{p}-{'bilinear' if b else 'convT'}" for p, b in UNET_ENGINES])
def unet_engine(request):
    from chessvision.hip_backend import HipEngine

    prec, bilinear = request.param
    net = synth.make_unet(seed=1, bilinear=bilinear)
    eng = HipEngine(precision=prec, unet_chunk=2)
    eng.load_unet(net.state_dict())
    yield eng, prec, bilinear
    try:
        eng.check_numerics()
    finally:
        eng.close()


def _resnet(arch):
    return synth.make_resnet(seed=2) if arch == "resnet18" else resnet34_ref.make_resnet34(synthetic.resnet34_state_dict(2))


@pytest.fixture(scope="module", params=RESNET_ENGINES, ids=[f"{a}-{p}" for a, p in RESNET_ENGINES])
def resnet_engine(request):
    from chessvision.hip_backend import HipEngine

    arch, prec = request.param
    sd = _resnet(arch).state_dict()
    eng = HipEngine(precision=prec, resnet_chunk=128)
    eng.load_resnet({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}, arch)
    yield eng, arch, prec
    try:
        eng.check_numerics()
    finally:
        eng.close()


_INPUTS = {}


def _unet_x3():
    if "unet3" not in _INPUTS:
        u8 = ll.unet_images_u8(5, ["random", "photo", "border"])
        _INPUTS["unet3"] = (u8, ll.unet_f32(u8))
    return _INPUTS["unet3"]


def _squares200():
    if "sq200" not in _INPUTS:
        u8 = ll.squares_u8(11, 200, ll.specials_from(131))
        _INPUTS["sq200"] = (u8, ll.squares_f32(u8))
    return _INPUTS["sq200"]


# ---- 1. layer-local: the pooling alone, on every layout the engines store -----------------------------------------------------------
def test_unet_channel_means_of_stored_taps_match_float64(unet_engine):
    eng, prec, bilinear = unet_engine
    assert eng.embedding_dim("unet") == (512 if bilinear else 1024)
    eng.unet_forward(_unet_x3()[1])                      # chunks of 2 + 1: the taps hold the border-saturated image
    worst = 0.0
    for tap in (BOTTLENECK,                              # 16 x 16 x 1024 | 512
                "inc.double_conv.5",                     # 256 x 256: 65536 values per channel; first half of a concatenated buffer
                "up1.up",                                # second half: a channel offset (and its own exponent)
                "down1.maxpool_conv.0"):                 # a pooled copy, exponent tied to the tensor it pools
        stored = eng.activation("unet", tap)
        assert stored.shape[0] == 1
        got = eng.activation_channel_means("unet", tap)
        worst = max(worst, _check_pool(f"unet {prec} {'bilinear' if bilinear else 'convT'} {tap}", got, _mean64(stored)))
    print(f"EMB pool worst unet-{prec}-{'bilinear' if bilinear else 'convT'}: err/bar {worst:.3f}")
    eng.check_numerics()


def test_resnet_channel_means_of_stored_taps_match_float64(resnet_engine):
    eng, arch, prec = resnet_engine
    assert eng.embedding_dim(arch) == 512
    eng.resnet18_forward(_squares200()[1])               # chunks of 128 + 72
    taps = ["maxpool", "layer2", "layer4"] + (["layer2.0.downsample"] if prec == "f16r" else [])   # f16r: a tensor that is an f32 twin only
    worst = 0.0
    for tap in taps:
        stored = eng.activation(arch, tap)
        assert stored.shape[0] == 72
        got = eng.activation_channel_means(arch, tap)
        worst = max(worst, _check_pool(f"{arch} {prec} {tap}", got, _mean64(stored)))
    assert _same_bits(eng.activation_channel_means(arch, "global_pool"), eng.activation_channel_means(arch, "layer4"))
    print(f"EMB pool worst {arch}-{prec}: err/bar {worst:.3f}")
    eng.check_numerics()


# ---- 2. forward + embedding = the plain forward + the pooled hook tap -----------------------------------------------------------------
@pytest.mark.parametrize("entry", ["float", "u8"])
def test_unet_forward_with_embedding_is_the_plain_forward_plus_the_pooled_bottleneck(unet_engine, entry):
    eng, prec, bilinear = unet_engine
    u8, f32 = _unet_x3()
    if entry == "float":
        run = lambda x, **kw: eng.unet_forward(x, **kw)
        x = f32
        plain = (run(x),)
    else:
        run = lambda x, **kw: eng.unet_forward_u8(x, threshold=0.4, want_mask=True, **kw)
        x = torch.from_numpy(u8)
        plain = run(x)
    *outs, emb = run(x, want_embedding=True)
    assert len(outs) == len(plain) and all(_same_bits(a, b) for a, b in zip(outs, plain))      # logits (and mask): bit for bit
    assert emb.shape == (3, eng.embedding_dim("unet")) and emb.dtype == torch.float32 and bool(torch.isfinite(emb).all())
    assert _same_bits(emb[2:], eng.activation_channel_means("unet", BOTTLENECK))                # the last chunk is what the tap holds
    emb = emb.cpu().numpy()
    run(x[:2])                                           # the first chunk as a forward of its own, same chunk shape
    _check_pool(f"unet {prec} {entry} rows of chunk 0", emb[:2], _mean64(eng.activation("unet", BOTTLENECK)))
    eng.check_numerics()


@pytest.mark.parametrize("entry", ["float", "u8"])
def test_resnet_forward_with_embedding_is_the_plain_forward_plus_the_pooled_layer4(resnet_engine, entry):
    eng, arch, prec = resnet_engine
    u8, f32 = _squares200()
    run = eng.resnet18_forward if entry == "float" else eng.resnet18_forward_u8
    x = f32 if entry == "float" else torch.from_numpy(u8)
    plain = run(x)
    out, emb = run(x, want_embedding=True)
    assert _same_bits(out, plain)
    assert emb.shape == (200, 512) and emb.dtype == torch.float32 and bool(torch.isfinite(emb).all())
    assert _same_bits(emb[128:], eng.activation_channel_means(arch, "layer4"))
    emb = emb.cpu().numpy()
    run(x[:128])
    _check_pool(f"{arch} {prec} {entry} rows of chunk 0", emb[:128], _mean64(eng.activation(arch, "layer4")))
    eng.check_numerics()


# ---- 3. graph replay and key separation -------------------------------------------------------------------------------------------------
def _graph_case(eng, emb_entry, plain_entry, x_dev, n, out_dev, emb_dev):
    """The same pointers every time (engine.cpp: run_graphed): eager, capture, replay of the pooling forward; then the plain forward on
    the same x / out (its own graph: eager, capture, replay), which must leave the embedding buffer alone; then the pooling one again."""
    lib, stream = eng._lib, torch.cuda.current_stream().cuda_stream
    first_emb = first_out = None
    for rep in range(3):
        emb_dev.fill_(float("nan"))
        assert getattr(lib, emb_entry)(eng._h, x_dev.data_ptr(), n, out_dev.data_ptr(), emb_dev.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(emb_dev).all()), rep
        if rep == 0:
            first_emb, first_out = emb_dev.clone(), out_dev.clone()
        assert _same_bits(emb_dev, first_emb) and _same_bits(out_dev, first_out), rep
    for rep in range(3):
        emb_dev.fill_(float("nan"))
        out_dev.zero_()
        assert getattr(lib, plain_entry)(eng._h, x_dev.data_ptr(), n, out_dev.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(emb_dev).all()), rep      # not a launch of the plain forward, eager or replayed
        assert _same_bits(out_dev, first_out), rep
    emb_dev.fill_(float("nan"))
    assert getattr(lib, emb_entry)(eng._h, x_dev.data_ptr(), n, out_dev.data_ptr(), emb_dev.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert _same_bits(emb_dev, first_emb) and _same_bits(out_dev, first_out)
    eng.check_numerics()


def test_unet_one_board_graph_replay_pools_and_the_plain_graph_does_not(unet_engine):
    eng, prec, bilinear = unet_engine
    x_dev = ll.unet_f32(ll.unet_images_u8(3, ["random"])).cuda()
    out = torch.empty((1, 1, 256, 256), device="cuda")
    emb = torch.empty((1, eng.embedding_dim("unet")), device="cuda")
    _graph_case(eng, "cv_unet_forward_emb", "cv_unet_forward", x_dev, 1, out, emb)
    assert _same_bits(emb, eng.activation_channel_means("unet", BOTTLENECK))


def test_resnet_one_board_graph_replay_pools_and_the_plain_graph_does_not(resnet_engine):
    eng, arch, prec = resnet_engine
    x_dev = ll.squares_f32(ll.squares_u8(12, 64, ll.specials_from(3))).cuda()
    out = torch.empty((64, 13), device="cuda")
    emb = torch.empty((64, 512), device="cuda")
    _graph_case(eng, "cv_resnet18_forward_emb", "cv_resnet18_forward", x_dev, 64, out, emb)
    assert _same_bits(emb, eng.activation_channel_means(arch, "layer4"))


# ---- 4. against the oracle's forward hooks ------------------------------------------------------------------------------------------------
_ORACLE = {}


def _hooked(net, index, x):
    """Output of ``named_modules()[index]`` of the torch-CPU oracle for input ``x``, as the reference's collector sees it."""
    module = list(net.named_modules())[index][1]
    seen = []
    handle = module.register_forward_hook(lambda m, i, o: seen.append(o.detach()))
    try:
        with torch.no_grad():
            net.eval()(x)
    finally:
        handle.remove()
    assert len(seen) == 1
    return seen[0].numpy()


def _oracle_unet(bilinear):
    if ("unet", bilinear) not in _ORACLE:
        x = ll.unet_f32(ll.unet_images_u8(21, ["random", "photo"]))
        hooked = _hooked(synth.make_unet(seed=1, bilinear=bilinear), embeddings.UNET_HOOK_INDEX, x)
        assert hooked.shape == (2, 512 if bilinear else 1024, 16, 16)
        _ORACLE[("unet", bilinear)] = (x, embeddings.channel_mean(hooked))
    return _ORACLE[("unet", bilinear)]


def _oracle_resnet(arch):
    if arch not in _ORACLE:
        x = ll.squares_f32(ll.squares_u8(22, 64, ll.specials_from(7)))
        hooked = _hooked(_resnet(arch), embeddings.module_names(arch).index("global_pool"), x)
        assert hooked.shape == (64, 512)
        _ORACLE[arch] = (x, embeddings.channel_mean(hooked))
    return _ORACLE[arch]


def _check_parity(tag, prec, got, ref):
    got = got.cpu().numpy()
    err, bar = float(np.abs(got - ref).max()), _parity_bar(ref)
    print(f"EMB oracle {tag} {prec}: err {err:.3e} bar {bar:.3e} err/bar {err / bar:.3f} max|ref| {np.abs(ref).max():.3f}")
    assert got.shape == ref.shape and np.isfinite(got).all()
    if prec in ("f32", "f16x3"):                         # f16 / f16r: measured and recorded, no bar
        assert err <= bar, (tag, prec, err, bar)


def test_unet_embedding_matches_the_oracle_hook_at_index_52(unet_engine):
    eng, prec, bilinear = unet_engine
    x, ref = _oracle_unet(bilinear)
    _, emb = eng.unet_forward(x, want_embedding=True)
    _check_parity(f"unet {'bilinear' if bilinear else 'convT'} [52]", prec, emb, ref)


def test_classifier_embedding_matches_the_oracle_hook_at_global_pool(resnet_engine):
    eng, arch, prec = resnet_engine
    assert embeddings.tap_for_index(arch, embeddings.module_names(arch).index("global_pool")) == "global_pool"
    x, ref = _oracle_resnet(arch)
    _, emb = eng.resnet18_forward(x, want_embedding=True)
    _check_parity(f"{arch} global_pool", prec, emb, ref)


# ---- 5. process_images(embeddings=True) -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipeline_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("weights_embeddings")
    pe, pc = synthetic.save_checkpoints(d, segmenting=True)
    cv = ChessVision(board_extractor_weights=str(pe), classifier_weights=str(pc), precision="f16x3")
    images = [synthetic.board_photo(500 + s) for s in range(5)]
    images.insert(3, np.zeros((512, 512, 3), np.uint8))   # blank: no board is found (no fallback quadrangle)
    kw = dict(pipeline_chunk=2, first_job=1)              # jobs of 1, 1, 2, 2 images
    timings = {}
    off = cv.process_images(images, **kw)
    on = cv.process_images(images, embeddings=True, timings=timings, **kw)
    return cv, images, kw, off, on, timings


def _fields(res):
    e, p = res.board_extraction, res.position
    arrays = [e.probabilities, e.binary_mask, e.quadrangle, e.board_image] + ([p.model_probabilities, p.squares] if p else [])
    return ([None if a is None else (a.dtype.str, a.shape, a.tobytes()) for a in arrays],
            None if p is None else (p.fen, p.original_fen, p.square_names, p.validation_fixes), res.quality)


def test_process_images_with_embeddings_changes_no_other_field(pipeline_runs):
    cv, images, kw, off, on, timings = pipeline_runs
    assert [_fields(r) for r in on] == [_fields(r) for r in off]
    assert all(r.embeddings is None for r in off)
    assert "embedding_ms" not in timings and timings["unet_ms"] > 0 and timings["jobs"] == 4
    channels = cv._get_engine("unet").embedding_dim("unet")
    assert on[3].position is None and sum(r.position is not None for r in on) >= 3     # the blank image; the synthetic boards are found
    for i, r in enumerate(on):
        e = r.embeddings
        assert e.board_extractor.shape == (channels,) and e.board_extractor.dtype == np.float32 and np.isfinite(e.board_extractor).all()
        assert (e.classifier is None) == (r.position is None)
        if e.classifier is not None:
            assert e.classifier.shape == (64, 512) and e.classifier.dtype == np.float32 and np.isfinite(e.classifier).all()


def test_process_images_embeddings_match_the_oracle_pipeline_hooks(pipeline_runs):
    cv, images, kw, off, on, timings = pipeline_runs
    usd = {k: torch.from_numpy(v) for k, v in synthetic.unet_state_dict(1, segmenting=True).items()}
    rsd = {k: torch.from_numpy(v) for k, v in synthetic.resnet18_state_dict(2).items()}
    unet, resnet = UNet(3, 1, False), ResNet18()
    unet.load_state_dict(usd, strict=False)
    resnet.load_state_dict(rsd, strict=False)
    unet, resnet = unet.eval(), resnet.eval()
    seen = {"unet": [], "resnet": []}
    handles = [list(unet.named_modules())[52][1].register_forward_hook(lambda m, i, o: seen["unet"].append(o.detach().numpy())),
               list(resnet.named_modules())[90][1].register_forward_hook(lambda m, i, o: seen["resnet"].append(o.detach().numpy()))]
    try:
        found = [i for i, r in enumerate(on) if r.position is not None]
        for i in (found[0], found[-1]):                  # an image of a one-image job, an image of the last job
            seen["unet"].clear(), seen["resnet"].clear()
            got = on[i]
            ref = pipeline_ref.process_image(unet, resnet, images[i])
            if not np.array_equal(ref.board_extraction.binary_mask, got.board_extraction.binary_mask):
                # a mask pixel inside the logit tolerance flipped (tests/test_gpu_e2e.py): the oracle continues from the product's mask
                seen["resnet"].clear()
                ref = pipeline_ref.process_from_mask(resnet, images[i], got.board_extraction.binary_mask, ref.board_extraction.probabilities)
            assert ref.position is not None and got.position is not None and ref.position.square_names == got.position.square_names
            ref_u, ref_c = embeddings.channel_mean(seen["unet"][-1])[0], embeddings.channel_mean(seen["resnet"][-1])
            for tag, g, r in (("board_extractor", got.embeddings.board_extractor, ref_u), ("classifier", got.embeddings.classifier, ref_c)):
                err, bar = float(np.abs(g - r).max()), _parity_bar(r)
                print(f"EMB pipeline image {i} {tag}: err {err:.3e} bar {bar:.3e} err/bar {err / bar:.3f}")
                assert g.shape == r.shape and err <= bar, (i, tag, err, bar)
    finally:
        for h in handles:
            h.remove()


def test_evaluate_images_carries_the_embeddings_when_the_instance_asks(pipeline_runs):
    """``evaluate_images`` keeps its pinned argument list; the instance attribute ``evaluation_embeddings`` switches the collection on."""
    cv, images, kw, off, on, timings = pipeline_runs
    fens = ["8/8/8/8/8/8/8/8"] * len(images)
    assert all(r.embeddings is None for r in cv.evaluate_images(images, true_fens=fens, pipeline_chunk=2).results)
    cv.evaluation_embeddings = True
    try:
        report = cv.evaluate_images(images, true_fens=fens, pipeline_chunk=2)
    finally:
        cv.evaluation_embeddings = False
    for i, (r, ref) in enumerate(zip(report.results, on)):
        e = r.embeddings
        assert (e.classifier is None) == (ref.embeddings.classifier is None)
        # other job boundaries than the process_images call (first_job): the same boards within the parity bar, not bit for bit
        assert np.abs(e.board_extractor - ref.embeddings.board_extractor).max() <= _parity_bar(ref.embeddings.board_extractor)
        if e.classifier is not None:
            assert np.abs(e.classifier - ref.embeddings.classifier).max() <= _parity_bar(ref.embeddings.classifier)


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_channel_means_argument_errors_name_the_tap(unet_engine):
    eng, prec, bilinear = unet_engine
    eng.unet_forward(_unet_x3()[1][:1])
    lib, stream = eng._lib, torch.cuda.current_stream().cuda_stream
    dims = (ctypes.c_int64 * 2)()
    out = torch.full((2048,), float("nan"), device="cuda")
    channels = eng.embedding_dim("unet")

    def call(tap, capacity):
        return lib.cv_activation_channel_means(eng._h, b"unet", tap.encode(), out.data_ptr(), capacity, dims, stream)

    assert call(BOTTLENECK, channels - 1) == CV_ERR_INVALID                      # too small a capacity
    assert BOTTLENECK.encode() in lib.cv_last_error() and b"too small" in lib.cv_last_error()
    assert call("down5.maxpool_conv.0", 2048) == CV_ERR_INVALID                  # unknown tap
    assert b"down5.maxpool_conv.0" in lib.cv_last_error()
    if prec == "f16x3":                                                          # fused away: exists only inside inc.double_conv.3's kernel
        assert call("inc.double_conv.2", 2048) == CV_ERR_INVALID
        assert b"inc.double_conv.2" in lib.cv_last_error()
        with pytest.raises(ValueError, match="inc.double_conv.2"):
            embeddings.tap_for_index("unet", 5, precision=prec)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                                          # nothing was launched
    assert call(BOTTLENECK, channels) == 0 and list(dims) == [1, channels]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:channels]).all()) and bool(torch.isnan(out[channels:]).all())
    ch = ctypes.c_int(0)
    assert lib.cv_embedding_dim(eng._h, b"resnet18", ctypes.byref(ch)) == 3      # CV_ERR_STATE: no classifier on this engine
    assert b"resnet18" in lib.cv_last_error()
    eng.check_numerics()

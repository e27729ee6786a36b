"""CPU: the host side of the embeddings feature -- module order and layer-index mapping (chessvision/embeddings.py) against the oracle
networks' ``named_modules()``, the host form of the reduction, the new C-ABI symbols and their argument handling without a device, and
the Python signatures."""
from __future__ import annotations

import ctypes
import inspect

import numpy as np
import pytest

import resnet34_ref
from chessvision import embeddings, synthetic
from oracle import synth

NEW_SYMBOLS = ["cv_embedding_dim", "cv_unet_forward_emb", "cv_unet_forward_u8_emb", "cv_resnet18_forward_emb", "cv_resnet18_forward_u8_emb",
               "cv_activation_channel_means"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from chessvision import hip_backend

    return hip_backend.load_library()


def _names(net):
    return [n for n, _ in net.named_modules()]


# ---- module order ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bilinear", [False, True], ids=["convT", "bilinear"])
def test_unet_module_names_are_named_modules_order(bilinear):
    assert embeddings.module_names("unet", bilinear=bilinear) == _names(synth.make_unet(seed=1, bilinear=bilinear))


def test_resnet_module_names_are_named_modules_order():
    assert embeddings.module_names("resnet18") == _names(synth.make_resnet(seed=2))
    assert embeddings.module_names("resnet34") == _names(resnet34_ref.make_resnet34(synthetic.resnet34_state_dict(2)))
    with pytest.raises(ValueError, match="resnet50"):
        embeddings.module_names("resnet50")


# ---- index mapping --------------------------------------------------------------------------------------------------------------
def test_the_reference_hook_indices_map_to_their_taps():
    assert embeddings.UNET_HOOK_INDEX == 52 and embeddings.CLASSIFIER_HOOK_INDEX == 90
    assert embeddings.tap_for_index("unet", 52) == "down4.maxpool_conv.1.double_conv.5"
    assert embeddings.tap_for_index("unet", 52, bilinear=True) == "down4.maxpool_conv.1.double_conv.5"
    assert embeddings.tap_for_index("resnet18", 90) == "global_pool"
    assert embeddings.module_names("resnet34").index("global_pool") == 162
    assert embeddings.tap_for_index("resnet34", 162) == "global_pool"


def test_every_index_maps_to_a_module_output_the_engine_holds_or_raises_naming_the_module():
    """Containers map to the tap of their last stored output, Identity modules to the tap before them; Conv2d / BatchNorm2d (folded
    into one launch), the root, OutConv and fc raise."""
    unet = synth.make_unet(seed=1)
    for i, (name, mod) in enumerate(unet.named_modules()):
        kind = type(mod).__name__
        if kind in ("Conv2d", "BatchNorm2d", "ConvTranspose2d", "UNet", "OutConv") and not name.endswith(".up"):
            with pytest.raises(ValueError) as exc:
                embeddings.tap_for_index("unet", i)
            assert f"index {i}" in str(exc.value) and f"'{name or '<root>'}'" in str(exc.value) and "nearest materialised" in str(exc.value)
        else:
            tap = embeddings.tap_for_index("unet", i)
            assert tap == name or name.startswith(tap), (i, name, tap)
    assert embeddings.tap_for_index("unet", 46) == "down4"                       # down4.maxpool_conv.1.double_conv (Sequential)
    assert embeddings.tap_for_index("unet", 54) == "up1.up"
    with pytest.raises(ValueError, match=r"index 50 .*'down4.maxpool_conv.1.double_conv.3'.*49 \(down4.maxpool_conv.1.double_conv.2\).*52 \("):
        embeddings.tap_for_index("unet", 50)
    resnet = synth.make_resnet(seed=2)
    for i, (name, mod) in enumerate(resnet.named_modules()):
        kind = type(mod).__name__
        if (kind in ("Conv2d", "BatchNorm2d", "Linear", "ResNet18") and not name.endswith("downsample.1")) or name.endswith("drop_block"):
            with pytest.raises(ValueError, match=f"index {i} "):
                embeddings.tap_for_index("resnet18", i)
        else:
            assert embeddings.tap_for_index("resnet18", i)
    assert embeddings.tap_for_index("resnet18", 14) == "layer1.0"                # layer1.0.act2: the block's output
    assert embeddings.tap_for_index("resnet18", 11) == "layer1.0.act1"           # aa: an Identity behind act1
    with pytest.raises(ValueError, match="'layer1.0.drop_block'"):               # an Identity behind bn1, whose output is never stored
        embeddings.tap_for_index("resnet18", 9)
    assert embeddings.tap_for_index("resnet18", 36) == "layer2.0.downsample"     # downsample.1: the shortcut after its BatchNorm
    with pytest.raises(ValueError, match="out of range"):
        embeddings.tap_for_index("resnet18", 94)


def test_a_tap_the_engine_fuses_away_raises_when_the_precision_is_given():
    assert embeddings.tap_for_index("unet", 5) == "inc.double_conv.2"
    assert embeddings.tap_for_index("unet", 5, precision="f32") == "inc.double_conv.2"
    with pytest.raises(ValueError, match=r"index 5 .*'inc.double_conv.2'.*fused away by the f16x3 engine.*8 \(inc.double_conv.5\)"):
        embeddings.tap_for_index("unet", 5, precision="f16x3")
    with pytest.raises(ValueError, match="'up4.conv.double_conv.5'"):
        embeddings.tap_for_index("unet", 92, precision="f16")
    with pytest.raises(ValueError, match="'layer1.0.act1'"):
        embeddings.tap_for_index("resnet18", 10, precision="f16r")
    assert embeddings.tap_for_index("resnet18", 10, precision="f16x3") == "layer1.0.act1"


# ---- host form ------------------------------------------------------------------------------------------------------------------
def test_channel_mean_is_the_float64_spatial_mean():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 24, 16, 16)) * 7 + 100).astype(np.float32)
    got = embeddings.channel_mean(x)
    assert got.dtype == np.float32 and got.shape == (3, 24)
    assert np.array_equal(got, x.astype(np.float64).mean(axis=(2, 3)).astype(np.float32))
    import torch

    assert np.array_equal(embeddings.channel_mean(torch.from_numpy(x)), got)
    pooled = rng.standard_normal((5, 512)).astype(np.float32)
    assert np.array_equal(embeddings.channel_mean(pooled), pooled)               # global_pool's (B, C): both reshape strategies coincide
    with pytest.raises(ValueError):
        embeddings.channel_mean(np.zeros(4, np.float32))


# ---- ABI and signatures ---------------------------------------------------------------------------------------------------------
def test_new_symbols_are_bound_and_exported(lib):
    from chessvision import hip_backend

    bound = {name for name, _, _ in hip_backend.SYMBOLS}
    for sym in NEW_SYMBOLS:
        assert sym in bound and hasattr(lib, sym), sym
    assert hip_backend.ABI_VERSION == 6 and lib.cv_abi_version() == 6
    for method in ("embedding_dim", "activation_channel_means"):
        assert hasattr(hip_backend.HipEngine, method)
    for method in ("unet_forward", "unet_forward_u8", "resnet18_forward", "resnet18_forward_u8"):
        assert inspect.signature(getattr(hip_backend.HipEngine, method)).parameters["want_embedding"].default is False


def test_python_surface():
    from chessvision import ChessVision
    from chessvision.cv_types import BoardExtractionResult, ChessVisionResult, Embeddings

    assert inspect.signature(ChessVision.process_images).parameters["embeddings"].default is False
    ext = BoardExtractionResult(probabilities=np.zeros((256, 256), np.float32), binary_mask=np.zeros((256, 256), np.uint8),
                                quadrangle=None, board_image=None)
    res = ChessVisionResult(ext, None, 0.25)
    assert res.embeddings is None
    res.embeddings = Embeddings(board_extractor=np.zeros(1024, np.float32), classifier=None)
    assert ChessVisionResult(ext, None, 0.5).embeddings is None                  # the default is the class's, not shared state
    assert list(Embeddings.__dataclass_fields__) == ["board_extractor", "classifier"]
    assert ChessVision.evaluation_embeddings is False


def test_null_engine_is_an_error_at_every_new_entry_point(lib):
    dims = (ctypes.c_int64 * 2)()
    ch = ctypes.c_int(0)
    calls = [lambda: lib.cv_embedding_dim(None, b"unet", ctypes.byref(ch)),
             lambda: lib.cv_unet_forward_emb(None, None, 1, None, None, None),
             lambda: lib.cv_unet_forward_u8_emb(None, None, 1, None, None, 0.5, None, None),
             lambda: lib.cv_resnet18_forward_emb(None, None, 64, None, None, None),
             lambda: lib.cv_resnet18_forward_u8_emb(None, None, 64, None, None, None),
             lambda: lib.cv_activation_channel_means(None, b"unet", b"inc", None, 0, dims, None)]
    for call in calls:
        assert call() != 0
        assert b"null engine" in lib.cv_last_error()

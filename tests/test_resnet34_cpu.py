"""ResNet-34 piece classifier, the parts that need no GPU: the CPU helper's structure, the synthetic state dict, the model id and
the library export."""
from __future__ import annotations

import ctypes
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
for _p in (str(ROOT), str(ROOT / "chessvision-3lc_amd"), str(ROOT / "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import resnet34_ref  # noqa: E402
from chessvision import synthetic, utils  # noqa: E402
from chessvision.hip_backend import HipBackendError, library_path  # noqa: E402
from oracle.resnet_ref import ResNet18  # noqa: E402


@pytest.fixture(scope="module")
def net():
    return resnet34_ref.ResNet34().eval()


def test_helper_structure_matches_timm_resnet34(net):
    names = [n for n, _ in net.named_modules()]
    assert len(names) == 166
    assert names.index("global_pool") == 162
    assert sum(p.numel() for p in net.parameters()) == 21_285_069
    assert resnet34_ref.macs(net) == 292_624_896


def test_helper_names_are_resnet18_names_with_the_extra_blocks_inserted(net):
    names34 = [n for n, _ in net.named_modules()]
    names18 = [n for n, _ in ResNet18().named_modules()]
    extra = {f"layer{l}.{b}" for l, d in zip(range(1, 5), resnet34_ref.DEPTHS) for b in range(2, d)}

    def block_of(name):
        parts = name.split(".")
        return ".".join(parts[:2]) if len(parts) >= 2 and parts[0].startswith("layer") else None

    assert [n for n in names34 if block_of(n) not in extra] == names18
    assert {block_of(n) for n in names34} - {None} - {block_of(n) for n in names18} == extra


def test_synthetic_state_dict_has_exactly_the_helper_keys_and_shapes(net):
    sd = synthetic.resnet34_state_dict(2)
    ref = {k: tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    assert len(sd) == 182
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref
    assert [k for k, _, _ in synthetic.resnet34_spec()] == list(sd)


def test_get_classifier_model_accepts_resnet34():
    model = utils.get_classifier_model("resnet34")
    assert model.model_name == "resnet34"
    assert utils.get_classifier_model("resnet18").model_name == "resnet18"
    assert utils.get_classifier_model("").model_name == "resnet18"
    with pytest.raises(HipBackendError, match="resnet18, resnet34"):
        utils.get_classifier_model("resnet50")


def test_checkpoint_architecture_is_recognised_for_the_error_message():
    assert utils._resnet_arch_of(synthetic.resnet34_state_dict(2)) == "resnet34"
    assert utils._resnet_arch_of(synthetic.resnet18_state_dict(2)) == "resnet18"
    assert utils._resnet_arch_of({"conv1.weight": None}) is None


def test_library_exports_cv_load_resnet():
    path = library_path()
    if not path.exists():
        pytest.fail(f"{path} is missing: build it first (__graft_entry__.build())")
    lib = ctypes.CDLL(str(path))
    assert hasattr(lib, "cv_load_resnet") and hasattr(lib, "cv_load_resnet18")

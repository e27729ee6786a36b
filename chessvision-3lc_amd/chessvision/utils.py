"""Model plumbing and small helpers behind ``ChessVision`` (counterpart of the reference's ``chessvision/utils.py``).

What differs from the reference: ``get_classifier_model`` / ``get_board_extractor_model`` do not build torch
modules (timm / Pytorch-UNet) -- they return the HIP model objects of ``hip_backend`` -- and checkpoint loading
yields a plain state dict that is packed by ``cv_load_unet`` / ``cv_load_resnet`` instead of
``module.load_state_dict``.  The four checkpoint layouts accepted are those of ``utils.py:57-80``.
"""
from __future__ import annotations

import logging
import os
from pathlib import Path
from typing import Any, Mapping

import numpy as np
import torch
from numpy.typing import NDArray

from . import classical, constants

logger = logging.getLogger(__name__)


def get_device() -> torch.device:
    """cuda (ROCm) when visible -- the only device the HIP backend runs on -- else cpu (reference utils.py:20-29)."""
    if torch.cuda.is_available():
        logger.info("Using CUDA (ROCm) device")
        return torch.device("cuda")
    logger.info("Using CPU device")
    return torch.device("cpu")


def read_checkpoint(checkpoint_path: str | os.PathLike) -> tuple[Mapping[str, Any], dict]:
    """Return (state_dict, metadata) from any of the reference's checkpoint layouts:
    {"model_state_dict", "metadata"?} | {"state_dict", ...} | {"model", ...} | a bare state dict."""
    assert checkpoint_path is not None and Path(checkpoint_path).exists(), f"Checkpoint not found: {checkpoint_path}"
    logger.info(f"Loading checkpoint from {checkpoint_path}")
    # weights_only=True (the torch >= 2.6 default the reference's plain torch.load gets, utils.py:51): a checkpoint path is user
    # input, and unpickling arbitrary objects executes code.  The reference's formats (tensors + a plain metadata dict) load in
    # this mode; a checkpoint that really needs full unpickling must be opted in explicitly.
    try:
        blob = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    except Exception as exc:
        if os.environ.get("CHESSVISION_ALLOW_PICKLE") != "1":
            raise RuntimeError(f"{checkpoint_path} does not load with weights_only=True ({type(exc).__name__}: {exc}); "
                               "set CHESSVISION_ALLOW_PICKLE=1 to unpickle it fully if you trust the file") from exc
        blob = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    metadata: dict = {}
    if isinstance(blob, dict):
        for key in ("model_state_dict", "state_dict", "model"):
            if key in blob:
                metadata = blob.get("metadata", {}) or {}
                return blob[key], metadata
    return blob, metadata


YOLO_CONVERSION = "YOLO(path).model.float().state_dict()"


def read_yolo_cls_checkpoint(checkpoint_path: str | os.PathLike) -> tuple[Mapping[str, Any], dict]:
    """(state_dict, metadata) of a YOLOv8-cls checkpoint: any layout ``read_checkpoint`` understands that holds the keys of
    ``YOLO(path).model.state_dict()``.  An ultralytics ``.pt`` pickles the model object; ``YOLO(path)`` unpickles it fully, which runs
    code from the file, so that route is taken only where ultralytics is importable AND ``CHESSVISION_ALLOW_PICKLE=1`` says the file
    is trusted -- the switch ``read_checkpoint`` asks for.  Otherwise the error prints the one-line conversion."""
    try:
        state, metadata = read_checkpoint(checkpoint_path)
        if isinstance(state, Mapping) and any(str(k).startswith("model.0.") for k in state):
            return state, metadata
        problem = "it holds no 'model.0.*' keys (an ultralytics .pt pickles the model object, not a state dict)"
    except (RuntimeError, ImportError, AttributeError) as exc:    # weights_only refused it, or full unpickling needs ultralytics' classes
        problem = f"{type(exc).__name__}: {exc}"
    convert = (f"convert it where ultralytics is installed: torch.save({YOLO_CONVERSION}, 'classifier_state.pt') and pass that file "
               "as classifier_weights")
    try:
        from ultralytics import YOLO
    except ImportError:
        raise RuntimeError(f"{checkpoint_path} is not a plain state-dict checkpoint ({problem}) and ultralytics is not importable "
                           f"here; {convert}") from None
    if os.environ.get("CHESSVISION_ALLOW_PICKLE") != "1":
        raise RuntimeError(f"{checkpoint_path} is not a plain state-dict checkpoint ({problem}); reading it through ultralytics "
                           f"unpickles it fully: set CHESSVISION_ALLOW_PICKLE=1 if you trust the file, or {convert}")
    return YOLO(str(checkpoint_path)).model.float().state_dict(), {}


def load_classifier_state(engine, arch: str, state: Mapping[str, Any]) -> None:
    """Pack ``state`` as the piece classifier ``arch`` into ``engine`` (the one place that knows which loader an id means)."""
    from .hip_backend import YOLO_CLS_ARCHS

    if arch in YOLO_CLS_ARCHS:
        engine.load_yolo_cls(state, arch)
    elif arch == "resnet18":
        engine.load_resnet18(state)
    else:
        engine.load_resnet(state, arch)


def read_classifier_checkpoint(checkpoint_path, arch: str):
    from .hip_backend import YOLO_CLS_ARCHS

    return read_yolo_cls_checkpoint(checkpoint_path) if arch in YOLO_CLS_ARCHS else read_checkpoint(checkpoint_path)


def load_model_checkpoint(model, checkpoint_path: str, device: torch.device | None = None):
    """Reference-compatible entry point (utils.py:42-86): ``model`` is a HIP model object; its engine receives the
    packed weights, ``model.metadata`` is set when the checkpoint carries one."""
    if model.model_name == "unet":
        state, metadata = read_checkpoint(checkpoint_path)
        model.engine.load_unet(state)
    else:
        # the architecture comes from the model id, never from the checkpoint (reference core.py:139-146); a mismatch fails on the
        # first key the other architecture lacks, and the message says which id the checkpoint needs
        from .hip_backend import HipBackendError

        state, metadata = read_classifier_checkpoint(checkpoint_path, model.model_name)
        try:
            load_classifier_state(model.engine, model.model_name, state)
        except HipBackendError as exc:
            found = _resnet_arch_of(state) or yolo_cls_arch(state)
            if found and found != model.model_name:
                kind = found if found.startswith("yolov8") else found + " state dict"
                raise HipBackendError(f"{exc} -- {checkpoint_path}: this is a {kind} checkpoint: pass "
                                      f"classifier_model_id={found!r}") from exc
            raise
    if metadata:
        model.metadata = metadata
    return model


def _resnet_arch_of(state: Mapping[str, Any]) -> str | None:
    """Which plain BasicBlock ResNet a state dict looks like, by the depth of its stages (error messages only)."""
    depth = []
    for layer in range(1, 5):
        blocks = {k.split(".")[1] for k in state if k.startswith(f"layer{layer}.") and k.split(".")[1].isdigit()}
        depth.append(len(blocks))
    return {(2, 2, 2, 2): "resnet18", (3, 4, 6, 3): "resnet34"}.get(tuple(depth))


_YOLO_CLS_STEM_WIDTH = {16: "yolov8n-cls", 32: "yolov8s-cls", 48: "yolov8m-cls", 64: "yolov8l-cls", 80: "yolov8x-cls"}


def yolo_cls_arch(state: Mapping[str, Any]) -> str | None:
    """Which YOLOv8-cls scale a state dict looks like, from its shapes: the stem's output channels tell the five scales apart (16 / 32 /
    48 / 64 / 80) and the number of Bottlenecks in ``model.2`` must agree (n, s: 1; m: 2; l, x: 3).  None: not a YOLOv8-cls dict.  Used for
    error messages; the architecture that is LOADED always comes from the model id."""
    stem = state.get("model.0.conv.weight") if hasattr(state, "get") else None
    shape = tuple(getattr(stem, "shape", ()))
    if len(shape) != 4:
        return None
    arch = _YOLO_CLS_STEM_WIDTH.get(int(shape[0]))
    blocks = {k.split(".")[3] for k in state if k.startswith("model.2.m.") and k.split(".")[3].isdigit()}
    want = {"n": 1, "s": 1, "m": 2, "l": 3, "x": 3}
    if arch is None or len(blocks) != want[arch[6]] or "model.9.linear.weight" not in state:
        return None
    return arch


def get_classifier_model(model_id: str = "resnet18", engine=None):
    """The piece classifier architecture (reference utils.py:32-39: timm ``model_id``, 13 classes, 1 input channel).
    ``resnet18`` and ``resnet34`` have a HIP implementation, and so have ultralytics' ``yolov8{n,s,m,l,x}-cls`` (the names the
    reference's ``train_yolo_classifier.py`` passes to ``--model``, minus ``.pt``); ``""`` / None mean ``resnet18``."""
    from .hip_backend import CLASSIFIER_ARCHS, HipBackendError, HipPieceClassifier

    arch = model_id or "resnet18"
    if arch not in CLASSIFIER_ARCHS:
        raise HipBackendError(f"classifier architecture {model_id!r} has no HIP implementation (supported: {', '.join(CLASSIFIER_ARCHS)})")
    return HipPieceClassifier(engine, arch=arch)


def get_board_extractor_model(engine=None):
    from .hip_backend import HipBoardExtractor

    return HipBoardExtractor(engine)


def ratio(a: float, b: float) -> float:
    """min/max, or -1 when either side is 0 (reference utils.py:89-93)."""
    if a == 0 or b == 0:
        return -1
    return min(a, b) / float(max(a, b))


def listdir_nohidden(path: str) -> list[str]:
    """Directory entries that do not start with a dot (public helper of the reference's ``utils.py:96-98``; its eval and
    data scripts import it from here)."""
    return [name for name in os.listdir(path) if name[:1] != "."]


def create_binary_mask(mask: NDArray[np.float32], threshold: float = 0.5) -> NDArray[np.uint8]:
    """probability > threshold -> 255 else 0 (reference utils.py:101-112)."""
    assert isinstance(mask, np.ndarray), "Mask must be a numpy array"
    assert mask.dtype == np.float32, "Mask must be float32"
    assert 0 <= threshold <= 1, "Threshold must be between 0 and 1"
    return np.where(mask > threshold, 255, 0).astype(np.uint8)


def extract_perspective(image: NDArray[np.uint8], approx: NDArray[np.float32], out_size: tuple[int, int]) -> NDArray[np.uint8]:
    """Rectify the quadrangle ``approx`` onto an ``out_size`` image: corners go to (0,0),(w,0),(w,h),(0,h)
    (reference utils.py:115-132)."""
    assert isinstance(image, np.ndarray), "Image must be a numpy array"
    assert image.dtype == np.uint8, "Image must be uint8"
    assert isinstance(approx, np.ndarray), "Approx must be a numpy array"
    assert approx.dtype == np.float32, "Approx must be float32"
    assert len(approx) == 4, "Approx must contain exactly 4 points"
    w, h = out_size
    dest = np.array(((0, 0), (w, 0), (w, h), (0, h)), np.float32)
    coeffs = classical.get_perspective_transform(np.asarray(approx, np.float32).reshape(4, 2), dest)
    return classical.warp_perspective(image, coeffs, out_size)

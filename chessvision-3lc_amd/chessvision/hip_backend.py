"""ctypes binding of ``libchessvision_hip.so`` + the model objects ChessVision plugs in.

The reference keeps two opaque callables in ``ChessVision._board_extractor`` / ``._classifier`` and only
ever does ``obj(tensor)``, ``obj.eval()``, ``obj.to(device)`` and ``hasattr(obj, "metadata")``
(reference ``chessvision/core.py:53-54,105-106,149-150,220,241``); its YOLO wrappers
(``chessvision/utils.py:205-227,257-278``) show the accepted duck type.  ``HipBoardExtractor`` and
``HipPieceClassifier`` follow that protocol and route the forward pass through the C ABI declared in
``include/chessvision_hip.h``.  PyTorch is used for device memory and streams only.

There is NO CPU fallback: if the shared library or a gfx950 device is missing, construction raises.
"""
from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path
from typing import Mapping

import numpy as np
import torch

_LIB_NAME = "libchessvision_hip.so"
PREC_F32, PREC_F16, PREC_F16X3, PREC_F16R = 0, 1, 2, 3
ABI_VERSION = 6
RESNET_ARCHS = ("resnet18", "resnet34")     # piece classifiers with a HIP implementation (cv_load_resnet)
# ultralytics YOLOv8-cls, all five scales (cv_load_yolo_cls): the names the reference's training script passes to --model, minus ".pt"
YOLO_CLS_ARCHS = ("yolov8n-cls", "yolov8s-cls", "yolov8m-cls", "yolov8l-cls", "yolov8x-cls")
CLASSIFIER_ARCHS = RESNET_ARCHS + YOLO_CLS_ARCHS
_PRECISIONS = {"f32": PREC_F32, "fp32": PREC_F32, "float32": PREC_F32, "f16": PREC_F16, "fp16": PREC_F16,
               "float16": PREC_F16, "f16x3": PREC_F16X3, "split": PREC_F16X3, "f16r": PREC_F16R}
_PREC_NAMES = {PREC_F32: "f32", PREC_F16: "f16", PREC_F16X3: "f16x3", PREC_F16R: "f16r"}


CV_ERR_NUMERIC = 5                               # include/chessvision_hip.h


class HipBackendError(RuntimeError):
    """Raised for every non-zero status of the C ABI (message = ``cv_last_error()``)."""


class NumericRangeError(HipBackendError):
    """CV_ERR_NUMERIC: a layer of an f16-based engine stored a non-finite value (an activation left the range the engine can hold, or
    a NaN reached it); the results of the call are invalid.  ``layer`` names the first such layer.  ``ChessVision.process_image`` /
    ``process_images`` / ``extract_board`` / ``classify_position`` catch it and repeat the request on an exact-f32 engine."""

    def __init__(self, message: str):
        super().__init__(message)
        self.layer = message.split("produced by '", 1)[1].split("'", 1)[0] if "produced by '" in message else "input tensor"


class _ImageResult(ctypes.Structure):             # mirrors cv_image_result_t (include/chessvision_hip.h); the pointer fields as plain
    _fields_ = [("logits", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("quadrangle", ctypes.c_float * 8),     # addresses: assigning
                ("found", ctypes.c_int32), ("board", ctypes.c_void_p), ("probabilities", ctypes.c_void_p),      # ndarray.ctypes.data costs
                ("labels", ctypes.c_void_p), ("fen", ctypes.c_char * 72), ("original_fen", ctypes.c_char * 72),   # a fifth of data_as()
                ("fixes", ctypes.c_int32 * 64), ("n_fixes", ctypes.c_int32), ("squares", ctypes.c_void_p)]


class _Param(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.POINTER(ctypes.c_float)), ("ndim", ctypes.c_int32),
                ("shape", ctypes.c_int64 * 4)]


def library_path() -> Path:
    env = os.environ.get("CHESSVISION_HIP_LIB")
    if env:
        return Path(env)
    return Path(__file__).resolve().parent.parent / "lib" / _LIB_NAME


_lib = None
_lib_lock = threading.Lock()

# (name, restype, argtypes) for every symbol include/chessvision_hip.h declares
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_fp = ctypes.POINTER(ctypes.c_float)
SYMBOLS = [
    ("cv_abi_version", _i, []),
    ("cv_last_error", ctypes.c_char_p, []),
    ("cv_device_count", _i, [ctypes.POINTER(_i)]),
    ("cv_engine_create", _i, [_i, _i, ctypes.POINTER(_vp)]),
    ("cv_engine_destroy", _i, [_vp]),
    ("cv_trim_memory", _i, [ctypes.POINTER(ctypes.c_size_t)]),
    ("cv_load_unet", _i, [_vp, ctypes.POINTER(_Param), _i]),
    ("cv_load_resnet18", _i, [_vp, ctypes.POINTER(_Param), _i]),
    ("cv_load_resnet", _i, [_vp, ctypes.c_char_p, ctypes.POINTER(_Param), _i]),
    ("cv_load_yolo_cls", _i, [_vp, ctypes.c_char_p, ctypes.POINTER(_Param), _i]),
    ("cv_engine_set_chunk", _i, [_vp, _i, _i]),
    ("cv_unet_forward", _i, [_vp, _vp, _i, _vp, _vp]),
    ("cv_resnet18_forward", _i, [_vp, _vp, _i, _vp, _vp]),
    ("cv_unet_forward_u8", _i, [_vp, _vp, _i, _vp, _vp, _f, _vp]),
    ("cv_resnet18_forward_u8", _i, [_vp, _vp, _i, _vp, _vp]),
    ("cv_softmax13", _i, [_vp, _vp, _i, _vp, _vp]),
    ("cv_embedding_dim", _i, [_vp, ctypes.c_char_p, ctypes.POINTER(_i)]),
    ("cv_unet_forward_emb", _i, [_vp, _vp, _i, _vp, _vp, _vp]),
    ("cv_unet_forward_u8_emb", _i, [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp]),
    ("cv_resnet18_forward_emb", _i, [_vp, _vp, _i, _vp, _vp, _vp]),
    ("cv_resnet18_forward_u8_emb", _i, [_vp, _vp, _i, _vp, _vp, _vp]),
    ("cv_activation_channel_means", _i, [_vp, ctypes.c_char_p, ctypes.c_char_p, _vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64), _vp]),
    ("cv_get_activation", _i, [_vp, ctypes.c_char_p, ctypes.c_char_p, _fp, ctypes.c_size_t,
                               ctypes.POINTER(ctypes.c_int64)]),
    ("cv_model_macs", _i, [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]),
    ("cv_profile_convs", _i, [_vp, ctypes.c_char_p, _vp, _i, _vp, _i, _vp, ctypes.POINTER(_f),
                              ctypes.POINTER(_i), ctypes.POINTER(_f)]),
    ("cv_profile_entry", _i, [_vp, _i, ctypes.c_char_p, _i, ctypes.POINTER(_f), ctypes.POINTER(ctypes.c_double),
                              ctypes.POINTER(_i)]),
    ("cv_op_conv2d", _i, [_vp, _vp, _i, _i, _i, _i, _fp, _i, _i, _i, _fp, _fp, _vp, _i, _vp, _vp]),
    ("cv_op_conv2d_act", _i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _fp, _i, _i, _i, _fp, _fp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    ("cv_op_conv_epilogue_ok", _i, [_i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(_i)]),
    ("cv_op_stem3x3s2", _i, [_vp, _vp, _i, _i, _i, _fp, _fp, _fp, _f, _f, _i, _vp, _vp]),
    ("cv_op_head_pool_fc", _i, [_vp, _vp, _i, _i, _i, _i, _fp, _fp, _i, _i, _vp, _vp, _vp]),
    ("cv_op_conv_transpose2x2", _i, [_vp, _vp, _i, _i, _i, _i, _fp, _i, _fp, _vp, _vp]),
    ("cv_op_outc_1x1", _i, [_vp, _vp, _i, _i, _i, _i, _fp, _fp, _f, _vp, _vp, _vp]),
    ("cv_op_maxpool2x2", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    ("cv_op_maxpool3x3s2", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    ("cv_op_upsample_bilinear2x", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    ("cv_selftest_mfma", _i, [_vp, ctypes.POINTER(_f), ctypes.POINTER(_f)]),
    ("cv_find_quadrangle", _i, [_vp, _i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_i)]),
    ("cv_find_quadrangles", _i, [_vp, _i, _i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), _i]),
    ("cv_find_contours", _i, [_vp, _i, _i, _i, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
                              ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    ("cv_resize_area_u8", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    ("cv_resize_antialias_f32", _i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    ("cv_unet_forward_mask", _i, [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp]),
    ("cv_extract_squares_u8", _i, [_vp, _vp, _i, _i, _i, ctypes.POINTER(ctypes.c_double), _vp, _vp, _vp]),
    ("cv_extract_squares_u8_dev", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    ("cv_engine_workspace_bytes", _i, [_vp, ctypes.POINTER(ctypes.c_size_t)]),
    ("cv_engine_numeric_status", _i, [_vp, _vp]),
    ("cv_get_activation_exponent", _i, [_vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(_i)]),
    ("cv_profile_entry_bytes", _i, [_vp, _i, ctypes.POINTER(ctypes.c_double)]),
    ("cv_profile_entry_kernel", _i, [_vp, _i, ctypes.c_char_p, _i]),
    ("cv_engine_export_calibration", _i, [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), _i, ctypes.POINTER(_i)]),
    ("cv_engine_import_calibration", _i, [_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32), _i, ctypes.POINTER(_i)]),
    ("cv_process_image", _i, [_vp, _vp, _vp, _i, _i, _f, _i, _i, ctypes.c_void_p, _vp]),
    ("cv_process_image_v2", _i, [_vp, _vp, _vp, _i, _i, _f, _i, _i, ctypes.c_void_p, ctypes.c_size_t, _vp]),
    ("cv_board_homographies", _i, [_fp, _i, _i, _i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    ("cv_decode_positions", _i, [_fp, _i, _i, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int8),
                                 ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    ("cv_extraction_scores", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    ("cv_extraction_scores_finish", _i, [_vp, _i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    ("cv_mask_completeness", _i, [_vp, _i, _i, ctypes.POINTER(ctypes.c_double)]),
    ("cv_mask_completenesses", _i, [_vp, _i, _i, _i, ctypes.POINTER(ctypes.c_double), _i]),
    ("cv_quadrangle_regularity", _i, [_fp, ctypes.POINTER(ctypes.c_double)]),
    ("cv_segmentation_scores", _i, [_vp, _vp, _vp, _i, _i, _f, _vp, _vp]),
    ("cv_segmentation_scores_finish", _i, [_vp, _i] + [ctypes.POINTER(ctypes.c_double)] * 6),
    ("cv_fen_labels", _i, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int8)]),
    ("cv_classification_scores", _i, [_fp, ctypes.POINTER(ctypes.c_int8), _i, _vp, _vp]),
    ("cv_resnet_forward_u8_norm", _i, [_vp, _vp, _i, _f, _f, _i, _vp, _vp, _vp]),
    ("cv_square_records", _i, [_vp, _vp, _vp, _i, _vp, _vp]),
    ("cv_square_records_finish", _i, [_vp, _i, _i, _vp]),
    ("cv_threshold_levels", _i, [_vp, _vp, _vp, _i, _i, _fp, _i, _vp, _vp, _vp]),
    ("cv_threshold_levels_finish", _i, [_vp, _i, _i] + [ctypes.POINTER(ctypes.c_double)] * 3),
    ("cv_jpeg_info", _i, [_vp, ctypes.c_size_t, _vp]),
    ("cv_jpeg_entropy_decode", _i, [_vp, ctypes.c_size_t, _vp, ctypes.c_size_t, _vp]),
    ("cv_jpeg_reconstruct_u8", _i, [_vp, _vp, _vp, _i, _vp, _i, _vp, ctypes.c_size_t, _vp, _vp]),
    ("cv_process_jpeg", _i, [_vp, _vp, _vp, ctypes.c_size_t, _f, _i, _i, ctypes.c_void_p, ctypes.c_size_t, _vp]),
    ("cv_jpeg_reconstruct_oriented_u8", _i, [_vp, _vp, _vp, _i, _vp, _i, _i, _vp, ctypes.c_size_t, _vp, _vp]),
    ("cv_process_jpeg_oriented", _i, [_vp, _vp, _vp, ctypes.c_size_t, _f, _i, _i, _i, ctypes.c_void_p, ctypes.c_size_t, _vp]),
    ("cv_jpeg_gray_header", _i, [_i, _i, _i, _vp, _vp]),
    ("cv_jpeg_gray_max_bytes", _i, [_i, _i, ctypes.POINTER(ctypes.c_size_t)]),
    ("cv_jpeg_encode_gray_u8", _i, [_vp, _vp, _i, _i, _i, _i, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    ("cv_jpeg_colour_header", _i, [_i, _i, _i, _i, _vp, _vp]),
    ("cv_jpeg_colour_max_bytes", _i, [_i, _i, _i, ctypes.POINTER(ctypes.c_size_t)]),
    ("cv_jpeg_encode_colour_u8", _i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    ("cv_embedding_neighbours_scratch_bytes", ctypes.c_size_t, [_i, _i, _i, _i]),
    ("cv_embedding_neighbours", _i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    ("cv_pacmap_plan", _i, [_i, _i, _i, _i, _i, _vp]),
    ("cv_pacmap_pairs", _i, [_vp, _vp, _i, _i, _i, _i, _i, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    ("cv_pacmap_optimise", _i, [_vp, _vp, _i, _vp, _vp, ctypes.c_int64, _i, _vp, _vp, ctypes.c_size_t, _vp]),
    ("cv_pacmap_place_plan", _i, [_i, _i, _i, _i, _vp]),
    ("cv_pacmap_basis_scale", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, ctypes.c_size_t, _vp]),
    ("cv_pacmap_place_pairs", _i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    ("cv_pacmap_place", _i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp]),
]
NEIGHBOURS_EXCLUDE_SELF, NEIGHBOURS_EXACT_ONLY = 1, 2
# cv_neighbour_stats_t (include/chessvision_hip.h): eight int32
NEIGHBOUR_STATS = ("query_rows", "certified_rows", "exact_rows", "nonfinite_query_rows", "nonfinite_corpus_rows")
# cv_pacmap_stats_t: the neighbour record, then two int64 and two int32
PACMAP_STATS = np.dtype({"names": ["neighbours", "mid_near_draws", "further_draws", "draw_overflow", "candidates"],
                         "formats": [("<i4", (8,)), "<i8", "<i8", "<i4", "<i4"], "offsets": [0, 32, 40, 48, 52], "itemsize": 64})


class PacmapPlan(ctypes.Structure):
    """cv_pacmap_plan_t"""
    _fields_ = [(name, ctypes.c_int32) for name in ("n", "c", "n_neighbors", "n_mn", "n_fp", "candidates")] + \
               [("pairs_scratch_bytes", ctypes.c_uint64), ("optimise_scratch_bytes", ctypes.c_uint64)]


class PacmapPlacePlan(ctypes.Structure):
    """cv_pacmap_place_plan_t"""
    _fields_ = [(name, ctypes.c_int32) for name in ("q", "n", "c", "n_neighbors", "candidates", "reserved")] + \
               [("scale_scratch_bytes", ctypes.c_uint64), ("pairs_scratch_bytes", ctypes.c_uint64)]

# cv_score_record_t (include/chessvision_hip.h): one 64-byte record per image
SCORE_RECORD = np.dtype({"names": ["hist", "above_half", "n_nan", "top_sum", "top_count", "reserved"],
                         "formats": [("<i4", (10,)), "<i4", "<i4", "<f8", "<i4", "<i4"],
                         "offsets": [0, 40, 44, 48, 56, 60], "itemsize": 64})
_TRANSFORMS = {"none": 0, "sigmoid": 1}
# cv_seg_record_t, cv_square_score_t, cv_board_score_t (include/chessvision_hip.h)
SEG_RECORD = np.dtype({"names": ["n_label", "n_pred", "n_both", "n_nan", "bce_sum", "sig_sum", "sig_label_sum", "count", "reserved"],
                       "formats": ["<i4", "<i4", "<i4", "<i4", "<f8", "<f8", "<f8", "<i4", ("<i4", (5,))],
                       "offsets": [0, 4, 8, 12, 16, 24, 32, 40, 44], "itemsize": 64})
# cv_level_record_t (include/chessvision_hip.h): one 320-byte record per image, CV_MAX_THRESHOLDS = 32
MAX_THRESHOLDS = 32
LEVEL_RECORD = np.dtype({"names": ["count", "n_thresholds", "n_nan", "hist", "reserved"],
                         "formats": ["<i4", "<i4", "<i4", ("<i4", (2, MAX_THRESHOLDS + 1)), ("<i4", (11,))],
                         "offsets": [0, 4, 8, 12, 276], "itemsize": 320})
SQUARE_SCORE = np.dtype({"names": ["predicted", "rank", "confidence", "reserved", "loss"],
                         "formats": ["<i4", "<i4", "<f4", "<i4", "<f8"], "offsets": [0, 4, 8, 12, 16], "itemsize": 24})
BOARD_SCORE = np.dtype({"names": ["hits", "n_nan", "mean_loss"], "formats": [("<i4", (13,)), "<i4", "<f8"],
                        "offsets": [0, 52, 56], "itemsize": 64})
# cv_square_record_t, cv_squares_summary_t (include/chessvision_hip.h)
SQUARE_RECORD = np.dtype({"names": ["predicted", "rank", "label", "flags", "confidence", "loss", "max_logit", "logsumexp"],
                          "formats": ["<i4", "<i4", "<i4", "<i4", "<f4", "<f4", "<f4", "<f4"], "itemsize": 32})
SQUARES_SUMMARY = np.dtype({"names": ["n", "n_labelled", "n_correct", "n_nan", "hits", "confusion", "loss_sum", "val_loss", "val_acc",
                                      "n_batches"],
                            "formats": ["<i8", "<i8", "<i8", "<i8", ("<i8", (13,)), ("<i8", (13, 13)), "<f8", "<f8", "<f8", "<i8"]})


def trim_memory() -> int:
    """Hand the blocks of closed engines, which the library keeps for the next load, back to the driver (``cv_trim_memory``);
    returns the bytes freed.  The counterpart of ``torch.cuda.empty_cache()`` for this library's own allocations."""
    n = ctypes.c_size_t(0)
    _check(load_library().cv_trim_memory(ctypes.byref(n)))
    return int(n.value)


def load_library():
    """dlopen the C-ABI library (built by ``__graft_entry__.build()``); raises if it is missing."""
    global _lib
    with _lib_lock:
        if _lib is None:
            path = library_path()
            if not path.exists():
                raise HipBackendError(
                    f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
            lib = ctypes.CDLL(str(path))
            lib.cv_abi_version.restype = ctypes.c_int
            lib.cv_abi_version.argtypes = []
            found = lib.cv_abi_version()
            if found != ABI_VERSION:               # before binding the rest: a stale build fails with this, not an AttributeError
                raise HipBackendError(f"{path}: ABI version {found}, this package needs {ABI_VERSION} -- rebuild the library "
                                      "(`python -c 'import __graft_entry__ as g; g.build()'`)")
            for name, restype, argtypes in SYMBOLS:
                fn = getattr(lib, name)            # AttributeError if the export is missing
                fn.restype = restype
                fn.argtypes = argtypes
            _lib = lib
    return _lib


def _check(status: int) -> None:
    if status != 0:
        msg = load_library().cv_last_error()
        text = f"[cv status {status}] {msg.decode(errors='replace') if msg else 'unknown error'}"
        raise NumericRangeError(text) if status == CV_ERR_NUMERIC else HipBackendError(text)


def _stream_ptr(device: torch.device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t: torch.Tensor) -> int:
    return int(t.data_ptr())


def _np_f32(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().to("cpu", torch.float32).numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _as_param_table(state_dict: Mapping[str, object]):
    keep = []                                   # keeps numpy buffers alive during the call
    entries = []
    for key, value in state_dict.items():
        if key.endswith("num_batches_tracked"):
            continue
        arr = _np_f32(value)
        if arr.ndim > 4:
            raise HipBackendError(f"state-dict entry {key} has {arr.ndim} dims")
        keep.append(arr)
        shape = (ctypes.c_int64 * 4)(*(list(arr.shape) + [0] * (4 - arr.ndim)))
        entries.append(_Param(key.encode(), arr.ctypes.data_as(_fp), arr.ndim, shape))
    table = (_Param * len(entries))(*entries)
    return table, len(entries), keep


def find_quadrangle(mask: np.ndarray):
    """Binary mask (H, W) uint8 -> (4,1,2) int32 quadrangle in the reference's vertex order, or None.
    Host-side C++ (csrc/contour.cpp); needs neither a GPU nor an engine.  Same result as
    ``ChessVision._find_quadrangle`` (which stays the readable numpy restatement and the test checker)."""
    lib = load_library()
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    if m.ndim != 2:
        raise HipBackendError("find_quadrangle expects a 2-D uint8 mask")
    quad = (ctypes.c_int32 * 8)()
    found = _i(0)
    _check(lib.cv_find_quadrangle(m.ctypes.data_as(_vp), m.shape[0], m.shape[1], quad, ctypes.byref(found)))
    if not found.value:
        return None
    return np.array(list(quad), dtype=np.int32).reshape(4, 1, 2)


def find_contours(mask: np.ndarray, tc89: bool = True):
    """``cv2.findContours(mask, RETR_CCOMP, CHAIN_APPROX_TC89_KCOS if tc89 else CHAIN_APPROX_NONE)[0]`` (reference core.py:360)
    from the native contour stage: list of (n,1,2) int32 contours in OpenCV's order, and the list of their hole flags."""
    lib = load_library()
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    if m.ndim != 2:
        raise HipBackendError("find_contours expects a 2-D uint8 mask")
    h, w = m.shape
    cap_pts, cap_c = 4 * h * w + 16, h * w + 16
    xy = np.zeros((cap_pts, 2), dtype=np.int32)
    counts = np.zeros(cap_c, dtype=np.int32)
    holes = np.zeros(cap_c, dtype=np.int32)
    n = ctypes.c_int64(0)
    i32p = ctypes.POINTER(ctypes.c_int32)
    _check(lib.cv_find_contours(m.ctypes.data_as(_vp), h, w, 1 if tc89 else 0, xy.ctypes.data_as(i32p), cap_pts,
                                counts.ctypes.data_as(i32p), holes.ctypes.data_as(i32p), cap_c, ctypes.byref(n)))
    out, at = [], 0
    for k in range(n.value):
        out.append(xy[at:at + counts[k]].reshape(-1, 1, 2).copy())
        at += int(counts[k])
    return out, [bool(v) for v in holes[:n.value]]


def find_quadrangles(masks: np.ndarray, n_threads: int = 0) -> list:
    """(N,H,W) uint8 masks -> list of (4,1,2) int32 quadrangles / None, on native host threads (GIL released)."""
    lib = load_library()
    m = np.ascontiguousarray(masks, dtype=np.uint8)
    if m.ndim != 3:
        raise HipBackendError("find_quadrangles expects (N,H,W) uint8 masks")
    n = m.shape[0]
    quads = np.zeros((n, 8), dtype=np.int32)
    found = np.zeros(n, dtype=np.int32)
    if n:
        _check(lib.cv_find_quadrangles(m.ctypes.data_as(_vp), n, m.shape[1], m.shape[2],
                                       quads.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                       found.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(n_threads)))
    return [quads[i].reshape(4, 1, 2).copy() if found[i] else None for i in range(n)]


def scores_finish(records: np.ndarray):
    """(N,) ``SCORE_RECORD`` array -> (confidence, distribution), two (N,) float64 arrays (``cv_extraction_scores_finish``):
    ``np.mean(np.abs(np.sort(v)[-k:] - 0.5)) * 2`` and ``1 - entropy(hist / hist.sum()) / log2(10)`` of the scored values."""
    lib = load_library()
    r = np.ascontiguousarray(records, dtype=SCORE_RECORD).reshape(-1)
    conf, dist = np.zeros(r.size, dtype=np.float64), np.zeros(r.size, dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    if r.size:
        _check(lib.cv_extraction_scores_finish(r.ctypes.data_as(_vp), int(r.size), conf.ctypes.data_as(dp), dist.ctypes.data_as(dp)))
    return conf, dist


def segmentation_scores_finish(records: np.ndarray) -> dict:
    """(N,) ``SEG_RECORD`` array -> {"bce", "dice_loss", "loss", "dice", "iou", "pixel_accuracy"}: (N,) float64 arrays
    (``cv_segmentation_scores_finish``; the formulas are in include/chessvision_hip.h)."""
    lib = load_library()
    r = np.ascontiguousarray(records, dtype=SEG_RECORD).reshape(-1)
    names = ("bce", "dice_loss", "loss", "dice", "iou", "pixel_accuracy")
    out = {k: np.zeros(r.size, dtype=np.float64) for k in names}
    dp = ctypes.POINTER(ctypes.c_double)
    if r.size:
        _check(lib.cv_segmentation_scores_finish(r.ctypes.data_as(_vp), int(r.size), *(out[k].ctypes.data_as(dp) for k in names)))
    return out


def threshold_levels_finish(records: np.ndarray, labels_present: bool = True) -> dict:
    """(N,) ``LEVEL_RECORD`` array -> {"dice", "iou", "pixel_accuracy"}: (N,T) float64 arrays, column k = the score of
    ``segmentation_scores_finish`` at the k-th (ascending) threshold (``cv_threshold_levels_finish``)."""
    lib = load_library()
    r = np.ascontiguousarray(records, dtype=LEVEL_RECORD).reshape(-1)
    t = int(r["n_thresholds"][0]) if r.size else 0
    names = ("dice", "iou", "pixel_accuracy")
    out = {k: np.zeros((r.size, max(t, 0)), dtype=np.float64) for k in names}
    dp = ctypes.POINTER(ctypes.c_double)
    if r.size:
        if not 1 <= t <= MAX_THRESHOLDS:
            raise HipBackendError(f"threshold_levels_finish: a record claims {t} thresholds")
        _check(lib.cv_threshold_levels_finish(r.ctypes.data_as(_vp), int(r.size), 1 if labels_present else 0,
                                              *(out[k].ctypes.data_as(dp) for k in names)))
    return out


def square_records_finish(records: np.ndarray, batch_size: int = 0) -> dict:
    """(N,) ``SQUARE_RECORD`` array -> the aggregate of the reference's ``validate()`` as a dict (``cv_square_records_finish``):
    n, n_labelled, n_correct, n_nan, hits (13,), confusion (13,13) true x predicted, loss_sum, val_loss (mean over consecutive batches
    of ``batch_size`` of each batch's mean loss; <= 0: one batch), val_acc (percent), n_batches."""
    lib = load_library()
    r = np.ascontiguousarray(records, dtype=SQUARE_RECORD).reshape(-1)
    out = np.zeros(1, dtype=SQUARES_SUMMARY)
    _check(lib.cv_square_records_finish(r.ctypes.data_as(_vp) if r.size else None, int(r.size), int(batch_size), out.ctypes.data_as(_vp)))
    o = out[0]
    return {k: (o[k].copy() if o[k].ndim else o[k].item()) for k in SQUARES_SUMMARY.names}


def fen_labels(fen: str) -> np.ndarray:
    """Piece-placement field of a FEN -> (64,) int8 class indices in a8..h1 order (``cv_fen_labels``); ``HipBackendError`` naming
    what is wrong with a malformed placement."""
    lib = load_library()
    labels = np.zeros(64, dtype=np.int8)
    _check(lib.cv_fen_labels(str(fen).encode(), labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int8))))
    return labels


def classification_scores(probabilities: np.ndarray, labels: np.ndarray):
    """(N,64,13) float32 probabilities and (N,64) true class indices, given per row -> (per_square (N,64) ``SQUARE_SCORE``, per_board
    (N,) ``BOARD_SCORE``) in one native call (``cv_classification_scores``, csrc/position.cpp)."""
    lib = load_library()
    p = np.ascontiguousarray(probabilities, dtype=np.float32)
    if p.ndim != 3 or p.shape[1:] != (64, 13):
        raise HipBackendError("classification_scores expects (N,64,13) float32 probabilities")
    t = np.ascontiguousarray(labels, dtype=np.int8)
    if t.shape != p.shape[:2]:
        raise HipBackendError("classification_scores expects one label per row of the probabilities, (N,64)")
    n = p.shape[0]
    per_square, per_board = np.zeros((n, 64), dtype=SQUARE_SCORE), np.zeros(n, dtype=BOARD_SCORE)
    if n:
        _check(lib.cv_classification_scores(p.ctypes.data_as(_fp), t.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), n,
                                            per_square.ctypes.data_as(_vp), per_board.ctypes.data_as(_vp)))
    return per_square, per_board


def mask_completeness(mask: np.ndarray) -> float:
    """Binary mask (H, W) uint8 (0 / non-0) -> foreground pixels of the whole mask / pixels of the filled outer border of its largest
    8-connected component (``cv_mask_completeness``); 0.0 for an empty mask.  Host-side C++; needs neither a GPU nor an engine."""
    lib = load_library()
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    if m.ndim != 2:
        raise HipBackendError("mask_completeness expects a 2-D uint8 mask")
    score = ctypes.c_double(0.0)
    _check(lib.cv_mask_completeness(m.ctypes.data_as(_vp), m.shape[0], m.shape[1], ctypes.byref(score)))
    return float(score.value)


def mask_completenesses(masks: np.ndarray, n_threads: int = 0) -> np.ndarray:
    """(N,H,W) uint8 masks -> (N,) float64 completeness scores on native host threads (GIL released)."""
    lib = load_library()
    m = np.ascontiguousarray(masks, dtype=np.uint8)
    if m.ndim != 3:
        raise HipBackendError("mask_completenesses expects (N,H,W) uint8 masks")
    scores = np.zeros(m.shape[0], dtype=np.float64)
    if m.shape[0]:
        _check(lib.cv_mask_completenesses(m.ctypes.data_as(_vp), m.shape[0], m.shape[1], m.shape[2],
                                          scores.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(n_threads)))
    return scores


def quadrangle_regularity(quad) -> float:
    """Four (x, y) vertices in the order given (any array of 8 numbers, e.g. (4,1,2)), or None -> 1 - 0.5 std(sides) / mean(sides)
    - 0.5 std(interior angles) / (pi / 2); 0.0 for None (``cv_quadrangle_regularity``)."""
    lib = load_library()
    score = ctypes.c_double(0.0)
    if quad is None:
        _check(lib.cv_quadrangle_regularity(None, ctypes.byref(score)))
    else:
        q = np.ascontiguousarray(quad, dtype=np.float32).reshape(-1)
        if q.size != 8:
            raise HipBackendError("quadrangle_regularity expects four (x, y) vertices")
        _check(lib.cv_quadrangle_regularity(q.ctypes.data_as(_fp), ctypes.byref(score)))
    return float(score.value)


def board_homographies(quads: np.ndarray, out_size=(512, 512), want_forward: bool = False):
    """(N,4,2) float32 quadrangles (source-image pixels, the reference's TR, TL, BL, BR order) -> (N,3,3) float64 INVERSE
    matrices (board pixel -> source pixel) of the warp ``utils.extract_perspective`` performs (reference utils.py:115-132), computed
    in OpenCV's order of operations by csrc/homography.cpp; with ``want_forward`` also the getPerspectiveTransform matrices.
    Bit-identical to ``classical.invert3(classical.get_perspective_transform(q, dest))``.  Needs neither a GPU nor an engine."""
    lib = load_library()
    q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 8)
    n = q.shape[0]
    inv = np.zeros((n, 3, 3), dtype=np.float64)
    fwd = np.zeros((n, 3, 3), dtype=np.float64) if want_forward else None
    dp = ctypes.POINTER(ctypes.c_double)
    if n:
        _check(lib.cv_board_homographies(q.ctypes.data_as(_fp), n, int(out_size[0]), int(out_size[1]),
                                         fwd.ctypes.data_as(dp) if want_forward else None, inv.ctypes.data_as(dp)))
    return (inv, fwd) if want_forward else inv


def process_image_native(unet_engine: "HipEngine", classifier_engine: "HipEngine", image: np.ndarray, threshold: float = 0.5,
                         flip: bool = False, fallback_quad: bool = False, stream: int | None = None) -> dict:
    """One host image through ``cv_process_image`` (the native form of ``ChessVision.process_image``, reference core.py:152-195):
    returns {"logits" (256,256) f32, "mask" (256,256) u8, "found", and when found "quadrangle" (4,1,2) f32, "board" (512,512) u8,
    "probabilities" (64,13) f32, "squares" (64,64,64,1) u8, "fen", "original_fen", "fixes" [(square index, original class, corrected class)]}."""
    lib = load_library()
    img = np.ascontiguousarray(image, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise HipBackendError("process_image_native expects an (H,W,3) uint8 image")
    res, arrays = _image_result_buffers()
    _check(lib.cv_process_image_v2(unet_engine._h, classifier_engine._h, img.ctypes.data, img.shape[0], img.shape[1],
                                   float(threshold), int(bool(flip)), int(bool(fallback_quad)), ctypes.byref(res), ctypes.sizeof(res),
                                   _stream_ptr(unet_engine.device) if stream is None else stream))    # stream: a request slot's own HIP stream
    return _image_result_dict(res, arrays)


def process_jpeg_native(unet_engine: "HipEngine", classifier_engine: "HipEngine", blob, threshold: float = 0.5, flip: bool = False,
                        fallback_quad: bool = False, stream: int | None = None, apply_orientation: bool = False) -> dict:
    """One JPEG stream through ``cv_process_jpeg``: ``process_image_native`` with the decode behind the C ABI as well (Huffman stage on
    this thread into the engine's page-locked block, reconstruction on the device).  Same dict.  ``apply_orientation``: the call is
    ``cv_process_jpeg_oriented``, which reconstructs the photo as its EXIF orientation tag turns it."""
    lib = load_library()
    blob = bytes(blob)
    res, arrays = _image_result_buffers()
    head = (unet_engine._h, classifier_engine._h, blob, len(blob), float(threshold), int(bool(flip)), int(bool(fallback_quad)))
    tail = (ctypes.byref(res), ctypes.sizeof(res), _stream_ptr(unet_engine.device) if stream is None else stream)
    status = lib.cv_process_jpeg_oriented(*head, 1, *tail) if apply_orientation else lib.cv_process_jpeg(*head, *tail)
    _check(status)
    return _image_result_dict(res, arrays)


def _image_result_buffers():
    logits = np.empty((256, 256), np.float32)
    mask = np.empty((256, 256), np.uint8)
    board = np.empty((512, 512), np.uint8)
    probs = np.empty((64, 13), np.float32)
    squares = np.empty((64, 64, 64, 1), np.uint8)           # PositionResult.squares, cut on the native side (-10 us against the numpy reshape)
    res = _ImageResult()
    res.logits, res.mask, res.board = logits.ctypes.data, mask.ctypes.data, board.ctypes.data
    res.probabilities, res.squares, res.labels = probs.ctypes.data, squares.ctypes.data, None
    return res, (logits, mask, board, probs, squares)


def _image_result_dict(res, arrays) -> dict:
    logits, mask, board, probs, squares = arrays
    out = {"logits": logits, "mask": mask, "found": bool(res.found)}
    if res.found:
        out.update(quadrangle=np.frombuffer(res.quadrangle, dtype=np.float32).reshape(4, 1, 2).copy(), board=board, probabilities=probs, squares=squares,
                   fen=res.fen.decode(), original_fen=res.original_fen.decode(),
                   fixes=[(int(res.fixes[4 * i + 1]), int(res.fixes[4 * i + 2]), int(res.fixes[4 * i + 3])) for i in range(res.n_fixes)])
    return out


def jpeg_gray_max_bytes(h: int, w: int) -> int:
    """The largest file ``HipEngine.jpeg_encode_gray`` can write for an h x w image (``cv_jpeg_gray_max_bytes``)."""
    v = ctypes.c_size_t(0)
    _check(load_library().cv_jpeg_gray_max_bytes(int(h), int(w), ctypes.byref(v)))
    return int(v.value)


def jpeg_gray_header(h: int, w: int, quality: int = 95):
    """``(header, qtable)``: the 328 bytes libjpeg writes in front of a gray image's entropy-coded segment and the (64,) uint16
    quantisation table in natural order (``cv_jpeg_gray_header``; host only)."""
    header, qt = np.zeros(328, np.uint8), np.zeros(64, np.uint16)
    _check(load_library().cv_jpeg_gray_header(int(h), int(w), int(quality), header.ctypes.data, qt.ctypes.data))
    return header.tobytes(), qt


JPEG_SUBSAMPLINGS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}          # CV_JPEG_SUB_* (include/chessvision_hip.h)


def _jpeg_subsampling(subsampling) -> int:
    from .jpeg import check_subsampling
    check_subsampling(subsampling)
    return JPEG_SUBSAMPLINGS[subsampling]


def jpeg_colour_max_bytes(h: int, w: int, subsampling: str = "4:2:0") -> int:
    """The largest file ``HipEngine.jpeg_encode_colour`` can write for an h x w image (``cv_jpeg_colour_max_bytes``)."""
    v = ctypes.c_size_t(0)
    _check(load_library().cv_jpeg_colour_max_bytes(int(h), int(w), _jpeg_subsampling(subsampling), ctypes.byref(v)))
    return int(v.value)


def jpeg_colour_header(h: int, w: int, quality: int = 95, subsampling: str = "4:2:0"):
    """``(header, qtables)``: the 623 bytes libjpeg writes in front of a colour image's entropy-coded segment and the (2, 64) uint16
    quantisation tables, luma and chroma, in natural order (``cv_jpeg_colour_header``; host only)."""
    header, qt = np.zeros(623, np.uint8), np.zeros((2, 64), np.uint16)
    _check(load_library().cv_jpeg_colour_header(int(h), int(w), int(quality), _jpeg_subsampling(subsampling), header.ctypes.data,
                                                qt.ctypes.data))
    return header.tobytes(), qt


def decode_positions(probabilities: np.ndarray, flip: bool = False):
    """(N,64,13) float32 class probabilities -> (fens, original_fens, labels (N,64) int8, fixes) for the whole job in one
    native call (csrc/position.cpp): per-square argmax, the pawn rule and both FEN strings, exactly as
    ``ChessVision.process_position_probabilities`` computes them per board.  ``fixes`` is a list of
    (board, square index, original class index, corrected class index).  Needs neither a GPU nor an engine."""
    lib = load_library()
    p = np.ascontiguousarray(probabilities, dtype=np.float32)
    if p.ndim != 3 or p.shape[1:] != (64, 13):
        raise HipBackendError("decode_positions expects (N,64,13) float32 probabilities")
    n = p.shape[0]
    fen = ctypes.create_string_buffer(max(1, n * 72))
    orig = ctypes.create_string_buffer(max(1, n * 72))
    labels = np.zeros((n, 64), dtype=np.int8)
    fixes = np.zeros((max(1, n * 16), 4), dtype=np.int32)
    n_fixes = ctypes.c_int32(0)
    if n:
        _check(lib.cv_decode_positions(p.ctypes.data_as(_fp), n, int(bool(flip)), fen, orig,
                                       labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)),
                                       fixes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(n_fixes)))
    raw_f, raw_o = fen.raw, orig.raw
    fens = [raw_f[i * 72:(i + 1) * 72].split(b"\0", 1)[0].decode() for i in range(n)]
    origs = [raw_o[i * 72:(i + 1) * 72].split(b"\0", 1)[0].decode() for i in range(n)]
    return fens, origs, labels, [tuple(int(v) for v in fixes[i]) for i in range(n_fixes.value)]


class HipEngine:
    """One engine = one device + one arithmetic precision + packed weights + workspace."""

    def __init__(self, device: torch.device | str | int | None = None, precision: str = "f16",
                 unet_chunk: int = 0, resnet_chunk: int = 0):
        self._lib = load_library()
        if not torch.cuda.is_available():
            raise HipBackendError("no ROCm device visible to PyTorch: the HIP backend has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise HipBackendError(f"HIP backend needs a cuda(ROCm) device, got {dev}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if precision not in _PRECISIONS:
            raise HipBackendError(f"precision must be one of {sorted(_PRECISIONS)}")
        self.device = dev
        self.precision = _PREC_NAMES[_PRECISIONS[precision]]
        self._h = ctypes.c_void_p()
        _check(self._lib.cv_engine_create(dev.index, _PRECISIONS[precision], ctypes.byref(self._h)))
        # chunk = images / squares per pass (0 = library default 64 / 16384).  The activation workspace is elastic: it is
        # allocated for the largest batch seen so far (at most one chunk), so a single-image server stays under 1 GB.
        unet_chunk = int(unet_chunk or os.environ.get("CHESSVISION_HIP_UNET_CHUNK", "0") or 0)
        resnet_chunk = int(resnet_chunk or os.environ.get("CHESSVISION_HIP_RESNET_CHUNK", "0") or 0)
        if unet_chunk or resnet_chunk:
            _check(self._lib.cv_engine_set_chunk(self._h, unet_chunk, resnet_chunk))
        self.resnet_chunk = resnet_chunk or 16384        # squares per pass of the classifier (the library's default) ...
        while self.precision == "f32" and self.resnet_chunk > 1 and self.resnet_chunk * 34 * 34 * 64 * 4 >= 1 << 32:
            self.resnet_chunk //= 2                      # ... which the f32 engine halves for its stem output (resnet.cpp: resnet_load)
        self.has_unet = False
        self.has_resnet = False
        self.classifier_arch: str | None = None      # "resnet18" | "resnet34" | "yolov8m-cls" | ... once a classifier is loaded

    # -- lifecycle ------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._lib.cv_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights --------------------------------------------------------------------------------
    def load_unet(self, state_dict: Mapping[str, object]) -> None:
        table, n, keep = _as_param_table(state_dict)
        _check(self._lib.cv_load_unet(self._h, table, n))
        del keep
        self.has_unet = True

    def load_resnet(self, state_dict: Mapping[str, object], arch: str = "resnet18") -> None:
        """Pack a timm ResNet piece classifier (in_chans=1, 13 classes): ``arch`` is "resnet18" or "resnet34" and decides which keys
        the state dict must hold -- exactly those, with their shapes.  The engine holds one ResNet; ``resnet18_forward`` and
        ``resnet18_forward_u8`` run whichever is loaded."""
        if arch not in RESNET_ARCHS:
            raise HipBackendError(f"ResNet architecture must be one of {RESNET_ARCHS}, got {arch!r}")
        table, n, keep = _as_param_table(state_dict)
        _check(self._lib.cv_load_resnet(self._h, arch.encode(), table, n))
        del keep
        self.has_resnet = True
        self.classifier_arch = arch

    def load_resnet18(self, state_dict: Mapping[str, object]) -> None:
        self.load_resnet(state_dict, "resnet18")

    def load_yolo_cls(self, state_dict: Mapping[str, object], arch: str) -> None:
        """Pack an ultralytics YOLOv8-cls piece classifier (13 classes): ``arch`` is one of ``YOLO_CLS_ARCHS`` and decides which keys
        the state dict must hold -- those of ``YOLO(path).model.state_dict()``, as trained or as ``model.fuse()`` leaves them.  It takes
        the engine's classifier slot: the ``resnet18_forward*`` entries then run it (embedding: (N,1280), the pooled ``model.9.conv``
        output).  Precisions f32, f16x3 and f16; f16r is refused."""
        if arch not in YOLO_CLS_ARCHS:
            raise HipBackendError(f"YOLOv8-cls architecture must be one of {YOLO_CLS_ARCHS}, got {arch!r}")
        table, n, keep = _as_param_table(state_dict)
        _check(self._lib.cv_load_yolo_cls(self._h, arch.encode(), table, n))
        del keep
        self.has_resnet = True                           # "the classifier slot is filled": what the pipeline entry points ask
        self.classifier_arch = arch

    # -- forward ----------------------------------------------------------------------------------
    def _dev_f32(self, x: torch.Tensor, shape_tail) -> torch.Tensor:
        if not isinstance(x, torch.Tensor):
            raise HipBackendError("input must be a torch.Tensor")
        if tuple(x.shape[1:]) != tuple(shape_tail):
            raise HipBackendError(f"input shape {tuple(x.shape)} != (N,{','.join(map(str, shape_tail))})")
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def check_numerics(self) -> None:
        """Synchronise the current stream and raise ``HipBackendError`` naming the first layer that produced a non-finite
        value since the last check (f16 range exceeded, NaN in the input); re-arms the guard."""
        _check(self._lib.cv_engine_numeric_status(self._h, _stream_ptr(self.device)))

    def export_calibration(self, model: str) -> np.ndarray:
        """The load-time range calibration of ``model`` ("unet" | the loaded ResNet's architecture) as an int32 vector (two exponents
        per tensor)."""
        n = _i()
        _check(self._lib.cv_engine_export_calibration(self._h, model.encode(), None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        _check(self._lib.cv_engine_export_calibration(self._h, model.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                      n.value, ctypes.byref(n)))
        return out

    def import_calibration(self, model: str, exponents: np.ndarray) -> bool:
        """Set the tensor exponents of ``model`` (a vector from ``export_calibration`` of an engine with the same precision and
        checkpoint layout); True when anything changed."""
        e = np.ascontiguousarray(exponents, dtype=np.int32)
        changed = _i()
        _check(self._lib.cv_engine_import_calibration(self._h, model.encode(), e.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                      int(e.size), ctypes.byref(changed)))
        return bool(changed.value)

    def workspace_bytes(self) -> int:
        v = ctypes.c_size_t()
        _check(self._lib.cv_engine_workspace_bytes(self._h, ctypes.byref(v)))
        return int(v.value)

    def embedding_dim(self, model: str) -> int:
        """Channels of ``model``'s embedding (``cv_embedding_dim``): "unet" 1024 (transposed-conv variant) or 512 (bilinear), the
        loaded ResNet 512."""
        v = _i()
        _check(self._lib.cv_embedding_dim(self._h, model.encode(), ctypes.byref(v)))
        return int(v.value)

    def _embedding_out(self, model: str, n: int) -> torch.Tensor:
        return torch.empty((n, self.embedding_dim(model)), dtype=torch.float32, device=self.device)

    def unet_forward(self, x: torch.Tensor, check: bool = True, want_embedding: bool = False):
        """(B,3,256,256) float32 in [0,1] -> (B,1,256,256) float32 logits (device tensor).  ``check`` consults the
        numeric guard (synchronises, like the ``.cpu()`` the reference does next); throughput loops pass False and call
        ``check_numerics()`` once at the end.  ``want_embedding``: -> (logits, embedding (B,C) float32 device tensor), the channel
        means of the bottleneck (the reference's hook at ``named_modules()[52]``), pooled inside the forward."""
        x = self._dev_f32(x, (3, 256, 256))
        out = torch.empty((x.shape[0], 1, 256, 256), dtype=torch.float32, device=self.device)
        if want_embedding:
            emb = self._embedding_out("unet", x.shape[0])
            _check(self._lib.cv_unet_forward_emb(self._h, _ptr(x), x.shape[0], _ptr(out), _ptr(emb), _stream_ptr(self.device)))
        else:
            _check(self._lib.cv_unet_forward(self._h, _ptr(x), x.shape[0], _ptr(out), _stream_ptr(self.device)))
        if check:
            self.check_numerics()
        return (out, emb) if want_embedding else out

    def resnet18_forward(self, x: torch.Tensor, check: bool = True, want_embedding: bool = False):
        """(N,1,64,64) float32 in [0,1] -> (N,13) float32 logits (device tensor) of the loaded ResNet (18 or 34).
        ``want_embedding``: -> (logits, embedding (N,512) float32 device tensor), the globally pooled ``layer4`` output (the
        reference's hook at ``named_modules()[90]``, ``global_pool``)."""
        x = self._dev_f32(x, (1, 64, 64))
        out = torch.empty((x.shape[0], 13), dtype=torch.float32, device=self.device)
        if want_embedding:
            emb = self._embedding_out(self.classifier_arch or "resnet18", x.shape[0])
            _check(self._lib.cv_resnet18_forward_emb(self._h, _ptr(x), x.shape[0], _ptr(out), _ptr(emb), _stream_ptr(self.device)))
        else:
            _check(self._lib.cv_resnet18_forward(self._h, _ptr(x), x.shape[0], _ptr(out), _stream_ptr(self.device)))
        if check:
            self.check_numerics()
        return (out, emb) if want_embedding else out

    def unet_forward_u8(self, x_u8: torch.Tensor, threshold: float = 0.5, want_mask: bool = True, want_embedding: bool = False):
        """(B,256,256,3) uint8 HWC -> (logits (B,1,256,256) f32, mask (B,256,256) u8 | None); with ``want_embedding`` the (B,C)
        float32 bottleneck embedding is appended."""
        if x_u8.dtype != torch.uint8 or tuple(x_u8.shape[1:]) != (256, 256, 3):
            raise HipBackendError("unet_forward_u8 expects (B,256,256,3) uint8")
        x_u8 = x_u8.to(self.device).contiguous()
        b = x_u8.shape[0]
        logits = torch.empty((b, 1, 256, 256), dtype=torch.float32, device=self.device)
        mask = torch.empty((b, 256, 256), dtype=torch.uint8, device=self.device) if want_mask else None
        if want_embedding:
            emb = self._embedding_out("unet", b)
            _check(self._lib.cv_unet_forward_u8_emb(self._h, _ptr(x_u8), b, _ptr(logits), _ptr(mask) if want_mask else None,
                                                    float(threshold), _ptr(emb), _stream_ptr(self.device)))
            return logits, mask, emb
        _check(self._lib.cv_unet_forward_u8(self._h, _ptr(x_u8), b, _ptr(logits), _ptr(mask) if want_mask else None,
                                            float(threshold), _stream_ptr(self.device)))
        return logits, mask

    def unet_forward_mask(self, x: torch.Tensor, threshold: float = 0.5, want_mask: bool = True, want_embedding: bool = False):
        """The float-input sibling of ``unet_forward_u8``: (B,3,256,256) float32 NCHW in [0,1] (what ``resize_antialias_f32``
        writes) -> (logits (B,1,256,256) f32, mask (B,256,256) u8 | None); with ``want_embedding`` the (B,C) float32 bottleneck
        embedding is appended.  Logits and embedding are ``unet_forward``'s bit for bit.  Like ``unet_forward_u8`` it does not
        consult the numeric guard: the batched pipeline calls ``check_numerics()`` once per call."""
        x = self._dev_f32(x, (3, 256, 256))
        b = x.shape[0]
        logits = torch.empty((b, 1, 256, 256), dtype=torch.float32, device=self.device)
        mask = torch.empty((b, 256, 256), dtype=torch.uint8, device=self.device) if want_mask else None
        emb = self._embedding_out("unet", b) if want_embedding else None
        _check(self._lib.cv_unet_forward_mask(self._h, _ptr(x), b, _ptr(logits), _ptr(mask) if want_mask else None, float(threshold),
                                              _ptr(emb) if want_embedding else None, _stream_ptr(self.device)))
        return (logits, mask, emb) if want_embedding else (logits, mask)

    def resnet18_forward_u8(self, squares_u8: torch.Tensor, want_embedding: bool = False):
        """(N,64,64) uint8 -> (N,13) float32 softmax probabilities of the loaded ResNet (18 or 34); with ``want_embedding`` ->
        (probabilities, embedding (N,512) float32)."""
        if squares_u8.dtype != torch.uint8 or tuple(squares_u8.shape[1:]) != (64, 64):
            raise HipBackendError("resnet18_forward_u8 expects (N,64,64) uint8")
        squares_u8 = squares_u8.to(self.device).contiguous()
        n = squares_u8.shape[0]
        out = torch.empty((n, 13), dtype=torch.float32, device=self.device)
        if want_embedding:
            emb = self._embedding_out(self.classifier_arch or "resnet18", n)
            _check(self._lib.cv_resnet18_forward_u8_emb(self._h, _ptr(squares_u8), n, _ptr(out), _ptr(emb), _stream_ptr(self.device)))
            return out, emb
        _check(self._lib.cv_resnet18_forward_u8(self._h, _ptr(squares_u8), n, _ptr(out), _stream_ptr(self.device)))
        return out

    def resnet_forward_u8_norm(self, squares_u8: torch.Tensor, normalize, softmax: bool = False, want_embedding: bool = False):
        """(N,64,64) uint8 -> (N,13) float32 logits (probabilities with ``softmax``) of the loaded ResNet with the squares normalised
        in the stem: ``normalize = (mean, std)`` is torchvision's ``ToTensor()`` + ``Normalize([mean], [std])``, bit for bit
        (``cv_resnet_forward_u8_norm``).  With ``want_embedding`` -> (out, embedding (N,512) float32).  Like ``resnet18_forward_u8`` it
        does not consult the numeric guard."""
        if squares_u8.dtype != torch.uint8 or tuple(squares_u8.shape[1:]) != (64, 64):
            raise HipBackendError("resnet_forward_u8_norm expects (N,64,64) uint8")
        mean, std = (float(v) for v in normalize)
        squares_u8 = squares_u8.to(self.device).contiguous()
        n = squares_u8.shape[0]
        out = torch.empty((n, 13), dtype=torch.float32, device=self.device)
        emb = self._embedding_out(self.classifier_arch or "resnet18", n) if want_embedding else None
        _check(self._lib.cv_resnet_forward_u8_norm(self._h, _ptr(squares_u8), n, mean, std, 1 if softmax else 0, _ptr(out),
                                                   _ptr(emb) if want_embedding else None, _stream_ptr(self.device)))
        return (out, emb) if want_embedding else out

    def square_records_dev(self, logits: torch.Tensor, labels: torch.Tensor | None = None) -> torch.Tensor:
        """The device half of ``square_records``: launches the records kernel on the current stream behind whatever produced
        ``logits`` ((N,13) float32 on this device, contiguous); ``labels``: (N,) int8 on this device (0..12, -1 = unlabelled) or None.
        Returns the (N,32) uint8 device tensor of records.  Nothing is synchronised or copied."""
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.device != self.device or logits.dim() != 2 \
                or logits.shape[1] != 13 or not logits.is_contiguous():
            raise HipBackendError("square_records expects contiguous (N,13) float32 logits on the engine's device")
        n = int(logits.shape[0])
        if labels is not None and (not isinstance(labels, torch.Tensor) or labels.dtype != torch.int8 or labels.device != self.device
                                   or tuple(labels.shape) != (n,) or not labels.is_contiguous()):
            raise HipBackendError("square_records expects (N,) int8 labels on the engine's device, or None")
        records = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        if n:
            _check(self._lib.cv_square_records(self._h, _ptr(logits), _ptr(labels) if labels is not None else None, n, _ptr(records),
                                               _stream_ptr(self.device)))
        return records

    def square_records(self, logits: torch.Tensor, labels=None) -> np.ndarray:
        """(N,13) logits (moved to the device if need be) and N class indices (-1 = unlabelled) or None -> the (N,) ``SQUARE_RECORD``
        array the kernel wrote: predicted, rank, label, flags, confidence, loss, max_logit, logsumexp.  Synchronises the current
        stream.  A label outside -1..12 raises."""
        logits = logits.to(self.device, torch.float32).contiguous()
        if labels is not None:
            lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels)
            if lab.size and (lab.min() < -1 or lab.max() > 12):
                raise HipBackendError("square_records: labels must be class indices 0..12, or -1 for an unlabelled square")
            labels = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int8)).to(self.device)
        return self.square_records_dev(logits, labels).cpu().numpy().view(SQUARE_RECORD).reshape(-1)

    def embedding_neighbours_dev(self, queries: torch.Tensor, corpus: torch.Tensor, k: int, exclude_self: bool = False,
                                 exact_only: bool = False):
        """The device half of ``embedding_neighbours`` (``cv_embedding_neighbours``): ``queries`` (Q, C) and ``corpus`` (N, C), dense
        float32 tensors on this device (the same tensor for a table against itself), -> ``(indices (Q, k) int32, sq_distances (Q, k)
        float64, stats (8,) int32)`` device tensors.  Launched on the current stream behind whatever produced the tables; the scratch
        comes from the caching allocator on that stream.  Nothing is synchronised or copied.  ``exact_only`` sends every row through
        the exact path (the device's own reference)."""
        for name, t in (("queries", queries), ("corpus", corpus)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != self.device or t.dim() != 2 \
                    or not t.is_contiguous() or t.shape[0] < 1 or t.shape[1] < 1:
                raise HipBackendError(f"embedding_neighbours expects {name} as a dense (rows, channels) float32 tensor on the engine's device")
        q, c = (int(v) for v in queries.shape)
        n = int(corpus.shape[0])
        if int(corpus.shape[1]) != c:
            raise HipBackendError(f"embedding_neighbours: queries have {c} channels, the corpus {int(corpus.shape[1])}")
        flags = (NEIGHBOURS_EXCLUDE_SELF if exclude_self else 0) | (NEIGHBOURS_EXACT_ONLY if exact_only else 0)
        need = int(self._lib.cv_embedding_neighbours_scratch_bytes(q, n, c, int(k)))
        with torch.cuda.device(self.device):
            scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            indices = torch.empty((q, max(int(k), 0)), dtype=torch.int32, device=self.device)
            dist = torch.empty((q, max(int(k), 0)), dtype=torch.float64, device=self.device)
            stats = torch.empty(8, dtype=torch.int32, device=self.device)
            _check(self._lib.cv_embedding_neighbours(self._h, _ptr(queries), q, _ptr(corpus), n, c, int(k), flags, _ptr(indices), _ptr(dist),
                                                     _ptr(stats), _ptr(scratch), need, _stream_ptr(self.device)))
        return indices, dist, stats

    def embedding_neighbours(self, queries, corpus=None, k: int = 10, exclude_self=None, exact_only: bool = False):
        """``chessvision.embeddings.neighbours`` on the device, bit for bit: host arrays or tensors in (moved to the device if need
        be), a ``Neighbours`` of numpy arrays out, ``stats`` telling how many rows the filter certified and how many went through the
        exact path.  ``corpus=None``: the table against itself without each row's own entry.  Synchronises the current stream."""
        from .embeddings import Neighbours, check_neighbour_arguments

        def dev(t):
            t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
            return t.to(self.device, torch.float32).contiguous()

        a = dev(queries)
        b = a if corpus is None else dev(corpus)
        if a.dim() != 2 or b.dim() != 2 or a.shape[0] < 1 or b.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError(f"embedding_neighbours expects (rows, channels) tables, got {tuple(a.shape)} and {tuple(b.shape)}")
        exclude_self = check_neighbour_arguments(a.shape[0], b.shape[0], a.shape[1], b.shape[1], k, corpus is not None, exclude_self)
        indices, dist, stats = self.embedding_neighbours_dev(a, b, int(k), exclude_self, exact_only)
        record = stats.cpu().numpy()
        return Neighbours(indices.cpu().numpy(), dist.cpu().numpy(), {name: int(record[i]) for i, name in enumerate(NEIGHBOUR_STATS)})

    def pacmap_plan(self, n: int, c: int, n_neighbors: int, n_mn: int, n_fp: int) -> PacmapPlan:
        """``cv_pacmap_plan``: the limits checked, kc and the two scratch sizes."""
        plan = PacmapPlan()
        _check(self._lib.cv_pacmap_plan(int(n), int(c), int(n_neighbors), int(n_mn), int(n_fp), ctypes.byref(plan)))
        return plan

    def pacmap_pairs_dev(self, pre: torch.Tensor, n_neighbors: int, n_mn: int, n_fp: int, seed: int = 0):
        """The device half of ``pacmap_pairs`` (``cv_pacmap_pairs``): ``pre`` (N, C), a dense finite float32 tensor on this device, ->
        ``(neighbours (N, n_neighbors), mid_near (N, n_mn), further (N, n_fp), stats (64,) uint8)`` device tensors, the pair sets
        int32.  Launched on the current stream; the scratch comes from the caching allocator on that stream.  Nothing is
        synchronised or copied."""
        if not isinstance(pre, torch.Tensor) or pre.dtype != torch.float32 or pre.device != self.device or pre.dim() != 2 \
                or not pre.is_contiguous():
            raise HipBackendError("pacmap_pairs expects pre as a dense (rows, channels) float32 tensor on the engine's device")
        n, c = (int(v) for v in pre.shape)
        plan = self.pacmap_plan(n, c, n_neighbors, n_mn, n_fp)
        need = int(plan.pairs_scratch_bytes)
        with torch.cuda.device(self.device):
            scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            nbr, mid, far = (torch.empty((n, int(k)), dtype=torch.int32, device=self.device) for k in (n_neighbors, n_mn, n_fp))
            stats = torch.empty(64, dtype=torch.uint8, device=self.device)
            _check(self._lib.cv_pacmap_pairs(self._h, _ptr(pre), n, c, int(n_neighbors), int(n_mn), int(n_fp),
                                             int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(nbr), _ptr(mid) if n_mn else None,
                                             _ptr(far) if n_fp else None, _ptr(stats), _ptr(scratch), need, _stream_ptr(self.device)))
        return nbr, mid, far, stats

    def pacmap_pairs(self, pre, n_neighbors=None, n_MN=None, n_FP=None, seed: int = 0):
        """``chessvision.embeddings.pacmap_pairs`` on the device, index for index: a host array or tensor in (moved to the device if
        need be), a ``PacmapPairs`` of numpy arrays out.  Synchronises the current stream."""
        from .embeddings import PacmapPairs, _finite_table, check_pacmap_arguments

        if isinstance(pre, torch.Tensor):
            pre = pre.to(self.device, torch.float32).contiguous()
            if pre.dim() != 2 or pre.shape[0] < 1 or pre.shape[1] < 1:
                raise ValueError(f"pre must be a (rows, channels) table, got shape {tuple(pre.shape)}")
            if not bool(torch.isfinite(pre).all()):
                raise ValueError("pre holds a NaN or an infinity")
        else:
            pre = torch.tensor(_finite_table(pre, "pre")).to(self.device)          # a copy: the caller's array may be read-only
        nn, nmn, nfp, kc = check_pacmap_arguments(pre.shape[0], n_neighbors, n_MN, n_FP)
        nbr, mid, far, stats = self.pacmap_pairs_dev(pre, nn, nmn, nfp, seed)
        record = stats.cpu().numpy().view(PACMAP_STATS)[0]
        if int(record["draw_overflow"]):
            raise RuntimeError("pacmap: a point gave up drawing candidates without filling its list")
        out = {name: int(record["neighbours"][i]) for i, name in enumerate(NEIGHBOUR_STATS)}
        out.update(candidates=int(record["candidates"]), mid_near_draws=int(record["mid_near_draws"]),
                   further_draws=int(record["further_draws"]))
        return PacmapPairs(nbr.cpu().numpy(), mid.cpu().numpy(), far.cpu().numpy(), out)

    def pacmap_optimise_dev(self, init: torch.Tensor, offsets: torch.Tensor, entries: torch.Tensor, iterations: int = 450) -> torch.Tensor:
        """The device half of ``pacmap_optimise`` (``cv_pacmap_optimise``): ``init`` (N, 2) float32, ``offsets`` (N + 1,) and
        ``entries`` int32 (``embeddings.pacmap_incidence``), dense tensors on this device, -> the (N, 2) float32 coordinates after
        ``iterations`` steps, one launch each on the current stream.  Nothing is synchronised or copied."""
        n = int(init.shape[0]) if isinstance(init, torch.Tensor) and init.dim() == 2 else 0
        for name, t, dtype, shape in (("init", init, torch.float32, (n, 2)), ("offsets", offsets, torch.int32, (n + 1,)),
                                      ("entries", entries, torch.int32, None)):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or not t.is_contiguous() \
                    or (shape is not None and tuple(t.shape) != shape) or t.dim() != (1 if shape is None else len(shape)) or n < 1:
                raise HipBackendError(f"pacmap_optimise expects {name} as a dense {dtype} tensor on the engine's device, init (N, 2), "
                                      "offsets (N + 1,), entries (E,)")
        need = int(self.pacmap_plan(n, 1, 1, 0, 0).optimise_scratch_bytes)    # depends on n alone
        with torch.cuda.device(self.device):
            scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            out = torch.empty((n, 2), dtype=torch.float32, device=self.device)
            _check(self._lib.cv_pacmap_optimise(self._h, _ptr(init), n, _ptr(offsets), _ptr(entries), int(entries.numel()), int(iterations),
                                                _ptr(out), _ptr(scratch), need, _stream_ptr(self.device)))
        return out

    def pacmap_optimise(self, init, pairs, iterations: int = 450) -> np.ndarray:
        """``chessvision.embeddings.pacmap_optimise`` on the device, bit for bit: the incidence lists are built on the host with the
        definition's own stable sort (``embeddings.pacmap_incidence``), uploaded, and walked by one launch per iteration.
        Synchronises the current stream."""
        from .embeddings import pacmap_incidence

        start = np.ascontiguousarray(np.asarray(init.detach().cpu() if isinstance(init, torch.Tensor) else init), dtype=np.float32)
        n = int(np.asarray(pairs.neighbours).shape[0])
        if start.shape != (n, 2) or not np.isfinite(start).all():
            raise ValueError(f"init must be a finite ({n}, 2) array, got shape {start.shape}")
        offsets, entries = pacmap_incidence(pairs)
        dev = [torch.tensor(a).to(self.device) for a in (start, offsets, entries)]
        return self.pacmap_optimise_dev(*dev, iterations=int(iterations)).cpu().numpy()

    def pacmap_place_plan(self, q: int, n: int, c: int, n_neighbors: int) -> PacmapPlacePlan:
        """``cv_pacmap_place_plan``: the limits checked, kc and the two scratch sizes."""
        plan = PacmapPlacePlan()
        _check(self._lib.cv_pacmap_place_plan(int(q), int(n), int(c), int(n_neighbors), ctypes.byref(plan)))
        return plan

    def _dense(self, what: str, name: str, t, dtype, shape) -> None:
        """``t`` is a dense tensor of ``dtype`` on this device; ``shape``: its shape with None for any extent of at least 1."""
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device or not t.is_contiguous() \
                or t.dim() != len(shape) or any(int(have) < 1 or (want is not None and int(have) != want) for have, want in zip(t.shape, shape)):
            raise HipBackendError(f"{what} expects {name} as a dense {dtype} tensor of shape {shape} on the engine's device")

    def pacmap_basis_scale_dev(self, pre: torch.Tensor, n_neighbors: int) -> torch.Tensor:
        """``cv_pacmap_basis_scale``: ``pre`` (N, C), a dense finite float32 tensor on this device, -> the (N,) float64 device tensor
        of the rows' scale in ``pacmap_pairs``' neighbour choice (``EmbeddingMap.sigma``).  Launched on the current stream; nothing
        is synchronised or copied."""
        self._dense("pacmap_basis_scale", "pre", pre, torch.float32, (None, None))
        n, c = (int(v) for v in pre.shape)
        need = int(self.pacmap_place_plan(1, n, c, n_neighbors).scale_scratch_bytes)
        with torch.cuda.device(self.device):
            scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            sigma = torch.empty(n, dtype=torch.float64, device=self.device)
            _check(self._lib.cv_pacmap_basis_scale(self._h, _ptr(pre), n, c, int(n_neighbors), _ptr(sigma), _ptr(scratch), need,
                                                   _stream_ptr(self.device)))
        return sigma

    def pacmap_place_pairs_dev(self, pre_new: torch.Tensor, pre: torch.Tensor, sigma: torch.Tensor, n_neighbors: int):
        """The device half of ``pacmap_place_pairs`` (``cv_pacmap_place_pairs``): ``pre_new`` (Q, C) and ``pre`` (N, C) dense finite
        float32, ``sigma`` (N,) float64, tensors on this device, -> ``(neighbours (Q, n_neighbors) int32, stats (8,) int32)`` device
        tensors.  Launched on the current stream; the scratch comes from the caching allocator on that stream.  Nothing is
        synchronised or copied."""
        self._dense("pacmap_place_pairs", "pre_new", pre_new, torch.float32, (None, None))
        q, c = (int(v) for v in pre_new.shape)
        self._dense("pacmap_place_pairs", "pre", pre, torch.float32, (None, c))
        n = int(pre.shape[0])
        self._dense("pacmap_place_pairs", "sigma", sigma, torch.float64, (n,))
        need = int(self.pacmap_place_plan(q, n, c, n_neighbors).pairs_scratch_bytes)
        with torch.cuda.device(self.device):
            scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
            nbr = torch.empty((q, int(n_neighbors)), dtype=torch.int32, device=self.device)
            stats = torch.empty(8, dtype=torch.int32, device=self.device)
            _check(self._lib.cv_pacmap_place_pairs(self._h, _ptr(pre_new), q, _ptr(pre), n, c, int(n_neighbors), _ptr(sigma), _ptr(nbr),
                                                   _ptr(stats), _ptr(scratch), need, _stream_ptr(self.device)))
        return nbr, stats

    def pacmap_place_pairs(self, map, pre_new):
        """``chessvision.embeddings.pacmap_place_pairs`` on the device, index for index: the map's basis and scale and the new rows
        are uploaded, -> ``(neighbours (Q, n_neighbors) int32 numpy array, stats dict)``.  Synchronises the current stream."""
        from .embeddings import _place_tables

        x, nn, kc = _place_tables(map, pre_new)
        dev = [torch.tensor(a).to(self.device) for a in (x, np.ascontiguousarray(map.pre, dtype=np.float32),
                                                         np.ascontiguousarray(map.sigma, dtype=np.float64))]
        nbr, stats = self.pacmap_place_pairs_dev(*dev, nn)
        record = stats.cpu().numpy()
        return nbr.cpu().numpy(), dict({name: int(record[i]) for i, name in enumerate(NEIGHBOUR_STATS)}, candidates=kc)

    def pacmap_place_dev(self, init: torch.Tensor, basis: torch.Tensor, pairs: torch.Tensor, iterations: int = 450) -> torch.Tensor:
        """The device half of ``pacmap_place`` (``cv_pacmap_place``): ``init`` (Q, 2) and ``basis`` (N, 2) float32, ``pairs``
        (Q, n_neighbors) int32, dense tensors on this device, -> the (Q, 2) float32 coordinates after ``iterations`` steps: one
        launch on the current stream.  Nothing is synchronised or copied."""
        self._dense("pacmap_place", "init", init, torch.float32, (None, 2))
        q = int(init.shape[0])
        self._dense("pacmap_place", "basis", basis, torch.float32, (None, 2))
        self._dense("pacmap_place", "pairs", pairs, torch.int32, (q, None))
        with torch.cuda.device(self.device):
            out = torch.empty((q, 2), dtype=torch.float32, device=self.device)
            _check(self._lib.cv_pacmap_place(self._h, _ptr(init), q, _ptr(basis), int(basis.shape[0]), _ptr(pairs), int(pairs.shape[1]),
                                             int(iterations), _ptr(out), _stream_ptr(self.device)))
        return out

    def pacmap_place(self, init, basis_coordinates, pairs, iterations: int = 450) -> np.ndarray:
        """``chessvision.embeddings.pacmap_place`` on the device, bit for bit.  Synchronises the current stream."""
        from .embeddings import check_pacmap_place_inputs

        dev = [torch.tensor(a).to(self.device) for a in check_pacmap_place_inputs(init, basis_coordinates, pairs)]
        return self.pacmap_place_dev(*dev, iterations=int(iterations)).cpu().numpy()

    def extraction_scores_dev(self, values: torch.Tensor, transform: str = "none", want_mask: bool = False):
        """The device half of ``extraction_scores``: launches the score kernel on the current stream behind whatever produced
        ``values`` ((N, ...) float32 on this device, each image contiguous) and returns (records (N,64) uint8 device tensor, half_mask
        (N,count) uint8 device tensor | None).  Nothing is synchronised or copied."""
        if transform not in _TRANSFORMS:
            raise HipBackendError(f"transform must be one of {sorted(_TRANSFORMS)}, got {transform!r}")
        if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.device != self.device or values.dim() < 1:
            raise HipBackendError("extraction_scores expects an (N, ...) float32 tensor on the engine's device")
        n = int(values.shape[0])
        count = int(values.numel() // n) if n else 0
        if n and not values.is_contiguous():
            raise HipBackendError("extraction_scores expects contiguous images")
        records = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        mask = torch.empty((n, count), dtype=torch.uint8, device=self.device) if want_mask else None
        _check(self._lib.cv_extraction_scores(self._h, _ptr(values), n, count, _TRANSFORMS[transform], _ptr(records),
                                              _ptr(mask) if want_mask else None, _stream_ptr(self.device)))
        return records, mask

    def extraction_scores(self, values: torch.Tensor, transform: str = "none", want_mask: bool = False):
        """(N, ...) float32 device tensor -> (records, confidence, distribution[, half_mask]): per image the ``SCORE_RECORD`` the
        kernel wrote (numpy), the two scores computed from it (float64; the reference's ``probability_confidence`` and
        ``probability_distribution`` of the values, or of their sigmoid with ``transform="sigmoid"``), and with ``want_mask`` the
        (N, count) uint8 mask ``v > 0.5``.  Synchronises the current stream."""
        records, mask = self.extraction_scores_dev(values, transform, want_mask)
        rec = records.cpu().numpy().view(SCORE_RECORD).reshape(-1)
        conf, dist = scores_finish(rec)
        return (rec, conf, dist, mask.cpu().numpy()) if want_mask else (rec, conf, dist)

    def segmentation_scores_dev(self, logits: torch.Tensor, labels: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
        """The device half of ``segmentation_scores``: launches the kernel on the current stream behind whatever produced ``logits``
        ((N, ...) float32 on this device, contiguous) and ``labels`` (uint8, the same number of elements per image, contiguous; a
        pixel is "board" iff its byte is non-zero) and returns the (N,64) uint8 device tensor of records.  Nothing is synchronised
        or copied."""
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.device != self.device or logits.dim() < 1:
            raise HipBackendError("segmentation_scores expects an (N, ...) float32 logits tensor on the engine's device")
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.device != self.device or labels.dim() < 1:
            raise HipBackendError("segmentation_scores expects an (N, ...) uint8 label tensor on the engine's device")
        n = int(logits.shape[0])
        count = int(logits.numel() // n) if n else 0
        if int(labels.shape[0]) != n or labels.numel() != logits.numel():
            raise HipBackendError("segmentation_scores expects one label byte per logit")
        if n and not (logits.is_contiguous() and labels.is_contiguous()):
            raise HipBackendError("segmentation_scores expects contiguous images")
        if not np.isfinite(float(threshold)):
            raise HipBackendError("segmentation_scores expects a finite threshold")
        records = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        _check(self._lib.cv_segmentation_scores(self._h, _ptr(logits), _ptr(labels), n, count, float(threshold), _ptr(records),
                                                _stream_ptr(self.device)))
        return records

    def segmentation_scores(self, logits: torch.Tensor, labels: torch.Tensor, threshold: float = 0.5):
        """-> (records, scores): per image the ``SEG_RECORD`` the kernel wrote (numpy) and the dict of float64 arrays
        ``segmentation_scores_finish`` makes of them (bce, dice_loss, loss, dice, iou, pixel_accuracy).  Synchronises the current
        stream."""
        rec = self.segmentation_scores_dev(logits, labels, threshold).cpu().numpy().view(SEG_RECORD).reshape(-1)
        return rec, segmentation_scores_finish(rec)

    def threshold_levels_dev(self, logits: torch.Tensor, thresholds, labels: torch.Tensor | None = None):
        """The device half of ``threshold_levels``: launches the levels kernel on the current stream behind whatever produced
        ``logits`` ((N, ...) float32 on this device, contiguous).  ``thresholds``: 1..32 values in [0, 1], strictly ascending as
        float32; ``labels``: uint8 on this device, one byte per logit, contiguous ("board" iff non-zero), or None.  Returns (levels
        (N,count) uint8, records (N,320) uint8) device tensors: ``levels > k`` is the mask at ``thresholds[k]``.  Nothing is
        synchronised or copied."""
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.device != self.device or logits.dim() < 1:
            raise HipBackendError("threshold_levels expects an (N, ...) float32 logits tensor on the engine's device")
        n = int(logits.shape[0])
        count = int(logits.numel() // n) if n else 0
        if labels is not None:
            if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.device != self.device or labels.dim() < 1:
                raise HipBackendError("threshold_levels expects an (N, ...) uint8 label tensor on the engine's device, or None")
            if int(labels.shape[0]) != n or labels.numel() != logits.numel():
                raise HipBackendError("threshold_levels expects one label byte per logit")
        if n and not (logits.is_contiguous() and (labels is None or labels.is_contiguous())):
            raise HipBackendError("threshold_levels expects contiguous images")
        thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))   # checked by the C entry, before any launch
        levels = torch.empty((n, count), dtype=torch.uint8, device=self.device)
        records = torch.empty((n, LEVEL_RECORD.itemsize), dtype=torch.uint8, device=self.device)
        _check(self._lib.cv_threshold_levels(self._h, _ptr(logits), _ptr(labels) if labels is not None else None, n, count,
                                             thr.ctypes.data_as(_fp), int(thr.size), _ptr(levels), _ptr(records),
                                             _stream_ptr(self.device)))
        return levels, records

    def threshold_levels(self, logits: torch.Tensor, thresholds, labels: torch.Tensor | None = None):
        """-> (levels (N,count) uint8, records (N,) ``LEVEL_RECORD``) as numpy.  Synchronises the current stream."""
        levels, records = self.threshold_levels_dev(logits, thresholds, labels)
        return levels.cpu().numpy(), records.cpu().numpy().view(LEVEL_RECORD).reshape(-1)

    def softmax13(self, logits: torch.Tensor) -> torch.Tensor:
        logits = logits.to(self.device, torch.float32).contiguous()
        out = torch.empty_like(logits)
        _check(self._lib.cv_softmax13(self._h, _ptr(logits), logits.shape[0], _ptr(out), _stream_ptr(self.device)))
        return out

    # -- classical stages on the device ------------------------------------------
    def resize_area_u8(self, images: torch.Tensor, out_hw=(256, 256)) -> torch.Tensor:
        """(N,H,W,C) uint8 -> (N,out_h,out_w,C) uint8 with INTER_AREA semantics (reference core.py:212)."""
        if images.dtype != torch.uint8 or images.dim() != 4:
            raise HipBackendError("resize_area_u8 expects (N,H,W,C) uint8")
        images = images.to(self.device).contiguous()
        n, h, w, c = images.shape
        out = torch.empty((n, out_hw[0], out_hw[1], c), dtype=torch.uint8, device=self.device)
        _check(self._lib.cv_resize_area_u8(self._h, _ptr(images), n, h, w, c, _ptr(out), out_hw[0], out_hw[1],
                                           _stream_ptr(self.device)))
        return out

    def resize_antialias_f32(self, images: torch.Tensor, out_hw=(256, 256)) -> torch.Tensor:
        """(N,H,W,C) uint8 HWC, C in 1..4 -> (N,C,out_h,out_w) float32 NCHW in [0,1]: the antialiased bilinear resize of the
        reference's enrichment job, ``F.interpolate(u8.float() / 255, out_hw, mode="bilinear", antialias=True,
        align_corners=False)`` (``classical.resize_antialias`` is the host form).  One launch on the current stream."""
        if images.dtype != torch.uint8 or images.dim() != 4 or not 1 <= images.shape[3] <= 4:
            raise HipBackendError("resize_antialias_f32 expects (N,H,W,C) uint8 with 1 to 4 channels")
        images = images.to(self.device).contiguous()
        n, h, w, c = images.shape
        out = torch.empty((n, c, out_hw[0], out_hw[1]), dtype=torch.float32, device=self.device)
        if n:
            _check(self._lib.cv_resize_antialias_f32(self._h, _ptr(images), n, h, w, c, _ptr(out), out_hw[0], out_hw[1],
                                                     _stream_ptr(self.device)))
        return out

    def extract_squares_u8(self, images: torch.Tensor, inverse_maps: np.ndarray, want_boards: bool = True):
        """images (N,H,W,3) uint8 BGR on the device + N inverse homographies (board pixel -> source pixel) ->
        (squares (N*64,64,64) uint8, boards (N,512,512) uint8 | None): warp + gray + flip + split, fused."""
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
            raise HipBackendError("extract_squares_u8 expects (N,H,W,3) uint8")
        images = images.to(self.device).contiguous()
        n, h, w, _ = images.shape
        # the matrices travel through a pinned staging tensor on the current stream; nothing here blocks the host, so the
        # next job's UNet (already queued on this stream) does not hold the classifier of this job back
        if isinstance(inverse_maps, torch.Tensor):           # already staged by the caller (page-locked, float64, n x 9)
            if inverse_maps.dtype != torch.float64 or inverse_maps.numel() != n * 9:
                raise HipBackendError("extract_squares_u8 expects n x 9 float64 matrices")
            inv = inverse_maps
        else:
            inv = torch.from_numpy(np.ascontiguousarray(inverse_maps, dtype=np.float64).reshape(n, 9)).pin_memory()
        inv_dev = inv.to(self.device, non_blocking=True)
        squares = torch.empty((n * 64, 64, 64), dtype=torch.uint8, device=self.device)
        boards = torch.empty((n, 512, 512), dtype=torch.uint8, device=self.device) if want_boards else None
        _check(self._lib.cv_extract_squares_u8_dev(self._h, _ptr(images), n, h, w, _ptr(inv_dev), _ptr(squares),
                                                   _ptr(boards) if want_boards else None, _stream_ptr(self.device)))
        return squares, boards

    # -- JPEG decode: host entropy stage (chessvision/jpeg.py), device reconstruction (csrc/jpeg.hip) ----------------------
    def jpeg_reconstruct_dev(self, coeffs: torch.Tensor, qtables: torch.Tensor, info, channel_order: str = "bgr",
                             out: torch.Tensor | None = None, orientation: int = 0) -> torch.Tensor:
        """Device form: ``coeffs`` int16 ``(n, 64 * info.blocks)`` and ``qtables`` ``(n, components, 64)`` (uint16 values in an int16
        tensor), both on the device and 16-byte aligned, as ``jpeg.entropy_decode`` wrote them for n images of the one geometry
        ``info`` -> ``(n, h, w, 3)`` uint8, or ``(n, h, w)`` for ``"gray"`` (written into ``out`` when given).  Two launches on the
        current stream; nothing waits.  ``orientation``: an EXIF tag 0..8 all n images are turned by in the colour stage's store
        (``cv_jpeg_reconstruct_oriented_u8``; ``info.orientation`` is not read); ``h`` and ``w`` are then ``jpeg.oriented_shape``'s.
        0 is the call it always was."""
        from .jpeg import ORDERS, check_tag, oriented_shape
        orientation = check_tag(orientation)
        if channel_order not in ORDERS:
            raise HipBackendError(f"channel_order must be one of {sorted(ORDERS)}")
        if coeffs.dtype != torch.int16 or qtables.dtype != torch.int16 or coeffs.dim() != 2 or not coeffs.is_contiguous() \
                or not qtables.is_contiguous() or coeffs.device != self.device or qtables.device != self.device:
            raise HipBackendError("jpeg_reconstruct_dev expects contiguous int16 device tensors")
        n = coeffs.shape[0]
        if coeffs.shape[1] != 64 * info.blocks or qtables.numel() != n * info.components * 64:
            raise HipBackendError("jpeg_reconstruct_dev: tensors do not match the geometry")
        shape = (n,) + oriented_shape(info, orientation) + (() if channel_order == "gray" else (3,))
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != self.device:
            raise HipBackendError(f"jpeg_reconstruct_dev: out must be a contiguous uint8 device tensor of shape {shape}")
        if n == 0:
            return out
        planes = torch.empty(n * 64 * info.blocks, dtype=torch.uint8, device=self.device)
        c_info = info.to_c()
        if orientation:
            _check(self._lib.cv_jpeg_reconstruct_oriented_u8(self._h, _ptr(coeffs), _ptr(qtables), n, ctypes.addressof(c_info),
                                                             ORDERS[channel_order], orientation, _ptr(planes), planes.numel(), _ptr(out),
                                                             _stream_ptr(self.device)))
            return out
        _check(self._lib.cv_jpeg_reconstruct_u8(self._h, _ptr(coeffs), _ptr(qtables), n, ctypes.addressof(c_info), ORDERS[channel_order],
                                                _ptr(planes), planes.numel(), _ptr(out), _stream_ptr(self.device)))
        return out

    def jpeg_decode(self, blobs, channel_order: str = "bgr", orientation: str = "ignore") -> torch.Tensor:
        """JPEG streams of ONE geometry (size, components, sampling) -> device tensor ``(n, h, w, 3)`` uint8 in ``"bgr"`` (default) or
        ``"rgb"`` order, or ``(n, h, w)`` for ``"gray"`` (1-component streams only).  The Huffman stage runs on host threads into one
        page-locked buffer, one copy takes it to the device, two launches reconstruct the pixels: libjpeg's, byte for byte.
        ``orientation="exif"`` turns the pictures as their EXIF orientation tag says, in the second launch's store (the table in
        ``chessvision/jpeg.py``); the streams must then share the effective tag as well (absent and 1 count as one), and ``h``, ``w``
        are the turned picture's.  Raises ``jpeg.UnsupportedJpeg`` (a ``ValueError``) naming the refused blobs, and ``ValueError``
        naming the streams whose tag differs from the first one's."""
        from . import jpeg as _jpeg
        _jpeg.check_orientation(orientation)
        blobs = list(blobs)
        if not blobs:
            raise HipBackendError("jpeg_decode needs at least one stream")
        infos = [_jpeg.jpeg_info(b) for b in blobs]
        bad = {i: f.reason for i, f in enumerate(infos) if not f.supported}
        if bad:
            raise _jpeg.UnsupportedJpeg(bad)
        info = infos[0]
        if any(f.geometry != info.geometry for f in infos):
            raise HipBackendError("jpeg_decode: all streams of one call must share one geometry (ChessVision.decode_jpegs groups them)")
        tag = _jpeg.effective_tag(info, orientation)                  # 0 for every stream under "ignore"
        odd = [i for i, f in enumerate(infos) if _jpeg.effective_tag(f, orientation) != tag]
        if odd:
            raise ValueError(f"jpeg_decode: streams {odd} do not carry the EXIF orientation of stream 0 ({tag or 1}); one call turns "
                             "all its pictures alike (ChessVision.decode_jpegs groups them)")
        n, count, tables = len(blobs), 64 * info.blocks, 64 * info.components
        staging = torch.empty(n * (count + tables), dtype=torch.int16).pin_memory()
        host = staging.numpy()
        co, qt = host[:n * count].reshape(n, count), host[n * count:].view(np.uint16).reshape(n, info.components, 64)
        _jpeg.entropy_decode_many(blobs, infos, co, qt)
        dev = staging.to(self.device, non_blocking=True)
        extra = {"orientation": tag} if tag else {}
        out = self.jpeg_reconstruct_dev(dev[:n * count].view(n, count), dev[n * count:].view(n, info.components, 64), info, channel_order, **extra)
        torch.cuda.current_stream(self.device).synchronize()          # the page-locked buffer is released on return
        return out

    # -- JPEG encode: tables and header on the host (csrc/jpeg.cpp), everything else on the device (csrc/jpeg_enc.hip) -----------
    def jpeg_encode_gray_dev(self, images: torch.Tensor, quality: int = 95):
        """Device form: ``images`` (n, h, w) uint8 on the device, n >= 1, h and w 1..4096 -> ``(out, offsets, lengths)`` device tensors:
        file i is ``out[offsets[i] : offsets[i] + lengths[i]]`` (uint8; int64 offsets in 16-byte steps, n + 1 of them: the last is the
        end of the last file; int32 lengths).  ``out`` is sized for the worst case (``jpeg_gray_max_bytes`` per image) and is never
        meant to be downloaded whole.  Launches on the current stream; nothing waits."""
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 3 or images.device != self.device \
                or not images.is_contiguous():
            raise HipBackendError("jpeg_encode_gray_dev expects a contiguous (n, h, w) uint8 tensor on the engine's device")
        n, h, w = (int(v) for v in images.shape)
        if n < 1 or not (1 <= h <= 4096 and 1 <= w <= 4096):
            raise HipBackendError("jpeg_encode_gray_dev: n >= 1 images of 1..4096 x 1..4096 pixels")
        each = jpeg_gray_max_bytes(h, w)
        out = torch.empty(n * each, dtype=torch.uint8, device=self.device)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        lengths = torch.empty(n, dtype=torch.int32, device=self.device)
        _check(self._lib.cv_jpeg_encode_gray_u8(self._h, _ptr(images), n, h, w, int(quality), _ptr(out), out.numel(), _ptr(offsets),
                                                _ptr(lengths), _stream_ptr(self.device)))
        return out, offsets, lengths

    def jpeg_encode_gray(self, images, quality: int = 95) -> list:
        """Gray images of ONE size, (n, h, w) uint8 as a device tensor or a numpy array -> n complete baseline JPEG files (``bytes``):
        libjpeg's with its defaults, byte for byte (``jpeg.encode_gray`` is the numpy form).  The offsets and lengths come back first,
        then exactly the bytes the files occupy; both waits are on events of the current stream, never device-wide."""
        if isinstance(images, np.ndarray):
            a = np.ascontiguousarray(images, dtype=np.uint8)
            if a.ndim != 3:
                raise HipBackendError("jpeg_encode_gray expects (n, h, w) uint8 images")
            images = torch.from_numpy(a).to(self.device)
        return self._fetch_files(*self.jpeg_encode_gray_dev(images.contiguous(), quality))

    @staticmethod
    def _fetch_files(out: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor) -> list:
        """What an encoder's device form returned, as ``bytes`` per file: the offsets and lengths come back first, then exactly the
        bytes the files occupy; both waits are on events of the current stream."""
        n = lengths.numel()
        table = torch.empty(2 * n + 1, dtype=torch.int64, pin_memory=True)
        table[:n + 1].copy_(offsets, non_blocking=True)
        table[n + 1:].copy_(lengths, non_blocking=True)          # widened on the device, one more small launch
        landed = torch.cuda.Event()
        landed.record()
        landed.synchronize()
        t = table.numpy()
        host = torch.empty(int(t[n]), dtype=torch.uint8, pin_memory=True)
        host.copy_(out[:int(t[n])], non_blocking=True)
        landed.record()
        landed.synchronize()
        h = host.numpy()
        return [h[int(t[i]):int(t[i]) + int(t[n + 1 + i])].tobytes() for i in range(n)]

    def jpeg_encode_colour_dev(self, images: torch.Tensor, quality: int = 95, subsampling: str = "4:2:0", channel_order: str = "bgr"):
        """Device form: ``images`` (n, h, w, 3) uint8 on the device in ``channel_order`` ("bgr" | "rgb": which byte of a pixel is R),
        n >= 1, h and w 1..4096 -> ``(out, offsets, lengths)`` device tensors as ``jpeg_encode_gray_dev`` returns them: file i is
        ``out[offsets[i] : offsets[i] + lengths[i]]``, a three-component baseline file with luma sampled as ``subsampling`` says
        ("4:2:0" | "4:2:2" | "4:4:4").  ``out`` is sized for the worst case (``jpeg_colour_max_bytes`` per image).  Launches on the
        current stream; nothing waits."""
        from .jpeg import ORDERS, check_colour_order
        check_colour_order(channel_order)
        sub = _jpeg_subsampling(subsampling)
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 \
                or images.device != self.device or not images.is_contiguous():
            raise HipBackendError("jpeg_encode_colour_dev expects a contiguous (n, h, w, 3) uint8 tensor on the engine's device")
        n, h, w = (int(v) for v in images.shape[:3])
        if n < 1 or not (1 <= h <= 4096 and 1 <= w <= 4096):
            raise HipBackendError("jpeg_encode_colour_dev: n >= 1 images of 1..4096 x 1..4096 pixels")
        each = jpeg_colour_max_bytes(h, w, subsampling)
        out = torch.empty(n * each, dtype=torch.uint8, device=self.device)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        lengths = torch.empty(n, dtype=torch.int32, device=self.device)
        _check(self._lib.cv_jpeg_encode_colour_u8(self._h, _ptr(images), n, h, w, ORDERS[channel_order], sub, int(quality), _ptr(out),
                                                  out.numel(), _ptr(offsets), _ptr(lengths), _stream_ptr(self.device)))
        return out, offsets, lengths

    def jpeg_encode_colour(self, images, quality: int = 95, subsampling: str = "4:2:0", channel_order: str = "bgr") -> list:
        """Colour images of ONE size, (n, h, w, 3) uint8 as a device tensor or a numpy array -> n complete baseline JPEG files
        (``bytes``): libjpeg's with its defaults, byte for byte (``jpeg.encode_colour`` is the numpy form).  Event waits only, and
        exactly the files' bytes are downloaded, as in ``jpeg_encode_gray``."""
        if isinstance(images, np.ndarray):
            a = np.ascontiguousarray(images, dtype=np.uint8)
            if a.ndim != 4 or a.shape[3] != 3:
                raise HipBackendError("jpeg_encode_colour expects (n, h, w, 3) uint8 images")
            images = torch.from_numpy(a).to(self.device)
        return self._fetch_files(*self.jpeg_encode_colour_dev(images.contiguous(), quality, subsampling, channel_order))

    # -- introspection ----------------------------------------------------------------------------
    def activation(self, model: str, name: str) -> np.ndarray:
        dims = (ctypes.c_int64 * 4)()
        _check(self._lib.cv_get_activation(self._h, model.encode(), name.encode(), None, 0, dims))
        out = np.empty(tuple(int(d) for d in dims), dtype=np.float32)
        _check(self._lib.cv_get_activation(self._h, model.encode(), name.encode(), out.ctypes.data_as(_fp), out.size,
                                           dims))
        return out

    def activation_channel_means(self, model: str, name: str) -> torch.Tensor:
        """(N,C) float32 device tensor: per-image channel means over H x W of the named activation, for the chunk the last forward
        left in the workspace (``cv_activation_channel_means``).  Enqueued on the current stream; nothing is synchronised or copied
        to the host.  The reference's ``--embedding_layer`` for layers other than the two hook points (``embeddings.tap_for_index``)."""
        dims = (ctypes.c_int64 * 2)()
        _check(self._lib.cv_activation_channel_means(self._h, model.encode(), name.encode(), None, 0, dims, None))
        out = torch.empty((int(dims[0]), int(dims[1])), dtype=torch.float32, device=self.device)
        _check(self._lib.cv_activation_channel_means(self._h, model.encode(), name.encode(), _ptr(out), out.numel(), dims,
                                                     _stream_ptr(self.device)))
        return out

    def activation_exponent(self, model: str, name: str) -> int:
        """Power-of-two exponent the tensor is stored with (stored = value * 2^-exponent), chosen by the load-time calibration."""
        v = _i()
        _check(self._lib.cv_get_activation_exponent(self._h, model.encode(), name.encode(), ctypes.byref(v)))
        return int(v.value)

    def model_macs(self, model: str) -> int:
        v = ctypes.c_int64()
        _check(self._lib.cv_model_macs(self._h, model.encode(), ctypes.byref(v)))
        return int(v.value)

    def profile(self, model: str, x: torch.Tensor, iters: int = 1):
        """Event-time every launch of `iters` forwards; returns (conv_ms, conv_launches, all_ms, entries)."""
        x = x.to(self.device, torch.float32).contiguous()
        n = x.shape[0]
        out = torch.empty((n, 1, 256, 256) if model == "unet" else (n, 13), dtype=torch.float32, device=self.device)
        conv_ms, all_ms, launches = _f(), _f(), _i()
        _check(self._lib.cv_profile_convs(self._h, model.encode(), _ptr(x), n, _ptr(out), iters,
                                          _stream_ptr(self.device), ctypes.byref(conv_ms), ctypes.byref(launches),
                                          ctypes.byref(all_ms)))
        entries = []
        idx = 0
        name, kern = ctypes.create_string_buffer(128), ctypes.create_string_buffer(160)
        ms, macs, is_conv, nbytes = _f(), ctypes.c_double(), _i(), ctypes.c_double()
        while self._lib.cv_profile_entry(self._h, idx, name, 128, ctypes.byref(ms), ctypes.byref(macs),
                                         ctypes.byref(is_conv)) == 0:
            _check(self._lib.cv_profile_entry_bytes(self._h, idx, ctypes.byref(nbytes)))
            _check(self._lib.cv_profile_entry_kernel(self._h, idx, kern, 160))
            entries.append({"name": name.value.decode(), "ms": ms.value, "macs": macs.value, "conv": bool(is_conv.value),
                            "bytes": nbytes.value, "kernel": kern.value.decode()})
            idx += 1
        return conv_ms.value, launches.value, all_ms.value, entries

    # -- single-layer entry points (parity tests) ------------------------------------------------
    def op_conv2d(self, x, w, stride=1, scale=None, shift=None, residual=None, relu=False) -> torch.Tensor:
        x = x.to(self.device, torch.float32).contiguous()
        w = _np_f32(w)
        n, cin, h, wd = x.shape
        cout, _, k, _ = w.shape
        pad = (k - 1) // 2
        ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
        y = torch.empty((n, cout, ho, wo), dtype=torch.float32, device=self.device)
        sc = _np_f32(scale) if scale is not None else None
        sh = _np_f32(shift) if shift is not None else None
        res = residual.to(self.device, torch.float32).contiguous() if residual is not None else None
        _check(self._lib.cv_op_conv2d(self._h, _ptr(x), n, cin, h, wd, w.ctypes.data_as(_fp), cout, k, stride,
                                      sc.ctypes.data_as(_fp) if sc is not None else None,
                                      sh.ctypes.data_as(_fp) if sh is not None else None,
                                      _ptr(res) if res is not None else None, int(bool(relu)), _ptr(y),
                                      _stream_ptr(self.device)))
        return y

    ACTS = {"none": 0, "relu": 1, "silu": 2}

    def op_conv2d_act(self, x, w, y_init, x_coff=0, y_coff=0, stride=1, scale=None, shift=None, act="silu", act_first=False,
                      res_coff=-1, in_exp=0, out_exp=0) -> torch.Tensor:
        """One convolution as the YOLOv8-cls plan launches it (``cv_op_conv2d_act``): reads channels [x_coff, x_coff + Cin) of ``x``
        (N, Cx, H, W), writes channels [y_coff, y_coff + Cout) of a tensor that starts as ``y_init`` (N, Cy, Ho, Wo) and returns the
        whole tensor; ``res_coff`` >= 0 adds channels [res_coff, res_coff + Cout) of ``y_init`` as the residual."""
        x = x.to(self.device, torch.float32).contiguous()
        y = y_init.to(self.device, torch.float32).contiguous().clone()
        w = _np_f32(w)
        cout, cin, k, _ = w.shape
        sc = _np_f32(scale) if scale is not None else None
        sh = _np_f32(shift) if shift is not None else None
        _check(self._lib.cv_op_conv2d_act(self._h, _ptr(x), x.shape[0], x.shape[1], x_coff, cin, x.shape[2], x.shape[3], w.ctypes.data_as(_fp),
                                          cout, k, stride, sc.ctypes.data_as(_fp) if sc is not None else None,
                                          sh.ctypes.data_as(_fp) if sh is not None else None, self.ACTS[act], int(bool(act_first)), _ptr(y),
                                          y.shape[1], y_coff, res_coff, in_exp, out_exp, _stream_ptr(self.device)))
        return y

    def op_stem3x3s2(self, x, w, scale, shift, normalize=None, out_exp=0) -> torch.Tensor:
        """The YOLOv8-cls stem alone: ``x`` (N,64,64) float32 in [0,1] or uint8 (``normalize`` = (mean, std): uint8 only) ->
        (N, C0, 32, 32) float32; ``w`` (C0, 9) is the one-channel filter bank."""
        u8 = x.dtype == torch.uint8
        x = x.to(self.device).contiguous() if u8 else x.to(self.device, torch.float32).contiguous()
        w, sc, sh = _np_f32(w), _np_f32(scale), _np_f32(shift)
        c0 = w.shape[0]
        y = torch.empty((x.shape[0], c0, 32, 32), dtype=torch.float32, device=self.device)
        mean, std = (float(v) for v in normalize) if normalize is not None else (0.0, 0.0)
        _check(self._lib.cv_op_stem3x3s2(self._h, _ptr(x), int(u8), x.shape[0], c0, w.ctypes.data_as(_fp), sc.ctypes.data_as(_fp),
                                         sh.ctypes.data_as(_fp), mean, std, out_exp, _ptr(y), _stream_ptr(self.device)))
        return y

    def op_head_pool_fc(self, x, w, bias, softmax=False, in_exp=0):
        """The YOLOv8-cls head alone: ``x`` (N, C, H, W) -> (logits or probabilities (N,13), pooled features (N, C))."""
        x = x.to(self.device, torch.float32).contiguous()
        w, bias = _np_f32(w), _np_f32(bias)
        n, c, h, wd = x.shape
        out = torch.empty((n, 13), dtype=torch.float32, device=self.device)
        pooled = torch.empty((n, c), dtype=torch.float32, device=self.device)
        _check(self._lib.cv_op_head_pool_fc(self._h, _ptr(x), n, c, h, wd, w.ctypes.data_as(_fp), bias.ctypes.data_as(_fp), int(bool(softmax)),
                                            in_exp, _ptr(out), _ptr(pooled), _stream_ptr(self.device)))
        return out, pooled

    def op_conv_transpose2x2(self, x, w, bias) -> torch.Tensor:
        x = x.to(self.device, torch.float32).contiguous()
        w, bias = _np_f32(w), _np_f32(bias)
        n, cin, h, wd = x.shape
        cout = w.shape[1]
        y = torch.empty((n, cout, 2 * h, 2 * wd), dtype=torch.float32, device=self.device)
        _check(self._lib.cv_op_conv_transpose2x2(self._h, _ptr(x), n, cin, h, wd, w.ctypes.data_as(_fp), cout,
                                                 bias.ctypes.data_as(_fp), _ptr(y), _stream_ptr(self.device)))
        return y

    def op_kernels(self) -> list[str]:
        """Kernel form strings of the launches the last op_conv2d / op_conv_transpose2x2 call (or profile()) recorded, in launch
        order: what the launch planner chose for that shape, e.g. ``conv3x3_halo_kernel<half_t,64,8x16,splitK4>``."""
        out = []
        kern = ctypes.create_string_buffer(160)
        while self._lib.cv_profile_entry(self._h, len(out), None, 0, None, None, None) == 0:
            _check(self._lib.cv_profile_entry_kernel(self._h, len(out), kern, 160))
            out.append(kern.value.decode())
        return out

    def op_outc_1x1(self, x, w, bias, threshold: float = 0.5):
        """(n,c,h,w) -> (logits (n,1,h,w) f32, mask (n,h,w) u8) through the stand-alone OutConv kernel."""
        x = x.to(self.device, torch.float32).contiguous()
        w, bias = _np_f32(w).reshape(-1), _np_f32(bias).reshape(-1)
        n, c, h, wd = x.shape
        logits = torch.empty((n, 1, h, wd), dtype=torch.float32, device=self.device)
        mask = torch.empty((n, h, wd), dtype=torch.uint8, device=self.device)
        _check(self._lib.cv_op_outc_1x1(self._h, _ptr(x), n, c, h, wd, w.ctypes.data_as(_fp), bias.ctypes.data_as(_fp),
                                        float(threshold), _ptr(logits), _ptr(mask), _stream_ptr(self.device)))
        return logits, mask

    def _op_pool(self, fn, x, ho, wo) -> torch.Tensor:
        x = x.to(self.device, torch.float32).contiguous()
        n, c, h, wd = x.shape
        y = torch.empty((n, c, ho(h), wo(wd)), dtype=torch.float32, device=self.device)
        _check(fn(self._h, _ptr(x), n, c, h, wd, _ptr(y), _stream_ptr(self.device)))
        return y

    def op_maxpool2x2(self, x):
        return self._op_pool(self._lib.cv_op_maxpool2x2, x, lambda h: h // 2, lambda w: w // 2)

    def op_maxpool3x3s2(self, x):
        return self._op_pool(self._lib.cv_op_maxpool3x3s2, x, lambda h: (h - 1) // 2 + 1, lambda w: (w - 1) // 2 + 1)

    def op_upsample_bilinear2x(self, x):
        return self._op_pool(self._lib.cv_op_upsample_bilinear2x, x, lambda h: 2 * h, lambda w: 2 * w)

    def selftest_mfma(self):
        a, b = _f(), _f()
        _check(self._lib.cv_selftest_mfma(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


class _HipModel:
    """Common duck-typed module surface: ``__call__``, ``eval``, ``train``, ``to``, ``metadata``."""

    model_name = ""

    def __init__(self, engine: HipEngine, metadata: dict | None = None):
        self.engine = engine
        if metadata:
            self.metadata = metadata

    def eval(self):
        return self                                    # inference-only engine

    def train(self, mode: bool = True):
        if mode:
            raise HipBackendError("the HIP backend is inference-only (reference training is out of scope)")
        return self

    def to(self, device=None, *_, **__):
        if device is not None and torch.device(device).type != "cuda":
            raise HipBackendError(f"HIP model cannot move to {device}: there is no CPU fallback")
        return self

    def parameters(self):
        return iter(())


class HipBoardExtractor(_HipModel):
    """UNet(3,1) forward on MI355X; drop-in for ``ChessVision.board_extractor`` (core.py:66-72,220)."""

    model_name = "unet"

    def __call__(self, image_batch: torch.Tensor) -> torch.Tensor:
        return self.engine.unet_forward(image_batch)


class HipPieceClassifier(_HipModel):
    """timm ResNet-18 / ResNet-34 (1ch, 13 classes) or ultralytics YOLOv8-cls forward on MI355X; drop-in for ``ChessVision.classifier`` (core.py:74-82,241).
    ``model_name`` is the architecture, which decides how a checkpoint is loaded (``utils.load_model_checkpoint``)."""

    model_name = "resnet18"

    def __init__(self, engine: HipEngine, metadata: dict | None = None, arch: str = "resnet18"):
        if arch not in CLASSIFIER_ARCHS:
            raise HipBackendError(f"classifier architecture {arch!r} has no HIP implementation (supported: {', '.join(CLASSIFIER_ARCHS)})")
        super().__init__(engine, metadata)
        self.model_name = arch

    def __call__(self, batch: torch.Tensor) -> torch.Tensor:
        return self.engine.resnet18_forward(batch)

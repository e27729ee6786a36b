"""``ChessVision`` -- image -> board -> FEN, with both CNN forwards running on MI355X through the C ABI.

Mirrors the public surface of the reference's ``chessvision/core.py`` (constructor kwargs, attributes read by
``scripts/eval/evaluate.py:357-358`` and ``tests/test_chessvision.py:29-42``, the two model properties, the three
pipeline methods and the static helpers) so the Flask endpoint and the evaluation script run unchanged.  The
model objects behind ``board_extractor`` / ``classifier`` are ``HipBoardExtractor`` / ``HipPieceClassifier``.

``process_image`` / ``predict`` / ``extract_board`` / ``classify_position`` -- the API the reference's callers use
(``app/computeroot/cv_endpoint.py:159``, ``scripts/eval/evaluate.py:270``) -- run the SAME native stages as the batched
``process_images``: device INTER_AREA resize -> ``cv_unet_forward_u8`` (sigmoid / threshold mask on device) -> C++ contours
(``cv_find_quadrangle``) -> OpenCV-order homography (``cv_board_homographies``) -> fused device warp + gray + flip + split
(``cv_extract_squares_u8_dev``) -> ``cv_resnet18_forward_u8`` (soft-max on device) -> ``cv_decode_positions``.  The numpy
restatements in ``classical.py`` and the static helpers below remain as the readable checker (and serve model objects that are
not HIP models, e.g. a test double plugged into ``_board_extractor``).

Deliberate deviations, all on the permissive side:
  * ``board_extractor_weights=None`` resolves to ``constants.BEST_EXTRACTOR_WEIGHTS`` at load time (the reference
    crashes on ``Path(None)``); the attribute itself keeps the value passed in.
  * model ids ``""`` / ``"unet"`` / ``"hip"`` select the UNet, ``""`` / ``"resnet18"`` the ResNet-18, ``"resnet34"`` the ResNet-34
    (``evaluate.py:212,214`` passes ``""``), ``"yolov8n-cls"`` .. ``"yolov8x-cls"`` an ultralytics YOLOv8-cls classifier (the names the
    reference's ``train_yolo_classifier.py`` passes to ``--model``, minus ``.pt``; it is fed as the reference feeds it: the (64,1,64,64)
    squares in [0,1], no resize or crop, index k = ``constants.LABEL_NAMES[k]``).  ``"yolo"`` still raises ImportError and ``None`` still
    means ResNet-18: the YOLO segmentation extractor is out of scope.  As in the reference, the classifier's architecture comes from
    the id, never from the checkpoint.
  * lazy initialisation is guarded by a lock (Flask request threads share one instance, ``cv_endpoint.py:131-133``).
  * extras: ``precision=`` kwarg (env ``CHESSVISION_HIP_PRECISION``: "f16x3" (default) | "f32" | "f16" | "f16r", or
    "<extractor>+<classifier>", e.g. "f16x3+f16r" = f32-grade UNet with the classifier in its fp16 mode -- one engine per model),
    ``process_images`` (batched), ``predict`` alias.
"""
from __future__ import annotations

import logging
import os
import threading
import time
from typing import Sequence

import numpy as np
import torch
from numpy.typing import NDArray

from . import classical, constants, utils
from .cv_types import BoardExtractionResult, ChessVisionResult, PositionResult, ValidationFix, pawn_rule_fix
from .fen import board_fen

logger = logging.getLogger(__name__)

_UNET_IDS = (None, "", "unet", "hip")
_RESNET_IDS = ("", "resnet18", "resnet34", "hip")
_PRECISION_NAMES = ("f16x3", "split", "f32", "fp32", "float32", "f16", "fp16", "float16", "f16r")


_FIRST_USE_LOCK = threading.Lock()          # first use of a slot's streams, one slot of the process at a time (ChessVision._warm_slot)


class _RequestSlot:
    """What ONE in-flight ``process_image`` needs for itself: an engine per model (activation workspace, page-locked staging block,
    captured hipGraphs -- none of which two forwards can share) and a HIP stream of its own.  Slot 0 wraps the instance's primary
    engines; further slots hold replicas loaded from the same checkpoints (same weights, same deterministic load-time calibration:
    bit-identical results)."""

    __slots__ = ("extractor_engine", "classifier_engine", "stream", "busy")

    def __init__(self, extractor_engine, classifier_engine, stream):
        self.extractor_engine, self.classifier_engine, self.stream, self.busy = extractor_engine, classifier_engine, stream, False


class ChessVision:
    """Chess position detection from images (drop-in for the reference class of the same name)."""

    # evaluate_images also collects the embeddings of process_images(embeddings=True) while this is set (its argument list is pinned)
    evaluation_embeddings = False
    # ... and resizes the way process_images(resize=...) does ("area" | "antialias")
    evaluation_resize = "area"

    def __init__(
        self,
        board_extractor_weights: str | None = None,
        board_extractor_model_id: str | None = None,
        classifier_weights: str | None = None,
        classifier_model_id: str | None = None,
        lazy_load: bool = True,
        precision: str | None = None,
    ):
        logger.info("Initializing ChessVision instance...")
        self.device = utils.get_device()
        self._board_extractor = None
        self._classifier = None
        self._board_extractor_weights = board_extractor_weights
        self._board_extractor_model_id = board_extractor_model_id
        self._classifier_weights = classifier_weights
        self._classifier_model_id = classifier_model_id
        self._precision = precision or os.environ.get("CHESSVISION_HIP_PRECISION", "f16x3")
        parts = self._precision.split("+")
        if not 1 <= len(parts) <= 2 or any(p not in _PRECISION_NAMES for p in parts):
            raise ValueError(f"precision must be one of {sorted(_PRECISION_NAMES)} or '<extractor>+<classifier>', got {self._precision!r}")
        self._engines: dict = {}
        self._streams = None
        self._copy_pool = None
        self._init_lock = threading.RLock()
        self._native_lock = threading.Lock()            # the single-image path shares its staging buffers between request threads
        self._stage: dict = {}
        self._last_board = None                         # (board array of the last native extraction, its squares on the device)
        self._f32_twin: ChessVision | None = None       # exact-f32 instance of the same checkpoints, created on the first numeric-guard trip
        # request slots of the single-image path (round 6): request threads of ONE instance -- the reference's Flask app keeps a global
        # instance, app/computeroot/cv_endpoint.py:131-133 -- run their B=1 forwards side by side on the device instead of queueing behind
        # one staging block.  A B=1 forward keeps the matrix pipes 5-26 % busy, so four of them overlap almost freely.
        self._slots: list[_RequestSlot] = []
        self._slot_cond = threading.Condition()
        self._slot_building = False
        self._max_slots = max(1, int(os.environ.get("CHESSVISION_REQUEST_SLOTS", "4")))
        self._guard_logged: set = set()
        if not lazy_load:
            logger.info("Eager loading models...")
            self._initialize_board_extractor()
            self._initialize_classifier()
            logger.info("Models loaded successfully")

    # ---- model objects ---------------------------------------------------------------------------
    def _get_engine(self, model: str = "unet"):
        """The engine that runs ``model`` ("unet" | "resnet18").  One engine serves both models unless the precision names two
        arithmetic types ("f16x3+f16r": extractor + classifier), in which case each model gets its own."""
        from .hip_backend import HipEngine              # raises when the library or the GPU is missing

        parts = self._precision.split("+")
        prec = parts[0] if model == "unet" or len(parts) == 1 else parts[1]
        with self._init_lock:
            if prec not in self._engines:
                self._engines[prec] = HipEngine(self.device, precision=prec)
        return self._engines[prec]

    @property
    def board_extractor(self):
        if self._board_extractor is None:
            with self._init_lock:
                if self._board_extractor is None:
                    self._initialize_board_extractor()
        assert self._board_extractor is not None
        return self._board_extractor

    @property
    def classifier(self):
        if self._classifier is None:
            with self._init_lock:
                if self._classifier is None:
                    self._initialize_classifier()
        assert self._classifier is not None
        if hasattr(self._classifier, "metadata"):
            logger.info(f"Classifier metadata: {self._classifier.metadata}")
        return self._classifier

    def _initialize_board_extractor(self) -> None:
        logger.info("Initializing board extraction model...")
        model_id = self._board_extractor_model_id
        if model_id == "yolo":
            raise ImportError("YOLO board extractors are outside the MI355X hot path (UNet only)")
        assert model_id in _UNET_IDS, f"Invalid board extractor model ID: {model_id}"
        model = utils.get_board_extractor_model(self._get_engine())
        model = utils.load_model_checkpoint(model, self._board_extractor_weights or constants.BEST_EXTRACTOR_WEIGHTS,
                                            self.device)
        if hasattr(model, "metadata"):
            logger.info(f"Board extractor metadata: {model.metadata}")
        model.eval()
        model.to(self.device)
        self._board_extractor = model

    def _initialize_classifier(self) -> None:
        logger.info("Initializing piece classifier model...")
        model_id = self._classifier_model_id
        if model_id == "yolo":
            raise ImportError("YOLO classifiers are outside the MI355X hot path (ResNet-18 / ResNet-34 only) under the id 'yolo': "
                              "name the architecture -- classifier_model_id='yolov8m-cls' (or n / s / l / x) runs a YOLOv8-cls checkpoint")
        if model_id is None:
            # the reference tries YOLO first and falls back to ResNet-18 on ImportError (core.py:113-130)
            logger.info("YOLO not available, falling back to ResNet18")
            self._classifier_model_id = "resnet18"
        weights = self._classifier_weights or constants.BEST_CLASSIFIER_WEIGHTS
        model = utils.get_classifier_model(self._classifier_model_id or "resnet18", self._get_engine("resnet18"))
        model = utils.load_model_checkpoint(model, weights, self.device)
        self._classifier_weights = weights
        model.eval()
        model.to(self.device)
        self._classifier = model

    # ---- pipeline -----------------------------------------------------------------------------------
    def process_image(self, image: NDArray[np.uint8], threshold: float = 0.5, flip: bool = False) -> ChessVisionResult:
        """Raw BGR image -> board extraction -> (if a board was found) position (reference core.py:152-195)."""
        assert isinstance(image, np.ndarray), "Image must be a numpy array"
        assert image.dtype == np.uint8, "Image must be uint8"
        assert len(image.shape) == 3, "Image must be 3-dimensional (H,W,C)"
        logger.info("Starting image processing pipeline...")
        started = time.time()
        if image.shape[2] == 3 and self._native(self.board_extractor) and self._native(self.classifier):
            return self._recover(lambda cv: cv._process_image_native(image, threshold, flip, started))
        board_result = self.extract_board(image, threshold)
        position_result = None
        if board_result.board_image is None:
            logger.info("No valid board found in image")
        else:
            logger.info("Board successfully extracted")
            position_result = self.classify_position(board_result.board_image, flip)
            logger.info("Position classification completed")
        elapsed = time.time() - started
        logger.info(f"Processing completed in {elapsed:.2f} seconds")
        return ChessVisionResult(board_extraction=board_result, position=position_result, processing_time=elapsed)

    predict = process_image                                  # name used by BASELINE.json's north_star

    # ---- numeric-guard recovery (the reference never fails on an image: core.py:152-195 has no failure mode here) -----------------
    def _recover(self, run):
        """``run(self)``; when an f16-based engine trips its numeric guard (``NumericRangeError``: an activation of THIS checkpoint on
        THIS image left the range f16 storage holds after calibration) the request is repeated on an exact-f32 instance of the same
        checkpoints -- native kernels on the f32-input MFMA, created on first use, never the oracle -- and that result is returned.
        The tripping layer is logged once per layer.  Only the serve-path methods recover; direct engine calls
        (``HipEngine.unet_forward`` ...) keep raising, and an instance that already runs in f32 has nothing to fall back to."""
        from .hip_backend import NumericRangeError

        try:
            return run(self)
        except NumericRangeError as exc:
            if set(self._precision.split("+")) <= {"f32", "fp32", "float32"}:
                raise
            if exc.layer not in self._guard_logged:
                self._guard_logged.add(exc.layer)
                logger.warning(f"numeric guard tripped at '{exc.layer}' ({self._precision}); re-running the request on the exact f32 engine. {exc}")
            return run(self._get_f32_twin())

    def _get_f32_twin(self) -> "ChessVision":
        with self._init_lock:
            if self._f32_twin is None:
                self._f32_twin = ChessVision(board_extractor_weights=self._board_extractor_weights,
                                             board_extractor_model_id=self._board_extractor_model_id,
                                             classifier_weights=self._classifier_weights,
                                             classifier_model_id=self._classifier_model_id, lazy_load=True, precision="f32")
        return self._f32_twin

    def _native(self, model) -> bool:
        from .hip_backend import _HipModel
        return isinstance(model, _HipModel)

    def extract_board(self, image: NDArray[np.uint8], threshold: float = 0.5) -> BoardExtractionResult:
        """Reference core.py:197-223 + 252-307.  With the HIP extractor plugged in every stage runs natively (see the module
        docstring); any other model object gets the reference's literal tensor path and the numpy stages."""
        model = self.board_extractor
        if self._native(model) and image.ndim == 3 and image.shape[2] == 3 and image.dtype == np.uint8:
            return self._recover(lambda cv: cv._extract_board_native(cv.board_extractor.engine, image, threshold))
        comp_image = classical.resize_area(image, constants.INPUT_SIZE)
        batch = torch.Tensor(np.array([comp_image])) / 255           # (1,256,256,3) float32, channels as given
        batch = batch.permute(0, 3, 1, 2).to(self.device)
        with torch.no_grad():
            logits = model(batch)[0].squeeze().cpu().numpy()
        return self.process_board_extraction_logits(logits, image, threshold)

    def classify_position(self, board_image: NDArray[np.uint8], flip: bool = False) -> PositionResult:
        """Reference core.py:225-249 + 309-355."""
        model = self.classifier
        if self._native(model) and board_image.dtype == np.uint8 and board_image.shape == (constants.BOARD_SIZE[1], constants.BOARD_SIZE[0]):
            return self._recover(lambda cv: cv._classify_position_native(cv.classifier.engine, board_image, flip))
        squares = self.extract_squares(board_image)
        square_names = constants.SQUARE_NAMES_FLIPPED if flip else constants.SQUARE_NAMES_NORMAL
        batch = torch.Tensor(squares).permute(0, 3, 1, 2).to(self.device)
        batch /= 255.0
        with torch.no_grad():
            predictions = model(batch)
            probabilities = torch.softmax(predictions, dim=1)
            probabilities_np = probabilities.detach().cpu().numpy()
        return self.process_position_probabilities(probabilities=probabilities_np, square_names=square_names,
                                                   square_crops=squares)

    # ---- the native single-image path -----------------------------------------------------------------
    def _process_image_native(self, image, threshold, flip, started, fallback_quad: bool = False, encoded: bool = False,
                              apply_orientation: bool = False) -> ChessVisionResult:
        """``process_image`` as ONE native call (``cv_process_image``): upload, resize, UNet, mask, contours, homography, warp, split,
        classifier, soft-max, FEN and the pawn rule all happen behind the C ABI; Python only wraps the arrays into the result records.
        ``encoded``: ``image`` is a JPEG stream and the call is ``cv_process_jpeg``, which decodes it behind the C ABI as well
        (``apply_orientation``: ``cv_process_jpeg_oriented``, which also turns the photo as its EXIF orientation says)."""
        from .hip_backend import process_image_native, process_jpeg_native

        extra = {"apply_orientation": True} if encoded and apply_orientation else {}
        slot = self._acquire_slot()
        try:
            r = (process_jpeg_native if encoded else process_image_native)(
                slot.extractor_engine, slot.classifier_engine, image, threshold, flip, fallback_quad, stream=slot.stream.cuda_stream, **extra)
        finally:
            self._release_slot(slot)
        if not r["found"]:
            logger.info("No valid board found in image")
            extraction = BoardExtractionResult(board_image=None, binary_mask=r["mask"], quadrangle=None, probabilities=r["logits"])
            return ChessVisionResult(board_extraction=extraction, position=None, processing_time=time.time() - started)
        names = constants.SQUARE_NAMES_FLIPPED if flip else constants.SQUARE_NAMES_NORMAL
        fixes = [pawn_rule_fix(names, *fix) for fix in r["fixes"]]
        extraction = BoardExtractionResult(board_image=r["board"], binary_mask=r["mask"], quadrangle=r["quadrangle"], probabilities=r["logits"])
        position = PositionResult(fen=r["fen"], original_fen=r["original_fen"], model_probabilities=r["probabilities"],
                                  squares=r["squares"], square_names=names, validation_fixes=fixes)
        elapsed = time.time() - started
        logger.info(f"Processing completed in {elapsed:.2f} seconds")
        return ChessVisionResult(board_extraction=extraction, position=position, processing_time=elapsed)

    # ---- request slots ----------------------------------------------------------------------------------------------------------
    def _acquire_slot(self) -> _RequestSlot:
        """A free slot, waiting for one if all are in flight.  The first request creates slot 0 around the primary engines; a request
        that finds every slot busy starts ONE background thread that loads a replica pair (a few seconds: pack + calibrate, while the
        existing slots keep serving) until ``CHESSVISION_REQUEST_SLOTS`` (default 4) exist -- so a single-threaded caller never pays for
        replicas, and a threaded server reaches its full width after its first busy seconds."""
        extractor, classifier = self.board_extractor, self.classifier      # lazy initialisation outside the slot lock
        first = None
        with self._slot_cond:
            if not self._slots:
                first = _RequestSlot(extractor.engine, classifier.engine, torch.cuda.Stream(self.device))
                first.busy = True
                self._slots.append(first)
        if first is not None:
            self._warm_slot(first)
            return first
        with self._slot_cond:
            while True:
                for slot in self._slots:
                    if not slot.busy:
                        slot.busy = True
                        return slot
                if len(self._slots) < self._max_slots and not self._slot_building:
                    self._slot_building = True
                    threading.Thread(target=self._build_slot, name="chessvision-slot-builder", daemon=True).start()
                self._slot_cond.wait()

    def _release_slot(self, slot: _RequestSlot) -> None:
        with self._slot_cond:
            slot.busy = False
            self._slot_cond.notify()

    def _build_slot(self) -> None:
        from .hip_backend import HipEngine

        try:
            parts = self._precision.split("+")
            engines = {}
            for prec in dict.fromkeys(parts):
                engines[prec] = HipEngine(self.device, precision=prec)
            unet_eng, cls_eng = engines[parts[0]], engines[parts[-1]]
            state, _ = utils.read_checkpoint(self._board_extractor_weights or constants.BEST_EXTRACTOR_WEIGHTS)
            unet_eng.load_unet(state)
            arch = getattr(self._classifier, "model_name", "") or "resnet18"  # the architecture of the primary classifier
            state, _ = utils.read_classifier_checkpoint(self._classifier_weights or constants.BEST_CLASSIFIER_WEIGHTS, arch)
            utils.load_classifier_state(cls_eng, arch, state)
            slot = _RequestSlot(unet_eng, cls_eng, torch.cuda.Stream(self.device))
            self._warm_slot(slot)
        except Exception as exc:                                            # no replica: the instance keeps serving with what it has
            logger.warning(f"request slot {len(self._slots)} could not be created ({exc}); staying at {len(self._slots)} slot(s)")
            with self._slot_cond:
                self._max_slots = len(self._slots)
                self._slot_building = False
                self._slot_cond.notify_all()
            return
        with self._slot_cond:
            self._slots.append(slot)
            self._slot_building = False
            self._slot_cond.notify_all()

    def _warm_slot(self, slot: _RequestSlot) -> None:
        """Two requests on a blank photo through a slot nobody else can see yet, one slot of the PROCESS at a time.  The HIP runtime binds
        a stream to a hardware queue when the stream is first used, and streams first used at the same moment end up sharing queues:
        four slots whose first requests arrived together served 1850-1880 requests/s for the rest of the process's life, the same slots
        first used one after the other 2340-2370 (profiles/r06_tuning.md section 5).  The two calls also grow the slot's workspace and
        record its hipGraphs, so the first real request on a new slot is as fast as any other."""
        from .hip_backend import process_image_native
        blank = np.zeros((512, 512, 3), dtype=np.uint8)
        with _FIRST_USE_LOCK:
            try:
                for _ in range(2):
                    process_image_native(slot.extractor_engine, slot.classifier_engine, blank, 0.5, False, True, stream=slot.stream.cuda_stream)
            except Exception as exc:                                        # a warm-up only: the slot serves without it
                logger.warning(f"request slot warm-up failed ({exc})")

    def warm_request_slots(self, n: int | None = None) -> int:
        """Create request slots now instead of under load (a server's start-up hook); returns how many exist afterwards."""
        want = min(self._max_slots, n or self._max_slots)
        self._release_slot(self._acquire_slot())                             # slot 0
        while True:
            with self._slot_cond:
                if len(self._slots) >= min(want, self._max_slots):
                    return len(self._slots)
                if not self._slot_building:
                    self._slot_building = True
                    threading.Thread(target=self._build_slot, name="chessvision-slot-builder", daemon=True).start()
                self._slot_cond.wait(timeout=1.0)

    def close(self) -> None:
        """Release everything the instance holds on the device and in page-locked memory NOW instead of at garbage collection: the
        primary engines, the replica engines of the request slots, the exact-f32 instance behind the numeric-guard recovery, the
        pipeline's streams, staging buffers and copy threads.  The instance goes back to its lazy state -- the next call loads the
        models again -- so a long-running server can shed its GPU memory between bursts.  Not part of the reference's surface (its
        torch modules are simply garbage-collected); idempotent.  Waits for in-flight ``process_image`` calls of other threads."""
        with self._slot_cond:
            while self._slot_building or any(slot.busy for slot in self._slots):
                self._slot_cond.wait(timeout=0.1)
            slots, self._slots = self._slots, []
        with self._init_lock, self._native_lock:
            twin, self._f32_twin = self._f32_twin, None
            engines = {id(e): e for e in self._engines.values()}
            for slot in slots:
                for e in (slot.extractor_engine, slot.classifier_engine):
                    engines.setdefault(id(e), e)
            self._engines = {}
            self._board_extractor = self._classifier = None
            self._stage, self._last_board, self._streams = {}, None, None
            pool, self._copy_pool = self._copy_pool, None
        if pool is not None:
            pool.shutdown(wait=True)
        if twin is not None:
            twin.close()
        if engines and torch.cuda.is_available():
            torch.cuda.synchronize(self.device)
        for e in engines.values():
            e.close()

    def __enter__(self) -> "ChessVision":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def _staging(self, shape=None):
        """Page-locked staging buffers of the single-image path: mask, logits, board, squares, probabilities, homography (shared),
        and one image buffer per image shape seen (a server sees few distinct camera formats)."""
        st = self._stage.get("common")
        pin = lambda s, d: torch.empty(s, dtype=d, pin_memory=True)          # noqa: E731
        if st is None:
            st = self._stage["common"] = {
                "mask": pin((256, 256), torch.uint8), "logits": pin((256, 256), torch.float32),
                "board": pin((constants.BOARD_SIZE[1], constants.BOARD_SIZE[0]), torch.uint8),
                "probs": pin((64, constants.NUM_CLASSES), torch.float32), "inv": pin((1, 9), torch.float64),
                "squares": pin((64, 64, 64), torch.uint8), "images": {}}
        if shape is not None and shape not in st["images"]:
            if len(st["images"]) >= 4:
                st["images"].clear()
            st["images"][shape] = pin(shape, torch.uint8)
        return st

    def _extract_board_native(self, eng, image: NDArray[np.uint8], threshold: float, fallback_quad: bool = False) -> BoardExtractionResult:
        from .hip_backend import board_homographies, find_quadrangle

        dev = self.device
        with self._native_lock, torch.no_grad():
            st = self._staging(tuple(image.shape))
            staged = st["images"][tuple(image.shape)]
            np.copyto(staged.numpy(), image)
            img_dev = staged.to(dev, non_blocking=True)[None]
            small = eng.resize_area_u8(img_dev, (constants.INPUT_SIZE[1], constants.INPUT_SIZE[0]))
            logits_dev, mask_dev = eng.unet_forward_u8(small, threshold=threshold, want_mask=True)
            st["mask"].copy_(mask_dev[0], non_blocking=True)                 # the contour stage waits for the mask only
            have_mask = torch.cuda.Event()
            have_mask.record()
            st["logits"].copy_(logits_dev[0, 0], non_blocking=True)
            have_mask.synchronize()
            binary_mask = st["mask"].numpy().copy()
            quadrangle = find_quadrangle(binary_mask)
            if quadrangle is None and fallback_quad:
                quadrangle = constants.WHOLE_MASK_QUADRANGLE
            if quadrangle is None:
                logger.info("Failed to extract board from image")
                eng.check_numerics()                                          # synchronises: the logits have landed
                return BoardExtractionResult(board_image=None, binary_mask=binary_mask, quadrangle=None,
                                             probabilities=st["logits"].numpy().copy())
            scaled = self._scale_quadrangle(quadrangle, (image.shape[0], image.shape[1]))
            st["inv"].numpy()[:] = board_homographies(scaled.reshape(1, 4, 2), constants.BOARD_SIZE).reshape(1, 9)
            squares_dev, board_dev = eng.extract_squares_u8(img_dev, st["inv"])
            st["board"].copy_(board_dev[0], non_blocking=True)
            eng.check_numerics()                                              # synchronises the stream: logits and board have landed
            board = st["board"].numpy().copy()
            self._last_board = (board, squares_dev, board.copy())             # process_image classifies exactly this board next (identity + content)
            return BoardExtractionResult(board_image=board, binary_mask=binary_mask, quadrangle=scaled,
                                         probabilities=st["logits"].numpy().copy())

    def _classify_position_native(self, eng, board_image: NDArray[np.uint8], flip: bool) -> PositionResult:
        from .hip_backend import decode_positions

        names = constants.SQUARE_NAMES_FLIPPED if flip else constants.SQUARE_NAMES_NORMAL
        squares = self.extract_squares(board_image)
        with self._native_lock, torch.no_grad():
            last = self._last_board
            # the board this instance just rectified AND still the same pixels (a caller may draw on the array it was handed before
            # classifying it: the reference classifies what it is given): its squares are still on the device
            if last is not None and last[0] is board_image and np.array_equal(last[2], board_image):
                squares_dev = last[1]
            else:
                st = self._staging()
                np.copyto(st["squares"].numpy(), squares[..., 0])
                squares_dev = st["squares"].to(self.device, non_blocking=True)
            self._last_board = None
            probs_dev = eng.resnet18_forward_u8(squares_dev)
            st = self._staging()
            st["probs"].copy_(probs_dev, non_blocking=True)
            eng.check_numerics()                                              # synchronises
            probs = st["probs"].numpy().copy()
        fens, origs, _, fixes = decode_positions(probs[None], flip)
        fix_list = [pawn_rule_fix(names, sq, old, new) for _, sq, old, new in fixes]
        return PositionResult(fen=fens[0], original_fen=origs[0], model_probabilities=probs, squares=squares, square_names=names,
                              validation_fixes=fix_list)

    def process_images(self, images: Sequence[NDArray[np.uint8]], threshold: float = 0.5, flip: bool = False,
                       fallback_quad: bool = False, pipeline_chunk: int = 64, return_crops: bool = True,
                       timings: dict | None = None, first_job: int = 16, last_job: int = 0, resize: str = "area",
                       embeddings: bool = False, board_jpeg: int | None = None,
                       quality: str | None = None) -> list[ChessVisionResult]:
        """Batched pipeline (``chessvision/batched.py``): the native stages of ``process_image``, cut into jobs of up to
        ``pipeline_chunk`` equally sized images and software-pipelined; the first job of a call is cut to ``first_job`` images and
        the last one to ``last_job`` (0: no split).  A call whose f16-based engine reports a non-finite value is repeated as a whole
        on the exact-f32 instance (``_recover``).

        Results have the layout of ``process_image``; their arrays are views into the page-locked result buffers of the
        call (copy them if they must outlive a long-running server's memory budget).  ``PositionResult.squares`` carries the
        (64,64,64,1) crops as in the reference; throughput callers pass ``return_crops=False`` (None instead: the crops are
        ``ChessVision.extract_squares(board_image)`` and cost a 256 KB host copy per board); ``timings`` (a dict) receives
        host-side seconds per stage and event-timed GPU milliseconds.  Host worker threads (staging copies, contour stage) are
        sized per rank: ``distributed.host_threads()`` = CPUs of this process / ranks on the host, capped.

        ``quality`` ("logits" | "sigmoid"; None = off, nothing extra is launched, copied or returned) attaches an ``ExtractionQuality``
        to every result: the four scores of the reference's enrichment job (``chessvision/quality.py``).  Per job one more kernel runs
        right behind the UNet on the logits where they are (``HipEngine.extraction_scores_dev``); its 64-byte records and its
        ``v > 0.5`` mask travel back behind the logits, and the host finishes the scores after the job's classifier has been queued.
        "logits" scores the raw logits (the reference's letter), "sigmoid" their sigmoid (what the column names promise).
        ``quad_score`` is that of the quadrangle found in the mask, in mask pixels; a fallback quadrangle scores 0 like none.

        ``embeddings`` (False = off, nothing extra is launched, allocated, copied or returned) attaches an ``Embeddings`` record to
        every result: what the reference collects with 3LC's ``EmbeddingsMetricsCollector`` at ``named_modules()[52]`` of the UNet and
        ``[90]`` of the classifier (``chessvision/embeddings.py``).  Both forwards pool their hook tensor on the device, once per
        internal chunk (``HipEngine.unet_forward_u8`` / ``resnet18_forward_u8`` with ``want_embedding``); the vectors travel back
        behind the logits / probabilities into page-locked buffers of the call.  The pooling launches ride inside ``unet_ms`` /
        ``resnet_ms`` of ``timings``: there is no ``embedding_ms`` key.  ``classifier`` is None where ``position`` is None; a call
        repeated on the exact-f32 instance (``_recover``) returns that instance's embeddings.  Out of scope: the single-image
        ``process_image`` / ``cv_process_image_v2`` (its result struct does not grow), ``distributed.process_images_sharded`` (which
        does not carry ``quality`` either), the PaCMAP reduction the reference runs on the collected table, and forward hooks on the
        HIP model objects (they are not ``nn.Module``s).

        ``resize`` ("area" = the default: nothing changes, no new launch, allocation or copy) chooses how a photo becomes the UNet's
        256 x 256 input.  "area" is ``process_image``'s way, ``cv2.resize(INTER_AREA)`` to bytes (reference core.py:212).
        "antialias" is the enrichment job's way (``v2.Resize((256, 256), antialias=True)`` on a float image,
        process_pipeline.py:340-344): ``F.interpolate(u8.float() / 255, (256, 256), mode="bilinear", antialias=True,
        align_corners=False)``, computed per job by one kernel (``HipEngine.resize_antialias_f32``) into float32 NCHW that the UNet's
        float entry takes (``HipEngine.unet_forward_mask``) -- no rounding to bytes in between, so logits, scores, embeddings and
        now and then a mask pixel are those of the reference's table, not ``process_image``'s.  The warp still reads the
        full-resolution u8 photo, and ``resize_ms`` / ``unet_ms`` of ``timings`` keep their meaning.  Any other value raises
        ``ValueError`` before anything is launched; a call repeated on the exact-f32 instance keeps its mode.  Out of scope: the
        single-image ``process_image`` / ``extract_board`` / ``cv_process_image_v2`` (the core.py:212 path: they stay INTER_AREA),
        ``distributed.process_images_sharded``, torchvision's uint8 path (fixed-point weights), PIL's resize (train_unet.py:52), and
        float-tensor inputs, including the job's ``(x * 255).astype(uint8)`` round trip of the photo.

        ``board_jpeg`` (an int quality, clamped to 1..100 as libjpeg clamps it; None = off: nothing extra is launched, allocated,
        copied or returned) attaches ``result.board_jpeg``: the rectified board as a complete baseline JPEG file (``bytes``), what the
        reference's endpoint writes to ``boards/<uuid>.jpg`` -- byte for byte the file libjpeg (Pillow) writes for
        ``board_extraction.board_image`` at that quality; None where no board was found.  The encoder (``csrc/jpeg_enc.hip``) is queued
        on the boards where the warp left them, behind the classifier; the file sizes and then exactly the files' bytes travel back
        on the download stream behind events.  ``board_image`` still comes back; ``timings`` gains ``encode_ms`` (device) and
        ``fetch_jpeg_s`` (host).  A call repeated on the exact-f32 instance keeps the keyword.  Out of scope: colour, optimised
        Huffman tables, progressive, restart markers, EXIF, PNG, the single-image API, ``process_images_sharded``, ``evaluate_*`` and
        per-square files (``encode_gray`` takes the crops)."""
        if quality not in (None, "logits", "sigmoid"):
            raise ValueError(f"quality must be None, 'logits' or 'sigmoid', got {quality!r}")
        self._check_resize(resize)
        extra = self._board_jpeg_keyword(board_jpeg)
        return self._recover(lambda cv: cv._process_images_native(images, threshold, flip, fallback_quad, pipeline_chunk, return_crops,
                                                                  timings, first_job, last_job, quality, None, bool(embeddings), resize,
                                                                  **extra))

    @staticmethod
    def _board_jpeg_keyword(board_jpeg) -> dict:
        """The keyword the native calls take for ``board_jpeg``: named only when it is on, so an off call is the call it always was."""
        if board_jpeg is None:
            return {}
        if isinstance(board_jpeg, bool) or not isinstance(board_jpeg, (int, np.integer)):
            raise ValueError(f"board_jpeg must be None or an int quality, got {board_jpeg!r}")
        return {"board_jpeg": int(board_jpeg)}

    def encode_gray(self, images: Sequence[NDArray[np.uint8]], quality: int = 95) -> list[bytes]:
        """Gray host arrays ``(h, w)`` uint8 of any mix of sizes (1..4096 each way) -> complete baseline JPEG files in input order:
        byte for byte what ``PIL.Image.fromarray(a, "L").save(f, "JPEG", quality=quality)`` writes.  Images are grouped by shape
        (as ``decode_jpegs`` groups by geometry); each group is one ``HipEngine.jpeg_encode_gray``.  The 64 x 64 crops of
        ``extract_squares`` (``(64, 64, 1)`` arrays are taken too), the training-folder format, go through this."""
        arrays = [np.asarray(a) for a in images]
        for a in arrays:
            if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 1)) or a.size == 0:
                raise ValueError("encode_gray expects non-empty (h, w) or (h, w, 1) uint8 arrays")
        groups: dict[tuple, list[int]] = {}
        for i, a in enumerate(arrays):
            groups.setdefault(a.shape[:2], []).append(i)
        out: list = [None] * len(arrays)
        eng = self._get_engine("unet")
        for shape, ids in groups.items():
            step = max(1, (64 << 20) // (shape[0] * shape[1]))       # 64 MB of pixels per upload
            for k0 in range(0, len(ids), step):
                part = ids[k0:k0 + step]
                files = eng.jpeg_encode_gray(np.stack([arrays[i].reshape(shape) for i in part]), quality)
                for i, blob in zip(part, files):
                    out[i] = blob
        return out

    _ENCODE_OUT_BYTES = 256 << 20                                # what one colour encode may allocate for its files' worst case

    @classmethod
    def _colour_slice(cls, h: int, w: int, subsampling: str) -> int:
        """Images of one colour encode: its output allocation is n x ``jpeg_colour_max_bytes``, bounded here; at most 64."""
        from .hip_backend import jpeg_colour_max_bytes
        return max(1, min(64, cls._ENCODE_OUT_BYTES // jpeg_colour_max_bytes(h, w, subsampling)))

    def encode_colour(self, images: Sequence[NDArray[np.uint8]], quality: int = 95, subsampling: str = "4:2:0",
                      channel_order: str = "bgr") -> list[bytes]:
        """Colour host arrays ``(h, w, 3)`` uint8 of any mix of sizes (1..4096 each way), BGR by default -> complete baseline JPEG
        files in input order: byte for byte what ``PIL.Image.fromarray(rgb).save(f, "JPEG", quality=quality, subsampling=subsampling)``
        writes, and with the default "4:2:0" what libjpeg's defaults give (``cv2.imwrite``, which has not been run here).
        ``subsampling``: "4:2:0" | "4:2:2" | "4:4:4"; ``channel_order`` only says which byte of a pixel is R.  Images are grouped by
        shape as in ``encode_gray``; each slice of a group is one ``HipEngine.jpeg_encode_colour``.  Bad arguments raise ``ValueError``
        before an engine exists."""
        from . import jpeg

        jpeg.check_subsampling(subsampling)
        jpeg.check_colour_order(channel_order)
        arrays = [jpeg.check_colour_image(a, "encode_colour") for a in images]
        groups: dict[tuple, list[int]] = {}
        for i, a in enumerate(arrays):
            groups.setdefault(a.shape[:2], []).append(i)
        out: list = [None] * len(arrays)
        if not arrays:
            return out
        eng = self._get_engine("unet")
        for (h, w), ids in groups.items():
            step = self._colour_slice(h, w, subsampling)
            for k0 in range(0, len(ids), step):
                part = ids[k0:k0 + step]
                files = eng.jpeg_encode_colour(np.stack([arrays[i] for i in part]), quality, subsampling, channel_order)
                for i, blob in zip(part, files):
                    out[i] = blob
        return out

    def transcode_jpegs(self, blobs: Sequence[bytes], quality: int = 95, subsampling: str = "4:2:0",
                        orientation: str = "ignore") -> list[bytes]:
        """JPEG streams -> the files libjpeg writes for the photos they decode to, in input order: the reference endpoint's
        ``cv2.imwrite(raw/<uuid>.jpg, cv2.imdecode(upload))`` in one call, equal to ``encode_colour(decode_jpegs(blobs, "bgr",
        orientation), quality, subsampling)`` byte for byte -- but the pixels never leave the device.  Per (geometry, effective tag)
        group and slice: the Huffman stage on host threads, the reconstruction (with the turn when ``orientation="exif"``) and the
        colour encoder on the tensor where the decoder left it; only the files come back.  One-component streams are written as
        three-component files, as ``IMREAD_COLOR`` followed by ``imwrite`` does.  Metadata (EXIF, ICC, comments) is dropped, as
        ``imwrite`` drops it; under ``"ignore"`` a tagged photo is therefore written as stored, without its tag.  Streams the decoder
        refuses raise ``jpeg.UnsupportedJpeg`` as in ``decode_jpegs``; a photo larger than 4096 either way raises ``ValueError``;
        both before any GPU work.  Cost as it stands: each slice goes through ``HipEngine.jpeg_decode``, which waits for its stream
        once (to release its page-locked buffer) before the slice's encode is queued, so the Huffman stage of the next slice does not
        overlap the device work of this one; 256 photos of 512 x 512 take 0.05 s of wall clock (``profiles/jpeg_colour_encode.md``)."""
        from . import jpeg

        jpeg.check_orientation(orientation)
        jpeg.check_subsampling(subsampling)
        blobs = [bytes(b) for b in blobs]
        infos = jpeg.parse_all(blobs)
        large = [i for i, f in enumerate(infos) if max(f.width, f.height) > jpeg.ENCODE_MAX_SIDE]
        if large:
            raise ValueError(f"transcode_jpegs: streams {large} are larger than {jpeg.ENCODE_MAX_SIDE} pixels in width or height")
        groups: dict[tuple, list[int]] = {}
        for i, info in enumerate(infos):
            groups.setdefault(jpeg.job_key(info, orientation), []).append(i)
        out: list = [None] * len(blobs)
        if not blobs:
            return out
        eng = self._get_engine("unet")
        for (_, tag), ids in groups.items():
            h, w = jpeg.oriented_shape(infos[ids[0]], tag)
            step = self._colour_slice(h, w, subsampling)
            for k0 in range(0, len(ids), step):
                part = ids[k0:k0 + step]
                photos = eng.jpeg_decode([blobs[i] for i in part], "bgr", orientation)
                for i, blob in zip(part, eng.jpeg_encode_colour(photos, quality, subsampling, "bgr")):
                    out[i] = blob
        return out

    # ---- encoded input: JPEG streams in, the decode inside the library (chessvision/jpeg.py, csrc/jpeg.cpp, csrc/jpeg.hip) ----------
    def process_jpeg(self, blob, threshold: float = 0.5, flip: bool = False, orientation: str = "ignore") -> ChessVisionResult:
        """``process_image`` for a JPEG stream (``bytes``): one native call, ``cv_process_jpeg``, over the request slots.  The Huffman
        stage runs on the calling thread into the slot engine's page-locked block, the device reconstructs the BGR photo where
        ``process_image`` uploads one, and everything after is the same code: the result equals ``process_image`` of the decoded
        photo bit for bit.  EXIF orientation is not applied by default (``jpeg.jpeg_info(blob).orientation`` reports it);
        ``orientation="exif"`` applies it in the reconstruction (``cv_process_jpeg_oriented``): the result is ``process_image`` of
        ``jpeg.apply_orientation(photo, tag)``, quadrangle included -- what the reference computes for an upload, if ``cv2.imdecode``
        turns the photo as OpenCV's source reads (not run here).  Raises ``jpeg.UnsupportedJpeg`` (a ``ValueError``) for a stream the
        decoder refuses, before any GPU work."""
        from . import jpeg

        extra = {"apply_orientation": True} if jpeg.check_orientation(orientation) else {}
        blob = bytes(blob)
        jpeg.parse_all([blob])
        started = time.time()
        _ = self.board_extractor, self.classifier
        return self._recover(lambda cv: cv._process_image_native(blob, threshold, flip, started, encoded=True, **extra))

    def decode_jpegs(self, blobs: Sequence[bytes], channel_order: str = "bgr", orientation: str = "ignore") -> list[NDArray[np.uint8]]:
        """JPEG streams -> host arrays ``(h, w, 3)`` uint8 (BGR by default, as ``cv2.imread`` hands them over), in input order: what
        the callers that take decoded arrays (``evaluate_images``, ``evaluate_thresholds``, ``process_images_sharded``) are fed with.
        Streams are grouped by geometry; each group is one ``HipEngine.jpeg_decode`` (Huffman stage on host threads, reconstruction
        on the device).  Pixels are libjpeg's, byte for byte.  EXIF orientation is not applied unless ``orientation="exif"``: the
        groups are then (geometry, effective tag) and every array comes back upright, ``(w, h, 3)`` for the transposing tags 5..8."""
        from . import jpeg

        jpeg.check_orientation(orientation)
        blobs = [bytes(b) for b in blobs]
        infos = jpeg.parse_all(blobs)
        groups: dict[tuple, list[int]] = {}
        for i, info in enumerate(infos):
            groups.setdefault(jpeg.job_key(info, orientation), []).append(i)
        out: list = [None] * len(blobs)
        eng = self._get_engine("unet")
        for ids in groups.values():
            for k0 in range(0, len(ids), 64):
                part = ids[k0:k0 + 64]
                pixels = eng.jpeg_decode([blobs[i] for i in part], channel_order, orientation).cpu().numpy()
                for k, i in enumerate(part):
                    out[i] = pixels[k]
        return out

    def process_encoded(self, blobs: Sequence[bytes], threshold: float = 0.5, flip: bool = False, fallback_quad: bool = False,
                        pipeline_chunk: int = 64, return_crops: bool = True, timings: dict | None = None, first_job: int = 16,
                        last_job: int = 0, resize: str = "area", embeddings: bool = False, orientation: str = "ignore",
                        board_jpeg: int | None = None, quality: str | None = None) -> list[ChessVisionResult]:
        """``process_images`` for JPEG streams: every keyword and the result type are ``process_images``'s, and so are the results,
        bit for bit, of the photos the streams decode to (libjpeg's pixels, BGR; EXIF orientation not applied by default).
        ``orientation="exif"``: each photo is reconstructed as its EXIF orientation tag turns it (``jpeg.apply_orientation``), jobs
        are planned on (geometry, effective tag), and resize, quadrangle and warp work on the upright photo the device holds.

        All headers are parsed first: if any stream is unsupported (progressive, arithmetic, 12-bit, CMYK, other sampling factors,
        several scans, truncated) ``jpeg.UnsupportedJpeg`` (a ``ValueError``) lists the indices and reasons before any GPU work.  Jobs
        are planned by ``plan_jobs`` on the geometry (size, components, sampling).  In the upload stage the copy threads run the Huffman
        stage straight into the pinned staging buffer, the coefficients travel where the pixels did, and two launches at the head of
        the job's compute reconstruct its photos on the device (``chessvision/encoded.py``).  ``timings`` gains ``entropy_s`` (host
        seconds in the Huffman stage) and ``jpeg_ms`` (device).  ``board_jpeg`` as in ``process_images``."""
        from . import jpeg

        if quality not in (None, "logits", "sigmoid"):
            raise ValueError(f"quality must be None, 'logits' or 'sigmoid', got {quality!r}")
        self._check_resize(resize)
        extra = self._board_jpeg_keyword(board_jpeg)
        if jpeg.check_orientation(orientation):
            extra["orientation"] = orientation               # named only when it is on, as board_jpeg is
        blobs = [bytes(b) for b in blobs]
        infos = jpeg.parse_all(blobs)
        return self._recover(lambda cv: cv._process_encoded_native(blobs, infos, threshold, flip, fallback_quad, pipeline_chunk, return_crops,
                                                                   timings, first_job, last_job, quality, bool(embeddings), resize, **extra))

    def _process_encoded_native(self, *args, **kw) -> list[ChessVisionResult]:
        from . import encoded

        return encoded.process_encoded(self, *args, **kw)

    @staticmethod
    def _check_resize(resize) -> None:
        from .batched import RESIZE_MODES

        if resize not in RESIZE_MODES:
            raise ValueError(f"resize must be one of {RESIZE_MODES}, got {resize!r}")

    def _process_images_native(self, *args, **kw) -> list[ChessVisionResult]:
        from . import batched

        return batched.process_images(self, *args, **kw)

    def evaluate_images(self, images: Sequence[NDArray[np.uint8]], true_fens: Sequence[str | None] | None = None,
                        label_masks: Sequence[NDArray[np.uint8] | None] | None = None, threshold: float = 0.5, flip: bool = False,
                        fallback_quad: bool = False, pipeline_chunk: int = 64, timings: dict | None = None):
        """``process_images`` plus the scores of every image against its ground truth (``chessvision/evaluation.py``): one call for
        the loop of the reference's ``scripts/eval/evaluate.py:264-360`` and for the per-image ``loss`` / ``val_dice`` of its UNet
        training side.  Returns an ``EvaluationReport``: ``results`` (exactly what ``process_images`` returns for these arguments),
        one ``ImageEvaluation`` per image and the ``aggregate`` record.

        ``true_fens`` / ``label_masks``: one entry per image, ``None`` for an unlabelled one; at least one of the two is required.
        A FEN's piece-placement field is compared square by square (row i of the probabilities with the true piece on
        ``square_names[i]``, so ``flip`` is followed); a label mask is a (256,256) uint8 array, "board" where non-zero.  A wrong
        length, shape or dtype, or a malformed FEN, raises ``ValueError`` naming the image before anything is queued.

        Per job the label masks travel to the device beside the photos, ONE more kernel runs right behind the UNet on the logits
        where they are (``HipEngine.segmentation_scores_dev``), its 64-byte records come back behind the logits, and the job's
        probabilities are scored by one native call right after its FENs are decoded.  An image with a FEN but no board found counts
        as an extraction failure, not as a zero-accuracy board.  With ``self.evaluation_embeddings = True`` (an
        attribute of the instance, default False: the argument list of this method is pinned) the call also collects the embeddings of
        ``process_images(embeddings=True)``; they are in ``report.results``.  ``self.evaluation_resize`` ("area" by default) is
        ``process_images``'s ``resize`` in the same way."""
        from .evaluation import Targets

        resize = self.evaluation_resize
        self._check_resize(resize)
        images = list(images)
        targets = Targets(len(images), true_fens, label_masks)
        results = self._recover(lambda cv: cv._process_images_native(images, threshold, flip, fallback_quad, pipeline_chunk, True,
                                                                     timings, 16, 0, None, targets, bool(self.evaluation_embeddings),
                                                                     resize))
        return targets.report(results)

    def evaluate_thresholds(self, images: Sequence[NDArray[np.uint8]], thresholds: Sequence[float],
                            true_fens: Sequence[str | None] | None = None,
                            label_masks: Sequence[NDArray[np.uint8] | None] | None = None, flip: bool = False,
                            fallback_quad: bool = False, pipeline_chunk: int = 64, timings: dict | None = None):
        """``evaluate_images`` at every mask threshold of ``thresholds`` for ONE upload, resize and UNet pass per job: the sweep the
        reference runs from outside (``scripts/eval/evaluate.py --threshold``, plotted by ``scripts/plot_sweep.py``).  Returns a
        ``ThresholdSweepReport`` (``chessvision/evaluation.py``): ``thresholds`` (the caller's values in the caller's order),
        ``reports`` (one ``EvaluationReport`` per threshold, what ``evaluate_images(..., threshold=t)`` returns), ``at(t)``,
        ``curve`` (every key of ``aggregate`` but ``avg_time_per_prediction``, plus ``mean_pixel_accuracy``, as lists aligned with
        ``thresholds``), ``best(key)``, ``boards_found`` and ``boards_classified``.

        ``thresholds``: 1 to 32 values in [0, 1], no two equal as float32, in any order; anything else raises ``ValueError`` before
        anything is queued.  Ground truth follows ``evaluate_images``: at least one of ``true_fens`` / ``label_masks``, checked first.

        Per job one kernel behind the UNet turns the logits into a level map (one byte per pixel: the number of thresholds the
        pixel's sigmoid exceeds, so every threshold's mask is a comparison of it) and every threshold's segmentation counts
        (``HipEngine.threshold_levels_dev``); the host finds the quadrangles of all T masks in one native call, and the warp and
        the classifier run once per DISTINCT quadrangle of an image (``evaluation.plan_threshold_groups``), not once per threshold
        (``chessvision/sweep.py``).  Against ``evaluate_images`` at the same threshold: logits, mask, quadrangle, board, crops and
        the segmentation scores are bit for bit the same; the probabilities agree to the cross-batch bar (1e-4), because a board
        classified in a group of another size takes another launch plan.

        The reports SHARE arrays: the logits always, board, crops, probabilities and per-square scores wherever two thresholds
        found the same quadrangle.  They are views into the call's page-locked buffers: copy before writing.
        ``self.evaluation_resize`` and ``self.evaluation_embeddings`` are honoured as in ``evaluate_images`` (the UNet embedding is
        shared by all thresholds, the classifier embedding follows the board).  ``processing_time`` of a result is the call's
        time divided by the number of images.  Out of scope: the single-image API, ``process_images_sharded``, ``quality=``."""
        from .evaluation import Targets, ThresholdSweepReport, check_thresholds

        if not isinstance(thresholds, (list, tuple, np.ndarray)):
            raise ValueError(f"thresholds must be a list, tuple or array of numbers, got {type(thresholds).__name__}")
        asked = check_thresholds(thresholds)
        resize = self.evaluation_resize
        self._check_resize(resize)
        images = list(images)
        targets = Targets(len(images), true_fens, label_masks)
        ascending = np.sort(asked)
        order = [int(np.searchsorted(ascending, t)) for t in asked]
        given = [float(t) for t in thresholds]               # returned as given; compared as float32 everywhere
        if not images:
            return ThresholdSweepReport.from_reports(given, [targets.report([]) for _ in asked])
        embeddings = bool(self.evaluation_embeddings)
        report = self._recover(lambda cv: cv._evaluate_thresholds_native(images, ascending, order, targets, flip, fallback_quad,
                                                                         pipeline_chunk, timings, embeddings, resize))
        report.thresholds = given
        return report

    def _evaluate_thresholds_native(self, *args):
        from . import sweep

        return sweep.evaluate_thresholds(self, *args)

    def evaluate_squares(self, squares: NDArray[np.uint8], labels=None, normalize="train", batch_size: int = 512,
                         embeddings: bool = False):
        """The classifier's validation pass over a table of squares: one call for ``validate()`` and the ``tlc.collect_metrics`` pass
        of the reference's ``scripts/train/train_classifier.py`` (:90-111, :274-292).  Returns a ``SquaresReport``
        (``chessvision/evaluation.py``): per square ``predicted``, ``confidence``, ``loss``, ``correct`` and ``rank``, optionally
        ``embeddings`` (N,512), and ``aggregate`` (``val_loss``, ``val_acc``, top-k hits, confusion matrix ...).

        ``squares``: (N,64,64) uint8, gray.  ``labels``: N class indices (-1 or None = unlabelled), label names in
        ``constants.LABEL_NAMES`` order or the reference's folder names ("_b" for "b"), or None: then ``loss`` is NaN and ``rank``
        -1 everywhere.  ``normalize``: "train" = ``constants.CLASSIFIER_NORMALIZATION``, the ``Normalize`` of the reference's
        ``val_transforms``; a (mean, std) pair; or None = the plain ``/255`` of ``classify_position``.  The transform runs inside
        the stem kernel, bit for bit ``ToTensor`` + ``Normalize``.

        The squares go up through page-locked staging in pieces of at most one engine chunk, the forward runs on the whole piece,
        the logits never visit the host: one more kernel makes a 32-byte record per square (``HipEngine.square_records_dev``) and
        only the records and the embeddings come back.  ``batch_size`` ONLY shapes the ``val_loss`` average (the mean over
        consecutive batches of each batch's mean loss, as ``validate()`` forms it); it does NOT split the forward, because a
        forward's bits depend on its batch shape.  A call whose f16-based engine reports a non-finite value is repeated on the
        exact-f32 instance (``_recover``).  A classifier that is not a HIP model raises ``TypeError``.  Out of scope: crops that are
        not 64 x 64 gray (PIL's ``Resize`` / ``Grayscale``), the training transforms, 3LC itself."""
        from .evaluation import square_label_indices

        if not self._native(self.classifier):
            raise TypeError("evaluate_squares needs the HIP classifier (HipPieceClassifier); there is no other path")
        sq = np.asarray(squares)
        if sq.dtype != np.uint8 or sq.ndim != 3 or sq.shape[1:] != (constants.PIECE_SIZE[1], constants.PIECE_SIZE[0]):
            raise ValueError(f"evaluate_squares expects (N,64,64) uint8 squares, got {sq.dtype} {sq.shape}")
        lab = square_label_indices(labels, sq.shape[0])
        if normalize is None:
            norm = (0.0, 1.0)                                # (v - 0) / 1 == v bit for bit: the /255 input, logits out
        elif isinstance(normalize, str):
            if normalize != "train":
                raise ValueError(f"normalize must be 'train', a (mean, std) pair or None, got {normalize!r}")
            norm = constants.CLASSIFIER_NORMALIZATION
        else:
            norm = (float(normalize[0]), float(normalize[1]))
            if len(normalize) != 2 or not (np.isfinite(norm[0]) and np.isfinite(norm[1]) and norm[1] > 0):
                raise ValueError(f"normalize must be a finite (mean, std) pair with std > 0, got {normalize!r}")
        return self._recover(lambda cv: cv._evaluate_squares_native(sq, lab, norm, int(batch_size), bool(embeddings)))

    def _evaluate_squares_native(self, sq, lab, norm, batch_size: int, embeddings: bool):
        from .evaluation import SquareScores, SquaresReport
        from .hip_backend import SQUARE_RECORD, square_records_finish

        eng = self.classifier.engine
        n = int(sq.shape[0])
        piece = max(1, min(int(eng.resnet_chunk), n))
        labelled = bool((lab >= 0).any())
        with self._native_lock, torch.no_grad():
            pin = lambda s, d: torch.empty(s, dtype=d, pin_memory=True)      # noqa: E731
            stage = [pin((piece, 64, 64), torch.uint8) for _ in range(2 if n > piece else 1)]
            sent = [None] * len(stage)                       # the upload that last read each staging buffer
            rec_host = pin((n, SQUARE_RECORD.itemsize), torch.uint8)
            emb_host = pin((n, 512), torch.float32) if embeddings else None
            for k, lo in enumerate(range(0, n, piece)):
                hi = min(n, lo + piece)
                buf = stage[k % len(stage)]
                if sent[k % len(stage)] is not None:
                    sent[k % len(stage)].synchronize()
                np.copyto(buf.numpy()[:hi - lo], sq[lo:hi])
                dev = buf[:hi - lo].to(self.device, non_blocking=True)
                sent[k % len(stage)] = torch.cuda.Event()
                sent[k % len(stage)].record()
                lab_dev = torch.from_numpy(lab[lo:hi]).to(self.device) if labelled else None
                out = eng.resnet_forward_u8_norm(dev, norm, want_embedding=embeddings)
                logits = out[0] if embeddings else out
                rec_host[lo:hi].copy_(eng.square_records_dev(logits, lab_dev), non_blocking=True)
                if embeddings:
                    emb_host[lo:hi].copy_(out[1], non_blocking=True)
            eng.check_numerics()                             # synchronises: records and embeddings have landed
            records = rec_host.numpy().view(SQUARE_RECORD).reshape(-1).copy()
            emb = emb_host.numpy().copy() if embeddings else None
        return SquaresReport(scores=SquareScores.from_records(records), embeddings=emb,
                             aggregate=square_records_finish(records, batch_size))

    def embedding_neighbours(self, queries, corpus=None, k: int = 10, exclude_self=None):
        """The exact k nearest neighbours of every row of an embedding table (``chessvision/embeddings.py``: ``neighbours`` is the
        definition) -- the graph the reference's PaCMAP reduction starts from, and the direct answer to "which earlier uploads look
        like this one".  ``queries`` / ``corpus``: (rows, channels) host arrays or device tensors, e.g. ``embeddings.stack(results)``;
        ``corpus=None``: the table against itself without each row's own entry.  Returns a ``Neighbours`` of numpy arrays.  With a HIP
        model plugged in the search runs on its engine, on the caller's current stream, and equals the numpy form bit for bit;
        otherwise the numpy form itself runs."""
        from . import embeddings as emb

        model = next((m for m in (self._classifier, self._board_extractor) if m is not None and self._native(m)), None)
        if model is None:                                    # nothing loaded yet counts as "no HIP model": no checkpoint is read for this
            return emb.neighbours(queries, corpus, k, exclude_self)
        with torch.cuda.device(self.device):
            return model.engine.embedding_neighbours(queries, corpus, k, exclude_self)

    def reduce_embeddings(self, table, method: str = "pacmap", n_neighbors=None, seed: int = 0, init="pca"):
        """An embedding table reduced to 2-D for browsing -- what the reference asks 3LC for right after collecting the table
        (``run.reduce_embeddings_by_foreign_table_url(..., method="pacmap")``).  ``table``: (N, C) host array or tensor, e.g.
        ``embeddings.stack(results)[0]``; ``init``: "pca" or an (N, 2) array of starting coordinates.  Returns a ``Reduction``
        (``coordinates`` (N, 2) float32, the pairs, the neighbour search's record).  ``chessvision/embeddings.py``: ``pacmap`` is the
        definition, a reading of the paper and of the package's defaults.  With a HIP model plugged in the pairs and the optimiser
        run on its engine, on the caller's current stream, and equal the numpy form bit for bit; otherwise the numpy form itself runs.
        Only ``method="pacmap"`` exists."""
        from . import embeddings as emb

        if method != "pacmap":
            raise ValueError(f"method must be 'pacmap', got {method!r}")
        model = next((m for m in (self._classifier, self._board_extractor) if m is not None and self._native(m)), None)
        if model is None:
            return emb.pacmap(table, n_neighbors=n_neighbors, seed=seed, init=init)
        pre, start = emb.pacmap_inputs(table, init)
        with torch.cuda.device(self.device):
            pairs = model.engine.pacmap_pairs(pre, n_neighbors, seed=seed)
            coords = model.engine.pacmap_optimise(start, pairs)
        return emb.Reduction(coords, pairs, int(pairs.neighbours.shape[1]), pairs.stats)

    def fit_embedding_map(self, table, method: str = "pacmap", n_neighbors=None, seed: int = 0, init="pca"):
        """``reduce_embeddings`` that keeps what placing other tables into the same map needs -- the first half of the reference's
        ``run.reduce_embeddings_by_foreign_table_url``, which fits the reducer on one table (the training set's embeddings) and
        applies it to every other table of the run.  Returns an ``embeddings.EmbeddingMap``; its ``reduction`` is what
        ``reduce_embeddings`` returns for the same arguments.  ``embeddings.pacmap_fit`` is the definition; with a HIP model plugged
        in the pairs, the optimiser and the basis rows' scale run on its engine and equal it bit for bit.  ``embeddings.save_map``
        / ``load_map`` keep a map across restarts."""
        from . import embeddings as emb

        if method != "pacmap":
            raise ValueError(f"method must be 'pacmap', got {method!r}")
        model = next((m for m in (self._classifier, self._board_extractor) if m is not None and self._native(m)), None)
        if model is None:
            return emb.pacmap_fit(table, n_neighbors=n_neighbors, seed=seed, init=init)
        pre, start, parameters = emb.pacmap_fit_inputs(table, init)
        with torch.cuda.device(self.device):
            pairs = model.engine.pacmap_pairs(pre, n_neighbors, seed=seed)
            coords = model.engine.pacmap_optimise(start, pairs)
            nn = int(pairs.neighbours.shape[1])
            sigma = model.engine.pacmap_basis_scale_dev(torch.tensor(pre).to(self.device), nn).cpu().numpy()
        return emb.map_from_fit(emb.Reduction(coords, pairs, nn, pairs.stats), pre, sigma, parameters)

    def place_embeddings(self, map, table, init="pca"):
        """Other rows -- the validation set, an earlier epoch, tonight's uploads -- placed into a fitted map (``fit_embedding_map``),
        whose points stay where they are: the second half of ``run.reduce_embeddings_by_foreign_table_url``.  ``table``: (Q, C) host
        array or tensor with the channels the map was fitted on; ``init``: "pca" (the fit's start evaluated at the new rows) or a
        (Q, 2) array.  Returns an ``embeddings.Placement`` (``coordinates`` (Q, 2) float32, the basis rows each new row was pulled
        towards, the neighbour search's record).  ``embeddings.pacmap_transform`` is the definition, a reading of the package's
        ``transform``; with a HIP model plugged in the pairs and all 450 steps (one launch) run on its engine, on the caller's
        current stream, and equal it bit for bit; otherwise the numpy form itself runs."""
        from . import embeddings as emb

        model = next((m for m in (self._classifier, self._board_extractor) if m is not None and self._native(m)), None)
        if model is None:
            return emb.pacmap_transform(map, table, init=init)
        pre_new, start = emb.pacmap_transform_inputs(map, table, init)
        with torch.cuda.device(self.device):
            nbr, stats = model.engine.pacmap_place_pairs(map, pre_new)
            coords = model.engine.pacmap_place(start, map.reduction.coordinates, nbr)
        return emb.Placement(coords, nbr, stats)

    def _pipeline_streams(self):
        """(host->device, device->host, compute) streams of ``process_images``, created once per instance."""
        if self._streams is None:
            self._streams = (torch.cuda.Stream(self.device), torch.cuda.Stream(self.device), torch.cuda.Stream(self.device))
        return self._streams

    # ---- host-side post-processing (static, usable without models) ----------------------------------
    @staticmethod
    def process_board_extraction_logits(logits: NDArray[np.float32], orig_image: NDArray[np.uint8],
                                        threshold: float) -> BoardExtractionResult:
        assert isinstance(logits, np.ndarray), "Logits must be a numpy array"
        assert logits.dtype == np.float32, "Logits must be float32"
        assert isinstance(orig_image, np.ndarray), "Original image must be a numpy array"
        assert orig_image.dtype == np.uint8, "Original image must be uint8"
        probabilities = torch.sigmoid(torch.from_numpy(logits)).numpy()
        binary_mask = utils.create_binary_mask(probabilities, threshold)
        quadrangle = ChessVision._find_quadrangle(binary_mask)
        if quadrangle is None:
            logger.info("Failed to extract board from image")
            return BoardExtractionResult(board_image=None, binary_mask=binary_mask, quadrangle=None, probabilities=logits)
        scaled = ChessVision._scale_quadrangle(quadrangle, (orig_image.shape[0], orig_image.shape[1]))
        assert scaled.dtype == np.float32, "Scaled quadrangle must be float32"
        board = utils.extract_perspective(orig_image, scaled, constants.BOARD_SIZE)
        board = classical.flip_horizontal(classical.bgr_to_gray(board))
        return BoardExtractionResult(board_image=board, binary_mask=binary_mask, quadrangle=scaled, probabilities=logits)

    @staticmethod
    def process_position_probabilities(probabilities: NDArray[np.float32], square_names: list[str],
                                       square_crops: NDArray[np.uint8]) -> PositionResult:
        best = np.argmax(probabilities, axis=1)
        labels = [constants.LABEL_NAMES[i] for i in best]
        original_fen = board_fen(labels, square_names)
        validated, fixes = ChessVision.validate_position(labels, probabilities, square_names)
        return PositionResult(fen=board_fen(validated, square_names), original_fen=original_fen,
                              model_probabilities=probabilities, squares=square_crops, square_names=square_names,
                              validation_fixes=fixes)

    @staticmethod
    def _find_quadrangle(mask: NDArray[np.uint8]) -> NDArray[np.int32] | None:
        """First contour that simplifies (epsilon = 10% of its perimeter) to exactly four vertices."""
        contours = classical.find_contours(mask)
        if len(contours) > 1:
            contours = ChessVision._filter_contours((mask.shape[0], mask.shape[1]), contours)
        for contour in contours:
            candidate = classical.approx_poly_dp(contour, 0.1 * classical.arc_length(contour, True))
            if len(candidate) == 4:
                return ChessVision._rotate_quadrangle(candidate)
        return None

    @staticmethod
    def _filter_contours(img_shape: tuple[int, int], contours: list[NDArray[np.int32]], min_ratio_bounding: float = 0.6,
                         min_area_percentage: float = 0.35, max_area_percentage: float = 1.0) -> list[NDArray[np.int32]]:
        """Keep contours covering 35%..100% of the mask whose bounding box is at least 0.6 square."""
        mask_area = float(img_shape[0] * img_shape[1])
        kept = []
        for contour in contours:
            share = classical.contour_area(contour) / mask_area
            if not (min_area_percentage <= share <= max_area_percentage):
                continue
            _, _, w, h = classical.bounding_rect(contour)
            if utils.ratio(h, w) >= min_ratio_bounding:
                kept.append(contour)
        return kept

    @staticmethod
    def _rotate_quadrangle(approx: NDArray[np.int32]) -> NDArray[np.int32]:
        """Start the vertex list at the top-right corner (the list runs counter-clockwise on screen)."""
        if approx[0, 0, 0] < approx[2, 0, 0]:
            approx = approx[[3, 0, 1, 2], :, :]
        return approx

    @staticmethod
    def _scale_quadrangle(approx: NDArray[np.int32], orig_size: tuple[int, int]) -> NDArray[np.float32]:
        """256-px mask coordinates -> input-image pixels; the factor uses the HEIGHT only (reference core.py:416)."""
        return np.array(approx * (orig_size[0] / 256.0), dtype=np.float32)

    @staticmethod
    def extract_squares(board: NDArray[np.uint8]) -> NDArray[np.uint8]:
        """(H, W) board -> (64, H/8, W/8, 1) squares in reading order a8..h8, ..., a1..h1."""
        h, w = board.shape
        sh, sw = h // 8, w // 8
        tiles = board[: sh * 8, : sw * 8].reshape(8, sh, 8, sw).swapaxes(1, 2)
        return tiles.reshape(64, sh, sw, 1)

    @staticmethod
    def validate_position(pred_labels: list[str], probabilities: NDArray[np.float32],
                          square_names: list[str]) -> tuple[list[str], list[ValidationFix]]:
        """Rule 1 (the only live rule in the reference, core.py:453-469): a pawn predicted on rank 1 or 8 is
        replaced by the most probable non-pawn class.  ``pred_labels`` is modified in place, as in the reference."""
        fixes: list[ValidationFix] = []
        order = np.argsort(probabilities)
        for i, (label, name) in enumerate(zip(pred_labels, square_names)):
            if label not in ("P", "p") or name not in constants.INVALID_PAWN_SQUARES:
                continue
            for alt in order[i][::-1]:
                piece = constants.LABEL_NAMES[alt]
                if piece not in ("P", "p"):
                    fixes.append(ValidationFix(square_name=name, original_piece=label, corrected_piece=piece,
                                               rule_name="no_pawns_on_ends"))
                    pred_labels[i] = piece
                    break
        return pred_labels, fixes

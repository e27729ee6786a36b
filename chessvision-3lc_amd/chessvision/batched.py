"""The batched pipeline behind ``ChessVision.process_images`` (new; the reference processes one image per call, core.py:152-195).

Images stay on the device between the two CNNs: INTER_AREA resize -> UNet (u8 in, logits + thresholded mask out; with
``resize="antialias"`` the enrichment job's antialiased bilinear resize to float32 and the UNet's float entry); only the 64 KB
masks come back for the C++ contour stage; the quadrangles go back as 3x3 maps and ONE fused warp+gray+flip+split kernel writes the
classifier input; the classifier runs with softmax on device; labels, pawn rule and FEN of a whole job are decoded by one native
call.  Work is cut into jobs of up to ``pipeline_chunk`` equally sized images (``plan_jobs``) and software-pipelined
(``_Call.issue``): host->device copies run on their own stream out of a pinned staging buffer filled by a few copy threads,
device->host copies on a third stream behind events, and while the GPU runs the UNet of job k+1 the host finds the quadrangles of
job k and decodes job k-1.  Nothing on the host blocks the compute stream.

The streams and the copy threads belong to the ``ChessVision`` instance and live across calls (the HIP runtime binds a stream to a
hardware queue at its first use); everything else here lives for one call.
"""
from __future__ import annotations

import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Sequence

import numpy as np
import torch

from . import constants
from .cv_types import BoardExtractionResult, ChessVisionResult, Embeddings, ExtractionQuality, PositionResult, pawn_rule_fix
from .distributed import host_threads
from .hip_backend import (SCORE_RECORD, SEG_RECORD, board_homographies, classification_scores, decode_positions, find_quadrangles,
                          mask_completenesses, quadrangle_regularity, scores_finish, segmentation_scores_finish)

RESIZE_MODES = ("area", "antialias")
_HOST_STAGES = ("stage_s", "wait_masks_s", "contours_s", "homography_s", "wait_probs_s", "decode_s", "assemble_s")


def plan_jobs(shapes: Sequence[tuple], pipeline_chunk: int, first: int, last: int) -> list[list[int]]:
    """Image indices per job: images of one shape together, at most ``pipeline_chunk`` per job, in order of first appearance.

    Pipeline fill and drain are the only parts of a call the GPU does not overlap: nothing hides the staging + upload of the FIRST
    job, and after the last UNet the host still finds the LAST job's quadrangles before its classifier can start.  Both ends can
    therefore be cut short: the first job to ``first`` images, the last one to ``last`` (measured on MI355X, r03: 3578 -> 3658
    boards/s for a 16-board first job at 256 boards, although the UNet runs ~5 % slower on part-chunks); 0 switches a split off,
    and a call of one job is never split."""
    groups: dict[tuple, list[int]] = {}
    for i, shape in enumerate(shapes):
        groups.setdefault(shape, []).append(i)
    step = max(1, int(pipeline_chunk))
    jobs = [ids[k:k + step] for ids in groups.values() for k in range(0, len(ids), step)]
    if len(jobs) > 1 and 0 < first < len(jobs[0]):
        jobs = [jobs[0][:first], jobs[0][first:]] + jobs[1:]
    if len(jobs) > 2 and 0 < last and len(jobs[-1]) >= 2 * last:
        jobs = jobs[:-1] + [jobs[-1][:-last], jobs[-1][-last:]]
    return jobs


@dataclass(slots=True)
class Boards:
    """One warp + classifier launch of a job (``_Call.warp_and_classify``): ``process_images`` makes one per job, from the positions
    that have a quadrangle; a threshold sweep one per group of distinct quadrangles."""
    found: list[int]                            # positions within the job
    quads: list                                 # their quadrangles in photo pixels
    boards: torch.Tensor | None = None          # pinned (found,512,512) u8
    probs: torch.Tensor | None = None           # pinned (found*64,13) f32
    cls_emb: torch.Tensor | None = None         # pinned (found*64,512) f32 classifier embeddings, ``embeddings`` only (behind probs_ready)
    probs_ready: torch.cuda.Event | None = None     # download stream: boards and probabilities have landed
    # ``board_jpeg`` only: the encoder's device tensors (out, offsets, lengths), their pinned offsets / lengths and the event behind those
    jpeg_dev: tuple | None = None
    jpeg_offsets: torch.Tensor | None = None    # pinned (found + 1,) int64
    jpeg_lengths: torch.Tensor | None = None    # pinned (found,) int32
    jpeg_sized: torch.cuda.Event | None = None  # download stream: offsets and lengths have landed
    jpeg_bytes: torch.Tensor | None = None      # pinned: exactly the bytes the files occupy (``_Call.fetch_jpegs``)
    jpegs: list | None = None                   # the files, one ``bytes`` per board


@dataclass(slots=True)
class Job:
    """One job on its way through upload -> compute -> classify -> finish.

    Lifetime invariant: a device tensor written on one stream and read by a copy on ANOTHER stream stays referenced from the job
    until the event recorded behind that copy has been synchronised -- otherwise the caching allocator, which orders reuse against
    the allocating stream only, may hand its memory to a later job while the copy still reads it.  ``unet_out`` (read by the
    download stream up to ``logits_ready``; set by ``_Call.send_back`` alone) and ``cls_out`` (one entry per ``Boards`` record of
    ``boards``, each read up to that record's ``probs_ready``; appended by ``_Call.warp_and_classify`` alone) exist for nothing else;
    ``release`` drops them once ``finish`` has synchronised ``logits_ready`` and every record's ``probs_ready``.  ``batch`` is written
    by the upload stream and read by the compute stream: it is handed over with ``record_stream`` and dropped as soon as its last
    kernel (the last warp) is queued; ``labels`` (the label masks of an evaluation call) likewise, dropped behind the
    segmentation-score kernel.  The embeddings of an ``embeddings=True`` call and the level map and records of a threshold sweep ride
    in ``unet_out`` / ``cls_out`` like every other device tensor the download stream reads."""
    ids: list[int]
    # upload
    staged: torch.Tensor | None = None          # pinned source of the upload
    batch: torch.Tensor | None = None           # the photos on the device
    label_staged: torch.Tensor | None = None    # pinned (n,256,256) u8 label masks (zero for an image without one), evaluation only
    labels: torch.Tensor | None = None          # the label masks on the device
    arrived: torch.cuda.Event | None = None     # upload stream: the batch (and the label masks) are there
    # compute
    unet_done: torch.cuda.Event | None = None   # compute stream: UNet (and scores) queued up to here; gates the upload two jobs on
    unet_out: tuple | None = None               # device: logits, masks (or level map), every record -- held for the download stream
    masks: torch.Tensor | None = None           # pinned (n,256,256) u8: the masks, or the level map of a threshold sweep
    logits: torch.Tensor | None = None          # pinned (n,256,256) f32
    records: torch.Tensor | None = None         # pinned (n,64) u8 score records, ``quality`` only
    half: torch.Tensor | None = None            # pinned (n,256,256) u8 ``v > 0.5`` masks, ``quality`` only
    level_records: torch.Tensor | None = None   # pinned (n,320) u8 level records, threshold sweep only
    seg_records: torch.Tensor | None = None     # pinned (n,64) u8 segmentation-score records, evaluation only
    unet_emb: torch.Tensor | None = None        # pinned (n,C) f32 bottleneck embeddings, ``embeddings`` only (behind logits_ready)
    masks_ready: torch.cuda.Event | None = None     # download stream: masks have landed
    logits_ready: torch.cuda.Event | None = None    # download stream: logits (and every record, half) have landed
    # classify
    quality: list[ExtractionQuality] | None = None
    cls_out: list | None = None                 # device, per ``Boards`` record: probabilities, boards, squares -- held for the download stream
    boards: list[Boards] = field(default_factory=list)
    sweep: object | None = None                 # what a threshold sweep keeps between classify and finish (sweep.py); host arrays only

    def release(self) -> None:
        self.batch = self.labels = self.unet_out = self.cls_out = self.sweep = None


@dataclass(slots=True)
class _ImageSlot:
    """What the jobs leave behind for image i; ``assemble`` wraps it into the result records."""
    logits: np.ndarray
    mask: np.ndarray
    quad: np.ndarray | None
    quality: ExtractionQuality | None
    board: np.ndarray | None = None
    position: PositionResult | None = None
    unet_emb: np.ndarray | None = None
    cls_emb: np.ndarray | None = None
    jpeg: bytes | None = None


def _pinned(shape, dtype):
    return torch.empty(shape, dtype=dtype, pin_memory=True)


def score_positions(ids, found, probs, validated, fix_lists, true, flip) -> list:
    """The probabilities of one ``Boards`` record against the true placements (one native call): board j shows image
    ``ids[found[j]]``, ``true[i]`` holds image i's class indices in a8..h1 order or None, and row i of a board is compared with the
    true piece on ``square_names[i]``.  Returns one ``PositionScores`` per board, None for a board without a true placement."""
    from .evaluation import PositionScores, row_labels

    out: list = [None] * len(found)
    sel = [j for j, k in enumerate(found) if true[ids[k]] is not None]
    if not sel:
        return out
    rows = np.stack([row_labels(true[ids[found[j]]], flip) for j in sel])
    per_square, per_board = classification_scores(probs[sel], rows)
    # once per record: the columns as arrays of their own (the scores below hold rows of them), the accuracies as lists
    predicted, valid = per_square["predicted"].astype(np.int8), validated[sel]
    rank, conf, loss = (np.ascontiguousarray(per_square[name]) for name in ("rank", "confidence", "loss"))
    top = (per_board["hits"][:, :3] / 64).tolist()
    acc_o = (np.count_nonzero(predicted == rows, axis=1) / 64).tolist()
    acc_v = (np.count_nonzero(valid == rows, axis=1) / 64).tolist()
    mean_loss = per_board["mean_loss"].tolist()
    for m, j in enumerate(sel):
        out[j] = PositionScores(
            top_k=tuple(top[m]), accuracy_original=acc_o[m], accuracy_validated=acc_v[m], mean_loss=mean_loss[m],
            num_fixes=len(fix_lists[j]), true_labels=rows[m], predicted_labels=predicted[m], validated_labels=valid[m],
            rank=rank[m], confidence=conf[m], loss=loss[m])
    return out


class _Call:
    """The state one ``process_images`` call shares between its stages.  ``run`` makes the compute stream ``main`` the current one."""

    board_jpeg = None                                    # the class default: a call built without __init__ (the recorders) encodes nothing

    def __init__(self, cv, images, threshold, flip, fallback_quad, return_crops, timings, quality, started, targets=None,
                 embeddings=False, resize="area", board_jpeg=None):
        for image in images:
            assert isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.ndim == 3
        _ = cv.board_extractor, cv.classifier
        self.cv, self.images, self.started = cv, images, started
        self.resize = resize                             # "area" | "antialias": how a photo becomes the UNet's input (forward)
        self.targets = targets                           # evaluation.Targets of an evaluate_images call, else None
        self.embeddings = bool(embeddings)               # both forwards also pool their hook tensor (HipEngine: want_embedding)
        self.board_jpeg = None if board_jpeg is None else int(board_jpeg)   # a quality: every found board also comes back as a JPEG file
        self.threshold, self.flip, self.fallback_quad, self.return_crops, self.quality = threshold, flip, fallback_quad, return_crops, quality
        self.eng, self.eng_cls, self.dev = cv._get_engine("unet"), cv._get_engine("resnet18"), cv.device
        self.names = constants.SQUARE_NAMES_FLIPPED if flip else constants.SQUARE_NAMES_NORMAL
        self.n_host = host_threads()
        # A caller that chose no stream gets the instance's own compute stream, not the NULL stream: kernels queued on the legacy
        # stream from one thread while other threads load models / run request slots was one of the two ingredients of the device
        # faults of the round-6 soak (profiles/r06_tuning.md section 8).  Everything the call returns has been waited for through
        # events when it ends, so nothing is left to order against the caller's stream.
        self.up, self.down, own = cv._pipeline_streams()
        current = torch.cuda.current_stream(self.dev)
        self.main = own if current == torch.cuda.default_stream(self.dev) else current
        if cv._copy_pool is None:
            cv._copy_pool = ThreadPoolExecutor(max_workers=min(16, self.n_host), thread_name_prefix="cv-stage")
        self.pool = cv._copy_pool
        self.timed = timings is not None                 # no events are created for a caller that does not ask
        self.tm = timings if self.timed else {}
        for key in _HOST_STAGES:
            self.tm.setdefault(key, 0.0)
        if quality:
            self.tm.setdefault("quality", 0.0)           # host seconds of the score stage (its kernel: quality_ms)
        if targets is not None:
            self.tm.setdefault("evaluation", 0.0)        # host seconds of the ground-truth scores (the kernel: seg_ms)
        if self.board_jpeg is not None:
            self.tm.setdefault("fetch_jpeg_s", 0.0)      # host seconds waiting for the files (the kernels: encode_ms)
        self.gpu_events: list[tuple[str, torch.cuda.Event, torch.cuda.Event]] = []
        self.slots: list[_ImageSlot | None] = [None] * len(images)

    def clock(self, key, t0):
        self.tm[key] += time.perf_counter() - t0

    def gpu_timed(self, name, fn, *args, **kw):
        if not self.timed:
            return fn(*args, **kw)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(*args, **kw)
        b.record()
        self.gpu_events.append((name, a, b))
        return out

    # ---- the four stages, each once per job -------------------------------------------------------------------------------------
    def upload(self, ids, sliced=False, gate=None) -> Job:
        """host -> pinned staging -> device, on the upload stream.  ``gate``: an event of the compute stream the copy must not start
        before.  Jobs are uploaded TWO ahead, gated on the end of the previous job's UNet, so that the 50 MB copy runs beside the
        (short, HBM-light) warp + classifier phase instead of beside a UNet, whose launches it slows by 4-7 % (r03_tuning.md step 17;
        the ungated one-ahead schedule lost its same-box A/B by 3.7 %, r04_tuning.md step 12)."""
        t0 = time.perf_counter()
        images, up = self.images, self.up
        shape = images[ids[0]].shape
        job = Job(ids, staged=_pinned((len(ids),) + shape, torch.uint8))
        view = job.staged.numpy()
        with torch.cuda.stream(up):
            job.batch = torch.empty((len(ids),) + shape, dtype=torch.uint8, device=self.dev)
            if gate is not None:
                up.wait_event(gate)
        # the first job of a call is staged and uploaded in slices of 16 images (the upload of a slice overlaps the host copies
        # of the next one: nothing else hides that job's staging); later jobs are staged in one go behind the GPU's work
        step = 16 if sliced else len(ids)

        def copy_group(lo, hi):                          # one task per group of images: few Python-level dispatches, the
            for k in range(lo, hi):                      # memcpys themselves run without the GIL
                np.copyto(view[k], images[ids[k]])

        for k0 in range(0, len(ids), step):
            k1 = min(len(ids), k0 + step)
            per = max(1, -(-(k1 - k0) // 16))
            list(self.pool.map(lambda lo: copy_group(lo, min(k1, lo + per)), range(k0, k1, per)))
            with torch.cuda.stream(up):
                job.batch[k0:k1].copy_(job.staged[k0:k1], non_blocking=True)
        label_masks = [self.targets.masks[i] for i in ids] if self.targets is not None else []
        if any(m is not None for m in label_masks):      # 64 KB per image beside its photo; an image without a mask gets zeros
            job.label_staged = _pinned((len(ids), 256, 256), torch.uint8)
            lview = job.label_staged.numpy()
            for k, m in enumerate(label_masks):
                if m is None:
                    lview[k] = 0
                else:
                    np.copyto(lview[k], m)
            with torch.cuda.stream(up):
                job.labels = torch.empty((len(ids), 256, 256), dtype=torch.uint8, device=self.dev)
                job.labels.copy_(job.label_staged, non_blocking=True)
        self.clock("stage_s", t0)
        with torch.cuda.stream(up):
            job.arrived = torch.cuda.Event()
            job.arrived.record()
        return job

    def forward(self, batch, want_mask=True):
        """The photos of one job -> (logits, mask | None, embedding | None) in the call's resize mode: "area" is INTER_AREA to bytes and
        the u8 UNet entry (``process_image``'s arithmetic, reference core.py:212); "antialias" is the antialiased bilinear resize to
        float32 NCHW and the float UNet entry (the enrichment job's arithmetic, process_pipeline.py:340-344).  Two engine calls either
        way, under the same two timing keys.  ``want_mask=False`` (a threshold sweep) leaves the fused mask out."""
        eng, size = self.eng, (constants.INPUT_SIZE[1], constants.INPUT_SIZE[0])
        if self.resize == "antialias":
            small, unet = self.gpu_timed("resize_ms", eng.resize_antialias_f32, batch, size), eng.unet_forward_mask
        else:
            small, unet = self.gpu_timed("resize_ms", eng.resize_area_u8, batch, size), eng.unet_forward_u8
        # with embeddings: the same forward plus one pooling launch per chunk, inside unet_ms.  The keywords are pinned by
        # tests/test_resize_antialias_cpu.py: a masked forward names want_embedding only when it is on
        kw = {} if want_mask and not self.embeddings else {"want_embedding": self.embeddings}
        out = self.gpu_timed("unet_ms", unet, small, threshold=self.threshold, want_mask=want_mask, **kw)
        return out[0], out[1], (out[2] if self.embeddings else None)

    def begin_compute(self, job: Job) -> None:
        """The compute stream takes the job's photos over from the upload stream."""
        self.main.wait_event(job.arrived)
        job.batch.record_stream(self.main)
        self.tm.setdefault("first_enqueue_s", time.time() - self.started)   # host time until the first kernel of the call is queued

    def send_back(self, job: Job, contour_input, lg, scored=None, level=None, seg=None, emb=None) -> None:
        """The UNet's outputs start back on the download stream: ``contour_input`` ((n,256,256) u8: the masks, or a sweep's level map)
        first, then the logits and whichever records the call made -- ``scored`` (quality: records, half masks), ``level`` (sweep),
        ``seg`` (evaluation) and the embedding.  Everything that stream reads is held in ``job.unet_out`` (``Job``'s docstring)."""
        n, down = len(job.ids), self.down
        job.unet_done = torch.cuda.Event()
        job.unet_done.record()
        job.unet_out = (lg, contour_input, scored, level, seg, emb)
        job.logits, job.masks = _pinned((n, 256, 256), torch.float32), _pinned((n, 256, 256), torch.uint8)
        job.masks_ready, job.logits_ready = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(down):
            down.wait_event(job.unet_done)
            job.masks.copy_(contour_input, non_blocking=True)    # first: the contour stage waits for them only
            job.masks_ready.record()
            job.logits.copy_(lg[:, 0], non_blocking=True)
            if scored is not None:
                job.records, job.half = _pinned((n, 64), torch.uint8), _pinned((n, 256, 256), torch.uint8)
                job.records.copy_(scored[0], non_blocking=True)
                job.half.copy_(scored[1].view(n, 256, 256), non_blocking=True)
            if level is not None:
                job.level_records = _pinned(tuple(level.shape), torch.uint8)
                job.level_records.copy_(level, non_blocking=True)
            if seg is not None:
                job.seg_records = _pinned((n, 64), torch.uint8)
                job.seg_records.copy_(seg, non_blocking=True)
            if emb is not None:
                job.unet_emb = _pinned(tuple(emb.shape), torch.float32)
                job.unet_emb.copy_(emb, non_blocking=True)
            job.logits_ready.record()

    def compute(self, job: Job) -> None:
        """resize + UNet (+ the score reductions, on the logits where the UNet left them) on the compute stream; masks start back."""
        eng = self.eng
        self.begin_compute(job)
        lg, mk, emb = self.forward(job.batch)
        scored = None
        if self.quality:
            scored = self.gpu_timed("quality_ms", eng.extraction_scores_dev, lg, "none" if self.quality == "logits" else "sigmoid",
                                    want_mask=True)
        seg = None
        if job.labels is not None:                       # the ground-truth reductions, on the logits where the UNet left them
            job.labels.record_stream(self.main)
            seg = self.gpu_timed("seg_ms", eng.segmentation_scores_dev, lg, job.labels, self.threshold)
            job.labels = None
        self.send_back(job, mk, lg, scored, seg=seg, emb=emb)

    def warp_and_classify(self, job: Job, found: list[int], quads: list) -> Boards:
        """One ``Boards`` record of the job: ``quads`` are the quadrangles, in mask pixels, of the photos at positions ``found``.
        Homographies (host) -> warp + split -> classifier (device); boards and probabilities start back."""
        t0 = time.perf_counter()
        ids, down = job.ids, self.down
        rec = Boards(found, [self.cv._scale_quadrangle(q, self.images[ids[k]].shape[:2]) for k, q in zip(found, quads)])
        inv = board_homographies(np.stack([q.reshape(4, 2) for q in rec.quads]), constants.BOARD_SIZE)
        self.clock("homography_s", t0)
        src = job.batch if len(found) == len(ids) else job.batch[torch.as_tensor(found, device=self.dev)]
        squares_dev, boards_dev = self.gpu_timed("warp_ms", self.eng.extract_squares_u8, src, inv)
        warped = torch.cuda.Event()
        warped.record()
        rec.boards = _pinned((len(found), constants.BOARD_SIZE[1], constants.BOARD_SIZE[0]), torch.uint8)
        with torch.cuda.stream(down):                    # the rectified boards travel back while the classifier runs
            down.wait_event(warped)
            rec.boards.copy_(boards_dev, non_blocking=True)
        cls_emb = None
        if self.embeddings:                              # the pooled layer4 output of every square, inside resnet_ms
            probs_dev, cls_emb = self.gpu_timed("resnet_ms", self.eng_cls.resnet18_forward_u8, squares_dev, want_embedding=True)
        else:
            probs_dev = self.gpu_timed("resnet_ms", self.eng_cls.resnet18_forward_u8, squares_dev)
        done = torch.cuda.Event()
        done.record()
        rec.probs = _pinned((len(found) * 64, constants.NUM_CLASSES), torch.float32)
        job.cls_out.append((probs_dev, boards_dev, squares_dev, cls_emb))
        rec.probs_ready = torch.cuda.Event()
        with torch.cuda.stream(down):
            down.wait_event(done)
            rec.probs.copy_(probs_dev, non_blocking=True)
            if cls_emb is not None:
                rec.cls_emb = _pinned(tuple(cls_emb.shape), torch.float32)
                rec.cls_emb.copy_(cls_emb, non_blocking=True)
            rec.probs_ready.record()
        if self.board_jpeg is not None:
            self.encode_boards(job, rec, boards_dev)
        return rec

    def encode_boards(self, job: Job, rec: Boards, boards_dev) -> None:
        """``board_jpeg``: the encoder is queued on the boards where the warp left them, behind the classifier (the probabilities are
        not held back); the offsets and lengths start back on the download stream.  The device tensors ride in ``job.cls_out``."""
        m = len(rec.found)
        rec.jpeg_dev = self.gpu_timed("encode_ms", self.eng.jpeg_encode_gray_dev, boards_dev, self.board_jpeg)
        encoded = torch.cuda.Event()
        encoded.record()
        job.cls_out.append(rec.jpeg_dev)
        rec.jpeg_offsets, rec.jpeg_lengths = _pinned((m + 1,), torch.int64), _pinned((m,), torch.int32)
        rec.jpeg_sized = torch.cuda.Event()
        with torch.cuda.stream(self.down):
            self.down.wait_event(encoded)
            rec.jpeg_offsets.copy_(rec.jpeg_dev[1], non_blocking=True)
            rec.jpeg_lengths.copy_(rec.jpeg_dev[2], non_blocking=True)
            rec.jpeg_sized.record()

    def fetch_jpegs(self, recs: list) -> None:
        """The files of the landed records: once the sizes are known, exactly the bytes the files occupy (each rounded up to 16)
        travel back on the download stream -- never the worst-case capacity of the device buffer."""
        t0 = time.perf_counter()
        landed = []
        for rec in recs:
            rec.jpeg_sized.synchronize()
            total = int(rec.jpeg_offsets[-1])
            rec.jpeg_bytes = _pinned((total,), torch.uint8)
            landed.append(torch.cuda.Event())
            with torch.cuda.stream(self.down):
                rec.jpeg_bytes.copy_(rec.jpeg_dev[0][:total], non_blocking=True)
                landed[-1].record()
        for rec, event in zip(recs, landed):
            event.synchronize()
            host, off, ln = rec.jpeg_bytes.numpy(), rec.jpeg_offsets.numpy(), rec.jpeg_lengths.numpy()
            rec.jpegs = [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(off[:-1], ln)]
            rec.jpeg_dev = None
        self.clock("fetch_jpeg_s", t0)

    def classify(self, job: Job) -> None:
        """masks -> quadrangles (host) -> warp + split + classifier (device); boards and probabilities start back."""
        t0 = time.perf_counter()
        job.masks_ready.synchronize()
        self.clock("wait_masks_s", t0)
        ids = job.ids
        t0 = time.perf_counter()
        found_quads = find_quadrangles(job.masks.numpy(), n_threads=self.n_host)
        self.clock("contours_s", t0)
        quads = [constants.WHOLE_MASK_QUADRANGLE if q is None and self.fallback_quad else q for q in found_quads]
        found = [k for k, q in enumerate(quads) if q is not None]
        job.cls_out = []
        if found:
            job.boards.append(self.warp_and_classify(job, found, [quads[k] for k in found]))
        job.batch = None
        if self.quality:                                 # the device has this job's classifier queued: finish its scores meanwhile
            t0 = time.perf_counter()
            job.logits_ready.synchronize()
            conf, dist = scores_finish(job.records.numpy().view(SCORE_RECORD).reshape(-1))
            comp = mask_completenesses(job.half.numpy(), n_threads=self.n_host)
            job.quality = [ExtractionQuality(confidence=float(conf[k]), quad_score=quadrangle_regularity(found_quads[k]),
                                             completeness=float(comp[k]), distribution=float(dist[k])) for k in range(len(ids))]
            self.clock("quality", t0)
        if job.seg_records is not None:                  # the same host gap: finish the segmentation scores
            from .evaluation import SegmentationScores

            t0 = time.perf_counter()
            job.logits_ready.synchronize()
            fin = segmentation_scores_finish(job.seg_records.numpy().view(SEG_RECORD).reshape(-1))
            for k, i in enumerate(ids):
                if self.targets.masks[i] is not None:
                    self.targets.segmentation[i] = SegmentationScores(**{name: float(col[k]) for name, col in fin.items()})
            self.clock("evaluation", t0)

    def finish(self, job: Job) -> None:
        """probabilities -> labels, FEN, pawn rule (one native call per job); the job's arrays go to its images' slots."""
        ids, slots = job.ids, self.slots
        t0 = time.perf_counter()
        job.logits_ready.synchronize()
        lg, mk = job.logits.numpy(), job.masks.numpy()
        for k, i in enumerate(ids):
            slots[i] = _ImageSlot(lg[k], mk[k], None, job.quality[k] if job.quality else None)
        if job.unet_emb is not None:
            ue = job.unet_emb.numpy()
            for k, i in enumerate(ids):
                slots[i].unet_emb = ue[k]
        for rec in job.boards:
            rec.probs_ready.synchronize()
        self.clock("wait_probs_s", t0)
        if self.board_jpeg is not None and job.boards:
            self.fetch_jpegs(job.boards)
        for rec in job.boards:
            for k, (quad, board, position, cls_emb, scores) in zip(rec.found, self.decode(job, rec)):
                slot = slots[ids[k]]
                slot.quad, slot.board, slot.position, slot.cls_emb = quad, board, position, cls_emb
                if scores is not None:
                    self.targets.position[ids[k]] = scores
            if rec.jpegs is not None:
                for k, blob in zip(rec.found, rec.jpegs):
                    slots[ids[k]].jpeg = blob

    def decode(self, job: Job, rec: Boards) -> list[tuple]:
        """A landed ``Boards`` record -> per board (quadrangle, board image, ``PositionResult``, classifier-embedding rows | None,
        ``PositionScores`` | None): labels, FEN and pawn rule of all its boards by one native call, their scores against the true
        placements (an evaluation call) by another."""
        t0 = time.perf_counter()
        m, names = len(rec.found), self.names
        probs = rec.probs.numpy().reshape(m, 64, constants.NUM_CLASSES)
        brd = rec.boards.numpy()
        fens, origs, validated, fixes = decode_positions(probs, self.flip)
        fix_lists: list[list] = [[] for _ in range(m)]
        for b, sq, old, new in fixes:
            fix_lists[b].append(pawn_rule_fix(names, sq, old, new))
        positions = [PositionResult(fen=fens[j], original_fen=origs[j], model_probabilities=probs[j],
                                    squares=self.cv.extract_squares(brd[j]) if self.return_crops else None, square_names=names,
                                    validation_fixes=fix_lists[j]) for j in range(m)]
        # the embedding rows follow square_names, as the probabilities do
        cls_emb = [None] * m if rec.cls_emb is None else rec.cls_emb.numpy().reshape(m, 64, -1)
        self.clock("decode_s", t0)
        scores = [None] * m
        if self.targets is not None:
            t0 = time.perf_counter()
            scores = score_positions(job.ids, rec.found, probs, validated, fix_lists, self.targets.labels, self.flip)
            self.clock("evaluation", t0)
        return list(zip(rec.quads, brd, positions, cls_emb, scores))

    # ---- the software pipeline --------------------------------------------------------------------------------------------------
    def issue(self, jobs: list[list[int]]) -> float:
        """All jobs through the four stages; returns the host clock at which only the last job's ``finish`` was left.

        The UNet of job k+1 is enqueued before the host works on job k, and the upload of job k+2 is issued behind the end of that
        UNet.  Uses nothing of the call but the four stages: tests/test_batched_pipeline_cpu.py pins this ORDER with recorders."""
        def retire(job):
            self.finish(job)
            job.release()                                # finish has synchronised the events behind every copy of the job

        first = self.upload(jobs[0], sliced=True)
        self.compute(first)                              # the first kernels are queued before anything else is staged
        computed, uploaded, classified = first, None, None
        if len(jobs) > 1:
            uploaded = self.upload(jobs[1])              # nothing to hide behind yet: beside the (short) first job's UNet
        for k in range(len(jobs)):
            nxt = uploaded
            if nxt is not None:
                self.compute(nxt)
                uploaded = self.upload(jobs[k + 2], gate=nxt.unet_done) if k + 2 < len(jobs) else None
            self.classify(computed)
            if classified is not None:
                retire(classified)
            classified, computed = computed, nxt
        t_last = time.perf_counter()
        retire(classified)
        return t_last

    def collect(self):
        """What the call returns, once every job is finished (``run``)."""
        return self.assemble(self.slots)

    def assemble(self, slots) -> list[ChessVisionResult]:
        t0 = time.perf_counter()
        per_image = (time.time() - self.started) / len(slots)
        results = []
        for s in slots:
            extraction = BoardExtractionResult(board_image=s.board, binary_mask=s.mask, quadrangle=s.quad, probabilities=s.logits)
            emb = Embeddings(board_extractor=s.unet_emb, classifier=s.cls_emb) if self.embeddings else None
            results.append(ChessVisionResult(board_extraction=extraction, position=s.position, processing_time=per_image,
                                             quality=s.quality))
            if emb is not None:
                results[-1].embeddings = emb             # an attribute, not a constructor argument (cv_types.ChessVisionResult)
            if self.board_jpeg is not None:
                results[-1].board_jpeg = s.jpeg          # likewise; None where no board was found
        self.clock("assemble_s", t0)
        return results


def process_images(cv, images, threshold, flip, fallback_quad, pipeline_chunk, return_crops, timings, first_job, last_job,
                   quality, targets=None, embeddings=False, resize="area", board_jpeg=None) -> list[ChessVisionResult]:
    """``ChessVision.process_images`` on the instance's native engines (arguments: see there).  ``targets`` (``evaluation.Targets``,
    from ``ChessVision.evaluate_images``) additionally scores every job against its ground truth and leaves the records there;
    ``embeddings`` attaches an ``Embeddings`` record to every result; ``resize`` ("area" | "antialias") chooses how a photo becomes
    the UNet's input (``_Call.forward``); ``board_jpeg`` (an int quality, None = off) also returns every found board as a JPEG file,
    encoded on the device (``_Call.encode_boards``)."""
    started = time.time()
    if resize not in RESIZE_MODES:
        raise ValueError(f"resize must be one of {RESIZE_MODES}, got {resize!r}")
    if not images:
        return []
    call = _Call(cv, images, threshold, flip, fallback_quad, return_crops, timings, quality, started, targets, embeddings, resize, board_jpeg)
    return run(call, plan_jobs([im.shape for im in images], pipeline_chunk, first=int(first_job), last=int(last_job)))


def run(call: _Call, jobs: list[list[int]]):
    """The driver of a call: all jobs on the call's compute stream, one look at the numeric guard, the call's results
    (``call.collect()``) and its timings."""
    with torch.cuda.stream(call.main):
        t_last = call.issue(jobs)
        call.eng.check_numerics()                        # one look at the numeric guard for the whole call
        if call.eng_cls is not call.eng:
            call.eng_cls.check_numerics()
        call.tm["drain_s"] = time.perf_counter() - t_last    # last job: wait for its classifier, copies back, decode
        out = call.collect()
        if call.timed:
            for name, a, b in call.gpu_events:
                call.tm[name] = call.tm.get(name, 0.0) + a.elapsed_time(b)
            call.tm["jobs"] = len(jobs)
            call.tm["total_s"] = time.time() - call.started
    return out

"""The threshold sweep behind ``ChessVision.evaluate_thresholds``: ``evaluate_images`` at T mask thresholds for one UNet pass.

The reference sweeps the mask threshold from outside (``scripts/eval/evaluate.py --threshold``, ``scripts/plot_sweep.py``): T complete
runs.  Nothing in the upload, the resize or the UNet depends on the threshold, and contours, warp and classifier depend on it only
through the quadrangle.  So a job here runs the stages of ``batched._Call`` with three differences:

* compute: the forward leaves no mask; ONE more kernel turns the logits, where they are, into a level map -- one byte per pixel,
  ``level = #{k: sigmoid(x) > t_k}`` over the ascending thresholds, so ``mask_k == (level > k)`` -- and a 320-byte record per image
  with every threshold's segmentation counts (``HipEngine.threshold_levels_dev``).  The download stays 64 KB per image whatever T is.
  With label masks the segmentation-score kernel runs once as well: its three float sums do not depend on the threshold.
* classify: the host expands the T masks per image, finds the T * n quadrangles in one native call and plans the boards
  (``evaluation.plan_threshold_groups``): group g holds every image's g-th DISTINCT quadrangle, at most one board per image, and goes
  through homographies -> warp -> classifier exactly as a job's ``found`` subset does in ``_Call.classify``.
* finish: one decode and one scoring call per group; every threshold's result of an image points at the board, crops, probabilities
  and scores of the quadrangle it found.

The job plan, the streams and the order of the stages (``_Call.issue``) are those of ``evaluate_images``, so the logits are its logits
bit for bit.
"""
from __future__ import annotations

import contextlib
import copy
import time
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np
import torch

from . import constants
from .batched import Job, _Call, _ImageSlot, _pinned, plan_jobs
from .cv_types import PositionResult, pawn_rule_fix
from .evaluation import SegmentationScores, ThresholdSweepReport, plan_threshold_groups
from .hip_backend import (LEVEL_RECORD, SEG_RECORD, board_homographies, decode_positions, find_quadrangles,
                          segmentation_scores_finish, threshold_levels_finish)


@dataclass
class _Group:
    """One warp + classifier launch of a job: the g-th distinct quadrangle of every image that has one."""
    found: list[int]                            # positions within the job
    quads: list                                 # their quadrangles in photo pixels
    boards: torch.Tensor | None = None          # pinned (found,512,512) u8
    probs: torch.Tensor | None = None           # pinned (found*64,13) f32
    cls_emb: torch.Tensor | None = None         # pinned (found*64,512) f32, ``embeddings`` only
    probs_ready: torch.cuda.Event | None = None


@dataclass
class _Side:
    """What a sweep keeps for a job beside ``batched.Job``."""
    level_records: torch.Tensor | None = None   # pinned (n,320) u8
    masks: np.ndarray | None = None             # (T,n,256,256) u8, the expanded masks
    use: list | None = None                     # use[k][position] = index of the group that holds its board, or None
    groups: list[_Group] = field(default_factory=list)
    segmentation: list | None = None            # [k][position] SegmentationScores | None


class _SweepCall(_Call):
    """``_Call`` with the three stages above replaced; ``upload`` and ``issue`` are inherited."""

    def __init__(self, cv, images, thresholds, flip, fallback_quad, timings, started, targets, embeddings, resize):
        super().__init__(cv, images, float(thresholds[0]), flip, fallback_quad, True, timings, None, started, targets, embeddings, resize)
        self.thresholds = thresholds                     # float32, ascending
        self.side: dict[int, _Side] = {}
        T = len(thresholds)
        self.sweep_slots = [[None] * len(images) for _ in range(T)]
        self.sweep_segmentation = [[None] * len(images) for _ in range(T)]
        self.sweep_position = [[None] * len(images) for _ in range(T)]
        self.boards_found = self.boards_classified = 0

    def compute(self, job: Job) -> None:
        n, eng, down = len(job.ids), self.eng, self.down
        side = self.side[id(job)] = _Side()
        self.main.wait_event(job.arrived)
        job.batch.record_stream(self.main)
        self.tm.setdefault("first_enqueue_s", time.time() - self.started)
        size = (constants.INPUT_SIZE[1], constants.INPUT_SIZE[0])
        if self.resize == "antialias":
            small, unet = self.gpu_timed("resize_ms", eng.resize_antialias_f32, job.batch, size), eng.unet_forward_mask
        else:
            small, unet = self.gpu_timed("resize_ms", eng.resize_area_u8, job.batch, size), eng.unet_forward_u8
        out = self.gpu_timed("unet_ms", unet, small, threshold=self.threshold, want_mask=False, want_embedding=self.embeddings)
        lg, emb = out[0], (out[2] if self.embeddings else None)
        if job.labels is not None:
            job.labels.record_stream(self.main)
        levels, recs = self.gpu_timed("levels_ms", eng.threshold_levels_dev, lg, self.thresholds, job.labels)
        seg = None
        if job.labels is not None:                       # the threshold-independent sums (BCE, soft Dice): once per job
            seg = self.gpu_timed("seg_ms", eng.segmentation_scores_dev, lg, job.labels, self.threshold)
            job.labels = None
        job.unet_done = torch.cuda.Event()
        job.unet_done.record()
        job.unet_out = (lg, levels, recs, seg, emb)
        job.logits, job.masks = _pinned((n, 256, 256), torch.float32), _pinned((n, 256, 256), torch.uint8)
        side.level_records = _pinned((n, LEVEL_RECORD.itemsize), torch.uint8)
        job.masks_ready, job.logits_ready = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(down):
            down.wait_event(job.unet_done)
            job.masks.copy_(levels.view(n, 256, 256), non_blocking=True)   # the level map first: the contour stage waits for it only
            job.masks_ready.record()
            job.logits.copy_(lg[:, 0], non_blocking=True)
            side.level_records.copy_(recs, non_blocking=True)
            if seg is not None:
                job.seg_records = _pinned((n, 64), torch.uint8)
                job.seg_records.copy_(seg, non_blocking=True)
            if emb is not None:
                job.unet_emb = _pinned(tuple(emb.shape), torch.float32)
                job.unet_emb.copy_(emb, non_blocking=True)
            job.logits_ready.record()

    def classify(self, job: Job) -> None:
        t0 = time.perf_counter()
        job.masks_ready.synchronize()
        self.clock("wait_masks_s", t0)
        ids, down, side, T = job.ids, self.down, self.side[id(job)], len(self.thresholds)
        n = len(ids)
        t0 = time.perf_counter()
        levels = job.masks.numpy()
        side.masks = np.empty((T, n, 256, 256), dtype=np.uint8)
        for k in range(T):
            np.multiply(levels > k, np.uint8(255), out=side.masks[k], casting="unsafe")
        flat = find_quadrangles(side.masks.reshape(T * n, 256, 256), n_threads=self.n_host)
        self.clock("contours_s", t0)
        t0 = time.perf_counter()
        rows = []
        for k in range(T):
            row = flat[k * n:(k + 1) * n]
            if self.fallback_quad:
                row = [constants.WHOLE_MASK_QUADRANGLE if q is None else q for q in row]
            rows.append(row)
            self.boards_found += sum(q is not None for q in row)
        distinct, side.use, groups = plan_threshold_groups(rows)
        self.boards_classified += sum(len(d) for d in distinct)
        self.clock("homography_s", t0)
        job.cls_out = []
        for members in groups:
            t0 = time.perf_counter()
            found = [p for p, _ in members]
            shapes = [self.images[ids[p]].shape for p in found]
            grp = _Group(found, [self.cv._scale_quadrangle(q, (s[0], s[1])) for (_, q), s in zip(members, shapes)])
            inv = board_homographies(np.stack([q.reshape(4, 2) for q in grp.quads]), constants.BOARD_SIZE)
            self.clock("homography_s", t0)
            src = job.batch if len(found) == n else job.batch[torch.as_tensor(found, device=self.dev)]
            squares_dev, boards_dev = self.gpu_timed("warp_ms", self.eng.extract_squares_u8, src, inv)
            warped = torch.cuda.Event()
            warped.record()
            grp.boards = _pinned((len(found), constants.BOARD_SIZE[1], constants.BOARD_SIZE[0]), torch.uint8)
            with torch.cuda.stream(down):
                down.wait_event(warped)
                grp.boards.copy_(boards_dev, non_blocking=True)
            cls_emb = None
            if self.embeddings:
                probs_dev, cls_emb = self.gpu_timed("resnet_ms", self.eng_cls.resnet18_forward_u8, squares_dev, want_embedding=True)
            else:
                probs_dev = self.gpu_timed("resnet_ms", self.eng_cls.resnet18_forward_u8, squares_dev)
            done = torch.cuda.Event()
            done.record()
            grp.probs = _pinned((len(found) * 64, constants.NUM_CLASSES), torch.float32)
            job.cls_out.append((probs_dev, boards_dev, squares_dev, cls_emb, src))   # held for the download stream (Job's docstring)
            grp.probs_ready = torch.cuda.Event()
            with torch.cuda.stream(down):
                down.wait_event(done)
                grp.probs.copy_(probs_dev, non_blocking=True)
                if cls_emb is not None:
                    grp.cls_emb = _pinned(tuple(cls_emb.shape), torch.float32)
                    grp.cls_emb.copy_(cls_emb, non_blocking=True)
                grp.probs_ready.record()
            side.groups.append(grp)
        job.batch = None
        t0 = time.perf_counter()                         # the device has this job's classifiers queued: finish its mask scores meanwhile
        job.logits_ready.synchronize()
        labelled = job.seg_records is not None
        records = side.level_records.numpy().view(LEVEL_RECORD).reshape(-1)
        if labelled:
            hard = threshold_levels_finish(records, labels_present=True)
            soft = segmentation_scores_finish(job.seg_records.numpy().view(SEG_RECORD).reshape(-1))
            for k in range(T):
                for p, i in enumerate(ids):
                    if self.targets.masks[i] is not None:
                        self.sweep_segmentation[k][i] = SegmentationScores(
                            bce=float(soft["bce"][p]), dice_loss=float(soft["dice_loss"][p]), loss=float(soft["loss"][p]),
                            dice=float(hard["dice"][p, k]), iou=float(hard["iou"][p, k]),
                            pixel_accuracy=float(hard["pixel_accuracy"][p, k]))
        self.clock("evaluation", t0)

    def finish(self, job: Job) -> None:
        ids, names, side, T = job.ids, self.names, self.side.pop(id(job)), len(self.thresholds)
        t0 = time.perf_counter()
        job.logits_ready.synchronize()
        lg = job.logits.numpy()
        ue = job.unet_emb.numpy() if job.unet_emb is not None else None
        for p, i in enumerate(ids):                      # one logits (and embedding) array per image, shared by its T results
            logits, emb = lg[p], (None if ue is None else ue[p])
            for k in range(T):
                self.sweep_slots[k][i] = _ImageSlot(logits, side.masks[k, p], None, None, unet_emb=emb)
        for grp in side.groups:
            grp.probs_ready.synchronize()
        self.clock("wait_probs_s", t0)
        boards: list[dict] = []                           # per group: position -> (quad, board, PositionResult, cls_emb, PositionScores)
        for grp in side.groups:
            t0 = time.perf_counter()
            m = len(grp.found)
            probs = grp.probs.numpy().reshape(m, 64, constants.NUM_CLASSES)
            brd = grp.boards.numpy()
            fens, origs, validated, fixes = decode_positions(probs, self.flip)
            ce = grp.cls_emb.numpy().reshape(m, 64, -1) if grp.cls_emb is not None else None
            fix_lists: list[list] = [[] for _ in range(m)]
            for b, sq, old, new in fixes:
                fix_lists[b].append(pawn_rule_fix(names, sq, old, new))
            positions = [PositionResult(fen=fens[j], original_fen=origs[j], model_probabilities=probs[j],
                                        squares=self.cv.extract_squares(brd[j]), square_names=names, validation_fixes=fix_lists[j])
                         for j in range(m)]
            self.clock("decode_s", t0)
            t0 = time.perf_counter()                      # once per distinct board, through the job-level scorer of _Call
            self.score_positions(SimpleNamespace(found=grp.found, ids=ids), probs, validated, fix_lists)
            held = {}
            for j, p in enumerate(grp.found):
                held[p] = (grp.quads[j], brd[j], positions[j], None if ce is None else ce[j], self.targets.position[ids[p]])
                self.targets.position[ids[p]] = None
            boards.append(held)
            self.clock("evaluation", t0)
        for k in range(T):
            for p, i in enumerate(ids):
                g = side.use[k][p]
                if g is None:
                    continue
                slot = self.sweep_slots[k][i]
                slot.quad, slot.board, slot.position, slot.cls_emb, self.sweep_position[k][i] = boards[g][p]

    def reports(self, order) -> ThresholdSweepReport:
        """One ``EvaluationReport`` per threshold, in the caller's order: ``order[j]`` = the ascending index of the caller's j-th."""
        out = []
        for k in order:
            self.slots = self.sweep_slots[k]
            targets = copy.copy(self.targets)
            targets.segmentation, targets.position = self.sweep_segmentation[k], self.sweep_position[k]
            out.append(targets.report(self.assemble()))
        return ThresholdSweepReport.from_reports([float(self.thresholds[k]) for k in order], out, self.boards_found,
                                                 self.boards_classified)


def evaluate_thresholds(cv, images, thresholds, order, targets, flip, fallback_quad, pipeline_chunk, timings, embeddings,
                        resize) -> ThresholdSweepReport:
    """``ChessVision.evaluate_thresholds`` on the instance's native engines.  ``thresholds``: float32, ascending (checked by the
    caller); ``order[j]``: the position in it of the caller's j-th threshold; ``targets``: the checked ground truth."""
    started = time.time()
    for image in images:
        assert isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.ndim == 3
    _ = cv.board_extractor, cv.classifier
    jobs = plan_jobs([im.shape for im in images], pipeline_chunk, first=16, last=0)      # evaluate_images' plan: the same logits
    own = torch.cuda.current_stream(cv.device) == torch.cuda.default_stream(cv.device)
    with torch.cuda.stream(cv._pipeline_streams()[2]) if own else contextlib.nullcontext():
        call = _SweepCall(cv, images, thresholds, flip, fallback_quad, timings, started, targets, embeddings, resize)
        t_last = call.issue(jobs)
        call.eng.check_numerics()
        if call.eng_cls is not call.eng:
            call.eng_cls.check_numerics()
        call.tm["drain_s"] = time.perf_counter() - t_last
        report = call.reports(order)
        if timings is not None:
            for name, a, b in call.gpu_events:
                timings[name] = timings.get(name, 0.0) + a.elapsed_time(b)
            timings["jobs"] = len(jobs)
            timings["total_s"] = time.time() - started
    return report

"""The threshold sweep behind ``ChessVision.evaluate_thresholds``: ``evaluate_images`` at T mask thresholds for one UNet pass.

The reference sweeps the mask threshold from outside (``scripts/eval/evaluate.py --threshold``, ``scripts/plot_sweep.py``): T complete
runs.  Nothing in the upload, the resize or the UNet depends on the threshold, and contours, warp and classifier depend on it only
through the quadrangle.  So a job here is a job of ``batched._Call``, built from the steps that class shares (``begin_compute``,
``forward``, ``send_back``, ``warp_and_classify``, ``decode``, ``assemble``, the driver ``batched.run``); this module holds only what a
sweep does differently in the three stages:

* compute: the forward leaves no mask; ONE more kernel turns the logits, where they are, into a level map -- one byte per pixel,
  ``level = #{k: sigmoid(x) > t_k}`` over the ascending thresholds, so ``mask_k == (level > k)`` -- and a 320-byte record per image
  with every threshold's segmentation counts (``HipEngine.threshold_levels_dev``).  The level map travels back where the mask would,
  so the download stays 64 KB per image whatever T is.  With label masks the segmentation-score kernel runs once as well: its three
  float sums do not depend on the threshold.
* classify: the host expands the T masks per image, finds the T * n quadrangles in one native call and plans the boards
  (``evaluation.plan_threshold_groups``): group g holds every image's g-th DISTINCT quadrangle, at most one board per image, and is
  one ``Boards`` record of the job, as a job's ``found`` subset is in ``process_images``.
* finish: every threshold's result of an image points at the decoded board, crops, probabilities and scores of the quadrangle it
  found.

The job plan, the streams and the order of the stages (``_Call.issue``) are those of ``evaluate_images``, so the logits are its logits
bit for bit.
"""
from __future__ import annotations

import time

import numpy as np

from . import constants
from .batched import Job, _Call, _ImageSlot, plan_jobs, run
from .evaluation import SegmentationScores, ThresholdSweepReport, build_report, plan_threshold_groups
from .hip_backend import LEVEL_RECORD, SEG_RECORD, find_quadrangles, segmentation_scores_finish, threshold_levels_finish


class _SweepCall(_Call):
    """``_Call`` for T thresholds: per threshold a slot table and the two score lists of an ``EvaluationReport``.  Between classify
    and finish a job keeps ``job.sweep = (masks, use)``: the expanded (T,n,256,256) masks and ``use[k][position]``, the index of the
    ``Boards`` record of the job that holds the position's board at threshold k, or None."""

    def __init__(self, cv, images, thresholds, order, flip, fallback_quad, timings, started, targets, embeddings, resize):
        super().__init__(cv, images, float(thresholds[0]), flip, fallback_quad, True, timings, None, started, targets, embeddings, resize)
        self.thresholds, self.order = thresholds, order  # float32, ascending; order[j] = the ascending index of the caller's j-th
        T = len(thresholds)
        self.sweep_slots = [[None] * len(images) for _ in range(T)]
        self.sweep_segmentation = [[None] * len(images) for _ in range(T)]
        self.sweep_position = [[None] * len(images) for _ in range(T)]
        self.boards_found = self.boards_classified = 0

    def compute(self, job: Job) -> None:
        eng = self.eng
        self.begin_compute(job)
        lg, _, emb = self.forward(job.batch, want_mask=False)
        if job.labels is not None:
            job.labels.record_stream(self.main)
        levels, recs = self.gpu_timed("levels_ms", eng.threshold_levels_dev, lg, self.thresholds, job.labels)
        seg = None
        if job.labels is not None:                       # the threshold-independent sums (BCE, soft Dice): once per job
            seg = self.gpu_timed("seg_ms", eng.segmentation_scores_dev, lg, job.labels, self.threshold)
            job.labels = None
        self.send_back(job, levels.view(len(job.ids), 256, 256), lg, level=recs, seg=seg, emb=emb)

    def classify(self, job: Job) -> None:
        t0 = time.perf_counter()
        job.masks_ready.synchronize()
        self.clock("wait_masks_s", t0)
        ids, T = job.ids, len(self.thresholds)
        n = len(ids)
        t0 = time.perf_counter()
        levels = job.masks.numpy()
        masks = np.empty((T, n, 256, 256), dtype=np.uint8)
        for k in range(T):
            np.multiply(levels > k, np.uint8(255), out=masks[k], casting="unsafe")
        flat = find_quadrangles(masks.reshape(T * n, 256, 256), n_threads=self.n_host)
        self.clock("contours_s", t0)
        t0 = time.perf_counter()
        rows = []
        for k in range(T):
            row = flat[k * n:(k + 1) * n]
            if self.fallback_quad:
                row = [constants.WHOLE_MASK_QUADRANGLE if q is None else q for q in row]
            rows.append(row)
            self.boards_found += sum(q is not None for q in row)
        distinct, use, groups = plan_threshold_groups(rows)
        self.boards_classified += sum(len(d) for d in distinct)
        self.clock("homography_s", t0)
        job.sweep, job.cls_out = (masks, use), []
        for members in groups:
            job.boards.append(self.warp_and_classify(job, [p for p, _ in members], [q for _, q in members]))
        job.batch = None
        t0 = time.perf_counter()                         # the device has this job's classifiers queued: finish its mask scores meanwhile
        job.logits_ready.synchronize()
        if job.seg_records is not None:
            hard = threshold_levels_finish(job.level_records.numpy().view(LEVEL_RECORD).reshape(-1), labels_present=True)
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
        ids, (masks, use) = job.ids, job.sweep
        t0 = time.perf_counter()
        job.logits_ready.synchronize()
        lg = job.logits.numpy()
        ue = job.unet_emb.numpy() if job.unet_emb is not None else None
        for p, i in enumerate(ids):                      # one logits (and embedding) array per image, shared by its T results
            logits, emb = lg[p], (None if ue is None else ue[p])
            for k, slots in enumerate(self.sweep_slots):
                slots[i] = _ImageSlot(logits, masks[k, p], None, None, unet_emb=emb)
        for rec in job.boards:
            rec.probs_ready.synchronize()
        self.clock("wait_probs_s", t0)
        decoded = [dict(zip(rec.found, self.decode(job, rec))) for rec in job.boards]   # once per distinct board
        for k, slots in enumerate(self.sweep_slots):
            for p, i in enumerate(ids):
                if use[k][p] is not None:
                    slot = slots[i]
                    slot.quad, slot.board, slot.position, slot.cls_emb, self.sweep_position[k][i] = decoded[use[k][p]][p]

    def collect(self) -> ThresholdSweepReport:
        """One ``EvaluationReport`` per threshold, in the caller's order."""
        reports = [build_report(self.assemble(self.sweep_slots[k]), self.targets.labels, self.sweep_segmentation[k],
                                self.sweep_position[k]) for k in self.order]
        return ThresholdSweepReport.from_reports([float(self.thresholds[k]) for k in self.order], reports, self.boards_found,
                                                 self.boards_classified)


def evaluate_thresholds(cv, images, thresholds, order, targets, flip, fallback_quad, pipeline_chunk, timings, embeddings,
                        resize) -> ThresholdSweepReport:
    """``ChessVision.evaluate_thresholds`` on the instance's native engines.  ``thresholds``: float32, ascending (checked by the
    caller); ``order[j]``: the position in it of the caller's j-th threshold; ``targets``: the checked ground truth."""
    call = _SweepCall(cv, images, thresholds, order, flip, fallback_quad, timings, time.time(), targets, embeddings, resize)
    return run(call, plan_jobs([im.shape for im in images], pipeline_chunk, first=16, last=0))   # evaluate_images' plan: the same logits

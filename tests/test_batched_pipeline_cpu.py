"""Host logic of the batched pipeline (chessvision/batched.py) with no GPU: how a call is cut into jobs (``plan_jobs``) and the ORDER
in which upload, compute, classify and finish are issued across jobs (``_Call.issue``, its four stages replaced by recorders).  Both
decide how much of a call the device overlaps: the short first job hides the only upload nothing else covers, and an upload two jobs
ahead must wait for the end of the UNet issued just before it (profiles/r04_tuning.md step 12).  Also ``score_positions``, the
scoring step both ``process_images`` and the threshold sweep call, against the host form ``evaluation.position_scores``."""
from __future__ import annotations

import numpy as np
import pytest

from chessvision import batched, constants, evaluation, hip_backend, sweep
from chessvision.cv_types import pawn_rule_fix

A, B = (512, 512, 3), (384, 512, 3)


def _sizes(jobs):
    return [len(j) for j in jobs]


@pytest.mark.parametrize("n, chunk, first, last, sizes", [
    (256, 64, 16, 0, [16, 48, 64, 64, 64]),
    (96, 64, 16, 0, [16, 48, 32]),
    (64, 64, 16, 0, [64]),                                  # a single job is never split
    (40, 64, 16, 16, [40]),
    (256, 64, 16, 16, [16, 48, 64, 64, 48, 16]),
])
def test_planner_job_sizes(n, chunk, first, last, sizes):
    jobs = batched.plan_jobs([A] * n, chunk, first, last)
    assert _sizes(jobs) == sizes
    assert [i for job in jobs for i in job] == list(range(n))       # one shape: the caller's order, every index once


MIXED = [A, B, A, B, A, B, A, B, A, A, B]


@pytest.mark.parametrize("shapes, chunk, first, last, want", [
    ([A] * 6, 4, 16, 0, [[0, 1, 2, 3], [4, 5]]),
    ([A] * 5, 2, 0, 1, [[0, 1], [2, 3], [4]]),              # last job too short to split
    ([A] * 4, 2, 1, 1, [[0], [1], [2], [3]]),
    (MIXED, 3, 1, 1, [[0], [2, 4], [6, 8, 9], [1, 3, 5], [7], [10]]),
])
def test_planner_jobs(shapes, chunk, first, last, want):
    jobs = batched.plan_jobs(shapes, chunk, first, last)
    assert jobs == want
    assert sorted(i for job in jobs for i in job) == list(range(len(shapes)))      # every index exactly once
    for job in jobs:
        assert len({shapes[i] for i in job}) == 1                                  # one shape per job


class _Stages:
    """The four stages replaced: each notes its letter and job number and what the real stage leaves on the job."""

    def __init__(self):
        self.log, self.jobs = [], []

    def upload(self, ids, sliced=False, gate=None):
        job = batched.Job(ids, staged="pinned", batch="device photos")
        self.jobs.append(job)
        gated = "" if gate is None else f"g{gate[1]}"
        self.log.append(f"U{ids[0]}{'s' if sliced else ''}{gated}")
        return job

    def compute(self, job):
        assert job.unet_done is None
        job.unet_done, job.unet_out = ("unet done", job.ids[0]), ("logits", "masks", None)
        self.log.append(f"C{job.ids[0]}")

    def classify(self, job):
        assert job.unet_out is not None and job.cls_out is None
        job.cls_out, job.sweep = [("probabilities", "boards", "squares")], ("expanded masks", "board plan")
        self.log.append(f"K{job.ids[0]}")

    def finish(self, job):
        assert job.cls_out is not None
        self.log.append(f"F{job.ids[0]}")


class _Recorder(_Stages, batched._Call):
    pass


class _SweepRecorder(_Stages, sweep._SweepCall):
    """The threshold sweep inherits ``issue`` and ``upload``: the same order, whatever its three stages do."""


ORDERS = [
    (1, "U0s C0 K0 F0"),
    (2, "U0s C0 U1 C1 K0 K1 F0 F1"),
    (3, "U0s C0 U1 C1 U2g1 K0 C2 K1 F0 K2 F1 F2"),
    (4, "U0s C0 U1 C1 U2g1 K0 C2 U3g2 K1 F0 C3 K2 F1 K3 F2 F3"),
]


@pytest.mark.parametrize("n, want", ORDERS)
def test_issue_order(n, want):
    _check_issue_order(_Recorder(), n, want)


@pytest.mark.parametrize("n, want", ORDERS)
def test_issue_order_of_the_threshold_sweep(n, want):
    _check_issue_order(_SweepRecorder(), n, want)


def _check_issue_order(call, n, want):
    call.issue([[k] for k in range(n)])                     # job k holds image k: a stage's number is its job's
    assert " ".join(call.log) == want
    uploads = [(pos, e) for pos, e in enumerate(call.log) if e[0] == "U"]
    assert [e for _, e in uploads[:2]] == ["U0s", "U1"][:n]                        # U1 carries no gate
    for pos, e in uploads[2:]:
        k = int(e[1:].split("g")[0])
        assert e == f"U{k}g{k - 1}" and call.log[pos - 1] == f"C{k - 1}"           # gated on the compute issued just before it
    assert [j.ids for j in call.jobs] == [[k] for k in range(n)]
    for job in call.jobs:                                   # every finished job has dropped its device references
        assert job.batch is None and job.unet_out is None and job.cls_out is None and job.sweep is None


# ---- score_positions: a function of its inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
def test_score_positions_returns_the_host_form_and_touches_nothing(flip):
    """Two boards of random probabilities, the photos 5 and 2 of a call of six; only photo 5 has a true placement."""
    rng = np.random.default_rng(21 + flip)
    e = np.exp(rng.normal(0, 3, (2, 64, 13)))
    probs = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    true_fen = "r1bqkb1r/pppp1ppp/2n2n2/4p3/2B1P3/5N2/PPPP1PPP/RNBQK2R"
    targets = evaluation.Targets(6, true_fens=[None] * 5 + [true_fen])
    labels_before = [None if t is None else t.copy() for t in targets.labels]
    names = constants.SQUARE_NAMES_FLIPPED if flip else constants.SQUARE_NAMES_NORMAL
    fens, origs, validated, fixes = hip_backend.decode_positions(probs, flip)
    fix_lists = [[], []]
    for b, sq, old, new in fixes:
        fix_lists[b].append(pawn_rule_fix(names, sq, old, new))
    assert fix_lists[0]                                     # random rows put pawns on the end ranks: the rule had work to do
    ids, found = [4, 5, 2], [1, 2]                          # a job of three photos; the second and third have a board
    got = batched.score_positions(ids, found, probs, validated, fix_lists, targets.labels, flip)
    assert len(got) == 2 and got[1] is None                 # photo 2 has no true placement
    want = evaluation.position_scores(probs[0], fens[0], origs[0], true_fen, num_fixes=len(fix_lists[0]), flip=flip)
    a = got[0]
    assert (a.top_k, a.num_fixes, a.accuracy_original, a.accuracy_validated) == (want.top_k, want.num_fixes, want.accuracy_original,
                                                                                 want.accuracy_validated)
    for name in ("true_labels", "predicted_labels", "validated_labels", "rank"):
        assert np.array_equal(getattr(a, name), getattr(want, name)), name
    assert abs(a.mean_loss - want.mean_loss) <= 1e-12 * abs(want.mean_loss)
    assert batched.score_positions(ids, found, probs, validated, fix_lists, [None] * 6, flip) == [None, None]
    assert batched.score_positions(ids, [], probs[:0], validated[:0], [], targets.labels, flip) == []
    # the ground truth of the call is read, never written
    assert targets.position == [None] * 6 and targets.segmentation == [None] * 6
    assert all((b is None and t is None) or np.array_equal(b, t) for b, t in zip(labels_before, targets.labels))

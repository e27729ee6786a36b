"""Host logic of ``process_encoded`` (chessvision/encoded.py) with no GPU: the encoded call is ``batched._Call`` with another front --
``issue`` and the stages behind the reconstruction are inherited, so the ORDER of the stages is the one
tests/test_batched_pipeline_cpu.py pins -- and its jobs group by the streams' geometry."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from chessvision import batched, encoded, jpeg

GOLDEN = Path(__file__).resolve().parent / "golden"


class _Stages:
    """The four stages replaced by recorders, as in tests/test_batched_pipeline_cpu.py."""

    def __init__(self):
        self.log, self.jobs = [], []

    def upload(self, ids, sliced=False, gate=None):
        job = encoded.EncodedJob(ids, staged="pinned coefficients", coeffs="device coefficients")
        self.jobs.append(job)
        self.log.append(f"U{ids[0]}{'s' if sliced else ''}{'' if gate is None else f'g{gate[1]}'}")
        return job

    def compute(self, job):
        assert job.unet_done is None
        job.coeffs, job.batch = None, "reconstructed photos"            # what begin_compute leaves
        job.unet_done, job.unet_out = ("unet done", job.ids[0]), ("logits", "masks", None)
        self.log.append(f"C{job.ids[0]}")

    def classify(self, job):
        assert job.unet_out is not None and job.cls_out is None
        job.cls_out = [("probabilities", "boards", "squares")]
        self.log.append(f"K{job.ids[0]}")

    def finish(self, job):
        assert job.cls_out is not None
        self.log.append(f"F{job.ids[0]}")


class _Recorder(_Stages, encoded._EncodedCall):
    pass


@pytest.mark.parametrize("n, want", [
    (1, "U0s C0 K0 F0"),
    (2, "U0s C0 U1 C1 K0 K1 F0 F1"),
    (3, "U0s C0 U1 C1 U2g1 K0 C2 K1 F0 K2 F1 F2"),
    (4, "U0s C0 U1 C1 U2g1 K0 C2 U3g2 K1 F0 C3 K2 F1 K3 F2 F3"),
])
def test_issue_order_is_that_of_the_pixel_call(n, want):
    call = _Recorder()
    call.issue([[k] for k in range(n)])
    assert " ".join(call.log) == want
    for job in call.jobs:                                   # every finished job has dropped its device references
        assert job.batch is None and job.coeffs is None and job.unet_out is None and job.cls_out is None


def test_only_the_front_of_a_job_is_overridden():
    call, base = encoded._EncodedCall, batched._Call
    assert call.upload is not base.upload and call.begin_compute is not base.begin_compute
    for stage in ("issue", "compute", "forward", "send_back", "classify", "warp_and_classify", "finish", "decode", "assemble", "collect"):
        assert getattr(call, stage) is getattr(base, stage), stage


def test_jobs_group_by_geometry():
    z = np.load(GOLDEN / "jpeg_cases.npz")
    names = ["mixed_64x48_0", "gray_33x33_0", "420_33x33_0", "mixed_64x48_1", "gray_33x33_1", "444_33x33_0", "gray_33x33_2", "422_33x33_0",
             "420_33x33_1"]
    infos = jpeg.parse_all([z[f"blob/{n}"].tobytes() for n in names])
    keys = [f.geometry for f in infos]
    assert keys[0] == (64, 48, 3, 2, 2) and keys[1] == (33, 33, 1, 1, 1) and len(set(keys)) == 5     # same size, four samplings: four keys
    jobs = batched.plan_jobs(keys, 2, 0, 0)
    assert jobs == [[0, 3], [1, 4], [6], [2, 8], [5], [7]]
    for job in jobs:
        assert len({keys[i] for i in job}) == 1


def test_headers_are_parsed_first_and_every_refusal_is_listed():
    z = np.load(GOLDEN / "jpeg_cases.npz")
    blobs = [z[f"blob/{n}"].tobytes() for n in ("420_16x16_0", "progressive", "sampling_411", "gray_1x1_0", "truncated_in_marker_length")]
    with pytest.raises(jpeg.UnsupportedJpeg) as err:
        jpeg.parse_all(blobs)
    assert isinstance(err.value, ValueError) and sorted(err.value.reasons) == [1, 2, 4]
    assert "progressive" in err.value.reasons[1] and "sampling" in err.value.reasons[2] and "truncated" in err.value.reasons[4]
    assert "[1]" in str(err.value) and "[4]" in str(err.value)

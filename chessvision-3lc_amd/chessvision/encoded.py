"""``ChessVision.process_encoded``: the batched pipeline (chessvision/batched.py) fed with JPEG streams instead of decoded arrays.

Only the front of a job changes.  In ``upload`` the copy threads run the Huffman stage (``jpeg.entropy_decode``, one image per thread,
GIL released) straight into the page-locked staging buffer where ``process_images`` copies pixels, and the upload stream carries
quantised coefficients (3 bytes per pixel at 4:2:0, what the BGR upload weighs).  In ``begin_compute`` two launches on the compute
stream reconstruct the job's BGR photos into ``job.batch`` (``HipEngine.jpeg_reconstruct_dev``: libjpeg's pixels, byte for byte), and
from there on every stage is ``_Call``'s own: the resize reads ``job.batch``, the warp later reads full-resolution BGR from it.
``issue`` is inherited and still uses nothing but the four stages.

``orientation="exif"``: the reconstruction's second launch stores each photo as its EXIF orientation tag turns it
(``jpeg.apply_orientation``), so ``job.batch`` holds upright photos and nothing behind it knows.  A launch turns all its photos alike:
jobs are planned on (geometry, effective tag), and the stand-in images carry the oriented shape, which is the one the quadrangle
scaling and the warp must use.
"""
from __future__ import annotations

import time
from dataclasses import dataclass

import numpy as np
import torch

from . import jpeg
from .batched import Job, _Call, _pinned, plan_jobs, run


@dataclass(slots=True)
class EncodedJob(Job):
    """A job whose photos arrive as coefficients: ``staged`` is the pinned int16 buffer (all coefficients, then all tables),
    ``coeffs`` its copy on the device until ``begin_compute`` has queued the reconstruction behind it."""
    coeffs: torch.Tensor | None = None
    info: jpeg.JpegInfo | None = None
    tag: int = 0                                 # the EXIF orientation the reconstruction applies (0: none)


_ZERO = np.zeros((), np.uint8)


class _EncodedCall(_Call):
    def __init__(self, cv, blobs, infos, *args, orientation="ignore", **kw):
        # the stages ask the call's images for nothing but their shape: a zero-stride array per stream stands in for the pixels
        self.tags = [jpeg.effective_tag(f, orientation) for f in infos]
        super().__init__(cv, [np.broadcast_to(_ZERO, jpeg.oriented_shape(f, t) + (3,)) for f, t in zip(infos, self.tags)], *args, **kw)
        self.blobs, self.infos = blobs, infos
        self.tm.setdefault("entropy_s", 0.0)             # host seconds inside the Huffman stage (wall clock of the copy threads' maps)

    def upload(self, ids, sliced=False, gate=None) -> EncodedJob:
        """streams -> (Huffman stage on the copy threads) -> pinned coefficients -> device, on the upload stream; ``gate`` and
        ``sliced`` as in ``_Call.upload``."""
        t0 = time.perf_counter()
        up, n, info = self.up, len(ids), self.infos[ids[0]]
        count, tables = 64 * info.blocks, 64 * info.components
        job = EncodedJob(ids, staged=_pinned((n * (count + tables),), torch.int16), info=info, tag=self.tags[ids[0]])
        host = job.staged.numpy()
        co = host[:n * count].reshape(n, count)
        qt = host[n * count:].view(np.uint16).reshape(n, info.components, 64)
        with torch.cuda.stream(up):
            job.coeffs = torch.empty(n * (count + tables), dtype=torch.int16, device=self.dev)
            if gate is not None:
                up.wait_event(gate)
        blobs, infos = [self.blobs[i] for i in ids], [self.infos[i] for i in ids]
        step = 16 if sliced else n
        for k0 in range(0, n, step):
            k1 = min(n, k0 + step)
            t1 = time.perf_counter()
            jpeg.entropy_decode_many(blobs[k0:k1], infos[k0:k1], co[k0:k1], qt[k0:k1], pool=self.pool)
            self.clock("entropy_s", t1)
            with torch.cuda.stream(up):
                job.coeffs[k0 * count:k1 * count].copy_(job.staged[k0 * count:k1 * count], non_blocking=True)
        self.clock("stage_s", t0)
        with torch.cuda.stream(up):
            job.coeffs[n * count:].copy_(job.staged[n * count:], non_blocking=True)
            job.arrived = torch.cuda.Event()
            job.arrived.record()
        return job

    def begin_compute(self, job: EncodedJob) -> None:
        """The compute stream takes the coefficients over from the upload stream and reconstructs the job's photos."""
        self.main.wait_event(job.arrived)
        job.coeffs.record_stream(self.main)
        n, info = len(job.ids), job.info
        count = 64 * info.blocks
        turned = {"orientation": job.tag} if job.tag else {}                # named only when there is something to turn
        job.batch = self.gpu_timed("jpeg_ms", self.eng.jpeg_reconstruct_dev, job.coeffs[:n * count].view(n, count),
                                   job.coeffs[n * count:].view(n, info.components, 64), info, "bgr", **turned)
        job.coeffs = None
        self.tm.setdefault("first_enqueue_s", time.time() - self.started)


def process_encoded(cv, blobs, infos, threshold, flip, fallback_quad, pipeline_chunk, return_crops, timings, first_job, last_job,
                    quality, embeddings=False, resize="area", orientation="ignore", board_jpeg=None):
    """``ChessVision.process_encoded`` on the instance's native engines; ``infos`` are the parsed, supported headers of ``blobs``."""
    started = time.time()
    jpeg.check_orientation(orientation)
    if not blobs:
        return []
    call = _EncodedCall(cv, blobs, infos, threshold, flip, fallback_quad, return_crops, timings, quality, started, None, embeddings, resize, board_jpeg,
                        orientation=orientation)
    return run(call, plan_jobs([jpeg.job_key(f, orientation) for f in infos], pipeline_chunk, first=int(first_job), last=int(last_job)))

"""GPU: ``cv_pacmap_basis_scale``, ``cv_pacmap_place_pairs`` and ``cv_pacmap_place`` held to the header's stream contract with the
probe of tests/stream_probe.py, exactly as tests/test_gpu_pacmap_stream.py holds the fit's entries: everything a call issues (the
clears, the candidate search, the sigma and choose kernels; the placement's single launch) is ordered on the stream it was handed -- it
reads the inputs a copy EARLIER on that stream wrote, behind a delay -- and the call returns to the host while the delay is still
running.  The scratch is the caller's: one block per row of the table, never touched by the test.

True and decoy partner arrays of the placement both index inside the same basis of N rows, so whatever mixture of the two a misplaced
launch might read, every index it follows stays inside the buffers."""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import neighbour_cases as nc
import stream_probe as sp
from chessvision import embeddings as emb, hip_backend as hb

pytestmark = pytest.mark.gpu

I32, F32, F64 = torch.int32, torch.float32, torch.float64
N, C, NN, Q = 257, 33, 10, 130
ITERATIONS = 450


def _ok(status: int) -> None:
    assert status == 0, status


def _rng(true: bool, salt: int) -> np.random.Generator:
    return np.random.default_rng(salt + (1 if true else 2))


def _pre(true: bool, rows: int = N) -> np.ndarray:
    return emb.pacmap_preprocess(nc.make("c", rows, C, (1 if true else 2) + (0 if rows == N else 10)))


def _scale_row() -> sp.Row:
    name = "cv_pacmap_basis_scale-257x33"

    def make(true: bool) -> list:
        return [torch.from_numpy(_pre(true))]

    def outputs(ctx) -> list:
        return [((N,), F64)]

    def call(ctx, ins, outs, stream) -> None:
        _ok(ctx.lib.cv_pacmap_basis_scale(ctx.engine._h, ins[0].data_ptr(), N, C, NN, outs[0].data_ptr(), ctx.scratch[name].data_ptr(),
                                          ctx.scratch[name].numel(), stream))

    return sp.Row(name, make, outputs, call, reps=3)


def _pairs_row() -> sp.Row:
    name = "cv_pacmap_place_pairs-130-into-257x33"

    def make(true: bool) -> list:
        sigma = _rng(true, 100).uniform(0.5, 2.0, N)          # any positive scale: the entry only reads it
        return [torch.from_numpy(_pre(true, Q)), torch.from_numpy(_pre(true)), torch.from_numpy(sigma)]

    def outputs(ctx) -> list:
        return [((Q, NN), I32), ((8,), I32)]

    def call(ctx, ins, outs, stream) -> None:
        _ok(ctx.lib.cv_pacmap_place_pairs(ctx.engine._h, ins[0].data_ptr(), Q, ins[1].data_ptr(), N, C, NN, ins[2].data_ptr(),
                                          outs[0].data_ptr(), outs[1].data_ptr(), ctx.scratch[name].data_ptr(), ctx.scratch[name].numel(),
                                          stream))

    return sp.Row(name, make, outputs, call, reps=3)


def _place_row() -> sp.Row:
    name = "cv_pacmap_place-130-into-257"

    def make(true: bool) -> list:
        rng = _rng(true, 200)
        init = (0.01 * rng.standard_normal((Q, 2))).astype(np.float32)
        basis = (10.0 * rng.standard_normal((N, 2))).astype(np.float32)
        partners = rng.integers(0, N, (Q, NN)).astype(np.int32)
        assert partners.min() >= 0 and partners.max() < N
        return [torch.from_numpy(init), torch.from_numpy(basis), torch.from_numpy(partners)]

    def outputs(ctx) -> list:
        return [((Q, 2), F32)]

    def call(ctx, ins, outs, stream) -> None:
        _ok(ctx.lib.cv_pacmap_place(ctx.engine._h, ins[0].data_ptr(), Q, ins[1].data_ptr(), N, ins[2].data_ptr(), NN, ITERATIONS,
                                    outs[0].data_ptr(), stream))

    return sp.Row(name, make, outputs, call, reps=3)


ROWS = [_scale_row(), _pairs_row(), _place_row()]


@pytest.fixture(scope="module")
def ctx():
    engine = hb.HipEngine(precision="f32")
    lib = engine._lib
    plan = hb.PacmapPlacePlan()
    _ok(lib.cv_pacmap_place_plan(Q, N, C, NN, ctypes.byref(plan)))
    scratch = {ROWS[0].name: torch.empty(int(plan.scale_scratch_bytes), dtype=torch.uint8, device="cuda"),
               ROWS[1].name: torch.empty(int(plan.pairs_scratch_bytes), dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    yield SimpleNamespace(engine=engine, lib=lib, scratch=scratch)
    engine.close()


@pytest.fixture(scope="module")
def probe(ctx):
    p = sp.Probe()
    p.baselines = {row.name: p.baseline(ctx, row) for row in ROWS}
    p.choose_delay(p.baselines)
    assert p.pick_streams() and all(p.control_result.values()), p.control_log
    yield p


def test_control_sees_a_default_stream_kernel_read_the_decoy(probe):
    assert probe.control_result == {"read_decoy": True, "delay_outlasted_kernel": True, "copy_landed": True}


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_entry_is_ordered_on_its_stream_and_returns_before_the_stream_gets_there(ctx, probe, row):
    outcomes = probe.run(ctx, row, probe.baselines[row.name])
    print(f"{row.name}: default-stream call {probe.baselines[row.name].ms:.3f} ms; " +
          ", ".join(f"rep {o.rep}: {o.verdict}, returned {'early' if o.returned_early else 'LATE'}" for o in outcomes))
    for o in outcomes:
        assert o.verdict == "true", (
            f"{row.name}, call {o.rep} on the side stream: the outputs hold '{o.verdict}' where the default-stream result was expected "
            "('decoy': work ran before the stream's earlier copy; 'sentinel': the last kernel ran elsewhere)")
    late = [o.rep for o in outcomes[1:] if not o.returned_early]
    assert not late, f"{row.name}: calls {late} returned only after the {probe.delay_ms:.0f} ms delay in front of them had run out"

"""GPU: ``cv_pacmap_pairs`` and ``cv_pacmap_optimise`` held to the header's stream contract with the probe of tests/stream_probe.py,
exactly as tests/test_gpu_neighbours_stream.py holds the neighbour search: everything a call issues (the clears, the candidate search
and the four pair kernels; the two clears and one launch per iteration over both coordinate buffers) is ordered on the stream it was
handed -- it reads the inputs a copy EARLIER on that stream wrote, behind a delay -- and the call returns to the host while the delay
is still running.  The scratch is the caller's: one block per row of the table, never touched by the test.

True and decoy inputs of the optimiser are the incidence lists of two different pair sets over the same table shape: both have
2 N (n_neighbors + n_MN + n_FP) entries and offsets inside them, so whatever mixture of the two a misplaced launch might read, every
index it follows stays inside the buffers."""
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

I32, F32, U8 = torch.int32, torch.float32, torch.uint8
N, C, NN, NMN, NFP = 257, 33, 10, 5, 20
ITERATIONS = 60                              # both coordinate buffers many times over, all three weight phases' kernels alike


def _ok(status: int) -> None:
    assert status == 0, status


def _pre(true: bool) -> np.ndarray:
    return emb.pacmap_preprocess(nc.make("c", N, C, 1 if true else 2))


def _pairs_row() -> sp.Row:
    name = "cv_pacmap_pairs-257x33"

    def make(true: bool) -> list:
        return [torch.from_numpy(_pre(true))]

    def outputs(ctx) -> list:
        return [((N, NN), I32), ((N, NMN), I32), ((N, NFP), I32), ((64,), U8)]

    def call(ctx, ins, outs, stream) -> None:
        _ok(ctx.lib.cv_pacmap_pairs(ctx.engine._h, ins[0].data_ptr(), N, C, NN, NMN, NFP, 5, outs[0].data_ptr(), outs[1].data_ptr(),
                                    outs[2].data_ptr(), outs[3].data_ptr(), ctx.scratch[name].data_ptr(), ctx.scratch[name].numel(), stream))

    return sp.Row(name, make, outputs, call, reps=3)


def _optimise_row() -> sp.Row:
    name = "cv_pacmap_optimise-257x60"

    def make(true: bool) -> list:
        pre = _pre(true)
        pairs = emb.pacmap_pairs(pre, NN, NMN, NFP, seed=5)
        offsets, entries = emb.pacmap_incidence(pairs)
        assert entries.size == 2 * N * (NN + NMN + NFP) and offsets[-1] == entries.size
        return [torch.from_numpy(emb.pacmap_init(pre)), torch.from_numpy(offsets), torch.from_numpy(entries)]

    def outputs(ctx) -> list:
        return [((N, 2), F32)]

    def call(ctx, ins, outs, stream) -> None:
        _ok(ctx.lib.cv_pacmap_optimise(ctx.engine._h, ins[0].data_ptr(), N, ins[1].data_ptr(), ins[2].data_ptr(), ins[2].numel(), ITERATIONS,
                                       outs[0].data_ptr(), ctx.scratch[name].data_ptr(), ctx.scratch[name].numel(), stream))

    return sp.Row(name, make, outputs, call, reps=3)


ROWS = [_pairs_row(), _optimise_row()]


@pytest.fixture(scope="module")
def ctx():
    engine = hb.HipEngine(precision="f32")
    lib = engine._lib
    plan = hb.PacmapPlan()
    _ok(lib.cv_pacmap_plan(N, C, NN, NMN, NFP, ctypes.byref(plan)))
    scratch = {ROWS[0].name: torch.empty(int(plan.pairs_scratch_bytes), dtype=U8, device="cuda"),
               ROWS[1].name: torch.empty(int(plan.optimise_scratch_bytes), dtype=U8, device="cuda")}
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

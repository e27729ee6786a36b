"""GPU: ``cv_embedding_neighbours`` held to the header's stream contract with the probe of tests/stream_probe.py, exactly as each row of
tests/test_gpu_stream_contract.py is: everything the call issues (three clears, the prepare kernels, filter, refine, exact path) is
ordered on the stream it was handed -- it reads the tables a copy EARLIER on that stream wrote, behind a delay -- and the call returns
to the host while the delay is still running.  Two shapes: the graph of a table against itself through the filter, and a handful of
queries with every row on the exact path.  The scratch is the caller's: one block per row of the table, never touched by the test."""
from __future__ import annotations

from types import SimpleNamespace

import pytest
import torch

import neighbour_cases as nc
import stream_probe as sp
from chessvision import hip_backend as hb

pytestmark = pytest.mark.gpu

I32, F64, U8 = torch.int32, torch.float64, torch.uint8


def _ok(status: int) -> None:
    assert status == 0, status


def _row(name: str, q: int, n: int, c: int, k: int, flags: int) -> sp.Row:
    self_graph = q == 0
    rows = n if self_graph else q

    def make(true: bool) -> list:
        seed = 1 if true else 2
        corpus = torch.from_numpy(nc.make("c", n, c, seed))
        return [corpus] if self_graph else [torch.from_numpy(nc.make("c", q, c, seed + 10)), corpus]

    def outputs(ctx) -> list:
        return [((rows, k), I32), ((rows, k), F64), ((8,), I32)]

    def call(ctx, ins, outs, stream) -> None:
        queries, corpus = ins[0], ins[-1]
        _ok(ctx.lib.cv_embedding_neighbours(ctx.engine._h, queries.data_ptr(), rows, corpus.data_ptr(), n, c, k, flags, outs[0].data_ptr(),
                                            outs[1].data_ptr(), outs[2].data_ptr(), ctx.scratch[name].data_ptr(), ctx.scratch[name].numel(), stream))

    return sp.Row(name, make, outputs, call, reps=3)


ROWS = [_row("cv_embedding_neighbours-self257x512", 0, 257, 512, 10, hb.NEIGHBOURS_EXCLUDE_SELF),
        _row("cv_embedding_neighbours-4x257x33-exact", 4, 257, 33, 5, hb.NEIGHBOURS_EXACT_ONLY)]
SHAPES = {"cv_embedding_neighbours-self257x512": (257, 257, 512, 10), "cv_embedding_neighbours-4x257x33-exact": (4, 257, 33, 5)}


@pytest.fixture(scope="module")
def ctx():
    engine = hb.HipEngine(precision="f32")
    lib = engine._lib
    scratch = {name: torch.empty(int(lib.cv_embedding_neighbours_scratch_bytes(*shape)), dtype=U8, device="cuda") for name, shape in SHAPES.items()}
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

"""The probe of tests/test_gpu_stream_contract.py: does a device entry point do ALL its work on the stream it was handed, and does it
come back to the host without waiting for that stream?

Every other GPU test hands the library ``torch.cuda.current_stream()``, the legacy default stream, on which everything serialises
whatever the library does.  The probe is deterministic instead of hoping for a race.  One probe of ``call(ins, outs, stream)``:

1. on the default stream the call runs on the TRUE input and on a DECOY input of the same shape (``Probe.baseline``); the two results
   must differ, or a stale read would be invisible;
2. the input buffers are filled with the decoy and the output buffers with a sentinel byte, and the device is synchronised;
3. on a side stream: a delay kernel, an event, a device copy of the true input into the input buffers, the call, a clone of the
   outputs;
4. right after the call returns, ``returned_early = not event.query()``: the delay was still running, so the call did not wait;
5. after the side stream has drained, the clone must equal the true result byte for byte.  Work the library issued on any other
   stream ran while the delay held the side stream back and read the decoy; a last kernel issued elsewhere leaves the sentinel.

The delay is measured, not assumed: ``torch.cuda._sleep`` is calibrated with events, and its length is 20 x the longest probed call,
within [50, 500] ms.  ``Probe.control`` shows that the set-up can see anything at all: a plain torch kernel on the DEFAULT stream,
launched while the side stream holds its delay, must read the decoy.  The runtime multiplexes streams onto a few hardware queues and
two streams of one queue run in issue order, so in a process that has used many streams a given side stream may not pass it:
``Probe.pick_streams`` tries the module's three streams in turn and fails only when none does.

The second half of this file is host arithmetic: the facts about the resize tables that make the two-stream table cases of the GPU
module unable to read outside their buffers even against a library that swaps the tables under a running kernel."""
from __future__ import annotations

import dataclasses
from typing import Callable

import numpy as np
import torch

SENTINEL = 0xA5
DELAY_FACTOR, DELAY_MIN_MS, DELAY_MAX_MS = 20.0, 50.0, 500.0


# ---- the two-stream table cases: what a WRONG table could make a kernel read ---------------------------------------------------------
TABLE_PAIR = (42, 41)                    # square photo sides of the two geometries
TABLE_OUT = 16                           # both shrink to 16 x 16
TABLE_BATCH, TABLE_CHANNELS = 2, 3


def area_table_facts(src: int, dst: int) -> dict:
    """One axis of the INTER_AREA table as ``resize_area_table`` (csrc/pipeline.hip) lays it out: ``dst + 1`` offsets, then one source
    index and one weight per entry."""
    from chessvision import classical

    idx, _, cnt = classical._area_tab(src, dst)
    total = int(cnt.sum())
    return {"lengths": (dst + 1, total, total), "widest": int(cnt.max()), "max_index": int(max(idx[d, :cnt[d]].max() for d in range(dst)))}


def antialias_table_facts(src: int, dst: int) -> dict:
    """One axis of the antialias tap table as ``resize_antialias_table`` lays it out: ``dst`` firsts, ``dst`` counts, ``dst`` rows of
    ``stride`` weights."""
    from chessvision import classical

    first, count, weights = classical.antialias_taps(src, dst)
    return {"lengths": (len(first), len(count), int(weights.size)), "widest": int(weights.shape[1]), "max_index": int((first + count - 1).max())}


def backing_bytes(n: int = TABLE_BATCH, c: int = TABLE_CHANNELS, pair=TABLE_PAIR) -> int:
    """Both geometries' batches are carved from allocations of this size: n images of the LARGER geometry."""
    return n * max(pair) * max(pair) * c


def assert_table_swap_cannot_leave_the_buffers(facts: Callable[[int, int], dict], pair=TABLE_PAIR, dst: int = TABLE_OUT,
                                               n: int = TABLE_BATCH, c: int = TABLE_CHANNELS) -> None:
    """The gate in front of the first launch of a two-stream table case.  A library that refills the cached table block while a
    launch of the other geometry still reads it must give wrong pixels, never an access outside a buffer:
    (1) the three arrays of both tables have the same lengths, so the block layout (every array 16-byte aligned in one block) is the
        same and an index INTO a table that is valid for one geometry is valid for the other;
    (2) the widest row is the same (the antialias kernel's weight stride; the area kernel's entry count per pixel);
    (3) every source index of either table lies inside an image of the larger geometry;
    and the batches are carved from ``backing_bytes``: the farthest byte the smaller geometry's launch can reach through the larger
    geometry's table -- last image, row and column at that table's largest index, last channel -- is inside the allocation."""
    a, b = (facts(side, dst) for side in pair)
    assert a["lengths"] == b["lengths"], (a, b)
    assert a["widest"] == b["widest"], (a, b)
    big, small = max(pair), min(pair)
    worst = max(a["max_index"], b["max_index"])
    assert worst < big, (a, b)
    farthest = (((n - 1) * small + worst) * small + worst) * c + c - 1
    assert farthest < backing_bytes(n, c, pair), (farthest, backing_bytes(n, c, pair))


# ---- the probe ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Row:
    """One entry point at one shape.  ``make(true)`` -> the true / decoy inputs as CPU tensors; ``outputs(ctx)`` -> [(shape, dtype)];
    ``call(ctx, ins, outs, stream_ptr)`` issues the entry on device tensors and raises on a status other than 0."""
    name: str
    make: Callable[[bool], list]
    outputs: Callable[[object], list]
    call: Callable[[object, list, list, int], None]
    reps: int = 2                         # probes on the same buffers; host asynchrony is asserted from the second on
    asynchronous: bool = True             # False only where include/chessvision_hip.h says the entry synchronises
    canon: Callable[[list], object] | None = None          # CPU outputs -> what is compared (default: every byte of every output)
    prepare: Callable[[object, list], None] | None = None  # default-stream work in front of a probe (decoy inputs on the device)


@dataclasses.dataclass
class Baseline:
    ins_true: list
    ins_decoy: list
    y_true: object
    y_decoy: object
    ms: float                             # the decoy run on the default stream, between two events


@dataclasses.dataclass
class Outcome:
    rep: int
    returned_early: bool
    verdict: str                          # "true" | "decoy" | "sentinel" | "other: ..."


def fill_sentinel(t: torch.Tensor) -> None:
    t.view(torch.uint8).fill_(SENTINEL)


def raw(t: torch.Tensor) -> bytes:
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def every_byte(outs_cpu: list) -> tuple:
    return tuple(raw(t) for t in outs_cpu)


def first_difference(got: bytes, want: bytes):
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if a.size != b.size:
        return f"{a.size} bytes for {b.size}"
    at = int(np.flatnonzero(a != b)[0])
    return f"byte {at}: {int(a[at])} for {int(b[at])} ({int((a != b).sum())} of {a.size} differ)"


class Probe:
    def __init__(self):
        # every stream this module opens.  Which hardware queue a stream shares with which other is the runtime's choice (it has fewer
        # queues than a long process has streams, and work of two streams on one queue runs in issue order): pick_streams() finds, with
        # the control, a candidate the default stream does not queue behind.
        self.candidates = [torch.cuda.Stream() for _ in range(3)]
        self.side = self.candidates[0]
        self.s2 = self.candidates[1]
        self.s2_independent = False
        self.cycles_per_ms = self._calibrate()
        self.delay_ms: float | None = None
        self.longest: tuple[str, float] | None = None
        self.control_result: dict = {}
        self.control_log: list = []

    def _calibrate(self) -> float:
        """``torch.cuda._sleep`` counts device clock ticks of a rate this file does not assume: time it, growing the count until the
        kernel lasts long enough for the event timer to mean something."""
        cycles = 1_000_000
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = self.candidates[0]
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)                         # first use: the kernel's load is not part of the figure
            for _ in range(8):
                e0.record(stream)
                torch.cuda._sleep(cycles)
                e1.record(stream)
                stream.synchronize()
                ms = e0.elapsed_time(e1)
                if ms >= 5.0:
                    return cycles / ms
                cycles *= 8
        raise AssertionError(f"torch.cuda._sleep({cycles // 8}) lasted {ms:.3f} ms: the delay kernel cannot be calibrated on this runtime")

    def sleep_ms(self, ms: float) -> None:
        torch.cuda._sleep(int(ms * self.cycles_per_ms))

    def choose_delay(self, baselines: dict) -> float:
        name, ms = max(((k, b.ms) for k, b in baselines.items()), key=lambda kv: kv[1])
        self.longest = (name, ms)
        self.delay_ms = min(DELAY_MAX_MS, max(DELAY_MIN_MS, DELAY_FACTOR * ms))
        return self.delay_ms

    # -- step 1 ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _alloc(specs) -> list:
        outs = [torch.empty(shape, dtype=dtype, device="cuda") for shape, dtype in specs]
        for o in outs:
            fill_sentinel(o)
        return outs

    def baseline(self, ctx, row: Row) -> Baseline:
        stream = torch.cuda.current_stream()
        assert stream.cuda_stream == 0, "the baseline belongs on the legacy default stream"
        canon = row.canon or every_byte
        ins_true, ins_decoy = ([t.contiguous().cuda() for t in row.make(flag)] for flag in (True, False))
        outs_true, outs_decoy = self._alloc(row.outputs(ctx)), self._alloc(row.outputs(ctx))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        row.call(ctx, ins_true, outs_true, 0)                 # also warms whatever the shape allocates at first use
        torch.cuda.synchronize()
        e0.record()
        row.call(ctx, ins_decoy, outs_decoy, 0)               # last: the engine's workspace is left holding the decoy
        e1.record()
        torch.cuda.synchronize()
        y_true, y_decoy = canon([o.cpu() for o in outs_true]), canon([o.cpu() for o in outs_decoy])
        assert y_true != y_decoy, f"{row.name}: true and decoy inputs give the same result, a stale read would be invisible"
        return Baseline(ins_true, ins_decoy, y_true, y_decoy, e0.elapsed_time(e1))

    # -- steps 2 to 5 ------------------------------------------------------------------------------------------------------------
    def run(self, ctx, row: Row, base: Baseline) -> list:
        assert self.delay_ms is not None
        canon = row.canon or every_byte
        ins = [torch.empty_like(t) for t in base.ins_true]
        outs = self._alloc(row.outputs(ctx))
        untouched = canon([o.cpu() for o in outs])
        outcomes = []
        for rep in range(row.reps):
            for buf, decoy in zip(ins, base.ins_decoy):
                buf.copy_(decoy)
            for o in outs:
                fill_sentinel(o)
            if row.prepare:
                row.prepare(ctx, base.ins_decoy)
            torch.cuda.synchronize()
            after_delay = torch.cuda.Event()
            with torch.cuda.stream(self.side):
                self.sleep_ms(self.delay_ms)
                after_delay.record(self.side)
                for buf, true in zip(ins, base.ins_true):
                    buf.copy_(true, non_blocking=True)
                row.call(ctx, ins, outs, self.side.cuda_stream)
                returned_early = not after_delay.query()
                clones = [o.clone() for o in outs]
            self.side.synchronize()
            got = canon([c.cpu() for c in clones])
            if got == base.y_true:
                verdict = "true"
            elif got == base.y_decoy:
                verdict = "decoy"
            elif got == untouched:
                verdict = "sentinel"
            else:
                which = next(k for k, (g, w) in enumerate(zip(got, base.y_true)) if g != w) if isinstance(got, tuple) else 0
                detail = first_difference(got[which], base.y_true[which]) if isinstance(got, tuple) and isinstance(got[which], bytes) else ""
                verdict = f"other: output {which} {detail}"
            outcomes.append(Outcome(rep, returned_early, verdict))
        return outcomes

    # -- the control -------------------------------------------------------------------------------------------------------------
    def control(self, holder=None, runner=None) -> dict:
        """A plain torch kernel on ``runner`` (None: the DEFAULT stream) while ``holder`` holds the delay in front of the copy: it must
        read the decoy, the delay must still be running when it has finished, and the copy must land afterwards."""
        assert self.delay_ms is not None
        holder = holder or self.side
        true = torch.arange(4096, dtype=torch.int32, device="cuda")
        decoy = true + 7
        buf = decoy.clone()
        torch.cuda.synchronize()
        after_delay = torch.cuda.Event()
        with torch.cuda.stream(holder):
            self.sleep_ms(self.delay_ms)
            after_delay.record(holder)
            buf.copy_(true, non_blocking=True)
        if runner is None:
            seen = buf + 0
            torch.cuda.current_stream().synchronize()
        else:
            with torch.cuda.stream(runner):
                seen = buf + 0
            runner.synchronize()
        held = not after_delay.query()
        holder.synchronize()
        torch.cuda.synchronize()
        return {"read_decoy": bool(torch.equal(seen, decoy)), "delay_outlasted_kernel": held, "copy_landed": bool(torch.equal(buf, true))}

    def pick_streams(self) -> bool:
        """``side``: the first candidate behind whose delay a default-stream kernel does NOT wait (the control of the module; False when
        there is none: the probe would see nothing).  ``s2``: another candidate, if there is one whose kernels do not wait behind
        ``side`` either -- the two-stream cases assert results only, so a second stream that shares ``side``'s queue weakens a case to
        device order but cannot make it fail."""
        for cand in self.candidates:
            result = self.control(cand)
            self.control_log.append(("default stream while candidate %d holds" % self.candidates.index(cand), result))
            if all(result.values()):
                self.side, self.control_result = cand, result
                break
        else:
            self.control_result = self.control_log[-1][1]
            return False
        others = [c for c in self.candidates if c is not self.side]
        self.s2 = others[0]
        for cand in others:
            result = self.control(self.side, cand)
            self.control_log.append(("candidate %d while side holds" % self.candidates.index(cand), result))
            if all(result.values()):
                self.s2, self.s2_independent = cand, True
                break
        return True
